"""GPU: the multi-layer LSTM decoder of the attention models (csrc/dec_stack.hip; decoder_num_layers > 1) -- the one-launch
dx + cell backward kernel and its generic twin against float64 autograd, the beam re-ordering against a numpy gather, the
native loops against the step-by-step statement (tests/_cpu_ops_att_stack.py), the models against the float64 statement of
the whole loss and of both decodes (tests/_att_stack_oracle.py), isolation of the one-layer path and repeatability.

Bars.  Kernel level: 1e-5 of the array's largest entry (the GRU cell's kernel test: fp32 operands, exact products, only the
summation order differs from float64).  Loop level: the GRU loop test's (forward 2e-5, backward 5e-5 of the array's largest
entry, floor 1e-2).  Model level, fp32: the plain models' (loss 1e-4 relative, logits 1e-4, gradients 2e-3 of the gradient's
largest entry, one momentum step 1e-5); bf16 operands: loss 2e-3, logits 3e-2, gradients 3e-2 of the gradient's largest
entry, against the statement with bf16-rounded encoder operands.  A decoded id is compared with the statement's where the
statement's top-two margin exceeds 10 x the logits bar; at most 10 % of positions may fall under it.

Shapes are tiny (Em = 8, A = 16, C = 6, T <= 12, To <= 6).  Kernel and loop tests: E2 = U = 16 runs the one-launch backward,
and 2U = 32 input columns keep the upper layers' forward on the product + cell pair (one case has U = 32: the image); one
loop case takes the smallest shape of tests/test_gpu_attention.py at which the fused attention step runs (E2 = 256, A = 64,
U = 48).  Model tests: H = 64, the narrowest encoder the device recurrence takes (asr_lstm_prep_layer refuses H % 64 != 0, so
the H = 8 of the kernel-level shapes cannot be a model's), hence E2 = U = 128; a batch's upper layers then run the image
forward, a beam's R = 36 rows the product + cell pair."""
import numpy as np
import pytest
import torch

import _att_stack_oracle as so
import _cpu_ops_att_stack as cs

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32
NAN = float('nan')
D_ = 'attention_decoder/decoder/'


def _ops():
    from tensorflow_end2end_speech_recognition_amd import ops
    return ops


def _rel(got, want, floor=1e-6):
    w = want.double().cpu().numpy()
    return float(np.abs(got.double().cpu().numpy() - w).max() / max(np.abs(w).max(), floor))


# ------------------------------------------------------------------------------------------- the backward kernel and its twin
_BWD_SHAPES = [(U, B, True) for U in (32, 96) for B in (3, 16, 17, 32)] + [(24, 3, False), (32, 33, False)]


@pytest.mark.parametrize('extras', [False, True])
@pytest.mark.parametrize('U,B,fused_shape', _BWD_SHAPES)
def test_lower_layer_backward_against_float64(cuda, U, B, fused_shape, extras):
    """asr_att_stack_bwd_step, fused form and generic twin, against float64 autograd of one stacked step
    (_att_stack_oracle.lower_step_f64): dpre, the carried dc / dh, d_hin and the peephole rows; with and without output mask,
    peepholes and a second carried-dh addend (a column block of a wider array).  live is mixed 0 / 1.  Every output is NaN
    before the call.  The counters say which form ran: the fused one exactly where B <= 32 and U % 16 == 0."""
    ops = _ops()
    rng = np.random.RandomState(U + B + int(extras))
    f = lambda *s, sc=1.0: torch.tensor(rng.randn(*s) * sc, dtype=F32, device=cuda)            # noqa: E731
    assert bool(ops.att_stack_bwd_ok(B, U)) == fused_shape
    dpre_up, W_up = f(B, 4 * U, sc=0.3), f(2 * U, 4 * U, sc=0.1)
    c_prev, h_prev, pre = f(B, U, sc=0.5), f(B, U, sc=0.5), f(B, 4 * U, sc=0.7)
    peep = f(3, U, sc=0.3) if extras else None
    mask = torch.tensor((rng.rand(B, U) < 0.8) / 0.8, dtype=F32, device=cuda) if extras else None
    live = torch.tensor((rng.rand(B) < 0.6).astype(np.float32), device=cuda)
    live[0], live[1] = 1.0, 0.0
    dc_next, dh_next, dh_2 = f(B, U, sc=0.3), f(B, U, sc=0.3), f(B, U, sc=0.3)
    wide = torch.full((B, U + 5), NAN, device=cuda)
    wide[:, :U] = dh_2
    cpu = lambda t: None if t is None else t.cpu()                                                # noqa: E731
    want = so.lower_step_f64(cpu(dpre_up), cpu(W_up), cpu(c_prev), cpu(h_prev), cpu(pre), cpu(peep), cpu(live), cpu(mask),
                             cpu(dc_next), cpu(dh_next + dh_2 if extras else dh_next))
    gates, c_raw = want['gates'].float().to(cuda), want['c_raw'].float().to(cuda)
    for fused in ([True, False] if fused_shape else [False]):
        ops.reset_att_stack_counts(0)
        dpre, dc_prev, carry, d_hin, dpeep = ops.att_stack_bwd_step(
            dpre_up, W_up, dc_next, dh_next, gates, c_raw, c_prev, live, peep=peep, use_mask=mask,
            dh_next2=wide[:, :U] if extras else None, fused=fused)
        assert ops.att_stack_counts(0) == dict(fwd_image=0, fwd_two_launch=0, bwd_fused=int(fused), bwd_generic=int(not fused))
        for name, g in (('dpre', dpre), ('dc_prev', dc_prev), ('dh_prev_carry', carry), ('d_hin', d_hin), ('dpeep', dpeep)):
            if g is None:
                assert want[name] is None
                continue
            assert not torch.isnan(g).any(), name
            e = _rel(g, want[name])
            print('stack bwd U=%d B=%d fused=%d extras=%d %s %.3g' % (U, B, fused, extras, name, e))
            assert e < 1e-5, (name, e)
        dead = (live == 0).cpu()
        assert float(dpre.cpu()[dead].abs().max()) == 0.0                       # a finished row: no parameter gradient
    assert ops.check_async_errors(0) == 0


def test_stack_reorder_is_a_gather(cuda):
    """asr_att_stack_reorder against a numpy gather, exact: L = 3 (two upper layers), W = 4, parents that repeat and that
    skip, block 0 NaN before the call; the columns [0,U) of `in` block 0 and all of block 1 are not written."""
    ops = _ops()
    rng = np.random.RandomState(0)
    B, W, U = 3, 4, 24
    R = B * W
    parent = torch.tensor([[0, 0, 2, 2], [3, 1, 1, 1], [2, 3, 0, 1]], dtype=I32, device=cuda)
    mk = lambda w: torch.tensor(rng.randn(2, R, w), dtype=F32, device=cuda)                      # noqa: E731
    c, h, x = [mk(U), mk(U)], [mk(U), mk(U)], [mk(2 * U), mk(2 * U)]
    for t in c + h:
        t[0] = NAN
    for t in x:
        t[0, :, U:] = NAN
    before = [t.clone() for t in c + h + x]
    ops.att_stack_reorder(parent, c, h, x)
    rows = (np.arange(B)[:, None] * W + parent.cpu().numpy()).reshape(-1)
    for t, b in zip(c + h, before[:4]):
        assert np.array_equal(t[0].cpu().numpy(), b[1].cpu().numpy()[rows]) and torch.equal(t[1], b[1])
    for t, b in zip(x, before[4:]):
        assert np.array_equal(t[0, :, U:].cpu().numpy(), b[1, :, U:].cpu().numpy()[rows])
        assert torch.equal(t[0, :, :U], b[0, :, :U]) and torch.equal(t[1], b[1])
    assert ops.check_async_errors(0) == 0


# ------------------------------------------------------------------------------------------------------------ native loops
# three rows whose labels are 2, 4 and 6 long: live for 1, 3 and 5 of the To = 5 steps (one row finishes at step 1)
_LOOP_CASES = {'location_carry': dict(A=16, hasq=1, mode=0, carry=1, U=16, E2=16, T=11),
               'luong_dot': dict(A=16, hasq=0, mode=1, carry=0, U=16, E2=16, T=11),
               # 2U = 64 input columns: the upper layers' forward step is ONE launch on the interleaved image
               'luong_dot_U32': dict(A=32, hasq=0, mode=1, carry=0, U=32, E2=32, T=11),
               # tests/test_gpu_attention.py's A64: the smallest shape with the fused attention step and the fused query-FC
               # + cell backward (here: of the TOP layer); T = 70 is two frame chunks
               'fused_attention': dict(A=64, hasq=1, mode=0, carry=0, U=48, E2=256, T=70, nokeys=True)}


def _loop_arrays(case, layers, seed=0):
    c = _LOOP_CASES[case]
    rng = np.random.RandomState(seed + len(case) + layers)
    B, To, Em = 3, 5, 8
    T, U, E2, A = c['T'], c['U'], c['E2'], c['A']
    Din = Em + E2 + U
    f = lambda *s, sc=1.0: torch.tensor(rng.randn(*s) * sc, dtype=F32)                        # noqa: E731
    drop = lambda *s: torch.tensor((rng.rand(*s) < 0.8) / 0.8, dtype=F32)                      # noqa: E731
    seq_len = torch.tensor([T, 7, 4], dtype=I32)
    enc = f(T, B, E2, sc=0.5) * (torch.arange(T).view(T, 1, 1) < seq_len.view(1, B, 1))
    live = torch.tensor((np.arange(To)[:, None] < (np.array([2, 4, 6]) - 1)[None, :]).astype(np.float32))
    taps = 201 if c['carry'] else 0
    nokeys = c['carry'] or c.get('nokeys')
    a = dict(To=To, B=B, T=T, U=U, Em=Em, E2=E2, A=A, att_mode=c['mode'], has_query_fc=c['hasq'], carry_alpha=c['carry'],
             taps=taps, enc_dtype=0, forget_bias=1.0, cell_clip=50.0, sharpening=1.5,
             W_cell=f(Din, 4 * U, sc=0.1), b_cell=f(4 * U, sc=0.1), peep=f(3, U, sc=0.2),
             W_q=f(U, A, sc=0.1) if c['hasq'] else None, b_q=f(A, sc=0.1) if c['carry'] else None,
             v=f(A, sc=0.5) if c['mode'] == 0 else None,
             keys=None if nokeys else (enc.clone() if case.startswith('luong_dot') else f(T, B, A, sc=0.5)), enc=enc,
             seq_len=seq_len, filt=f(taps, 1, 10, sc=0.3) if c['carry'] else None,
             wfil=f(10, A, sc=0.3) if c['carry'] else None, alpha_zero=torch.zeros(B, T) if c['carry'] else None,
             live=live, dmask=drop(To, B, U), dec_in=f(To, B, Din, sc=0.5), av_in=torch.full((To, B, U + E2), NAN),
             alpha_all=torch.full((To, B, T), NAN), gates_all=torch.full((To, B, 4 * U), NAN),
             craw_all=torch.full((To, B, U), NAN), c_all=torch.full((To + 1, B, U), NAN),
             h_all=torch.full((To + 1, B, U), NAN), qz_all=torch.full((To, B, A), NAN))
    a['c_all'][0], a['h_all'][0] = f(B, U, sc=0.3), f(B, U, sc=0.3)
    a['dec_in'][0, :, Em:Em + E2] = 0.0
    a['dec_in'][0, :, Em + E2:] = a['h_all'][0]
    a['dec_in'][1:, :, Em:] = NAN                              # the loop's to write
    ups = []
    for _ in range(1, layers):
        u = {'W': f(2 * U, 4 * U, sc=0.1), 'b': f(4 * U, sc=0.1), 'peep': f(3, U, sc=0.2), 'dmask': drop(To, B, U),
             'in': torch.full((To, B, 2 * U), NAN), 'c': torch.full((To + 1, B, U), NAN), 'h': torch.full((To + 1, B, U), NAN),
             'gates': torch.full((To, B, 4 * U), NAN), 'craw': torch.full((To, B, U), NAN)}
        u['c'][0], u['h'][0] = f(B, U, sc=0.3), f(B, U, sc=0.3)
        u['in'][0, :, U:] = u['h'][0]
        ups.append(u)
    a['stack'] = dict(layers=ups)
    bwd_in = dict(dav_cell=f(To, B, U, sc=0.3), dav_ctx=f(To, B, E2, sc=0.3))
    has_keys = a['keys'] is not None
    bwd_out = dict(dctx_all=(To, B, E2), dpre_all=(To, B, 4 * U), dqz_all=(To, B, A), dpeep_all=(To, B, 3 * U),
                   dv_all=(To, B, A) if c['mode'] == 0 else None, d_in_all=(To, B, Din),
                   dkeys=(T, B, A) if has_keys else None, dwfil_rows=(B, 10, A) if c['carry'] else None,
                   dfilt_rows=(B, taps, 10) if c['carry'] else None, dc0=(B, U), dh0=(B, U))
    up_out = dict(dpre=(To, B, 4 * U), d_hin=(To, B, U), dpeep=(To, B, 3 * U), dc0=(B, U), dh0=(B, U))
    return a, bwd_in, bwd_out, up_out


def _loop_clone(a, bwd_in, bwd_out, up_out, dev):
    mv = lambda v: v.clone().to(dev) if torch.is_tensor(v) else v                              # noqa: E731
    d = {k: mv(v) for k, v in a.items() if k != 'stack'}
    d['stack'] = dict(layers=[dict({n: mv(t) for n, t in u.items()},
                                   **{n: torch.zeros(s, device=dev) for n, s in up_out.items()})
                              for u in a['stack']['layers']])
    d.update({k: v.clone().to(dev) for k, v in bwd_in.items()})
    d.update({k: (torch.zeros(s, device=dev) if s is not None else None) for k, s in bwd_out.items()})
    return d


_LOOP_FWD = ('alpha_all', 'av_in', 'dec_in', 'c_all', 'h_all', 'qz_all', 'gates_all', 'craw_all')
_UP_FWD = ('in', 'c', 'h', 'gates', 'craw')


@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('case,layers', [('location_carry', 2), ('location_carry', 3), ('luong_dot', 2), ('luong_dot', 3),
                                         ('luong_dot_U32', 3), ('fused_attention', 2)])
def test_native_loops_against_the_step_by_step_statement(cuda, case, layers, fused):
    """asr_att_decoder_fwd_stack / _bwd_stack (all To steps from one call, dropout on every layer, peepholes, cell clip)
    against the float64 step-by-step statement of the same loops: every forward array of every layer (NaN before the call
    wherever the loop writes) and every backward array; the counters say which form ran at every step."""
    ops = _ops()
    a, bwd_in, bwd_out, up_out = _loop_arrays(case, layers)
    ref, got = _loop_clone(a, bwd_in, bwd_out, up_out, 'cpu'), _loop_clone(a, bwd_in, bwd_out, up_out, cuda)
    got['stack']['fused'] = fused
    To, nup = a['To'], layers - 1
    cs._att_decoder_fwd(ref)
    ops.reset_att_stack_counts(0)
    ops.reset_att_path_counts(0)
    ops.att_decoder_fwd(got)
    # 2U = 32 / 96 input columns are no multiple of 64: the product + cell pair; 2U = 64: the image
    img = (2 * a['U']) % 64 == 0
    fwd_counts = dict(fwd_image=To * nup if img else 0, fwd_two_launch=0 if img else To * nup)
    assert ops.att_stack_counts(0) == dict(fwd_counts, bwd_fused=0, bwd_generic=0)
    paths = {k: v for k, v in ops.att_path_counts(0).items() if v}
    assert paths.get('fwd_step_fused', 0) == (To if case == 'fused_attention' else 0), paths
    rel = lambda x, y: float(np.abs(x.cpu().double().numpy() - y.double().numpy()).max() /      # noqa: E731
                             max(np.abs(y.double().numpy()).max(), 1e-2))
    pairs = [(n, got[n], ref[n]) for n in _LOOP_FWD]
    for i in range(nup):
        pairs += [('up%d.%s' % (i + 1, n), got['stack']['layers'][i][n], ref['stack']['layers'][i][n]) for n in _UP_FWD]
    for name, g, r in pairs:
        assert not torch.isnan(g).any(), name
        err = rel(g, r)
        print('stack loop %s L=%d fwd %s %.3g' % (case, layers, name, err))
        assert err < 2e-5, (name, err)
    for name, g, r in pairs:                                 # the backward of both sides starts from the SAME saved forward
        g.copy_(r.to(cuda))
    cs._att_decoder_bwd(ref)
    ops.att_decoder_bwd(got)
    assert ops.att_stack_counts(0) == dict(fwd_counts, bwd_fused=To * nup if fused else 0,
                                           bwd_generic=0 if fused else To * nup)
    paths = {k: v for k, v in ops.att_path_counts(0).items() if v}
    assert paths.get('bwd_step_fused_q', 0) == (To if case == 'fused_attention' else 0), paths
    pairs = [(n, got[n], ref[n]) for n, s in bwd_out.items() if s is not None]
    for i in range(nup):
        pairs += [('up%d.%s' % (i + 1, n), got['stack']['layers'][i][n], ref['stack']['layers'][i][n]) for n in up_out]
    for name, g, r in pairs:
        err = rel(g, r)
        print('stack loop %s L=%d fused=%d bwd %s %.3g' % (case, layers, fused, name, err))
        assert err < 5e-5, (name, err)
    assert ops.check_async_errors(0) == 0


# ------------------------------------------------------------------------------------------------------------- model level
def _batch(rng, B, T, Din, C, lens):
    x = rng.randn(B, T, Din).astype(np.float32)
    sl = rng.randint(max(2, T // 2), T + 1, size=B).astype(np.int32)
    sl[0] = T
    lens = np.asarray(lens)
    labels = np.full((B, int(lens.max()) + 2), C + 1, dtype=np.int64)
    ctc = np.full((B, int(lens.max())), -1, dtype=np.int64)
    for b in range(B):
        x[b, sl[b]:] = 0
        y = rng.randint(0, C, size=lens[b])
        labels[b, 0] = C
        labels[b, 1:1 + lens[b]] = y
        ctc[b, :lens[b]] = y
    return x, sl, labels, lens + 2, ctc


_DIN, _H, _U, _A, _EM, _C = 12, 64, 128, 16, 8, 6


def _mk(cls, att, layers, dtype='f32', seed=5, device='cuda:0', **kw):
    kw.setdefault('max_decode_length', 8)
    return cls(input_size=_DIN, encoder_type='blstm', encoder_num_units=_H, encoder_num_layers=1, encoder_num_proj=None,
               attention_type=att, attention_dim=_A, decoder_type='lstm', decoder_num_units=_U, decoder_num_layers=layers,
               embedding_dim=_EM, num_classes=_C, sos_index=_C, eos_index=_C + 1, parameter_init=0.1, clip_grad_norm=5.0,
               clip_activation_encoder=50, clip_activation_decoder=50, dtype=dtype, seed=seed, device=device, **kw)


def _classes():
    from tensorflow_end2end_speech_recognition_amd.models.attention.attention_seq2seq import AttentionSeq2Seq
    from tensorflow_end2end_speech_recognition_amd.models.attention.joint_ctc_attention import JointCTCAttention
    return AttentionSeq2Seq, JointCTCAttention


_PARITY = {'location': ('location', 'zeros', False, 'f32', 2), 'luong_dot': ('luong_dot', 'zeros', False, 'f32', 2),
           'location_bf16': ('location', 'zeros', False, 'bf16', 2), 'joint': ('bahdanau_content', 'zeros', True, 'f32', 2),
           'location_carry_L3': ('location', 'carry', False, 'f32', 3)}


@pytest.mark.parametrize('case', sorted(_PARITY))
def test_model_parity(cuda, monkeypatch, case):
    """AttentionSeq2Seq / JointCTCAttention with a two- (one case: three-) layer decoder, decoder and embedding keep
    probability 0.8: loss, logits and every gradient against the float64 statement fed the device's own masks of every
    layer, at the bars of the module docstring, and the parameters after one momentum step (learning rate 1e-3) within 1e-5
    of the step the statement's gradients give.  Label lengths 1 / 5 / 3 / 5 / 2: rows finish at step 1 and at the last
    step.  The upper layers ran the one-launch backward (counted).

    Measured on the MI355X: fp32 loss 2e-8 .. 1e-7 relative, logits 1e-7 .. 2e-7, gradients 7e-7; bf16 loss 7e-7, logits 4e-5,
    gradients 4e-3 (the figures are printed)."""
    import _cpu_ops_att_ss as ss
    from oracle import lstm as olstm
    from tensorflow_end2end_speech_recognition_amd.utils.io.labels.sparsetensor import list2sparsetensor
    ops = _ops()
    att, prev, joint, dtype, layers = _PARITY[case]
    Att, Joint = _classes()
    B, T, C = 5, 12, _C
    x, sl, labels, lsl, ctc = _batch(np.random.RandomState(11), B, T, _DIN, C, [1, 5, 3, 5, 2])
    kw = dict(sharpening_factor=1.5, logits_temperature=2.0, prev_alpha=prev, dtype=dtype, device=cuda)
    model = _mk(Joint, att, layers, lambda_weight=0.5, honour_ctor_args=True, **kw) if joint else _mk(Att, att, layers, **kw)
    masks = ss.spy_dropout_masks(monkeypatch, ops)
    ops.reset_att_stack_counts(0)
    if joint:
        loss, logits, _, otr, _ = model.compute_loss(x, labels, list2sparsetensor(ctc, -1), sl, lsl, 1.0, 0.8, 0.8)
    else:
        loss, logits, otr, _ = model.compute_loss(x, labels, sl, lsl, 1.0, 0.8, 0.8)
    To, nup = int(lsl.max()) - 1, layers - 1
    assert ops.att_stack_counts(0) == dict(fwd_image=To * nup, fwd_two_launch=0, bwd_fused=0, bwd_generic=0)
    demb = [m for m in masks if m[2] == model.seed + 1][0][4][:, :B].transpose(0, 1).cpu().numpy()
    d0 = [m for m in masks if m[2] == model.seed + 2 and len(m[0]) == 3][0][4]
    dup = [m for m in masks if m[2] == model.seed + 2 and len(m[0]) == 4][0][4]
    ddec = torch.cat([d0.unsqueeze(0), dup], 0)[:, :, :B].cpu().numpy()
    sd0 = {k: v.clone() for k, v in model.store.state_dict().items()}
    sd = {k: v.cpu().numpy() for k, v in sd0.items()}
    ref = so.stack_model_forward(sd, x, labels, sl, lsl, 1, att, clip_enc=50.0, clip_dec=50.0, sharpening=1.5,
                                 temperature=2.0, drop_emb=demb, drop_dec=ddec, prev_alpha=prev,
                                 ctc_labels=[[int(v) for v in r if v >= 0] for r in ctc] if joint else None,
                                 lambda_weight=0.5 if joint else None,
                                 operand_round=olstm.bf16_round_t if dtype == 'bf16' else None)
    loss_rel = abs(loss.item() - ref['total_loss']) / abs(ref['total_loss'])
    logits_abs = float(np.abs(logits.cpu().numpy() - ref['logits'] * 2.0).max())
    opt = model._set_optimizer('momentum', 1e-3)
    gv = opt.compute_gradients(loss, model=model)
    assert ops.att_stack_counts(0) == dict(fwd_image=To * nup, fwd_two_launch=0, bwd_fused=To * nup, bwd_generic=0)
    worst, worst_name = 0.0, None
    for g, name in gv:
        r = ref['grads'][name]
        e = float(np.abs(g.cpu().numpy() - r).max() / max(np.abs(r).max(), 1e-3))
        if e > worst:
            worst, worst_name = e, name
    print('stack model %s: loss rel %.2e  logits abs %.2e  grad worst %.2e %s' % (case, loss_rel, logits_abs, worst, worst_name))
    names = {n for _, n in gv}
    for l in range(1, layers):
        for v in ('kernel', 'bias', 'w_i_diag', 'w_f_diag', 'w_o_diag'):
            n = D_ + 'lstm_cell_%d/%s' % (l, v)
            assert n in names and np.abs(ref['grads'][n]).max() > 0, n
    bars = dict(loss=1e-4, logits=1e-4, grad=2e-3) if dtype == 'f32' else dict(loss=2e-3, logits=3e-2, grad=3e-2)
    assert loss_rel < bars['loss'] and logits_abs < bars['logits'], (loss_rel, logits_abs)
    for g, name in gv:
        r = ref['grads'][name]
        err = np.abs(g.cpu().numpy() - r).max()
        assert err < bars['grad'] * max(np.abs(r).max(), 1e-3) + 1e-7, (name, err, np.abs(r).max())
    if dtype == 'f32':
        # one momentum step: p - lr * clip_by_norm(g, 5) from the statement's gradients
        grads64 = {name: ref['grads'][name] for _, name in gv}
        opt.apply_gradients(model._clip_gradients(gv))
        after = model.store.state_dict()
        for name, g in grads64.items():
            nrm = float(np.sqrt((g ** 2).sum()))
            want = sd[name].astype(np.float64) - 1e-3 * g * (5.0 / max(nrm, 5.0))
            err = float(np.abs(after[name].cpu().numpy() - want).max())
            assert err < 1e-5, (name, err)
    assert ops.check_async_errors(0) == 0


# Seeds (model and batch) found on the CPU with the float64 statement alone -- see each test's docstring for the counted
# share of positions under the margin.
_GREEDY_SEEDS = {'location_carry': 1, 'luong_dot': 1}
_BEAM_SEED = 2


def _decode_case(att, prev, seed, B, device, layers=2, max_decode_length=8):
    Att, _ = _classes()
    rng = np.random.RandomState(seed)
    T, C = 12, _C
    sl = rng.randint(T // 2, T + 1, size=B).astype(np.int32)
    sl[0] = T
    x = (rng.randn(B, T, _DIN) * (np.arange(T)[None, :, None] < sl[:, None, None])).astype(np.float32)
    model = _mk(Att, att, layers, seed=seed, sharpening_factor=1.5, prev_alpha=prev, device=device,
                max_decode_length=max_decode_length)
    sd = {k: v.clone() for k, v in model.store.state_dict().items()}
    sd[D_ + 'output_layer/weights'] *= 40.0            # (a head as sharp as a trained one: see tests/test_gpu_att_beam.py)
    sd[D_ + 'output_layer/biases'][C + 1] = 0.35
    model.store.load_state_dict(sd)
    return model, x, sl, C, {k: v.cpu().numpy() for k, v in sd.items()}


@pytest.mark.parametrize('att,prev', [('location', 'carry'), ('luong_dot', 'zeros')])
def test_greedy_decode_against_the_statement(cuda, att, prev):
    """infer() == the statement's greedy decode wherever its top-two margin exceeds 10 x the logits bar (1e-3), the class
    surface (AttentionDecoder.step over StackedLSTMDecoderCell) agrees, and _decode_beam(beam_width=1) == infer().  The
    float64 statement alone leaves at most 10 % of the live positions under the margin (asserted): seeds 1 / 1 have 0 of 33
    (location, carry; smallest margin 3.2e-3) and 0 of 29 (luong_dot; 8.5e-3) under it, counted on the CPU."""
    from tensorflow_end2end_speech_recognition_amd.models.attention.decoders.beam_search.beam_search_decoder import cut_at_eos
    ops = _ops()
    seed = _GREEDY_SEEDS[att + '_carry' if prev == 'carry' else att]
    model, x, sl, C, sd = _decode_case(att, prev, seed, 5, cuda)
    ids, margin, lmax = so.stack_model_infer(sd, x, sl, 1, att, C, C + 1, 8, clip_enc=50.0, clip_dec=50.0, sharpening=1.5,
                                             prev_alpha=prev)
    livepos = np.isfinite(margin)
    under = livepos & ~(margin > 10 * 1e-4)
    print('stack greedy %s: %d live positions, %d under the margin, largest |logit| %.2f' % (att, livepos.sum(), under.sum(), lmax))
    assert under.sum() <= 0.1 * livepos.sum()
    ops.reset_att_stack_counts(0)
    got = model.infer(x, sl)
    c = ops.att_stack_counts(0)
    assert c['fwd_image'] >= got.shape[1] and c['fwd_two_launch'] == 0
    n = min(got.shape[1], ids.shape[1])
    if under.any():
        n = min(n, int(np.where(under.any(0))[0].min()))     # ids behind a position under the margin may follow another path
    else:
        assert got.shape == ids.shape
    assert np.array_equal(got[:, :n], ids[:, :n])
    surf = model.infer(x, sl, native=False)
    assert np.array_equal(surf[:, :n], ids[:, :n])
    beam = model._decode_beam(ops.to_device(x, F32, model.device), ops.to_device(sl, I32, model.device), 1)
    if not under.any():
        for b in range(len(sl)):
            assert cut_at_eos(beam[b], C + 1) == cut_at_eos(got[b], C + 1), b
    assert np.array_equal(model.infer(x, sl, beam_width=1), got)
    assert ops.check_async_errors(0) == 0


def test_beam_search_against_the_host_statement(cuda):
    """infer(beam_width=4, length_penalty_weight=0.6) at 9 utterances (R = 36 rows) equals BeamSearchDecoder driven by the
    float64 stacked step: every hypothesis of every utterance whose margin (smallest gap among the top W + 1 candidate
    scores) is above 10 x the logits bar, ids exactly and scores to 1e-3.  The float64 statement alone leaves at most one
    utterance in ten -- i.e. none of nine -- under the margin (seed 2, chosen on the CPU: smallest margin 4.0e-3; asserted)."""
    ops = _ops()
    model, x, sl, C, sd = _decode_case('bahdanau_content', 'zeros', _BEAM_SEED, 9, cuda)
    want = so.stack_beam_infer(sd, x, sl, 1, 'bahdanau_content', C, C + 1, 8, 4, 0.6, clip_enc=50.0, clip_dec=50.0,
                               sharpening=1.5)
    skipped = [b for b, r in enumerate(want) if not r['margin'] > 10 * 1e-4]
    print('stack beam: margins %s' % ['%.3g' % r['margin'] for r in want])
    assert len(skipped) <= 0.1 * len(want), [r['margin'] for r in want]
    ops.reset_att_stack_counts(0)
    best = model.infer(x, sl, beam_width=4, length_penalty_weight=0.6)
    raw = model._beam_raw
    assert ops.att_stack_counts(0) == dict(fwd_image=0, fwd_two_launch=raw['steps_issued'], bwd_fused=0, bwd_generic=0)
    for b, r in enumerate(want):
        if b in skipped:
            continue
        for w in range(4):
            n = int(raw['hyp_len'][b, w])
            assert raw['ids'][b, w, :n].tolist() == r['ids'][w], (b, w)
            assert not raw['ids'][b, w, n:].any()
        assert np.abs(raw['scores'][b] - r['scores']).max() < 1e-3
        assert best[b, :len(r['ids'][0])].tolist() == r['ids'][0]
    assert ops.check_async_errors(0) == 0


# ------------------------------------------------------------------------------------------ isolation and repeatability
def _step(model, x, labels, sl, lsl):
    loss, logits, _, _ = model.compute_loss(x, labels, sl, lsl, 0.9, 0.8, 0.8)
    gv = model._set_optimizer('adam', 1e-3).compute_gradients(loss, model=model)
    return loss.item(), logits.clone(), [g.clone() for g, _ in gv]


def test_one_layer_decoder_is_untouched_by_a_stack_in_the_process(cuda):
    """A one-layer LSTM-decoder model built and stepped before and after a two-layer model in the same process: loss, logits
    and every gradient bit for bit, greedy and beam decodes equal, and none of the stack entry points called -- the counters
    stay zero through a training step, a greedy decode and a beam decode."""
    ops = _ops()
    Att, _ = _classes()
    x, sl, labels, lsl, _ = _batch(np.random.RandomState(3), 5, 12, _DIN, _C, [1, 5, 3, 5, 2])
    zero = dict(fwd_image=0, fwd_two_launch=0, bwd_fused=0, bwd_generic=0)
    runs = []
    for k in range(2):
        ops.reset_att_stack_counts(0)
        one = _mk(Att, 'location', 1, prev_alpha='carry', device=cuda)
        runs.append(_step(one, x, labels, sl, lsl) + (one.infer(x, sl), one.infer(x, sl, beam_width=3)))
        assert ops.att_stack_counts(0) == zero
        if k == 0:
            two = _mk(Att, 'location', 2, prev_alpha='carry', device=cuda)
            _step(two, x, labels, sl, lsl)
            two.infer(x, sl)
            two.infer(x, sl, beam_width=3)
            c = ops.att_stack_counts(0)
            assert c['fwd_image'] > 0 and c['bwd_fused'] > 0
    a, b = runs
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and all(torch.equal(p, q) for p, q in zip(a[2], b[2]))
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
    assert ops.check_async_errors(0) == 0


def test_seeded_two_layer_step_is_repeatable(cuda):
    """Two fresh two-layer models with the same seed: a training step (encoder, decoder and embedding dropout on) gives the
    same loss, logits and updated parameters bit for bit."""
    Att, _ = _classes()
    x, sl, labels, lsl, _ = _batch(np.random.RandomState(4), 5, 12, _DIN, _C, [1, 5, 3, 5, 2])
    runs = []
    for _ in range(2):
        model = _mk(Att, 'bahdanau_content', 2, device=cuda)
        loss, logits, _, _ = model.compute_loss(x, labels, sl, lsl, 0.9, 0.8, 0.8)
        model.train(loss, 'adam', 1e-3)
        loss2, *_ = model.compute_loss(x, labels, sl, lsl, 0.9, 0.8, 0.8)
        runs.append((loss.item(), logits.clone(), model.store.flat.clone(), loss2.item()))
    a, b = runs
    assert a[0] == b[0] and a[3] == b[3] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
