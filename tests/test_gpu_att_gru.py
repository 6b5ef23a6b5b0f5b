"""GPU: the GRU decoder of the attention models (csrc/gru_decoder.hip; decoder_type='gru') -- the cell kernels of both
paths against float64, the native loops against the step-by-step statement (tests/_cpu_ops_att_gru.py), the models against
the float64 statement of the whole loss and of both decodes (tests/_att_gru_oracle.py), isolation from the LSTM decoder and
repeatability.

Bars.  Cell level: 1e-5 of the array's largest entry (test_gpu_attention's cell-product tests: fp32 operands, exact
products, only the summation order differs from float64).  Loop level: test_native_decoder_loop_against_the_step_by_step_
statement's (forward 2e-5, backward 5e-5 of the array's largest entry, floor 1e-2).  Model level, fp32: those of
test_attention_model_parity (loss 1e-4 relative, logits 2e-4, gradients 2e-3 of the gradient's largest entry); bf16
operands: those test_gpu_sched_sampling quotes (loss 3e-2, logits 3e-2 x max(1, largest logit), gradients 4e-2 matrices /
8e-2 peepholes / 4e-2 relative L2).  A decoded id is compared with the statement's where the statement's top-two margin
exceeds 10 x the logits bar (the project's margin convention); at most 10 % of positions may fall under it."""
import numpy as np
import pytest
import torch

import _att_gru_oracle as go
import _cpu_ops_att_gru as cg

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32
NAN = float('nan')
D_ = 'attention_decoder/decoder/'


def _ops():
    from tensorflow_end2end_speech_recognition_amd import ops
    return ops


def _rel(got, want):
    w = want.double().cpu().numpy()
    return float(np.abs(got.double().cpu().numpy() - w).max() / max(np.abs(w).max(), 1e-6))


# ------------------------------------------------------------------------------------------------------------ cell kernels
_FUSED = [(1, 64, 16), (5, 192, 64), (17, 640, 128), (32, 1600, 512)]
_GENERAL = [(35, 375, 300), (3, 35, 12)]


@pytest.mark.parametrize('mask', [False, True])
@pytest.mark.parametrize('B,Din,U,fused', [s + (True,) for s in _FUSED] + [s + (False,) for s in _GENERAL] +
                         [(5, 192, 64, False)])
def test_cell_kernels_against_float64(cuda, B, Din, U, fused, mask):
    """asr_gru_cell_gemm_fwd (two launches) / asr_gru_cell_fwd_ex (four) and asr_gru_cell_bwd against float64 autograd of
    oracle.gru's cell: gates r | u | c | r*h, the state (live mixed 0 / 1: finished rows carry h), the cell output with and
    without a dropout mask, the pre-activation gradients, the cell-input gradient and the carried dh.  x is a row block
    of a wider, longer array whose other entries are NaN, every output is NaN before the call, and the scatter targets
    (attentional-vector columns, the next input's h columns, the query rows) equal the primary outputs bit for bit.
    Reference: attention_seq2seq.py:364-365 (tf.contrib.rnn.GRUCell)."""
    ops = _ops()
    rng = np.random.RandomState(B + Din + U + int(mask))
    f = lambda *s, sc=1.0: torch.tensor(rng.randn(*s) * sc, dtype=F32, device=cuda)            # noqa: E731
    assert bool(ops.gru_cell_gemm_ok(B, Din, U)) == ((B, Din, U) in _FUSED)
    wide = torch.full((B + 2, Din + 8), NAN, device=cuda)
    hp = f(B, U, sc=0.5)
    wide[:B, :Din - U] = f(B, Din - U, sc=0.5)
    wide[:B, Din - U:Din] = hp
    x = wide[:B, :Din]
    Wg, bg, Wc, bc = f(Din, 2 * U, sc=0.06), 1.0 + f(2 * U, sc=0.2), f(Din, U, sc=0.06), f(U, sc=0.2)
    live = torch.tensor((rng.rand(B) < 0.6).astype(np.float32), device=cuda)
    live[0] = 1.0
    if B > 1:
        live[1] = 0.0
    om = torch.tensor((rng.rand(B, U) < 0.8) / 0.8, dtype=F32, device=cuda) if mask else None
    dcell, dh_c, dh_2 = f(B, U, sc=0.3), f(B, U, sc=0.3), f(B, U, sc=0.3)
    W3 = ops.gru_cell_prep(Wg, bg, Wc, bc)
    assert torch.equal(W3[:Din, :2 * U], Wg) and torch.equal(W3[:Din - U, 2 * U:], Wc[:Din - U])
    assert float(W3[Din - U:Din, 2 * U:].abs().max()) == 0.0
    assert torch.equal(W3[Din, :2 * U], bg) and torch.equal(W3[Din, 2 * U:], bc)
    nan = lambda *s: torch.full(s, NAN, device=cuda)                                           # noqa: E731
    gates, h_out, av, nxt, qz = nan(B, 4 * U), nan(B, U), nan(B, U + 24), nan(B, Din), nan(B, U)
    ops.reset_att_gru_counts(0)
    ops.gru_cell_fwd(x, W3, Wc, hp, live, out_mask=om, fused=fused, h_also=nxt[:, Din - U:], cell_out_also=qz,
                     out=(gates, h_out, av[:, :U]))
    assert ops.att_gru_counts(0) == dict(fwd_fused=int(fused), fwd_general=int(not fused), bwd=0)
    want = go.cell_step_f64(x.cpu(), hp.cpu(), Wg.cpu(), bg.cpu(), Wc.cpu(), bc.cpu(), live.cpu(),
                            om.cpu() if mask else None, dcell.cpu(), (dh_c + dh_2).cpu())
    cell_out = av[:, :U]
    for name, g in (('gates', gates), ('h_out', h_out), ('cell_out', cell_out)):
        assert not torch.isnan(g).any(), name
        e = _rel(g, want[name])
        print('gru cell B=%d Din=%d U=%d fused=%d mask=%d fwd %s %.3g' % (B, Din, U, fused, mask, name, e))
        assert e < 1e-5, (name, e)
    assert torch.equal(nxt[:, Din - U:], h_out) and torch.equal(qz, cell_out)
    assert torch.isnan(nxt[:, :Din - U]).all() and torch.isnan(av[:, U:]).all()                # nothing else was written
    dead = live.cpu() == 0
    assert torch.equal(h_out.cpu()[dead], hp.cpu()[dead]) and (h_out.cpu()[~dead] != hp.cpu()[~dead]).any()
    # backward, from the float64 forward's saved activations (so the comparison is per kernel)
    g64 = want['gates'].float().to(cuda)
    wide2 = nan(B, U + 5)
    wide2[:, :U] = dh_2
    dpre, carry, d_in = ops.gru_cell_bwd(dcell, dh_c, g64, hp, W3, Wc, live, out_mask=om, dh_c2=wide2[:, :U])
    assert ops.att_gru_counts(0)['bwd'] == 1
    for name, g in (('dpre', dpre), ('d_in', d_in), ('dh_carry', carry)):
        assert not torch.isnan(g).any(), name
        e = _rel(g, want[name])
        print('gru cell B=%d Din=%d U=%d bwd %s %.3g' % (B, Din, U, name, e))
        assert e < 1e-5, (name, e)
    assert ops.check_async_errors(0) == 0


# ------------------------------------------------------------------------------------------------------------ native loops
# the narrowest shape of tests/test_gpu_sched_sampling.py: U = 2H = 64, A = 36, T = 11, three rows whose labels are 2, 4 and
# 6 long, i.e. live for 1, 3 and 5 of the To = 5 steps; Em = 64 makes the cell input 192 wide (the two-launch form)
_B, _T, _TO, _U, _E2, _EM = 3, 11, 5, 64, 64, 64
_LOOP_CASES = {'additive_q': dict(A=36, hasq=1, mode=0, carry=0), 'location_carry': dict(A=36, hasq=1, mode=0, carry=1),
               'luong_dot': dict(A=64, hasq=0, mode=1, carry=0)}


def _loop_arrays(case, seed=0):
    c = _LOOP_CASES[case]
    rng = np.random.RandomState(seed + len(case))
    B, T, To, U, E2, Em, A = _B, _T, _TO, _U, _E2, _EM, c['A']
    Din = Em + E2 + U
    f = lambda *s, sc=1.0: torch.tensor(rng.randn(*s) * sc, dtype=F32)                        # noqa: E731
    seq_len = torch.tensor([T, 7, 4], dtype=I32)
    enc = f(T, B, E2, sc=0.5) * (torch.arange(T).view(T, 1, 1) < seq_len.view(1, B, 1))
    live = torch.tensor((np.arange(To)[:, None] < (np.array([2, 4, 6]) - 1)[None, :]).astype(np.float32))
    taps = 201 if c['carry'] else 0
    a = dict(To=To, B=B, T=T, U=U, Em=Em, E2=E2, A=A, att_mode=c['mode'], has_query_fc=c['hasq'], carry_alpha=c['carry'],
             taps=taps, enc_dtype=0, forget_bias=1.0, cell_clip=0.0, sharpening=1.5,
             gru=dict(W_g=f(Din, 2 * U, sc=0.08), b_g=1.0 + f(2 * U, sc=0.1), W_c=f(Din, U, sc=0.08), b_c=f(U, sc=0.1)),
             W_q=f(U, A, sc=0.1) if c['hasq'] else None, b_q=f(A, sc=0.1) if c['carry'] else None,
             v=f(A, sc=0.5) if c['mode'] == 0 else None,
             keys=None if c['carry'] else (enc.clone() if case == 'luong_dot' else f(T, B, A, sc=0.5)), enc=enc,
             seq_len=seq_len, filt=f(taps, 1, 10, sc=0.3) if c['carry'] else None,
             wfil=f(10, A, sc=0.3) if c['carry'] else None, alpha_zero=torch.zeros(B, T) if c['carry'] else None,
             live=live, dmask=torch.tensor((rng.rand(To, B, U) < 0.8) / 0.8, dtype=F32),
             dec_in=f(To, B, Din, sc=0.5), av_in=torch.full((To, B, U + E2), NAN), alpha_all=torch.full((To, B, T), NAN),
             gates_all=torch.full((To, B, 4 * U), NAN), h_all=torch.full((To + 1, B, U), NAN),
             qz_all=torch.full((To, B, A), NAN))
    a['h_all'][0] = f(B, U, sc=0.3)
    a['dec_in'][0, :, Em:Em + E2] = 0.0
    a['dec_in'][0, :, Em + E2:] = a['h_all'][0]
    a['dec_in'][1:, :, Em:] = NAN                              # the loop's to write
    bwd_in = dict(dav_cell=f(To, B, U, sc=0.3), dav_ctx=f(To, B, E2, sc=0.3))
    has_keys = a['keys'] is not None
    bwd_out = dict(dctx_all=(To, B, E2), dpre_all=(To, B, 3 * U), dqz_all=(To, B, A),
                   dv_all=(To, B, A) if c['mode'] == 0 else None, d_in_all=(To, B, Din),
                   dkeys=(T, B, A) if has_keys else None, dwfil_rows=(B, 10, A) if c['carry'] else None,
                   dfilt_rows=(B, taps, 10) if c['carry'] else None, dh0=(B, U))
    return a, bwd_in, bwd_out


def _loop_clone(a, bwd_in, bwd_out, dev):
    mv = lambda v: v.clone().to(dev) if torch.is_tensor(v) else v                              # noqa: E731
    d = {k: ({n: mv(t) for n, t in v.items()} if k == 'gru' else mv(v)) for k, v in a.items()}
    d.update({k: v.clone().to(dev) for k, v in bwd_in.items()})
    d.update({k: (torch.zeros(s, device=dev) if s is not None else None) for k, s in bwd_out.items()})
    return d


_LOOP_FWD = ('alpha_all', 'av_in', 'dec_in', 'h_all', 'qz_all', 'gates_all')


@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('case', sorted(_LOOP_CASES))
def test_native_loops_against_the_step_by_step_statement(cuda, case, fused):
    """asr_att_decoder_fwd_gru / _bwd_gru (all To steps from one call, dropout on) against the float64 step-by-step
    statement of the same loops: every forward array (NaN before the call wherever the loop writes) and every backward
    array; the counters say which form of the cell ran at every step."""
    ops = _ops()
    a, bwd_in, bwd_out = _loop_arrays(case)
    ref, got = _loop_clone(a, bwd_in, bwd_out, 'cpu'), _loop_clone(a, bwd_in, bwd_out, cuda)
    got['gru']['fused'] = fused
    cg._att_decoder_fwd(ref)
    ops.reset_att_gru_counts(0)
    ops.att_decoder_fwd(got)
    assert ops.att_gru_counts(0) == dict(fwd_fused=_TO if fused else 0, fwd_general=0 if fused else _TO, bwd=0)
    rel = lambda x, y: float(np.abs(x.cpu().double().numpy() - y.double().numpy()).max() /      # noqa: E731
                             max(np.abs(y.double().numpy()).max(), 1e-2))
    for name in _LOOP_FWD:
        assert not torch.isnan(got[name]).any(), name
        err = rel(got[name], ref[name])
        print('gru loop %s fused=%d fwd %s %.3g' % (case, fused, name, err))
        assert err < 2e-5, (name, err)
    for name in _LOOP_FWD:                                   # the backward of both sides starts from the SAME saved forward
        got[name].copy_(ref[name].to(cuda))
    cg._att_decoder_bwd(ref)
    ops.att_decoder_bwd(got)
    assert ops.att_gru_counts(0)['bwd'] == _TO
    for name, shape in bwd_out.items():
        if shape is not None:
            err = rel(got[name], ref[name])
            print('gru loop %s bwd %s %.3g' % (case, name, err))
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


def _mk(cls, att, dtype='f32', seed=5, decoder_type='gru', device='cuda:0', **kw):
    # Em = 64: the cell input is 64 + 128 + 128 = 320 wide, so B <= 32 rows run the two-launch form
    Din, H, L, U, A, Em, C = 12, 64, 1, 128, 32, 64, 9
    kw.setdefault('max_decode_length', 12)
    return cls(input_size=Din, encoder_type='blstm', encoder_num_units=H, encoder_num_layers=L, encoder_num_proj=None,
               attention_type=att, attention_dim=A, decoder_type=decoder_type, decoder_num_units=U, decoder_num_layers=1,
               embedding_dim=Em, num_classes=C, sos_index=C, eos_index=C + 1, parameter_init=0.1, clip_grad_norm=5.0,
               clip_activation_encoder=50, clip_activation_decoder=50, dtype=dtype, seed=seed, device=device, **kw)


def _classes():
    from tensorflow_end2end_speech_recognition_amd.models.attention.attention_seq2seq import AttentionSeq2Seq
    from tensorflow_end2end_speech_recognition_amd.models.attention.joint_ctc_attention import JointCTCAttention
    return AttentionSeq2Seq, JointCTCAttention


_PARITY = {'location_zeros': ('location', 'zeros', False, 'f32'), 'location_carry': ('location', 'carry', False, 'f32'),
           'bahdanau': ('bahdanau_content', 'zeros', False, 'f32'), 'luong_dot': ('luong_dot', 'zeros', False, 'f32'),
           'joint_bahdanau': ('bahdanau_content', 'zeros', True, 'f32'), 'location_bf16': ('location', 'zeros', False, 'bf16')}


@pytest.mark.parametrize('case', sorted(_PARITY))
def test_model_parity(cuda, monkeypatch, case):
    """AttentionSeq2Seq / JointCTCAttention with a GRU decoder, decoder and embedding keep probability 0.8: loss, logits and
    every gradient against the float64 statement fed the device's own masks, at the bars of the module docstring, and the
    parameters after one momentum step (learning rate 1e-3) within 1e-5 of the step the statement's gradients give.
    Label lengths 1 / 5 / 3 / 5 / 2: rows finish at step 1 and at the last step.  The cell ran its two-launch form in
    the forward loop (counted)."""
    import _config_parity as cp
    import _cpu_ops_att_ss as ss
    from oracle import lstm as olstm
    from tensorflow_end2end_speech_recognition_amd.utils.io.labels.sparsetensor import list2sparsetensor
    ops = _ops()
    att, prev, joint, dtype = _PARITY[case]
    Att, Joint = _classes()
    B, T, C, L = 5, 17, 9, 1
    x, sl, labels, lsl, ctc = _batch(np.random.RandomState(11), B, T, 12, C, [1, 5, 3, 5, 2])
    kw = dict(sharpening_factor=1.5, logits_temperature=2.0, prev_alpha=prev, dtype=dtype, device=cuda)
    model = _mk(Joint, att, lambda_weight=0.5, honour_ctor_args=True, **kw) if joint else _mk(Att, att, **kw)
    masks = ss.spy_dropout_masks(monkeypatch, ops)
    ops.reset_att_gru_counts(0)
    if joint:
        loss, logits, _, otr, _ = model.compute_loss(x, labels, list2sparsetensor(ctc, -1), sl, lsl, 1.0, 0.8, 0.8)
    else:
        loss, logits, otr, _ = model.compute_loss(x, labels, sl, lsl, 1.0, 0.8, 0.8)
    To = int(lsl.max()) - 1
    assert ops.att_gru_counts(0) == dict(fwd_fused=To, fwd_general=0, bwd=0)
    by_seed = {m[2]: m for m in masks}
    demb = by_seed[model.seed + 1][4][:, :B].transpose(0, 1).cpu().numpy()
    ddec = by_seed[model.seed + 2][4][:, :B].cpu().numpy()
    sd0 = {k: v.clone() for k, v in model.store.state_dict().items()}
    sd = {k: v.cpu().numpy() for k, v in sd0.items()}
    ref = go.gru_model_forward(sd, x, labels, sl, lsl, L, att, clip_enc=50.0, sharpening=1.5, temperature=2.0,
                               drop_emb=demb, drop_dec=ddec, prev_alpha=prev,
                               ctc_labels=[[int(v) for v in r if v >= 0] for r in ctc] if joint else None,
                               lambda_weight=0.5 if joint else None,
                               operand_round=olstm.bf16_round_t if dtype == 'bf16' else None)
    loss_rel = abs(loss.item() - ref['total_loss']) / abs(ref['total_loss'])
    lmax = float(np.abs(ref['logits']).max()) * 2.0
    logits_abs = float(np.abs(logits.cpu().numpy() - ref['logits'] * 2.0).max())
    opt = model._set_optimizer('momentum', 1e-3)
    gv = opt.compute_gradients(loss, model=model)
    assert ops.att_gru_counts(0)['bwd'] == To
    report = []
    worst, worst_name = cp._grad_report(gv, ref['grads'], report, floor=1e-6)
    out = {}
    cp._split_grad_stats(out)
    print('gru model %s: loss rel %.2e  logits abs %.2e (max %.2f)  grad worst %.2e %s' % (case, loss_rel, logits_abs, lmax,
                                                                                         worst, worst_name))
    print('\n'.join(report))
    names = {n for _, n in gv}
    for n in ('gru_cell/gates/kernel', 'gru_cell/gates/bias', 'gru_cell/candidate/kernel', 'gru_cell/candidate/bias'):
        assert D_ + n in names and np.abs(ref['grads'][D_ + n]).max() > 0
    if dtype == 'f32':
        assert loss_rel < 1e-4 and logits_abs < 2e-4
        for g, name in gv:
            r = ref['grads'][name]
            err = np.abs(g.cpu().numpy() - r).max()
            assert err < 2e-3 * max(np.abs(r).max(), 1e-3) + 1e-7, (name, err, np.abs(r).max())
        # one momentum step: p - lr * clip_by_norm(g, 5) from the statement's gradients
        grads64 = {name: ref['grads'][name] for _, name in gv}
        opt.apply_gradients(model._clip_gradients(gv))
        after = model.store.state_dict()
        for name, g in grads64.items():
            nrm = float(np.sqrt((g ** 2).sum()))
            want = sd[name].astype(np.float64) - 1e-3 * g * (5.0 / max(nrm, 5.0))
            err = float(np.abs(after[name].cpu().numpy() - want).max())
            assert err < 1e-5, (name, err)
    else:
        assert loss_rel < 3e-2 and logits_abs < 3e-2 * max(1.0, lmax)
        assert out['grad_worst_matrices'] < 4e-2 and out['grad_worst_peepholes'] < 8e-2 and out['grad_worst_l2'] < 4e-2
    assert ops.check_async_errors(0) == 0


# Seeds (model and batch) found on the CPU with the float64 statement alone -- see each test's docstring for the counted
# share of positions under the margin.
_GREEDY_SEEDS = {'location_carry': 5, 'luong_dot': 5}
_BEAM_SEED = 18


def _decode_case(att, prev, seed, B, device, max_decode_length=12):
    Att, _ = _classes()
    rng = np.random.RandomState(seed)
    T, C = 40, 9
    sl = rng.randint(T // 2, T + 1, size=B).astype(np.int32)
    sl[0] = T
    x = (rng.randn(B, T, 12) * (np.arange(T)[None, :, None] < sl[:, None, None])).astype(np.float32)
    model = _mk(Att, att, seed=seed, sharpening_factor=1.5, prev_alpha=prev, device=device,
                max_decode_length=max_decode_length)
    sd = {k: v.clone() for k, v in model.store.state_dict().items()}
    sd[D_ + 'output_layer/weights'] *= 40.0            # (a head as sharp as a trained one: see tests/test_gpu_att_beam.py)
    sd[D_ + 'output_layer/biases'][C + 1] = 0.35
    model.store.load_state_dict(sd)
    return model, x, sl, C, {k: v.cpu().numpy() for k, v in sd.items()}


@pytest.mark.parametrize('att,prev', [('location', 'carry'), ('luong_dot', 'zeros')])
def test_greedy_decode_against_the_statement(cuda, att, prev):
    """infer() == the statement's greedy decode wherever its top-two margin exceeds 10 x the logits bar (2e-3), and
    _decode_beam(beam_width=1) == infer().  Seeds 5 / 5: under them the float64 statement alone has 0 of 49 (location,
    carry) and 0 of 54 (luong_dot) live positions under the margin (counted on the CPU; asserted <= 10 % here)."""
    from tensorflow_end2end_speech_recognition_amd.models.attention.decoders.beam_search.beam_search_decoder import cut_at_eos
    ops = _ops()
    seed = _GREEDY_SEEDS[att + '_carry' if prev == 'carry' else att]
    model, x, sl, C, sd = _decode_case(att, prev, seed, 5, cuda)
    ids, margin, lmax = go.gru_model_infer(sd, x, sl, 1, att, C, C + 1, 12, clip_enc=50.0, sharpening=1.5, prev_alpha=prev)
    livepos = np.isfinite(margin)
    under = livepos & ~(margin > 10 * 2e-4)
    print('gru greedy %s: %d live positions, %d under the margin, largest |logit| %.2f' % (att, livepos.sum(), under.sum(), lmax))
    assert under.sum() <= 0.1 * livepos.sum()
    ops.reset_att_gru_counts(0)
    got = model.infer(x, sl)
    c = ops.att_gru_counts(0)
    assert c['fwd_fused'] >= got.shape[1] and c['fwd_general'] == 0
    if not under.any():
        assert np.array_equal(got, ids)
    else:
        n = min(got.shape[1], ids.shape[1])
        first_bad = np.where(under.any(0))[0].min()          # ids behind a position under the margin may follow another path
        assert np.array_equal(got[:, :min(n, first_bad)], ids[:, :min(n, first_bad)])
    beam = model._decode_beam(ops.to_device(x, F32, model.device), ops.to_device(sl, I32, model.device), 1)
    for b in range(len(sl)):
        assert cut_at_eos(beam[b], C + 1) == cut_at_eos(got[b], C + 1), b
    assert np.array_equal(model.infer(x, sl, beam_width=1), got)
    assert ops.check_async_errors(0) == 0


def test_beam_search_against_the_host_statement(cuda):
    """infer(beam_width=4, length_penalty_weight=0.6) at 9 utterances -- R = 36 > 32 rows, so every step runs the
    four-launch form (counted) -- equals BeamSearchDecoder driven by the float64 GRU step: every hypothesis of every
    utterance whose margin (smallest gap among the top W + 1 candidate scores) is above 1e-3, ids exactly and scores to
    1e-3.  Seed 18: the float64 statement alone has 0 of 9 utterances under the margin (smallest 1.4e-3) (counted on the CPU; at most 10 %
    -- i.e. none of nine -- may be, asserted)."""
    ops = _ops()
    model, x, sl, C, sd = _decode_case('bahdanau_content', 'zeros', _BEAM_SEED, 9, cuda)
    want = go.gru_beam_infer(sd, x, sl, 1, 'bahdanau_content', C, C + 1, 12, 4, 0.6, clip_enc=50.0, sharpening=1.5)
    skipped = [b for b, r in enumerate(want) if not r['margin'] > 1e-3]
    print('gru beam: margins %s' % ['%.3g' % r['margin'] for r in want])
    assert len(skipped) <= 0.1 * len(want), [r['margin'] for r in want]
    ops.reset_att_gru_counts(0)
    best = model.infer(x, sl, beam_width=4, length_penalty_weight=0.6)
    raw = model._beam_raw
    assert ops.att_gru_counts(0) == dict(fwd_fused=0, fwd_general=raw['steps_issued'], bwd=0)
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


def test_lstm_decoder_is_untouched_by_a_gru_model_in_the_process(cuda):
    """An LSTM-decoder model built and stepped before and after a GRU model in the same process: loss, logits and every
    gradient bit for bit, greedy and beam decodes equal, and none of the GRU entry points called (their counters stay 0)."""
    ops = _ops()
    Att, _ = _classes()
    x, sl, labels, lsl, _ = _batch(np.random.RandomState(3), 5, 17, 12, 9, [1, 5, 3, 5, 2])
    runs = []
    for k in range(2):
        ops.reset_att_gru_counts(0)
        lstm = _mk(Att, 'location', decoder_type='lstm', prev_alpha='carry', device=cuda)
        runs.append(_step(lstm, x, labels, sl, lsl) + (lstm.infer(x, sl), lstm.infer(x, sl, beam_width=3)))
        assert ops.att_gru_counts(0) == dict(fwd_fused=0, fwd_general=0, bwd=0)
        if k == 0:
            gru = _mk(Att, 'location', prev_alpha='carry', device=cuda)
            _step(gru, x, labels, sl, lsl)
            gru.infer(x, sl)
            gru.infer(x, sl, beam_width=3)
            assert ops.att_gru_counts(0)['fwd_fused'] > 0 and ops.att_gru_counts(0)['bwd'] > 0
    a, b = runs
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and all(torch.equal(p, q) for p, q in zip(a[2], b[2]))
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
    assert ops.check_async_errors(0) == 0


def test_seeded_gru_step_is_repeatable(cuda):
    """Two fresh GRU-decoder models with the same seed: a training step (encoder, decoder and embedding dropout on) gives
    the same loss, logits and updated parameters bit for bit."""
    Att, _ = _classes()
    x, sl, labels, lsl, _ = _batch(np.random.RandomState(4), 5, 17, 12, 9, [1, 5, 3, 5, 2])
    runs = []
    for _ in range(2):
        model = _mk(Att, 'bahdanau_content', device=cuda)
        loss, logits, _, _ = model.compute_loss(x, labels, sl, lsl, 0.9, 0.8, 0.8)
        model.train(loss, 'adam', 1e-3)
        loss2, *_ = model.compute_loss(x, labels, sl, lsl, 0.9, 0.8, 0.8)
        runs.append((loss.item(), logits.clone(), model.store.flat.clone(), loss2.item()))
    a, b = runs
    assert a[0] == b[0] and a[3] == b[3] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
