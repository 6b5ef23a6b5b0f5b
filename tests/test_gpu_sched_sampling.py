"""GPU: scheduled sampling and label smoothing for the attention decoder (csrc/dec_loop.hip: asr_att_decoder_fwd_ss with
att_ss_select_kernel; csrc/attention.hip: asr_seq_xent_ls) -- the selection rule at the kernel's edges, the loop against asr_att_decoder_fwd
(no draw set) and asr_att_decoder_infer (every draw set), the models against the float64 statement of the whole loss
(tests/_cpu_ops_att_ss.py), the draws, the smoothed cross-entropy against float64, and repeatability.

Bars.  Loop level: the forward bar of test_gpu_attention's teacher-forced loop test (2e-5 of the array's largest entry).
Model level, fp32: those of test_gpu_attention.test_attention_model_parity (loss 1e-4 relative, logits 2e-4, gradients
2e-3 of the gradient's largest entry); bf16 operands: loss as test_gpu_attention.test_attention_bf16_operands (3e-2), logits
and gradients as the bf16 attention runs of test_gpu_configs (3e-2 x max(1, largest logit); 4e-2 matrices, 8e-2 peepholes,
4e-2 relative L2).  A fed id is compared with the statement's own argmax where the statement's top-two margin exceeds
10 x the logits bar (the project's margin convention); the share of sampled positions under it is capped at 10 %."""
import numpy as np
import pytest
import torch

import _cpu_ops_att_ss as ss

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32


def _ops():
    from tensorflow_end2end_speech_recognition_amd import ops
    return ops


# ------------------------------------------------------------------------------------------------------ the loop's operands
# U = 2H = 64, A = 36: the narrowest decoder the suite's loop test runs (its A36_general_q case); T = 11 frames; three rows
# whose labels are 2, 4 and 6 long (<SOS> and <EOS> included), i.e. live for 1, 3 and 5 of the To = 5 steps
_B, _T, _TO, _U, _A, _E2 = 3, 11, 5, 64, 36, 64
_LSL = np.array([2, 4, 6])
# set draws hold 2.0 (any non-zero value samples); set at finished positions too, clear at live ones
_DRAW = [[2, 2, 2], [2, 0, 2], [0, 2, 2], [2, 2, 0], [2, 2, 2]]


def _arrays(C2, Em, dropout, seed=0, tie=None):
    """CPU tensors: the loop dict `a` (row 0 of dec_in filled: embedding of <SOS> times its mask | zero context | h0), the
    head, teacher ids, live.  tie = (i, j): class j is a copy of class i in the output layer and both carry a bias that
    makes them the maximum of every row."""
    rng = np.random.RandomState(seed + C2 + Em)
    B, T, To, U, A, E2 = _B, _T, _TO, _U, _A, _E2
    Din = Em + E2 + U
    f = lambda *s, sc=1.0: torch.tensor(rng.randn(*s) * sc, dtype=F32)                     # noqa: E731
    seq_len = torch.tensor([T, 7, 4], dtype=I32)
    enc = f(T, B, E2, sc=0.5) * (torch.arange(T).view(T, 1, 1) < seq_len.view(1, B, 1))
    live = torch.tensor((np.arange(To)[:, None] < (_LSL - 1)[None, :]).astype(np.float32))
    sos, eos = C2 - 2, C2 - 1
    teacher = torch.full((To, B), eos, dtype=I32)
    for b in range(B):
        n = int(_LSL[b]) - 1                                  # <SOS> y: the tokens fed while the row is live
        teacher[0, b] = sos
        teacher[1:n, b] = torch.tensor(rng.randint(0, C2 - 2, size=n - 1), dtype=I32)
    emb = f(C2, Em, sc=0.5)
    emb_mask = torch.tensor((rng.rand(To, B, Em) < 0.8) / 0.8, dtype=F32) if dropout else None
    a = dict(To=To, B=B, T=T, U=U, Em=Em, E2=E2, A=A, att_mode=0, has_query_fc=1, carry_alpha=0, taps=0, enc_dtype=0,
             forget_bias=1.0, cell_clip=3.0, sharpening=1.5, W_cell=f(Din, 4 * U, sc=0.08), b_cell=f(4 * U, sc=0.1),
             peep=f(3, U, sc=0.1), W_q=f(U, A, sc=0.1), v=f(A, sc=0.5), keys=f(T, B, A, sc=0.5), enc=enc, seq_len=seq_len,
             live=live, dmask=torch.tensor((rng.rand(To, B, U) < 0.8) / 0.8, dtype=F32) if dropout else None,
             dec_in=torch.full((To, B, Din), float('nan')), av_in=torch.full((To, B, U + E2), float('nan')),
             alpha_all=torch.full((To, B, T), float('nan')), gates_all=torch.full((To, B, 4 * U), float('nan')),
             craw_all=torch.full((To, B, U), float('nan')), c_all=torch.full((To + 1, B, U), float('nan')),
             h_all=torch.full((To + 1, B, U), float('nan')), qz_all=torch.full((To, B, A), float('nan')))
    a['c_all'][0] = f(B, U, sc=0.3)
    a['h_all'][0] = f(B, U, sc=0.3)
    e0 = emb[teacher[0].long()]
    a['dec_in'][0, :, :Em] = e0 * emb_mask[0] if dropout else e0
    a['dec_in'][0, :, Em:Em + E2] = 0.0
    a['dec_in'][0, :, Em + E2:] = a['h_all'][0]
    head = dict(W_av=f(U + E2, U, sc=0.15), W_out=f(U, C2, sc=0.6), b_out=f(C2, sc=0.3), embedding=emb)
    if tie is not None:
        i, j = tie
        head['W_out'][:, j] = head['W_out'][:, i]
        head['b_out'][i] = head['b_out'][j] = 40.0
    return a, head, teacher, live, emb_mask


def _to(d, dev):
    return {k: (v.clone().to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}


def _nan_out(C2, dev):
    return (torch.full((_TO, _B, _U), float('nan'), device=dev), torch.full((_TO, _B, C2), float('nan'), device=dev),
            torch.full((_TO, _B), -1, dtype=I32, device=dev))


def _first_max(x2d):
    """First-maximum argmax of every row, spelled out (no library tie rule assumed)."""
    x = x2d.cpu().numpy()
    return np.array([int(np.flatnonzero(r == r.max())[0]) for r in x])


@pytest.mark.parametrize('tie', [False, True])
@pytest.mark.parametrize('C2,Em', [(7, 10), (300, 300), (7, 300), (300, 10)])
def test_selection_rule_at_the_kernels_edges(cuda, C2, Em, tie):
    """ids_fed[k] is the first-maximum argmax of the device's own logits[k-1] where draw[k] and live[k] are set and
    labels[:, k] everywhere else (draws set on finished rows included), exactly; the embedding columns of dec_in[k] are
    embedding[ids_fed[k]] * emb_mask[k], exactly; every output prefilled with NaN (-1 for the ids).  C2 = 300 / Em = 300
    run the kernel's stride loops past its 256 threads on widths that are no multiple of 64.  tie: the maximum stands at
    two classes in every row (classes in different waves of the reduction for C2 = 300) and the lower index is fed."""
    ops = _ops()
    pair = ((2, 5) if C2 == 7 else (70, 290)) if tie else None
    a, head, teacher, live, emb_mask = _arrays(C2, Em, dropout=True, tie=pair)
    draw = torch.tensor(_DRAW, dtype=F32)
    ga, gh = _to(a, cuda), _to(head, cuda)
    out = _nan_out(C2, cuda)
    av, logits, ids = ops.att_decoder_fwd_ss(ga, gh['W_av'], gh['W_out'], gh['b_out'], gh['embedding'], teacher.to(cuda),
                                             draw.to(cuda), emb_mask.to(cuda), out=out)
    torch.cuda.synchronize()
    assert ops.check_async_errors(0) == 0
    assert bool(torch.isfinite(av).all()) and bool(torch.isfinite(logits).all())
    for name in ('dec_in', 'av_in', 'alpha_all', 'gates_all', 'craw_all', 'c_all', 'h_all', 'qz_all'):
        assert bool(torch.isfinite(ga[name]).all()), name
    ids_h, n_sampled = ids.cpu().numpy(), 0
    assert np.array_equal(ids_h[0], teacher[0].numpy())
    for k in range(1, _TO):
        use = (draw[k].numpy() != 0) & (live[k].numpy() != 0)
        want = np.where(use, _first_max(logits[k - 1]), teacher[k].numpy())
        assert np.array_equal(ids_h[k], want), (k, ids_h[k], want)
        n_sampled += int(use.sum())
        if tie:
            assert torch.equal(logits[k - 1][:, pair[0]], logits[k - 1][:, pair[1]])
            assert (ids_h[k][use] == pair[0]).all()
    assert n_sampled == 4
    want_emb = gh['embedding'][ids.long()] * emb_mask.to(cuda)                                   # [To,B,Em]
    assert torch.equal(ga['dec_in'][:, :, :Em], want_emb)


@pytest.mark.parametrize('C2,Em', [(7, 10), (300, 300)])
def test_no_draw_set_is_the_teacher_forced_loop(cuda, C2, Em):
    """draw all zero: dec_in, alpha_all, c_all, h_all and av_in are asr_att_decoder_fwd's on the same inputs bit for bit
    (the same dec_fwd_step launches; the embedding columns are the same product), ids_fed are the labels, and the logits /
    attentional vectors are within the teacher-forced loop test's forward bar (2e-5 of the array's largest entry, floor
    1e-2) of the float64 step-by-step statement."""
    ops = _ops()
    a, head, teacher, live, emb_mask = _arrays(C2, Em, dropout=True)
    draw = torch.zeros(_TO, _B)
    ga, gh = _to(a, cuda), _to(head, cuda)
    av, logits, ids = ops.att_decoder_fwd_ss(ga, gh['W_av'], gh['W_out'], gh['b_out'], gh['embedding'], teacher.to(cuda),
                                             draw.to(cuda), emb_mask.to(cuda), out=_nan_out(C2, cuda))
    plain = _to(a, cuda)
    plain['dec_in'][:, :, :Em] = gh['embedding'][teacher.to(cuda).long()] * emb_mask.to(cuda)
    ops.att_decoder_fwd(plain)
    torch.cuda.synchronize()
    assert torch.equal(ids.cpu(), teacher)
    for name in ('dec_in', 'alpha_all', 'c_all', 'h_all', 'av_in', 'gates_all', 'craw_all', 'qz_all'):
        assert torch.equal(ga[name], plain[name]), name
    ra = _to(a, 'cpu')
    rav, rlg, rids = ss._att_decoder_fwd_ss(ra, head['W_av'], head['W_out'], head['b_out'], head['embedding'], teacher, draw,
                                            emb_mask)
    rel = lambda x, y: float(np.abs(x.cpu().double().numpy() - y.double().numpy()).max() /          # noqa: E731
                             max(np.abs(y.double().numpy()).max(), 1e-2))
    for name, got, ref in (('logits', logits, rlg), ('av', av, rav), ('alpha_all', ga['alpha_all'], ra['alpha_all'])):
        err = rel(got, ref)
        print('C2 %d Em %d %s %.3g' % (C2, Em, name, err))
        assert err < 2e-5, (name, err)
    assert torch.equal(rids, teacher)
    assert ops.check_async_errors(0) == 0


@pytest.mark.parametrize('C2,Em', [(7, 10), (300, 300)])
def test_every_draw_set_is_the_greedy_loop_while_both_are_live(cuda, C2, Em):
    """draw all one, no dropout: wherever a row is live here and in asr_att_decoder_infer on the same parameters, logits[k]
    is infer's bit for bit (the same launches on the same inputs) and ids_fed[k+1] is infer's ids[k]."""
    ops = _ops()
    a, head, teacher, live, _ = _arrays(C2, Em, dropout=False)
    head['b_out'][C2 - 1] -= 3.0                              # <EOS> seldom wins: infer's rows stay live for a few steps
    ga, gh = _to(a, cuda), _to(head, cuda)
    draw = torch.ones(_TO, _B)
    av, logits, ids = ops.att_decoder_fwd_ss(ga, gh['W_av'], gh['W_out'], gh['b_out'], gh['embedding'], teacher.to(cuda),
                                             draw.to(cuda), None, out=_nan_out(C2, cuda))
    ia = _to(a, cuda)
    ilive = torch.zeros(_TO + 1, _B, device=cuda)
    ilive[0] = 1.0
    ia.update(live=ilive, dmask=None)
    inf = ops.att_decoder_infer(ia, gh['W_av'], gh['W_out'], gh['b_out'], gh['embedding'], C2 - 1, _B, check_every=0)
    torch.cuda.synchronize()
    assert inf['steps_issued'] == _TO
    lv, il = live.numpy() != 0, inf['live'].cpu().numpy() != 0
    both = lv & il[:_TO]
    assert both[0].all() and both.sum() >= 6                   # (rows 1 and 2 are compared over several steps)
    lg, ilg = logits.cpu(), inf['logits'].cpu()
    ids_h, iids = ids.cpu().numpy(), inf['ids'].cpu().numpy()
    n_ids = 0
    for k in range(_TO):
        for b in range(_B):
            if both[k, b]:
                assert torch.equal(lg[k, b], ilg[k, b]), (k, b)
                if k + 1 < _TO and lv[k + 1, b]:
                    assert ids_h[k + 1, b] == iids[k, b], (k, b)
                    n_ids += 1
    assert n_ids >= 4
    assert ops.check_async_errors(0) == 0


# ------------------------------------------------------------------------------------------------------------- model level
def _mk(cls, att, dtype, seed, U, **kw):
    D, H, L, A, Em, C = 12, 64, 1, 32, 8, 9
    return cls(input_size=D, encoder_type='blstm', encoder_num_units=H, encoder_num_layers=L, encoder_num_proj=None,
               attention_type=att, attention_dim=A, decoder_type='lstm', decoder_num_units=U, decoder_num_layers=1,
               embedding_dim=Em, num_classes=C, sos_index=C, eos_index=C + 1, max_decode_length=12, parameter_init=0.1,
               clip_grad_norm=5.0, clip_activation_encoder=50, clip_activation_decoder=50, dtype=dtype, seed=seed,
               label_smoothing_prob=0.1, **kw)


# case -> (attention type, operand dtype, joint, model seed).  The seeds were chosen on the CPU with the float64 statement
# alone (scripts/probe_sched_sampling.py --seeds: the statement rolled out from its own argmax under every draw set and
# under three Bernoulli(0.5) tables; these seeds have no sampled position under the margin in any of the four, of 30 / 18 /
# 17 / 19 sampled positions).
_MODEL_CASES = {'location_f32': ('location', 'f32', False, 6), 'luong_dot_f32': ('luong_dot', 'f32', False, 7),
                'location_bf16': ('location', 'bf16', False, 5), 'joint_bahdanau_f32': ('bahdanau_content', 'f32', True, 8)}
_BATCH_SEED = 11


def model_case(name, device):
    """Model, batch and statement keywords of a parity case (also what the seed search of the probe script builds)."""
    from tensorflow_end2end_speech_recognition_amd.models.attention.attention_seq2seq import AttentionSeq2Seq
    from tensorflow_end2end_speech_recognition_amd.models.attention.joint_ctc_attention import JointCTCAttention
    from oracle import lstm as olstm
    att, dtype, joint, seed = _MODEL_CASES[name]
    B, T, D, C = 8, 17, 12, 9
    x, sl, labels, lsl, ctc = ss.batch(np.random.RandomState(_BATCH_SEED), B, T, D, C, 7)
    kw = dict(sharpening_factor=1.5, device=device)
    if joint:
        model = _mk(JointCTCAttention, att, dtype, seed, 128, lambda_weight=0.5, honour_ctor_args=True, **kw)
    else:
        model = _mk(AttentionSeq2Seq, att, dtype, seed, 128, **kw)
    sd = {k: v.clone() for k, v in model.store.state_dict().items()}
    if dtype == 'bf16':
        # the bf16 logits bar is 3e-2, the margin 0.3: wider than the top-two gaps of a freshly initialised head, so this
        # case gives one class (label 3) a bias of 1 and the fed prediction is that class nearly everywhere
        sd['attention_decoder/decoder/output_layer/biases'][3] = 1.0
    else:
        # a head sharpened a little, as a trained one is: the top-two gaps of a fresh head (logits of ~0.3) are within a
        # few times the 2e-3 margin too often for the 10 % cap to say anything
        sd['attention_decoder/decoder/output_layer/weights'] *= 4.0
    model.store.load_state_dict(sd)
    stmt = dict(clip_enc=50.0, clip_dec=50.0, sharpening=1.5, operand_round=olstm.bf16_round_t if dtype == 'bf16' else None)
    return model, (x, sl, labels, lsl, ctc if joint else None), stmt, dtype


@pytest.mark.parametrize('case', sorted(_MODEL_CASES))
def test_model_parity_with_sampling_smoothing_and_dropout(cuda, monkeypatch, case):
    """AttentionSeq2Seq (location fp32 and bf16 operands, luong_dot) and JointCTCAttention at p = 0.5, eps = 0.1, decoder and
    embedding keep probability 0.8: loss, logits and every gradient against the float64 statement fed the device's draws,
    masks and fed ids, at the bars of the module docstring; fed ids equal the statement's own argmax above the margin and
    the labels wherever nothing was sampled.  Seeds: batch 11; model 6 (location fp32), 7 (luong_dot), 5 (location bf16), 8
    (joint) -- under each the statement alone has 0 sampled positions under the margin (see _MODEL_CASES).  Share under
    the margin with the device's own draws and masks, measured on an MI355X: 0 of 15 (location fp32), 1 of 16 (luong_dot),
    0 of 15 (location bf16), 0 of 14 (joint)."""
    import _config_parity as cp
    ops = _ops()
    model, (x, sl, labels, lsl, ctc), stmt, dtype = model_case(case, cuda)
    r = ss.model_step_against_statement(monkeypatch, ops, model, x, labels, sl, lsl, 1, _MODEL_CASES[case][0], 0.5,
                                        (1.0, 0.8, 0.8), ctc_labels=ctc, **stmt)
    logits_bar = 2e-4 if dtype == 'f32' else 3e-2 * max(1.0, r['logits_max'])
    ss.judge_fed(r, 10 * logits_bar)
    report = []
    worst, worst_name = cp._grad_report(r['gv'], r['ref']['grads'], report, floor=1e-6)
    out = {}
    cp._split_grad_stats(out)
    print('%s: loss %.6f rel %.2e  logits abs %.2e (max %.2f)  sampled %d  under the margin %d  wrong %d  grad worst %.2e %s'
          % (case, r['loss'], r['loss_rel'], r['logits_abs'], r['logits_max'], r['n_sampled'], r['n_excluded'], r['n_wrong'],
             worst, worst_name))
    print('\n'.join(report))
    assert r['n_sampled'] >= 8 and r['teacher_ok']
    assert r['n_excluded'] <= 0.1 * r['n_sampled'], (r['n_excluded'], r['n_sampled'])
    assert r['n_wrong'] == 0
    assert (r['fed'] != labels[:, :r['fed'].shape[1]]).any()
    if dtype == 'f32':
        assert r['loss_rel'] < 1e-4 and r['logits_abs'] < 2e-4
        for name, (err, mag) in r['grads'].items():
            assert err < 2e-3 * max(mag, 1e-3) + 1e-7, (name, err, mag)
    else:
        assert r['loss_rel'] < 3e-2 and r['logits_abs'] < logits_bar
        assert out['grad_worst_matrices'] < 4e-2 and out['grad_worst_peepholes'] < 8e-2 and out['grad_worst_l2'] < 4e-2
    assert ops.check_async_errors(0) == 0


def test_draws_are_the_projects_generator(cuda, monkeypatch):
    """The draws a step used are ops.dropout_mask((To, Bp), p, seed + 3, calls << 40) exactly, and over a [64, 64] table at
    p = 0.25 the share of set draws is within 5 sigma of p (sigma = sqrt(p (1 - p) / 4096))."""
    ops = _ops()
    model, (x, sl, labels, lsl, _), _, _ = model_case('location_f32', cuda)
    model.compute_loss(x, labels, sl, lsl, 1.0, 0.8, 0.8, scheduled_sampling_prob=0.5)
    draw = model._ss_last['draw']
    To = int(lsl.max()) - 1
    assert draw.shape[0] == To and draw.shape[1] >= x.shape[0] and model._calls == 3
    again = ops.dropout_mask(tuple(draw.shape), 0.5, model.seed + 3, model._calls << 40, cuda)
    assert torch.equal(draw, again) and set(np.unique(draw.cpu().numpy()).tolist()) <= {0.0, 2.0}
    # a second step draws from another counter block
    model.compute_loss(x, labels, sl, lsl, 1.0, 0.8, 0.8, scheduled_sampling_prob=0.5)
    assert model._calls == 6 and not torch.equal(model._ss_last['draw'], draw)
    p = 0.25
    table = ops.dropout_mask((64, 64), p, 12345 + 3, 7 << 40, cuda)
    share = float((table != 0).float().mean())
    sigma = np.sqrt(p * (1 - p) / 4096)
    print('share of set draws %.4f (p %.2f, sigma %.4f)' % (share, p, sigma))
    assert abs(share - p) < 5 * sigma


@pytest.mark.parametrize('Cc', [5, 70])
def test_smoothed_cross_entropy_against_float64(cuda, Cc):
    """asr_seq_xent_ls: 9 rows, three of them masked and holding NaN logits; losses and gradients against float64 at the
    precision of the format -- the row loss carries the rounding of lse and x_t (magnitudes up to ~16, ulp 1e-6: bar 1e-5
    absolute), the gradient that of exp(x - lse) (argument up to ~20 in magnitude, 20 x 6e-8 relative on values <= 1: bar
    4e-6); masked rows exact zeros; eps = 0 through the new entry is asr_seq_xent bit for bit."""
    ops = _ops()
    rng = np.random.RandomState(Cc)
    rows = 9
    x = torch.tensor(rng.randn(rows, Cc) * 3, dtype=F32)
    tg = torch.tensor(rng.randint(0, Cc, size=rows), dtype=I32)
    w = torch.tensor([1, 0, 1, 0.5, 0, 1, 2, 0, 1], dtype=F32)
    x[w == 0] = float('nan')
    for ls in (0.1, 0.6):
        row, dl = ops.seq_xent(x.to(cuda), tg.to(cuda), w.to(cuda), 1e-10, 0.37, smoothing=ls)
        r64, d64 = ss.seq_xent_ls_f64(x, tg, w, 1e-10, ls, 0.37)
        assert torch.equal(row.cpu()[w == 0], torch.zeros(3)) and torch.equal(dl.cpu()[w == 0], torch.zeros(3, Cc))
        e_row = float((row.cpu().double() - r64).abs().max())
        e_dl = float((dl.cpu().double() - d64).abs().max())
        print('C %d eps %.1f: row loss %.2e  dlogits %.2e' % (Cc, ls, e_row, e_dl))
        assert e_row < 1e-5 and e_dl < 4e-6
        # against torch's own label-smoothed cross-entropy too (live rows)
        on = w != 0
        ce = torch.nn.functional.cross_entropy(x[on].double() + 1e-10, tg[on].long(), reduction='none', label_smoothing=ls)
        assert float((r64[on] - ce * w[on].double()).abs().max()) < 1e-12
        row2, none = ops.seq_xent(x.to(cuda), tg.to(cuda), w.to(cuda), 1e-10, 0.37, want_grad=False, smoothing=ls)
        assert none is None and torch.equal(row2, row)
    a = ops.seq_xent_ls(x.to(cuda), tg.to(cuda), w.to(cuda), 1e-10, 0.0, 0.37)
    b = ops.seq_xent(x.to(cuda), tg.to(cuda), w.to(cuda), 1e-10, 0.37)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert ops.check_async_errors(0) == 0


def test_seeded_step_with_sampling_is_repeatable(cuda):
    """Two fresh models with the same seed: a training step at p = 0.5 (dropout and smoothing on) gives the same loss, logits,
    fed ids and updated parameters bit for bit."""
    runs = []
    for _ in range(2):
        model, (x, sl, labels, lsl, _), _, _ = model_case('location_f32', cuda)
        loss, logits, _, _ = model.compute_loss(x, labels, sl, lsl, 0.9, 0.8, 0.8, scheduled_sampling_prob=0.5)
        fed = model._ss_last['ids_fed'].clone()
        model.train(loss, 'adam', 1e-3)
        loss2, *_ = model.compute_loss(x, labels, sl, lsl, 0.9, 0.8, 0.8, scheduled_sampling_prob=0.5)
        runs.append((loss.item(), logits.clone(), fed, model.store.flat.clone(), loss2.item()))
    a, b = runs
    assert a[0] == b[0] and a[4] == b[4] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    assert (a[2][:, :x.shape[0]].t().cpu().numpy() != labels[:, :a[2].shape[0]]).any()
