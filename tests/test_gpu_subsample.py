"""GPU: time subsampling (subsample_list / subsample_type) -- the two kernels against the numpy statement with exact
equality (they move data), and the CTC / joint CTC-attention models over the subsampled encoders against the float64
statement composed from the oracle's layers (tests/_cpu_ops_subsample.py) at the bars of the plain models' parity tests
(tests/test_gpu_model.py, tests/test_gpu_attention.py)."""
import numpy as np
import pytest
import torch

import _cpu_ops_subsample as sub
from oracle import attention as oatt
from oracle import ctc as octc
from oracle import decoders as odec
from oracle import optim as oopt

pytestmark = pytest.mark.gpu

KINDS = ('drop', 'concat')


# ---------------------------------------------------------------- the kernels
def _op_case(rng, T, W):
    Bp, B = 16, 5
    lens = np.zeros(Bp, dtype=np.int32)
    lens[:B] = [T, 8, 1, 2, 5]
    return Bp, B, lens, rng.randn(T, Bp, W).astype(np.float32)


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('kind', KINDS)
# 128: 16-byte groups everywhere; 20: 16-byte groups for fp32 (20 % 4 == 0), one element per lane for bf16 input
# (20 % 8 != 0); 18: one element per lane in every kernel
@pytest.mark.parametrize('W', [128, 20, 18])
@pytest.mark.parametrize('T', [9, 8])
def test_time_subsample_fwd_is_the_statement_and_reads_no_padded_frame(cuda, T, W, kind, dtype):
    from tensorflow_end2end_speech_recognition_amd import ops
    Bp, B, lens, x = _op_case(np.random.RandomState(T * W), T, W)
    xt = torch.tensor(x)
    if dtype == 'bf16':
        xt = xt.to(torch.bfloat16)
    x_seen = xt.float().numpy().copy()                 # the values the kernel loads (rounded once for bf16)
    for b in range(Bp):                                # NaN wherever the kernel must not look: frames >= 2 (len >> 1),
        xt[2 * (int(lens[b]) >> 1):, b] = float('nan')  # the odd trailing frame included, and every pad row
    y, lo = ops.time_subsample_fwd(xt.cuda().contiguous(), torch.tensor(lens).cuda(), B, kind)
    want, want_lo = sub.subsample_fwd_np(x_seen, lens, kind, B)
    y, lo = y.cpu().numpy(), lo.cpu().numpy()
    assert y.shape == (B, T // 2, W * (2 if kind == 'concat' else 1)) and y.dtype == np.float32
    assert np.array_equal(lo, want_lo) and np.array_equal(lo, lens >> 1) and lo.shape == (Bp,)
    assert np.isfinite(y).all()
    for b in range(B):
        assert not y[b, int(lo[b]):].any()
    assert np.array_equal(y, want)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('W', [128, 20, 18])        # 18: the scalar instantiation of the backward kernel
@pytest.mark.parametrize('T', [9, 8])
def test_time_subsample_bwd_is_the_transpose_and_writes_every_element(cuda, T, W, kind):
    from tensorflow_end2end_speech_recognition_amd import ops
    Bp, B, lens, _ = _op_case(np.random.RandomState(T + W), T, W)
    lo = lens >> 1
    Wo = W * (2 if kind == 'concat' else 1)
    dy = np.random.RandomState(3).randn(T // 2, Bp, Wo).astype(np.float32)
    want = sub.subsample_bwd_np(dy, lo, T, kind)
    dyt = torch.tensor(dy)
    for b in range(Bp):
        dyt[int(lo[b]):, b] = float('nan')             # never read at t' >= len_out[b]
    # the output buffer starts as NaN: every element has to be written, the zeros included
    out = torch.full((T, Bp, W), float('nan'), device='cuda')
    dx = ops.time_subsample_bwd(dyt.cuda().contiguous(), torch.tensor(lo.astype(np.int32)).cuda(), T, kind, out=out)
    assert dx is out
    dx = dx.cpu().numpy()
    assert dx.shape == (T, Bp, W)
    assert np.array_equal(dx, want)
    # <y, dy> = <x, dx>: the pair is a transpose pair on the device too
    x = np.random.RandomState(4).randn(T, Bp, W).astype(np.float32)
    y, _ = ops.time_subsample_fwd(torch.tensor(x).cuda(), torch.tensor(lens).cuda(), Bp, kind)
    lhs = float((y.cpu().numpy().astype(np.float64).transpose(1, 0, 2) * np.nan_to_num(dyt.numpy())).sum())
    assert abs(lhs - float((x.astype(np.float64) * dx).sum())) < 1e-9 * max(1.0, abs(lhs))


def test_time_subsample_ops_refuse_what_they_cannot_run(cuda):
    from tensorflow_end2end_speech_recognition_amd import ops
    x = torch.zeros((4, 16, 8), device='cuda')
    sl = torch.full((16,), 4, dtype=torch.int32, device='cuda')
    with pytest.raises(ValueError):
        ops.time_subsample_fwd(x, sl, 16, 'max')
    with pytest.raises(ValueError):
        ops.time_subsample_fwd(x, sl, 17, 'drop')
    with pytest.raises(RuntimeError):
        ops.time_subsample_fwd(x.cpu(), sl.cpu(), 16, 'drop')
    y, lo = ops.time_subsample_fwd(x[:1].contiguous(), sl, 16, 'drop')          # T // 2 == 0: lengths only
    assert y.shape == (16, 0, 8) and np.array_equal(lo.cpu().numpy(), np.zeros(16, dtype=np.int32))


# ---------------------------------------------------------------- the CTC model
def _batch(rng, B, T, D, C, k):
    """Odd T and odd lengths; labels of max(1, len_out // 2) symbols stay feasible even if every symbol repeats."""
    x = rng.randn(B, T, D).astype(np.float32)
    sl = rng.randint(max(2 << k, T // 2), T + 1, size=B).astype(np.int32)
    sl[0] = T
    labs = []
    for b in range(B):
        x[b, sl[b]:] = 0
        labs.append([int(v) for v in rng.randint(0, C, size=max(1, (int(sl[b]) >> k) // 2))])
    dense = np.full((B, max(len(l) for l in labs)), -1, dtype=np.int64)
    for b, l in enumerate(labs):
        dense[b, :len(l)] = l
    return x, sl, labs, dense


CTC_CASES = [('blstm', 5, 23, 12, 64, 3, 10, (False, True, False), 'drop'),
             ('blstm', 5, 23, 12, 64, 3, 10, (True, False, True), 'concat'),
             ('lstm', 16, 30, 24, 64, 2, 20, (True, False), 'drop')]


def _ctc(enc, D, H, L, C, lst, kind, **kw):
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    kw.setdefault('dtype', 'f32')
    kw.setdefault('seed', 3)
    return CTC(encoder_type=enc, input_size=D, num_units=H, num_layers=L, num_classes=C, parameter_init=0.1,
               clip_grad_norm=5.0, clip_activation=50, device='cuda:0', subsample_list=list(lst), subsample_type=kind,
               **kw)


@pytest.mark.parametrize('enc,B,T,D,H,L,C,lst,kind', CTC_CASES)
def test_subsampled_ctc_model_loss_grads_step_and_decoders(cuda, enc, B, T, D, H, L, C, lst, kind):
    from tensorflow_end2end_speech_recognition_amd.utils.io.labels.sparsetensor import list2sparsetensor, sparsetensor2list
    k = sum(lst)
    rng = np.random.RandomState(B + T)
    x, sl, labs, dense = _batch(rng, B, T, D, C, k)
    model = _ctc(enc, D, H, L, C, lst, kind, weight_decay=1e-4)
    sd = {n: v.cpu().numpy() for n, v in model.store.state_dict().items()}
    ref = sub.ctc_model_forward(sd, x, labs, sl, L, 2 if enc == 'blstm' else 1, lst, kind, cell_clip=50.0,
                                weight_decay=1e-4)
    loss, logits = model.compute_loss(x, list2sparsetensor(dense, -1), sl, keep_prob=1.0)
    sl_out = model.output_seq_len(sl)
    assert np.array_equal(sl_out, sl >> k) and np.array_equal(ref['seq_len'], sl >> k)
    assert logits.shape == (T >> k, B, C + 1)
    rel_loss = abs(loss.item() - ref['total_loss']) / abs(ref['total_loss'])
    rel_utt = np.abs(model.ctc_losses.cpu().numpy() - ref['ctc_losses']).max() / ref['ctc_losses'].max()
    abs_logits = np.abs(logits.cpu().numpy() - ref['logits']).max()
    print('loss rel %.3g  per-utterance rel %.3g  logits abs %.3g' % (rel_loss, rel_utt, abs_logits))
    assert rel_loss < 1e-4
    assert rel_utt < 1e-4
    assert abs_logits < 1e-4
    # greedy and width-4 beam labels: the oracle decoders on the oracle logits with the reduced lengths
    ref_bm = np.transpose(ref['logits'], (1, 0, 2))
    hyp = sparsetensor2list(model.decoder(logits, sl_out, beam_width=1), B)
    assert [list(h) for h in hyp] == odec.greedy_decode(ref_bm, sl_out, C)
    dec_b = model.decoder(logits, sl_out, beam_width=4, merge_repeated=False)
    ref_b, _ = odec.beam_search_decode(octc.log_softmax(ref_bm), sl_out, C, 4)
    assert [list(h) for h in sparsetensor2list(dec_b, B)] == ref_b
    # gradients (before clipping), then clip + one momentum step
    opt = model._set_optimizer('momentum', 0.01)
    gv = opt.compute_gradients(loss, model=model)
    assert sorted(n for _, n in gv) == sorted(ref['grads'])
    for g, name in gv:
        r = ref['grads'][name]
        rel = np.abs(g.cpu().numpy() - r).max() / max(np.abs(r).max(), 1e-8)
        assert rel < 2e-3, (name, rel)
    model._clip_gradients(gv)
    opt.apply_gradients(gv)
    for name in model.store.names:
        p_ref = sd[name].astype(np.float64) - 0.01 * oopt.clip_by_norm(ref['grads'][name], 5.0)
        assert np.abs(model.store[name].cpu().numpy() - p_ref).max() < 1e-5, name


@pytest.mark.parametrize('lst,kind', [((False, True, False), 'drop'), ((True, False, True), 'concat')])
def test_subsampled_ctc_trains_and_bf16_tracks_fp32(cuda, lst, kind):
    """As test_ctc_model_train_decreases_loss_and_bf16_close of the plain model: overfit one batch in both dtypes."""
    rng = np.random.RandomState(0)
    B, T, D, H, L, C = 16, 51, 24, 64, 3, 20
    x, sl, labs, dense = _batch(rng, B, T, D, C, sum(lst))
    losses = {}
    for dtype in ('f32', 'bf16'):
        model = _ctc('blstm', D, H, L, C, lst, kind, dtype=dtype, seed=1)
        cur = []
        for step in range(30):
            loss, logits = model.compute_loss(x, dense, sl, keep_prob=1.0)
            model.train(loss, 'adam', 1e-3)
            cur.append(loss.item())
        losses[dtype] = cur
        print(dtype, 'first %.4f last %.4f' % (cur[0], cur[-1]))
        assert cur[-1] < 0.7 * cur[0], cur
    assert abs(losses['bf16'][0] - losses['f32'][0]) / losses['f32'][0] < 2e-2


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_subsampled_ctc_dropout_runs_and_masks(cuda, dtype):
    rng = np.random.RandomState(0)
    B, T, D, H, L, C = 16, 21, 12, 64, 3, 10
    lst = (False, True, False)
    x, sl, labs, dense = _batch(rng, B, T, D, C, 1)
    model = _ctc('blstm', D, H, L, C, lst, 'drop', dtype=dtype, seed=1)
    l1, _ = model.compute_loss(x, dense, sl, keep_prob=1.0)
    l2, _ = model.compute_loss(x, dense, sl, keep_prob=0.8)
    model._set_optimizer('sgd', 0.1).compute_gradients(l2, model=model)     # the backward pass through the masks
    l3, _ = model.compute_loss(x, dense, sl, keep_prob=0.8)
    l4, _ = model.compute_loss(x, dense, sl, keep_prob=0.8, is_training=False)
    assert all(np.isfinite(v.item()) for v in (l1, l2, l3, l4))
    assert abs(l1.item() - l2.item()) > 1e-4 and abs(l2.item() - l3.item()) > 1e-6
    assert abs(l4.item() - l1.item()) < 1e-6 * abs(l1.item())


def test_subsampled_ctc_step_is_deterministic(cuda):
    enc, B, T, D, H, L, C, lst, kind = CTC_CASES[1]
    x, sl, labs, dense = _batch(np.random.RandomState(1), B, T, D, C, sum(lst))
    runs = []
    for _ in range(2):
        model = _ctc(enc, D, H, L, C, lst, kind, dtype='bf16', seed=7)
        loss, _ = model.compute_loss(x, dense, sl, keep_prob=0.9)
        opt = model._set_optimizer('sgd', 0.1)
        gv = opt.compute_gradients(loss, model=model)
        runs.append((loss.cpu().numpy().copy(), {n: g.cpu().numpy().copy() for g, n in gv}))
    assert runs[0][0].tobytes() == runs[1][0].tobytes()
    for n, g in runs[0][1].items():
        assert g.tobytes() == runs[1][1][n].tobytes(), n


def test_zero_frame_utterance_and_bad_lists_raise(cuda):
    x, sl, labs, dense = _batch(np.random.RandomState(2), 5, 23, 12, 10, 2)
    model = _ctc('blstm', 12, 64, 3, 10, (True, False, True), 'concat')
    sl = sl.copy()
    sl[3] = 3                                               # 3 >> 2 == 0
    with pytest.raises(ValueError):
        model.compute_loss(x, dense, sl, keep_prob=1.0)
    with pytest.raises(ValueError):
        _ctc('blstm', 12, 64, 3, 10, (True, False), 'drop')
    with pytest.raises(ValueError):
        _ctc('blstm', 12, 64, 3, 10, (True, False, False), 'max')


# ---------------------------------------------------------------- the joint CTC / attention model
def _att_batch(rng, B, T, D, C, k):
    x = rng.randn(B, T, D).astype(np.float32)
    sl = rng.randint(max(2 << k, T // 2), T + 1, size=B).astype(np.int32)
    sl[0] = T
    lens = np.array([max(1, min(5, (int(s) >> k) // 2)) for s in sl])
    sos, eos = C, C + 1
    labels = np.full((B, int(lens.max()) + 2), eos, dtype=np.int64)
    ctc_labels = np.full((B, int(lens.max())), -1, dtype=np.int64)
    for b in range(B):
        x[b, sl[b]:] = 0
        y = rng.randint(0, C, size=lens[b])
        labels[b, 0] = sos
        labels[b, 1:1 + lens[b]] = y
        ctc_labels[b, :lens[b]] = y
    return x, sl, labels, lens + 2, ctc_labels


def test_subsampled_joint_ctc_attention_parity_and_decoding(cuda, monkeypatch):
    from tensorflow_end2end_speech_recognition_amd.models.attention.joint_ctc_attention import JointCTCAttention
    from tensorflow_end2end_speech_recognition_amd.utils.io.labels.sparsetensor import list2sparsetensor
    B, T, D, H, L, U, A, Em, C = 4, 21, 12, 64, 2, 64, 32, 8, 7
    lst, kind, att = (True, False), 'drop', 'location'
    x, sl, labels, lsl, ctc_labels = _att_batch(np.random.RandomState(3), B, T, D, C, 1)
    model = JointCTCAttention(
        input_size=D, encoder_type='blstm', encoder_num_units=H, encoder_num_layers=L, encoder_num_proj=None,
        attention_type=att, attention_dim=A, decoder_type='lstm', decoder_num_units=U, decoder_num_layers=1,
        embedding_dim=Em, lambda_weight=0.5, num_classes=C, sos_index=C, eos_index=C + 1, max_decode_length=12,
        parameter_init=0.1, clip_grad_norm=5.0, clip_activation_encoder=50, clip_activation_decoder=50, dtype='f32',
        seed=5, subsample_list=list(lst), subsample_type=kind)
    sd = {n: v.cpu().numpy() for n, v in model.store.state_dict().items()}
    sl_out = model.output_seq_len(sl)
    assert np.array_equal(sl_out, sl >> 1)
    sub.patch_oracle_blstm_encoder(monkeypatch, sl, lst, kind)
    ctc_list = [[int(v) for v in row if v >= 0] for row in ctc_labels]
    ref = oatt.attention_model_forward(sd, x, labels, sl_out, lsl, L, att, clip_enc=50.0, clip_dec=50.0,
                                       ctc_labels=ctc_list, lambda_weight=0.5)
    loss, logits, ctc_logits, otr, oinf = model.compute_loss(x, labels, list2sparsetensor(ctc_labels, -1), sl, lsl,
                                                             1.0, 1.0, 1.0)
    assert ctc_logits.shape == (T // 2, B, C + 1) and otr.attention_weights.shape[2] == T // 2
    assert abs(loss.item() - ref['total_loss']) / abs(ref['total_loss']) < 1e-4
    assert np.abs(otr.attention_weights.cpu().numpy() - ref['alphas']).max() < 1e-5
    assert np.abs(ctc_logits.cpu().numpy() - ref['ctc_logits']).max() < 1e-4
    assert np.abs(model.ctc_losses.cpu().numpy() - ref['ctc_losses']).max() / ref['ctc_losses'].max() < 1e-4
    opt = model._set_optimizer('adam', 1e-3)
    for g, name in opt.compute_gradients(loss, model=model):
        r = ref['grads'][name]
        err = np.abs(g.cpu().numpy() - r).max()
        assert err < 2e-3 * max(np.abs(r).max(), 1e-3) + 1e-7, (name, err, np.abs(r).max())
    ref_ids = oatt.attention_model_infer(sd, x, sl_out, L, att, C, C + 1, 12, clip_enc=50.0, clip_dec=50.0)
    assert np.array_equal(model.infer(x, sl), ref_ids)
    # joint beam search (a head sharpened as a trained one is: the statement's margins are then far above the bound):
    # what the native loop is handed is the reduced encoder output and the reduced lengths, and every hypothesis equals
    # the float64 statement over the patched oracle encoder with the reduced lengths
    import _att_joint_oracle as jo
    from tensorflow_end2end_speech_recognition_amd import ops
    sd2 = {n: v.copy() for n, v in sd.items()}
    sd2['attention_decoder/decoder/output_layer/biases'][C + 1] = -0.3
    sd2['attention_decoder/decoder/output_layer/weights'] *= 3.0
    sd2['ctc_output/biases'][C] = 5.0
    model.store.load_state_dict({n: torch.tensor(v) for n, v in sd2.items()})
    want = jo.joint_beam_infer(sd2, x, sl_out, L, att, C, C + 1, 12, 3, 0.3, 0.0, clip_enc=50.0, clip_dec=50.0)
    assert all(r['margin'] >= 1e-3 for r in want), [r['margin'] for r in want]
    handed = {}
    native = ops.att_decoder_beam_joint

    def spy(loop, *a, **k):
        handed.update(T=loop['T'], enc=tuple(loop['enc'].shape), att_len=loop['seq_len'].cpu().numpy(),
                      y=tuple(k['y'].shape), ctc_len=k['seq_len'].cpu().numpy())
        return native(loop, *a, **k)
    monkeypatch.setattr(ops, 'att_decoder_beam_joint', spy)
    hyp = model.infer(x, sl, beam_width=3, ctc_weight=0.3)
    assert handed['T'] == T // 2 and handed['enc'] == (T // 2, B * 3, 2 * H) and handed['y'][0] == T // 2
    assert handed['y'][2] == C + 1
    assert np.array_equal(handed['att_len'], np.repeat(sl >> 1, 3)) and np.array_equal(handed['ctc_len'], sl >> 1)
    raw = model._beam_raw
    assert raw['ids'].shape[:2] == (B, 3)
    for b, r in enumerate(want):
        for w in range(3):
            n = int(raw['hyp_len'][b, w])
            assert raw['ids'][b, w, :n].tolist() == r['ids'][w], (b, w)
        assert np.abs(raw['scores'][b] - r['scores']).max() < 1e-3
        assert np.abs(raw['ctc_score'][b] - r['ctc_score']).max() < 1e-3
        assert hyp[b, :len(r['ids'][0])].tolist() == r['ids'][0]
