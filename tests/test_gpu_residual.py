"""GPU: skip connections between recurrent layers (encoder_residual / encoder_dense_residual) -- the two kernels against
the numpy statement with exact equality at its rounding points, and the CTC / joint CTC-attention models over the residual
encoders against the float64 statement composed from the oracle's layers (tests/_cpu_ops_residual.py) at the bars of the
plain and subsampled models' parity tests (tests/test_gpu_model.py, tests/test_gpu_subsample.py)."""
import numpy as np
import pytest
import torch

import _cpu_ops_residual as res
from oracle import attention as oatt
from oracle import ctc as octc
from oracle import decoders as odec
from oracle import lstm as olstm
from oracle import optim as oopt

pytestmark = pytest.mark.gpu

MODES = res.MODES
KW = {'residual': dict(encoder_residual=True), 'dense': dict(encoder_dense_residual=True)}
T_, BP = 9, 16
LENS = np.array([9, 8, 1, 2, 5, 0] + [0] * 10, dtype=np.int32)
# keep = 1 (no dropout); keep = 0.8 at a counter offset of a fourth call's third layer (64-bit arithmetic) and at 0
DROPS = [(1.0, 0), (0.8, (3 << 40) + (2 << 32)), (0.8, 0)]
SEED = 12345
NAN = float('nan')


def _tensor(rng, W, bf16):
    """([T,Bp,W] device tensor with NaN in every padded frame, the float32 values the kernel loads)."""
    t = torch.tensor(rng.randn(T_, BP, W).astype(np.float32))
    if bf16:
        t = t.to(torch.bfloat16)
    seen = t.float().numpy().copy()
    for b in range(BP):
        t[int(LENS[b]):, b] = NAN
    return t.cuda().contiguous(), seen


def _multipliers(ops, W, keep, offset):
    if keep >= 1.0:
        return None, None
    m = ops.dropout_mask((T_, BP, W), keep, SEED, offset, 'cuda').cpu().numpy()
    assert set(np.unique(m)) <= {0.0, np.float32(1.0 / keep)} and 0 < (m == 0).mean() < 0.5
    return m, (keep, SEED, offset)


# ---------------------------------------------------------------- the forward kernel
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('case', ['op_skip', 'op_skip_sum', 'f32_skip_inplace', 'f32_skip'])
# 128: 16-byte groups everywhere; 20: 16-byte groups for fp32 (20 % 4 == 0), one element per lane for bf16 (20 % 8 != 0);
# 18: one element per lane everywhere
@pytest.mark.parametrize('W', [128, 20, 18])
@pytest.mark.parametrize('keep,offset', DROPS)
def test_residual_fwd_is_the_statement_and_reads_no_padded_frame(cuda, dtype, case, W, keep, offset):
    from tensorflow_end2end_speech_recognition_amd import ops
    rng = np.random.RandomState(W + len(case))
    bf16 = dtype == 'bf16'
    h, h_seen = _tensor(rng, W, bf16)
    skip, skip_seen = _tensor(rng, W, bf16 and case.startswith('op'))
    lens = torch.tensor(LENS).cuda()
    m, drop = _multipliers(ops, W, keep, offset)
    want_o, want_s = res.residual_fwd_np(h_seen, skip_seen, LENS, m, bf16=bf16)
    out0 = torch.full((T_, BP, W), NAN, dtype=h.dtype, device='cuda')      # every element has to be written
    s = None
    if case == 'op_skip_sum':
        s0 = torch.full((T_, BP, W), NAN, device='cuda')
        out, s = ops.residual_fwd(h, skip, lens, drop, sum_out=s0, out=out0)
        assert s is s0
    elif case == 'f32_skip_inplace':
        out, s = ops.residual_fwd(h, skip, lens, drop, sum_out=skip, out=out0)
        assert s is skip
    else:
        out = ops.residual_fwd(h, skip, lens, drop, out=out0)
    assert out is out0 and out.dtype == h.dtype
    o = out.float().cpu().numpy()
    assert np.isfinite(o).all()
    for b in range(BP):
        assert not o[int(LENS[b]):, b].any()
    assert np.array_equal(o, want_o)
    if s is not None:
        sv = s.cpu().numpy()
        assert s.dtype == torch.float32 and np.isfinite(sv).all()
        for b in range(BP):
            assert not sv[int(LENS[b]):, b].any()
        assert np.array_equal(sv, want_s)
    if case == 'op_skip_sum' and keep == 1.0:
        out2, s2 = ops.residual_fwd(h, skip, lens, None, sum_out=True)      # a new sum tensor, a new out
        assert np.array_equal(out2.float().cpu().numpy(), want_o) and np.array_equal(s2.cpu().numpy(), want_s)


# ---------------------------------------------------------------- the backward kernel
@pytest.mark.parametrize('dense', [False, True])
@pytest.mark.parametrize('aliased', [False, True])
@pytest.mark.parametrize('W', [128, 20, 18])
@pytest.mark.parametrize('keep,offset', DROPS)
def test_residual_bwd_is_the_statement_and_reads_no_padded_frame(cuda, dense, aliased, W, keep, offset):
    from tensorflow_end2end_speech_recognition_amd import ops
    rng = np.random.RandomState(W + 7)
    dx, dx_seen = _tensor(rng, W, False)
    carry, carry_seen = _tensor(rng, W, False)
    lens = torch.tensor(LENS).cuda()
    m, drop = _multipliers(ops, W, keep, offset)
    want_d, want_c = res.residual_bwd_np(dx_seen, carry_seen, LENS, m, dense)
    if aliased:
        d, c = ops.residual_bwd(dx, carry, lens, drop, dense, dout=dx, carry_out=carry)
        assert d is dx and c is carry
    else:
        d0, c0 = torch.full((T_, BP, W), NAN, device='cuda'), torch.full((T_, BP, W), NAN, device='cuda')
        d, c = ops.residual_bwd(dx, carry, lens, drop, dense, dout=d0, carry_out=c0)
        assert d is d0 and c is c0
        d1, c1 = ops.residual_bwd(dx, carry, lens, drop, dense)             # new tensors
        assert torch.equal(d1, d) and torch.equal(c1, c)
    d, c = d.cpu().numpy(), c.cpu().numpy()
    assert np.isfinite(d).all() and np.isfinite(c).all()
    for b in range(BP):
        assert not d[int(LENS[b]):, b].any() and not c[int(LENS[b]):, b].any()
    assert np.array_equal(d, want_d) and np.array_equal(c, want_c)


@pytest.mark.parametrize('W', [128, 20, 18])
def test_residual_kernels_are_a_transpose_pair(cuda, W):
    """F: (h, skip) -> out = m h + skip and its transpose dy -> (m dy, dy), which is the backward kernel with dx_raw = 0
    and carry = dy: <F(h, skip), dy> = <h, dout> + <skip, carry_out> at keep = 0.8.  The inputs are multiples of 2^-6
    below 4 in magnitude and m is 0 or 1.25 (1.f / 0.8f rounds to 1.25): every product and sum the kernels form is exact
    in fp32, so the two sides differ only by the float64 summation here -- 1e-9 relative is a loose bar for that."""
    from tensorflow_end2end_speech_recognition_amd import ops
    rng = np.random.RandomState(W)
    grid = lambda: (rng.randint(-255, 256, size=(T_, BP, W)) / 64.0).astype(np.float32)
    h, skip, dy = grid(), grid(), grid()
    lens = torch.tensor(LENS).cuda()
    drop = (0.8, SEED, (3 << 40) + (2 << 32))
    out = ops.residual_fwd(torch.tensor(h).cuda(), torch.tensor(skip).cuda(), lens, drop).cpu().numpy().astype(np.float64)
    dout, cout = ops.residual_bwd(torch.zeros((T_, BP, W), device='cuda'), torch.tensor(dy).cuda(), lens, drop, False)
    lhs = float((out * dy).sum())
    rhs = float((h.astype(np.float64) * dout.cpu().numpy()).sum() + (skip.astype(np.float64) * cout.cpu().numpy()).sum())
    assert abs(lhs) > 1.0 and abs(lhs - rhs) < 1e-9 * abs(lhs)


def test_residual_ops_refuse_what_they_cannot_run(cuda):
    from tensorflow_end2end_speech_recognition_amd import ops
    x = torch.zeros((4, 16, 8), device='cuda')
    sl = torch.full((16,), 4, dtype=torch.int32, device='cuda')
    with pytest.raises(ValueError):
        ops.residual_fwd(x, x.double(), sl)                                  # skip: the operand dtype or fp32
    with pytest.raises(ValueError):
        ops.residual_fwd(x, x.to(torch.bfloat16), sl)
    with pytest.raises(ValueError):
        ops.residual_fwd(x.to(torch.float16), x, sl)
    with pytest.raises(ValueError):
        ops.residual_fwd(x, x[:3].contiguous(), sl)
    with pytest.raises(ValueError):
        ops.residual_fwd(x, x, sl[:15].contiguous())
    with pytest.raises(ValueError):
        ops.residual_fwd(x, x, sl.long())
    with pytest.raises(ValueError):
        ops.residual_fwd(x, x, sl, sum_out=x.to(torch.bfloat16))
    with pytest.raises(ValueError):
        ops.residual_fwd(x, x, sl, (0.0, 1, 0))
    with pytest.raises(RuntimeError):
        ops.residual_fwd(x.cpu(), x.cpu(), sl.cpu())
    with pytest.raises(ValueError):
        ops.residual_fwd(x, x.clone(), sl, out=x)                            # out over an input: the library says no
    with pytest.raises(ValueError):
        ops.residual_bwd(x.to(torch.bfloat16), x, sl)
    with pytest.raises(ValueError):
        ops.residual_bwd(x, x[:, :8].contiguous(), sl)
    with pytest.raises(ValueError):
        ops.residual_bwd(x, x, sl, dout=x[:2].contiguous())
    with pytest.raises(RuntimeError):
        ops.residual_bwd(x.cpu(), x.cpu(), sl.cpu())
    with pytest.raises(ValueError):
        ops.residual_bwd(x, x.clone(), sl, dout=x, carry_out=x)              # the two outputs over each other
    # T = 0: nothing to do, nothing launched
    e = x[:0].contiguous()
    assert ops.residual_fwd(e, e, sl).shape == (0, 16, 8)
    d, c = ops.residual_bwd(e, e, sl)
    assert d.shape == (0, 16, 8) and c.shape == (0, 16, 8)


# ---------------------------------------------------------------- the CTC model
def _batch(rng, B, T, D, C):
    """Odd T and ragged lengths; labels of max(1, len // 2) symbols stay feasible even if every symbol repeats."""
    x = rng.randn(B, T, D).astype(np.float32)
    sl = rng.randint(max(2, T // 2), T + 1, size=B).astype(np.int32)
    sl[0] = T
    labs = []
    for b in range(B):
        x[b, sl[b]:] = 0
        labs.append([int(v) for v in rng.randint(0, C, size=max(1, int(sl[b]) // 2))])
    dense = np.full((B, max(len(l) for l in labs)), -1, dtype=np.int64)
    for b, l in enumerate(labs):
        dense[b, :len(l)] = l
    return x, sl, labs, dense


CTC_CASES = [('blstm', 5, 23, 12, 64, 3, 10), ('lstm', 16, 30, 24, 64, 4, 20)]


def _ctc(enc, D, H, L, C, mode, **kw):
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    kw.setdefault('dtype', 'f32')
    kw.setdefault('seed', 3)
    kw.update(KW[mode] if mode else {})
    return CTC(encoder_type=enc, input_size=D, num_units=H, num_layers=L, num_classes=C, parameter_init=0.1,
               clip_grad_norm=5.0, clip_activation=50, device='cuda:0', **kw)


@pytest.mark.parametrize('keep', [1.0, 0.8])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('enc,B,T,D,H,L,C', CTC_CASES)
def test_residual_ctc_model_loss_grads_step_and_decoders(cuda, enc, B, T, D, H, L, C, mode, keep):
    """keep = 0.8: the statement is fed the device's own masks -- the case that catches a mask applied to the skip path, or
    a carry that was masked."""
    from tensorflow_end2end_speech_recognition_amd import ops
    from tensorflow_end2end_speech_recognition_amd.models.encoders.core.residual import load_residual
    from tensorflow_end2end_speech_recognition_amd.utils.io.labels.sparsetensor import list2sparsetensor, sparsetensor2list
    rng = np.random.RandomState(B + T)
    ndir = 2 if enc == 'blstm' else 1
    x, sl, labs, dense = _batch(rng, B, T, D, C)
    model = _ctc(enc, D, H, L, C, mode, weight_decay=1e-4)
    assert type(model.encoder) is load_residual(enc)
    sd = {n: v.cpu().numpy() for n, v in model.store.state_dict().items()}
    masks = None
    if keep < 1.0:      # first call with dropout of a model with seed 3: calls = 1
        Bp = B + (-B) % 16
        masks = [ops.dropout_mask((T, Bp, ndir * H), keep, 3, (1 << 40) + (li << 32), 'cuda').cpu().numpy()[:, :B]
                 for li in range(L)]
    ref = res.ctc_model_forward(sd, x, labs, sl, L, ndir, mode, cell_clip=50.0, weight_decay=1e-4, masks=masks)
    loss, logits = model.compute_loss(x, list2sparsetensor(dense, -1), sl, keep_prob=keep)
    assert logits.shape == (T, B, C + 1)
    rel_loss = abs(loss.item() - ref['total_loss']) / abs(ref['total_loss'])
    rel_utt = np.abs(model.ctc_losses.cpu().numpy() - ref['ctc_losses']).max() / ref['ctc_losses'].max()
    abs_logits = np.abs(logits.cpu().numpy() - ref['logits']).max()
    print('loss rel %.3g  per-utterance rel %.3g  logits abs %.3g' % (rel_loss, rel_utt, abs_logits))
    assert rel_loss < 1e-4
    assert rel_utt < 1e-4
    assert abs_logits < 1e-4
    # greedy and width-4 beam labels: the oracle decoders on the oracle logits
    ref_bm = np.transpose(ref['logits'], (1, 0, 2))
    hyp = sparsetensor2list(model.decoder(logits, sl, beam_width=1), B)
    assert [list(h) for h in hyp] == odec.greedy_decode(ref_bm, sl, C)
    dec_b = model.decoder(logits, sl, beam_width=4, merge_repeated=False)
    ref_b, _ = odec.beam_search_decode(octc.log_softmax(ref_bm), sl, C, 4)
    assert [list(h) for h in sparsetensor2list(dec_b, B)] == ref_b
    # gradients (before clipping), then clip + one momentum step
    opt = model._set_optimizer('momentum', 0.01)
    gv = opt.compute_gradients(loss, model=model)
    assert sorted(n for _, n in gv) == sorted(ref['grads'])
    worst = 0.0
    for g, name in gv:
        r = ref['grads'][name]
        rel = np.abs(g.cpu().numpy() - r).max() / max(np.abs(r).max(), 1e-8)
        worst = max(worst, rel)
        assert rel < 2e-3, (name, rel)
    print('worst gradient rel %.3g' % worst)
    model._clip_gradients(gv)
    opt.apply_gradients(gv)
    for name in model.store.names:
        p_ref = sd[name].astype(np.float64) - 0.01 * oopt.clip_by_norm(ref['grads'][name], 5.0)
        assert np.abs(model.store[name].cpu().numpy() - p_ref).max() < 1e-5, name


@pytest.mark.parametrize('mode', MODES)
def test_residual_ctc_trains_and_bf16_tracks_fp32(cuda, mode):
    """As test_subsampled_ctc_trains_and_bf16_tracks_fp32: overfit one batch in both dtypes."""
    rng = np.random.RandomState(0)
    B, T, D, H, L, C = 16, 51, 24, 64, 3, 20
    x, sl, labs, dense = _batch(rng, B, T, D, C)
    losses = {}
    for dtype in ('f32', 'bf16'):
        model = _ctc('blstm', D, H, L, C, mode, dtype=dtype, seed=1)
        cur = []
        for step in range(30):
            loss, logits = model.compute_loss(x, dense, sl, keep_prob=1.0)
            model.train(loss, 'adam', 1e-3)
            cur.append(loss.item())
        losses[dtype] = cur
        print(dtype, 'first %.4f last %.4f' % (cur[0], cur[-1]))
        assert cur[-1] < 0.7 * cur[0], cur
    assert abs(losses['bf16'][0] - losses['f32'][0]) / losses['f32'][0] < 2e-2


@pytest.mark.parametrize('mode', MODES)
def test_residual_ctc_bf16_against_the_statement_with_rounded_operands(cuda, mode):
    """The statement with the device path's rounding points (operand_round: inputs, kernels, output weights, every
    emitted h, every o_l once; S in fp32) at the bars test_gpu_model.py holds a bf16 model to against such a statement:
    loss 2e-3 relative, logits 3e-2 of max(1, max |logit|), gradients 3e-2 of their maximum."""
    enc, B, T, D, H, L, C = 'blstm', 5, 23, 12, 64, 4, 10
    rng = np.random.RandomState(2)
    x, sl, labs, dense = _batch(rng, B, T, D, C)
    model = _ctc(enc, D, H, L, C, mode, dtype='bf16')
    sd = {n: v.cpu().numpy() for n, v in model.store.state_dict().items()}
    for k in sd:
        if k.endswith('/bias') or k.endswith('/biases'):
            sd[k] = (rng.randn(*sd[k].shape) * 0.05).astype(np.float32)
    model.store.load_state_dict({k: torch.tensor(v) for k, v in sd.items()})
    ref = res.ctc_model_forward(sd, x, labs, sl, L, 2, mode, cell_clip=50.0, operand_round=olstm.bf16_round_t)
    loss, logits = model.compute_loss(x, dense, sl, keep_prob=1.0)
    rel = abs(loss.item() - ref['total_loss']) / abs(ref['total_loss'])
    valid = (np.arange(T)[:, None] < sl[None, :])
    elog = np.abs(logits.cpu().numpy() - ref['logits'])[valid].max()
    worst = 0.0
    gv = model._set_optimizer('sgd', 0.1).compute_gradients(loss, model=model)
    for g, name in gv:
        r = ref['grads'][name]
        worst = max(worst, np.abs(g.cpu().numpy() - r).max() / max(np.abs(r).max(), 1e-12))
    print('loss rel %.3g  logits abs %.3g (max |logit| %.2f)  worst gradient rel %.3g'
          % (rel, elog, np.abs(ref['logits']).max(), worst))
    assert rel < 2e-3
    assert elog < 3e-2 * max(1.0, np.abs(ref['logits']).max())
    assert worst < 3e-2


@pytest.mark.parametrize('mode', MODES)
def test_residual_ctc_bf16_dropout_step_is_bitwise_repeatable(cuda, mode):
    enc, B, T, D, H, L, C = CTC_CASES[0]
    x, sl, labs, dense = _batch(np.random.RandomState(1), B, T, D, C)
    runs = []
    for _ in range(2):
        model = _ctc(enc, D, H, L, C, mode, dtype='bf16', seed=7)
        loss, _ = model.compute_loss(x, dense, sl, keep_prob=0.8)
        gv = model._set_optimizer('sgd', 0.1).compute_gradients(loss, model=model)
        runs.append((loss.cpu().numpy().copy(), {n: g.cpu().numpy().copy() for g, n in gv}))
    assert np.isfinite(runs[0][0]).all()
    assert runs[0][0].tobytes() == runs[1][0].tobytes()
    for n, g in runs[0][1].items():
        assert np.isfinite(g).all(), n
        assert g.tobytes() == runs[1][1][n].tobytes(), n


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_flags_false_equal_the_plain_model_bit_for_bit(cuda, dtype):
    from tensorflow_end2end_speech_recognition_amd.models.encoders.load_encoder import load
    enc, B, T, D, H, L, C = CTC_CASES[0]
    x, sl, labs, dense = _batch(np.random.RandomState(4), B, T, D, C)
    runs = []
    for kw in ({}, dict(encoder_residual=False, encoder_dense_residual=False)):
        model = _ctc(enc, D, H, L, C, None, dtype=dtype, seed=7, **kw)
        assert type(model.encoder) is load(enc)
        loss, logits = model.compute_loss(x, dense, sl, keep_prob=0.8)
        gv = model._set_optimizer('sgd', 0.1).compute_gradients(loss, model=model)
        runs.append((loss.cpu().numpy().copy(), logits.cpu().numpy().copy(),
                     {n: g.cpu().numpy().copy() for g, n in gv}))
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
    for n, g in runs[0][2].items():
        assert g.tobytes() == runs[1][2][n].tobytes(), n


# ---------------------------------------------------------------- the joint CTC / attention model
def _att_batch(rng, B, T, D, C):
    x = rng.randn(B, T, D).astype(np.float32)
    sl = rng.randint(max(2, T // 2), T + 1, size=B).astype(np.int32)
    sl[0] = T
    lens = np.array([max(1, min(5, int(s) // 2)) for s in sl])
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


def test_residual_joint_ctc_attention_parity_and_greedy_infer(cuda, monkeypatch):
    from tensorflow_end2end_speech_recognition_amd.models.attention.joint_ctc_attention import JointCTCAttention
    from tensorflow_end2end_speech_recognition_amd.models.encoders.core.residual import ResidualBLSTMEncoder
    from tensorflow_end2end_speech_recognition_amd.utils.io.labels.sparsetensor import list2sparsetensor
    B, T, D, H, L, U, A, Em, C = 4, 21, 12, 64, 3, 64, 32, 8, 7
    att = 'location'
    x, sl, labels, lsl, ctc_labels = _att_batch(np.random.RandomState(3), B, T, D, C)
    model = JointCTCAttention(
        input_size=D, encoder_type='blstm', encoder_num_units=H, encoder_num_layers=L, encoder_num_proj=None,
        attention_type=att, attention_dim=A, decoder_type='lstm', decoder_num_units=U, decoder_num_layers=1,
        embedding_dim=Em, lambda_weight=0.5, num_classes=C, sos_index=C, eos_index=C + 1, max_decode_length=12,
        parameter_init=0.1, clip_grad_norm=5.0, clip_activation_encoder=50, clip_activation_decoder=50, dtype='f32',
        seed=5, encoder_residual=True)
    assert type(model.encoder) is ResidualBLSTMEncoder and not model.encoder.dense
    sd = {n: v.cpu().numpy() for n, v in model.store.state_dict().items()}
    res.patch_oracle_blstm_encoder(monkeypatch, 'residual')
    ctc_list = [[int(v) for v in row if v >= 0] for row in ctc_labels]
    ref = oatt.attention_model_forward(sd, x, labels, sl, lsl, L, att, clip_enc=50.0, clip_dec=50.0,
                                       ctc_labels=ctc_list, lambda_weight=0.5)
    loss, logits, ctc_logits, otr, oinf = model.compute_loss(x, labels, list2sparsetensor(ctc_labels, -1), sl, lsl,
                                                             1.0, 1.0, 1.0)
    assert ctc_logits.shape == (T, B, C + 1)
    assert abs(loss.item() - ref['total_loss']) / abs(ref['total_loss']) < 1e-4
    assert np.abs(otr.attention_weights.cpu().numpy() - ref['alphas']).max() < 1e-5
    assert np.abs(ctc_logits.cpu().numpy() - ref['ctc_logits']).max() < 1e-4
    assert np.abs(model.ctc_losses.cpu().numpy() - ref['ctc_losses']).max() / ref['ctc_losses'].max() < 1e-4
    opt = model._set_optimizer('adam', 1e-3)
    for g, name in opt.compute_gradients(loss, model=model):
        r = ref['grads'][name]
        err = np.abs(g.cpu().numpy() - r).max()
        assert err < 2e-3 * max(np.abs(r).max(), 1e-3) + 1e-7, (name, err, np.abs(r).max())
    ref_ids = oatt.attention_model_infer(sd, x, sl, L, att, C, C + 1, 12, clip_enc=50.0, clip_dec=50.0)
    assert np.array_equal(model.infer(x, sl), ref_ids)
