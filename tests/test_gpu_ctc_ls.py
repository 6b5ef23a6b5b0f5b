"""GPU: label smoothing for the CTC heads.  ops.ctc_loss_ls (asr_ctc_loss_ls) against the float64 statement of
tests/_ctc_ls_oracle.py at the project's CTC bars, its bit-level contracts (the loss is ctc_loss's, padding is never read,
the image is the cast of the gradient, the fused head continues from ctc_head_fwd's workspace, two calls give the same
bits), and CTC / MultitaskCTC / JointCTCAttention with the keyword against the statement composed with the oracle's
model statements, at the bars of their plain twins (tests/test_gpu_model.py, tests/test_gpu_attention.py)."""
import functools

import numpy as np
import pytest
import torch

import _ctc_ls_oracle as ols
from oracle import attention as oatt
from oracle import ctc as octc
from oracle import lstm as olstm
from oracle import model as omodel
from oracle import optim as oopt
from tensorflow_end2end_speech_recognition_amd._lib import ASR_BF16

pytestmark = pytest.mark.gpu

EPS = 0.2
CASES = [(12, 5, 7, 7), (40, 3, 62, 12), (40, 3, 300, 12), (40, 3, 3387, 12), (700, 2, 29, 200)]


def _ops():
    from tensorflow_end2end_speech_recognition_amd import ops
    return ops


def _flat(labs):
    flat = np.asarray(sum(labs, []) or [0], dtype=np.int32)
    off = np.zeros(len(labs) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(l) for l in labs])
    return flat, off


@functools.lru_cache(maxsize=None)
def _case(T, B, C, lmax):
    """(logits, seq_len, labels, the statement's pieces) of one case, computed once and left unchanged.  (12, 5, 7, 7): the
    lengths and labels of test_ctc_edge_cases; the others as test_ctc_loss_and_grad draws them, with an adjacent and a
    non-adjacent repeat forced and, at lmax = 200, one utterance that really has 200 labels (the multi-wave recursion)."""
    if (T, B, C) == (12, 5, 7):
        rng = np.random.RandomState(0)
        logits = rng.randn(T, B, C).astype(np.float32)
        sl = np.array([12, 5, 3, 0, 7], dtype=np.int32)
        labs = [[], [1, 1, 1], [2, 2, 2], [3], [0, 1, 2, 3, 4, 5, 0]]
    else:
        rng = np.random.RandomState(T + C)
        logits = (rng.randn(T, B, C) * 2.0).astype(np.float32)
        sl = rng.randint(max(1, T // 3), T + 1, size=B).astype(np.int32)
        sl[0] = T
        labs = []
        for b in range(B):
            L = rng.randint(3, min(lmax, sl[b] // 2) + 1)
            labs.append([int(v) for v in rng.randint(0, C - 1, size=L)])
        labs[0] = labs[0][:2] + labs[0][:2]                                     # an adjacent-free repeat pattern a b a b
        labs[1][1] = labs[1][0]                                                 # an adjacent repeat
        if lmax >= 200:
            labs[0] = [int(v) for v in rng.randint(0, C - 1, size=lmax)]
        labs[-1][2] = labs[-1][0]                                               # a non-adjacent repeat of a class
    x = logits.astype(np.float64)
    ctc, g_ctc = octc.ctc_loss_batch(x, labs, sl)
    kl, g_kl = ols.kl_uniform(x, labs, sl)
    ninf = sum(1 for b in range(B) if min(int(sl[b]), T) > 0 and not ols.feasible(labs[b], min(int(sl[b]), T)))
    for a in (logits, sl, ctc, g_ctc, kl, g_kl):
        a.setflags(write=False)
    return logits, sl, labs, dict(ctc=ctc, g_ctc=g_ctc, kl=kl, g_kl=g_kl, ninf=ninf)


def _dev_args(cuda, T, B, C, lmax):
    logits, sl, labs, ref = _case(T, B, C, lmax)
    flat, off = _flat(labs)
    return (torch.tensor(logits, device=cuda), torch.tensor(flat, device=cuda), torch.tensor(off, device=cuda),
            torch.tensor(sl, device=cuda), max(len(l) for l in labs)), ref


def _bits(t):
    return t.cpu().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).numpy()


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------- the op
@pytest.mark.parametrize('scale', [1.0, 1.0 / 3.0])
@pytest.mark.parametrize('eps', [0.1, 0.5])
@pytest.mark.parametrize('T,B,C,lmax', CASES)
def test_op_against_the_float64_statement(cuda, T, B, C, lmax, eps, scale):
    """The project's CTC bars (test_ctc_loss_and_grad): loss and kl 1e-5 of max(value, 1), grad 2e-5 * grad_scale -- the
    smoothed gradient is a convex combination of two terms that each meet the bar."""
    ops = _ops()
    args, ref = _dev_args(cuda, T, B, C, lmax)
    loss, kl, grad, img, ninf = ops.ctc_loss_ls(*args, eps, grad_scale=scale)
    assert img is None
    loss, kl, grad = loss.cpu().numpy(), kl.cpu().numpy(), grad.cpu().numpy()
    want_g = scale * ((1.0 - eps) * ref['g_ctc'] + eps * ref['g_kl'])
    e_loss = np.abs(loss - ref['ctc']).max() / max(ref['ctc'].max(), 1)
    e_kl = np.abs(kl - ref['kl']).max() / max(ref['kl'].max(), 1)
    e_grad = np.abs(grad - want_g).max()
    print('loss %.3g  kl %.3g  grad %.3g (bar %.3g)' % (e_loss, e_kl, e_grad, 2e-5 * scale))
    assert e_loss < 1e-5
    assert e_kl < 1e-5
    assert e_grad < 2e-5 * scale
    assert int(ninf.item()) == ref['ninf']
    if (T, B, C) == (12, 5, 7):
        assert ref['ninf'] == 1
        for b in (2, 3):                                  # infeasible; seq_len 0
            assert loss[b] == 0 and kl[b] == 0 and not grad[:, b].any()
        assert kl[0] > 0 and loss[0] > 0                  # the empty label row is smoothed like any other
    # want_grad=False still produces kl, with the same bits (the row kernel sums in the gradient kernel's order)
    l2, k2, g2, i2, n2 = ops.ctc_loss_ls(*args, eps, grad_scale=scale, want_grad=False)
    assert g2 is None and i2 is None and int(n2.item()) == ref['ninf']
    assert np.array_equal(l2.cpu().numpy().view(np.uint32), loss.view(np.uint32))
    assert np.array_equal(k2.cpu().numpy().view(np.uint32), kl.view(np.uint32))


@pytest.mark.parametrize('T,B,C,lmax', CASES)
def test_loss_is_bit_identical_to_ctc_loss_and_two_calls_agree(cuda, T, B, C, lmax):
    ops = _ops()
    args, ref = _dev_args(cuda, T, B, C, lmax)
    plain, _, n0 = ops.ctc_loss(*args, grad_scale=1.0)
    for eps in (0.1, 0.5):
        a = ops.ctc_loss_ls(*args, eps, grad_scale=0.25, want_image=True)
        b = ops.ctc_loss_ls(*args, eps, grad_scale=0.25, want_image=True)
        assert _same_bits(a[0], plain) and int(a[4].item()) == int(n0.item())
        for u, v in zip(a, b):                            # determinism: loss, kl, grad, image, ninf
            assert _same_bits(u, v)
    # eps -> the gradient really depends on it
    g1 = ops.ctc_loss_ls(*args, 0.1)[2]
    g5 = ops.ctc_loss_ls(*args, 0.5)[2]
    assert not torch.equal(g1, g5)


def _raw_call(ops, cuda, logits, flat, off, sl, lmax, eps, scale, fill):
    """asr_ctc_loss_ls through the C ABI on outputs prefilled with `fill`."""
    T, B, C = logits.shape
    h = ops._h(logits)
    Kp = (C + 63) // 64 * 64
    ws = ops.ctc_ls_workspace(T, B, lmax, cuda)
    loss = torch.full((B,), fill, dtype=torch.float32, device=cuda)
    kl = torch.full((B,), fill, dtype=torch.float32, device=cuda)
    grad = torch.full((T, B, C), fill, dtype=torch.float32, device=cuda)
    img = torch.full((T * B, Kp), fill, dtype=torch.bfloat16, device=cuda)
    ninf = torch.full((1,), 12345, dtype=torch.int32, device=cuda)
    p, s = ops._p, ops._s
    h.check(h.lib.asr_ctc_loss_ls(h.h, p(logits), T, B, C, p(flat), p(off), p(sl), int(lmax), float(scale), float(eps),
                                  p(loss), p(kl), p(grad), p(ninf), p(ws), ws.numel(), 0, p(img), Kp, s()),
            'asr_ctc_loss_ls')
    return loss, kl, grad, img, ninf


@pytest.mark.parametrize('T,B,C,lmax', [(12, 5, 7, 7), (40, 3, 62, 12), (40, 3, 300, 12)])
def test_padding_is_never_read_and_its_rows_are_zero(cuda, T, B, C, lmax):
    ops = _ops()
    (logits, flat, off, sl, lm), ref = _dev_args(cuda, T, B, C, lmax)
    clean = _raw_call(ops, cuda, logits, flat, off, sl, lm, EPS, 0.5, 0.0)
    dirty_logits = logits.clone()
    lens = sl.cpu().numpy()
    for b in range(B):
        dirty_logits[int(lens[b]):, b] = float('nan')
    dirty = _raw_call(ops, cuda, dirty_logits, flat, off, sl, lm, EPS, 0.5, float('nan'))
    for u, v in zip(clean, dirty):
        assert torch.isfinite(v.float()).all()
        assert _same_bits(u, v)
    grad, img = dirty[2], dirty[3].view(T, B, -1)
    for b in range(B):
        assert not grad[int(lens[b]):, b].any() and not img[int(lens[b]):, b].any()
    assert int(dirty[4].item()) == ref['ninf']


@pytest.mark.parametrize('T,B,C,lmax', CASES)
def test_image_is_the_cast_of_the_gradient(cuda, T, B, C, lmax):
    ops = _ops()
    args, _ = _dev_args(cuda, T, B, C, lmax)
    loss, kl, grad, img, _ = ops.ctc_loss_ls(*args, EPS, grad_scale=1.0 / 3.0, want_image=True)
    Kp = (C + 63) // 64 * 64
    assert img.shape == (T * B, Kp) and img.dtype == torch.bfloat16
    assert _same_bits(img[:, :C].contiguous(), ops.cast_from_f32(grad.view(T * B, C), ASR_BF16))
    assert not img[:, C:].any()
    l2, k2, g2, i2, _ = ops.ctc_loss_ls(*args, EPS, grad_scale=1.0 / 3.0)
    assert i2 is None and _same_bits(g2, grad) and _same_bits(k2, kl) and _same_bits(l2, loss)


def test_argument_checks(cuda):
    ops = _ops()
    args, _ = _dev_args(cuda, 12, 5, 7, 7)
    logits, flat, off, sl, lm = args
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            ops.ctc_loss_ls(*args, bad)
    with pytest.raises(ValueError):
        ops.ctc_loss_ls(*args, EPS, lse_done=True)
    # the C ABI refuses them as well, and a workspace of the plain size
    OK, ERR_INVALID_ARG, ERR_WORKSPACE = 0, -1, -4        # asr_status (include/asr_hip.h)
    h = ops._h(logits)
    p, s = ops._p, ops._s
    T, B, C = logits.shape
    out = [torch.empty((B,), device=cuda), torch.empty((B,), device=cuda), torch.empty((1,), dtype=torch.int32, device=cuda)]
    ws = ops.ctc_ls_workspace(T, B, lm, cuda)
    small = ops.ctc_workspace(T, B, lm, cuda)
    assert ws.numel() > small.numel()

    def rc(eps, w):
        return h.lib.asr_ctc_loss_ls(h.h, p(logits), T, B, C, p(flat), p(off), p(sl), lm, 1.0, eps, p(out[0]), p(out[1]),
                                     None, p(out[2]), p(w), w.numel(), 0, None, 0, s())
    ops.reset_ctc_ls_counts(0)
    for bad in (0.0, 1.0, -0.5, float('nan')):
        assert rc(bad, ws) == ERR_INVALID_ARG
    assert rc(EPS, small) == ERR_WORKSPACE
    assert ops.ctc_ls_counts(0)['calls'] == 1             # refused smoothing values are not counted
    assert rc(EPS, ws) == OK
    assert ops.ctc_ls_counts(0) == dict(calls=2, lse_done=0, no_grad=2)
    ops.reset_ctc_ls_counts(0)
    assert ops.ctc_ls_counts(0) == dict(calls=0, lse_done=0, no_grad=0)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the fused head
BP, NB = 16, 3


def _head_batch(T):
    """test_gpu_ctc_head.py's batch: a repeated label, an infeasible utterance, an empty label row, the batch padding."""
    lens = np.zeros(BP, dtype=np.int32)
    lens[0], lens[1], lens[2] = T, 1, max(1, T // 2)
    labs = [[1, 1, 0], [0, 1], []] + [[] for _ in range(BP - NB)]
    flat = np.array([l for u in labs for l in u], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum([len(u) for u in labs])]).astype(np.int32)
    return lens, flat, off, 3


@pytest.mark.parametrize('keep', [1.0, 0.8])
@pytest.mark.parametrize('T', [13, 70])
def test_fused_head_continues_from_the_forward_launch(cuda, T, keep):
    """E = 128, C = 62, bf16: ctc_head_fwd into a ctc_ls_workspace, then ctc_loss_ls(lse_done=True), against
    ctc_loss_ls(lse_done=False) on the head's own logits -- the same bits in loss, kl, grad and image; and ctc_head_bwd on
    that image against the unfused product (cast, gemm, dropout) on the valid rows, np.array_equal as
    test_gpu_ctc_head.py compares them.  T = 70: 1120 rows, the listed-row lean NT kernel."""
    from tensorflow_end2end_speech_recognition_amd.models.encoders.core import rnn_util
    ops = _ops()
    E, C = 128, 62
    g = torch.Generator(device='cpu').manual_seed(1000 * T + 10 * E + C)
    hout = torch.randn((T, BP, E), generator=g).to(torch.bfloat16).to(cuda)
    W = (torch.randn((E, C), generator=g) * 0.2).to(cuda)
    bias = (torch.randn((C,), generator=g) * 0.5).to(cuda)
    lens_np, flat_np, off_np, lmax = _head_batch(T)
    lens, flat, off = (torch.from_numpy(a).to(cuda) for a in (lens_np, flat_np, off_np))
    drop = (keep, 77, 5 << 20) if keep < 1.0 else None
    rows_np = rnn_util.valid_rows(lens_np, T, BP)
    rows = torch.from_numpy(rows_np).to(cuda)
    scale = 1.0 / NB
    Wt, Wp = ops.ctc_head_prep(W)
    ws = ops.ctc_ls_workspace(T, BP, lmax, cuda)
    ops.reset_ctc_head_counts(0)
    ops.reset_ctc_ls_counts(0)
    x, logits, ninf = ops.ctc_head_fwd(hout, drop, Wt, bias, C, flat, off, lens, lmax, ws)
    fused = ops.ctc_loss_ls(logits, flat, off, lens, lmax, EPS, grad_scale=scale, ws=ws, ninf=ninf, lse_done=True,
                            want_image=True)
    assert ops.ctc_head_counts(0) == dict(head_fwd=1, loss_ex=0, loss=0)
    assert ops.ctc_ls_counts(0) == dict(calls=1, lse_done=1, no_grad=0)
    sep = ops.ctc_loss_ls(logits, flat, off, lens, lmax, EPS, grad_scale=scale, want_image=True)
    for u, v in zip(fused, sep):
        assert _same_bits(u, v)
    assert int(fused[4].item()) == 1 and float(fused[1][1]) == 0.0 and float(fused[1][0]) > 0.0
    # a second continuation from the same workspace: the call leaves what ctc_head_fwd wrote intact
    again = ops.ctc_loss_ls(logits, flat, off, lens, lmax, EPS, grad_scale=scale, ws=ws, ninf=ninf, lse_done=True,
                            want_image=True)
    for u, v in zip(fused, again):
        assert _same_bits(u, v)
    # backward: the image through the head's product against the unfused sequence
    grad, img = fused[2], fused[3]
    Wsh = ops.cast_from_f32(W, ASR_BF16)
    dl_ref = ops.cast_from_f32(grad.view(T * BP, C), ASR_BF16)
    denc_ref = ops.gemm(dl_ref, Wsh, transB=True, out_dtype=torch.float32)
    if drop:
        denc_ref = ops.dropout_apply(denc_ref, *drop)
    denc = torch.full((T * BP, E), float('nan'), dtype=torch.float32, device=cuda)
    ops.ctc_head_bwd(img, Wp, denc, drop=drop, rows=(rows, rows_np.size))
    a, b = denc_ref.cpu().numpy()[rows_np], denc.cpu().numpy()[rows_np]
    assert np.isfinite(b).all() and np.array_equal(a, b)


# ---------------------------------------------------------------- models
def _batch(rng, B, T, D, C):
    x = rng.randn(B, T, D).astype(np.float32)
    sl = np.array([T, T // 2 + 1, T - 5][:B], dtype=np.int32)                  # ragged
    labs = []
    for b in range(B):
        x[b, sl[b]:] = 0
        labs.append([int(v) for v in rng.randint(0, C, size=max(1, sl[b] // 4))])
    dense = np.full((B, max(len(l) for l in labs)), -1, dtype=np.int64)
    for b, l in enumerate(labs):
        dense[b, :len(l)] = l
    return x, sl, labs, dense


def _randomise_biases(model, rng):
    sd = {k: v.cpu().numpy().copy() for k, v in model.store.state_dict().items()}
    for k in sd:
        if k.endswith('/bias') or k.endswith('/biases'):
            sd[k] = (rng.randn(*sd[k].shape) * 0.05).astype(np.float32)
    model.store.load_state_dict({k: torch.tensor(v) for k, v in sd.items()})
    return sd


B_, T_, D_, H_, L_, C_ = 3, 24, 12, 64, 2, 10


def _ctc(dtype, **kw):
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    return CTC(encoder_type='blstm', input_size=D_, num_units=H_, num_layers=L_, num_classes=C_, parameter_init=0.1,
               clip_grad_norm=5.0, clip_activation=50, dtype=dtype, device='cuda:0', seed=3, **kw)


def _momentum_step_fp32(model, gv, opt, sd, ref):
    """clip + first momentum step against the oracle's, test_ctc_model_loss_grads_and_step's bar."""
    model._clip_gradients(gv)
    opt.apply_gradients(gv)
    for name in model.store.names:
        want = sd[name].astype(np.float64) - 0.01 * oopt.clip_by_norm(ref['grads'][name], 5.0)
        assert np.abs(model.store[name].cpu().numpy() - want).max() < 1e-5, name


@pytest.mark.parametrize('temp', [1, 2])
def test_ctc_model_fp32_with_label_smoothing(cuda, temp):
    """CTC blstm fp32 (the separate head launches), softmax_temperature 1 and 2, at test_ctc_model_loss_grads_and_step's
    bars: loss 1e-4, logits 1e-4, gradients 2e-3 of their maximum, the momentum step 1e-5."""
    ops = _ops()
    rng = np.random.RandomState(B_ + T_)
    x, sl, labs, dense = _batch(rng, B_, T_, D_, C_)
    model = _ctc('f32', label_smoothing_prob=EPS, weight_decay=1e-4)
    sd = _randomise_biases(model, rng)
    okw = dict(ndir=2, cell_clip=50.0, weight_decay=1e-4, temperature=float(temp))
    with ols.patched(EPS):
        ref = omodel.ctc_model_forward(sd, x, labs, sl, L_, **okw)
    plain = omodel.ctc_model_forward(sd, x, labs, sl, L_, want_grads=False, **okw)
    ops.reset_ctc_ls_counts(0)
    ops.reset_ctc_head_counts(0)
    loss, logits = model.compute_loss(x, dense, sl, keep_prob=1.0, softmax_temperature=temp)
    assert ops.ctc_ls_counts(0) == dict(calls=1, lse_done=0, no_grad=0)
    assert ops.ctc_head_counts(0) == dict(head_fwd=0, loss_ex=0, loss=0)
    assert abs(loss.item() - ref['total_loss']) / abs(ref['total_loss']) < 1e-4
    assert abs(ref['total_loss'] - plain['total_loss']) > 1e-2
    assert np.abs(model.ctc_losses.cpu().numpy() - plain['ctc_losses']).max() / plain['ctc_losses'].max() < 1e-4
    assert np.abs(logits.cpu().numpy() - ref['logits']).max() < 1e-4
    opt = model._set_optimizer('momentum', 0.01)
    gv = opt.compute_gradients(loss, model=model)
    for g, name in gv:
        r = ref['grads'][name]
        rel = np.abs(g.cpu().numpy() - r).max() / max(np.abs(r).max(), 1e-8)
        assert rel < 2e-3, (name, rel)
    _momentum_step_fp32(model, gv, opt, sd, ref)
    # a dev loss: the plain CTC loss through today's calls
    model.store.load_state_dict({k: torch.tensor(v) for k, v in sd.items()})
    ops.reset_ctc_ls_counts(0)
    dev, _ = model.compute_loss(x, dense, sl, keep_prob=1.0, softmax_temperature=temp, is_training=False)
    assert ops.ctc_ls_counts(0)['calls'] == 0
    assert abs(dev.item() - plain['total_loss']) / abs(plain['total_loss']) < 1e-4


def test_ctc_model_bf16_takes_the_fused_head(cuda):
    """CTC blstm bf16, C = 11 <= 64: ctc_head_fwd, ctc_loss_ls(lse_done), ctc_head_bwd.  Against the statement on the
    bf16-rounded operands at test_cfgB_bf16_model_parity_at_the_benchmarked_shape's bars: loss 2e-3, logits 5e-2,
    gradients 2e-2 of their maximum.  The momentum step: with lr = 0.01 and a clip that only shrinks, a parameter moves by
    at most lr times its gradient's error, i.e. within 0.01 * 2e-2 of the gradient's maximum (+ 1e-6 for the fp32 update)."""
    ops = _ops()
    rng = np.random.RandomState(B_ + T_)
    x, sl, labs, dense = _batch(rng, B_, T_, D_, C_)
    model = _ctc('bf16', label_smoothing_prob=EPS)
    sd = _randomise_biases(model, rng)
    with ols.patched(EPS):
        ref = omodel.ctc_model_forward(sd, x, labs, sl, L_, cell_clip=50.0, operand_round=olstm.bf16_round_t)
    for reset in (ops.reset_ctc_ls_counts, ops.reset_ctc_head_counts):
        reset(0)
    loss, logits = model.compute_loss(x, dense, sl, keep_prob=1.0)
    assert ops.ctc_head_counts(0) == dict(head_fwd=1, loss_ex=0, loss=0)
    assert ops.ctc_ls_counts(0) == dict(calls=1, lse_done=1, no_grad=0)
    rel = abs(loss.item() - ref['total_loss']) / abs(ref['total_loss'])
    valid = (np.arange(T_)[:, None] < sl[None, :])
    elog = np.abs(logits.cpu().numpy() - ref['logits'])[valid].max()
    opt = model._set_optimizer('momentum', 0.01)
    gv = opt.compute_gradients(loss, model=model)
    worst = 0.0
    for g, name in gv:
        r = ref['grads'][name]
        worst = max(worst, np.abs(g.cpu().numpy() - r).max() / max(np.abs(r).max(), 1e-12))
    print('loss rel %.3g  logits abs %.3g  worst gradient rel %.3g' % (rel, elog, worst))
    assert rel < 2e-3
    assert elog < 5e-2
    assert worst < 2e-2
    model._clip_gradients(gv)
    opt.apply_gradients(gv)
    for name in model.store.names:
        r = ref['grads'][name]
        want = sd[name].astype(np.float64) - 0.01 * oopt.clip_by_norm(r, 5.0)
        assert np.abs(model.store[name].cpu().numpy() - want).max() < 0.01 * 2e-2 * np.abs(r).max() + 1e-6, name
    # one call per step, with dropout too
    for reset in (ops.reset_ctc_ls_counts, ops.reset_ctc_head_counts):
        reset(0)
    for _ in range(2):
        loss, _ = model.compute_loss(x, dense, sl, keep_prob=0.8)
        model.train(loss, 'momentum', 0.01)
    assert ops.ctc_head_counts(0) == dict(head_fwd=2, loss_ex=0, loss=0)
    assert ops.ctc_ls_counts(0) == dict(calls=2, lse_done=2, no_grad=0)
    assert np.isfinite(loss.item())


def test_multitask_ctc_with_label_smoothing(cuda):
    """test_multitask_ctc_parity_and_training's bars: loss 1e-4, logits 1e-4, gradients 2e-3 * max(|r|, 1e-3) + 1e-7."""
    from tensorflow_end2end_speech_recognition_amd.models.ctc.multitask_ctc import MultitaskCTC
    ops = _ops()
    rng = np.random.RandomState(17)
    Cm, Cs, w = 9, 4, 0.7
    x, sl, labs_m, dense_m = _batch(rng, B_, T_, D_, Cm)
    labs_s = [[int(v) for v in rng.randint(0, Cs, size=max(1, int(sl[b]) // 5))] for b in range(B_)]
    dense_s = np.full((B_, max(len(l) for l in labs_s)), -1, dtype=np.int64)
    for b, l in enumerate(labs_s):
        dense_s[b, :len(l)] = l
    model = MultitaskCTC(encoder_type='multitask_blstm', input_size=D_, num_units=H_, num_layers_main=2, num_layers_sub=1,
                         num_classes_main=Cm, num_classes_sub=Cs, main_task_weight=w, parameter_init=0.1,
                         clip_grad_norm=5.0, clip_activation=50, dtype='f32', seed=9, label_smoothing_prob=EPS)
    sd = _randomise_biases(model, rng)
    with ols.patched(EPS):
        ref = omodel.multitask_ctc_model_forward(sd, x, labs_m, labs_s, sl, 2, 1, w, ndir=2, cell_clip=50.0)
    ops.reset_ctc_ls_counts(0)
    loss, lg_m, lg_s = model.compute_loss(x, dense_m, dense_s, sl, keep_prob=1.0)
    assert ops.ctc_ls_counts(0)['calls'] == 2
    assert abs(loss.item() - ref['total_loss']) / abs(ref['total_loss']) < 1e-4
    assert np.abs(lg_m.cpu().numpy() - ref['logits_main']).max() < 1e-4
    assert np.abs(lg_s.cpu().numpy() - ref['logits_sub']).max() < 1e-4
    opt = model._set_optimizer('momentum', 0.01)
    gv = opt.compute_gradients(loss, model=model)
    seen = set()
    for g, name in gv:
        r = ref['grads'][name]
        seen.add(name)
        err = np.abs(g.cpu().numpy() - r).max()
        assert err < 2e-3 * max(np.abs(r).max(), 1e-3) + 1e-7, (name, err, np.abs(r).max())
    assert seen == set(ref['grads'])
    _momentum_step_fp32(model, gv, opt, sd, ref)


def _joint(**kw):
    from tensorflow_end2end_speech_recognition_amd.models.attention.joint_ctc_attention import JointCTCAttention
    return JointCTCAttention(input_size=D_, encoder_type='blstm', encoder_num_units=H_, encoder_num_layers=L_,
                             encoder_num_proj=None, attention_type='bahdanau_content', attention_dim=32,
                             decoder_type='lstm', decoder_num_units=64, decoder_num_layers=1, embedding_dim=8, num_classes=7,
                             sos_index=7, eos_index=8, max_decode_length=12, parameter_init=0.1, clip_grad_norm=5.0,
                             clip_activation_encoder=50, clip_activation_decoder=50, dtype='f32', seed=5,
                             lambda_weight=0.5, **kw)


def _att_batch(rng):
    C = 7
    x = rng.randn(B_, T_, D_).astype(np.float32)
    sl = np.array([T_, T_ // 2 + 1, T_ - 5], dtype=np.int32)
    lens = np.array([5, 2, 4])
    labels = np.full((B_, 7), C + 1, dtype=np.int64)
    ctc_labels = np.full((B_, 5), -1, dtype=np.int64)
    for b in range(B_):
        x[b, sl[b]:] = 0
        y = rng.randint(0, C, size=lens[b])
        labels[b, 0] = C
        labels[b, 1:1 + lens[b]] = y
        ctc_labels[b, :lens[b]] = y
    return x, sl, labels, lens + 2, ctc_labels


def test_joint_ctc_attention_with_ctc_label_smoothing(cuda):
    """test_joint_ctc_attention_parity_and_training's bars: loss 1e-4, ctc logits 1e-4, per-utterance CTC losses 1e-4,
    gradients 2e-3 * max(|r|, 1e-3) + 1e-7; the momentum step at the CTC model's 1e-5."""
    ops = _ops()
    rng = np.random.RandomState(3)
    x, sl, labels, lsl, ctc_labels = _att_batch(rng)
    model = _joint(ctc_label_smoothing_prob=EPS)
    sd = {k: v.cpu().numpy() for k, v in model.store.state_dict().items()}
    ctc_list = [[int(v) for v in row if v >= 0] for row in ctc_labels]
    okw = dict(clip_enc=50.0, clip_dec=50.0, ctc_labels=ctc_list, lambda_weight=0.5)
    with ols.patched(EPS):
        ref = oatt.attention_model_forward(sd, x, labels, sl, lsl, L_, 'bahdanau_content', **okw)
    plain = oatt.attention_model_forward(sd, x, labels, sl, lsl, L_, 'bahdanau_content', **okw)
    ops.reset_ctc_ls_counts(0)
    loss, logits, ctc_logits, otr, oinf = model.compute_loss(x, labels, ctc_labels, sl, lsl, 1.0, 1.0, 1.0)
    assert ops.ctc_ls_counts(0)['calls'] == 1
    assert abs(loss.item() - ref['total_loss']) / abs(ref['total_loss']) < 1e-4
    assert abs(ref['total_loss'] - plain['total_loss']) > 1e-2
    assert np.abs(ctc_logits.cpu().numpy() - ref['ctc_logits']).max() < 1e-4
    assert np.abs(model.ctc_losses.cpu().numpy() - plain['ctc_losses']).max() / plain['ctc_losses'].max() < 1e-4
    opt = model._set_optimizer('momentum', 0.01)
    gv = opt.compute_gradients(loss, model=model)
    for g, name in gv:
        r = ref['grads'][name]
        err = np.abs(g.cpu().numpy() - r).max()
        assert err < 2e-3 * max(np.abs(r).max(), 1e-3) + 1e-7, (name, err)
    _momentum_step_fp32(model, gv, opt, sd, ref)
    ops.reset_ctc_ls_counts(0)
    model.store.load_state_dict({k: torch.tensor(v) for k, v in sd.items()})
    dev = model.compute_loss(x, labels, ctc_labels, sl, lsl, 1.0, 1.0, 1.0, is_training=False)[0]
    assert ops.ctc_ls_counts(0)['calls'] == 0
    assert abs(dev.item() - plain['total_loss']) / abs(plain['total_loss']) < 1e-4


def _digest(model, loss_fn, opt_name):
    loss = loss_fn(model)
    gv = model._set_optimizer(opt_name, 0.01).compute_gradients(loss, model=model)
    return _bits(loss.reshape(1)).tobytes(), {name: _bits(g).tobytes() for g, name in gv}


@pytest.mark.parametrize('which', ['ctc_f32', 'ctc_bf16', 'multitask', 'joint'])
def test_eps_zero_is_the_model_without_the_keyword(cuda, which):
    """eps = 0 (and is_training=False at eps > 0): no call of the new entry point; loss and every gradient carry the bits
    of the model built without the keyword."""
    ops = _ops()
    rng = np.random.RandomState(9)
    if which == 'joint':
        x, sl, labels, lsl, ctc_labels = _att_batch(rng)
        mk = lambda kw: _joint(**({'ctc_label_smoothing_prob': kw} if kw is not None else {}))
        run = lambda m, **k: m.compute_loss(x, labels, ctc_labels, sl, lsl, 1.0, 1.0, 1.0, **k)[0]
    elif which == 'multitask':
        from tensorflow_end2end_speech_recognition_amd.models.ctc.multitask_ctc import MultitaskCTC
        x, sl, labs, dense = _batch(rng, B_, T_, D_, 9)
        dense_s = np.where(dense >= 0, dense % 4, -1)
        mk = lambda kw: MultitaskCTC(encoder_type='multitask_blstm', input_size=D_, num_units=H_, num_layers_main=2,
                                     num_layers_sub=1, num_classes_main=9, num_classes_sub=4, main_task_weight=0.7,
                                     dtype='f32', seed=9, **({'label_smoothing_prob': kw} if kw is not None else {}))
        run = lambda m, **k: m.compute_loss(x, dense, dense_s, sl, keep_prob=1.0, **k)[0]
    else:
        x, sl, labs, dense = _batch(rng, B_, T_, D_, C_)
        mk = lambda kw: _ctc(which[4:], **({'label_smoothing_prob': kw} if kw is not None else {}))
        run = lambda m, **k: m.compute_loss(x, dense, sl, keep_prob=1.0, **k)[0]
    ops.reset_ctc_ls_counts(0)
    base = _digest(mk(None), run, 'sgd')
    zero = _digest(mk(0.0), run, 'sgd')
    assert ops.ctc_ls_counts(0)['calls'] == 0
    assert zero[0] == base[0] and zero[1] == base[1]
    # a dev loss of the smoothed model: the plain model's, bit for bit, and no call
    dev_plain = run(mk(None), is_training=False)
    dev_ls = run(mk(EPS), is_training=False)
    assert ops.ctc_ls_counts(0)['calls'] == 0
    assert _bits(dev_plain.reshape(1)).tobytes() == _bits(dev_ls.reshape(1)).tobytes()
    # ... while its training loss differs and does call
    tr = run(mk(EPS))
    assert ops.ctc_ls_counts(0)['calls'] == (2 if which == 'multitask' else 1)
    assert _bits(tr.reshape(1)).tobytes() != base[0]
