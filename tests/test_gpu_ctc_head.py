"""GPU: the CTC head stretch in three launches (ops.ctc_head_fwd, ops.ctc_loss_ex, the lean NT product on the bf16
image of dlogits) against the separate launches it replaces, which stay in the library: dropout_apply, gemm, ctc_loss,
cast_from_f32, gemm, dropout_apply.  Every comparison is np.array_equal."""
import numpy as np
import pytest
import torch

from tensorflow_end2end_speech_recognition_amd._lib import ASR_BF16

pytestmark = pytest.mark.gpu

BP, NB = 16, 3          # padded batch, real utterances


def _ops():
    from tensorflow_end2end_speech_recognition_amd import ops
    return ops


def _np(t):
    return t.float().cpu().numpy() if t.dtype == torch.bfloat16 else t.cpu().numpy()


def _batch(T, C):
    """Utterance 0: length T, a repeated label where T leaves room for it (a single label at T = 1); utterance 1: length
    1 with two labels (infeasible: zero loss row, zero gradient, counted); utterance 2: no labels; rows 3..15: the batch
    padding (length 0, no labels).  blank = C - 1, labels 0 and 1."""
    lens = np.zeros(BP, dtype=np.int32)
    lens[0], lens[1], lens[2] = T, 1, max(1, T // 2)
    labs = [[1, 1, 0] if T >= 6 else [1], [0, 1], []] + [[] for _ in range(BP - NB)]
    flat = np.array([l for u in labs for l in u], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum([len(u) for u in labs])]).astype(np.int32)
    return lens, flat, off, max(len(u) for u in labs)


def _valid_rows(lens, T):
    from tensorflow_end2end_speech_recognition_amd.models.encoders.core import rnn_util
    return rnn_util.valid_rows(lens, T, BP)


def _run_pair(cuda, T, E, C, keep):
    """(separate launches, fused launches) of one head stretch on the same operands, as dicts of tensors."""
    ops = _ops()
    g = torch.Generator(device='cpu').manual_seed(1000 * T + 10 * E + C)
    hout = torch.randn((T, BP, E), generator=g).to(torch.bfloat16).to(cuda)
    W = (torch.randn((E, C), generator=g) * 0.2).to(cuda)
    bias = (torch.randn((C,), generator=g) * 0.5).to(cuda)
    lens_np, flat_np, off_np, lmax = _batch(T, C)
    lens, flat, off = (torch.from_numpy(a).to(cuda) for a in (lens_np, flat_np, off_np))
    drop = (keep, 77, 5 << 20) if keep < 1.0 else None
    rows_np = _valid_rows(lens_np, T)
    rows = torch.from_numpy(rows_np).to(cuda)
    scale = 1.0 / NB

    # today's sequence
    Wsh = ops.cast_from_f32(W, ASR_BF16)
    x_ref = ops.dropout_apply(hout, *drop) if drop else hout
    logits_ref = torch.empty((T, BP, C), dtype=torch.float32, device=cuda)
    ops.gemm(x_ref.view(T * BP, E), Wsh, bias=bias, out=logits_ref.view(T * BP, C))
    ops.reset_ctc_head_counts(0)
    loss_ref, grad_ref, ninf_ref = ops.ctc_loss(logits_ref, flat, off, lens, lmax, grad_scale=scale)
    assert ops.ctc_head_counts(0) == dict(head_fwd=0, loss_ex=0, loss=1)
    dl_ref = ops.cast_from_f32(grad_ref.view(T * BP, C), ASR_BF16)
    denc_ref = ops.gemm(dl_ref, Wsh, transB=True, out_dtype=torch.float32)
    if drop:
        denc_ref = ops.dropout_apply(denc_ref, *drop)
    old = dict(x=x_ref, logits=logits_ref, loss=loss_ref, grad=grad_ref, ninf=ninf_ref, dl=dl_ref, denc=denc_ref)

    # the fused launches
    assert ops.ctc_head_ok(T * BP, E, C)
    Wt, Wp = ops.ctc_head_prep(W)
    ws = ops.ctc_workspace(T, BP, lmax, cuda)
    ops.reset_ctc_head_counts(0)
    x, logits, ninf = ops.ctc_head_fwd(hout, drop, Wt, bias, C, flat, off, lens, lmax, ws)
    loss, grad, img, ninf = ops.ctc_loss_ex(logits, flat, off, lens, lmax, grad_scale=scale, ws=ws, ninf=ninf,
                                            lse_done=True)
    assert ops.ctc_head_counts(0) == dict(head_fwd=1, loss_ex=1, loss=0)
    denc = torch.full((T * BP, E), float('nan'), dtype=torch.float32, device=cuda)
    ops.reset_gemm_path_counts(0)
    ops.ctc_head_bwd(img, Wp, denc, drop=drop, rows=(rows, rows_np.size))
    lean = T * BP >= 1024 and E % 128 == 0          # the lean NT kernel's shapes (K = Kp = 64)
    assert ops.ctc_head_bwd_counts(0) == (dict(head_bwd_lean=1, head_bwd_full=0) if lean
                                          else dict(head_bwd_lean=0, head_bwd_full=1))
    assert ops.gemm_path_counts(0) == dict(rows_128=0, rows_256=0, rows_full=0)
    new = dict(x=x, logits=logits, loss=loss, grad=grad, ninf=ninf, img=img, denc=denc, Wp=Wp, Wt=Wt)
    return old, new, rows_np, W


@pytest.mark.parametrize('keep', [1.0, 0.8])
@pytest.mark.parametrize('C', [3, 62, 64])
@pytest.mark.parametrize('E', [64, 128])
@pytest.mark.parametrize('T', [1, 6, 13, 70])
def test_fused_head_launches_give_the_bits_of_the_separate_ones(cuda, T, E, C, keep):
    """T = 1, 6, 13 (the issue's; fewer rows than the lean NT kernel's M >= 1024, so the d(encoder output) product runs
    the full generic kernel) and T = 70 (1120 rows: with E = 128 the listed-row lean NT kernel runs, padded rows stay
    unwritten)."""
    old, new, rows, W = _run_pair(cuda, T, E, C, keep)
    assert np.array_equal(_np(old['x']), _np(new['x']))
    assert np.array_equal(_np(old['logits']), _np(new['logits']))            # every row
    assert np.isfinite(_np(new['logits'])).all()
    assert np.array_equal(_np(old['loss']), _np(new['loss']))
    assert np.array_equal(_np(old['grad']), _np(new['grad']))
    assert int(new['ninf'].item()) == 1 and int(old['ninf'].item()) == 1
    loss = _np(new['loss'])
    assert loss[1] == 0.0 and loss[0] > 0.0 and loss[2] > 0.0 and not loss[NB:].any()
    grad = _np(new['grad'])
    assert not grad[:, 1].any() and grad[:, 0].any()
    img = _np(new['img'])
    assert img.shape == (T * BP, 64)
    assert np.array_equal(img[:, :C], _np(old['dl']))
    assert not img[:, C:].any()
    # the weight images: the operand shadow's rounding, zero padding
    Wsh = _np(_ops().cast_from_f32(W, ASR_BF16))
    assert np.array_equal(_np(new['Wp'])[:, :C], Wsh) and not _np(new['Wp'])[:, C:].any()
    assert np.array_equal(_np(new['Wt'])[:C], Wsh.T) and not _np(new['Wt'])[C:].any()
    assert np.array_equal(_np(old['denc'])[rows], _np(new['denc'])[rows])
    assert np.isfinite(_np(new['denc'])[rows]).all()


def test_head_shapes_outside_the_fused_forward(cuda):
    ops = _ops()
    assert not ops.ctc_head_ok(16 * 13, 128, 65)         # more than one column tile
    assert not ops.ctc_head_ok(16 * 13, 96, 39)          # E % 64
    assert not ops.ctc_head_ok(16 * 13, 1024, 39)        # today's product would split K
    assert ops.ctc_head_ok(64 * 400, 1024, 39)           # ... and does not at >= 256 tiles of 64 rows
    assert ops.ctc_head_ok(16 * 745, 512, 39)            # the headline step


def _model_step(cuda, monkeypatch, fused, H=256, L=2, C=11, T=12, temp=1, bottleneck=None, nan_denc=False, keep=0.8):
    """One training step of CTC('blstm') on a fixed batch: (loss, logits on valid frames, updated parameters, counters)."""
    from tensorflow_end2end_speech_recognition_amd.models.ctc import ctc as ctc_mod
    ops = _ops()
    monkeypatch.setattr(ctc_mod, 'HEAD_FUSED', fused)
    if nan_denc:
        monkeypatch.setattr(ctc_mod.CTC, '_new_denc', staticmethod(
            lambda rows, E, device: torch.full((rows, E), float('nan'), dtype=torch.float32, device=device)))
    else:
        monkeypatch.setattr(ctc_mod.CTC, '_new_denc', staticmethod(
            lambda rows, E, device: torch.zeros((rows, E), dtype=torch.float32, device=device)))
    rng = np.random.RandomState(5)
    B, D = 3, 48
    x = rng.randn(B, T, D).astype(np.float32)
    sl = np.array([T, 1, max(1, T // 2)], dtype=np.int32)
    dense = np.full((B, 3), -1, dtype=np.int64)
    dense[0, :3] = [1, 1, 0]
    dense[1, :1] = [2]
    m = ctc_mod.CTC('blstm', D, H, L, C - 1, clip_grad_norm=5.0, clip_activation=50, dtype='bf16', seed=3,
                    bottleneck_dim=bottleneck)
    for reset in (ops.reset_ctc_head_counts, ops.reset_gemm_path_counts, ops.reset_recurrence_path_counts):
        reset(0)
    loss, logits = m.compute_loss(x, dense, sl, keep_prob=keep, softmax_temperature=temp)
    m.train(loss, 'adam', 1e-3)
    torch.cuda.synchronize()
    counts = dict(ops.ctc_head_counts(0), **ops.gemm_path_counts(0))
    counts.update(ops.recurrence_path_counts(0))
    counts.update(ops.ctc_head_bwd_counts(0))
    lg = logits.cpu().numpy()
    valid = np.concatenate([lg[:sl[b], b] for b in range(B)])
    return loss.item(), valid, {k: v.cpu().numpy() for k, v in m.store.state_dict().items()}, counts


def _same(a, b):
    assert a[0] == b[0] and np.isfinite(a[0])
    assert np.array_equal(a[1], b[1])
    for k in a[2]:
        assert np.array_equal(a[2][k], b[2][k]), k


def test_model_step_with_the_switch_on_and_off(cuda, monkeypatch):
    """2 x 256, T = 12, B = 3, dropout 0.8: loss, logits on valid frames and every updated parameter."""
    on = _model_step(cuda, monkeypatch, True)
    off = _model_step(cuda, monkeypatch, False)
    assert (on[3]['head_fwd'], on[3]['loss_ex'], on[3]['loss']) == (1, 1, 0), on[3]
    assert (off[3]['head_fwd'], off[3]['loss_ex'], off[3]['loss']) == (0, 0, 1), off[3]
    _same(on, off)


def test_model_step_without_dropout(cuda, monkeypatch):
    on = _model_step(cuda, monkeypatch, True, keep=1.0)
    off = _model_step(cuda, monkeypatch, False, keep=1.0)
    assert on[3]['head_fwd'] == 1
    _same(on, off)


def test_softmax_temperature_and_bottleneck_and_wide_heads_keep_the_old_forward(cuda, monkeypatch):
    t_on = _model_step(cuda, monkeypatch, True, temp=2)
    t_off = _model_step(cuda, monkeypatch, False, temp=2)
    assert (t_on[3]['head_fwd'], t_on[3]['loss_ex'], t_on[3]['loss']) == (0, 0, 1), t_on[3]
    _same(t_on, t_off)
    b_on = _model_step(cuda, monkeypatch, True, bottleneck=64)
    b_off = _model_step(cuda, monkeypatch, False, bottleneck=64)
    assert (b_on[3]['head_fwd'], b_on[3]['loss_ex'], b_on[3]['loss']) == (0, 0, 1), b_on[3]
    _same(b_on, b_off)
    # C = 65: the forward keeps its launches (more than one column tile); the backward half has no limit on C
    w_on = _model_step(cuda, monkeypatch, True, C=65)
    w_off = _model_step(cuda, monkeypatch, False, C=65)
    assert (w_on[3]['head_fwd'], w_on[3]['loss_ex'], w_on[3]['loss']) == (0, 1, 0), w_on[3]
    _same(w_on, w_off)


@pytest.mark.parametrize('H,path', [(256, 'lstm_cluster'), (64, 'lstm_single_cu')])
def test_padded_rows_of_the_head_gradient_are_never_used(cuda, monkeypatch, H, path):
    """T = 70 (1120 rows: the listed-row lean NT kernel writes the valid frames of d(encoder output) only): with NaN
    in the buffer beforehand the step's gradients equal those of a run on a zeroed buffer -- on the cluster BPTT
    kernels (H = 256) and on the single-CU ones (H = 64)."""
    clean = _model_step(cuda, monkeypatch, True, H=H, L=2, T=70)
    dirty = _model_step(cuda, monkeypatch, True, H=H, L=2, T=70, nan_denc=True)
    assert clean[3][path] > 0, clean[3]
    _same(clean, dirty)
    off = _model_step(cuda, monkeypatch, False, H=H, L=2, T=70)
    # the head's d(encoder output) product ran the listed-row lean NT kernel, under its own counter
    assert clean[3]['head_fwd'] == 1 and clean[3]['head_bwd_lean'] == 1 and clean[3]['head_bwd_full'] == 0, clean[3]
    assert off[3]['head_bwd_lean'] == 0 and off[3]['head_bwd_full'] == 0, off[3]
    assert clean[3]['rows_128'] == off[3]['rows_128'] and clean[3]['rows_full'] == off[3]['rows_full']
    _same(clean, off)
