"""GPU: the frames form of the reduction-major (weight-gradient) products, ops.gemm_tn_frames / asr_gemm_tn_frames.
The k rows of both operands are the frames of a time-major [T, Bp] batch and the second operand (the BPTT kernels'
dgates) is exactly zero in the rows of padded frames.  The product must have the bits of the plain ops.gemm(A, B,
transA=True) -- same tiles, slabs and reducer -- and it must not LOAD the rows of padded frames from either operand:
with NaN written there the result stays what it was.  Both shifted views of the recurrent product, the default split-K
slabs and the workgroup cap of products that run beside a recurrence kernel, shapes on the lean TN kernel (K >= 2048)
and on the generic one."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _ops():
    from tensorflow_end2end_speech_recognition_amd import ops
    return ops


def _lens(T, Bp, seed):
    """One utterance of length 0, one of length T, one of length 1, the rest mixed."""
    rng = np.random.RandomState(seed)
    lens = rng.randint(1, T + 1, size=Bp).astype(np.int32)
    lens[1], lens[2], lens[Bp - 1] = 0, T, 1
    return lens


def _operands(cuda, T, Bp, M, N, lens, seed):
    """h [T*Bp, M] and dgates [T*Bp, N] bf16; dgates exactly zero at padded frames; `pad` marks those rows."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    h = torch.randn((T * Bp, M), generator=g).to(torch.bfloat16)
    dg = (torch.randn((T * Bp, N), generator=g) * 0.25).to(torch.bfloat16)
    pad = (torch.arange(T)[:, None] >= torch.from_numpy(lens.astype(np.int64))[None, :]).reshape(T * Bp)
    dg[pad] = 0
    return h.to(cuda), dg.to(cuda), pad.to(cuda)


def _views(h, dg, pad, T, Bp):
    """(A, B, padded rows of the view, frame of B's first row) for the input product and the two shifted views of the
    recurrent product (rnn_util.LSTMLayer.backward): forward direction h(t-1) with dG(t), backward h(t+1) with dG(t)."""
    K1 = (T - 1) * Bp
    return [(h, dg, pad, 0),
            (h[:K1], dg[Bp:], pad[Bp:], 1),
            (h[Bp:], dg[:K1], pad[:K1], 0)]


def _lean(M, N, K):
    return K >= 2048 and M % 8 == 0 and N % 8 == 0


# the first two (T, Bp) keep K = T * Bp below the lean TN kernel's K >= 2048 (the generic kernel's frames form runs); the
# others are the smallest batches above it whose K is no multiple of 64 either: Bp = 16 and 32 (a thread's rows stay with
# one utterance: the per-thread bound) and Bp = 48, which does not divide 64 (the per-load test)
SHAPES = [(9, 16), (5, 32), (130, 16), (66, 32), (44, 48)]


@pytest.mark.parametrize('T,Bp', SHAPES)
@pytest.mark.parametrize('capped', [False, True])
def test_frames_product_has_the_plain_bits_and_does_not_load_padded_frames(cuda, T, Bp, capped):
    ops = _ops()
    lens_np = _lens(T, Bp, 7 * T + Bp)
    lens = torch.from_numpy(lens_np).to(cuda)
    for M in (8, 120, 136):
        for N in (128, 264):
            h, dg, pad = _operands(cuda, T, Bp, M, N, lens_np, 1000 * M + N + T)
            for vi, (A, B, vpad, frame0) in enumerate(_views(h, dg, pad, T, Bp)):
                K = A.shape[0]
                assert bool(vpad.any()) and not bool(vpad.all())

                def run(frames, a, b):
                    if frames:
                        return ops.gemm_tn_frames(a, b, lens, Bp, frame0)
                    return ops.gemm(a, b, transA=True, out_dtype=torch.float32)
                if capped:      # the cap lives on the side lanes' handles: both products run there
                    ops.set_side_gemm_workgroups(cuda, 128)
                    try:
                        with ops.side_lane(cuda, keep=(A, B, lens), lane=1):
                            plain = run(False, A, B)
                            ops.reset_gemm_path_counts(0)
                            got = run(True, A, B)
                            counts = ops.tn_frames_path_counts(0)
                            An, Bn = A.clone(), B.clone()
                            An[vpad] = float('nan')
                            Bn[vpad] = float('nan')
                            got_nan = run(True, An, Bn)
                        ops.join_side(cuda)
                    finally:
                        ops.set_side_gemm_workgroups(cuda, 0)
                else:
                    plain = run(False, A, B)
                    ops.reset_gemm_path_counts(0)
                    got = run(True, A, B)
                    counts = ops.tn_frames_path_counts(0)
                    An, Bn = A.clone(), B.clone()
                    An[vpad] = float('nan')
                    Bn[vpad] = float('nan')
                    got_nan = run(True, An, Bn)
                where = (T, Bp, M, N, vi, capped)
                want = dict(tn_frames=1, tn_frames_generic=0) if _lean(M, N, K) else dict(tn_frames=0, tn_frames_generic=1)
                assert counts == want, (where, counts)
                p, g, gn = plain.cpu().numpy(), got.cpu().numpy(), got_nan.cpu().numpy()
                assert np.isfinite(p).all() and np.abs(p).max() > 0, where
                assert np.array_equal(p, g), where
                assert np.array_equal(p, gn), where


def test_frames_product_accumulates_like_the_plain_one(cuda):
    """accumulate=True (the second half-batch pipeline adds its products to the first's), lean kernel and generic."""
    ops = _ops()
    for T, Bp in ((130, 16), (9, 16)):
        lens_np = _lens(T, Bp, 3)
        lens = torch.from_numpy(lens_np).to(cuda)
        h, dg, pad = _operands(cuda, T, Bp, 120, 264, lens_np, 11)
        base = torch.randn((120, 264), device=cuda)
        want = ops.gemm(h, dg, transA=True, out=base.clone(), accumulate=True)
        hn = h.clone()
        hn[pad] = float('nan')
        got = ops.gemm_tn_frames(hn, dg, lens, Bp, 0, out=base.clone(), accumulate=True)
        assert np.array_equal(want.cpu().numpy(), got.cpu().numpy())


def test_layer_backward_takes_the_frames_products_and_gives_the_same_gradients(cuda, monkeypatch):
    """One 2 x 256 bf16 BLSTM-CTC training step with the switch on and off: the LSTMLayer products are counted on the
    frames path, and loss and every updated parameter are equal."""
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    from tensorflow_end2end_speech_recognition_amd.models.encoders.core import rnn_util
    ops = _ops()
    rng = np.random.RandomState(5)
    B, T, D, C = 3, 140, 48, 11
    x = rng.randn(B, T, D).astype(np.float32)
    sl = np.array([T, 1, 77], dtype=np.int32)
    dense = np.full((B, 4), -1, dtype=np.int64)
    dense[0, :4] = [1, 2, 2, 3]
    dense[1, :1] = [4]
    dense[2, :3] = [5, 0, 6]
    outs = []
    for on in (True, False):
        monkeypatch.setattr(rnn_util, 'TN_FRAMES', on)
        m = CTC('blstm', D, 256, 2, C, clip_grad_norm=5.0, clip_activation=50, dtype='bf16', seed=3)
        ops.reset_gemm_path_counts(0)
        loss, _ = m.compute_loss(x, dense, sl, keep_prob=0.8)
        m.train(loss, 'adam', 1e-3)
        torch.cuda.synchronize()
        c = ops.tn_frames_path_counts(0)
        # per layer and direction: x^T dG and h_prev^T dG.  K = 140 * 16 = 2240 and 2224: the lean kernel takes all eight
        assert c == (dict(tn_frames=8, tn_frames_generic=0) if on else dict(tn_frames=0, tn_frames_generic=0)), c
        outs.append((loss.item(), {k: v.cpu().numpy() for k, v in m.store.state_dict().items()}))
    assert outs[0][0] == outs[1][0]
    for k in outs[0][1]:
        assert np.array_equal(outs[0][1][k], outs[1][1][k]), k
