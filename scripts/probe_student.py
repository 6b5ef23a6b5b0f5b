"""StudentCTC on the MI355X: per-kernel rates of the student CNN's pieces and training-step times (bf16, adam).

  conv3x4    the implicit 3x4 kernels (forward, data gradient, weight gradient) against asr_im2col + GEMM for the same
             product, at CNN2's two channel pairs (64 -> 128, 128 -> 256), F = 40 -> 14 rows, W = 10
  cnn1       the 9x9 3 -> C1 im2col + GEMM forward, and its share of the convolution FLOPs
  bn         asr_bn_stats, asr_bn_apply (with the [3,1] pool) and asr_bn_bwd on CNN1's activation, in GB/s of their own
             HBM traffic (stats: one read; apply: one read + the bf16 write; bwd: two passes over x and dz + the write)
  steps      ms per training step: XE at 512 frames, CTC at B = 16 with the bench's lengths U{100..778}, both sizes

    python scripts/probe_student.py [--steps 5] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import bench  # noqa: E402
from tensorflow_end2end_speech_recognition_amd import ops  # noqa: E402
from tensorflow_end2end_speech_recognition_amd._lib import ASR_BF16, ASR_F32  # noqa: E402
from tensorflow_end2end_speech_recognition_amd.models.ctc.student_ctc import StudentCTC  # noqa: E402

PEAK = 2.5e15            # dense bf16 peak of the MI355X (FLOP/s)
HBM = 8.0e12             # HBM3E peak (B/s)
F, W, DEV = 40, 10, 'cuda:0'


def timed(fn, reps=10):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def conv_ab(cin, cout, N):
    H = (F + 2) // 3
    g = torch.Generator(device=DEV).manual_seed(cin)
    x = torch.randn(N, H, W, cin, generator=g, device=DEV).to(torch.bfloat16)
    dy = torch.randn(N, H, W, cout, generator=g, device=DEV).to(torch.bfloat16)
    w = torch.randn(3, 4, cin, cout, generator=g, device=DEV) * 0.05
    b = torch.zeros(cout, device=DEV)
    wf, wb = ops.conv3x4_prep_weights(w)
    w2 = w.to(torch.bfloat16).view(12 * cin, cout)
    dw = torch.empty(12 * cin, cout, device=DEV)
    K = 12 * cin
    ldp = (K + 7) // 8 * 8

    def im_fwd():
        pat = ops.im2col(x, 3, 4, 1, 1, ldp=ldp)
        ops.gemm(pat[:, :K], w2, bias=b, relu=True, out_dtype=ASR_F32)

    def im_dgrad():
        dpat = ops.gemm(dy.view(-1, cout), w2, transB=True, out_dtype=ASR_F32)
        ops.col2im(dpat, N, H, W, cin, 3, 4, 1, 1)

    def im_wgrad():
        pat = ops.im2col(x, 3, 4, 1, 1, ldp=ldp)
        ops.gemm(pat[:, :K], dy.view(-1, cout), transA=True, out=dw)

    flop = 2.0 * N * H * W * K * cout
    r = {}
    for name, imp, im in (('fwd', lambda: ops.conv3x4_fwd(x, wf, b, True, ASR_F32), im_fwd),
                          ('dgrad', lambda: ops.conv3x4_bwd_data(dy, wb), im_dgrad),
                          ('wgrad', lambda: ops.conv3x4_bwd_weight_bias(x, dy, dw, None), im_wgrad)):
        a, c = timed(imp), timed(im)
        r[name] = dict(implicit_ms=round(a, 3), im2col_ms=round(c, 3), speedup=round(c / a, 2),
                       implicit_frac_peak=round(flop / a / 1e-3 / PEAK, 4))
    return r


def cnn1_and_bn(C1, N):
    g = torch.Generator(device=DEV).manual_seed(C1)
    x = torch.randn(N, F, W, 3, generator=g, device=DEV).to(torch.bfloat16)
    w = (torch.randn(243, C1, generator=g, device=DEV) * 0.05).to(torch.bfloat16)
    b = torch.zeros(C1, device=DEV)

    def cnn1():
        pat = ops.im2col(x, 9, 9, 1, 1, ldp=248)
        return ops.gemm(pat[:, :243], w, bias=b, relu=True, out_dtype=ASR_F32)

    a = cnn1().view(N, F, W, C1)
    gam, bet = torch.ones(C1, device=DEV), torch.zeros(C1, device=DEV)
    st = ops.bn_stats(a, 1e-3, 0.9, bet, gam)
    out, arg = ops.bn_apply(a, st[0], st[1], gam, bet, 1e-3, True, ASR_BF16)
    dz = torch.randn(out.shape, generator=g, device=DEV)
    dgam, dbet = torch.empty(C1, device=DEV), torch.empty(C1, device=DEV)
    nb = a.numel() * 4
    t_stats = timed(lambda: ops.bn_stats(a, 1e-3, 0.9, bet, gam))
    t_apply = timed(lambda: ops.bn_apply(a, st[0], st[1], gam, bet, 1e-3, True, ASR_BF16))
    t_bwd = timed(lambda: ops.bn_bwd(dz, arg, a, st, gam, dgam, dbet, ASR_BF16))
    t_cnn1 = timed(cnn1)
    by_apply = nb + out.numel() * 3                       # fp32 read, bf16 + uint8 argmax write
    by_bwd = 2 * (nb + dz.numel() * 5) + a.numel() * 2    # two passes over x, dz and the argmax, the bf16 write
    return dict(images=N, cnn1_ms=round(t_cnn1, 3),
                cnn1_frac_peak=round(2.0 * N * F * W * 243 * C1 / t_cnn1 / 1e-3 / PEAK, 4),
                bn_stats=dict(ms=round(t_stats, 3), GBps=round(nb / t_stats / 1e6, 1)),
                bn_apply_pool=dict(ms=round(t_apply, 3), GBps=round(by_apply / t_apply / 1e6, 1)),
                bn_bwd_pool=dict(ms=round(t_bwd, 3), GBps=round(by_bwd / t_bwd / 1e6, 1)))


def step_xe(enc, frames, steps):
    rng = np.random.RandomState(0)
    m = StudentCTC(enc, 3 * F * W, 3387, splice=5, num_stack=2, dtype='bf16', seed=0)
    x = torch.from_numpy(rng.randn(frames, 3 * F * W).astype(np.float32)).to(DEV)
    p = torch.softmax(torch.randn(frames, 3388, device=DEV), 1)
    for it in range(2 + steps):
        if it == 2:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        loss, _ = m.compute_xe_loss(x, p, 0.9)
        m.train(loss, 'adam', 1e-4)
    torch.cuda.synchronize()
    return dict(encoder=enc, frames=frames, ms_per_step=round((time.perf_counter() - t0) * 1e3 / steps, 2),
                loss=round(float(loss.item()), 3))


def step_ctc(enc, B, steps):
    x, sl, _, dense = bench.make_batch(1, B, F * W * 3, 29, 100, 778)
    xd, sd = torch.tensor(x, device=DEV), torch.tensor(sl, device=DEV)
    m = StudentCTC(enc, 3 * F * 2, 28, splice=5, num_stack=2, dtype='bf16', seed=0, clip_grad_norm=5.0)
    for it in range(1 + steps):
        if it == 1:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        loss, _ = m.compute_ctc_loss(xd, dense, sd, 0.9)
        m.train(loss, 'adam', 1e-4)
    torch.cuda.synchronize()
    return dict(encoder=enc, B=B, images=int(x.shape[0] * x.shape[1]), frames=int(sl.sum()),
                ms_per_step=round((time.perf_counter() - t0) * 1e3 / steps, 2), loss=round(float(loss.item()), 3),
                conv_path=m.encoder.conv_path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    N = 12448                                              # B = 16 x T = 778 images
    res = dict(conv3x4={'64x128': conv_ab(64, 128, N), '128x256': conv_ab(128, 256, N)},
               cnn1_bn={'C1=64': cnn1_and_bn(64, N), 'C1=128': cnn1_and_bn(128, N)})
    res['steps'] = [step_xe('student_cnn_compact_xe', 512, a.steps), step_xe('student_cnn_xe', 512, a.steps),
                    step_ctc('student_cnn_compact', 16, a.steps), step_ctc('student_cnn', 16, a.steps)]
    res['hbm_peak_GBps'] = HBM / 1e9
    s = json.dumps(res, indent=1)
    print(s)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(s)


if __name__ == '__main__':
    main()
