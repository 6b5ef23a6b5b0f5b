"""cnn_zhang CTC on the MI355X: ms per training step at the cfg C input geometry (F = 40, splice 11, bf16, dropout 0.2,
adam) on the bench's synthetic lengths (U{100..778}) with B = 16 and B = 64, and per-layer-shape kernel rates: the
implicit 3x5 kernels (forward, data gradient, weight gradient) against asr_im2col + GEMM for the same product.

    python scripts/probe_cnn_zhang.py [--batches 16,64] [--steps 5] [--no-ab] [--json out.json]
    rocprofv3 --kernel-trace --stats -d <dir> -o cnn_zhang -- python scripts/probe_cnn_zhang.py --batches 16 --no-ab
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
from tensorflow_end2end_speech_recognition_amd._lib import ASR_F32  # noqa: E402
from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC  # noqa: E402

PEAK = 2.5e15            # dense bf16 peak of the MI355X (FLOP/s)
F, W = 40, 11


def model_flop_per_frame(C=62):
    """Multiply-add FLOPs of one frame's training step: forward + data gradient + weight gradient of every layer, except
    CNN1's data gradient (never formed); the output layer included."""
    H0, H1 = F, (F + 2) // 3
    conv = [(3, 128, H0)] + [(128, 128, H1)] * 3 + [(128, 256, H1)] + [(256, 256, H1)] * 5
    fcs = [(H1 * W * 256, 1024), (1024, 1024), (1024, 1024), (1024, C)]
    flop = 0
    for i, (ci, co, h) in enumerate(conv):
        flop += (2 if i == 0 else 3) * 2 * h * W * 15 * ci * co
    for k, n in fcs:
        flop += 3 * 2 * k * n
    return flop


def step_ms(B, steps, warmup, dev):
    x, sl, _, dense = bench.make_batch(1, B, F * W * 3, 62, 100, 778)
    xd, sd = torch.tensor(x, device=dev), torch.tensor(sl, device=dev)
    m = CTC('cnn_zhang', 3 * F, 256, 10, 61, splice=W, parameter_init=0.03, clip_grad_norm=5.0, dtype='bf16',
            device=str(dev), seed=0)
    for it in range(warmup + steps):
        if it == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        loss, _ = m.compute_loss(xd, dense, sd, keep_prob=0.8)
        m.train(loss, 'adam', 1e-4)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    frames = int(sl.sum())
    flop = frames * model_flop_per_frame()
    return dict(B=B, frames=frames, ms_per_step=round(ms, 2), loss=round(float(loss.item()), 3),
                tflops_step=round(flop / ms / 1e9, 1), frac_peak=round(flop / ms / 1e-3 / PEAK, 4),
                conv_path=sorted(set(m.encoder.conv_path.values())))


def timed(fn, reps=10):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def layer_ab(N, dev):
    """One layer of each (Cin, Cout) shape over N images of 14 x 11: implicit kernels vs asr_im2col + GEMM."""
    rows = []
    H = (F + 2) // 3
    for cin, cout in [(128, 128), (128, 256), (256, 256)]:
        x = torch.randn(N, H, W, cin, device=dev).to(torch.bfloat16)
        dy = torch.randn(N, H, W, cout, device=dev).to(torch.bfloat16)
        w = torch.randn(3, 5, cin, cout, device=dev) * 0.03
        b = torch.zeros(cout, device=dev)
        wf, wb = ops.conv3x5_prep_weights(w)
        w2d = w.to(torch.bfloat16).view(15 * cin, cout)
        dw = torch.empty(15 * cin, cout, device=dev)
        db = torch.empty(cout, device=dev)
        K = 15 * cin
        chunk = max(1, (1 << 30) // (H * W * K * 2))

        def im2col_fwd():
            for c0 in range(0, N, chunk):
                pat = ops.im2col(x[c0:c0 + chunk], 3, 5, 1, 1)
                ops.gemm(pat, w2d, bias=b, relu=True)

        def im2col_wgrad():
            for ci, c0 in enumerate(range(0, N, chunk)):
                pat = ops.im2col(x[c0:c0 + chunk], 3, 5, 1, 1)
                n = min(chunk, N - c0)
                ops.gemm(pat, dy[c0:c0 + n].view(-1, cout), transA=True, out=dw, accumulate=ci > 0)
            ops.colsum(dy.view(-1, cout), out=db)

        def im2col_dgrad():
            for c0 in range(0, N, chunk):
                n = min(chunk, N - c0)
                dpat = ops.gemm(dy[c0:c0 + n].view(-1, cout), w2d, transB=True, out_dtype=ASR_F32)
                ops.col2im(dpat, n, H, W, cin, 3, 5, 1, 1)

        flop = 2.0 * N * H * W * 15 * cin * cout
        res = dict(shape='%dx%d' % (cin, cout), images=N, H=H, W=W, gflop=round(flop / 1e9, 1))
        for name, fn in (('fwd_implicit', lambda: ops.conv3x5_fwd(x, wf, b, relu=True)),
                         ('fwd_im2col_gemm', im2col_fwd),
                         ('dgrad_implicit', lambda: ops.conv3x5_bwd_data_relu(dy, wb, x)),
                         ('dgrad_gemm_col2im', im2col_dgrad),
                         ('wgrad_implicit', lambda: ops.conv3x5_bwd_weight_bias(x, dy, dw, db)),
                         ('wgrad_im2col_gemm', im2col_wgrad)):
            ms = timed(fn, reps=5)
            res[name + '_ms'] = round(ms, 3)
            res[name + '_tflops'] = round(flop / ms / 1e9, 1)
            res[name + '_frac_peak'] = round(flop / ms / 1e-3 / PEAK, 4)
        rows.append(res)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='16,64')
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--no-ab', action='store_true')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    out = dict(device=torch.cuda.get_device_name(0), geometry='F=40 splice=11 (14 x 11 images after the pool), bf16',
               steps=[step_ms(int(b), a.steps, a.warmup, dev) for b in a.batches.split(',')])
    for s in out['steps']:
        print(json.dumps(s))
    if not a.no_ab:
        N = out['steps'][0]['frames']
        out['layers'] = layer_ab(N, dev)
        for r in out['layers']:
            print(json.dumps(r))
    assert ops.check_async_errors(0) == 0
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
