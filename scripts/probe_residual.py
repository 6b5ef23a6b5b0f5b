#!/usr/bin/env python
"""Probe for the skip connections between the BLSTM encoder's layers (models/encoders/core/residual.py,
csrc/residual.hip).

    python scripts/probe_residual.py [--out profiles/residual_probe.json]

GPU.  From one process, with device events, a warm-up and medians of seven repeats that alternate the variants:
  * one training step of bench.py's headline workload (5 x 256 BLSTM-CTC, bf16, B = 16, the same synthetic shard, the
    same step: compute_loss -> clip -> rmsprop) for the plain model, encoder_residual and encoder_dense_residual, at
    keep_prob 1.0 and 0.8;
  * the two kernels on their own at that model's layer boundary ([T,16,512]: residual_fwd on the bf16 output of a layer
    with a bf16 skip, and with the fp32 running sum updated in place; residual_bwd in place, both modes), with and
    without a dropout descriptor: a sample is KERNEL_BATCH launches back to back between two events behind a busy
    stream, divided by the count.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

REPEATS = 7
KERNEL_BATCH = 100
VARIANTS = (('plain', {}), ('residual', dict(encoder_residual=True)), ('dense', dict(encoder_dense_residual=True)))


def alternate(calls, repeats=REPEATS, warmup=2, blocker=None):
    """{name: median ms} of the callables, run alternately `repeats` times after `warmup` rounds.  blocker: called before
    the first event of every sample (device work that keeps the stream busy while the host enqueues the sample)."""
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in calls}
    for _ in range(repeats):
        for k, fn in calls.items():
            if blocker is not None:
                blocker()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    return {k: float(np.median(v)) for k, v in times.items()}, {k: [round(t, 4) for t in v] for k, v in times.items()}


def headline_steps(dev, keep):
    import bench
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    from tensorflow_end2end_speech_recognition_amd.utils.training import multi_gpu
    H, L, C, D, B = 256, 5, 61, 120, 16
    x, seq_len, labels, dense = bench.make_batch(1, B, D, C + 1, 100, 778)
    xd, sld = torch.tensor(x, device=dev), torch.tensor(seq_len, device=dev)
    calls = {}
    for name, kw in VARIANTS:
        model = CTC('blstm', D, H, L, C, parameter_init=0.1, clip_grad_norm=5.0, clip_activation=50, dtype='bf16',
                    device=dev, seed=0, **kw)
        opt = model._set_optimizer('rmsprop', 1e-3)

        def step(model=model, opt=opt):
            loss, _ = model.compute_loss(xd, dense, sld, keep_prob=keep)
            multi_gpu.clip_and_average(model, opt, loss)
            opt.apply_gradients(None)
        calls[name] = step
    med, raw = alternate(calls, warmup=5)
    return dict(workload='5x256 BLSTM-CTC bf16, B=16, T=%d, %d frames (bench.py headline shard, seed 1), keep_prob %.1f, '
                         'rmsprop' % (x.shape[1], int(seq_len.sum()), keep),
                ms_per_step=med, ratio_to_plain={k: med[k] / med['plain'] for k in med}, ms_all=raw), x.shape[1], seq_len


def boundary_kernels(dev, T, seq_len):
    from tensorflow_end2end_speech_recognition_amd import ops
    Bp, W = 16, 512
    n = T * Bp * W
    h = torch.randn((T, Bp, W), device=dev).to(torch.bfloat16)
    skip = torch.randn((T, Bp, W), device=dev).to(torch.bfloat16)
    sl = torch.tensor(seq_len, device=dev, dtype=torch.int32)
    out = torch.empty_like(h)
    S = torch.zeros((T, Bp, W), device=dev)
    dx, carry = torch.zeros((T, Bp, W), device=dev), torch.zeros((T, Bp, W), device=dev)
    calls, nbytes = {}, {}
    for tag, drop in (('keep1', None), ('keep0.8', (0.8, 1, 1 << 40))):
        def fwd(drop=drop):
            for _ in range(KERNEL_BATCH):
                ops.residual_fwd(h, skip, sl, drop, out=out)

        def fwd_sum(drop=drop):
            for _ in range(KERNEL_BATCH):
                ops.residual_fwd(h, S, sl, drop, sum_out=S, out=out)

        def bwd(drop=drop):
            for _ in range(KERNEL_BATCH):
                ops.residual_bwd(dx, carry, sl, drop, False, dout=dx, carry_out=carry)

        def bwd_dense(drop=drop):
            for _ in range(KERNEL_BATCH):
                ops.residual_bwd(dx, carry, sl, drop, True, dout=dx, carry_out=carry)
        calls['fwd_' + tag], calls['fwd_sum_' + tag] = fwd, fwd_sum
        calls['bwd_' + tag], calls['bwd_dense_' + tag] = bwd, bwd_dense
        nbytes.update({'fwd_' + tag: n * (2 + 2 + 2), 'fwd_sum_' + tag: n * (2 + 4 + 2 + 4),
                       'bwd_' + tag: n * 16, 'bwd_dense_' + tag: n * 16})
    big = torch.randn((8192, 8192), device=dev)                 # ~10 ms of fp32 matrix product: the host enqueues a sample
    med, raw = alternate(calls, warmup=2, blocker=lambda: torch.mm(big, big))     # (~2 ms of launches) behind it
    med = {k: v / KERNEL_BATCH for k, v in med.items()}
    return dict(shape='[T=%d, Bp=16, W=512]: h, skip, out bf16 (fwd), S fp32 in place (fwd_sum); dx_raw, carry fp32 in place '
                      '(bwd); upper bounds on the bytes: padded frames are not read, only zero-filled' % T,
                launches_per_sample=KERNEL_BATCH, us_per_call={k: v * 1e3 for k, v in med.items()},
                gb_per_s_upper={k: nbytes[k] / (med[k] * 1e-3) / 1e9 for k in med}, ms_per_sample_all=raw)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=None, help='write the record to this JSON file')
    args = ap.parse_args(argv)
    dev = 'cuda:0'
    rec = dict(device=torch.cuda.get_device_name(0), repeats=REPEATS,
               method='device events around each call, medians of %d repeats alternating the variants' % REPEATS)
    for keep in (1.0, 0.8):
        key = 'headline_train_step_keep%.1f' % keep
        rec[key], T, seq_len = headline_steps(dev, keep)
        print(json.dumps({k: rec[key][k] for k in ('ms_per_step', 'ratio_to_plain')}), flush=True)
    rec['boundary_kernels'] = boundary_kernels(dev, T, seq_len)
    print(json.dumps(rec['boundary_kernels']['us_per_call']), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(rec, f, indent=1)


if __name__ == '__main__':
    main()
