#!/usr/bin/env python
"""Probe for time subsampling inside the BLSTM encoder (models/encoders/core/subsample.py, csrc/subsample.hip).

    python scripts/probe_subsample.py [--out profiles/subsample_probe.json]

GPU.  From one process, with device events, a warm-up and medians of seven repeats that alternate the variants:
  * one training step of bench.py's headline workload (5 x 256 BLSTM-CTC, bf16, B = 16, the same synthetic shard, the
    same step: compute_loss -> clip -> rmsprop) for the plain model and for subsample_list [F,T,F,F,F] with
    subsample_type drop and concat;
  * the two subsample kernels on their own, at the shape of that model's one boundary (time_subsample_fwd on the bf16
    [T,16,512] output of layer 2, time_subsample_bwd on the fp32 gradient), per type: a sample is KERNEL_BATCH launches
    back to back between two events, divided by the count (one launch of a few microseconds between two events would
    measure the launch, not the kernel);
  * greedy infer of bench.py's cfg D (5 x 512 BLSTM joint CTC-attention, location, B = 32) for the same three variants.
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
LIST = [False, True, False, False, False]
VARIANTS = (('plain', None, 'drop'), ('drop', LIST, 'drop'), ('concat', LIST, 'concat'))


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


def headline_steps(dev):
    import bench
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    from tensorflow_end2end_speech_recognition_amd.utils.training import multi_gpu
    H, L, C, D, B = 256, 5, 61, 120, 16
    x, seq_len, labels, dense = bench.make_batch(1, B, D, C + 1, 100, 778)
    xd, sld = torch.tensor(x, device=dev), torch.tensor(seq_len, device=dev)
    calls = {}
    for name, lst, kind in VARIANTS:
        model = CTC('blstm', D, H, L, C, parameter_init=0.1, clip_grad_norm=5.0, clip_activation=50, dtype='bf16',
                    device=dev, seed=0, subsample_list=lst, subsample_type=kind)
        opt = model._set_optimizer('rmsprop', 1e-3)

        def step(model=model, opt=opt):
            loss, _ = model.compute_loss(xd, dense, sld, keep_prob=0.8)
            multi_gpu.clip_and_average(model, opt, loss)
            opt.apply_gradients(None)
        calls[name] = step
    med, raw = alternate(calls, warmup=5)
    return dict(workload='5x256 BLSTM-CTC bf16, B=16, T=%d, %d frames (bench.py headline shard, seed 1), keep_prob 0.8, '
                         'rmsprop; subsample_list %s' % (x.shape[1], int(seq_len.sum()), LIST),
                ms_per_step=med, ratio_to_plain={k: med[k] / med['plain'] for k in med}, ms_all=raw), x.shape[1], seq_len


def boundary_kernels(dev, T, seq_len):
    from tensorflow_end2end_speech_recognition_amd import ops
    Bp, W = 16, 512
    x = torch.randn((T, Bp, W), device=dev).to(torch.bfloat16)
    sl = torch.tensor(seq_len, device=dev, dtype=torch.int32)
    calls = {}
    for kind in ('drop', 'concat'):
        y, lo = ops.time_subsample_fwd(x, sl, Bp, kind)
        dy = torch.randn((T // 2, Bp, y.shape[2]), device=dev)
        dx = torch.empty((T, Bp, W), device=dev)

        def fwd(kind=kind):
            for _ in range(KERNEL_BATCH):
                ops.time_subsample_fwd(x, sl, Bp, kind)

        def bwd(kind=kind, dy=dy, lo=lo, dx=dx):
            for _ in range(KERNEL_BATCH):
                ops.time_subsample_bwd(dy, lo, T, kind, out=dx)
        calls['fwd_' + kind], calls['bwd_' + kind] = fwd, bwd
    big = torch.randn((8192, 8192), device=dev)                 # ~10 ms of fp32 matrix product: the host enqueues a sample
    med, raw = alternate(calls, warmup=2, blocker=lambda: torch.mm(big, big))     # (~2 ms of launches) behind it
    med = {k: v / KERNEL_BATCH for k, v in med.items()}
    mb = dict(fwd_drop=(T // 2) * Bp * W * (2 + 4), fwd_concat=(T // 2) * Bp * W * 2 * (2 + 4),
              bwd_drop=T * Bp * W * 4 + (T // 2) * Bp * W * 4, bwd_concat=T * Bp * W * 4 * 2)
    return dict(shape='x [T=%d, Bp=16, W=512] bf16 -> y fp32; dy fp32 -> dx [T,16,512] fp32 (upper bounds on the bytes: '
                      'padded frames are neither read nor, in y, more than zero-filled)' % T,
                launches_per_sample=KERNEL_BATCH, us_per_call={k: v * 1e3 for k, v in med.items()},
                gb_per_s_upper={k: mb[k] / (med[k] * 1e-3) / 1e9 for k in med}, ms_per_sample_all=raw)


def cfgd_infer(dev):
    import bench
    from tensorflow_end2end_speech_recognition_amd.models.attention.joint_ctc_attention import JointCTCAttention
    seed, D, C, B, H, L, U, A, Em = 3, 240, 28, 32, 512, 5, 512, 128, 64
    rng = np.random.RandomState(seed)
    seq_len = rng.randint(100, 1601, size=B).astype(np.int32)
    Lmax = int(np.maximum(1, seq_len // 4).max()) + 2
    xd = bench.device_features(seed, seq_len, D, torch.device(dev))
    calls, steps = {}, {}
    for name, lst, kind in VARIANTS:
        model = JointCTCAttention(input_size=D, encoder_type='blstm', encoder_num_units=H, encoder_num_layers=L,
                                  encoder_num_proj=None, attention_type='location', attention_dim=A, decoder_type='lstm',
                                  decoder_num_units=U, decoder_num_layers=1, embedding_dim=Em, lambda_weight=0.5,
                                  num_classes=C, sos_index=C, eos_index=C + 1, max_decode_length=Lmax, parameter_init=0.1,
                                  clip_grad_norm=5.0, clip_activation_encoder=50, clip_activation_decoder=50,
                                  dtype='bf16', seed=5, device=dev, subsample_list=lst, subsample_type=kind)

        def run(model=model, name=name):
            ids = model.infer(xd, seq_len)
            steps[name] = int(ids.shape[1])
        calls[name] = run
    med, raw = alternate(calls, warmup=1)
    return dict(workload='cfg D: 5x512 BLSTM joint CTC-attention (location), bf16, B=32, T=%d, greedy infer with freshly '
                         'initialised weights, max_decode_length %d; subsample_list %s' % (int(seq_len.max()), Lmax, LIST),
                ms_per_call=med, ratio_to_plain={k: med[k] / med['plain'] for k in med}, decoded_steps=steps, ms_all=raw)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=None, help='write the record to this JSON file')
    ap.add_argument('--skip-infer', action='store_true')
    args = ap.parse_args(argv)
    dev = 'cuda:0'
    rec = dict(device=torch.cuda.get_device_name(0), repeats=REPEATS,
               method='device events around each call, medians of %d repeats alternating the variants' % REPEATS)
    rec['headline_train_step'], T, seq_len = headline_steps(dev)
    print(json.dumps({k: rec['headline_train_step'][k] for k in ('ms_per_step', 'ratio_to_plain')}), flush=True)
    rec['boundary_kernels'] = boundary_kernels(dev, T, seq_len)
    print(json.dumps(rec['boundary_kernels']['us_per_call']), flush=True)
    if not args.skip_infer:
        rec['cfgD_greedy_infer'] = cfgd_infer(dev)
        print(json.dumps({k: rec['cfgD_greedy_infer'][k] for k in ('ms_per_call', 'ratio_to_plain')}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(rec, f, indent=1)


if __name__ == '__main__':
    main()
