#!/usr/bin/env python
"""Probe for the on-device input augmentation (asr_input_augment, CTC / AttentionSeq2Seq(input_noise_std=...,
freq_mask_*=..., time_mask_*=...)).

    python scripts/probe_input_aug.py [--out profiles/input_aug_probe.json]

GPU.  From one process, with device events, a warm-up and medians of seven repeats that alternate the variants (the
convention of scripts/probe_weight_noise.py):
  * one training step of bench.py's headline workload (5 x 256 BLSTM-CTC, bf16, B = 16, the same synthetic shard, the same
    step: compute_loss -> clip -> rmsprop) with the augmentation off and on (noise 0.075, 2 x 6 frequency masks, 2 x 20
    time masks at ratio 0.2), STEPS_PER_SAMPLE steps back to back per sample;
  * the kernel on its own at [16, T, 123] (T and the lengths of that shard; 41 base channels) for noise only, masks only,
    both, and the all-off copy: a sample is KERNEL_BATCH calls back to back between two events behind a busy stream,
    divided by the count; beside each time, the rate its bytes come to -- 8 per element, a read and a write, for all of
    them: padded and masked frames are skipped by the noise generator, not by the copy -- and the share of elements that
    draw noise.
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

from scripts.probe_residual import KERNEL_BATCH, REPEATS, alternate          # noqa: E402

STEPS_PER_SAMPLE = 20
NOISE = 0.075
FREQ = (2, 6)
TIME = (2, 20, 0.2)
AUG = dict(input_noise_std=NOISE, freq_mask_num=FREQ[0], freq_mask_width=FREQ[1], time_mask_num=TIME[0],
           time_mask_width=TIME[1], time_mask_ratio=TIME[2])


def headline_steps(dev, keep):
    import bench
    from tensorflow_end2end_speech_recognition_amd import ops
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    from tensorflow_end2end_speech_recognition_amd.utils.training import multi_gpu
    H, L, C, D, B = 256, 5, 61, 120, 16
    x, seq_len, labels, dense = bench.make_batch(1, B, D, C + 1, 100, 778)
    xd, sld = torch.tensor(x, device=dev), torch.tensor(seq_len, device=dev)
    calls = {}
    for name, kw in (('off', {}), ('on', AUG)):
        model = CTC('blstm', D, H, L, C, parameter_init=0.1, clip_grad_norm=5.0, clip_activation=50, dtype='bf16',
                    device=dev, seed=0, **kw)
        opt = model._set_optimizer('rmsprop', 1e-3)

        def steps(model=model, opt=opt):
            for _ in range(STEPS_PER_SAMPLE):
                loss, _ = model.compute_loss(xd, dense, sld, keep_prob=keep)
                multi_gpu.clip_and_average(model, opt, loss)
                opt.apply_gradients(None)
        calls[name] = steps
    ops.reset_input_augment_counts(0)
    med, raw = alternate(calls, warmup=2)
    med = {k: v / STEPS_PER_SAMPLE for k, v in med.items()}
    return dict(workload='5x256 BLSTM-CTC bf16, B=16, T=%d, D=%d, %d frames (bench.py headline shard, seed 1), keep_prob '
                         '%.1f, rmsprop' % (x.shape[1], D, int(seq_len.sum()), keep),
                settings=AUG, ms_per_step=med, ratio_to_off=med['on'] / med['off'],
                added_us_per_step=(med['on'] - med['off']) * 1e3, calls_in_the_run=ops.input_augment_counts(0),
                steps_per_sample=STEPS_PER_SAMPLE, ms_per_sample_all=raw), x.shape[1], seq_len


def kernel_alone(dev, T, seq_len):
    from tensorflow_end2end_speech_recognition_amd import ops
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import _input_aug_oracle as iao
    B, F, n_ch = 16, 123, 41
    n = B * T * F
    x = torch.randn((B, T, F), device=dev)
    y = torch.empty_like(x)
    sl = torch.tensor(seq_len, device=dev, dtype=torch.int32)
    variants = dict(noise=dict(noise_std=NOISE), masks=dict(freq_masks=FREQ, time_masks=TIME),
                    both=dict(noise_std=NOISE, freq_masks=FREQ, time_masks=TIME), all_off_copy={})
    calls = {}
    for name, kw in variants.items():
        def run(kw=kw):
            for i in range(KERNEL_BATCH):
                ops.input_augment(x, sl, n_ch, seed=7, offset=(i + 1) << 40, out=y, **kw)
        calls[name] = run
    big = torch.randn((8192, 8192), device=dev)
    med, raw = alternate(calls, warmup=2, blocker=lambda: torch.mm(big, big))
    us = {k: v / KERNEL_BATCH * 1e3 for k, v in med.items()}
    valid, masked, _, _ = iao.cover((B, T, F), seq_len, n_ch, FREQ, TIME, 7, 1 << 40)
    valid_share = float(np.broadcast_to(valid, (B, T, F)).mean())
    return dict(shape=[B, T, F], elements=n, megabytes=n * 4 / 1e6, launches_per_sample=KERNEL_BATCH, us_per_call=us,
                tb_per_s_of_8_bytes_per_element={k: 8.0 * n / v / 1e6 for k, v in us.items()},
                share_of_elements_that_draw_noise=dict(noise=valid_share,
                                                       both=float((np.broadcast_to(valid, (B, T, F)) & ~masked).mean())),
                share_masked_at_offset_1=float(masked.mean()), ms_per_sample_all=raw)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=None, help='write the record to this JSON file')
    args = ap.parse_args(argv)
    dev = 'cuda:0'
    rec = dict(device=torch.cuda.get_device_name(0), repeats=REPEATS,
               method='device events around each call, medians of %d repeats alternating the variants' % REPEATS)
    rec['headline_train_step'], T, seq_len = headline_steps(dev, 0.8)
    print(json.dumps({k: rec['headline_train_step'][k] for k in ('ms_per_step', 'ratio_to_off', 'added_us_per_step',
                                                                 'calls_in_the_run')}), flush=True)
    rec['kernel_alone'] = kernel_alone(dev, T, seq_len)
    print(json.dumps({k: rec['kernel_alone'][k] for k in ('shape', 'us_per_call', 'tb_per_s_of_8_bytes_per_element',
                                                          'share_of_elements_that_draw_noise')}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(rec, f, indent=1)


if __name__ == '__main__':
    main()
