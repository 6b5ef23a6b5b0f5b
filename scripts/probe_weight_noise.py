#!/usr/bin/env python
"""Probe for the Gaussian weight noise (asr_weight_noise_perturb, CTC / AttentionSeq2Seq(weight_noise_std=...)).

    python scripts/probe_weight_noise.py [--out profiles/weight_noise_probe.json]

GPU.  From one process, with device events, a warm-up and medians of seven repeats that alternate the variants (the
convention of scripts/probe_residual.py):
  * one training step of bench.py's headline workload (5 x 256 BLSTM-CTC, bf16, B = 16, the same synthetic shard, the same
    step: compute_loss -> clip -> rmsprop) at weight_noise_std 0 and 1e-5, STEPS_PER_SAMPLE steps back to back per sample
    (one step's own scatter, a few tenths of a millisecond, is ten times the cost looked for);
  * the perturb kernel and the restore copy on their own at that model's flat buffer and at the buffer of the cfg D model
    (5 x 512 BLSTM encoder, location attention, decoder 512): a sample is KERNEL_BATCH calls back to back between two
    events behind a busy stream, divided by the count; beside each time, the rate its bytes (12 per element for the
    perturb, 8 for the restore) come to, and the largest |z_device - z| of the float64 statement over the first 2^20
    elements (tests/_weight_noise_oracle.py).
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

SIGMA = 1e-5
STEPS_PER_SAMPLE = 20


def headline_steps(dev, keep):
    import bench
    from tensorflow_end2end_speech_recognition_amd import ops
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    from tensorflow_end2end_speech_recognition_amd.utils.training import multi_gpu
    H, L, C, D, B = 256, 5, 61, 120, 16
    x, seq_len, labels, dense = bench.make_batch(1, B, D, C + 1, 100, 778)
    xd, sld = torch.tensor(x, device=dev), torch.tensor(seq_len, device=dev)
    calls, total = {}, 0
    for name, std in (('std0', 0.0), ('std1e-5', SIGMA)):
        model = CTC('blstm', D, H, L, C, parameter_init=0.1, clip_grad_norm=5.0, clip_activation=50, dtype='bf16',
                    device=dev, seed=0, weight_noise_std=std)
        opt = model._set_optimizer('rmsprop', 1e-3)
        total = model.store.total

        def steps(model=model, opt=opt):
            for _ in range(STEPS_PER_SAMPLE):
                loss, _ = model.compute_loss(xd, dense, sld, keep_prob=keep)
                multi_gpu.clip_and_average(model, opt, loss)
                opt.apply_gradients(None)
        calls[name] = steps
    ops.reset_weight_noise_counts(0)
    med, raw = alternate(calls, warmup=2)
    med = {k: v / STEPS_PER_SAMPLE for k, v in med.items()}
    return dict(workload='5x256 BLSTM-CTC bf16, B=16, T=%d, %d frames (bench.py headline shard, seed 1), keep_prob %.1f, '
                         'rmsprop' % (x.shape[1], int(seq_len.sum()), keep),
                flat_elements=total, ms_per_step=med, ratio_to_std0=med['std1e-5'] / med['std0'],
                added_us_per_step=(med['std1e-5'] - med['std0']) * 1e3, calls_in_the_run=ops.weight_noise_counts(0),
                steps_per_sample=STEPS_PER_SAMPLE, ms_per_sample_all=raw), total


def cfg_d_elements(dev):
    from tensorflow_end2end_speech_recognition_amd.models.attention.joint_ctc_attention import JointCTCAttention
    C = 28
    m = JointCTCAttention(input_size=240, encoder_type='blstm', encoder_num_units=512, encoder_num_layers=5,
                          encoder_num_proj=None, attention_type='location', attention_dim=128, decoder_type='lstm',
                          decoder_num_units=512, decoder_num_layers=1, embedding_dim=64, lambda_weight=0.5, num_classes=C,
                          sos_index=C, eos_index=C + 1, max_decode_length=402, parameter_init=0.1, clip_grad_norm=5.0,
                          clip_activation_encoder=50, clip_activation_decoder=50, dtype='bf16', seed=5, device=dev)
    return m.store.total


def kernel_alone(dev, n, label):
    from tensorflow_end2end_speech_recognition_amd import ops
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import _weight_noise_oracle as own
    w = torch.randn(n, device=dev) * 0.1
    backup = torch.empty_like(w)

    def perturb():
        for i in range(KERNEL_BATCH):
            ops.weight_noise_perturb(w, backup, SIGMA, 7, (i + 1) << 40)

    def restore():
        for _ in range(KERNEL_BATCH):
            w.copy_(backup)
    big = torch.randn((8192, 8192), device=dev)
    med, raw = alternate(dict(perturb=perturb, restore=restore), warmup=2, blocker=lambda: torch.mm(big, big))
    us = {k: v / KERNEL_BATCH * 1e3 for k, v in med.items()}
    m = min(n, 1 << 20)
    z0 = torch.zeros(m, device=dev)
    ops.weight_noise_perturb(z0, torch.empty_like(z0), 1.0, 1234, (3 << 40) + (2 << 32))
    err = float(np.abs(z0.cpu().numpy().astype(np.float64) - own.z(m, 1234, (3 << 40) + (2 << 32))).max())
    return dict(buffer=label, elements=n, megabytes=n * 4 / 1e6, launches_per_sample=KERNEL_BATCH, us_per_call=us,
                tb_per_s=dict(perturb=12.0 * n / us['perturb'] / 1e6, restore=8.0 * n / us['restore'] / 1e6),
                max_abs_z_error_first_2e20=err, ms_per_sample_all=raw)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=None, help='write the record to this JSON file')
    args = ap.parse_args(argv)
    dev = 'cuda:0'
    rec = dict(device=torch.cuda.get_device_name(0), repeats=REPEATS, weight_noise_std=SIGMA,
               method='device events around each call, medians of %d repeats alternating the variants' % REPEATS)
    rec['headline_train_step'], total = headline_steps(dev, 0.8)
    print(json.dumps({k: rec['headline_train_step'][k] for k in ('ms_per_step', 'ratio_to_std0', 'added_us_per_step',
                                                                 'calls_in_the_run')}), flush=True)
    for key, n, label in (('kernel_headline_buffer', total, 'the 5x256 CTC model'),
                          ('kernel_cfgD_buffer', cfg_d_elements(dev), 'the cfg D joint model (5x512, location, U=512)')):
        rec[key] = kernel_alone(dev, n, label)
        print(json.dumps({k: rec[key][k] for k in ('elements', 'us_per_call', 'tb_per_s', 'max_abs_z_error_first_2e20')}),
              flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(rec, f, indent=1)


if __name__ == '__main__':
    main()
