#!/usr/bin/env python
"""Probe for label smoothing of the CTC heads (asr_ctc_loss_ls, CTC(label_smoothing_prob=...)).

    python scripts/probe_ctc_ls.py [--out profiles/ctc_ls_probe.json]

GPU.  From one process, with device events, a warm-up and medians of seven repeats that alternate the variants (the
convention of scripts/probe_residual.py):
  * one training step of bench.py's headline workload (5 x 256 BLSTM-CTC, bf16, B = 16, the same synthetic shard, the same
    step: compute_loss -> clip -> rmsprop) at label_smoothing_prob 0 and 0.2, keep_prob 1.0 and 0.8;
  * the loss call on its own at that shard's logits [T,16,62] (continuing from one ctc_head_fwd, as the step does: lse_done,
    with the bf16 image) and at C = 3387 with 4 utterances (all launches, no image): ops.ctc_loss_ex against
    ops.ctc_loss_ls, and ctc_loss_ls without a gradient; a sample is KERNEL_BATCH calls back to back between two events
    behind a busy stream, divided by the count.
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

from scripts.probe_residual import REPEATS, alternate          # noqa: E402

KERNEL_BATCH = 50
EPS = 0.2


def headline_steps(dev, keep):
    import bench
    from tensorflow_end2end_speech_recognition_amd import ops
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    from tensorflow_end2end_speech_recognition_amd.utils.training import multi_gpu
    H, L, C, D, B = 256, 5, 61, 120, 16
    x, seq_len, labels, dense = bench.make_batch(1, B, D, C + 1, 100, 778)
    xd, sld = torch.tensor(x, device=dev), torch.tensor(seq_len, device=dev)
    calls = {}
    for name, eps in (('eps0', 0.0), ('eps0.2', EPS)):
        model = CTC('blstm', D, H, L, C, parameter_init=0.1, clip_grad_norm=5.0, clip_activation=50, dtype='bf16',
                    device=dev, seed=0, label_smoothing_prob=eps)
        opt = model._set_optimizer('rmsprop', 1e-3)

        def step(model=model, opt=opt):
            loss, _ = model.compute_loss(xd, dense, sld, keep_prob=keep)
            multi_gpu.clip_and_average(model, opt, loss)
            opt.apply_gradients(None)
        calls[name] = step
    ops.reset_ctc_ls_counts(0)
    ops.reset_ctc_head_counts(0)
    med, raw = alternate(calls, warmup=5)
    counts = dict(ops.ctc_head_counts(0), **{'ls_' + k: v for k, v in ops.ctc_ls_counts(0).items()})
    return dict(workload='5x256 BLSTM-CTC bf16, B=16, T=%d, %d frames (bench.py headline shard, seed 1), keep_prob %.1f, '
                         'rmsprop' % (x.shape[1], int(seq_len.sum()), keep),
                ms_per_step=med, ratio_to_eps0=med['eps0.2'] / med['eps0'], added_us_per_step=(med['eps0.2'] - med['eps0']) * 1e3,
                calls_in_the_run=counts, ms_all=raw), x.shape[1], seq_len


def loss_calls(dev, T, seq_len, C, B, lmax, fused):
    """us per call of ctc_loss_ex / ctc_loss_ls on logits [T,B,C]; fused: behind one ctc_head_fwd (E = 512), lse_done."""
    from tensorflow_end2end_speech_recognition_amd import ops
    rng = np.random.RandomState(C)
    sl_np = np.asarray(seq_len[:B], dtype=np.int32)
    labs = [[int(v) for v in rng.randint(0, C - 1, size=min(lmax, max(1, int(n) // 4)))] for n in sl_np]
    flat = torch.tensor(np.concatenate(labs).astype(np.int32), device=dev)
    off = torch.tensor(np.concatenate([[0], np.cumsum([len(l) for l in labs])]).astype(np.int32), device=dev)
    sl = torch.tensor(sl_np, device=dev)
    lm = max(len(l) for l in labs)
    scale = 1.0 / B
    if fused:
        E = 512
        hout = torch.randn((T, B, E), device=dev).to(torch.bfloat16)
        W = torch.randn((E, C), device=dev) * 0.05
        Wt, _ = ops.ctc_head_prep(W)
        ws = ops.ctc_ls_workspace(T, B, lm, dev)
        _, logits, ninf = ops.ctc_head_fwd(hout, None, Wt, torch.zeros((C,), device=dev), C, flat, off, sl, lm, ws)
        kw = dict(ws=ws, ninf=ninf, lse_done=True)
    else:
        logits = torch.randn((T, B, C), device=dev) * 2.0
        kw = dict(ws=ops.ctc_ls_workspace(T, B, lm, dev))
    img = bool(fused)

    def ex():
        for _ in range(KERNEL_BATCH):
            ops.ctc_loss_ex(logits, flat, off, sl, lm, grad_scale=scale, want_image=img, **kw)

    def ls():
        for _ in range(KERNEL_BATCH):
            ops.ctc_loss_ls(logits, flat, off, sl, lm, EPS, grad_scale=scale, want_image=img, **kw)

    def ls_no_grad():
        for _ in range(KERNEL_BATCH):
            ops.ctc_loss_ls(logits, flat, off, sl, lm, EPS, grad_scale=scale, want_grad=False, **kw)
    big = torch.randn((8192, 8192), device=dev)
    med, raw = alternate(dict(loss_ex=ex, loss_ls=ls, loss_ls_no_grad=ls_no_grad), warmup=2,
                         blocker=lambda: torch.mm(big, big))
    us = {k: v / KERNEL_BATCH * 1e3 for k, v in med.items()}
    return dict(shape='logits [T=%d, B=%d, C=%d], %d frames, labels up to %d; %s' % (
                    T, B, C, int(sl_np.sum()), lm,
                    'continuing from ctc_head_fwd (lse_done), with the bf16 image' if fused else 'all launches, no image'),
                launches_per_sample=KERNEL_BATCH, us_per_call=us, added_us_per_call=us['loss_ls'] - us['loss_ex'],
                ratio_ls_to_ex=us['loss_ls'] / us['loss_ex'], ms_per_sample_all=raw)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=None, help='write the record to this JSON file')
    args = ap.parse_args(argv)
    dev = 'cuda:0'
    rec = dict(device=torch.cuda.get_device_name(0), repeats=REPEATS, smoothing=EPS,
               method='device events around each call, medians of %d repeats alternating the variants' % REPEATS)
    for keep in (1.0, 0.8):
        key = 'headline_train_step_keep%.1f' % keep
        rec[key], T, seq_len = headline_steps(dev, keep)
        print(json.dumps({k: rec[key][k] for k in ('ms_per_step', 'ratio_to_eps0', 'added_us_per_step', 'calls_in_the_run')}),
              flush=True)
    rec['loss_call_headline_logits'] = loss_calls(dev, T, seq_len, 62, 16, 200, fused=True)
    print(json.dumps(rec['loss_call_headline_logits']['us_per_call']), flush=True)
    rec['loss_call_C3387'] = loss_calls(dev, T, seq_len, 3387, 4, 166, fused=False)
    print(json.dumps(rec['loss_call_C3387']['us_per_call']), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(rec, f, indent=1)


if __name__ == '__main__':
    main()
