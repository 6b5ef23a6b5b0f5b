#!/usr/bin/env python
"""Probe for scheduled sampling and label smoothing in the attention decoder (asr_att_decoder_fwd_ss, asr_seq_xent_ls).

    python scripts/probe_sched_sampling.py [--out profiles/sched_sampling_probe.json]
    python scripts/probe_sched_sampling.py --seeds            (CPU)

GPU.  From one process, with device events, a warm-up and medians of seven repeats that alternate the variants:
  * one training step of bench.py's cfg D shard (5 x 512 BLSTM joint CTC-attention, location, bf16, B = 32, dropout 0.2,
    adam) at scheduled_sampling_prob 0 -- the teacher-forced path -- against 0.2, on one model; host time of compute_loss
    per variant beside it (perf_counter around the call, no synchronisation: how long the host takes to enqueue the step);
  * the entry points a p = 0 step calls, counted by name, against those of a step that does not pass the keyword at all:
    the same multiset, nothing of the new path in it (the check that p = 0 costs nothing is this count, not a time);
  * asr_seq_xent against asr_seq_xent_ls at that shard's rows (decoder steps x 32) and classes (30): a sample is
    KERNEL_BATCH launches back to back between two events behind a blocker, divided by the count.

--seeds (CPU, no kernels): the seed search behind tests/test_gpu_sched_sampling.py's model cases.  For every case and
candidate model seed the float64 statement (tests/_cpu_ops_att_ss.ss_model_forward) is rolled out from its own argmax under
every draw set and under three Bernoulli(0.5) tables, and the share of sampled live positions whose top-two margin is at most
the case's margin (10 x its logits bar) is printed; the test keeps a seed with at most 5 % in each.
"""
import argparse
import collections
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

REPEATS = 7
KERNEL_BATCH = 100


def alternate(calls, repeats=REPEATS, warmup=2, blocker=None):
    """{name: median ms} of the callables, run alternately `repeats` times after `warmup` rounds (scripts/probe_subsample.py)."""
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


def cfgd(dev):
    import bench
    from tensorflow_end2end_speech_recognition_amd.models.attention.joint_ctc_attention import JointCTCAttention
    seed, D, C, B, H, L, U, A, Em = 3, 240, 28, 32, 512, 5, 512, 128, 64
    rng = np.random.RandomState(seed)
    seq_len = rng.randint(100, 1601, size=B).astype(np.int32)
    lens = np.maximum(1, seq_len // 4)
    Lmax = int(lens.max()) + 2
    labels = np.full((B, Lmax), C + 1, dtype=np.int64)
    ctc = np.full((B, int(lens.max())), -1, dtype=np.int64)
    for b in range(B):
        y = rng.randint(0, C, size=lens[b])
        labels[b, 0] = C
        labels[b, 1:1 + lens[b]] = y
        ctc[b, :lens[b]] = y
    xd = bench.device_features(seed, seq_len, D, torch.device(dev))
    model = JointCTCAttention(input_size=D, encoder_type='blstm', encoder_num_units=H, encoder_num_layers=L,
                              encoder_num_proj=None, attention_type='location', attention_dim=A, decoder_type='lstm',
                              decoder_num_units=U, decoder_num_layers=1, embedding_dim=Em, lambda_weight=0.5, num_classes=C,
                              sos_index=C, eos_index=C + 1, max_decode_length=Lmax, parameter_init=0.1, clip_grad_norm=5.0,
                              clip_activation_encoder=50, clip_activation_decoder=50, dtype='bf16', seed=5, device=dev)
    return model, (xd, labels, ctc, seq_len, lens + 2), Lmax - 1, C + 2


def train_steps(model, batch):
    host = collections.defaultdict(list)

    def make(name, kw):
        def step():
            t0 = time.perf_counter()
            loss, *_ = model.compute_loss(*batch, 0.8, 0.8, 0.8, **kw)
            host[name].append((time.perf_counter() - t0) * 1e3)
            model.train(loss, 'adam', 1e-3)
        return step
    calls = {'p0': make('p0', dict(scheduled_sampling_prob=0.0)), 'p0.2': make('p0.2', dict(scheduled_sampling_prob=0.2))}
    med, raw = alternate(calls, warmup=3)
    host_med = {k: float(np.median(v[-REPEATS:])) for k, v in host.items()}
    return dict(ms_per_step=med, ratio_to_p0=med['p0.2'] / med['p0'], host_ms_compute_loss=host_med, ms_all=raw)


def entry_point_counts(model, batch):
    """Entry points called (by the name every call is checked under) during one compute_loss + train."""
    from tensorflow_end2end_speech_recognition_amd import _lib
    real = _lib.Handle.check
    seen = collections.Counter()

    def check(self, rc, what):
        seen[what] += 1
        return real(self, rc, what)
    out = {}
    _lib.Handle.check = check
    try:
        for name, kw in (('no_keyword', {}), ('p0', dict(scheduled_sampling_prob=0.0)), ('p0.2', dict(scheduled_sampling_prob=0.2))):
            seen.clear()
            loss, *_ = model.compute_loss(*batch, 0.8, 0.8, 0.8, **kw)
            model.train(loss, 'adam', 1e-3)
            torch.cuda.synchronize()
            out[name] = dict(seen)
    finally:
        _lib.Handle.check = real
    new = ('asr_att_decoder_fwd_ss', 'asr_seq_xent_ls')
    same = out['p0'] == out['no_keyword'] and not any(n in out['p0'] for n in new)
    diff = {k: out['p0.2'].get(k, 0) - out['p0'].get(k, 0) for k in set(out['p0']) | set(out['p0.2'])
            if out['p0.2'].get(k, 0) != out['p0'].get(k, 0)}
    return dict(p0_equals_call_without_keyword=bool(same), entry_calls_p0=sum(out['p0'].values()),
                entry_calls_p02=sum(out['p0.2'].values()), p02_minus_p0=diff)


def xent_kernels(dev, rows, Cc):
    from tensorflow_end2end_speech_recognition_amd import ops
    x = torch.randn((rows, Cc), device=dev)
    tg = torch.randint(0, Cc, (rows,), device=dev, dtype=torch.int32)
    w = (torch.rand((rows,), device=dev) < 0.5).float()

    def plain():
        for _ in range(KERNEL_BATCH):
            ops.seq_xent(x, tg, w, 1e-10, 1.0)

    def smoothed():
        for _ in range(KERNEL_BATCH):
            ops.seq_xent(x, tg, w, 1e-10, 1.0, smoothing=0.2)
    big = torch.randn((8192, 8192), device=dev)
    med, raw = alternate({'seq_xent': plain, 'seq_xent_ls': smoothed}, blocker=lambda: torch.mm(big, big))
    return dict(shape='logits [%d, %d] fp32, half of the rows masked; loss and gradient' % (rows, Cc),
                launches_per_sample=KERNEL_BATCH, us_per_call={k: v / KERNEL_BATCH * 1e3 for k, v in med.items()},
                ms_per_sample_all=raw)


def seed_search(seeds):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import _cpu_ops_att_ss as ss
    import test_gpu_sched_sampling as tg
    for case in sorted(tg._MODEL_CASES):
        att, dtype, joint, _ = tg._MODEL_CASES[case]
        for seed in seeds:
            tg._MODEL_CASES[case] = (att, dtype, joint, seed)
            model, (x, sl, labels, lsl, ctc), stmt, _ = tg.model_case(case, 'cpu')
            sd = {k: v.numpy() for k, v in model.store.state_dict().items()}
            B, To = x.shape[0], int(lsl.max()) - 1
            tables = [np.ones((B, To))] + [np.random.RandomState(s).rand(B, To) < 0.5 for s in (1, 2, 3)]
            shares = []
            for draw in tables:
                ref = ss.ss_model_forward(sd, x, labels, sl, lsl, 1, att, draw=draw, smoothing=0.1,
                                          ctc_labels=[[int(v) for v in r if v >= 0] for r in ctc] if joint else None,
                                          lambda_weight=0.5 if joint else None, **stmt)
                bar = 2e-4 if dtype == 'f32' else 3e-2 * max(1.0, float(np.abs(ref['logits']).max()))
                samp = ss.sampled_positions(draw, ref['live'])
                shares.append('%d/%d' % (int((samp & (ref['margin'] <= 10 * bar)).sum()), int(samp.sum())))
            print('%-20s seed %d  under the margin (all draws, three Bernoulli tables): %s' % (case, seed, '  '.join(shares)),
                  flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=None, help='write the record to this JSON file')
    ap.add_argument('--seeds', nargs='*', type=int, default=None, help='CPU: the seed search of the GPU test (default 5 6 7)')
    args = ap.parse_args(argv)
    if args.seeds is not None:
        return seed_search(args.seeds or [5, 6, 7])
    dev = 'cuda:0'
    rec = dict(device=torch.cuda.get_device_name(0), repeats=REPEATS,
               method='device events around each call, medians of %d repeats alternating the variants' % REPEATS)
    model, batch, To, C2 = cfgd(dev)
    rec['workload'] = ('cfg D shard: 5x512 BLSTM joint CTC-attention (location, A=128, U=512, E=64, C=28, lambda 0.5), bf16, '
                       'B=32, %d decoder steps, dropout 0.2, adam, train step' % To)
    rec['entry_points'] = entry_point_counts(model, batch)
    print(json.dumps(rec['entry_points']), flush=True)
    rec['train_step'] = train_steps(model, batch)
    print(json.dumps({k: rec['train_step'][k] for k in ('ms_per_step', 'ratio_to_p0', 'host_ms_compute_loss')}), flush=True)
    rec['xent_kernels'] = xent_kernels(dev, To * 32, C2)
    print(json.dumps(rec['xent_kernels']['us_per_call']), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(rec, f, indent=1)


if __name__ == '__main__':
    main()
