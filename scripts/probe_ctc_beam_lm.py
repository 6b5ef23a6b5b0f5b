#!/usr/bin/env python
"""Probes for the CTC prefix beam search with LM fusion (models/ctc/decoders/charlm_beam_search_decoder.py,
csrc/ctc_beam_lm.hip).

    python scripts/probe_ctc_beam_lm.py           GPU: us per frame of asr_ctc_beam_decode_lm at C = 62, W = 20, B = 1 and
                                                  B = 16 with a 2 x 256 LSTM LM (V = 63), of the same call without an LM
                                                  (insertion bonus only: the frame kernels alone) and of asr_ctc_beam_decode
                                                  at the same shapes from the same process -- device events, a warm-up,
                                                  medians of seven repeats alternating the three, T = 400 against T = 100 so
                                                  that what does not scale with the frames cancels; the ratio to
                                                  asr_ctc_beam_decode and the share of a frame spent in the LM launches
                                                  (reorder, step, commit) = 1 - frames alone / fused
    python scripts/probe_ctc_beam_lm.py --seeds   CPU: seeds of the native-call test whose float64 margin is >= MARGIN
    python scripts/probe_ctc_beam_lm.py --bound   CPU: largest error of the float32 LM emulation against the statement
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

MARGIN = 1e-3            # 10 x the tests' 1e-4 bound


def find_seeds():
    import _cpu_ops_ctc_lm as K
    found = {}
    for C, B, W in K.LOOP_CASES:
        for clip in K.LOOP_CLIPS:
            for seed in range(200):
                case = K.loop_case(C, B, W, clip, seed)
                lab, _, _, margin = K.loop_statement(case, W, K.LOOP_ALPHA, K.LOOP_BETA)
                if margin >= MARGIN and all(len(l) > 0 for l in lab):
                    found[(C, B, W, clip)] = seed
                    break
            print('loop', (C, B, W, clip), found.get((C, B, W, clip)), flush=True)
    print('LOOP_SEEDS =', found)


def bound():
    import _cpu_ops_ctc_lm as K
    worst = 0.0
    for (C, B, W, clip), seed in sorted(K.LOOP_SEEDS.items()):
        e = K.emulation_error(K.loop_case(C, B, W, clip, seed), W, K.LOOP_ALPHA, K.LOOP_BETA)
        print('C=%d B=%d W=%d clip=%g: emulation error %.3g' % (C, B, W, clip, e), flush=True)
        worst = max(worst, e)
    print('largest emulated error %.3g; 4 x = %.3g; bound = %.3g' % (worst, 4 * worst, max(1e-4, 4 * worst)))


def measure(out_path):
    from tensorflow_end2end_speech_recognition_amd import ops
    from tensorflow_end2end_speech_recognition_amd.models.lm.base import RNNLM
    dev = 'cuda:0'
    C, W = 62, 20
    lm = RNNLM(num_classes=C + 1, embedding_dim=64, num_units=256, num_layers=2, sos_index=C, eos_index=C - 1, seed=11,
               device=dev)
    lmw = dict(lm.decode_weights(), eos=lm.eos_index)
    rec = dict(config='C=62, W=20, LM 2x256 fp32 (V=63), lm_weight 0.5, insertion_bonus 0.2; peaked posteriors (scale 3)',
               rows=[])
    for B in (1, 16):
        data = {}
        for T in (100, 400):
            rng = np.random.RandomState(T + B)
            data[T] = (torch.tensor((rng.randn(T, B, C) * 3.0).astype(np.float32), device=dev),
                       torch.full((B,), T, dtype=torch.int32, device=dev))
        calls = dict(fused=lambda x, s: ops.ctc_beam_decode_lm(x, s, W, lm=lmw, lm_weight=0.5, insertion_bonus=0.2),
                     frames_only=lambda x, s: ops.ctc_beam_decode_lm(x, s, W, insertion_bonus=0.2),
                     plain=lambda x, s: ops.ctc_beam_decode(x, s, W))
        times = {(k, T): [] for k in calls for T in data}
        for k, fn in calls.items():                                              # warm-up of every shape
            for T in data:
                fn(*data[T])
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(7):
            for T in data:
                for k, fn in calls.items():
                    e0.record()
                    fn(*data[T])
                    e1.record()
                    torch.cuda.synchronize()
                    times[(k, T)].append(e0.elapsed_time(e1))
        med = {k: float(np.median(v)) for k, v in times.items()}
        us = {k: (med[(k, 400)] - med[(k, 100)]) / 300.0 * 1e3 for k in calls}
        r = dict(B=B, us_per_frame_fused=us['fused'], us_per_frame_frames_only=us['frames_only'],
                 us_per_frame_ctc_beam_decode=us['plain'], ratio_fused_to_ctc_beam_decode=us['fused'] / us['plain'],
                 lm_launch_share=1.0 - us['frames_only'] / us['fused'],
                 ms={'%s_T%d' % k: v for k, v in med.items()})
        rec['rows'].append(r)
        print(json.dumps(r), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, 'w') as f:
            json.dump(rec, f, indent=1)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--seeds', action='store_true')
    ap.add_argument('--bound', action='store_true')
    ap.add_argument('--out', default=None, help='timing mode: write the record to this JSON file')
    args = ap.parse_args(argv)
    if args.seeds:
        find_seeds()
    if args.bound:
        bound()
    if not (args.seeds or args.bound):
        measure(args.out)


if __name__ == '__main__':
    main()
