"""Batches beyond the chip: the headline model (5 x 256 bf16, D = 120, 62 classes, seq_len ~ U{100..778}) and the cfg C
recurrent stack (3 x 512 bf16) at per-GPU batches on both sides of the point where a bidirectional layer needs more
clusters than the chip has CUs for in any form (on 256 CUs: B = 512 at H = 256, B = 256 at H = 512).  Below it the recurrences are one cluster launch;
above it they run in tile groups -- before that change on the single-CU kernels.  Prints ms per training step and the
recurrence path counters (LSTM and GRU); run it on two checkouts to compare them (a checkout without the counters prints
none).  Every figure is the median of REPEATS timed windows of STEPS steps, with the fastest and slowest window beside it.
    python scripts/probe_tile_groups.py [tag]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from tensorflow_end2end_speech_recognition_amd import ops  # noqa: E402
from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC  # noqa: E402

tag = sys.argv[1] if len(sys.argv) > 1 else 'this'
dev = torch.device('cuda:0')
WARMUP, STEPS, REPEATS = 2, 5, 3


def make_batch(seed, B, D, C, tmin, tmax):
    """the headline's batch: seq_len ~ U{tmin..tmax}, labels of len // 8 clipped to [5, 75], zeros past each length"""
    rng = np.random.RandomState(seed)
    sl = rng.randint(tmin, tmax + 1, size=B).astype(np.int32)
    x = rng.randn(B, int(sl.max()), D).astype(np.float32)
    labels = []
    for b in range(B):
        x[b, sl[b]:] = 0
        labels.append(rng.randint(0, C - 1, size=int(np.clip(sl[b] // 8, 5, 75))))
    dense = np.full((B, max(len(v) for v in labels)), -1, dtype=np.int64)
    for b, v in enumerate(labels):
        dense[b, :len(v)] = v
    return x, sl, dense


for H, L, batches in ((256, 5, (128, 256, 272, 384, 512, 528, 768)), (512, 3, (128, 144, 256, 272, 384, 512))):
    base = None
    for B in batches:
        x, sl, dense = make_batch(1, B, 120, 62, 100, 778)
        xd, sd = torch.tensor(x, device=dev), torch.tensor(sl, device=dev)
        m = CTC('blstm', 120, H, L, 61, parameter_init=0.1, clip_grad_norm=5.0, clip_activation=50.0, seed=0, dtype='bf16',
                device=str(dev))
        for _ in range(WARMUP):
            l_, _ = m.compute_loss(xd, dense, sd, keep_prob=0.8)
            m.train(l_, 'rmsprop', 1e-3)
        torch.cuda.synchronize()
        if hasattr(ops, 'reset_recurrence_path_counts'):
            ops.reset_recurrence_path_counts(0)
        win = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            for _ in range(STEPS):
                l_, _ = m.compute_loss(xd, dense, sd, keep_prob=0.8)
                m.train(l_, 'rmsprop', 1e-3)
            torch.cuda.synchronize()
            win.append((time.perf_counter() - t0) / STEPS * 1e3)
        ms = sorted(win)[REPEATS // 2]
        ops.check_async_errors(0)
        c = ops.recurrence_path_counts(0) if hasattr(ops, 'recurrence_path_counts') else {}
        base = base or (ms, B)
        print('%s  %dx%d bf16  B=%3d  T=%d  %9.2f ms/step (%.2f .. %.2f)  %8.0f frames/s  x%.2f of B=%d  loss %.4f  per step: %s'
              % (tag, L, H, B, x.shape[1], ms, min(win), max(win), float(sl.sum()) / ms * 1e3, ms / base[0], base[1],
                 float(l_.item()), ' '.join('%s=%g' % (k, v / (STEPS * REPEATS)) for k, v in c.items() if v) or '-'), flush=True)
        del m, xd
        torch.cuda.empty_cache()
