"""TEST INFRASTRUCTURE ONLY: the torch-CPU stand-in of ops.input_augment (asr_input_augment) and its counters, layered over
_cpu_ops.install so that the host logic of the input augmentation (the ModelBase hooks, the recipes) runs in the
`-m "not gpu"` suite.  The values are the numpy statement (tests/_input_aug_oracle.py); the argument checks are those of
the entry point."""
import math

import numpy as np
import torch

import _cpu_ops
import _input_aug_oracle as iao

CALLS = dict(calls=0, elements=0, vec_calls=0)   # stand-in calls since the last reset
LOG = []                                         # the keyword dict of every call since the last reset


def _input_augment(x, seq_len, n_ch, noise_std=0.0, freq_masks=(0, 0), time_masks=(0, 0, 1.0), mask_value=0.0, seed=0,
                   offset=0, out=None):
    if x.dtype != torch.float32 or x.dim() != 3:
        raise ValueError('input_augment: x must be [B,T,F] fp32')
    B, T, F = x.shape
    nf, fw = (int(v) for v in freq_masks)
    nt, tw, tr = int(time_masks[0]), int(time_masks[1]), float(time_masks[2])
    sd, mv, n_ch = float(noise_std), float(mask_value), int(n_ch)
    if not (1 <= n_ch <= F and F % n_ch == 0):
        raise ValueError('asr_input_augment: n_ch must be in [1, F] and divide F')
    if not (0 <= nf <= 8 and 0 <= nt <= 8):
        raise ValueError('asr_input_augment: mask counts must be in [0, 8]')
    if fw < 0 or tw < 0:
        raise ValueError('asr_input_augment: mask widths must be >= 0')
    if not 0.0 <= tr <= 1.0:
        raise ValueError('asr_input_augment: tmask_ratio must be in [0, 1]')
    if not (0.0 <= sd < float('inf')):
        raise ValueError('asr_input_augment: noise_std must be finite and >= 0')
    if not math.isfinite(mv):
        raise ValueError('asr_input_augment: mask_value must be finite')
    lens = torch.as_tensor(seq_len).to(torch.int32).cpu().numpy()
    if lens.size != B:
        raise ValueError('input_augment: seq_len has %d entries for a batch of %d' % (lens.size, B))
    CALLS['calls'] += 1
    CALLS['elements'] += x.numel()
    CALLS['vec_calls'] += 1
    LOG.append(dict(shape=(B, T, F), seq_len=lens.copy(), n_ch=n_ch, noise_std=sd, freq_masks=(nf, fw),
                    time_masks=(nt, tw, tr), mask_value=mv, seed=int(seed), offset=int(offset)))
    y = iao.augment(x.detach().cpu().numpy(), lens, n_ch, sd, (nf, fw), (nt, tw, tr), mv, seed, offset)
    y = torch.from_numpy(np.ascontiguousarray(y)).to(x.device)
    if out is not None:
        if out.data_ptr() == x.data_ptr():
            raise ValueError('asr_input_augment: y overlaps x')
        out.copy_(y)
        return out
    return y


def _input_augment_counts(device=0):
    return dict(CALLS)


def _reset_input_augment_counts(device=0):
    for k in CALLS:
        CALLS[k] = 0
    del LOG[:]


STAND_INS = dict(input_augment=_input_augment, input_augment_counts=_input_augment_counts,
                 reset_input_augment_counts=_reset_input_augment_counts)


def install(monkeypatch, base=None):
    """`base`: the stand-in module to layer over (its install(monkeypatch) returns ops); default _cpu_ops."""
    ops = (base or _cpu_ops).install(monkeypatch)
    for name, fn in STAND_INS.items():
        assert hasattr(ops, name), name
        if monkeypatch is not None:
            monkeypatch.setattr(ops, name, fn)
        else:
            setattr(ops, name, fn)
    _reset_input_augment_counts()
    return ops
