"""TEST INFRASTRUCTURE ONLY: the torch-CPU stand-in of ops.weight_noise_perturb (asr_weight_noise_perturb) and its
counters, layered over _cpu_ops.install so that the host logic of the weight noise (ParamStore.perturb / restore, the
ModelBase hooks, the recipes) runs in the `-m "not gpu"` suite.  The noise is the float64 statement
(tests/_weight_noise_oracle.py) rounded as the kernel rounds: fl32(w + fl32(std * z))."""
import numpy as np
import torch

import _cpu_ops
import _weight_noise_oracle as own

CALLS = dict(calls=0, elements=0, vec_calls=0)   # stand-in calls since the last reset
LOG = []                                         # (std, seed, offset, n) of every call since the last reset


def _weight_noise_perturb(flat, backup, std, seed, offset):
    sd = float(std)
    if not (0.0 <= sd < float('inf')):
        raise ValueError('weight_noise_perturb: std must be finite and >= 0, got %r' % (std,))
    if flat.dtype != torch.float32 or backup.dtype != torch.float32:
        raise ValueError('weight_noise_perturb: fp32 buffers')
    if backup.numel() != flat.numel():
        raise ValueError('weight_noise_perturb: backup has %d elements, flat %d' % (backup.numel(), flat.numel()))
    n = flat.numel()
    CALLS['calls'] += 1
    CALLS['elements'] += n
    CALLS['vec_calls'] += 1
    LOG.append((sd, int(seed), int(offset), n))
    backup.copy_(flat)
    if sd > 0.0:
        noise = (np.float32(sd) * own.z(n, seed, offset).astype(np.float32)).astype(np.float32)
        flat.add_(torch.from_numpy(noise).view(flat.shape))
    return flat


def _weight_noise_counts(device=0):
    return dict(CALLS)


def _reset_weight_noise_counts(device=0):
    for k in CALLS:
        CALLS[k] = 0
    del LOG[:]


STAND_INS = dict(weight_noise_perturb=_weight_noise_perturb, weight_noise_counts=_weight_noise_counts,
                 reset_weight_noise_counts=_reset_weight_noise_counts)


def install(monkeypatch, base=None):
    """`base`: the stand-in module to layer over (its install(monkeypatch) returns ops); default _cpu_ops."""
    ops = (base or _cpu_ops).install(monkeypatch)
    for name, fn in STAND_INS.items():
        assert hasattr(ops, name), name
        if monkeypatch is not None:
            monkeypatch.setattr(ops, name, fn)
        else:
            setattr(ops, name, fn)
    _reset_weight_noise_counts()
    return ops
