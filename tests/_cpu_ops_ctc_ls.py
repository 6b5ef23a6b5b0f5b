"""TEST INFRASTRUCTURE ONLY: the torch-CPU stand-in of ops.ctc_loss_ls (asr_ctc_loss_ls) and its counters, layered over
_cpu_ops.install so that the host logic of CTC / MultitaskCTC / JointCTCAttention with label smoothing runs in the
`-m "not gpu"` suite.  It computes in float64 what the kernels compute (oracle.ctc per utterance, the KL row terms from
log_softmax) and follows _cpu_ops._ctc_loss in what it counts as infeasible."""
import numpy as np
import torch

import _cpu_ops
from oracle import ctc as octc

CALLS = dict(calls=0, lse_done=0, no_grad=0)     # stand-in calls since the last reset (a test that must see none reads it)


def _ctc_loss_ls(logits, labels_flat, label_offsets, seq_len, max_label_len, smoothing, grad_scale=1.0, ws=None, ninf=None,
                 lse_done=False, want_grad=True, want_image=False):
    eps = float(smoothing)
    if not 0.0 < eps < 1.0:
        raise ValueError('ctc_loss_ls: smoothing must be in (0, 1), got %r' % (smoothing,))
    if lse_done and ws is None:
        raise ValueError('ctc_loss_ls: lse_done needs the workspace of ctc_head_fwd (ctc_ls_workspace)')
    if want_image and not want_grad:
        raise ValueError('ctc_loss_ls: the image is the image of the gradient (want_grad)')
    CALLS['calls'] += 1
    CALLS['lse_done'] += bool(lse_done)
    CALLS['no_grad'] += not want_grad
    T, B, Cc = logits.shape
    labs = _cpu_ops._labels_list(labels_flat, label_offsets, B)
    sl = seq_len.cpu().numpy()
    loss, kl = np.zeros(B), np.zeros(B)
    grad = np.zeros((T, B, Cc))
    n_inf = 0
    x = logits.double().numpy()
    for b in range(B):
        n = min(int(sl[b]), T)
        if n == 0 and len(labs[b]) == 0:
            continue                                  # batch-padding row
        l, g, ok = octc.ctc_loss_single(x[:n, b], labs[b])
        if not ok:
            n_inf += 1
            continue                                  # loss 0, kl 0, grad 0
        logp = octc.log_softmax(x[:n, b])
        loss[b] = l
        kl[b] = -(logp.mean(axis=1) + np.log(Cc)).sum()
        grad[:n, b] = (1.0 - eps) * g + eps * (np.exp(logp) - 1.0 / Cc)
    g = torch.from_numpy(grad * grad_scale).float() if want_grad else None
    img = None
    if want_image:
        Kp = (Cc + 63) // 64 * 64
        img = torch.zeros((T * B, Kp), dtype=torch.bfloat16)
        img[:, :Cc] = g.view(T * B, Cc).to(torch.bfloat16)
    return (torch.from_numpy(loss).float(), torch.from_numpy(kl).float(), g, img,
            torch.tensor([n_inf], dtype=torch.int32))


def _ctc_ls_counts(device=0):
    return dict(CALLS)


def _reset_ctc_ls_counts(device=0):
    for k in CALLS:
        CALLS[k] = 0


def _ctc_ls_workspace(T, B, max_label_len, device):
    return torch.empty((0,), dtype=torch.uint8)


STAND_INS = dict(ctc_loss_ls=_ctc_loss_ls, ctc_ls_counts=_ctc_ls_counts, reset_ctc_ls_counts=_reset_ctc_ls_counts,
                 ctc_ls_workspace=_ctc_ls_workspace)


def install(monkeypatch, base=None):
    """`base`: the stand-in module to layer over (its install(monkeypatch) returns ops); default _cpu_ops."""
    ops = (base or _cpu_ops).install(monkeypatch)
    for name, fn in STAND_INS.items():
        assert hasattr(ops, name), name
        monkeypatch.setattr(ops, name, fn)
    _reset_ctc_ls_counts()
    return ops
