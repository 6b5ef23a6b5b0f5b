"""TEST INFRASTRUCTURE ONLY: the float64 statement of label smoothing for the CTC heads (an EXTENSION of this project:
the reference's blstm_ctc_ls.yml sets label_smoothing_prob and none of its code reads it), built on
oracle.ctc.ctc_loss_batch and oracle.ctc.log_softmax.

For utterance b with len_b = min(seq_len[b], T) frames, p = softmax(x) over all C classes (blank included), 0 < eps < 1:
  kl[b]    = sum_{t < len_b} KL(uniform || p[t,b,:]) = sum_t (lse(x[t,b,:]) - mean_k x[t,b,k] - ln C)
  total[b] = (1 - eps) ctc[b] + eps kl[b]
  d total[b] / d x[t,b,k] = p[t,b,k] - (1 - eps) occ[t,b,k] - eps / C     (t < len_b)
An infeasible utterance (no alignment: fewer frames than labels plus adjacent repeats, or no frame) keeps ctc 0, kl 0 and
gradient 0.  `patched` composes the statement with the model statements of oracle.model / oracle.attention."""
import contextlib

import numpy as np
import torch

from oracle import attention as oatt
from oracle import ctc as octc
from oracle import model as omodel


def feasible(labels, n):
    """Whether n frames of finite logits admit an alignment of `labels`: one frame per label and one blank between equal
    neighbours."""
    lab = list(labels)
    return n > 0 and n >= len(lab) + sum(1 for i in range(1, len(lab)) if lab[i] == lab[i - 1])


def kl_uniform(logits_tbc, labels_list, seq_len):
    """kl [B] and its gradient [T,B,C] (p - 1/C on the frames of a feasible utterance, 0 elsewhere)."""
    x = np.asarray(logits_tbc, dtype=np.float64)
    T, B, C = x.shape
    kl = np.zeros(B)
    grad = np.zeros((T, B, C))
    for b in range(B):
        n = min(int(seq_len[b]), T)
        if not feasible(labels_list[b], n):
            continue
        logp = octc.log_softmax(x[:n, b])                  # -KL row = mean_k logp + ln C
        kl[b] = -(logp.mean(axis=1) + np.log(C)).sum()
        grad[:n, b] = np.exp(logp) - 1.0 / C
    return kl, grad


def ctc_ls_batch(logits_tbc, labels_list, seq_len, eps):
    """Returns dict(ctc [B], kl [B], total [B], grad [T,B,C] = d total[b] / d logits)."""
    x = np.asarray(logits_tbc, dtype=np.float64)
    ctc, g_ctc = octc.ctc_loss_batch(x, labels_list, np.asarray(seq_len))
    kl, g_kl = kl_uniform(x, labels_list, seq_len)
    return dict(ctc=ctc, kl=kl, total=(1.0 - eps) * ctc + eps * kl, grad=(1.0 - eps) * g_ctc + eps * g_kl)


class _LsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels_list, seq_len, eps):
        r = ctc_ls_batch(logits.detach().cpu().numpy().astype(np.float64), labels_list, seq_len, eps)
        ctx.save_for_backward(torch.from_numpy(r['grad']).to(logits.dtype))
        return torch.from_numpy(r['total']).to(logits.dtype)

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g.view(1, -1, 1), None, None, None


def ctc_ls_loss(logits_tbc, labels_list, seq_len, eps):
    """total [B] as a differentiable torch value (the twin of oracle.model.ctc_loss)."""
    return _LsFn.apply(logits_tbc, labels_list, np.asarray(seq_len), float(eps))


@contextlib.contextmanager
def patched(eps):
    """Within the block the model statements (oracle.model.*_model_forward, oracle.attention.attention_model_forward and
    the statements of the tests that call these) take the smoothed per-utterance loss where they take the CTC loss: the
    composition of this statement with theirs.  Their 'ctc_losses' entries are then the smoothed totals."""
    fn = lambda logits, labels_list, seq_len: ctc_ls_loss(logits, labels_list, seq_len, eps)
    old = omodel.ctc_loss, oatt._ctc_loss
    omodel.ctc_loss, oatt._ctc_loss = fn, fn
    try:
        yield
    finally:
        omodel.ctc_loss, oatt._ctc_loss = old
