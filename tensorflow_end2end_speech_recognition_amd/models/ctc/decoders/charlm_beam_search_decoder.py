"""CTC prefix beam search with a character / phone language model and an insertion bonus -- the reference's EMPTY
models/ctc/decoders/charlm_beam_search_decoder.py, filled.  EXTENSION: the reference's BeamSearchDecoder.__call__ takes
alpha ("language model weight") and beta ("insertion bonus") and carries `# TODO: add LM score here`
(models/ctc/decoders/beam_search_decoder.py:53,61-62,132); it never used them.

The float64 statement (what asr_ctc_beam_decode_lm is tested against) is charlm_prefix_search: a plain restatement of that
decoder's loop (:53-152 -- the same dict, the same vocab-major insertion order, the same stable sort) with ONE change at
the TODO line.  Every EXTENSION of `prefix` by a class c != blank uses

    p_t + alpha * log p_lm(c | <SOS>, prefix) + beta

in place of p_t: in the c != prefix_end branch and in the c == prefix_end branch (p_b only).  The blank update and the
merging case (the unchanged prefix collecting p_nb + p_t) get no LM term and no bonus.  The LM factor depends on the
resulting prefix alone, so dict merging stays consistent, and the quantity searched is exactly
p_ctc(l | x) * prod_k p_lm(l_k | l_<k)^alpha * e^(beta |l|).  Ranking key, trimming and the returned score
(-logsumexp(p_b, p_nb) of the best entry, LM and bonus terms included) are the reference's.

Classes: the CTC model has C classes (blank = C - 1 in this package's models, labels 0 .. C-2); the LM has V >= C + 1
classes, CTC label c is LM class c, and its <SOS> / <EOS> indices are >= C - 1 (the attention convention: a phone61 LM
of train_lm.py, V = 63, serves the 62-class CTC model as it is).  log p_lm is the log-softmax over all V classes.
Limits: no <EOS> term at the end of the utterance; no word-level LM for character models; no n-best output.

The LM is a callable (state, word) -> (logits [V], state).  rnnlm_callable gives the float64 restatement of RNNLM."""
import math

import numpy as np
import torch

from .... import ops
from ...attention.decoders.beam_search import lm_fusion as LF
from .greedy_decoder import _to_logits_tbc

NEG_INF = -float('inf')


def _lse(*args):
    """beam_search_decoder.py:23-32."""
    if all(a == NEG_INF for a in args):
        return NEG_INF
    m = max(args)
    return m + math.log(sum(math.exp(a - m) for a in args))


def log_softmax64(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max()
    return x - (m + math.log(np.exp(x - m).sum()))


def _gap(a, b):
    """a - b for totals a >= b that may be -inf."""
    if b == NEG_INF:
        return 0.0 if a == NEG_INF else float('inf')
    return a - b


def rnnlm_callable(params):
    """(lm, state0) for charlm_prefix_search from lm_fusion.lm_step's parameter dict: one history per call, float64."""
    def lm(state, word):
        logits, new = LF.lm_step(params, np.array([int(word)], dtype=np.int64), state)
        return logits[0], new
    return lm, LF.lm_initial_state(params, 1)


def charlm_prefix_search(log_probs, blank, beam_width=1, alpha=0., beta=0., lm=None, lm_state=None, sos=None, trace=None):
    """One utterance.  log_probs [T, C] (its own frames only); lm: None (alpha must be 0) or the callable above, started with
    lm(lm_state, sos).  Returns dict(labels, score, lm_score, min_margin): score = -logsumexp(p_b, p_nb) of the best entry,
    lm_score = its alpha-unweighted sum of log p_lm, min_margin = the smallest gap, over the frames, between the last kept
    and the first dropped total and (T >= 1) between the best and second-best final totals.  trace: a list that receives per
    frame dict(beam=[(prefix, p_b, p_nb, lm_total)], order_gap = the smallest non-zero gap between neighbours among the
    kept totals and the first dropped one)."""
    log_probs = np.asarray(log_probs, dtype=np.float64)
    T, C = log_probs.shape
    alpha, beta, W = float(alpha), float(beta), int(beam_width)
    if lm is None and alpha != 0.0:
        raise ValueError('alpha = %r needs a language model' % (alpha,))
    # per prefix: (LM state after it, log p_lm(. | <SOS>, prefix) [V], sum of log p_lm over its labels)
    if lm is not None:
        logits, st = lm(lm_state, sos)
        info = {(): (st, log_softmax64(logits), 0.0)}
    else:
        info = {(): (None, None, 0.0)}
    beam = [(tuple(), (0.0, NEG_INF))]
    min_margin = float('inf')
    for t in range(T):
        nxt = {}
        for c in range(C):
            p_t = float(log_probs[t, c])
            for prefix, (p_b, p_nb) in beam:
                if c == blank:
                    nb, nnb = nxt.get(prefix, (NEG_INF, NEG_INF))
                    nxt[prefix] = (_lse(nb, p_b + p_t, p_nb + p_t), nnb)
                    continue
                end = prefix[-1] if prefix else None
                new_prefix = prefix + (c,)
                lm_lp = info[prefix][1]
                # the reference's TODO (:132): the LM score and the insertion bonus of the extension
                p_e = p_t + alpha * (float(lm_lp[c]) if lm_lp is not None else 0.0) + beta
                nb, nnb = nxt.get(new_prefix, (NEG_INF, NEG_INF))
                if c != end:
                    nnb = _lse(nnb, p_b + p_e, p_nb + p_e)
                else:
                    nnb = _lse(nnb, p_b + p_e)
                nxt[new_prefix] = (nb, nnb)
                if c == end:
                    nb, nnb = nxt.get(prefix, (NEG_INF, NEG_INF))
                    nxt[prefix] = (nb, _lse(nnb, p_nb + p_t))
        ranked = sorted(((kv[0], kv[1], _lse(*kv[1])) for kv in nxt.items()), key=lambda e: e[2], reverse=True)
        if len(ranked) > W:
            min_margin = min(min_margin, _gap(ranked[W - 1][2], ranked[W][2]))
        if t == T - 1 and len(ranked) > 1:
            min_margin = min(min_margin, _gap(ranked[0][2], ranked[1][2]))
        beam = [(e[0], e[1]) for e in ranked[:W]]
        for prefix, _ in beam:
            if prefix not in info:
                st, lp, tot = info[prefix[:-1]]
                if lm is None:
                    info[prefix] = (None, None, 0.0)
                else:
                    logits, st2 = lm(st, prefix[-1])
                    info[prefix] = (st2, log_softmax64(logits), tot + float(lp[prefix[-1]]))
        if trace is not None:
            gaps = [_gap(ranked[i][2], ranked[i + 1][2]) for i in range(min(W, len(ranked) - 1))]
            trace.append(dict(beam=[(p, v[0], v[1], info[p][2]) for p, v in beam],
                              order_gap=min([g for g in gaps if g > 0.0] or [float('inf')])))
    best = beam[0]
    return dict(labels=list(best[0]), score=-_lse(*best[1]), lm_score=info[best[0]][2], min_margin=min_margin)


def charlm_beam_search_decode(log_probs_btc, seq_len, blank, beam_width=1, alpha=0., beta=0., lm=None, lm_state=None, sos=None):
    """The batch form, in oracle.decoders.beam_search_decode's conventions: log_probs [B, T, C].  Returns (list of best
    prefixes, np.array of scores, np.array of LM totals, min_margin over the batch)."""
    results, scores, lms, margin = [], [], [], float('inf')
    for b in range(len(seq_len)):
        o = charlm_prefix_search(np.asarray(log_probs_btc)[b, :int(seq_len[b])], blank, beam_width, alpha, beta, lm, lm_state, sos)
        results.append(o['labels'])
        scores.append(o['score'])
        lms.append(o['lm_score'])
        margin = min(margin, o['min_margin'])
    return results, np.array(scores), np.array(lms), margin


class CharLMBeamSearchDecoder(object):
    """BeamSearchDecoder's signature with the LM: CharLMBeamSearchDecoder(space_index, blank_index, lm) where lm is an RNNLM
    (models/lm), its decode_weights() dict (with 'sos', and 'eos' when known) or None; __call__(probs [B,T,C], seq_len,
    beam_width=1, alpha=0., beta=0.) -> (results, scores), executed by asr_ctc_beam_decode_lm on the GPU."""

    def __init__(self, space_index, blank_index, lm=None, device='cuda:0'):
        self._space = space_index
        self._blank = blank_index
        self._lm = lm
        self.device = torch.device(device)

    def __call__(self, probs, seq_len, beam_width=1, alpha=0., beta=0.):
        logits = _to_logits_tbc(probs, self.device)
        sl = torch.as_tensor(np.asarray(seq_len), dtype=torch.int32, device=self.device)
        lab, n, score, _ = ops.ctc_beam_decode_lm(logits, sl, int(beam_width), lm=lm_weights_of(self._lm), lm_weight=alpha,
                                                  insertion_bonus=beta, blank=self._blank)
        lab, n = lab.cpu().numpy(), n.cpu().numpy()
        return [lab[b, :n[b]].tolist() for b in range(lab.shape[0])], score.cpu().numpy()


def lm_weights_of(lm):
    """None, a decode_weights() dict as it is, or an RNNLM's decode_weights() with its <EOS> index."""
    if lm is None or isinstance(lm, dict):
        return lm
    return dict(lm.decode_weights(), eos=lm.eos_index)
