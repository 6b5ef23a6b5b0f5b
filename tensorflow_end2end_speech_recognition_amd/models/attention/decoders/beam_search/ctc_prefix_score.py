"""One-pass joint CTC / attention beam search, host statement in float64 (Watanabe et al. 2017, Hori et al. 2017).

EXTENSION: the reference has no such decoder (its attention beam search is dead wiring); like prev_alpha='carry' and
beam_width= this is an addition, switched on by JointCTCAttention.infer(ctc_weight > 0).  The reference-pinned files next to
this one (beam_search_decoder.py, util.py) are not touched.

Vocabularies: the attention classes are C2 = N + 2 (labels 0 .. N-1, <SOS> = N, <EOS> = N + 1), the CTC classes Cc = N + 1
(blank = N).  y [T_b, Cc] is the log-softmax of the CTC head's logits of one utterance over its T_b valid frames.

A hypothesis g (its labels without <SOS>) carries r_n[t] / r_b[t] -- the log-probability of all frame paths over frames
0 .. t that collapse to exactly g and end in a non-blank / a blank --, `last` (its last label, -1 when g is empty) and
ctc_score.  psi(g.c) is the log-probability that the utterance's collapsed CTC output STARTS WITH g.c;
psi(g.<EOS>) = log p_ctc(g); psi of <SOS> is -inf.  logaddexp(-inf, -inf) = -inf, never NaN.

Candidates of a selection step: per unfinished slot the W classes other than <EOS> with the largest attention logits (ties
by lower index) plus <EOS> -- the set att_beam_select_kernel extracts.  With attention-only scores that pruning loses
nothing; with fused scores it IS the preselection (the literature's "CTC pre-beam"), fixed here at W.

This is what csrc/ctc_prefix.hip (the prefix scorer: ops.ctc_prefix_score / ctc_prefix_advance) and csrc/att_beam.hip (the
selection: ops.att_beam_select_joint; the loop ops.att_decoder_beam_joint issues both) compute in fp32, and the oracle of
their tests."""
import collections

import numpy as np
import torch

from .util import check_beam_width, gather_tree_py, normalize_score

NEG_INF = float('-inf')

PrefixState = collections.namedtuple('PrefixState', ['r_n', 'r_b', 'last', 'ctc_score'])
JointBeamState = collections.namedtuple('JointBeamState', ['log_probs', 'finished', 'lengths', 'ctc'])
JointStepOutput = collections.namedtuple('JointStepOutput', ['scores', 'predicted_ids', 'beam_parent_ids'])


def check_ctc_weight(ctc_weight):
    lam = float(ctc_weight)
    if not 0.0 <= lam <= 1.0:
        raise ValueError('ctc_weight must be in [0, 1], got %r' % (ctc_weight,))
    return lam


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))


def prefix_init(y, blank):
    """The empty hypothesis: r_n = -inf, r_b[t] = sum of y[tau, blank] over tau <= t in ascending tau; psi = 0."""
    y = np.asarray(y, dtype=np.float64)
    r_b = np.empty(y.shape[0])
    acc = 0.0
    for t in range(y.shape[0]):
        acc = acc + y[t, blank]
        r_b[t] = acc
    return PrefixState(r_n=np.full(y.shape[0], NEG_INF), r_b=r_b, last=-1, ctc_score=0.0)


def prefix_extend(y, blank, state, labels):
    """Extension of one hypothesis by each of `labels` (CTC labels < blank).  Returns (r_n' [K, T], r_b' [K, T], psi [K])."""
    y = np.asarray(y, dtype=np.float64)
    c = np.asarray(labels, dtype=np.int64).reshape(-1)
    T, K = y.shape[0], len(c)
    r_n, r_b = np.full((K, T), NEG_INF), np.full((K, T), NEG_INF)
    r_n[:, 0] = y[0, c] if state.last < 0 else NEG_INF
    psi = r_n[:, 0].copy()
    same = c == state.last
    for t in range(1, T):
        phi = np.where(same, state.r_b[t - 1], np.logaddexp(state.r_n[t - 1], state.r_b[t - 1]))
        r_n[:, t] = np.logaddexp(r_n[:, t - 1], phi) + y[t, c]
        r_b[:, t] = np.logaddexp(r_n[:, t - 1], r_b[:, t - 1]) + y[t, blank]
        psi = np.logaddexp(psi, phi + y[t, c])
    return r_n, r_b, psi


def prefix_eos(state):
    """psi(g.<EOS>) = log p_ctc(g)."""
    return float(np.logaddexp(state.r_n[-1], state.r_b[-1]))


def prefix_scores(y, blank, state, candidates, n_labels):
    """psi of g.c for attention classes `candidates` (labels, <SOS> = n_labels, <EOS> = n_labels + 1)."""
    cand = np.asarray(candidates, dtype=np.int64).reshape(-1)
    psi = np.full(len(cand), NEG_INF)
    lab = np.flatnonzero((cand >= 0) & (cand < n_labels))
    if len(lab):
        psi[lab] = prefix_extend(y, blank, state, cand[lab])[2]
    psi[cand == n_labels + 1] = prefix_eos(state)
    return psi


def prefix_advance(y, blank, state, word, n_labels, ctc_score=None):
    """The state of g.word: the extension for a label, the parent's own arrays for <EOS> (or a finished parent, whose
    word is <EOS>)."""
    score = state.ctc_score if ctc_score is None else float(ctc_score)
    if not 0 <= int(word) < n_labels:
        return PrefixState(state.r_n, state.r_b, state.last, score)
    r_n, r_b, _ = prefix_extend(y, blank, state, [int(word)])
    return PrefixState(r_n[0], r_b[0], int(word), score)


def preselect(logits_row, beam_width, eos):
    """The W classes other than <EOS> with the largest logits, ties by lower index (fewer when there are fewer)."""
    x = np.asarray(logits_row, dtype=np.float64)
    others = np.array([c for c in range(len(x)) if c != eos], dtype=np.int64)
    order = others[np.argsort(-x[others], kind='stable')]
    return order[:beam_width]


def initial_joint_state(y, blank, beam_width):
    first = prefix_init(y, blank)
    return JointBeamState(log_probs=np.zeros(beam_width), finished=np.zeros(beam_width, dtype=bool),
                          lengths=np.zeros(beam_width, dtype=np.int64), ctc=[first] * beam_width)


def joint_beam_search_step(time, logits, state, y, n_labels, beam_width, ctc_weight, length_penalty_weight,
                           want_margin=False):
    """One joint selection for ONE utterance.  logits [W, C2] (float64), state a JointBeamState, y [T_b, n_labels + 1].
    It follows beam_search_step with three differences: the candidates are the preselected W + 1 classes per slot, the
    score is ((1 - lambda) * total_att + lambda * ctc) / penalty (a candidate whose ctc is -inf is dropped), and the next
    state keeps total_att as log_probs (so that lambda weights totals, not increments) beside ctc_score, last and the
    prefix arrays.  Returns (JointStepOutput, JointBeamState[, margin]): margin = the smallest gap among the top W + 1
    scores."""
    W, N = int(beam_width), int(n_labels)
    lam = check_ctc_weight(ctc_weight)
    C2, eos, blank = N + 2, N + 1, N
    logits = np.asarray(logits, dtype=np.float64)
    assert logits.shape == (W, C2), (logits.shape, W, C2)
    cands = []                                               # (flat, total_att, ctc, length)
    for w in range(W if int(time) > 0 else 1):
        hyp = state.ctc[w]
        if state.finished[w]:                                # all its mass on <EOS>: p = 0, its carried CTC score
            cands.append((w * C2 + eos, state.log_probs[w] + 0.0, hyp.ctc_score, int(state.lengths[w])))
            continue
        logp = log_softmax(logits[w])
        classes = list(preselect(logits[w], W, eos)) + [eos]
        psi = prefix_scores(y, blank, hyp, classes, N)
        for c, p in zip(classes, psi):
            cands.append((w * C2 + int(c), state.log_probs[w] + logp[c], float(p), int(state.lengths[w]) + (c != eos)))
    cands = [c for c in cands if c[2] != NEG_INF]
    if len(cands) < W:
        raise ValueError('joint beam search: %d candidates with a finite CTC prefix score, beam width %d' % (len(cands), W))
    flat = np.array([c[0] for c in cands], dtype=np.int64)
    total = np.array([c[1] for c in cands])
    ctc = np.array([c[2] for c in cands])
    lens = np.array([c[3] for c in cands], dtype=np.int64)
    joint = (1.0 - lam) * total + lam * ctc
    score = normalize_score(torch.as_tensor(joint), torch.as_tensor(lens), length_penalty_weight).numpy()
    order = np.lexsort((flat, -score))                       # score descending, flat index ascending
    top = score[order[:W + 1]]
    margin = float((top[:-1] - top[1:]).min()) if len(top) > 1 else float('inf')
    sel = order[:W]
    word, parent = flat[sel] % C2, flat[sel] // C2
    finished = state.finished[parent] | (word == eos)
    lengths = state.lengths[parent] + ((word != eos) & ~finished)
    nxt = [prefix_advance(y, blank, state.ctc[p], wd, N, ctc_score=s) for p, wd, s in zip(parent, word, ctc[sel])]
    out = JointStepOutput(scores=score[sel], predicted_ids=word, beam_parent_ids=parent)
    new = JointBeamState(log_probs=total[sel], finished=finished, lengths=lengths, ctc=nxt)
    return (out, new, margin) if want_margin else (out, new)


class JointBeamSearchDecoder(object):
    """BeamSearchDecoder's driver over the joint step: step_fn(time, predicted_ids, beam_parent_ids, decoder_state) ->
    (logits [W, C2], decoder_state) as there (ids are torch tensors, None at time 0); y [T_b, n_labels + 1] are the
    utterance's CTC log-posteriors.  min_margin: the smallest gap among the top W + 1 scores over the steps."""

    def __init__(self, step_fn, beam_width, n_labels, ctc_weight, length_penalty_weight, max_decode_length):
        self.step_fn = step_fn
        self.n_labels = int(n_labels)
        self.beam_width = check_beam_width(beam_width, self.n_labels + 1)
        self.eos_index = self.n_labels + 1
        self.ctc_weight = check_ctc_weight(ctc_weight)
        self.length_penalty_weight = length_penalty_weight
        self.max_decode_length = int(max_decode_length)

    def __call__(self, decoder_state, y):
        y = np.asarray(y, dtype=np.float64)
        state = initial_joint_state(y, self.n_labels, self.beam_width)
        words, parents, scores = [], [], []
        word = parent = None
        self.min_margin = float('inf')
        for k in range(self.max_decode_length):
            logits, decoder_state = self.step_fn(k, word, parent, decoder_state)
            out, state, margin = joint_beam_search_step(k, logits.detach().double().cpu().numpy(), state, y, self.n_labels,
                                                        self.beam_width, self.ctc_weight, self.length_penalty_weight,
                                                        want_margin=True)
            self.min_margin = min(self.min_margin, margin)
            word, parent = torch.as_tensor(out.predicted_ids), torch.as_tensor(out.beam_parent_ids)
            words.append(out.predicted_ids)
            parents.append(out.beam_parent_ids)
            scores.append(out.scores)
            if bool(state.finished.all()):
                break
        w, p = np.stack(words), np.stack(parents)
        return dict(predicted_ids=gather_tree_py(w, p), word=w, parent=p, scores=np.stack(scores), state=state), decoder_state
