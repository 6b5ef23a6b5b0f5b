"""Shallow fusion of an RNN language model into the attention beam search, host statement in float64 (Hori et al. 2017).

EXTENSION: the reference intended a language model and never finished one -- models/lm/{base,char_rnnlm,word_rnnlm}.py
raise NotImplementedError, models/ctc/decoders/charlm_beam_search_decoder.py is empty, and its CTC BeamSearchDecoder takes
`alpha` ("language model weight") and carries `# TODO: add LM score here` (models/ctc/decoders/beam_search_decoder.py:53,
61, 132).  The definition below is this project's; it is switched on by AttentionSeq2Seq.infer(lm=, lm_weight > 0) and
combines with JointCTCAttention's ctc_weight.  The reference-pinned files next to this one are not touched.  numpy only:
no torch, no device.

State.  Beside log_probs / finished / lengths (and, with CTC, the prefix state of ctc_prefix_score.py) every slot carries
lm_score -- the sum of the LM log-probabilities of the words emitted so far -- and the LM's per-layer (c, h).  At step k the
LM reads its own embedding of the slot's last word (<SOS> at step 0) and its state and gives p_lm = log_softmax(lm_logits)
over the same C2 = N + 2 classes (labels, <SOS> = N, <EOS> = N + 1) as the attention decoder.

Candidates.  local[c] = p_att[c] + lm_weight * p_lm[c]; per unfinished slot the W classes other than <EOS> with the largest
local (ties by lower index) and <EOS>.  Without CTC this pruning loses nothing in exact arithmetic: within a slot every
class but <EOS> shares its length and carried totals, so the fused scores are ordered as local is (the argument of
csrc/att_beam.hip's header comment).  With CTC it is the pre-beam, fixed at W.  NOTE: for lm_weight > 0 this deliberately
differs from the joint decoder's attention-only preselection (ctc_prefix_score.preselect) and equals it as lm_weight goes
to 0.  A finished slot offers its <EOS> alone with p_att = p_lm = 0 (lm_score is carried unchanged); at the first step
only slot 0 has candidates.

Score.  total_att = log_probs + p_att[c]; lm_total = lm_score + p_lm[c]; ctc = the prefix score psi, or a finished slot's
ctc_score, exactly as joint_beam_search_step;
    fused = (1 - ctc_weight) * total_att + ctc_weight * ctc + lm_weight * lm_total      (no CTC term at ctc_weight = 0)
    score = fused / penalty(length)       (the length rule and the lpw == 1 quirk of normalize_score)
A candidate with ctc = -inf is dropped; the W best by (score descending, flat index ascending) are selected.  Next state:
log_probs = total_att (attention alone), lm_score = lm_total, ctc_score / finished / lengths / last as the joint step; the
LM state of a selected hypothesis is the LM's NEW state of its parent row (the LM has consumed the parent's last word; the
chosen word is the next step's input).

Out of scope: an insertion bonus (`beta`), a word-level LM for character models, n-best rescoring, and an LM in the CTC
prefix beam search (csrc/beam.hip).

This is what csrc/lm_fusion.hip (the language model: ops.lm_step / lm_beam_reorder) and csrc/att_beam.hip (the selection:
ops.att_beam_select_fused; the loop ops.att_decoder_beam_lm issues both) compute in fp32, and the oracle of their tests."""
import collections
import math

import numpy as np

from . import ctc_prefix_score as S

NEG_INF = float('-inf')

FusedBeamState = collections.namedtuple('FusedBeamState', ['log_probs', 'finished', 'lengths', 'lm_score', 'ctc'])
FusedStepOutput = collections.namedtuple('FusedStepOutput', ['scores', 'predicted_ids', 'beam_parent_ids'])


def check_lm_weight(lm_weight):
    """A finite float >= 0."""
    mu = float(lm_weight)
    if not (mu >= 0.0 and math.isfinite(mu)):
        raise ValueError('lm_weight must be a finite number >= 0, got %r' % (lm_weight,))
    return mu


# ----------------------------------------------------------------------------------------------- the language model step
def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def lm_initial_state(params, rows):
    """(c, h), each [L, rows, H] zeros: the empty history."""
    L, H = len(params['kernels']), np.asarray(params['biases'][0]).shape[0] // 4
    return np.zeros((L, rows, H)), np.zeros((L, rows, H))


def lm_step(params, words, state):
    """One step of the LSTM language model on `rows` histories.  params: emb [C2, Em], kernels = L arrays [Din_l + H, 4H]
    (gate columns i, ci, f, o: LSTMBlockCell), biases = L arrays [4H], W_out [H, C2], b_out [C2], cell_clip (0 / None: off).
    words [rows]: each row's last word; state (c, h) [L, rows, H].  Forget bias 1, no peepholes; the new cell state is
    clipped before the output gate reads it.  Returns (lm_logits [rows, C2] raw, (c', h'))."""
    c, h = (np.asarray(t, dtype=np.float64) for t in state)
    clip = float(params.get('cell_clip') or 0.0)
    x = np.asarray(params['emb'], dtype=np.float64)[np.asarray(words, dtype=np.int64)]
    c2, h2 = np.empty_like(c), np.empty_like(h)
    for l, (kernel, bias) in enumerate(zip(params['kernels'], params['biases'])):
        pre = np.concatenate([x, h[l]], axis=1) @ np.asarray(kernel, dtype=np.float64) + np.asarray(bias, dtype=np.float64)
        i, g, f, o = np.split(pre, 4, axis=1)
        cn = np.tanh(g) * _sigmoid(i) + c[l] * _sigmoid(f + 1.0)
        if clip > 0.0:
            cn = np.clip(cn, -clip, clip)
        hn = np.tanh(cn) * _sigmoid(o)
        c2[l], h2[l] = cn, hn
        x = hn
    logits = x @ np.asarray(params['W_out'], dtype=np.float64) + np.asarray(params['b_out'], dtype=np.float64)
    return logits, (c2, h2)


def lm_step_fn(params, beam_width, sos_index):
    """The LM as a step function of LMFusedBeamSearchDecoder for one utterance tiled to W rows:
    fn(time, predicted_ids, beam_parent_ids, lm_state) -> (lm_logits [W, C2], lm_state); at time 0 both ids are None
    (<SOS>, the empty history; lm_state may be None); later the state is gathered by beam_parent_ids first."""
    W = int(beam_width)

    def fn(time, word, parent, state):
        if word is None:
            state = lm_initial_state(params, W) if state is None else state
            words = np.full(W, int(sos_index), dtype=np.int64)
        else:
            p = np.asarray(parent, dtype=np.int64)
            state = (state[0][:, p], state[1][:, p])
            words = np.asarray(word, dtype=np.int64)
        return lm_step(params, words, state)
    return fn


# ------------------------------------------------------------------------------------------------------ the fused step
def normalize(fused, lengths, length_penalty_weight):
    """normalize_score (util.py) on numpy arrays: fused / ((5 + len)^a / 6^a); a == 1 leaves it as it is (the quirk)."""
    a = 0.0 if length_penalty_weight is None else float(length_penalty_weight)
    if a == 1.0:
        return fused
    return fused / ((5.0 + np.asarray(lengths, dtype=np.float64)) ** a / (6.0 ** a))


def preselect_local(local_row, beam_width, eos):
    """The W classes other than <EOS> with the largest local score, ties by lower index (fewer when there are fewer)."""
    return S.preselect(local_row, beam_width, eos)


def initial_fused_state(beam_width, y=None, blank=None):
    W = int(beam_width)
    ctc = [S.prefix_init(y, blank)] * W if y is not None else None
    return FusedBeamState(log_probs=np.zeros(W), finished=np.zeros(W, dtype=bool), lengths=np.zeros(W, dtype=np.int64),
                          lm_score=np.zeros(W), ctc=ctc)


def fused_beam_search_step(time, logits, lm_logits, state, n_labels, beam_width, lm_weight, length_penalty_weight,
                           ctc_weight=0.0, y=None, want_margin=False, prune=True, log_softmax=S.log_softmax,
                           normalize_fn=None):
    """One fused selection for ONE utterance.  logits / lm_logits [W, C2] (float64, raw), state a FusedBeamState, y
    [T_b, n_labels + 1] CTC log-posteriors (needed iff ctc_weight > 0; state.ctc then holds the PrefixStates).
    prune=False ranks every class of every slot (no preselection): the search the pruning is lossless against.
    log_softmax / normalize_fn(fused, lengths, length_penalty_weight, flat_index): the two primitives, replaceable -- the
    earlier statements differ from each other in the last bit of theirs (beam_search_step uses torch's log_softmax and pow on a
    [W, C2] tensor, joint_beam_search_step ctc_prefix_score.log_softmax and torch's pow on the candidate list), so a
    bit-for-bit comparison with either hands its primitive in; the defaults are numpy's.
    Returns (FusedStepOutput, FusedBeamState[, margin]): margin = the smallest gap among the top W + 1 scores."""
    W, N = int(beam_width), int(n_labels)
    mu, lam = check_lm_weight(lm_weight), S.check_ctc_weight(ctc_weight)
    C2, eos, blank = N + 2, N + 1, N
    logits, lm_logits = np.asarray(logits, dtype=np.float64), np.asarray(lm_logits, dtype=np.float64)
    assert logits.shape == (W, C2) and lm_logits.shape == (W, C2), (logits.shape, lm_logits.shape, W, C2)
    if lam > 0.0 and (y is None or state.ctc is None):
        raise ValueError('ctc_weight > 0 needs the CTC log-posteriors and the prefix state')
    cands = []                                               # (flat, total_att, lm_total, ctc, length)
    for w in range(W if int(time) > 0 else 1):
        hyp = state.ctc[w] if lam > 0.0 else None
        if state.finished[w]:                                # all its mass on <EOS>: p_att = p_lm = 0, carried scores
            cands.append((w * C2 + eos, state.log_probs[w] + 0.0, state.lm_score[w] + 0.0,
                          hyp.ctc_score if hyp is not None else 0.0, int(state.lengths[w])))
            continue
        p_att, p_lm = log_softmax(logits[w]), log_softmax(lm_logits[w])
        local = p_att + mu * p_lm
        classes = (list(preselect_local(local, W, eos)) if prune else [c for c in range(C2) if c != eos]) + [eos]
        psi = S.prefix_scores(y, blank, hyp, classes, N) if hyp is not None else np.zeros(len(classes))
        for c, p in zip(classes, psi):
            cands.append((w * C2 + int(c), state.log_probs[w] + p_att[c], state.lm_score[w] + p_lm[c], float(p),
                          int(state.lengths[w]) + (c != eos)))
    cands = [c for c in cands if c[3] != NEG_INF]
    if len(cands) < W:
        raise ValueError('fused beam search: %d candidates with a finite CTC prefix score, beam width %d' % (len(cands), W))
    flat = np.array([c[0] for c in cands], dtype=np.int64)
    total = np.array([c[1] for c in cands])
    lm_total = np.array([c[2] for c in cands])
    ctc = np.array([c[3] for c in cands])
    lens = np.array([c[4] for c in cands], dtype=np.int64)
    fused = (1.0 - lam) * total
    if lam > 0.0:
        fused = fused + lam * ctc
    fused = fused + mu * lm_total
    score = normalize_fn(fused, lens, length_penalty_weight, flat) if normalize_fn else normalize(fused, lens, length_penalty_weight)
    order = np.lexsort((flat, -score))                       # score descending, flat index ascending
    top = score[order[:W + 1]]
    margin = float((top[:-1] - top[1:]).min()) if len(top) > 1 else float('inf')
    sel = order[:W]
    word, parent = flat[sel] % C2, flat[sel] // C2
    finished = state.finished[parent] | (word == eos)
    lengths = state.lengths[parent] + ((word != eos) & ~finished)
    nxt = None
    if lam > 0.0:
        nxt = [S.prefix_advance(y, blank, state.ctc[p], wd, N, ctc_score=s) for p, wd, s in zip(parent, word, ctc[sel])]
    out = FusedStepOutput(scores=score[sel], predicted_ids=word, beam_parent_ids=parent)
    new = FusedBeamState(log_probs=total[sel], finished=finished, lengths=lengths, lm_score=lm_total[sel], ctc=nxt)
    return (out, new, margin) if want_margin else (out, new)


class LMFusedBeamSearchDecoder(object):
    """The beam search driver over the fused step, for one utterance.  step_fn(time, predicted_ids, beam_parent_ids,
    decoder_state) -> (logits [W, C2], decoder_state) is the attention decoder as for BeamSearchDecoder /
    JointBeamSearchDecoder (ids are numpy arrays, None at time 0; a result with .detach() is accepted); lm_fn has the same
    protocol for the language model (lm_step_fn builds one).  y [T_b, n_labels + 1]: CTC log-posteriors, needed iff
    ctc_weight > 0.  min_margin: the smallest gap among the top W + 1 scores over the steps."""

    def __init__(self, step_fn, lm_fn, beam_width, n_labels, lm_weight, length_penalty_weight, max_decode_length,
                 ctc_weight=0.0, prune=True):
        self.step_fn, self.lm_fn = step_fn, lm_fn
        self.n_labels = int(n_labels)
        self.beam_width = S.check_beam_width(beam_width, self.n_labels + 1)
        self.eos_index = self.n_labels + 1
        self.lm_weight = check_lm_weight(lm_weight)
        self.ctc_weight = S.check_ctc_weight(ctc_weight)
        self.length_penalty_weight = length_penalty_weight
        self.max_decode_length = int(max_decode_length)
        self.prune = bool(prune)

    @staticmethod
    def _f64(x):
        if hasattr(x, 'detach'):
            x = x.detach().double().cpu().numpy()
        return np.asarray(x, dtype=np.float64)

    def __call__(self, decoder_state, lm_state=None, y=None):
        if self.ctc_weight > 0.0:
            if y is None:
                raise ValueError('ctc_weight > 0 needs the CTC log-posteriors y')
            y = np.asarray(y, dtype=np.float64)
        state = initial_fused_state(self.beam_width, y if self.ctc_weight > 0.0 else None, self.n_labels)
        words, parents, scores = [], [], []
        word = parent = None
        self.min_margin = float('inf')
        for k in range(self.max_decode_length):
            logits, decoder_state = self.step_fn(k, word, parent, decoder_state)
            lm_logits, lm_state = self.lm_fn(k, word, parent, lm_state)
            out, state, margin = fused_beam_search_step(k, self._f64(logits), self._f64(lm_logits), state, self.n_labels,
                                                        self.beam_width, self.lm_weight, self.length_penalty_weight,
                                                        self.ctc_weight, y, want_margin=True, prune=self.prune)
            self.min_margin = min(self.min_margin, margin)
            word, parent = out.predicted_ids, out.beam_parent_ids
            words.append(word)
            parents.append(parent)
            scores.append(out.scores)
            if bool(state.finished.all()):
                break
        w, p = np.stack(words), np.stack(parents)
        return (dict(predicted_ids=S.gather_tree_py(w, p), word=w, parent=p, scores=np.stack(scores), state=state),
                decoder_state, lm_state)
