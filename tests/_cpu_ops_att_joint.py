"""TEST INFRASTRUCTURE ONLY: the joint CTC / attention beam search on arrays -- the float64 statement of
models/attention/decoders/beam_search/ctc_prefix_score.py in the array conventions of ops.ctc_prefix_* /
ops.att_beam_select_joint / ops.att_decoder_beam_joint (what the GPU tests compare the kernels with), torch-CPU stand-ins
for those front ends layered over _cpu_ops_att_beam.install, a numpy float32 emulation of the kernels' stated operation
order (the source of the tests' fp32 bound), and the shared test cases."""
import functools

import numpy as np
import torch

import _cpu_ops_att_beam as cpub
from tensorflow_end2end_speech_recognition_amd.models.attention.decoders.beam_search import ctc_prefix_score as S

I32 = torch.int32
NEG_INF = float('-inf')


# ------------------------------------------------------------------------------------------ float64, array conventions
def _np(t, dtype=np.float64):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).astype(dtype)


def states_of(r, last, ctc_score, seq_len, W):
    """Per device row a PrefixState on the utterance's valid frames, from r [R,2,T], last [R], ctc_score [R] or None."""
    out = []
    for row in range(r.shape[0]):
        Tb = int(seq_len[row // W])
        out.append(S.PrefixState(r[row, 0, :Tb].copy(), r[row, 1, :Tb].copy(), int(last[row]),
                                 float(ctc_score[row]) if ctc_score is not None else 0.0))
    return out


def arrays_of(states, T):
    """r [R,2,T] float64 (NaN where t >= T_b: never written), last [R], ctc_score [R]."""
    r = np.full((len(states), 2, T), np.nan)
    for i, s in enumerate(states):
        r[i, 0, :len(s.r_n)], r[i, 1, :len(s.r_b)] = s.r_n, s.r_b
    return r, np.array([s.last for s in states], dtype=np.int64), np.array([s.ctc_score for s in states])


def init64(y, seq_len, W, blank):
    states = []
    for b, Tb in enumerate(seq_len):
        states += [S.prefix_init(y[:int(Tb), b], blank)] * W
    return states


def score64(y, seq_len, states, finished, cand, n_labels, blank, W):
    psi = np.full(cand.shape, NEG_INF)
    for row, st in enumerate(states):
        b = row // W
        p = S.prefix_scores(y[:int(seq_len[b]), b], blank, st, cand[row], n_labels)
        if finished is not None and finished[row]:
            p = np.where(cand[row] == n_labels + 1, p, NEG_INF)
        psi[row] = p
    return psi


def advance64(y, seq_len, states, parent, word, n_labels, blank):
    B, W = parent.shape
    out = []
    for b in range(B):
        for w in range(W):
            src = states[b * W + int(parent[b, w])]
            out.append(S.prefix_advance(y[:int(seq_len[b]), b], blank, src, int(word[b, w]), n_labels))
    return out


def select_joint64(logits, y, seq_len, states, n_labels, ctc_weight, lpw, first_step, log_probs, finished, lengths, W):
    """One joint selection per utterance on float64 arrays.  Returns a dict: word, parent [B,W], score [B,W], log_probs,
    finished, lengths, last, ctc_score [R], states (the next PrefixStates) and margin (over utterances that still search)."""
    R = logits.shape[0]
    B = R // W
    out = dict(word=np.zeros((B, W), np.int64), parent=np.zeros((B, W), np.int64), score=np.zeros((B, W)),
               log_probs=np.zeros(R), finished=np.zeros(R, bool), lengths=np.zeros(R, np.int64), states=[], margin=float('inf'))
    for b in range(B):
        rs = slice(b * W, (b + 1) * W)
        st = S.JointBeamState(log_probs=log_probs[rs], finished=finished[rs].astype(bool), lengths=lengths[rs].astype(np.int64),
                              ctc=states[rs])
        o, nxt, margin = S.joint_beam_search_step(0 if first_step else 1, logits[rs], st, y[:int(seq_len[b]), b], n_labels, W,
                                                  ctc_weight, lpw, want_margin=True)
        if not st.finished.all():
            out['margin'] = min(out['margin'], margin)
        out['word'][b], out['parent'][b], out['score'][b] = o.predicted_ids, o.beam_parent_ids, o.scores
        out['log_probs'][rs], out['finished'][rs], out['lengths'][rs] = nxt.log_probs, nxt.finished, nxt.lengths
        out['states'] += nxt.ctc
    out['last'] = np.array([s.last for s in out['states']], dtype=np.int64)
    out['ctc_score'] = np.array([s.ctc_score for s in out['states']])
    return out


# ------------------------------------------------------------------------- float32 emulation of the kernels' order
F = np.float32


def _lae32(a, b):
    """lae() of csrc/ctc_prefix.hip on float32 arrays: max + log1p(exp(min - max)), -inf for two -inf."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    m, lo = np.maximum(a, b), np.minimum(a, b)
    with np.errstate(invalid='ignore', divide='ignore'):
        out = (m + np.log1p(np.exp((lo - m).astype(F)).astype(F)).astype(F)).astype(F)
    return np.where(m == -np.inf, F(-np.inf), out).astype(F)


def emulate_score32(y32, r32, last, finished, cand, seq_len, n_labels, W):
    """ctc_prefix_score_kernel in numpy float32: phi per frame, 64-frame chunks, chunk maximum, rescaled running sum,
    exp(v - max) added frame by frame, max + log(sum)."""
    R, K = cand.shape
    psi = np.full((R, K), -np.inf, F)
    for row in range(R):
        b, lst = row // W, int(last[row])
        Tb = int(seq_len[b])
        rn, rb = r32[row, 0, :Tb], r32[row, 1, :Tb]
        same_phi, diff_phi = np.full(Tb, -np.inf, F), np.full(Tb, -np.inf, F)
        same_phi[0] = diff_phi[0] = F(0.0) if lst < 0 else F(-np.inf)
        same_phi[1:], diff_phi[1:] = rb[:-1], _lae32(rn[:-1], rb[:-1])
        fin = finished is not None and bool(finished[row])
        for k in range(K):
            c = int(cand[row, k])
            if c == n_labels + 1:
                psi[row, k] = _lae32(rn[Tb - 1], rb[Tb - 1])
            if not (0 <= c < n_labels) or fin:
                continue
            v = ((same_phi if c == lst else diff_phi) + y32[:Tb, b, c]).astype(F)
            m, s = F(-np.inf), F(0.0)
            for t0 in range(0, Tb, 64):
                ch = v[t0:t0 + 64]
                mc = ch.max()
                if mc == -np.inf:
                    continue
                if mc > m:
                    s = F(s * np.exp(F(m - mc)).astype(F))
                    m = mc
                for x in ch:
                    s = F(s + np.exp(F(x - m)).astype(F))
            psi[row, k] = F(m + np.log(s).astype(F)) if m != -np.inf else F(-np.inf)
    return psi


def emulate_advance32(y32, r32, last, parent, word, seq_len, n_labels, blank):
    """ctc_prefix_advance_kernel in numpy float32 (T dependent steps of two lae each)."""
    B, W = parent.shape
    out = np.full(r32.shape, np.nan, F)
    for b in range(B):
        Tb = int(seq_len[b])
        for w in range(W):
            src, wd = b * W + int(parent[b, w]), int(word[b, w])
            rn, rb = r32[src, 0, :Tb], r32[src, 1, :Tb]
            if not 0 <= wd < n_labels:
                out[b * W + w, 0, :Tb], out[b * W + w, 1, :Tb] = rn, rb
                continue
            lst = int(last[src])
            phi = np.concatenate([[F(-np.inf)], rb[:-1] if wd == lst else _lae32(rn[:-1], rb[:-1])]).astype(F)
            cn, cb = (y32[0, b, wd] if lst < 0 else F(-np.inf)), F(-np.inf)
            on, ob = [cn], [cb]
            for t in range(1, Tb):
                nn = F(_lae32(cn, phi[t]) + y32[t, b, wd])
                nb = F(_lae32(cn, cb) + y32[t, b, blank])
                cn, cb = nn, nb
                on.append(cn)
                ob.append(cb)
            out[b * W + w, 0, :Tb], out[b * W + w, 1, :Tb] = on, ob
    return out


def max_err(got, want):
    """Largest |got - want| over the finite entries of `want`; -inf must meet -inf exactly and nothing may be NaN (NaN in
    `want` marks entries that are never written: ignored).  Returns (error, largest finite |want|)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    keep = ~np.isnan(want)
    g, w = got[keep], want[keep]
    assert not np.isnan(g).any(), 'NaN in the result'
    inf = np.isinf(w)
    assert np.array_equal(g[inf], w[inf]), 'an infeasible entry is not exactly -inf'
    assert not np.isinf(g[~inf]).any(), 'a feasible entry is infinite'
    if not (~inf).any():
        return 0.0, 0.0
    return float(np.abs(g[~inf] - w[~inf]).max()), float(np.abs(w[~inf]).max())


# ------------------------------------------------------------------------------------------------------ shared cases
PREFIX_T, PREFIX_SEQ = 70, (70, 65, 64, 63, 2, 1)
PREFIX_CASES = [(W, Cc) for W in (1, 5, 32) for Cc in (4, 41, 3388)]


def ctc_posteriors(rng, T, B, Cc, boost=2.0):
    """fp32 log-posteriors [T,B,Cc] with the blank (last class) holding most of the mass (boost, a number or one per
    utterance: the blank's logit is raised by log(Cc) + boost), so that whole-utterance scores stay above -64 at any Cc,
    and their float64 copy (both sides of a comparison read the same numbers)."""
    lg = rng.randn(T, B, Cc)
    lg[:, :, Cc - 1] += np.log(Cc) + np.broadcast_to(np.asarray(boost, dtype=np.float64), (B,))[None, :]
    y32 = S.log_softmax(lg).astype(np.float32)
    return y32, y32.astype(np.float64)


@functools.lru_cache(maxsize=None)
def prefix_case(W, Cc):
    """Operands and float64 expectations of the scorer / advance test: T = 70 (crosses the 64-frame chunk), B = 6 with
    seq_len 70, 65, 64, 63, 2, 1; hypotheses of depth 0, 1 and 3 (on the 2- and 1-frame utterances some no longer fit:
    their state is all -inf), one finished row; K = W + 3 candidates per row: the hypothesis's own last label (a repeat),
    <SOS>, <EOS> and W random labels.  Then a selection for ctc_prefix_advance: random parents (utterance 0: slot 2 chosen
    three times, slots 1 and 3 by none, from W = 5 on), words that include <EOS>, <EOS> behind the finished row."""
    rng = np.random.RandomState(1000 * W + Cc)
    T, seq, B, N, blank = PREFIX_T, np.array(PREFIX_SEQ), len(PREFIX_SEQ), Cc - 1, Cc - 1
    R, K = B * W, W + 3
    y32, y = ctc_posteriors(rng, T, B, Cc)
    states, depth = [], np.zeros(R, np.int64)
    for b in range(B):
        for w in range(W):
            d = 3 if (b >= 4 and w == 0) else (0, 1, 3)[(b + w) % 3]
            st = S.prefix_init(y[:seq[b], b], blank)
            g = list(rng.randint(0, N, size=d))
            if d == 3 and w % 2 == 0 and N > 1:
                g[1] = g[0]                                  # an immediate repeat inside the hypothesis
            for c in g:
                st = S.prefix_advance(y[:seq[b], b], blank, st, int(c), N)
            states.append(st._replace(ctc_score=S.prefix_eos(st)))
            depth[b * W + w] = d
    finished = np.zeros(R, np.int64)
    finished[1 * W + 0] = 1                                  # utterance 1, slot 0: depth 1
    cand = rng.randint(0, N, size=(R, K))
    for row, st in enumerate(states):
        cand[row, 0] = st.last if st.last >= 0 else cand[row, 0]
        cand[row, 1], cand[row, 2] = N, N + 1
    psi = score64(y, seq, states, finished, cand, N, blank, W)
    parent = rng.randint(0, W, size=(B, W))
    if W >= 5:
        parent[0] = rng.randint(4, W, size=W)
        parent[0, :5] = [2, 2, 2, 0, 4]
    word = rng.randint(0, N, size=(B, W))
    word[rng.rand(B, W) < 0.25] = N + 1
    for b in range(B):
        for w in range(W):
            if finished[b * W + parent[b, w]]:
                word[b, w] = N + 1
            elif word[b, w] != N + 1 and rng.rand() < 0.3 and states[b * W + parent[b, w]].last >= 0:
                word[b, w] = states[b * W + parent[b, w]].last         # a repeat of the parent's last label
    r, last, _ = arrays_of(states, T)
    r_next, _, _ = arrays_of(advance64(y, seq, states, parent, word, N, blank), T)
    return dict(W=W, Cc=Cc, N=N, blank=blank, T=T, B=B, R=R, K=K, seq_len=seq, y32=y32, y=y, r=r, last=last, depth=depth,
                finished=finished, cand=cand, psi=psi, parent=parent, word=word, r_next=r_next)


SELECT_CASES = [(2, 3), (5, 40), (20, 3389)]                 # (W, C2)
SELECT_SEQ, SELECT_T, SELECT_STEPS = (24, 9, 3), 24, 4


def select_case(W, C2, lam, lpw, seed):
    """A 4-step joint search of 3 utterances (24, 9 and 3 frames: on the last one hypotheses stop fitting) in float64 over
    seeded random logits whose <EOS> grows with the step; per step the statement's input and output state.  Returns
    (case dict, min margin)."""
    rng = np.random.RandomState(seed)
    N, T, seq, B = C2 - 2, SELECT_T, np.array(SELECT_SEQ), len(SELECT_SEQ)
    R = B * W
    y32, y = ctc_posteriors(rng, T, B, N + 1)
    states = init64(y, seq, W, N)
    lp, fin, ln = np.zeros(R), np.zeros(R, bool), np.zeros(R, np.int64)
    steps, margin = [], float('inf')
    for k in range(SELECT_STEPS):
        lg = (rng.randn(R, C2) * 6.0).astype(np.float32)
        lg[:, N + 1] += 3.0 * k - 4.0
        r, last, ctc = arrays_of(states, T)
        o = select_joint64(lg.astype(np.float64), y, seq, states, N, lam, lpw, k == 0, lp.astype(np.float32).astype(np.float64),
                           fin, ln, W)
        steps.append(dict(logits=lg, first=k == 0, r=r, last=last, ctc_score=ctc, log_probs=lp.astype(np.float32),
                          finished=fin.astype(np.int32), lengths=ln.astype(np.int32), out=o))
        margin = min(margin, o['margin'])
        states, lp, fin, ln = o['states'], o['log_probs'], o['finished'], o['lengths']
    return dict(W=W, C2=C2, N=N, T=T, B=B, seq_len=seq, y32=y32, y=y, steps=steps), margin


def table_case(seed, W=3, N=6, steps=6, T=12):
    """A step function whose logits depend on the step and the last word (as test_beam_search_decoder_class_surface), and
    CTC log-posteriors for it."""
    rng = np.random.RandomState(seed)
    C2 = N + 2
    table = torch.tensor(rng.uniform(-2, 2, size=(steps, C2, C2)))
    _, y = ctc_posteriors(rng, T, 1, N + 1, boost=0.0)

    def step_fn(k, word, parent, state):
        last = torch.full((W,), N, dtype=torch.long) if word is None else word.long()
        return table[k][last], state
    return step_fn, y[:, 0], W, N, steps


def best_hypotheses(seed, lam=0.5):
    from tensorflow_end2end_speech_recognition_amd.models.attention.decoders.beam_search.beam_search_decoder import (
        BeamSearchDecoder, cut_at_eos)
    step_fn, y, W, N, steps = table_case(seed)
    att = BeamSearchDecoder(step_fn, W, N + 2, N + 1, 0.0, steps)
    final, _ = att(None)
    joint = S.JointBeamSearchDecoder(step_fn, W, N, lam, 0.0, steps)
    out, _ = joint(None, y)
    return (cut_at_eos(final.predicted_ids[:, 0], N + 1), cut_at_eos(out['predicted_ids'][:, 0], N + 1),
            min(att.min_margin, joint.min_margin))


LOOP_SEQ = (40, 31, 17)                                     # the utterance lengths of test_gpu_att_beam.beam_loop_arrays


def loop_posteriors(seed):
    """CTC log-posteriors [40,3,11] for the operands of the beam loop test (12 attention classes: 10 labels): utterance 0,
    which that test makes finish early, has a dominant blank; on the others ending early costs CTC probability."""
    return ctc_posteriors(np.random.RandomState(10000 + seed), 40, 3, 11, boost=np.array([2.0, 0.0, 0.0]))


# ------------------------------------------------------------------------------------------------- torch-CPU stand-ins
def _log_softmax_rows(x2d, out=None):
    res = torch.log_softmax(x2d.double(), dim=1).float()
    if out is not None:
        out.copy_(res)
        return out
    return res


def _blank(y, blank):
    return y.shape[2] - 1 if blank is None else int(blank)


def _ctc_prefix_init(y, seq_len, beam_width, blank=None):
    W, T = int(beam_width), y.shape[0]
    r, last, score = arrays_of(init64(_np(y), _np(seq_len, np.int64), W, _blank(y, blank)), T)
    return torch.tensor(r, dtype=torch.float32), torch.tensor(last, dtype=I32), torch.tensor(score, dtype=torch.float32)


def _ctc_prefix_score(y, seq_len, r, last, finished, cand, n_labels, blank=None):
    sl = _np(seq_len, np.int64)
    W = cand.shape[0] // len(sl)
    states = states_of(_np(r), _np(last, np.int64), None, sl, W)
    psi = score64(_np(y), sl, states, _np(finished, np.int64) if finished is not None else None, _np(cand, np.int64),
                  int(n_labels), _blank(y, blank), W)
    return torch.tensor(psi, dtype=torch.float32)


def _ctc_prefix_advance(y, seq_len, r, last, parent, word, n_labels, blank=None):
    sl = _np(seq_len, np.int64)
    W = parent.shape[1]
    states = states_of(_np(r), _np(last, np.int64), None, sl, W)
    nxt = advance64(_np(y), sl, states, _np(parent, np.int64), _np(word, np.int64), int(n_labels), _blank(y, blank))
    return torch.tensor(arrays_of(nxt, y.shape[0])[0], dtype=torch.float32)


LAST = {}                 # what the last joint select saw: 'margin', and 'states' (the float64 next state)


def _att_beam_select_joint(logits, y, seq_len, r, last, ctc_score, n_labels, ctc_weight, length_penalty_weight, first_step,
                           log_probs, finished, lengths, unfinished=None, blank=None, _states=None):
    sl = _np(seq_len, np.int64)
    R = logits.shape[0]
    W = R // len(sl)
    states = _states if _states is not None else states_of(_np(r), _np(last, np.int64), _np(ctc_score), sl, W)
    o = select_joint64(_np(logits), _np(y), sl, states, int(n_labels), float(ctc_weight), length_penalty_weight,
                       bool(first_step), _np(log_probs), _np(finished, np.int64) != 0, _np(lengths, np.int64), W)
    LAST['margin'], LAST['states'] = o['margin'], o['states']
    if unfinished is not None:
        unfinished += int((~o['finished']).sum())
    t = lambda a, dt: torch.tensor(np.asarray(a), dtype=dt)                             # noqa: E731
    return (t(o['word'], I32), t(o['parent'], I32), t(o['score'], torch.float32), t(o['log_probs'], torch.float32),
            t(o['finished'], I32), t(o['lengths'], I32), t(o['last'], I32), t(o['ctc_score'], torch.float32))


def _att_decoder_beam_joint(a, W_av, W_out, b_out, embedding, eos, beam_width, y, seq_len, ctc_weight,
                            length_penalty_weight=0.0, check_every=8, blank=None):
    """_cpu_ops_att_beam._att_decoder_beam's loop with the joint selection in place of its select; the prefix state is
    carried in float64 between the steps."""
    C2 = W_out.shape[1]
    N, W = C2 - 2, int(beam_width)
    S.check_beam_width(W, N + 1)
    if not 0.0 < float(ctc_weight) <= 1.0:
        raise ValueError('ctc_weight must be in (0, 1]')
    sl = _np(seq_len, np.int64)
    carried = dict(states=init64(_np(y), sl, W, _blank(y, blank)))

    def select(lg, W_, eos_, lpw, first, lp, fin, ln, unfinished=None):
        res = _att_beam_select_joint(lg, y, seq_len, None, None, None, N, ctc_weight, lpw, first, lp, fin, ln,
                                     _states=carried['states'])
        carried['states'] = LAST['states']
        cpub.LAST['margin'] = LAST['margin']
        return res[:6]

    saved = cpub._att_beam_select
    cpub._att_beam_select = select
    try:
        out = cpub._att_decoder_beam(a, W_av, W_out, b_out, embedding, eos, W, length_penalty_weight, check_every)
    finally:
        cpub._att_beam_select = saved
    B = a['B'] // W
    out['ctc_score'] = torch.tensor([s.ctc_score for s in carried['states']], dtype=torch.float32).view(B, W)
    return out


def att_joint_counts(device=0):
    return dict(score=0, advance=0, joint_select=0)


STAND_INS = dict(log_softmax_rows=_log_softmax_rows, ctc_prefix_init=_ctc_prefix_init, ctc_prefix_score=_ctc_prefix_score,
                 ctc_prefix_advance=_ctc_prefix_advance, att_beam_select_joint=_att_beam_select_joint,
                 att_decoder_beam_joint=_att_decoder_beam_joint)


def install(monkeypatch):
    ops = cpub.install(monkeypatch)
    for name, fn in STAND_INS.items():
        assert hasattr(ops, name), name
        monkeypatch.setattr(ops, name, fn)
    return ops
