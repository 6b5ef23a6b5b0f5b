"""TEST INFRASTRUCTURE ONLY: shallow LM fusion on arrays -- the float64 statement of
models/attention/decoders/beam_search/lm_fusion.py in the array conventions of ops.lm_step / ops.att_beam_select_fused /
ops.lm_beam_reorder / ops.att_decoder_beam_lm (what the GPU tests compare the kernels with), torch-CPU stand-ins for those
front ends layered over _cpu_ops_att_joint.install, a numpy float32 emulation of the selection kernels' stated operation
order (the source of the tests' fp32 bound), and the shared test cases."""
import numpy as np
import torch

import _cpu_ops_att_beam as cpub
import _cpu_ops_att_joint as J
from tensorflow_end2end_speech_recognition_amd.models.attention.decoders.beam_search import ctc_prefix_score as S
from tensorflow_end2end_speech_recognition_amd.models.attention.decoders.beam_search import lm_fusion as LF

I32 = torch.int32
F = np.float32
NEG_INF = float('-inf')
LM_WEIGHT = 0.3
_np = J._np


# ------------------------------------------------------------------------------------------------- the language model
def lm_params(rng, C2, Em, H, L, clip=1.5, scale=0.4, out_scale=1.0):
    """A random LSTM language model in float32 numpy (both sides of a comparison read the same numbers): the dict of
    lm_fusion.lm_step.  clip 1.5 with these scales is reached by some cells (asserted where it matters)."""
    kernels, biases = [], []
    for l in range(L):
        din = Em if l == 0 else H
        kernels.append((rng.randn(din + H, 4 * H) * scale).astype(F))
        biases.append((rng.randn(4 * H) * 0.2).astype(F))
    return dict(emb=rng.randn(C2, Em).astype(F), kernels=kernels, biases=biases,
                W_out=(rng.randn(H, C2) * out_scale).astype(F), b_out=(rng.randn(C2) * 0.2).astype(F), cell_clip=clip)


def params_torch(p, device=None):
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=device)             # noqa: E731
    return dict(emb=t(p['emb']), kernels=[t(k) for k in p['kernels']], biases=[t(b) for b in p['biases']],
                W_out=t(p['W_out']), b_out=t(p['b_out']), cell_clip=p.get('cell_clip'))


def params_numpy(lm):
    n = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)          # noqa: E731
    return dict(emb=n(lm['emb']), kernels=[n(k) for k in lm['kernels']], biases=[n(b) for b in lm['biases']],
                W_out=n(lm['W_out']), b_out=n(lm['b_out']), cell_clip=lm.get('cell_clip'))


# ------------------------------------------------------------------------------------------ float64, array conventions
def select_fused64(logits, lm_logits, n_labels, lm_weight, lpw, first_step, log_probs, finished, lengths, lm_score, W,
                   ctc_weight=0.0, y=None, seq_len=None, states=None):
    """One fused selection per utterance on float64 arrays.  Returns a dict: word, parent, score [B,W], log_probs, finished,
    lengths, lm_score [R], margin (over utterances that still search) and, with CTC, last, ctc_score [R] and states."""
    R = logits.shape[0]
    B = R // W
    out = dict(word=np.zeros((B, W), np.int64), parent=np.zeros((B, W), np.int64), score=np.zeros((B, W)),
               log_probs=np.zeros(R), finished=np.zeros(R, bool), lengths=np.zeros(R, np.int64), lm_score=np.zeros(R),
               states=[] if ctc_weight > 0 else None, margin=float('inf'))
    for b in range(B):
        rs = slice(b * W, (b + 1) * W)
        st = LF.FusedBeamState(log_probs=log_probs[rs], finished=finished[rs].astype(bool), lengths=lengths[rs].astype(np.int64),
                               lm_score=lm_score[rs], ctc=states[rs] if ctc_weight > 0 else None)
        o, nxt, margin = LF.fused_beam_search_step(0 if first_step else 1, logits[rs], lm_logits[rs], st, n_labels, W, lm_weight,
                                                   lpw, ctc_weight, y[:int(seq_len[b]), b] if ctc_weight > 0 else None,
                                                   want_margin=True)
        if not st.finished.all():
            out['margin'] = min(out['margin'], margin)
        out['word'][b], out['parent'][b], out['score'][b] = o.predicted_ids, o.beam_parent_ids, o.scores
        out['log_probs'][rs], out['finished'][rs], out['lengths'][rs] = nxt.log_probs, nxt.finished, nxt.lengths
        out['lm_score'][rs] = nxt.lm_score
        if ctc_weight > 0:
            out['states'] += nxt.ctc
    if ctc_weight > 0:
        out['last'] = np.array([s.last for s in out['states']], dtype=np.int64)
        out['ctc_score'] = np.array([s.ctc_score for s in out['states']])
    return out


# ------------------------------------------------------------------------- float32 emulation of the kernels' order
def lse32(x):
    """row_lse of csrc/att_beam.hip (the order of att_beam_select_kernel) on one float32 row: lane l takes the columns l,
    l + 64, ... in ascending order, the 64 partials meet in a butterfly (xor 32 .. 1); max + log(sum)."""
    x = np.asarray(x, F)
    pad = (-len(x)) % 64
    g = np.concatenate([x, np.full(pad, -np.inf, F)]).reshape(-1, 64)
    m = F(x.max())
    s = np.add.accumulate(np.exp((g - m).astype(F)).astype(F), axis=0, dtype=F)[-1]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = (s + s[lanes ^ o]).astype(F)
    return F(m + F(np.log(s[0])))


def emulate_select32(step, W, n_labels, lam, mu, lpw, y32=None, seq_len=None):
    """att_select_candidates_kernel<true> + (ctc_prefix_score_kernel) + att_select_rank_kernel<CTC, true> of csrc/att_beam.hip
    in numpy float32 on one step of select_case, evaluated AT the float64 statement's selection (word / parent of
    step['out']): the fp32 score, log_probs, lm_score and ctc_score of those W winners per utterance.  Returns a dict of
    [R] float32 arrays."""
    o = step['out']
    N, C2, eos = n_labels, n_labels + 2, n_labels + 1
    B = o['word'].shape[0]
    R = B * W
    lam32, mu32, a = F(lam), F(mu), F(lpw)
    res = dict(score=np.zeros(R, F), log_probs=np.zeros(R, F), lm_score=np.zeros(R, F), ctc_score=np.zeros(R, F))
    pen6 = np.power(F(6.0), a, dtype=F)
    for b in range(B):
        for w in range(W):
            pa, wd = int(o['parent'][b, w]), int(o['word'][b, w])
            row = b * W + pa
            fin = bool(step['finished'][row])
            lp, ls = F(step['log_probs'][row]), F(step['lm_score'][row])
            if fin:
                tot, lmt = F(lp + F(0)), F(ls + F(0))
            else:
                x, z = step['logits'][row].astype(F), step['lm_logits'][row].astype(F)
                tot = F(lp + F(x[wd] - lse32(x)))
                lmt = F(ls + F(z[wd] - lse32(z)))
            fused = F(F(F(1.0) - lam32) * tot)
            ctc = F(0)
            if lam > 0:
                if fin:
                    ctc = F(step['ctc_score'][row])
                else:
                    ctc = J.emulate_score32(y32, step['r'].astype(F), step['last'], step['finished'],
                                            _one_cand(R, row, wd), seq_len, N, W)[row, 0]
                fused = F(fused + F(lam32 * ctc))
            fused = F(fused + F(mu32 * lmt))
            ln = int(step['lengths'][row]) + (1 if (wd != eos and not fin) else 0)
            sc = fused if lpw == 1.0 else F(fused / F(np.power(F(5.0 + ln), a, dtype=F) / pen6))
            i = b * W + w
            res['score'][i], res['log_probs'][i], res['lm_score'][i], res['ctc_score'][i] = sc, tot, lmt, ctc
    return res


def _one_cand(R, row, wd):
    c = np.full((R, 1), -1, np.int64)
    c[row, 0] = wd
    return c


def emulation_error(case, W, lam, mu, lpw):
    """Largest |fp32 emulation - float64 statement| over score / log_probs / lm_score / ctc_score of every step of a case."""
    worst = 0.0
    for s in case['steps']:
        e32 = emulate_select32(s, W, case['N'], lam, mu, lpw, case.get('y32'), case['seq_len'])
        o = s['out']
        for k in ('score', 'log_probs', 'lm_score') + (('ctc_score',) if lam > 0 else ()):
            worst = max(worst, float(np.abs(e32[k].astype(np.float64) - np.asarray(o[k]).reshape(-1)).max()))
    return worst


# ------------------------------------------------------------------------------------------------------ shared cases
SELECT_CASES = [(2, 4), (5, 40), (20, 3389)]                 # (W, C2)
SELECT_LAMS, SELECT_LPWS = (0.0, 0.3), (0.0, 0.6, 1.0)
SELECT_STEPS = 4


def select_case(W, C2, lam, lpw, seed, mu=LM_WEIGHT, att_scale=6.0, lm_scale=3.0):
    """_cpu_ops_att_joint.select_case's generator plus LM logits: a 4-step fused search of 3 utterances (24, 9 and 3 frames)
    in float64 over seeded random attention logits (scale 6, <EOS> growing with the step) and LM logits (scale 3); per step
    the statement's input and output state.  lam = 0: no CTC arrays.  Returns (case dict, min margin)."""
    rng = np.random.RandomState(seed)
    N, T, seq, B = C2 - 2, J.SELECT_T, np.array(J.SELECT_SEQ), len(J.SELECT_SEQ)
    R = B * W
    y32, y = J.ctc_posteriors(rng, T, B, N + 1)
    states = J.init64(y, seq, W, N) if lam > 0 else None
    lp, fin, ln, ls = np.zeros(R), np.zeros(R, bool), np.zeros(R, np.int64), np.zeros(R)
    steps, margin = [], float('inf')
    for k in range(SELECT_STEPS):
        lg = (rng.randn(R, C2) * att_scale).astype(F)
        lg[:, N + 1] += 3.0 * k - 4.0
        zl = (rng.randn(R, C2) * lm_scale).astype(F)
        st = dict(logits=lg, lm_logits=zl, first=k == 0, log_probs=lp.astype(F), lm_score=ls.astype(F),
                  finished=fin.astype(np.int32), lengths=ln.astype(np.int32))
        if lam > 0:
            st['r'], st['last'], st['ctc_score'] = J.arrays_of(states, T)
        o = select_fused64(lg.astype(np.float64), zl.astype(np.float64), N, mu, lpw, k == 0, st['log_probs'].astype(np.float64),
                           fin, ln, st['lm_score'].astype(np.float64), W, lam, y, seq, states)
        st['out'] = o
        steps.append(st)
        margin = min(margin, o['margin'])
        states, lp, fin, ln, ls = o['states'], o['log_probs'], o['finished'], o['lengths'], o['lm_score']
    return dict(W=W, C2=C2, N=N, T=T, B=B, seq_len=seq, y32=y32, y=y, steps=steps), margin


# (W, C2, ctc_weight, length_penalty_weight) -> seed under which the float64 statement's selection margin is >= 1e-3 at every
# step of select_case (asserted in the tests; found on the CPU, scripts/probe_lm_fusion.py --seeds)
SELECT_SEEDS = {(2, 4, 0.0, 0.0): 0, (2, 4, 0.0, 0.6): 0, (2, 4, 0.0, 1.0): 0, (2, 4, 0.3, 0.0): 0,
                (2, 4, 0.3, 0.6): 0, (2, 4, 0.3, 1.0): 0, (5, 40, 0.0, 0.0): 0, (5, 40, 0.0, 0.6): 0,
                (5, 40, 0.0, 1.0): 0, (5, 40, 0.3, 0.0): 0, (5, 40, 0.3, 0.6): 0, (5, 40, 0.3, 1.0): 0,
                (20, 3389, 0.0, 0.0): 44, (20, 3389, 0.0, 0.6): 3, (20, 3389, 0.0, 1.0): 44, (20, 3389, 0.3, 0.0): 2,
                (20, 3389, 0.3, 0.6): 6, (20, 3389, 0.3, 1.0): 2}

LOOP_LM = dict(H=64, L=2, Em=8)


def loop_lm(seed, C2=12):
    """The language model of the native loop test: H = 64, L = 2, Em_lm = 8 over the loop's 12 classes."""
    return lm_params(np.random.RandomState(20000 + seed), C2, LOOP_LM['Em'], LOOP_LM['H'], LOOP_LM['L'], out_scale=0.5)


# (W, attention type, ctc_weight) -> seed of the native loop test (scripts/probe_lm_fusion.py --seeds)
LOOP_SEEDS = {(1, 'bahdanau_content', 0.0): 1, (1, 'bahdanau_content', 0.3): 1, (1, 'location', 0.0): 0,
              (1, 'location', 0.3): 0, (4, 'bahdanau_content', 0.0): 1, (4, 'bahdanau_content', 0.3): 1,
              (4, 'location', 0.0): 0, (4, 'location', 0.3): 0, (5, 'bahdanau_content', 0.0): 1,
              (5, 'bahdanau_content', 0.3): 1, (5, 'location', 0.0): 4, (5, 'location', 0.3): 0}


# ------------------------------------------------------------------------------------------------- torch-CPU stand-ins
def _lm_step(lm, words, c, h):
    logits, (c2, h2) = LF.lm_step(params_numpy(lm), _np(words, np.int64), (_np(c), _np(h)))
    t = lambda a: torch.tensor(a, dtype=torch.float32)                                         # noqa: E731
    return t(logits), t(c2), t(h2)


LAST = {}                 # what the last fused select saw: 'margin', 'states' (float64 CTC states), 'lm_score' (float64)


def _att_beam_select_fused(logits, lm_logits, n_labels, lm_weight, length_penalty_weight, first_step, log_probs, finished,
                           lengths, lm_score, beam_width=None, ctc_weight=0.0, y=None, seq_len=None, r=None, last=None,
                           ctc_score=None, unfinished=None, blank=None, _states=None, _lm_score=None):
    R = logits.shape[0]
    lam = float(ctc_weight)
    if not float(lm_weight) > 0.0:
        raise ValueError('lm_weight must be > 0')
    sl = _np(seq_len, np.int64) if lam > 0 else None
    W = R // len(sl) if lam > 0 else int(beam_width)
    states = None
    if lam > 0:
        states = _states if _states is not None else J.states_of(_np(r), _np(last, np.int64), _np(ctc_score), sl, W)
    o = select_fused64(_np(logits), _np(lm_logits), int(n_labels), float(lm_weight), length_penalty_weight, bool(first_step),
                       _np(log_probs), _np(finished, np.int64) != 0, _np(lengths, np.int64),
                       _lm_score if _lm_score is not None else _np(lm_score), W, lam, _np(y) if lam > 0 else None, sl, states)
    LAST.update(margin=o['margin'], states=o['states'], lm_score=o['lm_score'])
    if unfinished is not None:
        unfinished += int((~o['finished']).sum())
    t = lambda a, dt: torch.tensor(np.asarray(a), dtype=dt)                                     # noqa: E731
    return (t(o['word'], I32), t(o['parent'], I32), t(o['score'], torch.float32), t(o['log_probs'], torch.float32),
            t(o['finished'], I32), t(o['lengths'], I32), t(o['lm_score'], torch.float32),
            t(o['last'], I32) if lam > 0 else None, t(o['ctc_score'], torch.float32) if lam > 0 else None)


def _lm_beam_reorder(parent, word, c_src, h_src, emb):
    pr = cpub._rows(parent)
    L, R, H = c_src.shape
    Em = emb.shape[1]
    c, h = c_src[:, pr].clone(), h_src[:, pr].clone()
    ins = []
    for l in range(L):
        x = emb[word.reshape(-1).long()] if l == 0 else torch.zeros((R, H))
        ins.append(torch.cat([x, h[l]], dim=1))
    return c, h, ins


def _att_decoder_beam_lm(a, W_av, W_out, b_out, embedding, eos, beam_width, lm, lm_weight, length_penalty_weight=0.0,
                         check_every=8, y=None, seq_len=None, ctc_weight=0.0, blank=None):
    """_cpu_ops_att_beam._att_decoder_beam's loop with the fused selection in place of its select; the LM state, lm_score and
    the CTC prefix state are carried in float64 between the steps."""
    C2 = W_out.shape[1]
    N, W = C2 - 2, int(beam_width)
    S.check_beam_width(W, N + 1)
    lam, mu = float(ctc_weight), float(lm_weight)
    if not mu > 0.0 or not 0.0 <= lam <= 1.0:
        raise ValueError('lm_weight must be > 0 and ctc_weight in [0, 1]')
    R = a['B']
    p = params_numpy(lm)
    sl = _np(seq_len, np.int64) if lam > 0 else None
    car = dict(states=J.init64(_np(y), sl, W, J._blank(y, blank)) if lam > 0 else None, lm=LF.lm_initial_state(p, R),
               words=np.full(R, N, np.int64), lm_score=np.zeros(R))

    def select(lg, W_, eos_, lpw, first, lp, fin, ln, unfinished=None):
        lm_logits, new = LF.lm_step(p, car['words'], car['lm'])
        res = _att_beam_select_fused(lg, lm_logits, N, mu, lpw, first, lp, fin, ln, None, W, lam, y, seq_len,
                                     _states=car['states'], _lm_score=car['lm_score'])
        pr = cpub._rows(res[1]).numpy()
        car.update(states=LAST['states'], lm_score=LAST['lm_score'], lm=(new[0][:, pr], new[1][:, pr]),
                   words=res[0].reshape(-1).numpy().astype(np.int64))
        cpub.LAST['margin'] = LAST['margin']
        return res[:6]

    saved = cpub._att_beam_select
    cpub._att_beam_select = select
    try:
        out = cpub._att_decoder_beam(a, W_av, W_out, b_out, embedding, eos, W, length_penalty_weight, check_every)
    finally:
        cpub._att_beam_select = saved
    B = R // W
    out['lm_score'] = torch.tensor(car['lm_score'], dtype=torch.float32).view(B, W)
    if lam > 0:
        out['ctc_score'] = torch.tensor([s.ctc_score for s in car['states']], dtype=torch.float32).view(B, W)
    return out


def att_lm_counts(device=0):
    return dict(lm_step=0, fused_select=0, lm_reorder=0)


STAND_INS = dict(lm_step=_lm_step, att_beam_select_fused=_att_beam_select_fused, lm_beam_reorder=_lm_beam_reorder,
                 att_decoder_beam_lm=_att_decoder_beam_lm)


def install(monkeypatch):
    ops = J.install(monkeypatch)
    for name, fn in STAND_INS.items():
        assert hasattr(ops, name), name
        monkeypatch.setattr(ops, name, fn)
    return ops
