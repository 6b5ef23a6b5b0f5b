"""Runs the reference's OWN beam search functions (unchanged files under /root/reference) on the eager float64 TensorFlow
stand-in of tests/golden/tf_shim and records what they compute: tests/golden/att_beam_v1.npz.

    python tests/golden/make_golden_att_beam.py          # needs /root/reference; the GPU box never runs this

What is executed (reference file:line):
  * models/attention/decoders/beam_search/beam_search_decoder.py:234-332 -- beam_search_step
  * models/attention/decoders/beam_search/util.py:37-68, 71-95, 14-26 -- mask_probs, normalize_score, gather_tree_py
The module imports an RNNDecoder that attention_decoder.py does not define (the reason the reference's beam search is
dead code); the name is planted before the import.  tf.mod / tf.div, which the stand-in lacks, are added to its module
object here; tf_shim itself is not edited.  choose_successors_fn is a stable numpy top-k (tf.nn.top_k's order: score
descending, index ascending).

Per case (tests/_att_beam_golden.py: cases(), logits()) a chain of steps is run, each step on the state the previous one
returned, and per step the input state, the selection and the output state are recorded, plus gather_tree_py over the
chain's (word, parent).  Asserted per step: neighbouring scores among the top W + 1 candidates, and at the W-th / (W+1)-th
place of every unfinished row (the kernel's prune boundary), differ by more than 1e-3 -- except the ties the tie case is
about -- and every recorded value is below 64 in magnitude.  A step's seed is the first one under which all of that
holds."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'tf_shim'))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, '/root/reference')

import tensorflow as tf                                    # noqa: E402  (the stand-in)
import torch                                               # noqa: E402

import _att_beam_golden as G                               # noqa: E402

tf.mod = lambda a, b, name=None: tf.convert_to_tensor(np.mod(np.asarray(_np(a)), _np(b)))


def _np(x):
    return x.numpy() if hasattr(x, 'numpy') else np.asarray(x)


def _div(a, b, name=None):
    """TF1's tf.div: floor division of integers, true division of floats."""
    a_, b_ = np.asarray(_np(a)), np.asarray(_np(b))
    if a_.dtype.kind in 'iu' and b_.dtype.kind in 'iu':
        return tf.convert_to_tensor(a_ // b_)
    return tf.convert_to_tensor(a_ / b_)


tf.div = _div

from models.attention.decoders import attention_decoder as ref_attention_decoder  # noqa: E402

ref_attention_decoder.RNNDecoder = object

from models.attention.decoders.beam_search.beam_search_decoder import beam_search_step  # noqa: E402
from models.attention.decoders.beam_search.namedtuple import BeamSearchDecoderState     # noqa: E402
from models.attention.decoders.beam_search import util as ref_util                       # noqa: E402


def stable_top_k(scores_flat, k):
    s = _np(scores_flat).reshape(-1)
    idx = np.argsort(-s, kind='stable')[:k]
    return tf.convert_to_tensor(s[idx]), tf.convert_to_tensor(idx.astype(np.int64))


class MarginError(Exception):
    pass


def margins_ok(case, time, x, state, out):
    """The assertions on one step, on the statement's own float64 scores (recomputed with numpy from the same inputs)."""
    W, C2, a = case['W'], case['C2'], case['alpha']
    eos = C2 - 1
    lp, fin, ln = state
    p = x - x.max(1, keepdims=True)
    p = p - np.log(np.exp(p).sum(1, keepdims=True))
    p[fin] = np.finfo(np.float32).min
    p[fin, eos] = 0.0
    total = lp[:, None] + p
    clen = ln[:, None] + (np.arange(C2)[None] != eos) * (~fin[:, None])
    score = total if a == 1.0 else total / ((5.0 + clen) ** a / 6.0 ** a)
    live_rows = [w for w in range(W) if not fin[w]] if time > 0 else [0]
    rows = {w: np.sort(score[w])[::-1] for w in live_rows}
    flat = [score[w, eos] for w in range(W) if fin[w] and time > 0]
    for w in live_rows:
        flat.extend(rows[w].tolist())
    flat = np.sort(np.asarray(flat))[::-1][:W + 1]
    if not np.allclose(flat[:W], _np(out.scores), rtol=0, atol=1e-12):
        raise AssertionError('the numpy restatement disagrees with the reference')
    gaps = [float(np.min(flat[:-1] - flat[1:]))] if len(flat) > 1 else []
    for w in live_rows:
        if C2 > W:
            gaps.append(float(rows[w][W - 1] - rows[w][W]))
    if case['kind'] != 'tie' and gaps and min(gaps) <= G.MARGIN:
        raise MarginError(min(gaps))
    return min(gaps) if gaps else float('inf')


def run_case(name, case, base):
    W, C2, a = case['W'], case['C2'], case['alpha']
    eos = C2 - 1
    if case['kind'] == 'tie':
        time0 = 1
        state = (np.array([-1.5, -1.5, -2.25]), np.zeros(W, dtype=bool), np.array([2, 2, 2]))
    else:
        time0 = 0
        state = (np.zeros(W), np.zeros(W, dtype=bool), np.zeros(W, dtype=np.int64))
    rec = {k: [] for k in ('in_log_probs', 'in_finished', 'in_lengths', 'word', 'parent', 'score', 'out_log_probs',
                           'out_finished', 'out_lengths')}
    min_gap = float('inf')
    seeds = []
    for s in range(case['steps']):
        bs = BeamSearchDecoderState(log_probs=tf.convert_to_tensor(state[0]), finished=tf.convert_to_tensor(state[1]),
                                    lengths=tf.convert_to_tensor(state[2].astype(np.int64)))
        for seed in range(100 * base, 100 * base + 100):       # the step's seed: the first whose margins hold
            x = G.logits(name, case, s, seed)
            out, nxt = beam_search_step(time0 + s, tf.convert_to_tensor(x), bs, W, C2, eos, a, stable_top_k)
            try:
                min_gap = min(min_gap, margins_ok(case, time0 + s, x, state, out))
                break
            except MarginError:
                continue
        else:
            raise MarginError('no seed for step %d' % s)
        seeds.append(seed)
        new = (_np(nxt.log_probs).astype(np.float64), _np(nxt.finished).astype(bool),
               np.rint(_np(nxt.lengths)).astype(np.int64))
        for k, v in (('in_log_probs', state[0]), ('in_finished', state[1]), ('in_lengths', state[2]),
                     ('word', _np(out.predicted_ids)), ('parent', _np(out.beam_parent_ids)), ('score', _np(out.scores)),
                     ('out_log_probs', new[0]), ('out_finished', new[1]), ('out_lengths', new[2])):
            rec[k].append(np.asarray(v))
        state = new
    arr = {k: np.stack(v) for k, v in rec.items()}
    for k in ('word', 'parent', 'in_lengths', 'out_lengths'):
        arr[k] = arr[k].astype(np.int32)
    for k in ('score', 'in_log_probs', 'out_log_probs'):
        if np.abs(arr[k]).max() >= 64:
            raise MarginError('magnitude')
    arr['gathered'] = ref_util.gather_tree_py(arr['word'], arr['parent'])
    fin_at = arr['out_finished'].argmax(0) + 10 * (~arr['out_finished'].any(0))
    if case['kind'] == 'chain':
        if case['all_eos_from'] is not None:
            if not arr['out_finished'][-2].all():
                raise MarginError('not all finished before the end of the chain')
        elif W > 1 and len(set(fin_at.tolist())) < 2:
            raise MarginError('slots do not finish at different steps')
    else:
        sc = arr['score'][0]
        assert sc[0] == sc[1] and arr['parent'][0].tolist()[:2] == [0, 1], arr     # the tie, lower flat index first
    return arr, time0, min_gap, seeds


def main():
    out, meta = {}, {}
    for name, case in G.cases().items():
        for base in range(40):                  # ... and the chain's: the first under which its slots finish as asked
            try:
                arr, time0, gap, seeds = run_case(name, case, base)
                break
            except MarginError:
                continue
        else:
            raise SystemExit('no seed for ' + name)
        meta[name] = dict(case, seeds=seeds, time0=time0, min_gap=gap)
        for k, v in arr.items():
            out['%s|%s' % (name, k)] = v
        print('%-28s seeds %s  min gap %.3g  finished per step %s' % (name, seeds, gap, arr['out_finished'].sum(1).tolist()))
    out['meta_json'] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    np.savez_compressed(G.PATH, **out)
    print('%d arrays, %d cases -> %s (%.1f KB)' % (len(out), len(meta), G.PATH, os.path.getsize(G.PATH) / 1024))


if __name__ == '__main__':
    main()
