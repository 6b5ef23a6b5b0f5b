"""The attention beam search fixture (tests/golden/att_beam_v1.npz, written by tests/golden/make_golden_att_beam.py from
the reference's own beam_search_step / mask_probs / normalize_score / gather_tree_py) and the recipe of its logits, which
the generator and the tests share: the logits of the widest case alone would be 3 MB, so the fixture holds what the
reference computed from them and the recipe below is the input."""
import json
import os
import zlib

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'att_beam_v1.npz')

SHAPES = [(1, 9), (2, 3), (4, 11), (5, 40), (20, 3388)]          # (W, C2); <EOS> is class C2 - 1
ALPHAS = [0.0, 0.6, 1.0]
MARGIN = 1e-3


def cases():
    """name -> dict(W, C2, alpha, steps, eos_rate, all_eos_from, kind).  One chain per (shape, alpha); the chain's length
    (6 .. 10) and how eagerly <EOS> turns up vary with its index; the alpha = 0.6 chains end with every slot finished
    (<EOS> dominates every row from step `all_eos_from` on)."""
    out = {}
    for i, (W, C2) in enumerate(SHAPES):
        for j, a in enumerate(ALPHAS):
            n = 3 * i + j
            out['chain_W%d_C%d_a%g' % (W, C2, a)] = dict(W=W, C2=C2, alpha=a, steps=6 + n % 5, eos_rate=0.15 + 0.1 * (n % 3),
                                                         all_eos_from=3 if a == 0.6 else None, kind='chain')
    out['tie_W3_C7'] = dict(W=3, C2=7, alpha=0.6, steps=1, eos_rate=0.0, all_eos_from=None, kind='tie')
    return out


def logits(name, case, step, seed):
    """[W, C2] float64 array of float32 values in [-4, 4].  Bulk classes are uniform in [-4, 1]; per row min(C2, W + 2)
    head classes lie in (1, 4], spaced 0.02 .. 0.12 apart, so that the selection margins the generator asserts are
    reachable at C2 = 3388 (uniform draws alone would put neighbours of the top W closer than 1e-3).  <EOS> joins the
    head with probability eos_rate; from step all_eos_from on it is 4 and everything else sits 4 lower."""
    W, C2 = case['W'], case['C2']
    rng = np.random.RandomState((zlib.crc32(name.encode()) + 7919 * step + 104729 * seed) & 0x7fffffff)
    all_eos = case['all_eos_from'] is not None and step >= case['all_eos_from']
    top = 0.0 if all_eos else 4.0
    x = rng.uniform(-4.0, top - 3.0, size=(W, C2))
    eos = C2 - 1
    nh = min(C2, W + 2)
    for w in range(W):
        vals = top - rng.uniform(0.0, 0.3) - np.cumsum(rng.uniform(0.02, 0.12, size=nh))
        cls = rng.choice(C2 - 1, size=min(nh, C2 - 1), replace=False)
        x[w, cls] = rng.permutation(vals)[:len(cls)]
        if all_eos:
            x[w, eos] = 4.0
        else:
            x[w, eos] = vals[rng.randint(nh)] + 0.007 if rng.rand() < case['eos_rate'] else rng.uniform(-4.0, 1.0)
    if case['kind'] == 'tie':
        x[1] = x[0]
    return x.astype(np.float32).astype(np.float64)


_cache = {}


def load():
    """(meta, arrays): meta[name] = the case dict + 'seeds' (one per step) + 'time0'; arrays['<name>|<field>'] as recorded."""
    if 'z' not in _cache:
        z = np.load(PATH)
        _cache['z'] = ({k: z[k] for k in z.files if k != 'meta_json'}, json.loads(bytes(z['meta_json']).decode()))
    arrays, meta = _cache['z']
    return meta, arrays
