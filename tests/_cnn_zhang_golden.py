"""Loader and weight recipe of tests/golden/cnn_zhang_v1.npz: what the REFERENCE'S OWN cnn_zhang.py + ctc.py computed on the
eager TensorFlow stand-in (generator: tests/golden/make_golden_cnn_zhang.py, which needs the reference checkout; the
fixture travels).

The 66 M parameters are not stored: every variable is drawn by `values(case, name, shape)` (a truncated normal from its own
seed, stddev sqrt(2 / fan-in) for weights, 0.05 for biases).  Gradients of up to BIG elements are stored whole; larger ones
as their L2 norm and NPROJ projections on seeded standard-normal vectors (`projections`)."""
import json
import os
import zlib

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'cnn_zhang_v1.npz')
BIG = 20000
NPROJ = 8
_cache = {}


def seed_of(case, name):
    return zlib.crc32((case + '|' + name).encode()) & 0x7fffffff


def values(case, name, shape):
    shape = tuple(int(s) for s in shape)
    rng = np.random.RandomState(seed_of(case, name))
    std = 0.05 if len(shape) == 1 else float(np.sqrt(2.0 / np.prod(shape[:-1])))
    x = rng.normal(0.0, std, size=shape)
    bad = np.abs(x) > 2 * std
    while bad.any():
        x[bad] = rng.normal(0.0, std, size=int(bad.sum()))
        bad = np.abs(x) > 2 * std
    return x


def projections(name, g):
    """[NPROJ] float64: <g, r_k> with r_k standard normal (float32) from default_rng(crc32(name)), k = 0 .. NPROJ - 1."""
    g = np.asarray(g, dtype=np.float32).reshape(-1)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    return np.array([float(np.dot(rng.standard_normal(g.size, dtype=np.float32).astype(np.float64), g.astype(np.float64)))
                     for _ in range(NPROJ)])


def load():
    if 'z' not in _cache:
        with np.load(PATH) as f:
            _cache['z'] = {k: f[k] for k in f.files}
        _cache['meta'] = json.loads(bytes(_cache['z']['meta_json']).decode())
    return _cache['z'], _cache['meta']


def cases():
    return sorted(load()[1])


def gradient_error(z, case, name, g):
    """Relative L2 error of gradient g against the fixture: whole, or (for large ones) the worst of |norm| and the
    projections, each relative to the reference norm."""
    g = np.asarray(g, dtype=np.float64)
    key = '%s|grad|%s' % (case, name)
    if key in z:
        r = z[key].astype(np.float64)
        return float(np.linalg.norm(g - r) / max(np.linalg.norm(r), 1e-300))
    nr = float(z['%s|gnorm|%s' % (case, name)])
    pr = z['%s|gproj|%s' % (case, name)]
    pg = projections(name, g)
    return max(abs(float(np.linalg.norm(g)) - nr), float(np.abs(pg - pr).max())) / max(nr, 1e-300)
