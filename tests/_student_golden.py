"""Loader and variable recipe of tests/golden/student_v1.npz: what the REFERENCE'S OWN student_ctc.py and the four student
encoders computed on the eager TensorFlow stand-in (generator: tests/golden/make_golden_student.py, which needs the
reference checkout; the fixture travels).

Variables are not stored: `values(case, name, shape)` draws each from its own seed (the cnn_zhang recipe: truncated
normal, stddev sqrt(2 / fan-in) for weights, 0.05 for biases and beta); gamma is 1 + that, the moving averages are
seeded non-trivial values (avg_mean 0.5 * that, avg_variance 1 + |that| * 10).  Gradients of up to BIG elements are stored
whole, larger ones as their L2 norm and NPROJ seeded projections."""
import json
import os

import numpy as np

import _cnn_zhang_golden as _Z

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'student_v1.npz')
BIG = 10000
NPROJ = _Z.NPROJ
projections = _Z.projections
_cache = {}


def values(case, name, shape):
    base = _Z.values(case, name, shape)
    leaf = name.rsplit('/', 1)[-1]
    if leaf == 'gamma':
        return 1.0 + base
    if leaf == 'avg_mean':
        return 0.5 * base
    if leaf == 'avg_variance':
        return 1.0 + 10.0 * np.abs(base)
    return base


def load():
    if 'z' not in _cache:
        with np.load(PATH) as f:
            _cache['z'] = {k: f[k] for k in f.files}
        _cache['meta'] = json.loads(bytes(_cache['z']['meta_json']).decode())
    return _cache['z'], _cache['meta']


def gradient_error(z, case, name, g):
    """Relative L2 error of gradient g against the fixture (whole, or the worst of |norm| and the projections)."""
    g = np.asarray(g, dtype=np.float64)
    key = '%s|grad|%s' % (case, name)
    if key in z:
        r = z[key].astype(np.float64)
        return float(np.linalg.norm(g - r) / max(np.linalg.norm(r), 1e-300))
    nr = float(z['%s|gnorm|%s' % (case, name)])
    pr = z['%s|gproj|%s' % (case, name)]
    pg = projections(name, g)
    return max(abs(float(np.linalg.norm(g)) - nr), float(np.abs(pg - pr).max())) / max(nr, 1e-300)
