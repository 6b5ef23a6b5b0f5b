"""Runs the reference's OWN cnn_zhang encoder and CTC model (models/encoders/core/cnn_zhang.py:41-174,
models/ctc/ctc.py:175-323, cnn_util.py:13-84; unchanged files of the reference checkout) on the eager TensorFlow stand-in
of tests/golden/tf_shim and records what they compute: tests/golden/cnn_zhang_v1.npz.

    python tests/golden/make_golden_cnn_zhang.py --reference <checkout of the reference>

Cases: F in {40, 41} (the pool's two padding geometries), W = splice * num_stack in {11, 22}, B = 2 with ragged lengths
(T = 6 and 4), 61 labels + blank, keep_prob 1, fp64.  Variables are created by the reference's own scopes on a first pass,
then overwritten with _cnn_zhang_golden.values (seeded truncated normals) and the model is evaluated again; the second pass
is recorded: total loss, the per-utterance CTC losses, the logits of the valid frames, and the gradient of every variable
(whole up to 20 000 elements, else its L2 norm and 8 seeded projections)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'tf_shim'))
sys.path.insert(0, os.path.dirname(HERE))
if '--reference' not in sys.argv:
    sys.exit(__doc__)
REF = sys.argv[sys.argv.index('--reference') + 1]
sys.path.insert(0, REF)

import tensorflow as tf                                    # noqa: E402  (the stand-in)

import _cnn_zhang_golden as G                              # noqa: E402
from models.ctc.ctc import CTC                             # noqa: E402

OUT, META = {}, {}
_LOSSES = {}
_ctc_loss = tf.nn.ctc_loss


def _capture_ctc_loss(*a, **k):                            # the per-utterance losses inside CTC.compute_loss
    v = _ctc_loss(*a, **k)
    _LOSSES['v'] = v
    return v


tf.nn.ctc_loss = _capture_ctc_loss


def put(case, group, name, value):
    OUT['%s|%s|%s' % (case, group, name)] = np.asarray(value)


def sparse(rows):
    idx = [[b, j] for b, r in enumerate(rows) for j in range(len(r))]
    val = [v for r in rows for v in r]
    L = max(len(r) for r in rows)
    T = tf.convert_to_tensor
    return tf.SparseTensor(T(np.asarray(idx, dtype=np.int64).reshape(-1, 2)), T(np.asarray(val, dtype=np.int64)),
                           T(np.asarray([len(rows), L], dtype=np.int64)))


def main():
    for k, (F, num_stack) in enumerate([(40, 1), (41, 1), (40, 2), (41, 2)]):
        splice, C = 11, 61
        W = splice * num_stack
        case = 'cnn_zhang_F%d_W%d' % (F, W)
        rng = np.random.RandomState(7000 + k)
        B, Tn = 2, 6
        lens = np.array([6, 4])
        x = rng.randn(B, Tn, 3 * F * W) * (np.arange(Tn)[None, :, None] < lens[:, None, None])
        x = x.astype(np.float32).astype(np.float64)         # the recorded inputs are exactly what was run
        rows = [rng.randint(0, C, size=3).tolist(), rng.randint(0, C, size=2).tolist()]
        kw = dict(encoder_type='cnn_zhang', input_size=3 * F, splice=splice, num_stack=num_stack, num_units=256,
                  num_layers=10, num_classes=C, parameter_init=0.1, num_proj=0)

        def run():
            model = CTC(**kw)
            total, logits = model.compute_loss(tf.convert_to_tensor(x), sparse(rows), tf.convert_to_tensor(lens), 1.0)
            return model, total, logits

        tf.shim_reset(seed=300 + k)
        run()
        names = []
        for name, v in tf.shim_variables().items():
            shape = [int(d) for d in v._t.shape]
            tf.shim_set_variable(name, G.values(case, name, shape))
            names.append([name, shape])
        tf.shim_reset(keep_variables=True)
        model, total, logits = run()
        tf.shim_zero_grads()
        total._t.backward()
        for name, v in tf.shim_variables().items():
            g = v._t.grad.numpy()
            if g.size <= G.BIG:
                put(case, 'grad', name, g)
            else:
                put(case, 'gnorm', name, np.linalg.norm(g.astype(np.float64)))
                put(case, 'gproj', name, G.projections(name, g))
        lg = logits.numpy()                                   # [T, B, C + 1]
        put(case, 'in', 'inputs', x.astype(np.float32))
        put(case, 'in', 'inputs_seq_len', lens)
        put(case, 'in', 'labels_flat', np.asarray([v for r in rows for v in r], dtype=np.int64))
        put(case, 'in', 'labels_len', np.asarray([len(r) for r in rows], dtype=np.int64))
        put(case, 'out', 'total_loss', total.numpy())
        put(case, 'out', 'ctc_losses', _LOSSES['v'].numpy())
        put(case, 'out', 'logits_valid', np.concatenate([lg[:lens[b], b] for b in range(B)], 0))
        META[case] = dict(F=F, W=W, splice=splice, num_stack=num_stack, num_classes=C, vars=names)
        print(case, float(total.numpy()), len(names), 'variables')
    OUT['meta_json'] = np.frombuffer(json.dumps(META, sort_keys=True).encode(), dtype=np.uint8)
    np.savez_compressed(G.PATH, **OUT)
    print('%d arrays -> %s (%.1f KB)' % (len(OUT), G.PATH, os.path.getsize(G.PATH) / 1024))


if __name__ == '__main__':
    main()
