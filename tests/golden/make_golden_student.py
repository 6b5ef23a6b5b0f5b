"""Runs the reference's OWN StudentCTC and its four student encoders (models/ctc/student_ctc.py,
models/encoders/core/student_cnn_{,compact_}{ctc,xe}.py, cnn_util.py:13-149; unchanged files of the reference checkout)
on the eager TensorFlow stand-in of tests/golden/tf_shim and records what they compute: tests/golden/student_v1.npz.

    python tests/golden/make_golden_student.py --reference <checkout of the reference>

The stand-in lacks tf.nn.moments, tf.nn.batch_normalization, tf.assign and tf.nn.softmax_cross_entropy_with_logits;
they are attached here, TF 1.x-faithful (moments: reduce_mean, then the mean of squared_difference against
stop_gradient(mean); batch_normalization: inv = rsqrt(var + eps) * scale, x * inv + (offset - mean * inv); assign:
eager in-place update; softmax_cross_entropy_with_logits: -sum(labels * log_softmax(logits)) with TF's gradient
softmax(logits) - labels).

Cases (fp64, keep_prob 1, F = 40, splice 5, num_stack 2 -> W = 10):
  ctc_<enc>_T5 / _T7   student_cnn and student_cnn_compact, B = 2, lengths (5, 3), 30 labels + blank, the same
                       utterances padded with zero frames to T = 5 and T = 7 (batch statistics include the padding)
  ctc_wd               student_cnn_compact, T = 5, weight_decay 1e-3
  ctc_eval             student_cnn_compact, T = 5, is_training=False (the seeded moving averages normalize)
  xe_<enc>             student_cnn_xe and student_cnn_compact_xe, 6 frames, 30 + 1 classes, soft targets that sum to 1
Recorded: total loss, per-utterance CTC losses (or per-frame XE losses), the logits (valid frames on the CTC path), every
gradient (whole up to 10 000 elements, else norm + 8 projections), the moving averages after the eager assigns of the
step, and the variable metadata (name, shape, trainable, creation order)."""
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

import torch                                               # noqa: E402
import tensorflow as tf                                    # noqa: E402  (the stand-in)

import _student_golden as G                                # noqa: E402


def _t(x):
    return x._t if isinstance(x, tf.Tensor) else torch.as_tensor(np.asarray(x), dtype=torch.float64)


def moments(x, axes, shift=None, name=None, keep_dims=False):
    y = _t(x)
    mean = y.mean(dim=tuple(axes), keepdim=True)
    var = ((y - mean.detach()) ** 2).mean(dim=tuple(axes), keepdim=True)
    if not keep_dims:
        mean, var = mean.reshape(-1), var.reshape(-1)
    return tf.Tensor(mean), tf.Tensor(var)


def batch_normalization(x, mean, variance, offset, scale, variance_epsilon, name=None):
    inv = torch.rsqrt(_t(variance) + variance_epsilon)
    if scale is not None:
        inv = inv * _t(scale)
    off = (_t(offset) - _t(mean) * inv) if offset is not None else -_t(mean) * inv
    return tf.Tensor(_t(x) * inv + off)


def assign(ref, value, name=None, **kw):
    return ref.assign(value)


class _SoftXent(torch.autograd.Function):
    @staticmethod
    def forward(ctx, labels, logits):
        ls = torch.log_softmax(logits, dim=-1)
        ctx.save_for_backward(labels, ls)
        return -(labels * ls).sum(-1)

    @staticmethod
    def backward(ctx, g):
        labels, ls = ctx.saved_tensors
        return None, g.unsqueeze(-1) * (ls.exp() - labels)          # TF's kernel: softmax - labels


def softmax_cross_entropy_with_logits(_sentinel=None, labels=None, logits=None, dim=-1, name=None):
    return tf.Tensor(_SoftXent.apply(_t(labels).detach(), _t(logits)))


tf.nn.moments = moments
tf.nn.batch_normalization = batch_normalization
tf.nn.softmax_cross_entropy_with_logits = softmax_cross_entropy_with_logits
tf.assign = assign

from models.ctc.student_ctc import StudentCTC              # noqa: E402

OUT, META = {}, {}
_LOSSES = {}
_ctc_loss = tf.nn.ctc_loss
_xent = tf.nn.softmax_cross_entropy_with_logits


def _capture_ctc_loss(*a, **k):
    v = _ctc_loss(*a, **k)
    _LOSSES['v'] = v
    return v


def _capture_xent(*a, **k):
    v = _xent(*a, **k)
    _LOSSES['v'] = v
    return v


tf.nn.ctc_loss = _capture_ctc_loss
tf.nn.softmax_cross_entropy_with_logits = _capture_xent

F, SPLICE, NUM_STACK, C = 40, 5, 2, 30
W = SPLICE * NUM_STACK


def put(case, group, name, value):
    OUT['%s|%s|%s' % (case, group, name)] = np.asarray(value)


def sparse(rows):
    idx = [[b, j] for b, r in enumerate(rows) for j in range(len(r))]
    val = [v for r in rows for v in r]
    L = max(len(r) for r in rows)
    T = tf.convert_to_tensor
    return tf.SparseTensor(T(np.asarray(idx, dtype=np.int64).reshape(-1, 2)), T(np.asarray(val, dtype=np.int64)),
                           T(np.asarray([len(rows), L], dtype=np.int64)))


def record(case, vkey, seed, kw, run, inputs, is_training, extra):
    tf.shim_reset(seed=seed)
    run(StudentCTC(**kw), True)
    names = []
    for name, v in tf.shim_variables().items():
        shape = [int(d) for d in v._t.shape]
        tf.shim_set_variable(name, G.values(vkey, name, shape))
        names.append([name, shape, bool(v.trainable)])
    tf.shim_reset(keep_variables=True)
    total, logits = run(StudentCTC(**kw), is_training)
    if is_training:
        tf.shim_zero_grads()
        total._t.backward()
        for name, v in tf.shim_variables().items():
            if not v.trainable:
                continue
            g = v._t.grad.numpy()
            if g.size <= G.BIG:
                put(case, 'grad', name, g)
            else:
                put(case, 'gnorm', name, np.linalg.norm(g.astype(np.float64)))
                put(case, 'gproj', name, G.projections(name, g))
    for name, v in tf.shim_variables().items():
        if not v.trainable:
            put(case, 'avg_after', name, v._t.detach().numpy())
    for k, val in inputs.items():
        put(case, 'in', k, val)
    put(case, 'out', 'total_loss', total.numpy())
    put(case, 'out', 'losses', _LOSSES['v'].numpy())
    put(case, 'out', 'logits', extra(logits.numpy()))
    META[case] = dict(F=F, W=W, splice=SPLICE, num_stack=NUM_STACK, num_classes=C, vars=names,
                      encoder_type=kw['encoder_type'], weight_decay=kw.get('weight_decay', 0.0),
                      is_training=bool(is_training), input_size=kw['input_size'], vkey=vkey)
    print(case, float(total.numpy()), len(names), 'variables')


def ctc_case(case, enc, T, seed, weight_decay=0.0, is_training=True):
    rng = np.random.RandomState(8000)                      # the same utterances for every padding
    B, lens = 2, np.array([5, 3])
    x5 = rng.randn(B, 5, 3 * F * W) * (np.arange(5)[None, :, None] < lens[:, None, None])
    x = np.zeros((B, T, 3 * F * W))
    x[:, :5] = x5
    x = x.astype(np.float32).astype(np.float64)
    rows = [rng.randint(0, C, size=2).tolist(), rng.randint(0, C, size=1).tolist()]
    kw = dict(encoder_type=enc, input_size=3 * F * NUM_STACK, num_classes=C, splice=SPLICE, num_stack=NUM_STACK,
              parameter_init=0.1, weight_decay=weight_decay)

    def run(model, training):
        return model.compute_ctc_loss(tf.convert_to_tensor(x), sparse(rows), tf.convert_to_tensor(lens), 1.0,
                                      is_training=training)

    inputs = dict(inputs=x.astype(np.float32), inputs_seq_len=lens,
                  labels_flat=np.asarray([v for r in rows for v in r], dtype=np.int64),
                  labels_len=np.asarray([len(r) for r in rows], dtype=np.int64))
    record(case, 'ctc_%s' % enc if weight_decay == 0 and is_training else case, seed, kw, run, inputs, is_training,
           lambda lg: np.concatenate([lg[:lens[b], b] for b in range(B)], 0))


def xe_case(case, enc, seed):
    rng = np.random.RandomState(8100)
    B = 6
    x = rng.randn(B, 3 * F * W).astype(np.float32).astype(np.float64)
    p = rng.gamma(0.3, size=(B, C + 1))
    p = p / p.sum(1, keepdims=True)
    kw = dict(encoder_type=enc, input_size=3 * F * W, num_classes=C, splice=SPLICE, num_stack=NUM_STACK,
              parameter_init=0.1)

    def run(model, training):
        return model.compute_xe_loss(tf.convert_to_tensor(x), tf.convert_to_tensor(p), 1.0, is_training=training)

    record(case, case, seed, kw, run, dict(inputs=x.astype(np.float32), soft_targets=p), True, lambda lg: lg)


def main():
    for k, enc in enumerate(['student_cnn', 'student_cnn_compact']):
        for T in (5, 7):
            ctc_case('ctc_%s_T%d' % (enc, T), enc, T, 400 + k)
    ctc_case('ctc_wd', 'student_cnn_compact', 5, 410, weight_decay=1e-3)
    ctc_case('ctc_eval', 'student_cnn_compact', 5, 411, is_training=False)
    for k, enc in enumerate(['student_cnn_xe', 'student_cnn_compact_xe']):
        xe_case('xe_%s' % enc, enc, 420 + k)
    OUT['meta_json'] = np.frombuffer(json.dumps(META, sort_keys=True).encode(), dtype=np.uint8)
    np.savez_compressed(G.PATH, **OUT)
    print('%d arrays -> %s (%.1f KB)' % (len(OUT), G.PATH, os.path.getsize(G.PATH) / 1024))


if __name__ == '__main__':
    main()
