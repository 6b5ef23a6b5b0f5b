"""Batch normalization layer -- mirror of models/encoders/core/cnn_util.py:87-149 (batch_normalization with its defaults:
epsilon 1e-3, momentum 0.9, fused_batch_norm False) over NHWC activations, on the asr_bn_* kernels.

Variables, in creation order under `<scope>/batch_norm/`: beta (zeros) and gamma (ones), trainable -- they live in the
model's ParamStore and are decayed and clipped like any other variable whose name lacks 'bias' -- then avg_mean (zeros)
and avg_variance (ones), trainable=False: they live in a StateStore beside the flat buffer, so the optimizer, the clip and
the weight decay never see them.

is_training=True normalizes with the batch statistics (tf.nn.moments over N, H, W; biased variance) and leaves the
moving-average update pending; `commit()` applies it (avg <- 0.9 avg + 0.1 stat, the UPDATE_OPS the train op depends on,
model_base.py:120,129) on the device, once per training step.  is_training=False normalizes with the moving averages.
"""
from .... import ops

EPSILON = 1e-3
MOMENTUM = 0.9


class BatchNorm(object):

    def __init__(self, scope, channels):
        self.scope = scope + '/batch_norm'
        self.channels = channels
        self.names = [self.scope + '/' + n for n in ('beta', 'gamma', 'avg_mean', 'avg_variance')]
        self.pending = None
        self.ctx = None

    def declare(self, store, state, np_ones, np_zeros):
        c = self.channels
        store.declare(self.names[0], (c,), np_zeros(c))
        store.declare(self.names[1], (c,), np_ones(c))
        state.declare(self.names[2], (c,), np_zeros(c))
        state.declare(self.names[3], (c,), np_ones(c))
        self.store, self.state = store, state

    def forward(self, x, is_training, pool, out_dtype):
        """x fp32 [N,H,W,C] (a ReLU output) -> (the next layer's operand [N, Ho, W, C] in out_dtype, argmax of the pool)."""
        st, sv = self.store, self.state
        beta, gamma = st[self.names[0]], st[self.names[1]]
        avg_m, avg_v = sv[self.names[2]], sv[self.names[3]]
        if is_training:
            stats = ops.bn_stats(x, EPSILON, MOMENTUM, avg_m, avg_v)
            out, arg = ops.bn_apply(x, stats[0], stats[1], gamma, beta, EPSILON, pool, out_dtype)
            self.pending = stats
        else:
            stats = None
            out, arg = ops.bn_apply(x, avg_m, avg_v, gamma, beta, EPSILON, pool, out_dtype)
        self.ctx = dict(x=x, stats=stats, arg=arg)
        return out, arg

    def backward(self, dz, out_dtype):
        """dz fp32 = gradient at the (pooled) output -> gradient at the convolution's pre-activation (ReLU gate fused), in
        out_dtype; dgamma and dbeta go into the flat gradient buffer."""
        c = self.ctx
        if c is None or c['stats'] is None:
            raise RuntimeError('%s: backward needs a preceding forward with is_training=True' % self.scope)
        st = self.store
        dx = ops.bn_bwd(dz.contiguous(), c['arg'], c['x'], c['stats'], st[self.names[1]], st.g(self.names[1]),
                        st.g(self.names[0]), out_dtype)
        self.ctx = None
        return dx

    def commit(self):
        """Apply the pending moving-average update of the last training forward (device copies, no host sync)."""
        if self.pending is None:
            return
        sv = self.state
        sv[self.names[2]].copy_(self.pending[3])
        sv[self.names[3]].copy_(self.pending[4])
        self.pending = None
