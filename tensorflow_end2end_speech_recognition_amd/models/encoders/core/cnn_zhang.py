"""CNN encoder -- mirror of models/encoders/core/cnn_zhang.py:41-174 (class CNNEncoder, after Zhang et al. 2017,
arXiv:1701.02720).

__call__(inputs [B,T,num_channels*(splice*num_stack)*3], inputs_seq_len, keep_prob, is_training):
reshape to [B*T, F = input_size // 3, W = splice*num_stack, 3] (:105-107); CNN1 conv 3x5 SAME 3->128 + relu, max_pool
[3,1] / [3,1] SAME (Ho = ceil(F/3)), dropout; CNN2-4 128->128, CNN5 128->256, CNN6-10 256->256, each conv 3x5 SAME +
relu + dropout (:117-146); flatten NHWC to [B*T, Ho*W*256] (:149-150); fc1, fc2, fc3 -> 1024 relu, dropout after fc1 and
fc2 (:153-164) -> outputs [T,B,1024] (time_major) and final_state None.  Variables, in creation order:
CNN{1..10}/conv/{weight,bias} (tf.Variable(truncated_normal(stddev=parameter_init)) and zeros, cnn_util.py:66-69),
fc{1,2,3}/{weights,biases}.

Execution.  Only the valid frames are convolved (every frame is an independent image, as in vgg_blstm.py): the rows of
`outputs` at padded positions are zeros, where the reference carries the network's response to the padding.  CTC loss,
gradients and decoders stop at seq_len, so nothing downstream sees the difference.
  bf16 models: CNN2-10 are implicit GEMMs (asr_conv3x5_*: no patch matrix) with ReLU + dropout in the forward epilogue
  and the ReLU / dropout backward of the layer below in the data gradient's epilogue; the 3-channel CNN1 (0.3 % of the
  FLOPs) is asr_im2col + GEMM with fused bias + ReLU, its pool + dropout one asr_maxpool3x1_fwd pass.
  fp32 models (the parity path), and any layer outside the implicit kernels' limits: asr_im2col + GEMM chunked over
  frames, backward through asr_col2im.  `conv_path` records which path each layer took in the last forward.
"""
import os

import numpy as np
import torch

from .... import ops
from ...._lib import ASR_BF16, ASR_F32
from ....utils.parameter import ParamStore
from . import cnn_util

CONVS = ([('CNN1/conv', 3, 128)] + [('CNN%d/conv' % i, 128, 128) for i in (2, 3, 4)] + [('CNN5/conv', 128, 256)] +
         [('CNN%d/conv' % i, 256, 256) for i in (6, 7, 8, 9, 10)])
FCS = ['fc1', 'fc2', 'fc3']
FC_UNITS = 1024
KH, KW = 3, 5


class CNNEncoder(object):
    """models/encoders/core/cnn_zhang.py:41 CNNEncoder."""

    def __init__(self, input_size, splice, num_stack, parameter_init, time_major, name='cnn_zhang_encoder',
                 dtype=ASR_F32, seed=0):
        assert input_size % 3 == 0
        self.num_channels = input_size // 3
        self.splice = splice
        self.num_stack = num_stack
        self.parameter_init = parameter_init
        self.time_major = time_major
        self.name = name
        self.dtype = ops.dtype_id(dtype)
        self.seed = seed
        self.F = self.num_channels
        self.W = splice * num_stack
        self.Hp = (self.F + 2) // 3                      # rows after the [3,1] / [3,1] SAME pool
        self.flat = self.Hp * self.W * CONVS[-1][2]
        self.output_dim = FC_UNITS
        self.layers = None
        self.store = None
        self.want_f32_outputs = True
        # A/B switch (probe, tests): False runs every layer as asr_im2col + GEMM
        self.implicit = os.environ.get('ASR_CNN_ZHANG_IMPLICIT', '1') != '0'
        self.conv_path = {}
        self.ctx = None

    # ------------------------------------------------------------------ variables
    def build(self, store, input_dim, rng, scope_prefix=''):
        assert input_dim == self.F * self.W * 3, 'input_dim %d != num_channels * splice * num_stack * 3' % input_dim
        p = scope_prefix
        for name, cin, cout in CONVS:
            cnn_util.declare_conv(store, p + name, KH, KW, cin, cout, rng, self.parameter_init)
        din = self.flat
        for name in FCS:
            cnn_util.declare_fc(store, p + name, din, FC_UNITS, rng, self.parameter_init)
            din = FC_UNITS
        self.store, self._p = store, p
        self.layers = [n for n, _, _ in CONVS] + FCS
        return FC_UNITS

    def _implicit_ok(self, cin, cout, npix):
        return (self.implicit and self.dtype == ASR_BF16 and cin % 64 == 0 and cout % 64 == 0 and
                npix < (1 << 31) - 128)

    # ------------------------------------------------------------------ valid-frame index
    def _index(self, lens, T, Bp, dev):
        """(valid frames in b*T + t order, their rows t*Bp + b of the time-major padded output, the inverse: for each of
        the T*Bp output rows the valid-frame index or N = the appended zero row), cached per batch geometry."""
        key = (lens.tobytes(), int(T), int(Bp), str(dev))
        cache = self.__dict__.setdefault('_index_cache', {})
        hit = cache.get(key)
        if hit is None:
            B = len(lens)
            b, t = np.nonzero(np.arange(T)[None, :] < lens[:, None])           # row-major: b * T + t order
            valid = (b * T + t).astype(np.int32)
            rows_tm = (t * Bp + b).astype(np.int32)
            inv = np.full(T * Bp, len(valid), dtype=np.int32)
            inv[rows_tm] = np.arange(len(valid), dtype=np.int32)
            if len(cache) >= 16:
                cache.clear()
            hit = cache[key] = tuple(ops.to_device(a, torch.int32, dev) for a in (valid, rows_tm, inv)) + (len(valid),)
        return hit

    # ------------------------------------------------------------------ one layer's views
    def _w2d(self, li):
        """the [15*Cin, Cout] view of layer li's weight in the operand dtype"""
        name, cin, cout = CONVS[li]
        return self.store.shadow(self.dtype)[self._p + name + '/weight'].view(KH * KW * cin, cout)

    def _g2d(self, li):
        """(the [15*Cin, Cout] view of layer li's weight gradient, its bias gradient)"""
        name, cin, cout = CONVS[li]
        return self.store.g(self._p + name + '/weight').view(KH * KW * cin, cout), self.store.g(self._p + name + '/bias')

    def _images(self, name):
        cache = self.ctx.setdefault('wimg', {})
        if name not in cache:
            cache[name] = ops.conv3x5_prep_weights(self.store[self._p + name + '/weight'])
        return cache[name]

    # ------------------------------------------------------------------ forward
    def __call__(self, inputs, inputs_seq_len, keep_prob, is_training, drop_masks=None, rng_state=None):
        """inputs [B,T,F*W*3] fp32 (cuda).  Returns (outputs [T,B,1024] if time_major else [B,T,1024], None)."""
        if self.layers is None:
            store = ParamStore(inputs.device)
            self.build(store, inputs.shape[-1], np.random.RandomState(self.seed))
            store.finalize()
        st, p = self.store, self._p
        sh = st.shadow(self.dtype)
        B, T, D = inputs.shape
        assert D == self.F * self.W * 3
        dev = inputs.device
        lens_host = getattr(self, '_lens_host', None)
        self._lens_host = None
        if lens_host is None or len(lens_host) != B:
            lens_host = ops.host_ints(inputs_seq_len)
        lens = np.minimum(np.maximum(np.asarray(lens_host, dtype=np.int64), 0), T)
        Bp = B + (-B) % 16                                 # the heads and the CTC kernels tile 16 utterances
        valid, rows_tm, inv, N = self._index(lens, T, Bp, dev)
        seq = ops.to_device(np.concatenate([lens, np.zeros(Bp - B, np.int64)]).astype(np.int32), torch.int32, dev)
        keep = float(keep_prob) if keep_prob is not None else 1.0
        drop = is_training and keep < 1.0
        if drop and rng_state is None:                     # used on its own: fresh masks every training call
            self._dropout_calls = getattr(self, '_dropout_calls', 0) + 1
            rng_state = (self.seed, self._dropout_calls << 40)
        descs = {}

        def desc(i):
            if not drop:
                return None
            d = (keep, rng_state[0] + 7, rng_state[1] + (i << 32))
            descs[i] = d
            return d

        self.batch = B
        self.seq_len_padded = seq
        F, W = self.F, self.W
        bf = self.dtype == ASR_BF16
        tdt = torch.bfloat16 if bf else torch.float32
        table = torch.empty((N + 1, FC_UNITS), dtype=tdt, device=dev)
        table[N:].zero_()
        self.ctx = dict(N=N, B=B, T=T, Bp=Bp, rows_tm=rows_tm, drop=drop, descs=descs)
        if N > 0:
            x = ops.embedding_gather(inputs.contiguous().view(B * T, D), valid).view(N, F, W, 3)
            x0 = ops.cast_from_f32(x, self.dtype) if bf else x
            # CNN1: im2col + GEMM (3 input channels), then pool + dropout in one pass
            a1 = cnn_util.conv_im2col(x0, KH, KW, self._w2d(0), st[p + CONVS[0][0] + '/bias'], x0.dtype)
            p1, arg1 = ops.maxpool3x1_fwd(a1, drop=desc(1))
            path = {CONVS[0][0]: 'im2col'}
            fused = bf and all(self._implicit_ok(c[1], c[2], N * self.Hp * W) for c in CONVS[1:])
            acts = [p1]           # inputs of CNN2..10 as the layers consumed them (dropped)
            relu_outs = [None]    # undropped ReLU outputs (im2col path only; the fused path keeps the dropped ones)
            for li in range(1, len(CONVS)):
                name, cin, cout = CONVS[li]
                x_in = acts[-1]
                d = desc(li + 1)
                if fused:
                    wf = self._images(name)[0]
                    b = st[p + name + '/bias']
                    y = ops.conv3x5_fwd_drop(x_in, wf, b, d) if d is not None else ops.conv3x5_fwd(x_in, wf, b, relu=True)
                    relu_outs.append(None)
                    acts.append(y)
                    path[name] = 'implicit'
                else:
                    y = cnn_util.conv_im2col(x_in, KH, KW, self._w2d(li), st[p + name + '/bias'], x_in.dtype)
                    relu_outs.append(y)
                    acts.append(ops.dropout_apply(y, *d) if d is not None else y)
                    path[name] = 'im2col'
            self.conv_path = path
            # dropout after fc1 and fc2 (:153-164); fc3 writes the row table
            drops = [desc(len(CONVS) + 1 + k) for k in range(len(FCS) - 1)] + [None]
            _, fc = cnn_util.fc_forward(st, sh, [p + n for n in FCS], acts[-1].view(N, self.flat), drops, out=table[:N])
            self.ctx.update(x0=x0, a1=a1, arg1=arg1, acts=acts, relu_outs=relu_outs, fused=fused, fc=fc)
        # back to the time-major padded grid: padded rows read the zero row
        out_tm = cnn_util.gather_time_major(table, inv).view(T, Bp, FC_UNITS)
        self._out_op = out_tm
        want = self.want_f32_outputs
        out = ops.cast_to_f32(out_tm) if (bf and want) else out_tm
        self._out_tm = out
        out_user = out[:, :B]
        if not self.time_major:
            out_user = out_user.transpose(0, 1)
        return out_user, None

    # ------------------------------------------------------------------ backward
    def backward(self, d_outputs, d_final=None, need_input_grad=False, d_outputs_sub=None):
        """d_outputs [T,Bp,1024] fp32 (time-major, padded batch): the gradients of every variable."""
        c, st, p = self.ctx, self.store, self._p
        dev = d_outputs.device
        if c is None:
            raise RuntimeError('CNNEncoder.backward needs a preceding forward')
        N = c['N']
        if N == 0:
            st.grad.zero_()
            ops.join_side(dev)
            self.ctx = None
            return None
        sh = st.shadow(self.dtype)
        d = ops.embedding_gather(d_outputs.reshape(-1, FC_UNITS).contiguous(), c['rows_tm'])      # [N,1024] fp32
        d = cnn_util.fc_backward(st, sh, [p + n for n in FCS], c['fc'], d)
        acts, relu_outs, descs = c['acts'], c['relu_outs'], c['descs']
        Hp, W = self.Hp, self.W
        last = len(CONVS) - 1
        d = d.view(N, Hp, W, CONVS[-1][2])
        # the pre-activation gradient of CNN10
        if c['fused']:
            dr = descs.get(last + 1)
            dpre = ops.relu_bwd_scaled(d, acts[-1], dr[0]) if dr is not None else ops.relu_bwd(d, acts[-1])
        else:
            dpre = ops.relu_bwd(d, relu_outs[-1], drop=descs.get(last + 1))
        for li in range(last, 0, -1):
            name, cin, cout = CONVS[li]
            x_in = acts[li - 1]
            below_drop = descs.get(li)       # dropout of the tensor layer li consumed (pooled output for li == 1)
            if c['fused']:
                ops.conv3x5_bwd_weight_bias(x_in, dpre, *self._g2d(li))
                # ReLU / dropout backward of the tensor below, in the epilogue: its stored form is the dropped one (> 0
                # where active and kept); for CNN2 that is the pooled CNN1 output, > 0 exactly where its maximum was
                dpre = ops.conv3x5_bwd_data_relu(dpre, self._images(name)[1], x_in, drop=below_drop,
                                                 dropped=below_drop is not None)
            else:
                cnn_util.wgrad_im2col(x_in, dpre, KH, KW, *self._g2d(li))
                din = cnn_util.dgrad_im2col(dpre, KH, KW, self._w2d(li))      # fp32, through GEMM + col2im
                below = relu_outs[li - 1] if li > 1 else None
                if below is None:            # the pooled CNN1 output: non-negative, > 0 where its window's maximum was
                    below = self._pooled_undropped(x_in, below_drop)
                dpre = ops.relu_bwd(din, below, drop=below_drop)
        # dpre is the gradient at the pooled CNN1 output (ReLU and dropout already applied): un-pool, then CNN1's
        # weight gradient (no data gradient)
        dpre1 = ops.maxpool3x1_bwd(dpre, c['arg1'], self.F)
        cnn_util.wgrad_im2col(c['x0'], dpre1, KH, KW, *self._g2d(0))
        ops.join_side(dev)           # the heads' gradients were issued on side lane 1
        self.ctx = None
        return None

    def _pooled_undropped(self, p1d, dr):
        """The gate of the pooled CNN1 output on the im2col path: its dropped form is > 0 where active and kept, the mask
        itself is applied by relu_bwd(drop=...), so the sign source must be the undropped pool -- recomputed from the
        stored ReLU output (one HBM pass over a 128-channel tensor)."""
        if dr is None:
            return p1d
        return ops.maxpool3x1_fwd(self.ctx['a1'])[0]
