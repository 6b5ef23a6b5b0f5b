"""Student CNN encoders -- mirrors of models/encoders/core/student_cnn_ctc.py, student_cnn_compact_ctc.py,
student_cnn_xe.py and student_cnn_compact_xe.py (the distillation students of StudentCTC).

Every frame is an image [H = num_channels, W = splice * num_stack, 3]:
  CNN1  conv 9x9 SAME 3 -> C1 + bias + ReLU, batch_norm, max_pool [3,1] / [3,1] SAME (H -> ceil(H / 3))
  CNN2  conv 3x4 SAME C1 -> C2 + bias + ReLU, batch_norm, max_pool [1,1] (the identity)
  flatten NHWC, then n_fc fully connected layers of U units with ReLU; dropout(keep_prob) after each of them in the CTC
  forms and in student_cnn_compact_xe, none in student_cnn_xe (student_cnn_xe.py:119-128).
Sizes: student_cnn*: C1 128, C2 256, 4 x 2048; student_cnn_compact*: C1 64, C2 128, 2 x 768.
num_channels = input_size // 3 // num_stack for the CTC forms (input [B, T, input_size * splice]) and
input_size // 3 // num_stack // splice for the XE forms (input [B, input_size]), as each reference class defines it.

Variables, in creation order: CNN1/conv/{weight,bias} (truncated normal(parameter_init), zeros; cnn_util.py:66-69),
CNN1/batch_norm/{beta,gamma,avg_mean,avg_variance}, the same for CNN2, fc{i}/{weights,biases}.  The moving averages are
trainable=False and live in the model's StateStore (batch_norm.py).

Batch statistics are taken over every image the encoder is handed: on the CTC path all B x T frames of the batch,
padded frames included (the reference reshapes the whole [B, T, D] input), so padding changes the valid frames' outputs
exactly as it does in the reference.

Execution.  bf16 models: CNN1 is asr_im2col + GEMM (3 input channels, K = 243) with bias + ReLU in the epilogue and an
fp32 output; CNN2 is the implicit 3x4 GEMM (asr_conv3x4_*, bf16 operands, fp32 output).  Batch statistics are fp32
(asr_bn_stats); asr_bn_apply writes the next layer's bf16 operand, fused with the pool.  fp32 models (the parity path):
both convolutions are asr_im2col + GEMM, backward through asr_col2im.  `conv_path` records the path each layer took.
"""
import numpy as np
import torch

from .... import ops
from ...._lib import ASR_BF16, ASR_F32
from . import cnn_util
from .batch_norm import BatchNorm


class _StudentCNN(object):
    C1, C2, N_FC, UNITS = 128, 256, 4, 2048
    XE = False
    FC_DROPOUT = True

    def __init__(self, input_size, splice, num_stack, parameter_init, time_major=True, name=None, dtype=ASR_F32):
        assert input_size % 3 == 0
        if self.XE:
            self.num_channels = (input_size // 3) // num_stack // splice
        else:
            self.num_channels = (input_size // 3) // num_stack
        self.splice = splice
        self.num_stack = num_stack
        self.parameter_init = parameter_init
        self.time_major = time_major
        self.name = name or self.NAME
        self.dtype = ops.dtype_id(dtype)
        self.seed = 0                 # dropout stream when used without a model (StudentCTC sets its own)
        self.F = self.num_channels
        self.W = splice * num_stack
        self.Hp = (self.F + 2) // 3
        self.flat = self.Hp * self.W * self.C2
        self.output_dim = self.UNITS
        self.convs = [('CNN1/conv', 9, 9, 3, self.C1), ('CNN2/conv', 3, 4, self.C1, self.C2)]
        self.fcs = ['fc%d' % i for i in range(1, self.N_FC + 1)]
        self.bns = [BatchNorm('CNN1', self.C1), BatchNorm('CNN2', self.C2)]
        self.implicit = True          # A/B switch (probe, tests): False runs CNN2 as asr_im2col + GEMM on bf16 models
        self.conv_path = {}
        self.ctx = None
        self.store = None

    @property
    def input_dim(self):
        return self.F * self.W * 3

    # ------------------------------------------------------------------ variables
    def build(self, store, state, rng):
        """Declares the variables in the reference's creation order; returns the output width."""
        zeros = lambda n: np.zeros(n)
        ones = lambda n: np.ones(n)
        for (name, kh, kw, cin, cout), bn in zip(self.convs, self.bns):
            cnn_util.declare_conv(store, name, kh, kw, cin, cout, rng, self.parameter_init)
            bn.declare(store, state, ones, zeros)
        din = self.flat
        for name in self.fcs:
            cnn_util.declare_fc(store, name, din, self.UNITS, rng, self.parameter_init)
            din = self.UNITS
        self.store, self.state = store, state
        return self.UNITS

    def var_order(self):
        """(name, trainable) of every variable in creation order."""
        out = []
        for (name, _, _, _, _), bn in zip(self.convs, self.bns):
            out += [(name + '/weight', True), (name + '/bias', True)]
            out += [(bn.names[0], True), (bn.names[1], True), (bn.names[2], False), (bn.names[3], False)]
        for name in self.fcs:
            out += [(name + '/weights', True), (name + '/biases', True)]
        return out

    # ------------------------------------------------------------------ one layer's views
    def _w2d(self, li):
        """the [kh*kw*Cin, Cout] view of layer li's weight in the operand dtype"""
        name, kh, kw, cin, cout = self.convs[li]
        return self.store.shadow(self.dtype)[name + '/weight'].view(kh * kw * cin, cout)

    def _g2d(self, li):
        """(the [kh*kw*Cin, Cout] view of layer li's weight gradient, its bias gradient)"""
        name, kh, kw, cin, cout = self.convs[li]
        return self.store.g(name + '/weight').view(kh * kw * cin, cout), self.store.g(name + '/bias')

    def _images(self):
        c = self.ctx.setdefault('wimg', None)
        if c is None:
            c = self.ctx['wimg'] = ops.conv3x4_prep_weights(self.store['CNN2/conv/weight'])
        return c

    # ------------------------------------------------------------------ forward / backward over images
    def forward_images(self, x, keep_prob, is_training, rng_state=None):
        """x fp32 [N, F*W*3] (frame-major rows) -> [N, U] in the operand dtype."""
        st = self.store
        sh = st.shadow(self.dtype)
        bf = self.dtype == ASR_BF16
        N = x.shape[0]
        F, W = self.F, self.W
        keep = float(keep_prob) if keep_prob is not None else 1.0
        drop = is_training and keep < 1.0 and self.FC_DROPOUT
        if drop and rng_state is None:
            self._dropout_calls = getattr(self, '_dropout_calls', 0) + 1
            rng_state = (self.seed, self._dropout_calls << 40)
        self.ctx = {}
        x0 = x.contiguous().view(N, F, W, 3)
        x0 = ops.cast_from_f32(x0, ASR_BF16) if bf else x0
        a1 = cnn_util.conv_im2col(x0, 9, 9, self._w2d(0), st['CNN1/conv/bias'], torch.float32)    # fp32 ReLU output
        p1, _ = self.bns[0].forward(a1, is_training, True, self.dtype)   # [N, Hp, W, C1] operand
        path = {'CNN1/conv': 'im2col'}
        if bf and self.implicit:
            wf = self._images()[0]
            a2 = ops.conv3x4_fwd(p1, wf, st['CNN2/conv/bias'], relu=True, out_dtype=ASR_F32)
            path['CNN2/conv'] = 'implicit'
        else:
            a2 = cnn_util.conv_im2col(p1, 3, 4, self._w2d(1), st['CNN2/conv/bias'], torch.float32)
            path['CNN2/conv'] = 'im2col'
        self.conv_path = path
        z2, _ = self.bns[1].forward(a2, is_training, False, self.dtype)  # [N, Hp, W, C2] operand
        drops = [(keep, rng_state[0] + 7, rng_state[1] + (k << 32)) if drop else None for k in range(len(self.fcs))]
        h_in, fc = cnn_util.fc_forward(st, sh, self.fcs, z2.view(N, self.flat), drops)
        self.ctx.update(x0=x0, p1=p1, a2=a2, fc=fc, implicit=path['CNN2/conv'] == 'implicit', N=N)
        return h_in

    def backward_images(self, d):
        """d fp32 [N, U]: gradient at the encoder output; fills the gradients of every variable."""
        c, st = self.ctx, self.store
        if c is None:
            raise RuntimeError('%s: backward needs a preceding forward' % self.name)
        sh = st.shadow(self.dtype)
        N = c['N']
        d = cnn_util.fc_backward(st, sh, self.fcs, c['fc'], d)
        dz2 = d.view(N, self.Hp, self.W, self.C2)
        dpre2 = self.bns[1].backward(dz2, self.dtype)
        p1 = c['p1']
        if c['implicit']:
            ops.conv3x4_bwd_weight_bias(p1, dpre2, *self._g2d(1))
            dp1 = ops.conv3x4_bwd_data(dpre2, self._images()[1])
        else:
            cnn_util.wgrad_im2col(p1, dpre2, 3, 4, *self._g2d(1))
            dp1 = cnn_util.dgrad_im2col(dpre2, 3, 4, self._w2d(1))
        dpre1 = self.bns[0].backward(dp1, self.dtype)
        cnn_util.wgrad_im2col(c['x0'], dpre1, 9, 9, *self._g2d(0))
        self.ctx = None

    def commit(self):
        for bn in self.bns:
            bn.commit()


class _StudentCNNCTC(_StudentCNN):
    """The CTC forms: __call__(inputs [B, T, F*W*3], inputs_seq_len, keep_prob, is_training) -> (outputs, None)."""

    def __call__(self, inputs, inputs_seq_len, keep_prob, is_training, rng_state=None):
        B, T, D = inputs.shape
        assert D == self.input_dim, 'input_dim %d != num_channels * splice * num_stack * 3' % D
        out = self.forward_images(inputs.contiguous().view(B * T, D), keep_prob, is_training, rng_state)
        out = out.view(B, T, self.UNITS)
        return (out.transpose(0, 1) if self.time_major else out), None


class _StudentCNNXE(_StudentCNN):
    """The XE forms: __call__(inputs [B, F*W*3], keep_prob, is_training) -> outputs [B, U]."""
    XE = True

    def __call__(self, inputs, keep_prob, is_training, rng_state=None):
        B, D = inputs.shape
        assert D == self.input_dim, 'input_dim %d != num_channels * splice * num_stack * 3' % D
        return self.forward_images(inputs, keep_prob, is_training, rng_state)


class StudentCNNCTCEncoder(_StudentCNNCTC):
    """student_cnn_ctc.py:32 StudentCNNCTCEncoder."""
    NAME = 'cnn_student_encoder'


class StudentCNNCompactCTCEncoder(_StudentCNNCTC):
    """student_cnn_compact_ctc.py:32 StudentCNNCompactCTCEncoder."""
    NAME = 'cnn_student_compact_encoder'
    C1, C2, N_FC, UNITS = 64, 128, 2, 768


class StudentCNNXEEncoder(_StudentCNNXE):
    """student_cnn_xe.py:32 StudentCNNXEEncoder (no dropout after its FC layers)."""
    NAME = 'cnn_student_xe_encoder'
    FC_DROPOUT = False


class StudentCNNCompactXEEncoder(_StudentCNNXE):
    """student_cnn_compact_xe.py:32 StudentCNNCompactXEEncoder (dropout after each FC layer)."""
    NAME = 'cnn_student_compact_xe_encoder'
    C1, C2, N_FC, UNITS = 64, 128, 2, 768
