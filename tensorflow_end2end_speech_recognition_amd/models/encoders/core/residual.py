"""Residual and dense-residual connections between the layers of the BLSTM / LSTM encoders
(encoder_residual / encoder_dense_residual).

The reference's recipes ask for them (config/ctc/encoders/residual_blstm_ctc.yml, dense_residual_blstm_ctc.yml,
config/attention/encoders/att_residual_blstm_location.yml, att_dense_residual_blstm_location.yml; both keys also stand in
blstm_ctc_baseline.yml and att_baseline.yml) and none of its running code reads them.  It has no statement of them, so the
semantics are fixed here.  With

  h_l   the output of layer l's cells (zero at frames t >= len[b]),
  m_l   that layer's dropout multiplier (1 / keep or 0; 1 without dropout),
  y_l   = m_l * h_l, what the DropoutWrapper emits,
  o_l   what layer l + 1 consumes; o_L is the encoder's `outputs`,

layer 1's input has another width, so the connections start behind layer 2:

  plain                    o_l = y_l
  encoder_residual         o_1 = y_1,  o_l = y_l + o_{l-1}            (l >= 2)
  encoder_dense_residual   o_1 = y_1,  o_l = y_l + sum_{k<l} o_k       (l >= 2): every earlier layer's SUMMED output is
                           added.  With the running sum S_l = sum_{k<=l} o_k:  o_l = y_l + S_{l-1},  S_l = S_{l-1} + o_l
                           (S_1 = o_1), so one extra tensor is enough; it is fp32 in both model dtypes.

The final state (c, h of the cells) is unchanged; rows past len[b] of every o_l are zero; both flags true raise
ValueError; a flag with num_layers < 2 builds the plain encoder.  No variable is added: a residual model and its plain
twin load each other's checkpoints.

Backward.  Let G_l = dL/do_l (everything that reaches o_l) and dx_{l+1} the input gradient of layer l + 1.  o_l feeds
layer l + 1 and, besides,
  residual   o_{l+1}:                     G_l = dx_{l+1} + G_{l+1}
  dense      S_l, which feeds o_{l+1} and S_{l+1}: with C_l = dL/dS_l,  C_l = G_{l+1} + C_{l+1}  (C_L = 0: nothing reads
             S_L) and  G_l = dx_{l+1} + C_l.
y_l enters o_l with factor one, so the layer's own output gradient is m_l * G_l: the mask applies to the sum, never to
what is passed on.  As one recursion over an fp32 tensor `carry` [T,Bp,W] that starts as d_outputs (= G_L = C_{L-1}):
the top layer L runs as in the plain stack (its mask applied by LSTMLayer.backward, its dx product issued WITHOUT the
mask of the layer below), and for l = L-1 .. 1, with dx_raw the dx product of layer l + 1,

  g      = dx_raw + carry            (= G_l)
  dout_l = m_l * g                   -> LSTMLayer.backward(..., dout_masked=True)
  carry  <- g  (residual)   or   g + carry  (dense: C_{l-1} = G_l + C_l)

Rounding points (the tests hold the kernels to them bit for bit): forward out = round_op(fl32(fl32(m * float(h)) +
float(skip))), multiply and add unfused, one rounding to the operand dtype; S = fl32(float(skip) + float(out)) from the
STORED out; backward g = fl32(dx_raw + carry), dout = fl32(m * g), dense carry fl32(g + carry).

One kernel pair (ops.residual_fwd / ops.residual_bwd, csrc/residual.hip) sits on the chain between two recurrences.  With
a dropout descriptor the forward kernel replaces that layer's asr_dropout_apply launch, so a training step gains no forward
launch and one backward launch per connected layer; a mask TENSOR from the caller keeps apply_mask and the kernels run
with keep = 1.  The dx product is written on valid frames only; the backward kernel knows the lengths and never loads a
padded frame.  The encoders always run one pipeline (ASR_ENC_HALVES is ignored) and never defer the top layer's dropout
to a head kernel.
"""
from .... import ops
from .blstm import WARM_BPTT, BLSTMEncoder
from .lstm import LSTMEncoder


def check_residual(encoder_residual, encoder_dense_residual):
    """None, 'residual' or 'dense' for the two recipe keys.  ValueError when both are true."""
    if encoder_residual and encoder_dense_residual:
        raise ValueError('encoder_residual and encoder_dense_residual exclude each other')
    return 'residual' if encoder_residual else ('dense' if encoder_dense_residual else None)


class _ResidualMixin(object):
    """The plain encoder (same variables, scopes, side-lane schedule, row plans, hooks) with skip connections."""

    def __init__(self, *args, **kw):
        self.dense = bool(kw.pop('dense', False))
        super(_ResidualMixin, self).__init__(*args, **kw)
        self._skip = self._sum = None

    # never deferred to a head kernel: the skip connection's kernel applies the top layer's dropout
    defer_top_dropout = property(lambda self: False, lambda self, value: None)

    def _split_rows(self, Bp):
        return 0

    def _connects(self, li):
        return li >= 1

    def _connect(self, li, x, mask, seq_len):
        if li == 0:
            self._skip, self._sum = x, None           # o_1 = y_1 (= S_1)
            return x
        drop = mask if isinstance(mask, tuple) else None    # (a mask tensor was applied by the layer: keep = 1 here)
        top = li + 1 == len(self.layers)
        if not self.dense:
            out = ops.residual_fwd(x, self._skip, seq_len, drop)
        elif top:                                     # nothing reads S_L
            out = ops.residual_fwd(x, self._sum if self._sum is not None else self._skip, seq_len, drop)
        elif self._sum is None:                       # layer 2: S_1 = o_1 in the operand dtype, S_2 a new fp32 tensor
            out, self._sum = ops.residual_fwd(x, self._skip, seq_len, drop, sum_out=True)
        else:                                         # S_l = S_{l-1} + o_l in place
            out, self._sum = ops.residual_fwd(x, self._sum, seq_len, drop, sum_out=self._sum)
        self._skip = None if top else out
        if top:
            self._sum = None
        return out

    def backward(self, d_outputs, d_final=None, need_input_grad=False, d_outputs_sub=None, top_masked=False):
        """As the plain encoder's; the recursion of the module docstring between two BPTT kernels."""
        if d_outputs_sub is not None or top_masked:
            raise ValueError('backward: the residual encoders take neither a sub-task gradient nor a masked top gradient')
        L = len(self.layers)
        seq_len = self.seq_len_padded
        d_outputs = d_outputs.contiguous()
        dout, carry = d_outputs, None
        for li in reversed(range(L)):
            top = li == L - 1
            dcf, dhf = d_final if (d_final is not None and top) else (None, None)
            if not top:
                mask = self.layers[li].ctx['mask']
                # the first carry is a new tensor (d_outputs is the caller's); from then on it is updated in place, and
                # dout always replaces dx_raw
                dout, carry = ops.residual_bwd(dout, carry if carry is not None else d_outputs, seq_len,
                                               mask if isinstance(mask, tuple) else None, self.dense, dout=dout,
                                               carry_out=carry)
                if mask is not None and not isinstance(mask, tuple):
                    dout = ops.apply_mask(dout, mask)
            cb = self.layers[li - 1].ctx if (li > 0 and WARM_BPTT) else None
            if cb is not None and (cb['gates'].numel() * cb['gates'].element_size() +
                                   cb['cs'].numel() * cb['cs'].element_size()) > (128 << 20):
                cb = None
            dout = self.layers[li].backward(dout, dcf, dhf, need_dx=(li > 0 or need_input_grad), dout_masked=not top,
                                            dx_mask=None, background=(li > 0),
                                            warm=(cb['gates'], cb['cs']) if cb is not None else None,
                                            dx_valid_only=(li > 0))
            ops.wait_event(getattr(self.layers[li], 'warm_event', None))
            if self.grad_ready_hook is not None:
                self.grad_ready_hook(li, self.layers[li])
        ops.join_side(d_outputs.device)
        return dout


class ResidualBLSTMEncoder(_ResidualMixin, BLSTMEncoder):
    """BLSTMEncoder with encoder_residual (dense=False) / encoder_dense_residual (dense=True)."""


class ResidualLSTMEncoder(_ResidualMixin, LSTMEncoder):
    """LSTMEncoder with encoder_residual (dense=False) / encoder_dense_residual (dense=True)."""


RESIDUAL = {'blstm': ResidualBLSTMEncoder, 'lstm': ResidualLSTMEncoder}


def load_residual(encoder_type):
    """The class with skip connections of an encoder key; ValueError for the families that have none."""
    if encoder_type not in RESIDUAL:
        raise ValueError('skip connections (encoder_residual / encoder_dense_residual) are implemented for the blstm and '
                         'lstm encoders, not for %r' % (encoder_type,))
    return RESIDUAL[encoder_type]
