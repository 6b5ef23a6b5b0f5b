"""Time subsampling inside the BLSTM / LSTM encoders (subsample_list / subsample_type).

The reference's recipes ask for it (examples/timit/config/ctc/regularization/blstm_ctc_subsample.yml:
subsample_list [False, True, False, False, False]; config/attention/att_baseline.yml: subsample_type drop) and its
models/encoders/core/pyramidal_blstm.py is an unfinished attempt at the 'concat' form (frames t, t+1 stacked, :160-170,
lengths halved with floor, :120-122).  It has no running statement, so the semantics are fixed here:

  subsample_list  num_layers booleans; entry i (0-based) true: the output of layer i+1, after its dropout wrapper, is
                  reduced 2x in time before layer i+2 consumes it (a true last entry reduces the encoder's own output);
  one reduction   of x [T,B,W] with lengths len: T' = T // 2, len' = len // 2, an odd trailing frame is discarded;
                  'drop'   y[t'] = x[2t'+1]              (the second frame of the pair: the forward direction has seen both)
                  'concat' y[t'] = [x[2t'] ; x[2t'+1]]   (W' = 2W: the next layer's kernel has 2W input rows)
                  rows t' >= len' are zero; the backward pass is the exact transpose.

The stack is cut into segments of consecutive layers at one time resolution.  Each segment is an ordinary BLSTMEncoder /
LSTMEncoder building into the shared ParamStore under the plain encoder's variable names (a layer offset continues the
numbering), so a 'drop' model is checkpoint-compatible with its unsubsampled twin and a 'concat' model differs only in the
input height of the kernels that follow a reduction.  Between two segments sits one kernel pair
(ops.time_subsample_fwd / _bwd); the segments' own code paths -- the tuned default -- are untouched.
"""
import numpy as np
import torch

from .... import ops
from ...._lib import ASR_F32
from ....utils.parameter import ParamStore
from .blstm import BLSTMEncoder
from .lstm import LSTMEncoder

SUBSAMPLE_TYPES = ('drop', 'concat')


def check_subsample(subsample_list, subsample_type, num_layers):
    """The list as a tuple of bools (None: all false).  ValueError on a wrong length or an unknown type."""
    if subsample_type not in SUBSAMPLE_TYPES:
        raise ValueError('subsample_type is "drop" or "concat", got %r' % (subsample_type,))
    if subsample_list is None:
        return (False,) * int(num_layers)
    flags = tuple(bool(f) for f in subsample_list)
    if len(flags) != int(num_layers):
        raise ValueError('subsample_list has %d entries for %d layers' % (len(flags), num_layers))
    return flags


def any_subsample(subsample_list):
    return subsample_list is not None and any(bool(f) for f in subsample_list)


def shift_lengths(seq_len, k):
    """seq_len >> k for a numpy array, a list or a tensor."""
    if torch.is_tensor(seq_len):
        return seq_len >> k if k else seq_len
    return np.asarray(seq_len) >> k


class _Offset(object):
    """A segment: layers layer_offset+1 .. of the whole stack, named as the plain encoder names them."""
    layer_offset = 0

    def _declare(self, store, i, din, rng):
        return super(_Offset, self)._declare(store, i + self.layer_offset, din, rng)

    def _declare_projected(self, store, i, din, P, rng):
        return super(_Offset, self)._declare_projected(store, i + self.layer_offset, din, P, rng)


class _BLSTMSegment(_Offset, BLSTMEncoder):
    pass


class _LSTMSegment(_Offset, LSTMEncoder):
    pass


class _SubsampledEncoderBase(object):
    segment_cls = None

    def __init__(self, num_units, num_proj, num_layers, lstm_impl, use_peephole, parameter_init,
                 clip_activation, time_major=True, name='lstm_encoder', dtype=ASR_F32, seed=0,
                 subsample_list=None, subsample_type='drop'):
        self.subsample_list = check_subsample(subsample_list, subsample_type, num_layers)
        self.subsample_type = subsample_type
        if lstm_impl == 'LSTMCell' and num_proj not in (None, 0):
            raise ValueError('time subsampling is not implemented for LSTMCell projection layers (num_proj)')
        self.num_units, self.num_layers = num_units, num_layers
        self.time_major = time_major
        self.name = name
        self.dtype = ops.dtype_id(dtype)
        self.seed = seed
        self.num_reductions = sum(self.subsample_list)
        # segments: a cut behind every layer whose entry is true; a true LAST entry reduces the encoder's own output
        cuts = [i + 1 for i, f in enumerate(self.subsample_list[:-1]) if f]
        starts, ends = [0] + cuts, cuts + [num_layers]
        self._reduce_last = bool(self.subsample_list[-1])
        self._offsets = starts
        self.segments = []
        for lo, hi in zip(starts, ends):
            # (num_proj: dropped, as the plain encoder drops it for every lstm_impl but LSTMCell, refused above)
            seg = self.segment_cls(num_units=num_units, num_proj=None, num_layers=hi - lo, lstm_impl=lstm_impl,
                                   use_peephole=use_peephole, parameter_init=parameter_init,
                                   clip_activation=clip_activation, time_major=True, name=name, dtype=dtype, seed=seed)
            seg.layer_offset = lo
            self.segments.append(seg)
        self.layers = None
        self.store = None
        self.scope_prefix = ''
        self.grad_ready_hook = None    # callable(global layer index, LSTMLayer), fired per finished layer, top layer first
        self.side_extra = None         # run once per call, on the first segment's side lane
        self.side_extra_event = None
        self.want_f32_outputs = True   # only the last segment makes the fp32 copy
        self._lens_host = None
        self._bounds = []

    def build(self, store, input_dim, rng, scope_prefix=''):
        self.store, self.scope_prefix = store, scope_prefix
        self.layers = []
        din = input_dim
        for seg in self.segments:
            din = seg.build(store, din, rng, scope_prefix)
            self.layers += seg.layers
            if seg is not self.segments[-1] or self._reduce_last:
                din = self._reduced_width(din)
        self.output_dim = din
        return din

    def _reduced_width(self, w):
        return 2 * w if self.subsample_type == 'concat' else w

    def _ensure_built(self, inputs):
        if self.layers is None:
            store = ParamStore(inputs.device)
            self.build(store, inputs.shape[-1], np.random.RandomState(self.seed))
            store.finalize()

    def output_seq_len(self, seq_len):
        """The lengths of the encoder's outputs for input lengths seq_len: seq_len >> (number of true entries)."""
        return shift_lengths(seq_len, self.num_reductions)

    def _check_lengths(self, lens_host):
        lens = np.asarray(lens_host).ravel()
        gone = (lens > 0) & ((lens >> self.num_reductions) == 0)
        if gone.any():
            raise ValueError('%d utterance(s) shorter than %d frames reduce to zero frames under subsample_list %r'
                             % (int(gone.sum()), 1 << self.num_reductions, list(self.subsample_list)))

    def __call__(self, inputs, inputs_seq_len, keep_prob, is_training, drop_masks=None, rng_state=None):
        """As BLSTMEncoder.__call__; outputs [T >> k, B, output_dim] (k: the number of true entries).  drop_masks[li]
        has layer li's own [T_li, Bpad, ndir*H] shape."""
        self._ensure_built(inputs)
        lens_host, self._lens_host = self._lens_host, None
        if lens_host is not None:
            self._check_lengths(lens_host)
        if rng_state is None and drop_masks is None and is_training and keep_prob is not None and keep_prob < 1.0:
            self._dropout_calls = getattr(self, '_dropout_calls', 0) + 1
            rng_state = (self.seed, self._dropout_calls << 40)
        B = inputs.shape[0]
        x_bt, lens = inputs, inputs_seq_len
        finals, self._bounds = [], []
        n = len(self.segments)
        for s, (seg, off) in enumerate(zip(self.segments, self._offsets)):
            last = s == n - 1
            reduce = not last or self._reduce_last
            seg.side_extra = self.side_extra if s == 0 else None
            seg.want_f32_outputs = self.want_f32_outputs and not reduce
            # s reductions lie below segment s: its row plans stay host-built
            seg._lens_host = None if lens_host is None else np.asarray(lens_host).ravel() >> s
            # the dropout counters stay indexed by the global layer number: the segment adds li * 2^32 to what it is given
            rs = (rng_state[0], rng_state[1] + off * (1 << 32)) if rng_state is not None else None
            dm = drop_masks[off:off + seg.num_layers] if drop_masks is not None else None
            seg(x_bt, lens, keep_prob, is_training, drop_masks=dm, rng_state=rs)
            if s == 0:
                self.side_extra_event = seg.side_extra_event
            finals += seg._finals
            if reduce:
                x_tb = seg._out_op
                # between two segments the real utterances only (the next segment pads its batch itself); the
                # encoder's own output keeps the padded batch the heads work on
                y, len_out = ops.time_subsample_fwd(x_tb, seg.seq_len_padded, x_tb.shape[1] if last else B,
                                                    self.subsample_type)
                self._bounds.append((x_tb.shape[0], len_out))
                x_bt, lens = y, len_out[:B]
        top = self.segments[-1]
        self.batch, self.pad_b = B, top.pad_b
        if self._reduce_last:
            x = ops.bt_to_tb(x_bt, self.dtype)                   # [T',Bp,W'] in the operand dtype, as a segment leaves it
            self.seq_len_padded = self._bounds[-1][1]
            out = ops.cast_to_f32(x) if (x.dtype != torch.float32 and self.want_f32_outputs) else x
        else:
            x, out, self.seq_len_padded = top._out_op, top._out_tm, top.seq_len_padded
        self._out_op, self._out_tm = x, out
        self._final_ch = top._final_ch
        self._finals = finals
        final_state = top._state_tuple(finals, len(finals))
        out_user = out[:, :B]
        if not self.time_major:
            out_user = out_user.transpose(0, 1)
        return out_user, final_state

    def backward(self, d_outputs, d_final=None, need_input_grad=False):
        """d_outputs: gradient w.r.t. the time-major padded-batch outputs [T >> k, Bpad, output_dim] fp32.  The top
        segment first; between two segments the transpose of the reduction maps the upper one's input gradient to the
        lower one's time rate."""
        bounds = list(self._bounds)
        dx = d_outputs
        if self._reduce_last:
            T, len_out = bounds.pop()
            dx = ops.time_subsample_bwd(dx.contiguous(), len_out, T, self.subsample_type)
        n = len(self.segments)
        hook = self.grad_ready_hook
        for s in reversed(range(n)):
            seg, off = self.segments[s], self._offsets[s]
            seg.grad_ready_hook = (lambda li, layer, off=off: hook(off + li, layer)) if hook is not None else None
            dx = seg.backward(dx, d_final if s == n - 1 else None, need_input_grad=(s > 0 or need_input_grad))
            if s > 0:
                T, len_out = bounds.pop()
                dx = ops.time_subsample_bwd(dx.contiguous(), len_out, T, self.subsample_type)
        self._bounds = []
        return dx


class SubsampledBLSTMEncoder(_SubsampledEncoderBase):
    """BLSTMEncoder with subsample_list / subsample_type."""
    segment_cls = _BLSTMSegment


class SubsampledLSTMEncoder(_SubsampledEncoderBase):
    """LSTMEncoder with subsample_list / subsample_type."""
    segment_cls = _LSTMSegment


SUBSAMPLED = {'blstm': SubsampledBLSTMEncoder, 'lstm': SubsampledLSTMEncoder}


def load_subsampled(encoder_type):
    """The subsampled class of an encoder key; ValueError for the families that have none."""
    if encoder_type not in SUBSAMPLED:
        raise ValueError('time subsampling (subsample_list with a true entry) is implemented for the blstm and lstm '
                         'encoders, not for %r' % (encoder_type,))
    return SUBSAMPLED[encoder_type]
