"""Student CTC model -- mirror of models/ctc/student_ctc.py:20-389 (class StudentCTC) on the HIP path.

Same constructor arguments and asserts (student_ctc.py:56-62), attributes (name, num_classes = +1 blank, *_pl_list,
summaries_*), and methods: create_placeholders_ctc / create_placeholders_xe, compute_ctc_loss -> (total_loss,
logits [T,B,C]), compute_xe_loss -> (total_loss, logits [B,C]), train (ModelBase), decoder, posteriors, compute_ler (as in
CTC).  The encoder is imported directly, as the reference does (student_ctc.py:14-17, 89-120), not through the registry.

`is_training` selects BOTH the batch-normalization mode and whether the backward is kept:
  is_training=True   batch statistics (over every image handed in: on the CTC path all B x T frames, padding included),
                     dropout at keep_prob, activations kept for train(); the moving averages are updated by train() --
                     once per step, from that step's forward statistics (the UPDATE_OPS dependency of the train op,
                     model_base.py:120,129) -- and never by a forward alone.
  is_training=False  the moving averages normalize, no dropout, nothing kept (train() after it raises).
The reference's own evaluation (eval_student.py:85-93) runs with is_training=True and no train op: batch statistics,
nothing updated -- here, compute_*_loss(..., is_training=True) without train().

Weight decay follows 'bias' not in name over the trainable variables: the batch-norm gamma and beta ARE decayed, the
biases and the moving averages (not trainable) are not.  Single device only: the moving averages are per replica, and
data-parallel training would let them diverge, so world_size > 1 raises.

Extra keyword arguments of the HIP build (not in the reference): `dtype` ('f32' parity path | 'bf16' operands with fp32
accumulate and fp32 batch statistics), `device`, `seed`, `world_size`.
"""
import numpy as np
import torch

from ... import ops
from ..._lib import ASR_BF16, ASR_F32
from ...utils.parameter import ParamStore, StateStore
from ..encoders.core import cnn_util
from ..encoders.core.subsample import any_subsample, load_subsampled
from ..encoders.core.student_cnn import (StudentCNNCTCEncoder, StudentCNNCompactCTCEncoder, StudentCNNXEEncoder,
                                         StudentCNNCompactXEEncoder)
from ..model_base import ModelBase
from .ctc import CTC, Placeholder, _not_enough_time, truncated_normal

ENCODERS = {
    'student_cnn': StudentCNNCTCEncoder,
    'student_cnn_compact': StudentCNNCompactCTCEncoder,
    'student_cnn_xe': StudentCNNXEEncoder,
    'student_cnn_compact_xe': StudentCNNCompactXEEncoder,
}


class StudentCTC(ModelBase):
    """models/ctc/student_ctc.py:20 StudentCTC (see the module docstring for is_training)."""
    head_scope = 'output'

    def __init__(self, encoder_type, input_size, num_classes, splice=1, num_stack=1, parameter_init=0.1,
                 clip_grad_norm=None, weight_decay=0.0, time_major=True, dtype='f32', device='cuda:0', seed=0,
                 world_size=None, subsample_list=None, subsample_type='drop'):
        super(StudentCTC, self).__init__()
        if any_subsample(subsample_list):
            load_subsampled(encoder_type)        # ValueError: the student CNNs have no subsampled form
        assert input_size % 3 == 0, 'input_size must be divisible by 3 (+ delta, double delta features).'
        assert splice % 2 == 1, 'splice must be the odd number'
        if clip_grad_norm is not None:
            assert float(clip_grad_norm) > 0, 'clip_grad_norm must be larger than 0.'
        assert float(weight_decay) >= 0, 'weight_decay must not be a negative value.'
        if world_size is None:
            from ...utils.training.multi_gpu import is_distributed
            world_size = torch.distributed.get_world_size() if is_distributed() else 1
        if int(world_size) > 1:
            raise ValueError('StudentCTC trains on a single device: its batch-normalization moving averages are '
                             'per replica and would diverge under data-parallel training (world_size = %d)'
                             % int(world_size))

        self.encoder_type = encoder_type
        self.input_size = input_size
        self.splice = splice
        self.num_stack = num_stack
        self.num_classes = num_classes + 1  # + blank
        self.parameter_init = parameter_init
        self.clip_grad_norm = clip_grad_norm
        self.weight_decay = weight_decay
        self.summaries_train = []
        self.summaries_dev = []
        self.inputs_pl_list = []
        self.labels_pl_list = []
        self.inputs_seq_len_pl_list = []
        self.keep_prob_pl_list = []
        self.time_major = time_major
        self.name = encoder_type + '_ctc'
        if encoder_type not in ENCODERS:
            raise NotImplementedError
        self.dtype = ops.dtype_id(dtype)
        self.device = torch.device(device)
        self.seed = seed
        self._dropout_calls = 0
        cls = ENCODERS[encoder_type]
        if cls.XE:
            self.encoder = cls(input_size=input_size, splice=splice, num_stack=num_stack, parameter_init=parameter_init,
                               dtype=self.dtype)
        else:
            self.encoder = cls(input_size=input_size, splice=splice, num_stack=num_stack, parameter_init=parameter_init,
                               time_major=time_major, dtype=self.dtype)
        self.encoder.seed = seed

        rng = np.random.RandomState(seed)
        self.store = ParamStore(self.device)
        self.state = StateStore(self.device)
        enc_dim = self.encoder.build(self.store, self.state, rng)
        self.store.declare(self.head_scope + '/weights', (enc_dim, self.num_classes),
                           truncated_normal(rng, parameter_init, (enc_dim, self.num_classes)))
        self.store.declare(self.head_scope + '/biases', (self.num_classes,), np.zeros(self.num_classes))
        self.store.finalize()
        self.state.finalize()
        self._tape = None

    def variables(self):
        """(name, shape, trainable) of every variable in the reference's creation order."""
        order = self.encoder.var_order() + [(self.head_scope + '/weights', True), (self.head_scope + '/biases', True)]
        return [(n, tuple((self.store if t else self.state)[n].shape), t) for n, t in order]

    # ------------------------------------------------------------------ placeholders
    def create_placeholders_ctc(self):
        """student_ctc.py:198-211."""
        self.inputs_pl_list.append(Placeholder('input', np.float32, [None, None, self.input_size * self.splice]))
        self.labels_pl_list.append(Placeholder('labels'))
        self.inputs_seq_len_pl_list.append(Placeholder('inputs_seq_len', np.int32, [None]))
        self.keep_prob_pl_list.append(Placeholder('keep_prob', np.float32))

    def create_placeholders_xe(self):
        """student_ctc.py:213-223."""
        self.inputs_pl_list.append(Placeholder('input', np.float32, [None, self.input_size]))
        self.labels_pl_list.append(Placeholder('label', np.float32, [None, self.num_classes]))
        self.keep_prob_pl_list.append(Placeholder('keep_prob', np.float32))

    # ------------------------------------------------------------------ graph pieces
    def _rng_state(self, keep_prob, is_training):
        if is_training and keep_prob is not None and float(keep_prob) < 1.0:
            self._dropout_calls += 1
            return (self.seed, self._dropout_calls << 40)
        return None

    def _head(self, x_op):
        sh = self.store.shadow(self.dtype)
        return ops.gemm(x_op, sh[self.head_scope + '/weights'], bias=self.store[self.head_scope + '/biases'],
                        out_dtype=ASR_F32)

    def _weight_decay_loss(self, loss):
        if self.weight_decay > 0:
            l2 = torch.zeros((), dtype=torch.float32, device=self.device)
            ops.weight_decay(None, self.store.flat, self.store.plan, self.store.decay_mask, self.weight_decay,
                             l2_out=l2)
            return loss + l2
        return loss

    def _check_encoder(self, xe):
        if self.encoder.XE != xe:
            raise ValueError('%s is a%s encoder: use compute_%s_loss' % (self.encoder_type, 'n XE' if not xe else ' CTC',
                                                                         'xe' if not xe else 'ctc'))

    def compute_ctc_loss(self, inputs, labels, inputs_seq_len, keep_prob, scope=None, softmax_temperature=1,
                         is_training=True):
        """student_ctc.py:225-300.  inputs [B,T,input_size*splice] fp32; labels: SparseTensor triple or dense [B,Lmax]
        padded -1; inputs_seq_len [B].  Returns (total_loss 0-dim tensor, logits [T,B,num_classes])."""
        self._check_encoder(False)
        dev = self.device
        inputs = ops.to_device(inputs, torch.float32, dev)
        B, T, D = inputs.shape
        flat, offsets, max_len = CTC._labels_to_flat(labels, B)
        Bp = B + (-B) % 16                               # the CTC kernels tile 16 utterances
        lens = np.minimum(np.maximum(np.asarray(ops.host_ints(inputs_seq_len), dtype=np.int64), 0), T)
        if Bp > B:
            offsets = np.concatenate([offsets, np.full(Bp - B, offsets[-1], dtype=np.int32)])
        seq_pad = np.concatenate([lens, np.zeros(Bp - B, np.int64)]).astype(np.int32)
        seq_d, off_d, flat_d = ops.upload_ints(dev, [seq_pad, offsets, flat if len(flat) else np.zeros(1, np.int32)])
        N = B * T
        enc = self.encoder.forward_images(inputs.view(N, D), keep_prob, is_training,
                                          self._rng_state(keep_prob, is_training))          # [N, U], b*T + t order
        U = enc.shape[1]
        # time-major rows t*Bp + b; the utterances that fill the 16-row tile read an appended zero row
        inv, fwd = self._tm_index(B, T, Bp, dev)
        x_tm = cnn_util.gather_time_major(torch.cat([enc, enc.new_zeros(1, U)], 0), inv)
        logits = self._head(x_tm).view(T, Bp, self.num_classes)
        inv_temp = 1.0 / float(softmax_temperature)
        ctc_in = ops.scale_(logits.clone(), inv_temp) if softmax_temperature != 1 else logits
        ctc_losses, grad, ninf = ops.ctc_loss(ctc_in, flat_d, off_d, seq_d, max_len, grad_scale=inv_temp / B,
                                              want_grad=is_training)
        total_loss = self._weight_decay_loss(ctc_losses[:B].mean())
        self.ctc_losses = ctc_losses[:B]
        self.num_infeasible = ninf
        ops.defer_zero_check(ninf, _not_enough_time, blocking=not is_training)
        self._tape = dict(kind='ctc', dlogits=grad, x=x_tm, fwd=fwd, B=B, T=T, Bp=Bp, N=N) if is_training else None
        total_loss._asr_model = self
        return total_loss, logits[:, :B]

    def _tm_index(self, B, T, Bp, dev):
        """(for each row t*Bp + b of the time-major padded grid its image b*T + t, or B*T = the appended zero row; for
        each image its row of the grid), cached per batch geometry."""
        key = (B, T, Bp, str(dev))
        cache = self.__dict__.setdefault('_index_cache', {})
        if key not in cache:
            t, b = np.meshgrid(np.arange(T), np.arange(Bp), indexing='ij')
            inv = np.where(b < B, b * T + t, B * T).astype(np.int32).reshape(-1)       # row t*Bp + b
            fwd = (np.arange(T)[None, :] * Bp + np.arange(B)[:, None]).astype(np.int32)          # image b*T + t
            if len(cache) >= 16:
                cache.clear()
            cache[key] = (ops.to_device(inv, torch.int32, dev), ops.to_device(fwd.reshape(-1), torch.int32, dev))
        return cache[key]

    def compute_xe_loss(self, inputs, soft_targets, keep_prob, scope=None, softmax_temperature=1, is_training=True):
        """student_ctc.py:302-359: reduce_mean(softmax_cross_entropy_with_logits(labels=soft_targets, logits)).
        inputs [B, input_size] fp32, soft_targets [B, num_classes].  `softmax_temperature` is accepted and IGNORED, as
        in the reference (its division is commented out, student_ctc.py:323-326)."""
        self._check_encoder(True)
        dev = self.device
        inputs = ops.to_device(inputs, torch.float32, dev)
        targets = ops.to_device(soft_targets, torch.float32, dev).contiguous()
        B = inputs.shape[0]
        enc = self.encoder.forward_images(inputs, keep_prob, is_training, self._rng_state(keep_prob, is_training))
        logits = self._head(enc)
        row_loss, grad = ops.softmax_xent_soft(logits, targets, grad_scale=1.0 / B, want_grad=is_training)
        total_loss = self._weight_decay_loss(row_loss.mean())
        self.xe_losses = row_loss
        self._tape = dict(kind='xe', dlogits=grad, x=enc, B=B, N=B) if is_training else None
        total_loss._asr_model = self
        return total_loss, logits

    # ------------------------------------------------------------------ backward / step
    def _backward(self):
        if self._tape is None:
            raise RuntimeError('train()/compute_gradients() needs a preceding compute_*_loss(is_training=True)')
        tape, st = self._tape, self.store
        C = self.num_classes
        dl2d = tape['dlogits'].reshape(-1, C)
        x_op = tape['x']
        sh = st.shadow(self.dtype)
        dl_op = ops.cast_from_f32(dl2d, ASR_BF16) if self.dtype == ASR_BF16 else dl2d
        ops.gemm(x_op, dl_op, transA=True, out=st.g(self.head_scope + '/weights'))
        ops.colsum(dl2d, out=st.g(self.head_scope + '/biases'))
        d = ops.gemm(dl_op, sh[self.head_scope + '/weights'], transB=True, out_dtype=ASR_F32)
        if tape['kind'] == 'ctc':                        # time-major padded rows back to the b*T + t images
            d = ops.embedding_gather(d, tape['fwd'])
        self.encoder.backward_images(d)
        if self.weight_decay > 0:
            ops.weight_decay(st.grad, st.flat, st.plan, st.decay_mask, self.weight_decay)
        self._tape = None

    def train(self, loss, optimizer, learning_rate):
        """ModelBase.train, then the batch-normalization UPDATE_OPS of that step's forward (model_base.py:120,129)."""
        step = super(StudentCTC, self).train(loss, optimizer, learning_rate)
        self.encoder.commit()
        return step

    # ------------------------------------------------------------------ decode / eval (as CTC)
    decoder = CTC.decoder
    posteriors = CTC.posteriors
    compute_ler = CTC.compute_ler
