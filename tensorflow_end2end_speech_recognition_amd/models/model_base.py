"""Base class for all models -- mirror of models/model_base.py:23-166.

The reference builds TF graph ops; here every method executes eagerly on the
HIP kernels.  Kept: OPTIMIZER_CLS_NAMES keys (model_base.py:12-20, including the
'nestrov' spelling), _set_optimizer (momentum 0.9 for momentum/nestrov),
train(loss, optimizer, learning_rate), _clip_gradients (per-variable
tf.clip_by_norm, model_base.py:148-152) and the ValueError on unknown names.
"""
import numpy as np
import torch

from .. import ops
from .._lib import OPTIMIZER_IDS

OPTIMIZER_CLS_NAMES = dict((k, k) for k in OPTIMIZER_IDS)

# TF1 slot initial values: Adagrad accumulator 0.1, RMSProp rms ones
_SLOT0_INIT = {'adagrad': 0.1, 'rmsprop': 1.0}


class Optimizer(object):
    """tf.train.*Optimizer stand-in over the model's flat parameter buffer."""

    def __init__(self, name, learning_rate, store):
        self.name = name
        self.opt_id = OPTIMIZER_IDS[name]
        self.learning_rate = learning_rate
        self.store = store
        self.slot0 = self.slot1 = None
        if name != 'sgd':
            self.slot0 = torch.full_like(store.flat, _SLOT0_INIT.get(name, 0.0))
        if name in ('adadelta', 'rmsprop', 'adam'):
            self.slot1 = torch.zeros_like(store.flat)
        self.global_step = 0

    def compute_gradients(self, loss, model=None):
        """Runs the backward pass of the model that produced `loss`; returns the list of
        (gradient view, variable name) pairs (train_ctc.py:112 tower_grads)."""
        model = model or getattr(loss, '_asr_model', None)
        if model is None:
            raise ValueError('compute_gradients needs the model that produced the loss')
        model._backward()
        st = self.store
        return [(st.g(n), n) for n in st.names]

    def apply_gradients(self, grads_and_vars=None, global_step=None, learning_rate=None):
        lr = self.learning_rate if learning_rate is None else learning_rate
        st = self.store
        if st.perturbed:
            raise RuntimeError('apply_gradients: the weights still carry weight noise (compute_gradients of the model that '
                               'perturbed them restores the clean ones); an update must not land on noisy weights')
        self.global_step += 1
        ops.optimizer_step(self.opt_id, st.flat, st.grad, self.slot0, self.slot1, lr, self.global_step)
        st.mark_dirty()
        if st.flat.is_cuda:
            # hand-off timeouts of the multi-CU recurrence kernels must not train on silently (raises AsrError)
            ops.watch_async_errors(st.flat.device)
        return self.global_step

    def state_dict(self):
        return {'slot0': self.slot0, 'slot1': self.slot1, 'global_step': self.global_step,
                'name': self.name}


class ModelBase(object):
    # Gaussian weight noise (extension keyword weight_noise_std of CTC / AttentionSeq2Seq; 0: none of it runs)
    weight_noise_std = 0.0
    _noise_calls = 0
    # input augmentation (extension keywords input_noise_std, freq_mask_*, time_mask_*, input_channels; off: none of it runs)
    input_noise_std = 0.0
    freq_mask_num = freq_mask_width = time_mask_num = time_mask_width = 0
    time_mask_ratio = 1.0
    input_channels = None
    _augment_calls = 0

    def __init__(self, *args, **kwargs):
        self.optimizer = None
        self.clip_grad_norm = None
        self.store = None

    # ---- weight noise (the rules: _noise_begin)
    def _set_weight_noise(self, std):
        std = float(std or 0.0)
        if not 0.0 <= std < float('inf'):
            raise ValueError('weight_noise_std must be finite and >= 0, got %r' % (std,))
        self.weight_noise_std = std

    def _noise_begin(self):
        """Top of a training compute_loss.  Weight noise (Graves 2011): at every training step zero-mean Gaussian noise of
        standard deviation weight_noise_std is added to ALL trainable variables (store.flat, biases and peepholes included)
        for the forward and the backward pass, and the update goes to the clean weights.  Step k (the k-th training
        compute_loss, from 1) draws ops.weight_noise_perturb(seed = model.seed + 7, offset = k << 40).  The perturbed
        weights live from here to the end of this model's _backward(), which puts the clean bits back BEFORE the
        weight-decay gradient, the clip, the data-parallel mean and the optimizer; weight decay (both terms) and
        store.state_dict() read the clean weights (store.clean) throughout.  Any other use of the weights in between -- a
        dev compute_loss, infer / decode, load_state_dict, a second training compute_loss -- first restores the clean
        weights and drops the tape, so a later train() raises.
        Data parallel: ranks build the model with one seed and so draw the same noise; a rank with an empty shard makes no
        compute_loss and so no perturbation that step, which is harmless because every replica applies the identical
        update to identical clean weights."""
        if self.weight_noise_std > 0.0:
            self._noise_guard()
            self._noise_calls += 1
            self.store.perturb(self.weight_noise_std, self.seed + 7, self._noise_calls << 40)

    def _noise_end(self):
        """In _backward(), behind the last product on the perturbed weights and before the weight-decay gradient."""
        if self.store.perturbed:
            self.store.restore()

    def _noise_guard(self):
        """Every other entry that reads the weights: a perturbation still live ends here, and with it its tape."""
        if self.store.perturbed:
            self.store.restore()
            self._tape = None

    def _noise_tape(self):
        """Top of _backward(): the tape of a forward whose perturbation is gone (load_state_dict) is no tape."""
        if self.weight_noise_std > 0.0 and not self.store.perturbed:
            self._tape = None

    # ---- input augmentation (the rules: _augment_inputs)
    def _set_input_augment(self, input_size, input_noise_std=0.0, freq_mask_num=0, freq_mask_width=0, time_mask_num=0,
                           time_mask_width=0, time_mask_ratio=1.0, input_channels=None):
        """The seven extension keywords of CTC / AttentionSeq2Seq (and their subclasses); all defaults: nothing runs.
        `input_size`: the model's input_size; the columns it is fed are stacked / spliced copies of that many."""
        std = float(input_noise_std or 0.0)
        if not 0.0 <= std < float('inf'):
            raise ValueError('input_noise_std must be finite and >= 0, got %r' % (input_noise_std,))
        nf, nt = int(freq_mask_num or 0), int(time_mask_num or 0)
        fw, tw = int(freq_mask_width or 0), int(time_mask_width or 0)
        for name, n in (('freq_mask_num', nf), ('time_mask_num', nt)):
            if not 0 <= n <= 8:
                raise ValueError('%s must be in [0, 8], got %r' % (name, n))
        if fw < 0 or tw < 0:
            raise ValueError('freq_mask_width / time_mask_width must be >= 0, got %r / %r' % (fw, tw))
        ratio = float(1.0 if time_mask_ratio is None else time_mask_ratio)
        if not 0.0 <= ratio <= 1.0:
            raise ValueError('time_mask_ratio must be in [0, 1], got %r' % (time_mask_ratio,))
        input_size = int(input_size)
        if input_channels is None:
            input_channels = input_size // 3 if input_size % 3 == 0 else input_size
        n_ch = int(input_channels)
        if not 1 <= n_ch <= input_size or input_size % n_ch != 0:
            raise ValueError('input_channels must divide input_size = %d, got %r' % (input_size, input_channels))
        if fw >= n_ch:
            raise ValueError('freq_mask_width must be below input_channels = %d, got %r' % (n_ch, fw))
        self.input_noise_std = std
        self.freq_mask_num, self.freq_mask_width = nf, fw
        self.time_mask_num, self.time_mask_width, self.time_mask_ratio = nt, tw, ratio
        self.input_channels = n_ch

    def _augment_on(self):
        return (self.input_noise_std > 0.0 or (self.freq_mask_num > 0 and self.freq_mask_width > 0) or
                (self.time_mask_num > 0 and self.time_mask_width > 0 and self.time_mask_ratio > 0.0))

    def _augment_key(self):
        """seed + 11 + (rank << 32): data-parallel ranks draw different noise and masks for their shards (keys seed + 1,
        2, 3, 7, 13 are taken by the dropout streams, scheduled sampling and the weight noise)."""
        rank = 0
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            rank = torch.distributed.get_rank()
        return self.seed + 11 + (rank << 32)

    def _augment_inputs(self, inputs_dev, seq_len_dev):
        """A TRAINING compute_loss, behind ops.to_device of the inputs and the lengths and in front of _build: Gaussian
        noise of input_noise_std on every valid element, freq_mask_num bands of at most freq_mask_width of the
        input_channels base channels (the same band in the static / delta / double-delta groups and in every stacked or
        spliced copy) and time_mask_num runs of at most min(time_mask_width, time_mask_ratio * len_b) frames per
        utterance set to 0 (Park et al. 2019, without the time warp), in ONE ops.input_augment call into a fresh tensor:
        the caller's tensor is never written, padded frames keep their bits.  The k-th augmented training call of this
        model (from 1; a counter of its own, apart from the dropout and weight-noise counters) draws under key
        _augment_key() at offset k << 40.  Dev losses, infer and decode see the clean inputs; what a model derives lazily
        from a training forward is that of the augmented inputs.  Every setting off: the argument comes back, nothing is
        counted."""
        if not self._augment_on():
            return inputs_dev
        self._augment_calls += 1
        x = inputs_dev if inputs_dev.is_contiguous() else inputs_dev.contiguous()
        return ops.input_augment(x, seq_len_dev, self.input_channels, noise_std=self.input_noise_std,
                                 freq_masks=(self.freq_mask_num, self.freq_mask_width),
                                 time_masks=(self.time_mask_num, self.time_mask_width, self.time_mask_ratio),
                                 mask_value=0.0, seed=self._augment_key(), offset=self._augment_calls << 40)

    def _build(self, *args, **kwargs):
        """Construct model graph."""
        raise NotImplementedError  # (the reference raises NotADirectoryError by typo, model_base.py:30)

    def create_placeholders(self):
        """Create placeholders and append them to list."""
        raise NotImplementedError

    def compute_loss(self, *args, **kwargs):
        """Operation for computing loss."""
        raise NotImplementedError

    def _add_noise_to_inputs(self, inputs, stddev=0.075, inputs_seq_len=None):
        """model_base.py:40-55 (declared there with its body commented out): inputs [B,T,F] + N(0, stddev^2), as a new
        device tensor; the caller's tensor is untouched.  The op of _augment_inputs with the noise alone: the same key,
        and the model's next augmentation offset.  `inputs_seq_len` (extension argument): frames t >= len_b stay as
        they are; default: every frame is valid."""
        stddev = float(stddev)
        if not 0.0 <= stddev < float('inf'):
            raise ValueError('stddev must be finite and >= 0, got %r' % (stddev,))
        x = ops.to_device(inputs, torch.float32, self.device).contiguous()
        if inputs_seq_len is None:
            inputs_seq_len = np.full((x.shape[0],), x.shape[1], dtype=np.int32)
        lens = ops.to_device(inputs_seq_len, torch.int32, self.device)
        self._augment_calls += 1
        return ops.input_augment(x, lens, x.shape[2], noise_std=stddev, seed=self._augment_key(),
                                 offset=self._augment_calls << 40)

    def _add_noise_to_gradients(self, grads_and_vars, gradient_noise_scale, stddev=0.075):
        raise NotImplementedError

    def _set_optimizer(self, optimizer, learning_rate):
        """model_base.py:68-95."""
        optimizer = optimizer.lower()
        if optimizer not in OPTIMIZER_CLS_NAMES:
            raise ValueError(
                "Optimizer name should be one of [%s], you provided %s." %
                (", ".join(OPTIMIZER_CLS_NAMES), optimizer))
        return Optimizer(optimizer, learning_rate, self.store)

    def train(self, loss, optimizer, learning_rate):
        """One training step for the forward pass that produced `loss`
        (model_base.py:97-133: compute_gradients -> _clip_gradients -> apply_gradients)."""
        if self.optimizer is None or self.optimizer.name != optimizer.lower():
            self.optimizer = self._set_optimizer(optimizer, learning_rate)
        self.optimizer.learning_rate = learning_rate
        grads_and_vars = self.optimizer.compute_gradients(loss, model=self)
        if self.clip_grad_norm is not None:
            grads_and_vars = self._clip_gradients(grads_and_vars)
        return self.optimizer.apply_gradients(grads_and_vars)

    def _clip_gradients(self, grads_and_vars):
        """Per-variable tf.clip_by_norm(grad, clip_norm=self.clip_grad_norm), model_base.py:135-166,
        as one multi-tensor pass over the flat gradient buffer."""
        ops.clip_by_norm_multi(self.store.grad, self.store.plan, float(self.clip_grad_norm))
        return grads_and_vars
