"""Base class for all models -- mirror of models/model_base.py:23-166.

The reference builds TF graph ops; here every method executes eagerly on the
HIP kernels.  Kept: OPTIMIZER_CLS_NAMES keys (model_base.py:12-20, including the
'nestrov' spelling), _set_optimizer (momentum 0.9 for momentum/nestrov),
train(loss, optimizer, learning_rate), _clip_gradients (per-variable
tf.clip_by_norm, model_base.py:148-152) and the ValueError on unknown names.
"""
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

    def _build(self, *args, **kwargs):
        """Construct model graph."""
        raise NotImplementedError  # (the reference raises NotADirectoryError by typo, model_base.py:30)

    def create_placeholders(self):
        """Create placeholders and append them to list."""
        raise NotImplementedError

    def compute_loss(self, *args, **kwargs):
        """Operation for computing loss."""
        raise NotImplementedError

    def _add_noise_to_inputs(self, inputs, stddev=0.075):
        raise NotImplementedError

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
