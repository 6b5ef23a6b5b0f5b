"""RNN language model (models/lm/base.py of the reference: class RNNLM, whose __init__ raises NotImplementedError there).

EXTENSION: the reference intended a language model (its CTC BeamSearchDecoder takes `alpha`, "language model weight", and
carries `# TODO: add LM score here`, models/ctc/decoders/beam_search_decoder.py:53,61,132) and defines none, so the
definition is this project's: an embedding, num_layers unidirectional LSTMBlockCell layers (forget bias 1, no peepholes,
optional cell clip, dropout on the layer outputs -- the encoder stack of models/encoders/core/lstm.py, not a second
recurrence path), a fully connected output layer with bias, and the masked token cross-entropy with the sequence_loss
weighting of AttentionSeq2Seq.compute_loss (asr_seq_xent) plus weight decay on non-bias variables.  The classes are the
attention decoder's output classes -- labels, <SOS>, <EOS> with the ids of the attention model it is fused with
(AttentionSeq2Seq.infer(lm=, lm_weight=), decoders/beam_search/lm_fusion.py).  fp32 operands only.

Variables (TF-style names, saved and restored by utils/training/checkpoint.Saver):
rnnlm/embedding/W_embedding [C2,Em], rnnlm/lstm_hidden{l}/lstm_cell/{kernel [Din_l+H,4H], bias [4H]} (l from 1),
rnnlm/output/{weights [H,C2], biases [C2]}."""
import numpy as np
import torch

from ... import ops
from ..._lib import ASR_F32
from ...utils.parameter import ParamStore
from ..encoders.core.lstm import LSTMEncoder
from ..encoders.core.rnn_util import declare_lstm_vars
from ..model_base import ModelBase

EMB = 'rnnlm/embedding/W_embedding'
OUT_W, OUT_B = 'rnnlm/output/weights', 'rnnlm/output/biases'


class _LMStack(LSTMEncoder):
    """LSTMEncoder under the language model's variable names."""

    def _declare(self, store, i, din, rng):
        return declare_lstm_vars(store, None, din, self.num_units, 1, False, self.parameter_init, rng,
                                 cell_scope='rnnlm/lstm_hidden%d/lstm_cell' % i)


class RNNLM(ModelBase):
    """RNNLM(num_classes, embedding_dim, num_units, num_layers, sos_index, eos_index, ...): num_classes is the attention
    decoder's output width (labels + <SOS> + <EOS>)."""

    def __init__(self, num_classes, embedding_dim, num_units, num_layers, sos_index, eos_index, parameter_init=0.1,
                 clip_grad_norm=None, clip_activation=None, weight_decay=0.0, name='rnnlm', dtype='f32', device='cuda:0',
                 seed=0):
        super(RNNLM, self).__init__()
        if ops.dtype_id(dtype) != ASR_F32:
            raise ValueError('RNNLM has fp32 operands only, got dtype=%r' % (dtype,))
        assert float(weight_decay) >= 0, 'weight_decay must not be a negative value.'
        assert clip_grad_norm is None or clip_grad_norm > 0, 'clip_grad_norm must be larger than 0.'
        self.num_classes, self.embedding_dim = int(num_classes), int(embedding_dim)
        self.num_units, self.num_layers = int(num_units), int(num_layers)
        self.sos_index, self.eos_index = int(sos_index), int(eos_index)
        if not (0 <= self.sos_index < self.num_classes and 0 <= self.eos_index < self.num_classes) or self.num_layers < 1:
            raise ValueError('RNNLM: <SOS> / <EOS> must be among the %d classes, num_layers >= 1' % self.num_classes)
        self.parameter_init = parameter_init
        self.clip_grad_norm = clip_grad_norm
        self.clip_activation = clip_activation
        self.weight_decay = float(weight_decay)
        self.name = name
        self.dtype = ASR_F32
        self.device = torch.device(device)
        self.seed = seed
        self._calls = 0
        self._tape = None
        rng = np.random.RandomState(seed)
        u = lambda *s: rng.uniform(-parameter_init, parameter_init, size=s)              # noqa: E731
        self.store = st = ParamStore(self.device)
        st.declare(EMB, (self.num_classes, self.embedding_dim), u(self.num_classes, self.embedding_dim))
        self.encoder = _LMStack(num_units=self.num_units, num_proj=None, num_layers=self.num_layers,
                                lstm_impl='LSTMBlockCell', use_peephole=False, parameter_init=parameter_init,
                                clip_activation=clip_activation, time_major=True, name='rnnlm_stack', dtype='f32', seed=seed)
        self.encoder.build(st, self.embedding_dim, rng)
        st.declare(OUT_W, (self.num_units, self.num_classes), u(self.num_units, self.num_classes))
        st.declare(OUT_B, (self.num_classes,), np.zeros(self.num_classes))
        st.finalize()

    # ------------------------------------------------------------------ training
    def _tables(self, labels, labels_seq_len):
        labels_np = (ops.host_ints(labels) if torch.is_tensor(labels) else np.asarray(labels)).astype(np.int64)
        lsl = (ops.host_ints(labels_seq_len) if torch.is_tensor(labels_seq_len) else np.asarray(labels_seq_len)).astype(np.int64)
        B = labels_np.shape[0]
        if labels_np.ndim != 2 or lsl.shape != (B,) or (lsl < 2).any() or lsl.max() > labels_np.shape[1]:
            raise ValueError('RNNLM: labels [B,L] (<SOS> first, <EOS> last, padded) and labels_seq_len [B] >= 2')
        To = int(lsl.max()) - 1
        live = (np.arange(To)[None, :] < (lsl - 1)[:, None])                              # [B,To]
        ids = np.where(live, labels_np[:, :To], self.eos_index)
        tgt = np.where(live, labels_np[:, 1:To + 1], 0)
        if ((ids < 0) | (ids >= self.num_classes) | (tgt < 0) | (tgt >= self.num_classes)).any():
            raise ValueError('RNNLM: a label lies outside the %d classes' % self.num_classes)
        return B, To, lsl, live, ids, tgt

    def compute_loss(self, labels, labels_seq_len, keep_prob=1.0, is_training=True):
        """labels [B,L] (<SOS> first, <EOS> last, padded) and labels_seq_len [B], as utils/dataset/attention.py yields them:
        the model reads labels[:, :-1] and is scored against labels[:, 1:].  Returns (loss 0-dim, logits [B,To,C2])."""
        dev, st = self.device, self.store
        B, To, lsl, live, ids, tgt = self._tables(labels, labels_seq_len)
        Bp = B + (-B) % 16                                   # the recurrence pads the batch to whole 16-row tiles
        C2, Em, H = self.num_classes, self.embedding_dim, self.num_units
        tm = lambda a, fill, dt: np.concatenate([a.T, np.full((To, Bp - B), fill, a.dtype)], axis=1).astype(dt)   # noqa: E731
        ids_tm = ops.to_device(tm(ids, self.eos_index, np.int32), torch.int32, dev)        # [To,Bp]
        tgt_tm = ops.to_device(tm(tgt, 0, np.int32), torch.int32, dev)
        live_tm = ops.to_device(tm(live.astype(np.float32), 0.0, np.float32), torch.float32, dev)
        ids_bm = ops.to_device(ids.astype(np.int32), torch.int32, dev)                      # [B,To]
        lens = (lsl - 1).astype(np.int32)
        self.encoder._lens_host = lens
        emb = ops.embedding_gather(st[EMB], ids_bm.view(-1)).view(B, To, Em)
        rs = None
        if is_training and keep_prob is not None and float(keep_prob) < 1.0:
            self._calls += 1
            rs = (self.seed, self._calls << 40)
        self.encoder(emb, ops.to_device(lens, torch.int32, dev), float(keep_prob if keep_prob is not None else 1.0),
                     is_training, rng_state=rs)
        out = self.encoder._out_tm.contiguous()                                             # [To,Bp,H]
        logits2d = ops.gemm(out.view(To * Bp, H), st[OUT_W], bias=st[OUT_B])
        wsum = float(live.sum())
        row_loss, dlogits = ops.seq_xent(logits2d, tgt_tm.view(-1), live_tm.view(-1), 1e-10, 1.0 / (wsum + 1e-12),
                                         want_grad=is_training)
        seq_loss = row_loss.sum() / (wsum + 1e-12)
        total = seq_loss
        if self.weight_decay > 0:
            l2 = torch.zeros((), dtype=torch.float32, device=dev)
            ops.weight_decay(None, st.flat, st.plan, st.decay_mask, self.weight_decay, l2_out=l2)
            total = total + l2
        self.sequence_loss = seq_loss
        self._tape = dict(dlogits=dlogits, out=out, ids=ids_tm, live=live_tm, To=To, Bp=Bp) if is_training else None
        total._asr_model = self
        return total, logits2d.view(To, Bp, C2)[:, :B].transpose(0, 1)

    def _backward(self):
        if self._tape is None:
            raise RuntimeError('train()/compute_gradients() needs a preceding compute_loss(is_training=True)')
        tp, st = self._tape, self.store
        To, Bp, H, Em = tp['To'], tp['Bp'], self.num_units, self.embedding_dim
        dl = tp['dlogits']
        ops.gemm(tp['out'].view(To * Bp, H), dl, transA=True, out=st.g(OUT_W))
        ops.colsum(dl, out=st.g(OUT_B))
        dout = ops.gemm(dl, st[OUT_W], transB=True)
        dx = self.encoder.backward(dout.view(To, Bp, H), need_input_grad=True).contiguous()
        # (frames behind a sequence's end carry no gradient into the embedding)
        dx = ops.apply_mask(dx.view(To * Bp, Em), tp['live'].view(-1, 1).expand(To * Bp, Em).contiguous())
        ops.embedding_scatter(dx, tp['ids'].view(-1), self.num_classes, st.g(EMB))
        ops.join_side(self.device)
        if self.weight_decay > 0:
            ops.weight_decay(st.grad, st.flat, st.plan, st.decay_mask, self.weight_decay)
        self._tape = None

    def perplexity(self, labels, labels_seq_len):
        """exp of the mean token cross-entropy (no dropout, no weight decay term)."""
        self.compute_loss(labels, labels_seq_len, 1.0, is_training=False)
        return float(torch.exp(self.sequence_loss))

    # ------------------------------------------------------------------ single step (the decode path's form)
    def decode_weights(self):
        """What ops.lm_step / ops.att_decoder_beam_lm read: views of the variables, nothing copied."""
        st = self.store
        cells = ['rnnlm/lstm_hidden%d/lstm_cell' % (l + 1) for l in range(self.num_layers)]
        return dict(emb=st[EMB], kernels=[st[c + '/kernel'] for c in cells], biases=[st[c + '/bias'] for c in cells],
                    W_out=st[OUT_W], b_out=st[OUT_B], cell_clip=float(self.clip_activation or 0.0), sos=self.sos_index)

    def step_state(self, batch):
        """(c, h) [L,batch,H] zeros: the empty history."""
        z = lambda: torch.zeros((self.num_layers, int(batch), self.num_units), dtype=torch.float32, device=self.device)  # noqa: E731
        return z(), z()

    def step(self, words, state):
        """One step: words [batch] int32 (each row's last word, <SOS> first), state (c, h).  Returns (logits [batch,C2] raw,
        (c', h'))."""
        words = ops.to_device(words, torch.int32, self.device)
        logits, c, h = ops.lm_step(self.decode_weights(), words, state[0], state[1])
        return logits, (c, h)
