"""TEST INFRASTRUCTURE ONLY: torch-CPU stand-ins for the time subsampling kernels (asr_time_subsample_fwd / _bwd), layered
over _cpu_ops.install, so that the host logic of models/encoders/core/subsample.py runs in the `-m "not gpu"` suite -- and
the statement the kernels and the models are held against: the reduction in numpy (forward and backward) and a float64
autograd encoder composed from oracle.lstm's layers with torch indexing for the reduction."""
import numpy as np
import torch

import _cpu_ops
from oracle import lstm as olstm
from oracle import model as omodel


# ---------------------------------------------------------------- the statement, in numpy
def subsample_fwd_np(x_tb, lens, kind, batch=None):
    """x [T,Bp,W], lens [Bp] -> (y [batch,T//2,W'] batch-major float32, lens >> 1 for all Bp rows)."""
    x_tb, lens = np.asarray(x_tb), np.asarray(lens)
    T, Bp, W = x_tb.shape
    B = Bp if batch is None else batch
    T2, lo = T // 2, np.minimum(np.maximum(lens, 0), T) >> 1
    y = np.zeros((B, T2, 2 * W if kind == 'concat' else W), dtype=np.float32)
    for b in range(B):
        for t in range(int(lo[b])):
            y[b, t] = x_tb[2 * t + 1, b] if kind == 'drop' else np.concatenate([x_tb[2 * t, b], x_tb[2 * t + 1, b]])
    return y, lo.astype(np.int32)


def subsample_bwd_np(dy_tb, len_out, T, kind):
    """dy [T//2,Bp,W'], len_out [Bp] -> dx [T,Bp,W] float32: the transpose of subsample_fwd_np."""
    dy_tb, len_out = np.asarray(dy_tb), np.asarray(len_out)
    T2, Bp, Wo = dy_tb.shape
    assert T2 == T // 2
    W = Wo // 2 if kind == 'concat' else Wo
    dx = np.zeros((T, Bp, W), dtype=np.float32)
    for b in range(Bp):
        for t in range(int(len_out[b])):
            if kind == 'drop':
                dx[2 * t + 1, b] = dy_tb[t, b]
            else:
                dx[2 * t, b], dx[2 * t + 1, b] = dy_tb[t, b, :W], dy_tb[t, b, W:]
    return dx


# ---------------------------------------------------------------- stand-ins of ops.time_subsample_*
def _time_subsample_fwd(x_tb, seq_len, batch, kind='drop'):
    if kind not in ('drop', 'concat'):
        raise ValueError('subsample_type is "drop" or "concat", got %r' % (kind,))
    y, lo = subsample_fwd_np(x_tb.detach().float().numpy(), seq_len.numpy(), kind, batch)
    return torch.from_numpy(y), torch.from_numpy(lo)


def _time_subsample_bwd(dy_tb, len_out, T, kind='drop', out=None):
    assert out is None
    return torch.from_numpy(subsample_bwd_np(dy_tb.detach().float().numpy(), len_out.numpy(), int(T), kind))


STAND_INS = dict(time_subsample_fwd=_time_subsample_fwd, time_subsample_bwd=_time_subsample_bwd)


def install(monkeypatch):
    ops = _cpu_ops.install(monkeypatch)
    for name, fn in STAND_INS.items():
        assert hasattr(ops, name), name
        monkeypatch.setattr(ops, name, fn)
    return ops


# ---------------------------------------------------------------- the statement with autograd (float64 torch)
def reduce_torch(x_tm, sl, kind):
    """x [T,B,W] (torch, differentiable), sl LongTensor [B] -> (y [T//2,B,W'], sl // 2)."""
    T2 = x_tm.shape[0] // 2
    first, second = x_tm[0:2 * T2:2], x_tm[1:2 * T2:2]
    y = second if kind == 'drop' else torch.cat([first, second], dim=2)
    sl2 = sl // 2
    live = (torch.arange(T2).unsqueeze(1) < sl2.unsqueeze(0)).to(y.dtype).unsqueeze(2)
    return y * live, sl2


def subsampled_encoder(inputs_bm, seq_len, layers, ndir, subsample_list, kind, drop_masks=None, **kw):
    """The plain oracle encoders (oracle.lstm.blstm_encoder / lstm_encoder) with a reduction behind every layer whose
    entry is true.  Returns (outputs [T >> k, B, E], reduced lengths, final state as the plain encoder's)."""
    assert len(subsample_list) == len(layers)
    x, sl = inputs_bm.transpose(0, 1), seq_len
    final, finals = None, []
    for li, layer in enumerate(layers):
        m = drop_masks[li] if drop_masks is not None else None
        if ndir == 2:
            m = m if m is not None else (None, None)
            x, final = olstm.blstm_layer(x, sl, layer[0], layer[1], m[0], m[1], **kw)
        else:
            x, st = olstm.dynamic_rnn(x, sl, layer, False, m, **kw)
            finals.append(st)
        if subsample_list[li]:
            x, sl = reduce_torch(x, sl, kind)
    return x, sl, (final if ndir == 2 else finals)


def ctc_model_forward(sd, inputs_btd, labels_list, seq_len, num_layers, ndir, subsample_list, kind, cell_clip=0.0,
                      operand_round=None, weight_decay=0.0):
    """oracle.model.ctc_model_forward for a subsampled encoder: dict(total_loss, ctc_losses, logits [T >> k,B,C],
    grads, seq_len (reduced)).  operand_round: the rounding points of the bf16-operand device path (inputs, kernels,
    output weights, every emitted h), as oracle.model.ctc_model_forward places them."""
    dtype = torch.float64
    if operand_round is not None:
        sd = dict(sd)
        for k in list(sd):
            if k.endswith('/kernel') or k == 'output/weights':
                sd[k] = operand_round(torch.as_tensor(np.asarray(sd[k]), dtype=dtype)).numpy()
        inputs_btd = operand_round(torch.as_tensor(np.asarray(inputs_btd), dtype=dtype)).numpy()
    layers = omodel.params_from_state_dict(sd, num_layers, ndir, dtype)
    w_out = torch.as_tensor(np.asarray(sd['output/weights']), dtype=dtype).clone().requires_grad_(True)
    b_out = torch.as_tensor(np.asarray(sd['output/biases']), dtype=dtype).clone().requires_grad_(True)
    x = torch.as_tensor(np.asarray(inputs_btd), dtype=dtype)
    sl = torch.as_tensor(np.asarray(seq_len), dtype=torch.long)
    peep = layers[0][0]['_peep'] if ndir == 2 else layers[0]['_peep']
    kw = dict(forget_bias=1.0, cell_clip=cell_clip, use_peephole=peep)
    if operand_round is not None:
        kw['h_round'] = operand_round
    enc, sl2, final = subsampled_encoder(x, sl, layers, ndir, subsample_list, kind, **kw)
    T, B, E = enc.shape
    logits = (enc.reshape(T * B, E) @ w_out + b_out).reshape(T, B, -1)
    losses = omodel.ctc_loss(logits, labels_list, sl2.numpy())
    total = losses.mean()
    named = {'output/weights': w_out, 'output/biases': b_out}
    for layer in layers:
        for p in (layer if ndir == 2 else (layer,)):
            base = p['_base']
            named[base + '/kernel'], named[base + '/bias'] = p['w'], p['b']
            if p['_peep']:
                named[base + '/w_i_diag'], named[base + '/w_f_diag'], named[base + '/w_o_diag'] = \
                    p['wci'], p['wcf'], p['wco']
    if weight_decay > 0:
        total = total + weight_decay * sum(0.5 * (v ** 2).sum() for n, v in named.items() if 'bias' not in n.lower())
    total.backward()
    return dict(total_loss=float(total.detach()), ctc_losses=losses.detach().numpy(), logits=logits.detach().numpy(),
                grads={n: v.grad.detach().numpy().copy() for n, v in named.items()}, enc=enc.detach().numpy(),
                seq_len=sl2.numpy(), final=final)


def patch_oracle_blstm_encoder(monkeypatch, full_seq_len, subsample_list, kind):
    """oracle.attention calls oracle.lstm.blstm_encoder by module attribute: swap it for the subsampled statement.  The
    wrapper closes over the FULL lengths and returns the reduced outputs; the oracle itself is then called with the
    reduced lengths (what its attention masks and its CTC head need)."""
    full = torch.as_tensor(np.asarray(full_seq_len), dtype=torch.long)

    def wrapped(inputs_bm, seq_len, layers, drop_masks=None, **kw):
        enc, sl2, final = subsampled_encoder(inputs_bm, full, layers, 2, subsample_list, kind, drop_masks, **kw)
        assert torch.equal(sl2, torch.as_tensor(np.asarray(seq_len), dtype=torch.long))
        return enc, final

    monkeypatch.setattr(olstm, 'blstm_encoder', wrapped)
