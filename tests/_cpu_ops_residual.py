"""TEST INFRASTRUCTURE ONLY: the statement of the skip connections between recurrent layers (encoder_residual /
encoder_dense_residual, models/encoders/core/residual.py) -- the two kernels in numpy with their rounding points, torch-CPU
stand-ins for ops.residual_fwd / ops.residual_bwd layered over _cpu_ops.install (so that the host logic runs in the
`-m "not gpu"` suite), and a float64 autograd encoder composed from oracle.lstm's layers, which are called WITHOUT masks:
the dropout multiplier, the sum and its roundings are the statement's own."""
import numpy as np
import torch

import _cpu_ops
from oracle import lstm as olstm
from oracle import model as omodel

MODES = ('residual', 'dense')


# ---------------------------------------------------------------- the kernels, in numpy
def bf16_np(a):
    """float32 array rounded to bf16 (nearest even) and back."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def _live(lens, T, Bp):
    lens = np.minimum(np.maximum(np.asarray(lens).astype(np.int64), 0), T)
    assert lens.shape == (Bp,)
    return (np.arange(T)[:, None] < lens[None, :])[:, :, None]


def residual_fwd_np(h, skip, lens, m=None, bf16=False):
    """h, skip [T,Bp,W] float32 (the values the kernel loads), lens [Bp], m the fp32 multipliers or None (keep = 1) ->
    (out float32 holding the operand-dtype values, sum float32): out = round_op(fl32(fl32(m h) + skip)),
    sum = fl32(skip + out as stored); zero at t >= len, where nothing is looked at."""
    h, skip = np.asarray(h, dtype=np.float32), np.asarray(skip, dtype=np.float32)
    T, Bp, W = h.shape
    live = _live(lens, T, Bp)
    with np.errstate(invalid='ignore'):
        a = h if m is None else (np.asarray(m, dtype=np.float32) * h).astype(np.float32)
        o = (a + skip).astype(np.float32)
        if bf16:
            o = bf16_np(o)
        s = (skip + o).astype(np.float32)
    zero = np.zeros_like(o)
    return np.where(live, o, zero), np.where(live, s, zero)


def residual_bwd_np(dx_raw, carry, lens, m=None, dense=False, dtype=np.float32):
    """g = dx_raw + carry, dout = m g, carry_out = g or g + carry (dense), each rounded to `dtype` (float32: the kernel;
    float64: the recursion of the host test); zero at t >= len."""
    dx_raw, carry = np.asarray(dx_raw, dtype=dtype), np.asarray(carry, dtype=dtype)
    T, Bp, W = dx_raw.shape
    live = _live(lens, T, Bp)
    with np.errstate(invalid='ignore'):
        g = (dx_raw + carry).astype(dtype)
        d = g if m is None else (np.asarray(m, dtype=dtype) * g).astype(dtype)
        c = (g + carry).astype(dtype) if dense else g
    zero = np.zeros_like(g)
    return np.where(live, d, zero), np.where(live, c, zero)


# ---------------------------------------------------------------- stand-ins of ops.residual_*
def _mask_of(shape, drop):
    if drop is None or float(drop[0]) >= 1.0:
        return None
    return _cpu_ops._dropout_mask(tuple(shape), *drop).numpy()


def _residual_fwd(h_tb, skip, seq_len, drop=None, sum_out=None, out=None):
    assert out is None
    if tuple(skip.shape) != tuple(h_tb.shape) or seq_len.shape[0] != h_tb.shape[1]:
        raise ValueError('residual_fwd: shapes')
    o, s = residual_fwd_np(h_tb.detach().float().numpy(), skip.detach().float().numpy(), seq_len.numpy(),
                           _mask_of(h_tb.shape, drop), bf16=h_tb.dtype == torch.bfloat16)
    out = torch.from_numpy(o).to(h_tb.dtype)
    if sum_out is None:
        return out
    if sum_out is True:
        return out, torch.from_numpy(s)
    sum_out.copy_(torch.from_numpy(s))
    return out, sum_out


def _residual_bwd(dx_raw, carry, seq_len, drop=None, dense=False, dout=None, carry_out=None):
    d, c = residual_bwd_np(dx_raw.detach().numpy(), carry.detach().numpy(), seq_len.numpy(),
                           _mask_of(dx_raw.shape, drop), dense)
    d, c = torch.from_numpy(d), torch.from_numpy(c)
    if dout is not None:
        d = dout.copy_(d)
    if carry_out is not None:
        c = carry_out.copy_(c)
    return d, c


STAND_INS = dict(residual_fwd=_residual_fwd, residual_bwd=_residual_bwd)


def install(monkeypatch):
    ops = _cpu_ops.install(monkeypatch)
    for name, fn in STAND_INS.items():
        assert hasattr(ops, name), name
        monkeypatch.setattr(ops, name, fn)
    return ops


# ---------------------------------------------------------------- the statement with autograd (float64 torch)
def _f32_round(x):
    return x.to(torch.float32).to(x.dtype)


def connect_step(mode, li, y, o_prev, S, operand_round=None):
    """One layer of the statement: (o_l, S_l) from y_l, o_{l-1} and S_{l-1} (li 0-based).  o_1 = y_1; residual
    o_l = y_l + o_{l-1}; dense o_l = y_l + S_{l-1}, S_l = S_{l-1} + o_l (S_1 = o_1).  mode None: the plain stack.
    operand_round: one (straight-through) rounding of every o_l to the operand dtype, the running sum kept in fp32."""
    assert mode in MODES + (None,)
    rnd = (lambda t: olstm.ste_round(t, operand_round)) if operand_round is not None else (lambda t: t)
    if li == 0 or mode is None:
        o = rnd(y)
    else:
        o = rnd(y + (o_prev if mode == 'residual' else S))
    if mode == 'dense':
        S = o if li == 0 else S + o
        if operand_round is not None and li > 0:
            S = olstm.ste_round(S, _f32_round)
    return o, S


def residual_encoder(inputs_bm, seq_len, layers, ndir, mode, masks=None, operand_round=None, **kw):
    """The oracle's layers (blstm_layer / dynamic_rnn, no masks handed to them) with the connections of `mode` between
    them.  masks[li]: the multipliers m_l [T,B,ndir*H] or None.  Returns (outputs [T,B,E], final state as the plain oracle
    encoders give it, [o_1 .. o_L])."""
    x = inputs_bm.transpose(0, 1)
    final, finals, outs, S = None, [], [], None
    for li, layer in enumerate(layers):
        if ndir == 2:
            h, final = olstm.blstm_layer(x, seq_len, layer[0], layer[1], None, None, **kw)
        else:
            h, st = olstm.dynamic_rnn(x, seq_len, layer, False, None, **kw)
            finals.append(st)
        y = h * masks[li] if (masks is not None and masks[li] is not None) else h
        o, S = connect_step(mode, li, y, outs[-1] if outs else None, S, operand_round)
        outs.append(o)
        x = o
    return x, (final if ndir == 2 else finals), outs


def ctc_model_forward(sd, inputs_btd, labels_list, seq_len, num_layers, ndir, mode, cell_clip=0.0, operand_round=None,
                      weight_decay=0.0, masks=None):
    """oracle.model.ctc_model_forward over residual_encoder: dict(total_loss, ctc_losses, logits [T,B,C], grads, enc).
    operand_round: the rounding points of the bf16-operand device path (inputs, kernels, output weights, every emitted h
    through h_round, every o_l once).  masks[li]: numpy / torch multipliers [T,B,ndir*H] of layer li, or None."""
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
    if masks is not None:
        masks = [None if m is None else torch.as_tensor(np.asarray(m), dtype=dtype) for m in masks]
    enc, final, _ = residual_encoder(x, sl, layers, ndir, mode, masks, operand_round, **kw)
    T, B, E = enc.shape
    logits = (enc.reshape(T * B, E) @ w_out + b_out).reshape(T, B, -1)
    losses = omodel.ctc_loss(logits, labels_list, sl.numpy())
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
                final=final)


def patch_oracle_blstm_encoder(monkeypatch, mode):
    """oracle.attention calls oracle.lstm.blstm_encoder by module attribute: swap it for the statement with the
    connections of `mode` (no dropout: the attention oracle hands no masks)."""
    def wrapped(inputs_bm, seq_len, layers, drop_masks=None, **kw):
        assert drop_masks is None
        enc, final, _ = residual_encoder(inputs_bm, torch.as_tensor(np.asarray(seq_len), dtype=torch.long), layers, 2,
                                         mode, None, kw.get('h_round'), **kw)
        return enc, final

    monkeypatch.setattr(olstm, 'blstm_encoder', wrapped)
