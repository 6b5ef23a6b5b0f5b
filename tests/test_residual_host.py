"""Host logic of the skip connections between recurrent layers (encoder_residual / encoder_dense_residual) on the CPU
stand-ins: the backward recursion of models/encoders/core/residual.py against autograd of the statement, the encoders under
CTC / JointCTCAttention against the float64 statement (tests/_cpu_ops_residual.py), the keyword contract of the models,
and the TIMIT recipe."""
import os
import sys

import numpy as np
import pytest
import torch

import _cpu_ops
import _cpu_ops_residual as res
from _corpus import make_timit_like
from oracle import attention as oatt
from oracle import optim as oopt

MODES = res.MODES
KW = {'residual': dict(encoder_residual=True), 'dense': dict(encoder_dense_residual=True)}


# ---------------------------------------------------------------- the recursion itself
@pytest.mark.parametrize('L', [2, 4])
@pytest.mark.parametrize('mode', MODES)
def test_backward_recursion_equals_autograd_of_the_statement(mode, L):
    """Toy layers h = live * tanh(x A_l) in place of the recurrences; the carry rules in numpy float64 (residual_bwd_np,
    the statement of the backward kernel) against autograd through connect_step.  dx_raw is NaN at padded frames, as the
    dx product leaves them unwritten."""
    rng = np.random.RandomState(L)
    T, Bp, W = 6, 5, 4
    lens = np.array([6, 1, 0, 3, 5])
    live = (np.arange(T)[:, None] < lens[None, :])[:, :, None].astype(np.float64)
    A = [rng.randn(W, W) * 0.5 for _ in range(L)]
    m = [(rng.rand(T, Bp, W) < 0.8) / 0.8 for _ in range(L)]
    R = rng.randn(T, Bp, W)
    x0 = torch.tensor(rng.randn(T, Bp, W), requires_grad=True)
    At = [torch.tensor(a, requires_grad=True) for a in A]
    x, outs, S, xs, hs = x0, [], None, [], []
    for li in range(L):
        h = torch.tanh(x @ At[li]) * torch.tensor(live)
        xs.append(x.detach().numpy())
        hs.append(h.detach().numpy())
        o, S = res.connect_step(mode, li, h * torch.tensor(m[li]), outs[-1] if outs else None, S)
        outs.append(o)
        x = o
    (outs[-1] * torch.tensor(R)).sum().backward()

    dA = [None] * L

    def layer_bwd(li, dout):
        dpre = np.where(live > 0, dout * (1.0 - hs[li] ** 2), 0.0)
        dA[li] = np.einsum('tbi,tbj->ij', xs[li], dpre)
        dx = dpre @ A[li].T
        return np.where(live > 0, dx, np.nan)

    dx = layer_bwd(L - 1, m[L - 1] * R)            # the top layer as in the plain stack: its own mask on d_outputs
    carry = R.copy()
    for li in reversed(range(L - 1)):
        dout, carry = res.residual_bwd_np(dx, carry, lens, m[li], mode == 'dense', dtype=np.float64)
        assert np.isfinite(dout).all() and np.isfinite(carry).all()
        assert not (dout * (1 - live)).any() and not (carry * (1 - live)).any()
        dx = layer_bwd(li, dout)
    for li in range(L):
        assert np.abs(dA[li] - At[li].grad.numpy()).max() < 1e-12, li
    assert np.abs(np.nan_to_num(dx) - x0.grad.numpy()).max() < 1e-12


def test_stand_in_kernels_update_in_place_and_zero_the_padding(monkeypatch):
    res.install(monkeypatch)
    from tensorflow_end2end_speech_recognition_amd import ops
    rng = np.random.RandomState(0)
    T, Bp, W = 5, 4, 6
    lens = torch.tensor([5, 0, 1, 3], dtype=torch.int32)
    h, skip = torch.tensor(rng.randn(T, Bp, W).astype(np.float32)), torch.tensor(rng.randn(T, Bp, W).astype(np.float32))
    S = skip.clone()
    out, S2 = ops.residual_fwd(h, S, lens, (0.8, 3, 1 << 40), sum_out=S)
    assert S2 is S
    mk = _cpu_ops._dropout_mask((T, Bp, W), 0.8, 3, 1 << 40).numpy()
    want_o, want_s = res.residual_fwd_np(h.numpy(), skip.numpy(), lens.numpy(), mk)
    assert np.array_equal(out.numpy(), want_o) and np.array_equal(S.numpy(), want_s)
    assert not out[1:, 2].any() and not out[:, 1].any()
    dx, carry = h.clone(), skip.clone()
    d, c = ops.residual_bwd(dx, carry, lens, (0.8, 3, 1 << 40), dense=True, dout=dx, carry_out=carry)
    assert d is dx and c is carry
    want_d, want_c = res.residual_bwd_np(h.numpy(), skip.numpy(), lens.numpy(), mk, True)
    assert np.array_equal(dx.numpy(), want_d) and np.array_equal(carry.numpy(), want_c)


# ---------------------------------------------------------------- CTC
def _batch(rng, B, T, D, C):
    x = rng.randn(B, T, D).astype(np.float32)
    sl = rng.randint(max(2, T // 2), T + 1, size=B).astype(np.int32)
    sl[0] = T
    labs = []
    for b in range(B):
        x[b, sl[b]:] = 0
        labs.append([int(v) for v in rng.randint(0, C, size=max(1, int(sl[b]) // 2))])
    dense = np.full((B, max(len(l) for l in labs)), -1, dtype=np.int64)
    for b, l in enumerate(labs):
        dense[b, :len(l)] = l
    return x, sl, labs, dense


def _ctc(enc, D, H, L, C, **kw):
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    return CTC(encoder_type=enc, input_size=D, num_units=H, num_layers=L, num_classes=C, parameter_init=0.1,
               clip_grad_norm=0.05, clip_activation=50, dtype='f32', seed=3, device='cpu', **kw)


def _plain_cls(enc):
    from tensorflow_end2end_speech_recognition_amd.models.encoders.load_encoder import load
    return load(enc)


@pytest.mark.parametrize('keep', [1.0, 0.8])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('enc', ['blstm', 'lstm'])
def test_residual_ctc_model_host_logic(monkeypatch, enc, mode, keep):
    res.install(monkeypatch)
    from tensorflow_end2end_speech_recognition_amd.models.encoders.core import residual as R
    rng = np.random.RandomState(5)
    B, T, D, H, L, C = 5, 13, 6, 8, 4, 6                # B is padded to 16 utterances inside the encoder
    ndir = 2 if enc == 'blstm' else 1
    x, sl, labs, dense = _batch(rng, B, T, D, C)
    model = _ctc(enc, D, H, L, C, **KW[mode])
    plain = _ctc(enc, D, H, L, C)
    assert type(model.encoder) is R.load_residual(enc) and isinstance(model.encoder, _plain_cls(enc))
    assert model.encoder.dense == (mode == 'dense')
    # no new variables: names, order, shapes and initial values are the plain model's
    assert list(model.store.names) == list(plain.store.names)
    for name in plain.store.names:
        assert torch.equal(model.store[name], plain.store[name]), name
    sd = {n: v.numpy().copy() for n, v in model.store.state_dict().items()}
    for n in sd:
        if n.endswith('/bias') or n.endswith('/biases'):
            sd[n] = (rng.randn(*sd[n].shape) * 0.05).astype(np.float32)
    model.store.load_state_dict({n: torch.tensor(v) for n, v in sd.items()})
    masks = None
    if keep < 1.0:      # the stand-in generator's masks, drawn where the model draws them: first call, layer li
        masks = [_cpu_ops._dropout_mask((T, 16, ndir * H), keep, 3, (1 << 40) + (li << 32)).numpy()[:, :B]
                 for li in range(L)]
    ref = res.ctc_model_forward(sd, x, labs, sl, L, ndir, mode, cell_clip=50.0, masks=masks)
    loss, logits = model.compute_loss(x, dense, sl, keep_prob=keep)
    assert logits.shape == (T, B, C + 1)
    assert abs(loss.item() - ref['total_loss']) / abs(ref['total_loss']) < 1e-5
    assert np.abs(logits.numpy() - ref['logits']).max() < 1e-5
    enc_out = model.encoder._out_tm.numpy()
    for b in range(16):
        assert not enc_out[(int(sl[b]) if b < B else 0):, b].any()
    assert np.array_equal(model.encoder.seq_len_padded[:B].numpy(), sl)
    # every gradient; the hook fires once per layer, top layer first
    fired = []
    model.encoder.grad_ready_hook = lambda li, layer: fired.append((li, layer))
    opt = model._set_optimizer('sgd', 0.1)
    seen = set()
    for g, name in opt.compute_gradients(loss, model=model):
        r = ref['grads'][name]
        seen.add(name)
        err = np.abs(g.numpy() - r).max()
        assert err < 1e-4 * max(np.abs(r).max(), 1e-3) + 1e-7, (name, err, np.abs(r).max())
    assert seen == set(ref['grads'])
    assert [li for li, _ in fired] == list(reversed(range(L)))
    assert all(layer is model.encoder.layers[li] for li, layer in fired)
    model.encoder.grad_ready_hook = None
    if keep < 1.0:
        return
    # one full training step: per-variable clip, then the update
    before = {n: v.numpy().copy() for n, v in model.store.state_dict().items()}
    loss, _ = model.compute_loss(x, dense, sl, keep_prob=1.0)
    model.train(loss, 'momentum', 0.1)
    after = model.store.state_dict()
    for name, r in ref['grads'].items():
        want = before[name] - 0.1 * oopt.clip_by_norm(r, 0.05)
        assert np.abs(after[name].numpy() - want).max() < 1e-5, name
    # the final state is the cells' own: the statement's
    model.store.load_state_dict({n: torch.tensor(v) for n, v in sd.items()})
    out, final = model.encoder(torch.tensor(x), torch.tensor(sl), 1.0, False)
    assert np.abs(out.numpy() - ref['enc']).max() < 1e-5
    rf = ref['final']
    for i, st in enumerate(final):
        c_ref, h_ref = rf[i]
        assert np.abs(st.c.numpy() - c_ref.detach().numpy()).max() < 1e-5
        assert np.abs(st.h.numpy() - h_ref.detach().numpy()).max() < 1e-5


def test_caller_supplied_mask_tensors_keep_apply_mask(monkeypatch):
    """drop_masks= from a caller: the layer applies the tensor, the kernels run with keep = 1 -- same numbers as the
    descriptor path with the same multipliers."""
    ops = res.install(monkeypatch)
    from tensorflow_end2end_speech_recognition_amd.models.encoders.core.residual import ResidualBLSTMEncoder
    kw = dict(num_units=8, num_proj=None, num_layers=3, lstm_impl='LSTMBlockCell', use_peephole=True, parameter_init=0.1,
              clip_activation=50, seed=2)
    rng = np.random.RandomState(0)
    x = torch.tensor(rng.randn(3, 7, 6).astype(np.float32))
    sl = torch.tensor([7, 4, 1], dtype=torch.int32)
    dy = torch.tensor(rng.randn(7, 16, 16).astype(np.float32))
    got = []
    for tensors in (False, True):
        enc = ResidualBLSTMEncoder(dense=True, **kw)
        drops = []
        real = ops.residual_fwd
        monkeypatch.setattr(ops, 'residual_fwd', lambda h, s, l, drop=None, sum_out=None:
                            (drops.append(drop), real(h, s, l, drop, sum_out))[1])
        masks = [_cpu_ops._dropout_mask((7, 16, 16), 0.8, 9, (1 << 40) + (li << 32)) for li in range(3)]
        if tensors:
            out, _ = enc(x, sl, 0.8, True, drop_masks=masks)
            assert drops == [None, None]
        else:
            out, _ = enc(x, sl, 0.8, True, rng_state=(9, 1 << 40))
            assert drops == [(0.8, 9, (1 << 40) + (li << 32)) for li in (1, 2)]
        monkeypatch.setattr(ops, 'residual_fwd', real)
        dx = enc.backward(dy.clone(), need_input_grad=True)
        got.append((out.clone(), dx.clone(), {n: enc.store.g(n).clone() for n in enc.store.names}))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    for n in got[0][2]:
        assert torch.equal(got[0][2][n], got[1][2][n]), n


@pytest.mark.parametrize('enc', ['blstm', 'lstm'])
def test_flags_false_build_exactly_the_plain_model(monkeypatch, enc):
    res.install(monkeypatch)
    rng = np.random.RandomState(6)
    B, T, D, H, L, C = 4, 11, 6, 8, 2, 6
    x, sl, labs, dense = _batch(rng, B, T, D, C)
    plain = _ctc(enc, D, H, L, C)
    b, lb = plain.compute_loss(x, dense, sl, keep_prob=1.0)
    gb = {n: g.numpy().copy() for g, n in plain._set_optimizer('sgd', 0.1).compute_gradients(b, model=plain)}
    model = _ctc(enc, D, H, L, C, encoder_residual=False, encoder_dense_residual=False)
    assert type(model.encoder) is type(plain.encoder) is _plain_cls(enc)
    assert list(model.store.names) == list(plain.store.names)
    a, la = model.compute_loss(x, dense, sl, keep_prob=1.0)
    assert a.numpy().tobytes() == b.numpy().tobytes() and torch.equal(la, lb)
    for g, n in model._set_optimizer('sgd', 0.1).compute_gradients(a, model=model):
        assert g.numpy().tobytes() == gb[n].tobytes(), n
    # a flag with fewer than two layers: nothing to connect, the plain encoder
    for kw in KW.values():
        assert type(_ctc(enc, D, H, 1, C, **kw).encoder) is _plain_cls(enc)


@pytest.mark.parametrize('mode', MODES)
def test_checkpoints_interchange_with_the_plain_twin(monkeypatch, tmp_path, mode):
    res.install(monkeypatch)
    rng = np.random.RandomState(7)
    B, T, D, H, L, C = 3, 9, 6, 8, 3, 6
    x, sl, labs, dense = _batch(rng, B, T, D, C)
    model = _ctc('blstm', D, H, L, C, **KW[mode])
    plain = _ctc('blstm', D, H, L, C)
    sd = {n: torch.tensor(rng.randn(*v.shape).astype(np.float32) * 0.1) for n, v in plain.store.state_dict().items()}
    plain.store.load_state_dict(sd)
    path = str(tmp_path / 'plain.pt')
    torch.save(plain.store.state_dict(), path)
    model.store.load_state_dict(torch.load(path))                   # plain -> residual
    for n in sd:
        assert torch.equal(model.store[n], sd[n]), n
    loss, _ = model.compute_loss(x, dense, sl, keep_prob=1.0)
    model.train(loss, 'sgd', 0.1)
    path2 = str(tmp_path / 'res.pt')
    torch.save(model.store.state_dict(), path2)
    plain.store.load_state_dict(torch.load(path2))                  # residual -> plain
    for n in sd:
        assert torch.equal(plain.store[n], model.store[n]), n
    assert np.isfinite(plain.compute_loss(x, dense, sl, keep_prob=1.0)[0].item())


@pytest.mark.parametrize('mode', MODES)
def test_dropout_counters_are_indexed_by_the_layer(monkeypatch, mode):
    """Layer li draws its mask at rng_state[1] + li * 2^32, as the plain stack does: layer 1 through dropout_apply,
    the connected layers through the descriptor handed to residual_fwd, and the backward kernels get the same ones."""
    ops = res.install(monkeypatch)
    from tensorflow_end2end_speech_recognition_amd.models.encoders.core.residual import ResidualBLSTMEncoder
    applied, fwd, bwd = [], [], []
    r_apply, r_fwd, r_bwd = ops.dropout_apply, ops.residual_fwd, ops.residual_bwd
    monkeypatch.setattr(ops, 'dropout_apply', lambda t, keep, seed, offset:
                        (applied.append((seed, offset)), r_apply(t, keep, seed, offset))[1])
    monkeypatch.setattr(ops, 'residual_fwd', lambda h, s, l, drop=None, sum_out=None:
                        (fwd.append(drop), r_fwd(h, s, l, drop, sum_out))[1])
    monkeypatch.setattr(ops, 'residual_bwd', lambda dx, c, l, drop=None, dense=False, dout=None, carry_out=None:
                        (bwd.append((drop, dense)), r_bwd(dx, c, l, drop, dense, dout, carry_out))[1])
    enc = ResidualBLSTMEncoder(num_units=8, num_proj=None, num_layers=3, lstm_impl='LSTMBlockCell', use_peephole=True,
                               parameter_init=0.1, clip_activation=50, seed=2, dense=mode == 'dense')
    x = torch.tensor(np.random.RandomState(0).randn(2, 8, 6).astype(np.float32))
    enc(x, torch.tensor([8, 5], dtype=torch.int32), 0.8, True, rng_state=(9, 1 << 40))
    d = lambda li: (0.8, 9, (1 << 40) + li * (1 << 32))
    assert applied == [(9, 1 << 40)]                                # layer 1 only: no forward launch is added
    assert fwd == [d(1), d(2)]
    enc.backward(torch.zeros(8, 16, 16))
    # the top layer's own mask goes through dropout_apply (LSTMLayer.backward); the kernels take layers 2, 1
    assert applied == [(9, 1 << 40), (9, (1 << 40) + 2 * (1 << 32))]
    assert bwd == [(d(1), mode == 'dense'), (d(0), mode == 'dense')]


def test_value_errors(monkeypatch):
    res.install(monkeypatch)
    from tensorflow_end2end_speech_recognition_amd.models.ctc.multitask_ctc import MultitaskCTC
    from tensorflow_end2end_speech_recognition_amd.models.encoders.core.residual import check_residual, load_residual
    from tensorflow_end2end_speech_recognition_amd.models.encoders.load_encoder import load
    with pytest.raises(ValueError):
        _ctc('blstm', 6, 8, 3, 6, encoder_residual=True, encoder_dense_residual=True)
    with pytest.raises(ValueError):
        check_residual(True, True)
    assert check_residual(False, False) is None and check_residual(True, False) == 'residual'
    assert check_residual(False, True) == 'dense'
    for kw in KW.values():
        for enc in ('gru', 'bgru', 'vgg_blstm', 'vgg_lstm', 'cldnn_wang', 'cnn_zhang'):
            with pytest.raises(ValueError):
                _ctc(enc, 6, 8, 2, 6, **kw)
            with pytest.raises(ValueError):
                load_residual(enc)
        with pytest.raises(ValueError):
            _ctc('blstm', 6, 8, 2, 6, lstm_impl='LSTMCell', num_proj=4, **kw)
        with pytest.raises(ValueError):
            _ctc('blstm', 6, 8, 2, 6, subsample_list=[True, False], **kw)
        _ctc('blstm', 6, 8, 2, 6, subsample_list=[False, False], **kw)       # an all-false list is no subsampling
        with pytest.raises(ValueError):
            MultitaskCTC(encoder_type='multitask_blstm', input_size=6, num_units=8, num_layers_main=2, num_layers_sub=1,
                         num_classes_main=6, num_classes_sub=3, main_task_weight=0.5, device='cpu', **kw)
    # no registry key
    for key in ('residual_blstm', 'pyramid_blstm', 'vgg_wang'):
        with pytest.raises(ValueError):
            load(key)
    # the encoder refuses what only the plain stack's callers hand over
    model = _ctc('blstm', 6, 8, 2, 6, encoder_residual=True)
    with pytest.raises(ValueError):
        model.encoder.backward(torch.zeros(3, 16, 16), top_masked=True)
    model.encoder.defer_top_dropout = True
    assert model.encoder.defer_top_dropout is False


# ---------------------------------------------------------------- joint CTC / attention
def _att_batch(rng, B, T, D, C):
    x = rng.randn(B, T, D).astype(np.float32)
    sl = rng.randint(max(2, T // 2), T + 1, size=B).astype(np.int32)
    sl[0] = T
    lens = np.array([max(1, min(4, int(s) // 2)) for s in sl])
    sos, eos = C, C + 1
    labels = np.full((B, int(lens.max()) + 2), eos, dtype=np.int64)
    ctc_labels = np.full((B, int(lens.max())), -1, dtype=np.int64)
    for b in range(B):
        x[b, sl[b]:] = 0
        y = rng.randint(0, C, size=lens[b])
        labels[b, 0] = sos
        labels[b, 1:1 + lens[b]] = y
        ctc_labels[b, :lens[b]] = y
    return x, sl, labels, lens + 2, ctc_labels


def _mk_att(cls, att, D, H, L, U, A, Em, C, **kw):
    return cls(input_size=D, encoder_type='blstm', encoder_num_units=H, encoder_num_layers=L,
               encoder_num_proj=None, attention_type=att, attention_dim=A, decoder_type='lstm',
               decoder_num_units=U, decoder_num_layers=1, embedding_dim=Em, num_classes=C, sos_index=C,
               eos_index=C + 1, max_decode_length=8, parameter_init=0.1, clip_grad_norm=5.0,
               clip_activation_encoder=50, clip_activation_decoder=50, dtype='f32', seed=5, device='cpu', **kw)


@pytest.mark.parametrize('joint,att,mode', [(True, 'location', 'residual'), (True, 'bahdanau_content', 'dense'),
                                            (False, 'location', 'dense')])
def test_residual_attention_models_host_logic(monkeypatch, joint, att, mode):
    res.install(monkeypatch)
    from tensorflow_end2end_speech_recognition_amd.models.attention.attention_seq2seq import AttentionSeq2Seq
    from tensorflow_end2end_speech_recognition_amd.models.attention.joint_ctc_attention import JointCTCAttention
    from tensorflow_end2end_speech_recognition_amd.models.encoders.core.residual import ResidualBLSTMEncoder
    rng = np.random.RandomState(11)
    B, T, D, H, L, U, A, Em, C = 3, 11, 6, 8, 3, 12, 10, 4, 6
    x, sl, labels, lsl, ctc_labels = _att_batch(rng, B, T, D, C)
    cls, extra = (JointCTCAttention, dict(lambda_weight=0.5)) if joint else (AttentionSeq2Seq, {})
    model = _mk_att(cls, att, D, H, L, U, A, Em, C, **dict(extra, **KW[mode]))
    plain = _mk_att(cls, att, D, H, L, U, A, Em, C, **extra)
    assert type(model.encoder) is ResidualBLSTMEncoder and type(plain.encoder) is _plain_cls('blstm')
    assert type(_mk_att(cls, att, D, H, L, U, A, Em, C, encoder_residual=False, encoder_dense_residual=False,
                        **extra).encoder) is _plain_cls('blstm')
    assert list(model.store.names) == list(plain.store.names)
    sd = {n: v.numpy().copy() for n, v in model.store.state_dict().items()}
    res.patch_oracle_blstm_encoder(monkeypatch, mode)
    okw = dict(clip_enc=50.0, clip_dec=50.0)
    if joint:
        ctc_list = [[int(v) for v in row if v >= 0] for row in ctc_labels]
        ref = oatt.attention_model_forward(sd, x, labels, sl, lsl, L, att, ctc_labels=ctc_list, lambda_weight=0.5, **okw)
        loss, logits, ctc_logits, out_train, out_infer = model.compute_loss(x, labels, ctc_labels, sl, lsl, 1.0, 1.0, 1.0)
        assert np.abs(ctc_logits.numpy() - ref['ctc_logits']).max() < 1e-5
    else:
        ref = oatt.attention_model_forward(sd, x, labels, sl, lsl, L, att, **okw)
        loss, logits, out_train, out_infer = model.compute_loss(x, labels, sl, lsl, 1.0, 1.0, 1.0)
    assert abs(loss.item() - ref['total_loss']) / abs(ref['total_loss']) < 1e-5
    assert np.abs(out_train.attention_weights.numpy() - ref['alphas']).max() < 1e-5
    opt = model._set_optimizer('adam', 1e-3)
    seen = set()
    for g, name in opt.compute_gradients(loss, model=model):
        r = ref['grads'][name]
        seen.add(name)
        err = np.abs(g.numpy() - r).max()
        assert err < 1e-4 * max(np.abs(r).max(), 1e-3) + 1e-7, (name, err, np.abs(r).max())
    assert seen == set(ref['grads'])
    ref_ids = oatt.attention_model_infer(sd, x, sl, L, att, C, C + 1, 8, **okw)
    assert np.array_equal(model.infer(x, sl), ref_ids)
    with pytest.raises(ValueError):
        _mk_att(cls, att, D, H, L, U, A, Em, C, encoder_residual=True, encoder_dense_residual=True, **extra)
    with pytest.raises(ValueError):
        _mk_att(cls, att, D, H, L, U, A, Em, C, subsample_list=[True, False, False], **dict(extra, **KW[mode]))


# ---------------------------------------------------------------- the recipe
def test_timit_residual_recipe_on_cpu_stand_ins(monkeypatch, tmp_path):
    """examples/timit/config/ctc/blstm_ctc_phone61_dense_residual.yml through train_ctc.py and eval_ctc.py on a generated
    corpus; the other two recipe files parse and carry their keys."""
    import random
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    res.install(monkeypatch)
    from examples.timit.training import train_attention, train_ctc
    from examples.timit.evaluation import eval_ctc
    from tensorflow_end2end_speech_recognition_amd.models.encoders.core.residual import ResidualBLSTMEncoder
    cfgs = {}
    for rel in ('ctc/blstm_ctc_phone61_residual.yml', 'ctc/blstm_ctc_phone61_dense_residual.yml',
                'attention/blstm_attention_phone61_residual.yml'):
        with open(os.path.join(root, 'examples/timit/config', rel)) as f:
            cfgs[rel] = yaml.safe_load(f)
    assert cfgs['ctc/blstm_ctc_phone61_residual.yml']['param']['encoder_residual'] is True
    assert cfgs['ctc/blstm_ctc_phone61_residual.yml']['param']['encoder_dense_residual'] is False
    att = cfgs['attention/blstm_attention_phone61_residual.yml']['param']
    assert att['encoder_residual'] is True and att['attention_type'] == 'location'
    assert train_attention.run_name(att).endswith('_res')
    att.update(num_classes=61, device='cpu', dtype='f32', encoder_num_units=8, encoder_num_layers=2,
               decoder_num_units=8, attention_dim=8, embedding_dim=4, input_size=6)
    kw = train_attention.model_kwargs(att)
    assert kw['encoder_residual'] is True and kw['encoder_dense_residual'] is False
    from tensorflow_end2end_speech_recognition_amd.models.attention.attention_seq2seq import AttentionSeq2Seq
    assert type(AttentionSeq2Seq(**kw).encoder) is ResidualBLSTMEncoder
    cfg = cfgs['ctc/blstm_ctc_phone61_dense_residual.yml']
    assert cfg['param']['encoder_dense_residual'] is True and cfg['param']['num_layers'] == 5
    corpus = str(tmp_path / 'corpus')
    make_timit_like(corpus, np.random.RandomState(0))
    # the topology shrunk as the plain recipe test shrinks it
    cfg['param'].update(num_layers=3, input_size=6, num_units=8, batch_size=8, num_epoch=30, eval_start_epoch=1,
                        print_step=3, optimizer='adam', learning_rate=0.05, dropout=0.0, weight_decay=0, decay_start_epoch=2,
                        dtype='f32', device='cpu', dataset_root=corpus, sort_stop_epoch=2, not_improved_patient_epoch=100)
    cfg_path = str(tmp_path / 'cfg.yml')
    with open(cfg_path, 'w') as f:
        yaml.safe_dump(cfg, f)
    random.seed(0)
    built = train_ctc.build_model(dict(cfg['param']))
    assert type(built.encoder) is ResidualBLSTMEncoder and built.encoder.dense
    res_run = train_ctc.main(cfg_path, str(tmp_path / 'runs'))
    run = res_run['save_path']
    assert run.endswith(os.path.join('ctc', 'phone61', 'blstm_ctc_8_3_adam_lr0.05_dres'))
    assert len(res_run['ler_dev']) == 30 and res_run['checkpoints'] and res_run['ler_test'] is not None
    assert min(res_run['ler_dev']) < 0.9
    log = open(os.path.join(run, 'train.log')).read()
    assert '-----EPOCH:30' in log and 'PER:' in log
    per = eval_ctc.main([run, '--beam_width', '1', '--device', 'cpu'])      # rebuilt from the run's config.yml
    assert abs(per - res_run['ler_test']) < 1e-9


def test_timit_residual_ctc_and_attention_recipes_train_and_evaluate(monkeypatch, tmp_path):
    """blstm_ctc_phone61_residual.yml through train_ctc.py / eval_ctc.py and blstm_attention_phone61_residual.yml through
    train_joint_ctc_attention.py / eval_attention.py (one short run each, the topology shrunk): the evaluation scripts
    rebuild the residual model from the run's config.yml and score what the trained model object scores."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import test_host_logic as thl
    res.install(monkeypatch)
    from examples.timit.evaluation import eval_attention, eval_ctc
    from examples.timit.metrics.attention import do_eval_per
    from examples.timit.training import train_ctc, train_joint_ctc_attention as drv
    from examples.timit.training.train_attention import make_datasets
    from tensorflow_end2end_speech_recognition_amd.models.encoders.core.residual import ResidualBLSTMEncoder
    from tensorflow_end2end_speech_recognition_amd.utils.training.checkpoint import Saver
    corpus = str(tmp_path / 'corpus')
    thl._make_timit_like(corpus, np.random.RandomState(0), n_train=8, n_dev=2, n_test=3, multitask=False)
    cfg = thl._recipe_cfg(root, 'examples/timit/config/ctc/blstm_ctc_phone61_residual.yml', tmp_path, num_layers=2,
                          input_size=6, num_units=8, batch_size=8, num_epoch=2, eval_start_epoch=1, print_step=2,
                          optimizer='adam', learning_rate=0.02, weight_decay=0, decay_start_epoch=2, dtype='f32',
                          device='cpu', dataset_root=corpus, sort_stop_epoch=2)
    out = train_ctc.main(cfg, str(tmp_path / 'runs'))
    assert out['save_path'].endswith('_res') and type(out['model'].encoder) is ResidualBLSTMEncoder
    assert not out['model'].encoder.dense
    Saver().save(out['model'], os.path.join(out['save_path'], 'model.ckpt'), global_step=99)
    assert 0.0 <= eval_ctc.main([out['save_path'], '--beam_width', '1', '--device', 'cpu'])
    cfg = thl._recipe_cfg(root, 'examples/timit/config/attention/blstm_attention_phone61_residual.yml', tmp_path,
                          encoder_num_units=8, encoder_num_layers=2, attention_dim=6, decoder_num_units=8,
                          embedding_dim=4, max_decode_length=10, dropout_encoder=0.0, dropout_decoder=0.0,
                          dropout_embedding=0.0, input_size=6, batch_size=8, num_epoch=1, eval_start_epoch=1, print_step=2,
                          optimizer='adam', learning_rate=0.02, weight_decay=0, decay_start_epoch=2, dtype='f32',
                          device='cpu', dataset_root=corpus, sort_stop_epoch=2)
    out = drv.main(cfg, str(tmp_path / 'runs'))
    run, model = out['save_path'], out['model']
    assert '_res_' in os.path.basename(run) and type(model.encoder) is ResidualBLSTMEncoder
    Saver().save(model, os.path.join(run, 'model.ckpt'), global_step=99)
    map_dir = os.path.join(run, 'mapping_files')
    params = dict(label_type='phone61', splice=1, num_stack=1, num_skip=1, batch_size=8, num_epoch=1, sort_stop_epoch=1,
                  dataset_root=corpus)
    test_data = make_datasets(drv.Dataset, params, map_dir)[2]
    want = do_eval_per(None, None, None, model, test_data, 'phone61', is_test=True, eval_batch_size=1, map_dir=map_dir,
                       is_jointctcatt=True)
    got = eval_attention.main([run, '--device', 'cpu', '--joint'])
    assert abs(got - want) < 1e-9
