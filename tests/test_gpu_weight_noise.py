"""Gaussian weight noise (weight_noise_std, an extension) on the device: asr_weight_noise_perturb against the float64
statement (tests/_weight_noise_oracle.py), and the models -- a noisy step must be the plain model's step at the perturbed
weights, bit for bit, with the update on the clean weights.

The op's bar, 1e-5 absolute on z, is derived, not measured: at |z| <= 5.77 the fp32 roundings of ln u_a (1 ulp of up to
16.6: 1.9e-6, halved twice on the way through -2 ln and the square root: 3.3e-7), of the square root (2.4e-7), of cos / sin
(2 ulp of 1 times r: 1.4e-6) and of the product (2.4e-7) stay near 4e-6; a float32 emulation on the host gives 1.4e-6."""
import functools

import numpy as np
import pytest
import torch

import _weight_noise_oracle as own

pytestmark = pytest.mark.gpu

BAR = 1e-5
SIGMA = 0.05                       # far above every parity bar: a path that ignored the noise fails
OFFSETS = [0, (3 << 40) + (2 << 32)]
STRIDE_N = 4 * (2048 * 256) + 4 * 1000 + 3      # more groups than the capped grid has lanes: the grid-stride loop wraps
SIZES = [1, 3, 4, 5, 63, 1023, 4096, 4096 + 16 * 3 + 2]
SEED = 1234


def _ops():
    from tensorflow_end2end_speech_recognition_amd import ops
    return ops


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _z(n, offset):
    z = own.z(n, SEED, offset)
    z.setflags(write=False)
    return z


def _perturb(cuda, w_host, std, offset, lead=0):
    """One call on a device copy of w_host placed `lead` elements into a larger buffer; backup prefilled with NaN.
    Returns (w after, backup)."""
    ops = _ops()
    n = len(w_host)
    buf = torch.zeros(lead + n, dtype=torch.float32, device=cuda)
    w = buf[lead:]
    w.copy_(torch.from_numpy(w_host))
    backup = torch.full((n,), float('nan'), dtype=torch.float32, device=cuda)
    ops.weight_noise_perturb(w, backup, std, SEED, offset)
    if lead:
        assert not buf[:lead].any()
    return w, backup


# ---------------------------------------------------------------- the op
@pytest.mark.parametrize('offset', OFFSETS)
@pytest.mark.parametrize('n', SIZES + [STRIDE_N])
def test_op_zero_weights_give_the_statement(cuda, n, offset):
    ops = _ops()
    ops.reset_weight_noise_counts(0)
    w0 = np.zeros(n, dtype=np.float32)
    out, backup = _perturb(cuda, w0, 1.0, offset)
    assert ops.weight_noise_counts(0) == dict(calls=1, elements=n, vec_calls=1)
    assert np.array_equal(_bits(backup), w0.view(np.int32))
    err = np.abs(out.cpu().numpy().astype(np.float64) - _z(n, offset)).max()
    print('n %d offset %#x: max |z_device - z| = %.3g' % (n, offset, err))
    assert err < BAR
    assert np.abs(out.cpu().numpy()).max() <= own.Z_MAX
    out2, _ = _perturb(cuda, w0, 1.0, offset)
    assert _same(out, out2)                                   # two calls, the same bits


@pytest.mark.parametrize('lead', [0, 16, 1])                  # 1: not 16-byte aligned, the element-by-element kernel
@pytest.mark.parametrize('offset', OFFSETS)
@pytest.mark.parametrize('n', SIZES)
def test_op_random_weights_views_and_paths(cuda, n, offset, lead):
    ops = _ops()
    rng = np.random.RandomState(n + lead)
    w0 = (rng.randn(n) * 0.1).astype(np.float32)
    ops.reset_weight_noise_counts(0)
    out, backup = _perturb(cuda, w0, SIGMA, offset, lead=lead)
    assert ops.weight_noise_counts(0) == dict(calls=1, elements=n, vec_calls=0 if lead == 1 else 1)
    assert np.array_equal(_bits(backup), w0.view(np.int32))   # the original bits over the NaN prefill
    got = (out.cpu().numpy().astype(np.float64) - w0) / float(np.float32(SIGMA))
    err = np.abs(got - _z(n, offset)) - own.ulp32(w0) / SIGMA
    print('n %d lead %d: max excess over ulp(w)/std = %.3g' % (n, lead, err.max()))
    assert err.max() < BAR
    # the aligned and the unaligned kernel, and a second call, write the same bits
    ref, _ = _perturb(cuda, w0, SIGMA, offset)
    assert _same(out, ref)
    # std = 0 leaves w bit for bit (a -0 included) and still takes the backup
    w0z = w0.copy()
    w0z[0] = -0.0
    same, backup = _perturb(cuda, w0z, 0.0, offset, lead=lead)
    assert np.array_equal(_bits(same), w0z.view(np.int32)) and np.array_equal(_bits(backup), w0z.view(np.int32))


@pytest.mark.parametrize('offset', OFFSETS)
@pytest.mark.parametrize('a,b', [(0, 4), (4, 7), (1024, 3003), (4144, 4146), (2048, 4146)])
def test_op_slice_equals_the_whole_buffer_call(cuda, a, b, offset):
    n = SIZES[-1]
    w0 = (np.random.RandomState(7).randn(n) * 0.1).astype(np.float32)
    whole, _ = _perturb(cuda, w0, SIGMA, offset)
    part, backup = _perturb(cuda, w0[a:b].copy(), SIGMA, offset + a // 4, lead=16)
    assert _same(part, whole[a:b]) and np.array_equal(_bits(backup), w0[a:b].view(np.int32))


def test_op_argument_checks(cuda):
    ops = _ops()
    w = torch.zeros(64, device=cuda)
    for bad in (-1e-9, float('inf'), float('nan')):
        with pytest.raises(ValueError):
            ops.weight_noise_perturb(w, torch.zeros(64, device=cuda), bad, 0, 0)
    with pytest.raises(ValueError):
        ops.weight_noise_perturb(w, torch.zeros(60, device=cuda), 0.1, 0, 0)
    with pytest.raises(Exception, match='overlaps'):
        ops.weight_noise_perturb(w[:32], w[16:48], 0.1, 0, 0)
    assert not w.any()
    ops.weight_noise_perturb(w[:0], w[:0], 0.1, 0, 0)         # empty: nothing launched


# ---------------------------------------------------------------- models
B_, T_, D_, H_, L_, C_ = 3, 40, 12, 64, 2, 7
SL = np.array([T_, 1, 23], dtype=np.int32)                    # ragged, one utterance of a single frame


def _ctc_batch(C=C_):
    rng = np.random.RandomState(11)
    x = rng.randn(B_, T_, D_).astype(np.float32)
    labs = []
    for b in range(B_):
        x[b, SL[b]:] = 0
        labs.append([int(v) for v in rng.randint(0, C, size=max(1, SL[b] // 4))])
    dense = np.full((B_, max(len(l) for l in labs)), -1, dtype=np.int64)
    for b, l in enumerate(labs):
        dense[b, :len(l)] = l
    return x, dense


def _att_batch():
    rng = np.random.RandomState(3)
    x = rng.randn(B_, T_, D_).astype(np.float32)
    lens = np.array([5, 1, 4])
    labels = np.full((B_, 7), C_ + 1, dtype=np.int64)
    ctc_labels = np.full((B_, 5), -1, dtype=np.int64)
    for b in range(B_):
        x[b, SL[b]:] = 0
        y = rng.randint(0, C_, size=lens[b])
        labels[b, 0] = C_
        labels[b, 1:1 + lens[b]] = y
        ctc_labels[b, :lens[b]] = y
    return x, labels, lens + 2, ctc_labels


def _family(which):
    """-> (mk(**noise keywords) -> model, run(model, **kw) -> the tuple compute_loss returns)."""
    from tensorflow_end2end_speech_recognition_amd.models.attention.attention_seq2seq import AttentionSeq2Seq
    from tensorflow_end2end_speech_recognition_amd.models.attention.joint_ctc_attention import JointCTCAttention
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    from tensorflow_end2end_speech_recognition_amd.models.ctc.multitask_ctc import MultitaskCTC
    ckw = dict(input_size=D_, num_units=H_, parameter_init=0.1, clip_grad_norm=5.0, clip_activation=50, device='cuda:0',
               seed=3)
    if which in ('ctc_f32', 'ctc_bf16', 'ctc_lstmp'):
        x, dense = _ctc_batch()
        extra = dict(ctc_f32=dict(encoder_type='blstm', dtype='f32'), ctc_bf16=dict(encoder_type='blstm', dtype='bf16'),
                     ctc_lstmp=dict(encoder_type='lstm', dtype='f32', lstm_impl='LSTMCell', num_proj=32))[which]
        keep = 0.8 if which == 'ctc_bf16' else 1.0
        mk = lambda **kw: CTC(num_layers=L_, num_classes=C_, **dict(ckw, **extra), **kw)          # noqa: E731
        run = lambda m, **k: m.compute_loss(x, dense, SL, keep_prob=keep, **k)                    # noqa: E731
    elif which == 'multitask':
        x, dense = _ctc_batch(9)
        dense_s = np.where(dense >= 0, dense % 4, -1)
        mk = lambda **kw: MultitaskCTC(encoder_type='multitask_blstm', num_layers_main=2, num_layers_sub=1,   # noqa: E731
                                       num_classes_main=9, num_classes_sub=4, main_task_weight=0.7, dtype='f32',
                                       **ckw, **kw)
        run = lambda m, **k: m.compute_loss(x, dense, dense_s, SL, keep_prob=1.0, **k)            # noqa: E731
    else:
        x, labels, lsl, ctc_labels = _att_batch()
        akw = dict(input_size=D_, encoder_type='blstm', encoder_num_units=H_, encoder_num_layers=L_, encoder_num_proj=None,
                   attention_type='location', attention_dim=32, decoder_type='lstm', decoder_num_units=64,
                   decoder_num_layers=1, embedding_dim=8, num_classes=C_, sos_index=C_, eos_index=C_ + 1,
                   max_decode_length=12, parameter_init=0.1, clip_grad_norm=5.0, clip_activation_encoder=50,
                   clip_activation_decoder=50, seed=5, device='cuda:0')
        if which == 'attention':
            mk = lambda **kw: AttentionSeq2Seq(dtype='f32', **akw, **kw)                          # noqa: E731
            run = lambda m, **k: m.compute_loss(x, labels, SL, lsl, 0.9, 0.9, 0.9, **k)           # noqa: E731
        else:
            assert which == 'joint_bf16'
            mk = lambda **kw: JointCTCAttention(dtype='bf16', lambda_weight=0.5, **akw, **kw)     # noqa: E731
            run = lambda m, **k: m.compute_loss(x, labels, ctc_labels, SL, lsl, 0.9, 0.9, 0.9, **k)   # noqa: E731
    return mk, run


def _tensors(result):
    return [t for t in result if torch.is_tensor(t)]


def _twin_forward(a, b, run):
    """A's training forward, then B's at A's perturbed weights (padding included); asserts equal bits.  -> (ra, rb)."""
    ra = run(a)
    assert a.store.perturbed
    b.store.flat.copy_(a.store.flat)
    b.store.mark_dirty()
    rb = run(b)
    ta, tb = _tensors(ra), _tensors(rb)
    assert len(ta) == len(tb) >= 2
    for i, (u, v) in enumerate(zip(ta, tb)):
        assert _same(u, v), 'output %d of compute_loss' % i
    return ra, rb


FAMILIES = ['ctc_f32', 'ctc_bf16', 'ctc_lstmp', 'multitask', 'attention', 'joint_bf16']


@pytest.mark.parametrize('which', FAMILIES)
def test_noisy_step_is_the_plain_step_at_the_perturbed_weights(cuda, which):
    ops = _ops()
    mk, run = _family(which)
    a, b = mk(weight_noise_std=SIGMA), mk()
    clean = a.store.flat.clone()
    assert _same(clean, b.store.flat)
    ops.reset_weight_noise_counts(0)
    ops.reset_ctc_head_counts(0)
    ra, rb = _twin_forward(a, b, run)
    assert ops.weight_noise_counts(0) == dict(calls=1, elements=a.store.total, vec_calls=1)
    if which == 'ctc_bf16':                                   # the fused head (ctc_head_fwd -> ctc_loss_ex), once per model
        assert ops.ctc_head_counts(0) == dict(head_fwd=2, loss_ex=2, loss=0)
    assert not _same(a.store.flat, clean) and _same(a.store.clean, clean)
    opt_a, opt_b = a._set_optimizer('sgd', 0.05), b._set_optimizer('sgd', 0.05)
    opt_a.compute_gradients(ra[0], model=a)
    opt_b.compute_gradients(rb[0], model=b)
    assert a.store.grad.abs().max().item() > 0
    assert _same(a.store.grad, b.store.grad)
    assert not a.store.perturbed and _same(a.store.flat, clean)      # the clean weights, bit for bit
    # a whole train() step: the update of the CLEAN weights with the gradients of the perturbed ones
    b.store.flat.copy_(clean)
    b.store.mark_dirty()
    ra, rb = _twin_forward(a, b, run)
    opt_b.compute_gradients(rb[0], model=b)
    b._clip_gradients(None)
    a.train(ra[0], 'sgd', 0.05)
    want = clean.clone()
    ops.optimizer_step(opt_b.opt_id, want, b.store.grad, None, None, 0.05, 1)
    assert _same(a.store.flat, want) and not _same(want, clean) and not a.store.perturbed
    assert ops.weight_noise_counts(0)['calls'] == 2


@pytest.mark.parametrize('which', ['ctc_f32', 'joint_bf16'])
def test_noise_identity_per_step(cuda, which):
    mk, run = _family(which)
    a = mk(weight_noise_std=SIGMA)
    n = a.store.total
    deltas = []
    for k in (1, 2):
        clean = a.store.flat.clone()
        ra = run(a)
        noisy = a.store.flat.clone()
        a.train(ra[0], 'sgd', 0.05)
        w = clean.cpu().numpy()
        got = (noisy.cpu().numpy().astype(np.float64) - w) / float(np.float32(SIGMA))
        err = np.abs(got - own.z(n, a.seed + 7, k << 40)) - own.ulp32(w) / SIGMA
        print('step %d: max excess %.3g' % (k, err.max()))
        assert err.max() < BAR
        deltas.append(got)
    assert np.abs(deltas[0] - deltas[1]).max() > 1.0


def test_weight_decay_reads_the_clean_weights(cuda):
    ops = _ops()
    mk, run = _family('ctc_f32')
    wd = 1e-3
    a, a0, plain = mk(weight_noise_std=SIGMA, weight_decay=wd), mk(weight_noise_std=SIGMA), mk(weight_decay=wd)
    clean = a.store.flat.clone()
    la, la0 = run(a)[0], run(a0)[0]
    assert a.store.perturbed and _same(a.ctc_losses, a0.ctc_losses)
    # the loss is the CTC term of the perturbed weights plus the l2 of the model without noise, bits and all
    l2p = torch.zeros((), device=cuda)
    ops.weight_decay(None, plain.store.flat, plain.store.plan, plain.store.decay_mask, wd, l2_out=l2p)
    l2n = torch.zeros((), device=cuda)
    ops.weight_decay(None, a.store.flat, a.store.plan, a.store.decay_mask, wd, l2_out=l2n)
    assert l2p.item() > 0 and not _same(l2p.reshape(1), l2n.reshape(1))
    assert _same(la.reshape(1), (a.ctc_losses.mean() + l2p).reshape(1))
    assert _same(la0.reshape(1), a0.ctc_losses.mean().reshape(1))
    sd, sdp = a.store.state_dict(), plain.store.state_dict()
    assert all(_same(sd[k], sdp[k]) for k in sdp)             # state_dict: the clean weights while perturbed
    # the gradient differs from the wd = 0 run by wd * w_clean on the decayed variables (wd * sigma * z would be ~5e-5,
    # hundreds of fp32 spacings of these gradients)
    a._set_optimizer('sgd', 0.1).compute_gradients(la, model=a)
    a0._set_optimizer('sgd', 0.1).compute_gradients(la0, model=a0)
    mask = np.zeros(a.store.total, dtype=np.float32)
    for name in a.store.names:
        if 'bias' not in name.lower():
            v = a.store.views[name]
            mask[v.storage_offset():v.storage_offset() + v.numel()] = 1.0
    g, g0, w = a.store.grad.cpu().numpy(), a0.store.grad.cpu().numpy(), clean.cpu().numpy()
    want = g0.astype(np.float64) + wd * w.astype(np.float64) * mask
    assert np.abs(g - want).max() <= 2 * np.spacing(np.float32(np.abs(want).max()))


@pytest.mark.parametrize('which', ['ctc_bf16', 'attention'])
def test_sigma_zero_is_the_model_without_the_keyword(cuda, which):
    ops = _ops()
    mk, run = _family(which)
    ops.reset_weight_noise_counts(0)
    traces = []
    for kw in ({}, dict(weight_noise_std=0.0)):
        m = mk(**kw)
        trace = []
        for _ in range(2):
            r = run(m)
            m.train(r[0], 'momentum', 0.01)
            trace.append([_bits(t).tobytes() for t in _tensors(r)] + [_bits(m.store.flat).tobytes()])
        assert m.store._backup is None
        traces.append(trace)
    assert traces[0] == traces[1]
    assert ops.weight_noise_counts(0) == dict(calls=0, elements=0, vec_calls=0)


@pytest.mark.parametrize('which,use', [('ctc_f32', 'dev'), ('attention', 'infer'), ('attention', 'dev')])
def test_other_use_between_forward_and_train_restores_and_drops_the_tape(cuda, which, use):
    mk, run = _family(which)
    a, plain = mk(weight_noise_std=SIGMA), mk()
    clean = a.store.flat.clone()
    x = _att_batch()[0]
    want = plain.infer(x, SL) if use == 'infer' else run(plain, is_training=False)[0]
    ra = run(a)
    assert a.store.perturbed
    got = a.infer(x, SL) if use == 'infer' else run(a, is_training=False)[0]
    assert np.array_equal(got, want) if use == 'infer' else _same(got.reshape(1), want.reshape(1))   # no noise seen
    assert not a.store.perturbed and _same(a.store.flat, clean)
    with pytest.raises(RuntimeError, match='needs a preceding compute_loss'):
        a.train(ra[0], 'sgd', 0.05)
    assert _same(a.store.flat, clean)
    ra = run(a)                                               # and the model trains on
    a.train(ra[0], 'sgd', 0.05)
    assert not a.store.perturbed and not _same(a.store.flat, clean)


def test_two_fresh_models_repeat_each_other(cuda):
    mk, run = _family('ctc_bf16')
    ends = []
    for _ in range(2):
        m = mk(weight_noise_std=SIGMA)
        for _ in range(2):
            m.train(run(m)[0], 'adam', 0.01)
        ends.append(_bits(m.store.flat).tobytes())
    assert ends[0] == ends[1]
