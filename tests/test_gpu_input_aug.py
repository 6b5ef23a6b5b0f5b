"""On-device input augmentation (input_noise_std, freq_mask_*, time_mask_*: an extension) on the device: asr_input_augment
against the numpy statement (tests/_input_aug_oracle.py), and the models -- a step with augmentation must be the plain
twin's step on ops.input_augment(x, ..., seed + 11, k << 40), bit for bit.

Bars: the masks and every copied element are exact.  The noise has the bar tests/test_gpu_weight_noise.py derives for this
generator (1e-5 absolute on z, from the fp32 roundings of ln, sqrt, cos / sin at |z| <= 5.77) plus the fp32 rounding of
the sum, ulp(x) / std, in the form of its test_op_random_weights_views_and_paths."""
import functools

import numpy as np
import pytest
import torch

import _input_aug_oracle as iao
import _weight_noise_oracle as own

pytestmark = pytest.mark.gpu

BAR = 1e-5
STD = 0.05
MASK_VALUE = 0.25                  # not a value the data takes, and not the default
OFFSETS = [0, (3 << 40) + (2 << 32)]
SEED = 1234


def _bench_lens():
    rng = np.random.RandomState(0)
    lens = rng.randint(150, 746, size=16).astype(np.int32)
    lens[0] = 745
    return lens


# name -> (shape, n_ch, lengths, (number, width) of frequency masks, (number, width, ratio) of time masks)
CASES = {
    'small': ((3, 40, 12), 4, np.array([40, 17, 1], np.int32), (2, 3), (2, 10, 0.5)),
    'straddle': ((2, 9, 123), 41, np.array([9, 0], np.int32), (2, 6), (2, 4, 1.0)),      # T F % 4 = 3
    'ragged': ((5, 33, 123), 41, np.array([33, 32, 5, 2, 0], np.int32), (2, 6), (2, 10, 0.5)),
    'bench': ((16, 745, 123), 41, _bench_lens(), (2, 6), (2, 20, 0.2)),
}
SMALL = ['small', 'straddle', 'ragged']


def _ops():
    from tensorflow_end2end_speech_recognition_amd import ops
    return ops


def _bits(t):
    if torch.is_tensor(t):
        return t.detach().contiguous().view(torch.int32).cpu().numpy()
    return np.ascontiguousarray(t, dtype=np.float32).view(np.int32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _x(case):
    """Features with NaN in every padded frame and one -0.0 among the valid elements."""
    shape, _, lens, _, _ = CASES[case]
    x = np.random.RandomState(len(case)).randn(*shape).astype(np.float32)
    x[0, 0, 1] = -0.0
    for b, n in enumerate(lens):
        x[b, n:] = np.nan
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _cover(case, offset):
    """The statement's (valid, masked, z) of a case, computed once; asserts that the case is not vacuous."""
    shape, n_ch, lens, fm, tm = CASES[case]
    valid, masked, fd, td = iao.cover(shape, lens, n_ch, fm, tm, SEED, offset)
    assert fd[:, :, 0].max() >= 1 and td[:, :, 0].max() >= 1, 'no mask of width >= 1 on an axis: pick other draws'
    z = iao.noise(int(np.prod(shape)), SEED, offset).reshape(shape)
    for a in (valid, masked, z):
        a.setflags(write=False)
    return valid, masked, z


def _run(cuda, case, offset, lead=0, noise=False, masks=False):
    """One call on a device copy of the case's x placed `lead` elements into a larger buffer, into a NaN-prefilled y
    placed likewise.  -> (y, x on the device after the call)."""
    ops = _ops()
    shape, n_ch, lens, fm, tm = CASES[case]
    n = int(np.prod(shape))
    xbuf = torch.zeros(lead + n, dtype=torch.float32, device=cuda)
    ybuf = torch.full((lead + n,), float('nan'), dtype=torch.float32, device=cuda)
    xd, yd = xbuf[lead:].view(shape), ybuf[lead:].view(shape)
    xd.copy_(torch.from_numpy(_x(case).copy()))
    y = ops.input_augment(xd, torch.from_numpy(lens).to(cuda), n_ch, noise_std=STD if noise else 0.0,
                          freq_masks=fm if masks else (0, 0), time_masks=tm if masks else (0, 0, 1.0),
                          mask_value=MASK_VALUE, seed=SEED, offset=offset, out=yd)
    assert y.data_ptr() == yd.data_ptr()
    if lead:
        assert not xbuf[:lead].any() and bool(torch.isnan(ybuf[:lead]).all())
    return y, xd


def _noise_excess(y, x, z, where):
    """max over `where` of |(y - x) / std - z| - ulp(x) / std."""
    got = (y.astype(np.float64) - x) / float(np.float32(STD))
    with np.errstate(invalid='ignore'):
        err = np.abs(got - z) - own.ulp32(x) / STD
    return err[where].max()


# ---------------------------------------------------------------- the op
@pytest.mark.parametrize('lead', [0, 1])                      # 1: not 16-byte aligned, the element path
@pytest.mark.parametrize('offset', OFFSETS)
@pytest.mark.parametrize('case', SMALL)
def test_op_masks_only_is_the_statement_bit_for_bit(cuda, case, offset, lead):
    ops = _ops()
    shape, n_ch, lens, fm, tm = CASES[case]
    valid, masked, _ = _cover(case, offset)
    ops.reset_input_augment_counts(0)
    y, xd = _run(cuda, case, offset, lead=lead, masks=True)
    assert ops.input_augment_counts(0) == dict(calls=1, elements=int(np.prod(shape)), vec_calls=0 if lead else 1)
    want = iao.augment(_x(case), lens, n_ch, 0.0, fm, tm, MASK_VALUE, SEED, offset)
    assert _same(xd, _x(case))                                # the caller's tensor is never written
    assert _same(y, want)
    yh = y.cpu().numpy()
    assert masked.any() and (yh[masked] == np.float32(MASK_VALUE)).all()
    assert np.array_equal(_bits(yh)[~masked], _bits(_x(case))[~masked])       # -0.0 and the padded NaN as they are
    y2, _ = _run(cuda, case, offset, lead=lead, masks=True)
    assert _same(y, y2)                                       # two calls, the same bits


@pytest.mark.parametrize('lead', [0, 1])
@pytest.mark.parametrize('offset', OFFSETS)
@pytest.mark.parametrize('case', SMALL)
def test_op_noise_only_and_both(cuda, case, offset, lead):
    ops = _ops()
    shape = CASES[case][0]
    valid, masked, z = _cover(case, offset)
    valid = np.broadcast_to(valid, shape)
    x = _x(case)
    ops.reset_input_augment_counts(0)
    yn, xd = _run(cuda, case, offset, lead=lead, noise=True)
    assert ops.input_augment_counts(0) == dict(calls=1, elements=x.size, vec_calls=0 if lead else 1)
    assert _same(xd, x)
    ynh = yn.cpu().numpy()
    assert np.array_equal(_bits(ynh)[~valid], _bits(x)[~valid])       # padded frames: x's bits, NaN included
    err = _noise_excess(ynh, x, z, valid)
    print('%s offset %#x lead %d: noise only, max excess over ulp(x)/std = %.3g' % (case, offset, lead, err))
    assert err < BAR
    assert np.abs(ynh[valid] - x[valid]).max() > STD          # and there is noise
    # both: a masked element is exactly mask_value, every other one is as in noise only
    yb, xd = _run(cuda, case, offset, lead=lead, noise=True, masks=True)
    assert _same(xd, x)
    ybh = yb.cpu().numpy()
    assert masked.any() and (ybh[masked] == np.float32(MASK_VALUE)).all()
    assert np.array_equal(_bits(ybh)[~masked], _bits(ynh)[~masked])
    # the 16-byte and the element path, and a second call, write the same bits
    ref, _ = _run(cuda, case, offset, noise=True, masks=True)
    assert _same(yb, ref)


@pytest.mark.parametrize('case', SMALL)
def test_op_all_off_is_a_copy(cuda, case):
    ops = _ops()
    ops.reset_input_augment_counts(0)
    for lead in (0, 1):
        y, xd = _run(cuda, case, 0, lead=lead)
        assert _same(y, _x(case)) and _same(xd, _x(case))
    assert ops.input_augment_counts(0) == dict(calls=2, elements=2 * _x(case).size, vec_calls=0)


def test_op_bench_shard(cuda):
    """[16,745,123], the headline shard, once: noise and masks in one call against the statement."""
    ops = _ops()
    case, offset = 'bench', OFFSETS[1]
    shape, n_ch, lens, fm, tm = CASES[case]
    valid, masked, z = _cover(case, offset)
    valid = np.broadcast_to(valid, shape)
    x = _x(case)
    ops.reset_input_augment_counts(0)
    y, xd = _run(cuda, case, offset, noise=True, masks=True)
    assert ops.input_augment_counts(0) == dict(calls=1, elements=x.size, vec_calls=1)
    assert _same(xd, x)
    yh = y.cpu().numpy()
    assert masked.any() and (yh[masked] == np.float32(MASK_VALUE)).all()
    assert np.array_equal(_bits(yh)[~valid], _bits(x)[~valid])
    err = _noise_excess(yh, x, z, valid & ~masked)
    print('bench shard: max excess over ulp(x)/std = %.3g' % err)
    assert err < BAR


def test_op_argument_checks(cuda):
    ops = _ops()
    x = torch.zeros((2, 6, 12), device=cuda)
    sl = torch.tensor([6, 3], dtype=torch.int32, device=cuda)
    good = dict(n_ch=4, noise_std=0.1, freq_masks=(1, 2), time_masks=(1, 2, 1.0), mask_value=0.0)
    ops.input_augment(x, sl, **good)
    bad = [dict(n_ch=0), dict(n_ch=5), dict(n_ch=24), dict(freq_masks=(9, 2)), dict(freq_masks=(-1, 2)),
           dict(time_masks=(9, 2, 1.0)), dict(time_masks=(-1, 2, 1.0)), dict(freq_masks=(1, -1)),
           dict(time_masks=(1, -1, 1.0)), dict(time_masks=(1, 2, 1.5)), dict(time_masks=(1, 2, -0.1)),
           dict(time_masks=(1, 2, float('nan'))), dict(noise_std=-1e-9), dict(noise_std=float('inf')),
           dict(noise_std=float('nan')), dict(mask_value=float('inf')), dict(mask_value=float('nan'))]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.input_augment(x, sl, **dict(good, **kw))
    buf = torch.zeros(2 * 6 * 12 + 8, device=cuda)
    with pytest.raises(ValueError, match='overlaps'):
        ops.input_augment(buf[:144].view(2, 6, 12), sl, out=buf[8:152].view(2, 6, 12), **good)
    with pytest.raises(ValueError):
        ops.input_augment(x, sl[:1], **good)
    with pytest.raises(ValueError):
        ops.input_augment(x, sl, out=torch.zeros((2, 6, 8), device=cuda), **good)
    with pytest.raises(ValueError):
        ops.input_augment(x.double(), sl, **good)
    assert not x.any() and not buf.any()
    y = ops.input_augment(x[:0], sl[:0], **good)              # empty: nothing launched
    assert y.shape == (0, 6, 12)


# ---------------------------------------------------------------- models
B_, T_, D_, H_, L_, C_ = 3, 40, 12, 64, 2, 7
SL = np.array([T_, 1, 23], dtype=np.int32)                    # ragged, one utterance of a single frame
AUG = dict(input_noise_std=STD, freq_mask_num=2, freq_mask_width=3, time_mask_num=2, time_mask_width=10)
VGG_SPLICE = 5


def _features(D, seed):
    x = np.random.RandomState(seed).randn(B_, T_, D).astype(np.float32)
    for b in range(B_):
        x[b, SL[b]:] = 0
    return x


def _ctc_labels(C=C_):
    rng = np.random.RandomState(11)
    labs = [[int(v) for v in rng.randint(0, C, size=max(1, SL[b] // 4))] for b in range(B_)]
    dense = np.full((B_, max(len(l) for l in labs)), -1, dtype=np.int64)
    for b, l in enumerate(labs):
        dense[b, :len(l)] = l
    return dense


def _att_labels():
    rng = np.random.RandomState(3)
    lens = np.array([5, 1, 4])
    labels = np.full((B_, 7), C_ + 1, dtype=np.int64)
    ctc_labels = np.full((B_, 5), -1, dtype=np.int64)
    for b in range(B_):
        y = rng.randint(0, C_, size=lens[b])
        labels[b, 0] = C_
        labels[b, 1:1 + lens[b]] = y
        ctc_labels[b, :lens[b]] = y
    return labels, lens + 2, ctc_labels


def _family(which):
    """-> (mk(**keywords) -> model, run(model, x, **kw) -> the tuple compute_loss returns, x host features)."""
    from tensorflow_end2end_speech_recognition_amd.models.attention.attention_seq2seq import AttentionSeq2Seq
    from tensorflow_end2end_speech_recognition_amd.models.attention.joint_ctc_attention import JointCTCAttention
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    from tensorflow_end2end_speech_recognition_amd.models.ctc.multitask_ctc import MultitaskCTC
    ckw = dict(input_size=D_, num_units=H_, parameter_init=0.1, clip_grad_norm=5.0, clip_activation=50, device='cuda:0',
               seed=3)
    x = _features(D_, 11)
    if which in ('ctc_f32', 'ctc_bf16', 'ctc_vgg', 'ctc_wn'):
        dense = _ctc_labels()
        extra = dict(ctc_f32=dict(encoder_type='blstm', dtype='f32'), ctc_bf16=dict(encoder_type='blstm', dtype='bf16'),
                     ctc_vgg=dict(encoder_type='vgg_blstm', dtype='f32', splice=VGG_SPLICE),
                     ctc_wn=dict(encoder_type='blstm', dtype='f32', weight_noise_std=0.05))[which]
        if which == 'ctc_vgg':
            x = _features(D_ * VGG_SPLICE, 12)
        keep = 0.8 if which == 'ctc_bf16' else 1.0
        mk = lambda **kw: CTC(num_layers=L_, num_classes=C_, **dict(ckw, **extra), **kw)          # noqa: E731
        run = lambda m, xx, **k: m.compute_loss(xx, dense, SL, keep_prob=keep, **k)               # noqa: E731
    elif which == 'multitask':
        dense = _ctc_labels(9)
        dense_s = np.where(dense >= 0, dense % 4, -1)
        mk = lambda **kw: MultitaskCTC(encoder_type='multitask_blstm', num_layers_main=2, num_layers_sub=1,   # noqa: E731
                                       num_classes_main=9, num_classes_sub=4, main_task_weight=0.7, dtype='f32',
                                       **ckw, **kw)
        run = lambda m, xx, **k: m.compute_loss(xx, dense, dense_s, SL, keep_prob=1.0, **k)       # noqa: E731
    else:
        x = _features(D_, 3)
        labels, lsl, ctc_labels = _att_labels()
        akw = dict(input_size=D_, encoder_type='blstm', encoder_num_units=H_, encoder_num_layers=L_, encoder_num_proj=None,
                   attention_type='location', attention_dim=32, decoder_type='lstm', decoder_num_units=64,
                   decoder_num_layers=1, embedding_dim=8, num_classes=C_, sos_index=C_, eos_index=C_ + 1,
                   max_decode_length=12, parameter_init=0.1, clip_grad_norm=5.0, clip_activation_encoder=50,
                   clip_activation_decoder=50, seed=5, device='cuda:0')
        if which == 'attention':
            mk = lambda **kw: AttentionSeq2Seq(dtype='f32', **akw, **kw)                          # noqa: E731
            run = lambda m, xx, **k: m.compute_loss(xx, labels, SL, lsl, 0.9, 0.9, 0.9, **k)      # noqa: E731
        else:
            assert which == 'joint_bf16'
            mk = lambda **kw: JointCTCAttention(dtype='bf16', lambda_weight=0.5, **akw, **kw)     # noqa: E731
            run = lambda m, xx, **k: m.compute_loss(xx, labels, ctc_labels, SL, lsl, 0.9, 0.9, 0.9, **k)   # noqa: E731
    return mk, run, x


def _tensors(result):
    return [t for t in result if torch.is_tensor(t)]


def _twin_input(ops, m, x_dev, sl_dev, k):
    return ops.input_augment(x_dev, sl_dev, m.input_channels, noise_std=STD, freq_masks=(2, 3), time_masks=(2, 10, 1.0),
                             seed=m.seed + 11, offset=k << 40)


FAMILIES = ['ctc_f32', 'ctc_bf16', 'ctc_vgg', 'multitask', 'attention', 'joint_bf16', 'ctc_wn']


@pytest.mark.parametrize('which', FAMILIES)
def test_augmented_step_is_the_plain_step_on_the_augmented_inputs(cuda, which):
    ops = _ops()
    mk, run, x = _family(which)
    a, b = mk(**AUG), mk()
    assert a.input_channels == D_ // 3 and _same(a.store.flat, b.store.flat)
    x_dev = torch.from_numpy(x).to(cuda)
    sl_dev = torch.from_numpy(SL).to(cuda)
    ops.reset_input_augment_counts(0)
    ops.reset_ctc_head_counts(0)
    ops.reset_weight_noise_counts(0)
    for k in (1, 2):
        xa = _twin_input(ops, a, x_dev, sl_dev, k)
        xah = xa.cpu().numpy()
        assert (xah[x != 0] == 0).any() and np.abs(xah - x).max() > STD     # masks and noise are there
        assert not _same(xa, _twin_input(ops, a, x_dev, sl_dev, k + 1))     # and each step has its own
        calls = ops.input_augment_counts(0)['calls']
        ra = run(a, x_dev)
        assert ops.input_augment_counts(0)['calls'] == calls + 1 and a._augment_calls == k
        assert _same(x_dev, x)                                # the caller's tensor is untouched
        rb = run(b, xa)
        assert ops.input_augment_counts(0)['calls'] == calls + 1 and b._augment_calls == 0
        ta, tb = _tensors(ra), _tensors(rb)
        assert len(ta) == len(tb) >= 2
        for i, (u, v) in enumerate(zip(ta, tb)):
            assert _same(u, v), 'step %d: output %d of compute_loss' % (k, i)
        if which == 'ctc_wn':
            # the weight noise counts on its own: call k of both models, whatever the augmentation counted
            assert a._noise_calls == b._noise_calls == k and _same(a.store.flat, b.store.flat)
        before = a.store.flat.clone()
        a.train(ra[0], 'momentum', 0.05)
        b.train(rb[0], 'momentum', 0.05)
        # every gradient (the buffer train() leaves: clipped), and the weights after the update
        assert a.store.grad.abs().max().item() > 0
        assert _same(a.store.grad, b.store.grad), 'step %d: gradients' % k
        assert _same(a.store.flat, b.store.flat) and not _same(a.store.flat, before), 'step %d: weights' % k
    if which == 'ctc_bf16':                                   # the fused head (ctc_head_fwd -> ctc_loss_ex) in every forward
        assert ops.ctc_head_counts(0) == dict(head_fwd=4, loss_ex=4, loss=0)
    assert ops.weight_noise_counts(0)['calls'] == (4 if which == 'ctc_wn' else 0)


@pytest.mark.parametrize('which', ['ctc_bf16', 'attention'])
def test_keywords_off_and_dev_losses_are_the_model_without_them(cuda, which):
    ops = _ops()
    mk, run, x = _family(which)
    ops.reset_input_augment_counts(0)
    traces = []
    off = dict(input_noise_std=0.0, freq_mask_num=0, freq_mask_width=0, time_mask_num=0, time_mask_width=0)
    for kw in ({}, off, dict(freq_mask_num=2, time_mask_num=2), dict(freq_mask_width=3, time_mask_width=10)):
        m = mk(**kw)
        trace = []
        for _ in range(2):
            r = run(m, x)
            m.train(r[0], 'momentum', 0.01)
            trace.append([_bits(t).tobytes() for t in _tensors(r)] + [_bits(m.store.flat).tobytes()])
        assert m._augment_calls == 0
        traces.append(trace)
    assert all(t == traces[0] for t in traces[1:])
    # a dev loss of an augmenting model: the clean inputs
    a, b = mk(**AUG), mk()
    ra, rb = run(a, x, is_training=False), run(b, x, is_training=False)
    assert all(_same(u, v) for u, v in zip(_tensors(ra), _tensors(rb))) and a._augment_calls == 0
    assert ops.input_augment_counts(0) == dict(calls=0, elements=0, vec_calls=0)


def test_infer_sees_the_clean_inputs(cuda):
    ops = _ops()
    mk, run, x = _family('attention')
    a, b = mk(**AUG), mk()
    ops.reset_input_augment_counts(0)
    assert np.array_equal(a.infer(x, SL), b.infer(x, SL))
    assert ops.input_augment_counts(0)['calls'] == 0 and a._augment_calls == 0


def test_two_fresh_models_repeat_each_other(cuda):
    mk, run, x = _family('ctc_bf16')
    ends = []
    for _ in range(2):
        m = mk(**AUG)
        for _ in range(2):
            m.train(run(m, x)[0], 'adam', 0.01)
        ends.append(_bits(m.store.flat).tobytes())
    assert ends[0] == ends[1]
