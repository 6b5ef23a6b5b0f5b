"""The weight images of an LSTM stack in one launch (asr_lstm_prep_layers, ops.lstm_prep_layers) against the per-layer
launch (asr_lstm_prep_layer), byte for byte, and the encoder's cache of them: kept while the variables are what they
were built from (ParamStore.image_key), rebuilt once -- one grouped launch -- after every kind of write, and a model
with the cache computes the bits of a model without it (encoder.weight_images = False: the images per call and layer).

Everything here is an equality of bits: the images are conversions of single fp32 values, so no order of evaluation can
move them, and the cache changes which launch writes an image and when, never its contents."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
TAIL = 256                         # sentinel bytes behind every image


def _ops():
    from tensorflow_end2end_speech_recognition_amd import ops
    return ops


def _dt(name):
    from tensorflow_end2end_speech_recognition_amd._lib import ASR_BF16, ASR_F32
    return ASR_BF16 if name == 'bf16' else ASR_F32


def _ints(t):
    """The bits of a contiguous fp32 / bf16 tensor as an integer tensor."""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _stack(cuda, layers, H, ndir, din0, peep, seed):
    """Variables of `layers` stacked layers: per layer a list over directions of (kernel, bias, 3 peepholes or None)."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g).to(cuda)      # noqa: E731
    out, din = [], din0
    for _ in range(layers):
        rows = []
        for _d in range(ndir):
            rows.append(tuple([mk(din + H, 4 * H), mk(4 * H)] + ([mk(H), mk(H), mk(H)] if peep else [None, None, None])))
        out.append((rows, din))
        din = ndir * H
    return out


def _guarded(like):
    """A tensor of like's shape and dtype at the head of a sentinel-filled buffer -> (view, whole buffer as bytes)."""
    nbytes = like.numel() * like.element_size()
    buf = torch.full((nbytes + TAIL,), SENTINEL, dtype=torch.uint8, device=like.device)
    return buf[:nbytes].view(like.dtype).view(like.shape), buf


# the smallest case first: one layer, H = 64, one direction
@pytest.mark.parametrize('dtype', ['bf16', 'f32'])
@pytest.mark.parametrize('peep', [False, True])
@pytest.mark.parametrize('ndir', [1, 2])
@pytest.mark.parametrize('H', [64, 256, 320])
def test_grouped_launch_writes_the_bytes_of_the_per_layer_launches(cuda, H, ndir, peep, dtype):
    ops = _ops()
    dt = _dt(dtype)
    for layers in (1, 2, 3):
        for din0, ldk0 in ((39, 64), (120, 128)):
            stack = _stack(cuda, layers, H, ndir, din0, peep, seed=H + 7 * layers + din0)
            specs = [dict(variables=rows, din=din, H=H, dtype=dt, ldk=ldk0 if li == 0 else None)
                     for li, (rows, din) in enumerate(stack)]
            want = [ops.lstm_prep_layer(sp['variables'], sp['din'], H, dt, ldk=sp['ldk']) for sp in specs]
            outs, bufs = [], []
            for w in want:
                o, b = {}, {}
                for k, t in w.items():
                    o[k], b[k] = _guarded(t) if t is not None else (None, None)
                outs.append(o)
                bufs.append(b)
            ops.reset_prep_counts(0)
            got = ops.lstm_prep_layers(specs, out=outs)
            assert ops.prep_counts(0) == dict(grouped=1, per_layer=0)
            tag = 'layers %d din %d' % (layers, din0)
            for li, (w, o, b) in enumerate(zip(want, got, bufs)):
                assert o is outs[li]
                for k, t in w.items():
                    if t is None:
                        assert o[k] is None
                        continue
                    assert torch.equal(_ints(o[k]), _ints(t)), '%s: image %s of layer %d' % (tag, k, li)
                    nbytes = t.numel() * t.element_size()
                    assert bool((b[k][nbytes:] == SENTINEL).all()), '%s: bytes behind %s of layer %d' % (tag, k, li)
                assert (w['peep'] is None) == (not peep)
            # the zero padding of the bottom layer's wxT up to ldk (the sentinel is no zero)
            assert not _ints(got[0]['wxT'][:, din0:]).any()
            assert got[0]['wxT'].shape == (ndir * 4 * H, ldk0)
            # without out: fresh tensors, the same bytes
            fresh = ops.lstm_prep_layers(specs)
            for w, f in zip(want, fresh):
                assert all((f[k] is None) if t is None else torch.equal(_ints(f[k]), _ints(t)) for k, t in w.items())


def test_front_end_checks(cuda):
    ops = _ops()
    (rows, din), = _stack(cuda, 1, 64, 1, 39, False, seed=1)
    sp = dict(variables=rows, din=din, H=64, dtype=_dt('bf16'), ldk=64)
    assert ops.lstm_prep_layers([]) == []
    with pytest.raises(ValueError):
        ops.lstm_prep_layers([sp], out=[])
    with pytest.raises(ValueError):
        ops.lstm_prep_layers([sp, dict(sp, dtype=_dt('f32'))])
    good = ops.lstm_prep_layers([sp])[0]
    with pytest.raises(ValueError):
        ops.lstm_prep_layers([sp], out=[dict(good, wxT=good['wxT'][:, :32])])      # wrong shape, not contiguous
    with pytest.raises(ValueError):
        ops.lstm_prep_layers([dict(sp, din=40)])
    ops.reset_prep_counts(0)
    with pytest.raises(Exception, match='multiple of 64'):                          # refused by the library: nothing runs
        bad = tuple([torch.zeros(39 + 32, 128, device=cuda), torch.zeros(128, device=cuda), None, None, None])
        ops.lstm_prep_layers([sp, dict(variables=[bad], din=39, H=32, dtype=_dt('bf16'))])
    assert ops.prep_counts(0) == dict(grouped=0, per_layer=0)


# ---------------------------------------------------------------- the encoder's cache
B_, T_, D_, H_, L_, C_ = 16, 7, 12, 64, 2, 7
SL = np.array([7, 1, 5, 7, 3, 2, 6, 7, 4, 1, 7, 5, 3, 6, 2, 7], dtype=np.int32)


def _batch():
    rng = np.random.RandomState(11)
    x = rng.randn(B_, T_, D_).astype(np.float32)
    labs = []
    for b in range(B_):
        x[b, SL[b]:] = 0
        labs.append([int(v) for v in rng.randint(0, C_, size=max(1, SL[b] // 3))])
    dense = np.full((B_, max(len(l) for l in labs)), -1, dtype=np.int64)
    for b, l in enumerate(labs):
        dense[b, :len(l)] = l
    return x, dense


def _model(cache=True, **kw):
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    m = CTC(encoder_type='blstm', input_size=D_, num_units=H_, num_layers=L_, num_classes=C_, parameter_init=0.1,
            clip_grad_norm=5.0, clip_activation=50, dtype='bf16', device='cuda:0', seed=3, **kw)
    assert m.encoder.weight_images is True                      # the default of a process without the switch
    m.encoder.weight_images = bool(cache)
    return m


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy().tobytes()


def _run(m, keep=1.0, **kw):
    x, dense = _batch()
    loss, logits = m.compute_loss(x, dense, SL, keep_prob=keep, **kw)
    return loss, (_bits(loss.reshape(1)), _bits(logits))


def test_second_call_reuses_the_images(cuda):
    ops = _ops()
    m = _model()
    ops.reset_prep_counts(0)
    _, first = _run(m)
    assert ops.prep_counts(0) == dict(grouped=1, per_layer=0)
    imgs = m.encoder._images
    _, second = _run(m)
    assert ops.prep_counts(0) == dict(grouped=1, per_layer=0)
    assert m.encoder._images is imgs and second == first
    _, dev = _run(m, is_training=False)                          # a dev pass and a decode-style call: still the same images
    assert ops.prep_counts(0) == dict(grouped=1, per_layer=0)
    # the model without the cache: one launch per layer and call, the same bits
    off = _model(cache=False)
    ops.reset_prep_counts(0)
    assert _run(off)[1] == first and _run(off)[1] == first
    assert ops.prep_counts(0) == dict(grouped=0, per_layer=2 * L_)
    assert _run(off, is_training=False)[1] == dev


def _fake_broadcast(monkeypatch, ops):
    """multi_gpu.broadcast_parameters as a rank that receives: the collective writes store.flat from outside torch's
    version counter (here: a native in-place kernel), and mark_dirty is all that tells."""
    from tensorflow_end2end_speech_recognition_amd.utils.training import multi_gpu
    monkeypatch.setattr(multi_gpu, 'is_distributed', lambda: True)
    monkeypatch.setattr(multi_gpu.dist, 'broadcast', lambda t, src=0: ops.scale_(t, 0.75))
    return multi_gpu


WRITERS = ['optimizer', 'load_state_dict', 'flat_copy', 'view_write', 'perturb_restore', 'broadcast']


@pytest.mark.parametrize('writer', WRITERS)
def test_every_writer_makes_the_images_stale(cuda, monkeypatch, writer):
    ops = _ops()
    a, off = _model(), _model(cache=False)
    loss, before = _run(a)

    def check(what):
        """a's next forward: exactly one grouped launch, and the bits of the model without the cache at a's weights."""
        off.store.flat.copy_(a.store.flat)
        off.store.mark_dirty()
        want = _run(off)[1]
        ops.reset_prep_counts(0)
        got = _run(a)[1]
        assert ops.prep_counts(0) == dict(grouped=1, per_layer=0), what
        assert got == want, what
        ops.reset_prep_counts(0)
        assert _run(a)[1] == want and ops.prep_counts(0) == dict(grouped=0, per_layer=0), what
        return got

    if writer == 'optimizer':
        a.train(loss, 'sgd', 0.5)
    elif writer == 'load_state_dict':
        a.store.load_state_dict({k: v * 0.5 for k, v in a.store.state_dict().items()})
    elif writer == 'flat_copy':
        a.store.flat.copy_(a.store.flat * 1.5)
    elif writer == 'view_write':
        name = [n for n in a.store.names if n.endswith('fw/lstm_cell/kernel')][-1]      # the top layer's
        a.store[name].mul_(-1.0)
    elif writer == 'perturb_restore':
        clean = a.store.flat.clone()
        a.store.perturb(0.05, 9, 1 << 40)
        noisy = check('after perturb')
        assert noisy != before
        a.store.restore()
        assert torch.equal(a.store.flat, clean)
        assert check('after restore') == before
        return
    else:
        version = a.store.flat._version
        _fake_broadcast(monkeypatch, ops).broadcast_parameters(a.store)
        assert a.store.flat._version == version                 # only the epoch can tell
    assert check(writer) != before


@pytest.mark.parametrize('noise', [0.0, 0.05])
def test_training_with_and_without_the_cache_is_bit_identical(cuda, noise):
    ops = _ops()
    ends = []
    for cache in (True, False):
        m = _model(cache=cache, **(dict(weight_noise_std=noise) if noise else {}))
        ops.reset_prep_counts(0)
        trace = []
        for _ in range(3):
            loss, bits = _run(m, keep=0.8)
            m.train(loss, 'rmsprop', 1e-3)
            trace.append(bits)
        # with noise a step builds the images of the perturbed weights; the restore makes them stale for the next one
        assert ops.prep_counts(0) == (dict(grouped=3, per_layer=0) if cache else dict(grouped=0, per_layer=3 * L_))
        ends.append((trace, _bits(m.store.flat)))
    assert ends[0] == ends[1]
    assert len(set(ends[0][0])) == 3                             # the steps differ: the weights moved
