"""The H = 256 bf16 forward recurrence on clusters of 16 CUs x four waves x 4 units (lstm_fwd_cluster16_kernel) against the
8-CU x 4-wave x 8-unit form (lstm_fwd_cluster8_kernel<256, ..., 32>): the two accumulate the k-chunks of h W_h in the same
order with the same MFMA operand roles, so every value of a valid frame must be BIT-identical.  ASR_LSTM_DFLAGS bit 13 flips
between the two forms inside one process, whichever is the default."""
import functools

import numpy as np
import pytest
import torch

from oracle import lstm as olstm

pytestmark = pytest.mark.gpu

H = 256
FLIP = 8192          # ASR_LSTM_DFLAGS bit 13: the other one of the 16-CU / 8-CU forward forms
WRITE_THROUGH = 16   # bit 4: placement-independent write-through exchange


def _ops():
    from tensorflow_end2end_speech_recognition_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _weights(ndir):
    """Random packed W_h (any bf16 values are a valid image) and peepholes, made once per ndir."""
    g = torch.Generator(device='cpu').manual_seed(100 + ndir)
    whf = (torch.rand((ndir, 4 * H * H), generator=g) * 0.2 - 0.1).to(torch.bfloat16)
    peep = torch.rand((ndir, 3, H), generator=g) * 0.6 - 0.3
    return whf, peep


def _lens(kind, T, B):
    rng = np.random.RandomState(T * 31 + B)
    if kind == 'full':
        return np.full(B, T, dtype=np.int32)
    lens = rng.randint(1, T + 1, size=B).astype(np.int32)
    if kind == 'ragged1':
        lens[0], lens[5] = T, 1
    else:                                     # a row of length 0, the maximum in the last row of every tile
        lens = np.minimum(lens, max(T - 1, 1)).astype(np.int32)
        lens[2] = 0
        lens[15::16] = T
    return lens


def _run_both(cuda, T, B, ndir, lens, use_peep, clip, base_flags=0, scale=1.0):
    ops = _ops()
    from tensorflow_end2end_speech_recognition_amd._lib import ASR_BF16
    whf, peep = _weights(ndir)
    g = torch.Generator(device='cpu').manual_seed(T * 1000 + B * 10 + ndir)
    xproj = (torch.randn((T, B, ndir * 4 * H), generator=g) * scale).to(cuda)
    whf_d = whf.to(cuda)
    peep_d = peep.to(cuda) if use_peep else None
    sl = torch.tensor(lens, dtype=torch.int32, device=cuda)
    res = []
    try:
        for flags in (base_flags, base_flags | FLIP):
            ops.debug_set_lstm_flags(flags)
            gates, hout, cs, cf, hf = ops.lstm_fwd(xproj, whf_d, peep_d, sl, H, ndir, ASR_BF16, 1.0, clip)
            assert ops.check_async_errors(0) == 0
            res.append(dict(gates=gates.view(torch.int16).view(T, B, ndir * H, 4).cpu().numpy(),
                            hout=hout.view(torch.int16).cpu().numpy(), cs=cs.cpu().numpy(),
                            cf=cf.cpu().numpy(), hf=hf.cpu().numpy()))
    finally:
        ops.debug_set_lstm_flags(0)
    return res


def _assert_same(a, b, lens, T, B, clip):
    assert np.array_equal(a['hout'], b['hout'])
    assert np.array_equal(a['cf'], b['cf'])
    assert np.array_equal(a['hf'], b['hf'])
    valid = np.arange(T)[:, None] < np.asarray(lens)[None, :]          # [T, B]
    for r in (a, b):
        assert not r['hout'][~valid].any()                              # padded frames exactly zero
    assert np.array_equal(a['gates'][valid], b['gates'][valid])         # parked positions are unspecified
    assert np.array_equal(a['cs'][valid], b['cs'][valid])
    if valid.any():
        assert a['hout'][valid].any()
    if clip:
        cmax = np.abs(a['cs'][valid]).max()
        assert cmax == np.float32(clip)                                 # the clip is active


@pytest.mark.parametrize('clip', [0.0, 0.5])
@pytest.mark.parametrize('use_peep', [True, False])
@pytest.mark.parametrize('kind', ['full', 'ragged1', 'ragged0'])
@pytest.mark.parametrize('ndir', [1, 2])
@pytest.mark.parametrize('B', [16, 32])
@pytest.mark.parametrize('T', [1, 2, 3, 6, 7])
def test_fwd_cu16_same_bits_as_cu8(cuda, T, B, ndir, kind, use_peep, clip):
    lens = _lens(kind, T, B)
    a, b = _run_both(cuda, T, B, ndir, lens, use_peep, clip, scale=4.0 if clip else 1.0)
    _assert_same(a, b, lens, T, B, clip)


def test_fwd_cu16_same_bits_with_write_through_exchange(cuda):
    T, B, ndir = 7, 32, 2
    lens = _lens('ragged0', T, B)
    a, b = _run_both(cuda, T, B, ndir, lens, True, 0.0, base_flags=WRITE_THROUGH)
    _assert_same(a, b, lens, T, B, 0.0)


@pytest.mark.parametrize('flags', [0, FLIP])
def test_fwd_forms_against_the_oracle(cuda, flags):
    """Each form against oracle.lstm.layer_forward_np on the same bf16-rounded operands; the forward bounds of
    test_lstm_cluster_bf16_gradient_parity_headline_shapes (tests/test_gpu_ops.py)."""
    ops = _ops()
    from tensorflow_end2end_speech_recognition_amd._lib import ASR_BF16
    T, B, D, ndir = 7, 16, 24, 2
    rng = np.random.RandomState(11)
    lens = _lens('ragged1', T, B)
    x = olstm.bf16_round(rng.randn(B, T, D))
    for b in range(B):
        x[b, lens[b]:] = 0
    ps = [olstm.init_lstm_params(rng, D, H, init=0.1) for _ in range(ndir)]
    for p in ps:
        p['b'] = torch.tensor(rng.uniform(-0.1, 0.1, 4 * H))
    xd = ops.bt_to_tb(torch.tensor(x, dtype=torch.float32, device=cuda), ASR_BF16)
    xproj = torch.empty((T, B, ndir * 4 * H), dtype=torch.float32, device=cuda)
    whf = torch.empty((ndir, 4 * H * H), dtype=torch.bfloat16, device=cuda)
    for d, p in enumerate(ps):
        w = ops.lstm_prep_weights(torch.tensor(p['w'].numpy(), dtype=torch.float32, device=cuda),
                                  torch.tensor(p['b'].numpy(), dtype=torch.float32, device=cuda), D, H, ASR_BF16)
        ops.gemm(xd.view(T * B, D), w['wx_il'], bias=w['bias_il'], out=xproj.view(T * B, -1)[:, d * 4 * H:(d + 1) * 4 * H])
        whf[d].copy_(w['pf'])
    peep = torch.tensor(np.stack([np.stack([p['wci'].numpy(), p['wcf'].numpy(), p['wco'].numpy()]) for p in ps]),
                        dtype=torch.float32, device=cuda)
    sl = torch.tensor(lens, dtype=torch.int32, device=cuda)
    try:
        ops.debug_set_lstm_flags(flags)
        gates, hout, cs, cf, hf = ops.lstm_fwd(xproj, whf, peep, sl, H, ndir, ASR_BF16, 1.0, 50.0)
        assert ops.check_async_errors(0) == 0
    finally:
        ops.debug_set_lstm_flags(0)
    hout, cs, cf, hf = hout.float().cpu().numpy(), cs.cpu().numpy(), cf.cpu().numpy(), hf.cpu().numpy()
    gates = gates.float().view(T, B, ndir, H, 4).permute(2, 0, 1, 4, 3).contiguous().cpu().numpy()
    xt = np.ascontiguousarray(np.transpose(x, (1, 0, 2)))
    valid = np.arange(T)[:, None] < lens[None, :]
    for d in range(ndir):
        pn = {k: v.detach().numpy() for k, v in ps[d].items()}
        f = olstm.layer_forward_np(xt, lens, pn, d == 1, 1.0, 50.0, True, round_fn=olstm.bf16_round)
        s = slice(d * H, (d + 1) * H)
        e = np.abs(hout[:, :, s] - f['hout'])
        assert e.max() <= 2 ** -7 and e.mean() <= 2e-4, (e.max(), e.mean())
        assert np.abs(hout[:, :, s][~valid]).max() == 0
        ecs = np.abs(cs[:, :, s] - f['cs'])[valid]
        assert ecs.max() / max(1.0, np.abs(f['cs']).max()) <= 2e-2 and ecs.mean() <= 8e-4, (ecs.max(), ecs.mean())
        eg = np.abs(gates[d] - f['gates'])[valid]
        assert eg.max() <= 2 ** -6 and eg.mean() <= 3.5e-4, (eg.max(), eg.mean())
        assert np.abs(cf[d] - f['c_final']).max() <= 2e-2
        assert np.abs(hf[d] - f['h_final']).max() <= 5e-3
