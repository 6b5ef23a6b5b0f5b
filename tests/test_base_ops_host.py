"""The statements of tests/_base_ops.py held to facts from outside the project (torch's CPU conversions and pooling,
unfold / fold, the Random123 known answer), and the case lists of tests/test_gpu_base_ops.py held to what their comments
claim.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _base_ops as base

KAT = [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]       # Random123 kat_vectors, philox4x32-10, counter 0, key 0


def _bf16_tensor(bits_u16):
    return torch.from_numpy(np.ascontiguousarray(bits_u16).view(np.int16)).view(torch.bfloat16)


# ---------------------------------------------------------------- bf16
def test_bf16_rne_is_torchs_conversion_on_the_structured_set():
    bits = base.cast_patterns()
    assert bits.size == 6 * 65536
    nan = base.f32_is_nan(bits)
    assert int(nan.sum()) == 1534 and int((~nan).sum()) == 391682
    got = base.bf16_rne(bits)
    ref = torch.from_numpy(bits.view(np.int32)).view(torch.float32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert int((got[~nan] != ref[~nan]).sum()) == 0
    assert base.bf16_is_nan(got[nan]).all()
    # the facts the device test leans on: overflow of the largest finite values, ties to even, signed zeros
    assert [int(v) for v in base.bf16_rne(np.array([0x7F7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0xFF7F8000], np.uint32))] == \
        [0x7F80, 0x7F80, 0x7F7F, 0xFF80]
    assert [int(v) for v in base.bf16_rne(np.array([0x3F808000, 0x3F818000, 0x3F808001, 0x80000000, 0x00008000, 0x00018000],
                                                   np.uint32))] == [0x3F80, 0x3F82, 0x3F81, 0x8000, 0x0000, 0x0002]


def test_bf16_widen_is_torchs_float():
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    ref = _bf16_tensor(bits).float().view(torch.int32).numpy().view(np.uint32)
    assert np.array_equal(base.bf16_widen(bits), ref)
    assert int(base.bf16_is_nan(bits).sum()) == 254


# ---------------------------------------------------------------- dropout mask
@pytest.mark.parametrize('keep', [0.5, 0.7, 0.9, 1.0])
def test_dropout_mask_first_block_follows_from_the_known_answer(keep):
    u = [(w >> 8) / 2.0 ** 24 for w in KAT]                   # 0.399, 0.881, 0.736, 0.605
    inv = np.float32(1) / np.float32(keep)
    want = np.array([inv if v < float(np.float32(keep)) else 0 for v in u], dtype=np.float32)
    got = base.dropout_mask(4, keep, 0, 0)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if keep == 0.5:
        assert got.tolist() == [2.0, 0.0, 0.0, 0.0]


def test_dropout_mask_chunks_are_slices():
    seed, off = (7 << 32) + 11, (5 << 32) + 17
    whole = base.dropout_mask(1003, 0.8, seed, off)
    parts = [base.dropout_mask(400, 0.8, seed, off), base.dropout_mask(200, 0.8, seed, off + 100),
             base.dropout_mask(403, 0.8, seed, off + 150)]
    assert np.array_equal(np.concatenate(parts), whole)
    assert np.array_equal(base.dropout_mask(3, 0.8, seed, off), whole[:3])
    assert not np.array_equal(base.dropout_mask(64, 0.8, seed, off), base.dropout_mask(64, 0.8, seed + (1 << 32), off))
    assert not np.array_equal(base.dropout_mask(64, 0.8, seed, off), base.dropout_mask(64, 0.8, seed, off + (1 << 32)))


def test_dropout_mask_cases_can_tell_a_dropped_high_counter_word():
    _, sizes, keep, seed, off = [c for c in base.DROPOUT_MASK_CASES if c[0] == 'counter-carry'][0]
    n = sizes[0]
    assert off == 2 ** 32 - 2 and n == 16
    full = base.dropout_mask(n, keep, seed, off)
    low_only = np.concatenate([base.dropout_mask(4, keep, seed, (off + i) & 0xFFFFFFFF) for i in range(n // 4)])
    assert np.array_equal(full[:8], low_only[:8])             # blocks 2^32 - 2 and 2^32 - 1 have no high word yet
    assert not np.array_equal(full[8:12], low_only[8:12]) or not np.array_equal(full[12:], low_only[12:])
    assert not np.array_equal(full, low_only)
    for name in ('high-words', 'offset-2^50'):
        _, sizes, keep, seed, off = [c for c in base.DROPOUT_MASK_CASES if c[0] == name][0]
        m = (sizes[0] + 3) // 4
        low_only = np.concatenate([base.dropout_mask(4, keep, seed, (off + i) & 0xFFFFFFFF) for i in range(min(m, 64))])
        assert not np.array_equal(base.dropout_mask(4 * min(m, 64), keep, seed, off), low_only), name


# ---------------------------------------------------------------- pooling
def _torch_pool(x_nhwc64):
    x = torch.from_numpy(x_nhwc64).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = F.max_pool2d(x, kernel_size=2, stride=2, ceil_mode=True)
    return x, y


@pytest.mark.parametrize('W', [1, 2, 3, 4])
@pytest.mark.parametrize('H', [1, 2, 5, 6])
def test_maxpool_values_and_gradient_are_torchs(H, W):
    rng = np.random.RandomState(100 * H + W)
    x = rng.permutation(3 * H * W * 5).reshape(3, H, W, 5).astype(np.float64) - 20.0         # tie-free, both signs
    val, arg = base.maxpool2x2_fwd(x)
    xt, yt = _torch_pool(x)
    assert val.shape == (3, (H + 1) // 2, (W + 1) // 2, 5) and arg.dtype == np.uint8
    assert np.array_equal(val, yt.detach().permute(0, 2, 3, 1).numpy())
    dout = rng.randn(*val.shape).astype(np.float32)
    yt.backward(torch.from_numpy(dout.astype(np.float64)).permute(0, 3, 1, 2))
    din = base.maxpool2x2_bwd(dout, arg, H, W)
    assert din.dtype == np.float32
    assert np.array_equal(din.astype(np.float64), xt.grad.permute(0, 2, 3, 1).numpy())
    # every argmax names a cell inside the image
    hh = 2 * np.arange(val.shape[1])[None, :, None, None] + (arg >> 1)
    ww = 2 * np.arange(val.shape[2])[None, None, :, None] + (arg & 1)
    assert (hh < H).all() and (ww < W).all()


def _one_window(cells, H=2, W=2):
    """cells: the H x W values of one window in row-major order -> (value, argmax)."""
    x = np.array(cells, dtype=np.float32).reshape(1, H, W, 1)
    v, a = base.maxpool2x2_fwd(x)
    assert v.shape == (1, 1, 1, 1)
    return float(v[0, 0, 0, 0]), int(a[0, 0, 0, 0])


def test_maxpool_argmax_on_hand_built_windows():
    assert _one_window([0, 0, 0, 0]) == (0.0, 0)                       # all equal: the first cell
    assert _one_window([-3, -3, -3, -3]) == (-3.0, 0)
    for k in range(4):                                                 # the maximum in each of the four cells
        cells = [1.0, 2.0, 3.0, 4.0]
        cells[k] = 9.0
        assert _one_window(cells) == (9.0, k)
    assert _one_window([1, 5, 5, 0]) == (5.0, 1)                       # two equal maxima: the earlier one
    assert _one_window([0, 1, 7, 7]) == (7.0, 2)
    assert _one_window([7, 1, 0, 7]) == (7.0, 0)
    assert _one_window([0, 0, 0, 2]) == (2.0, 3)
    assert _one_window([-0.0, 0.0, 0.0, 0.0]) == (0.0, 0)              # -0.0 and +0.0 compare equal: still the first
    assert _one_window([2, 6], H=2, W=1) == (6.0, 2)                   # odd right edge: only cells 0 and 2 exist
    assert _one_window([6, 2], H=2, W=1) == (6.0, 0)
    assert _one_window([4, 4], H=2, W=1) == (4.0, 0)
    assert _one_window([2, 6], H=1, W=2) == (6.0, 1)                   # odd bottom edge: only cells 0 and 1 exist
    assert _one_window([-5, -6], H=1, W=2) == (-5.0, 0)
    assert _one_window([-8], H=1, W=1) == (-8.0, 0)                    # the corner of an odd x odd image: cell 0 alone
    # a tie sends the whole gradient to the first maximum and nothing to the second
    x = np.array([1, 5, 5, 0], dtype=np.float32).reshape(1, 2, 2, 1)
    _, a = base.maxpool2x2_fwd(x)
    assert base.maxpool2x2_bwd(np.full((1, 1, 1, 1), 3.0, np.float32), a, 2, 2).reshape(-1).tolist() == [0, 3, 0, 0]


# ---------------------------------------------------------------- im2col / col2im
@pytest.mark.parametrize('shape', [(2, 5, 3, 3), (1, 1, 1, 1), (2, 4, 6, 2)])
def test_im2col_is_unfold_and_col2im_is_fold(shape):
    N, H, W, Cin = shape
    rng = np.random.RandomState(5)
    x = rng.randn(*shape)
    cols = F.unfold(torch.from_numpy(x).permute(0, 3, 1, 2), kernel_size=3, padding=1)       # [N, Cin * 9, H W], (ci, tap)
    want = cols.view(N, Cin, 9, H * W).permute(0, 3, 2, 1).reshape(N * H * W, 9 * Cin).numpy()
    assert np.array_equal(base.im2col3x3(x), want)
    ldp = 9 * Cin + 5
    padded = base.im2col3x3(x, ldp=ldp, fill=-7.0)
    assert np.array_equal(padded[:, :9 * Cin], want) and (padded[:, 9 * Cin:] == -7.0).all()
    dp = rng.randn(N * H * W, ldp)
    folded = F.fold(torch.from_numpy(dp[:, :9 * Cin].copy()).view(N, H * W, 9, Cin).permute(0, 3, 2, 1)
                    .reshape(N, Cin * 9, H * W), output_size=(H, W), kernel_size=3, padding=1)
    din, mag = base.col2im3x3(dp, N, H, W, Cin)
    assert np.allclose(din, folded.permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-13)
    assert (mag >= np.abs(din) - 1e-13).all()
    # adjoint of each other: <im2col(x), dp> == <x, col2im(dp)>
    assert abs((want * dp[:, :9 * Cin]).sum() - (x * din).sum()) < 1e-10


# ---------------------------------------------------------------- the case lists
def test_dropout_cases_keep_and_drop():
    names = [c[0] for c in base.DROPOUT_MASK_CASES]
    assert len(set(names)) == len(names)
    for name, sizes, keep, seed, off in base.DROPOUT_MASK_CASES:
        m = base.dropout_mask(max(sizes), keep, seed, off)
        inv = np.float32(1) / np.float32(keep)
        assert set(np.unique(m).tolist()) <= {0.0, float(inv)}, name
        if keep == 1.0:
            assert (m == 1.0).all(), name
        else:
            assert (m == 0).any() and (m == inv).any(), name
    for keep, seed, off in base.ELEMENTWISE_DROPS:
        for n in [n for n in base.ELEMENTWISE_N if n >= 4]:
            m = base.dropout_mask(n, keep, seed, off)
            assert (m == 0).any() or n < 16
            assert (m != 0).any()
    assert float(np.float32(1) / np.float32(0.9)) != 1 / 0.9          # the `1/keep inexact` case is inexact


def test_grid_stride_cases_exceed_their_caps():
    assert base.GRID_FOR_CAP == 2048 * 256 and base.GRIDV_CAP == 4096 * 256
    for name, sizes, _, _, _ in base.DROPOUT_MASK_CASES:
        if name in base.DROPOUT_STRIDE_CASES:
            assert (max(sizes) + 3) // 4 > base.GRID_FOR_CAP
    assert set(base.DROPOUT_STRIDE_CASES) <= {c[0] for c in base.DROPOUT_MASK_CASES}
    assert base.CAST_REPEATS * base.cast_patterns().size > base.GRID_FOR_CAP          # cast_from_f32: grid_for(n)
    assert max(base.ELEMENTWISE_N) > base.GRID_FOR_CAP                                 # apply_mask: grid_for(n)
    assert (base.ELEMENTWISE_STRIDE_N + 3) // 4 > base.GRID_FOR_CAP                    # dropout_apply: grid_for(n / 4)
    assert base.ELEMENTWISE_STRIDE_N > base.GRIDV_CAP                                  # relu_bwd(_scaled): gridv(n)
    assert base.ELEMENTWISE_STRIDE_N % 4 == 3
    stride = {c[0]: c for c in base.POOL_CASES if c[0].startswith('stride')}
    assert set(stride) == {'stride-scalar', 'stride-vec'}
    _, shape, _, _, mis = stride['stride-scalar']
    assert (shape[3] % 4 != 0 or mis) and base.pool_work_items(shape, vec=False) > base.GRIDV_CAP
    _, shape, _, _, mis = stride['stride-vec']
    assert shape[3] % 4 == 0 and not mis and base.pool_work_items(shape, vec=True) > base.GRIDV_CAP
    assert int(np.prod(shape)) > base.GRIDV_CAP                                        # maxpool_bwd_kernel: gridv(N H W C)


def test_pool_cases_are_what_they_say():
    names = [c[0] for c in base.POOL_CASES]
    assert len(set(names)) == len(names)
    for name, shape, dtypes, kind, mis in base.POOL_CASES:
        assert set(dtypes) <= {'f32', 'bf16'} and kind in ('normal', 'ties', 'negative')
        if name.startswith('vec') or name == 'stride-vec':
            assert shape[3] % 4 == 0 and not mis, name
        if name.startswith('scalar') or name.endswith('scalar'):
            assert shape[3] % 4 != 0 or mis, name
        if mis:
            assert shape[3] % 4 == 0, name                             # so that the alignment alone picks the kernel
        if np.prod(shape) > 1 << 20:
            continue                                                   # the stride cases: checked on the device
        x = base.pool_input(name, shape, kind)
        assert x.dtype == np.float32 and x.shape == shape
        assert np.array_equal(base.bf16_values(base.bf16_rne(base.f32_bits(x))), x), name       # exact in bf16
        if kind == 'ties':
            assert base.tied_window_fraction(x) >= base.POOL_TIE_FRACTION, name
            assert 0.3 <= float((x == 0).mean()) <= 0.7 and (x >= 0).all(), name
            best, _ = base.maxpool2x2_fwd(x)
            assert (best > 0).mean() > 0.3, name                       # ties among positive maxima too, not only zeros
        if kind == 'negative':
            assert (x < 0).all(), name
        if kind == 'normal' and x.size >= 64:
            assert (x < 0).any() and (x > 0).any(), name


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_misaligned_views_are_misaligned(dtype):
    cases = [shape for _, shape, _, _, mis in base.POOL_CASES if mis] + [(n,) for n in base.ELEMENTWISE_N] + [(1000,)]
    assert len(cases) > len(base.ELEMENTWISE_N) + 1
    for shape in cases:
        vals = np.arange(int(np.prod(shape)), dtype=np.float32).reshape(shape) % 64
        t = base.as_tensor(vals, dtype, 'cpu', misaligned=True)
        assert t.is_contiguous() and tuple(t.shape) == shape and t.data_ptr() % 16 != 0
        assert np.array_equal(t.float().numpy(), vals)
        a = base.as_tensor(vals, dtype, 'cpu')
        assert a.is_contiguous() and a.data_ptr() % 16 == 0


def test_activation_values_have_every_sign():
    for n in base.ELEMENTWISE_N + [base.ELEMENTWISE_STRIDE_N]:
        act, dout = base.elementwise_inputs(n)
        assert act.dtype == np.float32 and dout.dtype == np.float32 and act.shape == (n,) == dout.shape
        assert np.array_equal(base.bf16_values(base.bf16_rne(base.f32_bits(act))), act)          # exact in bf16
        bits = base.f32_bits(act)
        if n >= 4:
            for share in ((bits == 0).mean(), (bits == 0x80000000).mean(), (act < 0).mean(), (act > 0).mean()):
                assert share >= 0.10, n
            assert (dout < 0).any() and (dout > 0).any()
        assert not np.array_equal(base.bf16_values(base.bf16_rne(base.f32_bits(dout))), dout) or n < 4
