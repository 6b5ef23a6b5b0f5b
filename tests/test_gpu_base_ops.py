"""The base elementwise and pooling ops on the device against the plain statements of tests/_base_ops.py: the dropout
mask, the casts, apply_mask / dropout_apply / relu_bwd / relu_bwd_scaled, 2x2 pooling, im2col3x3 / col2im3x3, tanh and
the row softmax.  The fused kernels are tested as "equal to these ops, bit for bit"; here the ops themselves are held to
something: bit for bit where the operation is exact or a single rounding, within a derived bound otherwise.

The cases and the kernel branch each is there for are listed in tests/_base_ops.py; tests/test_base_ops_host.py holds
the statements to torch's CPU results and the Random123 known answer, and the case lists to their comments."""
import functools

import numpy as np
import pytest
import torch

import _base_ops as base

pytestmark = pytest.mark.gpu

DT = {'f32': torch.float32, 'bf16': torch.bfloat16}
EPS = 2.0 ** -24


def _ops():
    from tensorflow_end2end_speech_recognition_amd import ops
    return ops


def _bits(t):
    """Device tensor -> numpy bit patterns (uint32 for float32, uint16 for bf16, uint8 as it is)."""
    t = t.detach().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32).cpu().numpy().view(np.uint32)
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    assert t.dtype == torch.uint8
    return t.cpu().numpy()


def _from_bits(bits, cuda):
    """numpy uint32 / uint16 bit patterns -> float32 / bf16 device tensor with exactly those bits."""
    if bits.dtype == np.uint32:
        return torch.from_numpy(bits.view(np.int32)).to(cuda).view(torch.float32)
    return torch.from_numpy(bits.view(np.int16)).to(cuda).view(torch.bfloat16)


def _first_diff(got, want):
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    return 'no difference' if not bad.size else '%d differ, first at %d: got 0x%x want 0x%x' % (
        bad.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


def _assert_bits(got_tensor, want_bits):
    got = _bits(got_tensor)
    assert got.dtype == want_bits.dtype and got.shape == want_bits.shape
    assert np.array_equal(got, want_bits), _first_diff(got, want_bits)


def _frozen(a):
    a.setflags(write=False)
    return a


# ================================================================ 1. dropout mask
@functools.lru_cache(maxsize=None)
def _mask(n, keep, seed, offset):
    return _frozen(base.dropout_mask(n, keep, seed, offset))


@pytest.mark.parametrize('name,n', [(c[0], n) for c in base.DROPOUT_MASK_CASES for n in c[1]])
def test_dropout_mask_is_the_statement(cuda, name, n):
    _, _, keep, seed, offset = [c for c in base.DROPOUT_MASK_CASES if c[0] == name][0]
    got = _ops().dropout_mask((n,), keep, seed, offset, cuda)
    _assert_bits(got, base.f32_bits(_mask(n, keep, seed, offset)))


# ================================================================ 2. casts
def test_cast_to_f32_widens_every_bf16_pattern(cuda):
    ops = _ops()
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    got = _bits(ops.cast_to_f32(_from_bits(bits, cuda)))
    nan = base.bf16_is_nan(bits)
    assert np.array_equal(got[~nan], base.bf16_widen(bits)[~nan]), _first_diff(got[~nan], base.bf16_widen(bits)[~nan])
    assert base.f32_is_nan(got[nan]).all()


def test_cast_from_f32_rounds_to_nearest_even(cuda):
    """asr_cast_from_f32 to bf16 = f32_to_bf16 (csrc/common.h), the epilogue of every bf16 kernel, on every upper half x
    the lower halves {0000, 0001, 7FFF, 8000, 8001, FFFF}, laid out twice so that the second copy runs in the kernel's
    grid-stride loop.  Zeros, normal numbers, infinities and the overflow of the largest finite values to infinity must
    be the integer round-to-nearest-even form bit for bit; a NaN must give a NaN (payload and sign free).  Subnormal
    float32 inputs (below 2^-126, where the result is subnormal, zero or the smallest normal number) are held to the
    same form.  Measured on an MI355X: all 1534 of them round to nearest even, none is flushed to zero, so the claim at
    f32_to_bf16, "same result for every finite input and infinities", stands as written.  The figures are printed
    before the assertions."""
    ops = _ops()
    one = base.cast_patterns()
    bits = np.concatenate([one] * base.CAST_REPEATS)
    got = _bits(ops.cast_from_f32(_from_bits(bits, cuda), ops.dtype_id(torch.bfloat16)))
    want = base.bf16_rne(bits)
    nan = base.f32_is_nan(bits)
    sub = ((bits & np.uint32(0x7F800000)) == 0) & ((bits & np.uint32(0x007FFFFF)) != 0)
    plain = ~nan & ~sub
    assert int(nan.sum()) == base.CAST_REPEATS * 1534 and int(sub.sum()) == base.CAST_REPEATS * (2 * 128 * 6 - 2)
    diff_sub = sub & (got != want)
    flushed = diff_sub & (got == (bits >> np.uint32(16)).astype(np.uint16) & np.uint16(0x8000))
    print('cast_from_f32: %d values, %d NaN, %d subnormal inputs; differing from RNE: %d normal, %d subnormal '
          '(%d of those are zeros of the input\'s sign)' % (bits.size, nan.sum(), sub.sum(),
                                                           (plain & (got != want)).sum(), diff_sub.sum(), flushed.sum()))
    assert np.array_equal(got[plain], want[plain]), _first_diff(got[plain], want[plain])
    assert base.bf16_is_nan(got[nan]).all()
    assert np.array_equal(got[sub], want[sub]), _first_diff(got[sub], want[sub])
    # the facts by name: signed zeros, infinities, overflow to infinity, ties to even
    for src, dst in [(0x00000000, 0x0000), (0x80000000, 0x8000), (0x7F800000, 0x7F80), (0xFF800000, 0xFF80),
                     (0x7F7FFFFF, 0x7F80), (0x7F7F8000, 0x7F80), (0xFF7F8000, 0xFF80), (0x7F7F7FFF, 0x7F7F),
                     (0x3F808000, 0x3F80), (0x3F818000, 0x3F82), (0x3F808001, 0x3F81), (0x3F807FFF, 0x3F80)]:
        at = np.flatnonzero(bits == src)
        assert at.size == base.CAST_REPEATS and (got[at] == dst).all(), hex(src)


@pytest.mark.parametrize('which', ['from', 'to'])
def test_f32_casts_to_f32_are_copies(cuda, which):
    ops = _ops()
    bits = np.ascontiguousarray(base.cast_patterns()[17::393][:1000])         # NaN payloads and subnormals among them
    assert bits.size == 1000 and base.f32_is_nan(bits).any()
    buf = torch.zeros(1001, dtype=torch.int32, device=cuda)
    src = buf[1:]                                                              # 4 bytes past the allocation: misaligned
    src.copy_(torch.from_numpy(bits.view(np.int32)))
    src = src.view(torch.float32)
    assert src.data_ptr() % 16 != 0
    got = ops.cast_from_f32(src, ops.dtype_id(torch.float32)) if which == 'from' else ops.cast_to_f32(src)
    assert got.dtype == torch.float32
    _assert_bits(got, bits)


# ================================================================ 3. mask application and ReLU backward
@functools.lru_cache(maxsize=None)
def _ew(n):
    act, dout = base.elementwise_inputs(n)
    return _frozen(act), _frozen(dout)


def _ew_tensors(cuda, n, dtype, mis):
    act, dout = _ew(n)
    return (act, dout, base.as_tensor(act, DT[dtype], cuda, misaligned=mis),
            base.as_tensor(dout, torch.float32, cuda, misaligned=mis))


EW_PARAMS = [(n, mis) for n in base.ELEMENTWISE_N for mis in (False, True)] + [(base.ELEMENTWISE_STRIDE_N, False)]
ew_cases = pytest.mark.parametrize('n,mis', EW_PARAMS, ids=['%d%s' % (n, '-misaligned' if m else '') for n, m in EW_PARAMS])
both_dtypes = pytest.mark.parametrize('dtype', ['f32', 'bf16'])
both_drops = pytest.mark.parametrize('drop', base.ELEMENTWISE_DROPS, ids=['keep0.9', 'keep0.8'])


def _check_alignment(mis, *tensors):
    for t in tensors:
        assert (t.data_ptr() % 16 != 0) == mis


@ew_cases
@both_dtypes
@both_drops
def test_apply_mask_is_one_float32_product(cuda, dtype, n, mis, drop):
    act, _, x, _ = _ew_tensors(cuda, n, dtype, mis)
    mask = _mask(n, *drop)
    m = base.as_tensor(mask, torch.float32, cuda, misaligned=mis)
    _check_alignment(mis, x, m)
    _assert_bits(_ops().apply_mask(x, m), base.apply_mask(act, mask, dtype))


@ew_cases
@both_dtypes
@both_drops
def test_dropout_apply_is_the_mask_applied(cuda, dtype, n, mis, drop):
    act, _, x, _ = _ew_tensors(cuda, n, dtype, mis)
    _check_alignment(mis, x)
    _assert_bits(_ops().dropout_apply(x, *drop), base.apply_mask(act, _mask(n, *drop), dtype))


@ew_cases
@both_dtypes
def test_relu_bwd_plain(cuda, dtype, n, mis):
    act, dout, a, g = _ew_tensors(cuda, n, dtype, mis)
    _check_alignment(mis, a, g)
    _assert_bits(_ops().relu_bwd(g, a), base.relu_bwd(dout, act, dtype))


@ew_cases
@both_dtypes
@both_drops
def test_relu_bwd_with_a_mask_tensor_and_with_the_mask_formed_in_the_kernel(cuda, dtype, n, mis, drop):
    act, dout, a, g = _ew_tensors(cuda, n, dtype, mis)
    mask = _mask(n, *drop)
    m = base.as_tensor(mask, torch.float32, cuda, misaligned=mis)
    want = base.relu_bwd(dout, act, dtype, mask=mask)
    _assert_bits(_ops().relu_bwd(g, a, mask=m), want)
    _assert_bits(_ops().relu_bwd(g, a, drop=drop), want)


@ew_cases
@both_dtypes
@pytest.mark.parametrize('keep', [d[0] for d in base.ELEMENTWISE_DROPS])
def test_relu_bwd_scaled(cuda, dtype, n, mis, keep):
    act, dout, a, g = _ew_tensors(cuda, n, dtype, mis)
    _assert_bits(_ops().relu_bwd_scaled(g, a, keep), base.relu_bwd_scaled(dout, act, keep, dtype))


@both_dtypes
@pytest.mark.parametrize('n', [1, 3, 5, 7, 4099])
@pytest.mark.parametrize('entry', ['dropout_apply', 'relu_bwd_drop'])
def test_vector_path_writes_nothing_past_n(cuda, dtype, n, entry):
    """dropout_apply_kernel stores four elements at once where `vec_ok && e0 + 4 <= n`; the last group of an n that is no
    multiple of four must go element by element.  The output is the head of a larger aligned buffer here, so a vector
    store over the end lands on sentinel values instead of in the allocator's slack."""
    ops = _ops()
    from tensorflow_end2end_speech_recognition_amd import _lib
    keep, seed, offset = base.ELEMENTWISE_DROPS[0]
    act, dout = base.elementwise_inputs(n)
    guard = 8
    buf = torch.full((n + guard,), -7.0, dtype=DT[dtype], device=cuda)
    out = buf[:n]
    h = _lib.handle(0, 0)
    if entry == 'dropout_apply':
        x = base.as_tensor(act, DT[dtype], cuda)
        _check_alignment(False, x, out)
        h.check(h.lib.asr_dropout_apply(h.h, ops.dtype_id(DT[dtype]), ops._p(x), ops._p(out), n, keep, seed, offset,
                                        ops._s()), 'asr_dropout_apply')
        want = base.dropout_apply(act, keep, seed, offset, dtype)
    else:
        a = base.as_tensor(act, DT[dtype], cuda)
        g = base.as_tensor(dout, torch.float32, cuda)
        _check_alignment(False, a, g, out)
        h.check(h.lib.asr_relu_bwd_drop(h.h, ops.dtype_id(DT[dtype]), ops._p(g), ops._p(a), n, keep, seed, offset,
                                        ops._p(out), ops._s()), 'asr_relu_bwd_drop')
        want = base.relu_bwd(dout, act, dtype, drop=(keep, seed, offset))
    _assert_bits(out, want)
    assert (buf[n:].float() == -7.0).all().item(), 'elements past n were written'


# ================================================================ 4. 2x2 pooling
POOL_PARAMS = [(c[0], dt) for c in base.POOL_CASES for dt in c[2]]


@functools.lru_cache(maxsize=2)
def _pool_statement(name):
    _, shape, _, kind, _ = [c for c in base.POOL_CASES if c[0] == name][0]
    x = base.pool_input(name, shape, kind)
    val, arg = base.maxpool2x2_fwd(x)
    return _frozen(x), _frozen(val), _frozen(arg)


@pytest.mark.parametrize('name,dtype', POOL_PARAMS, ids=['%s-%s' % p for p in POOL_PARAMS])
def test_maxpool2x2_values_argmax_and_gradient(cuda, name, dtype):
    """Values and argmax of asr_maxpool2x2_fwd equal the statement's -- of equal maxima the first cell in row-major order
    wins, cells outside the image never do -- and asr_maxpool2x2_bwd routes dout by the argmax."""
    ops = _ops()
    _, shape, _, kind, mis = [c for c in base.POOL_CASES if c[0] == name][0]
    N, H, W, C = shape
    x, val, arg = _pool_statement(name)
    xt = base.as_tensor(x, DT[dtype], cuda, misaligned=mis)
    _check_alignment(mis, xt)
    got_val, got_arg = ops.maxpool2x2_fwd(xt)
    assert got_val.dtype == DT[dtype] and got_arg.dtype == torch.uint8
    arg_dev = _bits(got_arg)
    assert np.array_equal(arg_dev, arg), _first_diff(arg_dev, arg)
    _assert_bits(got_val, base.rounded(val, dtype))
    hh = 2 * np.arange(arg.shape[1])[None, :, None, None] + (arg_dev >> 1)
    ww = 2 * np.arange(arg.shape[2])[None, None, :, None] + (arg_dev & 1)
    assert (hh < H).all() and (ww < W).all()                  # every argmax is a cell of the image
    if kind == 'ties' and x.size <= 1 << 20:
        assert base.tied_window_fraction(x) >= base.POOL_TIE_FRACTION
    rng = np.random.RandomState(11)
    dout = rng.randn(*val.shape).astype(np.float32)
    din = ops.maxpool2x2_bwd(torch.from_numpy(dout).to(cuda), got_arg, H, W)
    got_din = _bits(din)
    for a in (arg_dev, arg):
        want = base.f32_bits(base.maxpool2x2_bwd(dout, a, H, W))
        assert np.array_equal(got_din, want), _first_diff(got_din, want)


# ================================================================ 5. im2col3x3 / col2im3x3
IM2COL_PARAMS = [(s, ldp) for s in base.IM2COL_SHAPES for ldp in base.im2col_ldps(s[3])]
im2col_cases = pytest.mark.parametrize('shape,ldp', IM2COL_PARAMS, ids=['%dx%dx%dx%d-ld%d' % (s + (l,)) for s, l in IM2COL_PARAMS])
SENTINEL = -7.0


@im2col_cases
@both_dtypes
def test_im2col3x3_moves_the_right_values_and_leaves_the_padding_columns(cuda, dtype, shape, ldp):
    ops = _ops()
    N, H, W, Cin = shape
    rng = np.random.RandomState(3)
    x = (rng.randint(-127, 128, size=shape) / 8.0).astype(np.float32)          # exact in bf16, zero among the values
    xt = base.as_tensor(x, DT[dtype], cuda)
    out = torch.full((N * H * W, ldp), SENTINEL, dtype=DT[dtype], device=cuda)
    got = ops.im2col3x3(xt, ldp=ldp, out=out)
    assert got is out
    fill = base.rounded(np.array([SENTINEL], np.float32), dtype)[0]
    want = base.im2col3x3(base.rounded(x, dtype), ldp=ldp, fill=fill)
    got = _bits(out)
    k = 9 * Cin
    assert np.array_equal(got[:, :k], want[:, :k]), _first_diff(got[:, :k], want[:, :k])
    assert (got[:, k:] == fill).all()                         # not written: the callers zero these columns once
    if ldp == k:                                              # and the form that allocates its own output
        _assert_bits(ops.im2col3x3(xt), want)


@im2col_cases
def test_col2im3x3_sums_nine_terms(cuda, shape, ldp):
    """Against the float64 statement within 9 * 2^-24 * sum |terms| per element: eight float32 additions of at most
    2^-24 relative each on partial sums bounded by sum |terms|, one to spare.  The general asr_col2im at 3x3 stride 1
    adds the same terms and is held to the same bound, and to the 3x3 kernel within it."""
    ops = _ops()
    N, H, W, Cin = shape
    rng = np.random.RandomState(4)
    dp = rng.randn(N * H * W, ldp).astype(np.float32)
    dpt = torch.from_numpy(dp).to(cuda)
    ref, mag = base.col2im3x3(dp, N, H, W, Cin)
    bound = 9 * EPS * mag
    got = ops.col2im3x3(dpt, N, H, W, Cin).double().cpu().numpy()
    gen = ops.col2im(dpt, N, H, W, Cin, 3, 3, 1, 1).double().cpu().numpy()
    assert got.shape == ref.shape == gen.shape
    print('col2im3x3 %s ld %d: worst error / bound %.3f (3x3), %.3f (general)' % (
        shape, ldp, (np.abs(got - ref) / np.maximum(bound, 1e-300)).max(), (np.abs(gen - ref) / np.maximum(bound, 1e-300)).max()))
    assert (np.abs(got - ref) <= bound).all()
    assert (np.abs(gen - ref) <= bound).all()
    assert (np.abs(got - gen) <= bound).all()


# ================================================================ 6. tanh, softmax
@functools.lru_cache(maxsize=None)
def _tanh_points():
    x = np.concatenate([np.linspace(-20.0, 20.0, 100001), base.TANH_POINTS]).astype(np.float32)
    return _frozen(x)


def test_tanh_fwd_within_two_ulp(cuda):
    """common.h: "precise libm forms, <= 1-2 ulp".  Exact at +-0 (sign kept) and +-inf."""
    x = _tanh_points()
    y = _ops().tanh_fwd(torch.from_numpy(x).to(cuda))
    got = y.double().cpu().numpy()
    ref = base.tanh_fwd(x)
    err = np.abs(got - ref) / base.ulp32(ref)
    print('tanh_fwd: worst error %.3f ulp at x = %r' % (err.max(), float(x[err.argmax()])))
    assert (err <= 2.0).all()
    yb, xb = _bits(y), base.f32_bits(x)
    zero = (xb & np.uint32(0x7FFFFFFF)) == 0
    assert zero.sum() >= 2 and np.array_equal(yb[zero], xb[zero])
    assert np.array_equal(got[np.isinf(x)], np.sign(x[np.isinf(x)])) and np.isinf(x).sum() == 2
    assert (np.abs(got) <= 1.0).all()


def test_tanh_bwd_within_three_roundings(cuda):
    """dx = dy (1 - y^2): the square, the difference and the product round once each, every one at most 2^-24 |dy|
    (|y| <= 1); 4 * 2^-24 |dy| leaves room for a contraction of the first two into one operation either way."""
    x = _tanh_points()
    y = np.tanh(x.astype(np.float64)).astype(np.float32)
    rng = np.random.RandomState(8)
    dy = (rng.randn(x.size) * np.exp(rng.uniform(-10, 10, x.size))).astype(np.float32)
    got = _ops().tanh_bwd(torch.from_numpy(dy).to(cuda), torch.from_numpy(y).to(cuda)).double().cpu().numpy()
    ref = base.tanh_bwd(dy, y)
    bound = 4 * EPS * np.abs(dy.astype(np.float64))
    print('tanh_bwd: worst error / bound %.3f' % (np.abs(got - ref) / bound).max())
    assert (np.abs(got - ref) <= bound).all()


@pytest.mark.parametrize('spread', base.SOFTMAX_SPREADS)
@pytest.mark.parametrize('rows,C', base.SOFTMAX_SHAPES)
def test_softmax_rows_against_float64(cuda, rows, C, spread):
    rng = np.random.RandomState(rows * 131 + C)
    x = (rng.randn(rows, C) * spread).astype(np.float32)
    x[rows // 2, C - 1] = -np.inf                             # one masked entry: exp gives exactly 0, the row still sums to 1
    got_t = _ops().softmax_rows(torch.from_numpy(x).to(cuda))
    got = got_t.double().cpu().numpy()
    ref = base.softmax_rows(x)
    print('softmax_rows %dx%d spread %g: worst error %.3g, worst row sum error %.3g (bound %.3g)' % (
        rows, C, spread, np.abs(got - ref).max(), np.abs(got.sum(axis=1) - 1).max(), C * EPS))
    assert np.isfinite(got).all() and (got >= 0).all()
    assert got[rows // 2, C - 1] == 0.0
    assert (np.abs(got - ref) <= 1e-6).all()
    assert (np.abs(got.sum(axis=1) - 1.0) <= C * EPS).all()
