"""TEST INFRASTRUCTURE ONLY: plain numpy statements of the base elementwise and pooling ops -- the operations that the
fused kernels' "equal to the separate passes, bit for bit" tests stand on -- and the case lists of
tests/test_gpu_base_ops.py.  Nothing here imports the package's ops or tests/_cpu_ops.py.

Conventions: a bf16 array is its uint16 bit patterns; activations enter the statements as float32 VALUES (a bf16
activation widened, which is exact) and leave through `rounded(values, dtype)`, the bits the kernel stores: uint32 for
'f32', uint16 (round-to-nearest-even) for 'bf16'.  Every product is one float32 multiply, so the results are known bit
for bit, the sign of a zero included."""
import numpy as np

from _weight_noise_oracle import philox_blocks        # tied to the Random123 known answer (test_weight_noise_host.py)

M64 = 0xFFFFFFFFFFFFFFFF
F32_ONE = np.float32(1)
F32_ZERO = np.float32(0)


# ---------------------------------------------------------------- bf16
def bf16_rne(bits_u32):
    """float32 bit patterns -> bf16 bit patterns, round to nearest, ties to even, in integers: add 0x7FFF plus the
    lowest kept bit, keep the upper half.  The largest finite values carry into infinity.  A NaN gives a NaN (quiet
    bit set on the upper half); which NaN is not part of the statement."""
    b = np.asarray(bits_u32).astype(np.uint64)
    r = (b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)
    nan = (b & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000)
    r = np.where(nan, (b >> np.uint64(16)) | np.uint64(0x0040), r)
    return r.astype(np.uint16)


def bf16_widen(bits_u16):
    """bf16 bit patterns -> the float32 bit patterns of the same values: << 16."""
    return np.asarray(bits_u16).astype(np.uint32) << np.uint32(16)


def bf16_is_nan(bits_u16):
    return (np.asarray(bits_u16).astype(np.uint32) & np.uint32(0x7FFF)) > np.uint32(0x7F80)


def f32_is_nan(bits_u32):
    return (np.asarray(bits_u32).astype(np.uint32) & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def f32_bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def bf16_values(bits_u16):
    """bf16 bit patterns -> float32 values."""
    return bf16_widen(bits_u16).view(np.float32)


def rounded(values_f32, dtype):
    """The bits a kernel stores for float32 values: uint32 as they are ('f32'), or uint16 after bf16_rne ('bf16')."""
    bits = f32_bits(values_f32)
    return bits if dtype == 'f32' else bf16_rne(bits)


CAST_LOWER_HALVES = (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)


def cast_patterns():
    """The structured float32 set of the cast tests: every upper half x the lower halves that sit on, next to and
    halfway between bf16 values.  uint32 [6 * 65536]."""
    up = np.arange(65536, dtype=np.uint32) << np.uint32(16)
    return np.concatenate([up | np.uint32(lo) for lo in CAST_LOWER_HALVES])


# ---------------------------------------------------------------- dropout
def dropout_mask(n, keep, seed, offset):
    """asr_dropout_mask: element e takes word e % 4 of the Philox4x32-10 block of counter offset + e // 4 (64-bit, as
    {lo, hi, 0, 0}) under key seed; u = (word >> 8) 2^-24; float32(1) / float32(keep) where u < float32(keep), else 0.
    The 24-bit integer, its scaling and the comparison are exact in float32."""
    n = int(n)
    m = (n + 3) // 4
    with np.errstate(over='ignore'):
        ctr = np.arange(m, dtype=np.uint64) + np.uint64(int(offset) & M64)        # wraps like the kernel's uint64_t
    words = philox_blocks(ctr, seed).reshape(-1)[:n]
    u = (words >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    keep32 = np.float32(keep)
    return np.where(u < keep32, F32_ONE / keep32, F32_ZERO).astype(np.float32)


def apply_mask(x, mask, dtype):
    """x * mask, one float32 multiply, stored in dtype."""
    return rounded(np.asarray(x, np.float32) * np.asarray(mask, np.float32), dtype)


def dropout_apply(x, keep, seed, offset, dtype):
    """apply_mask with the mask of dropout_mask(x.size, keep, seed, offset)."""
    x = np.asarray(x, np.float32)
    return apply_mask(x, dropout_mask(x.size, keep, seed, offset).reshape(x.shape), dtype)


def relu_bwd(dout, out, dtype, mask=None, drop=None):
    """dpre = (out > 0) ? dout (* mask) : +0, stored in dtype.  out > 0 is false for -0.0 (and for +0.0).
    drop = (keep, seed, offset) stands for the mask tensor dropout_mask gives."""
    g = np.asarray(dout, np.float32)
    out = np.asarray(out, np.float32)
    if drop is not None:
        mask = dropout_mask(g.size, *drop).reshape(g.shape)
    if mask is not None:
        g = g * np.asarray(mask, np.float32)
    return rounded(np.where(out > 0, g, F32_ZERO), dtype)


def relu_bwd_scaled(dout, out_dropped, keep, dtype):
    """dpre = (out_dropped > 0) ? dout * (float32(1) / float32(keep)) : +0, stored in dtype."""
    scale = F32_ONE / np.float32(keep)
    g = np.asarray(dout, np.float32) * scale
    return rounded(np.where(np.asarray(out_dropped, np.float32) > 0, g, F32_ZERO), dtype)


# ---------------------------------------------------------------- 2x2 pooling
def maxpool2x2_fwd(x):
    """max_pool 2x2 stride 2 SAME on [N,H,W,C]: window (ho, wo) holds the cells k = 2 dh + dw at (2 ho + dh, 2 wo + dw)
    that lie inside the image, visited in the order k = 0, 1, 2, 3; a cell replaces the best so far only when strictly
    greater, so of equal maxima the first in row-major order wins.  -> (values like x, argmax uint8 = that k)."""
    x = np.asarray(x)
    N, H, W, C = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    best = np.full((N, Ho, Wo, C), -np.inf, dtype=x.dtype)
    arg = np.zeros((N, Ho, Wo, C), dtype=np.uint8)
    for k in range(4):
        dh, dw = k >> 1, k & 1
        cell = x[:, dh::2, dw::2, :]                      # the windows whose cell k exists: the first hk x wk of them
        hk, wk = cell.shape[1], cell.shape[2]
        b, a = best[:, :hk, :wk, :], arg[:, :hk, :wk, :]
        gt = cell > b
        b[gt] = cell[gt]
        a[gt] = k
    return best, arg


def maxpool2x2_bwd(dout, arg, H, W):
    """din[n, h, w, c] = dout[n, h // 2, w // 2, c] where arg there names cell 2 (h & 1) + (w & 1), else 0."""
    dout = np.asarray(dout, np.float32)
    N, _, _, C = dout.shape
    din = np.zeros((N, H, W, C), dtype=np.float32)
    for k in range(4):
        dh, dw = k >> 1, k & 1
        tgt = din[:, dh::2, dw::2, :]
        hk, wk = tgt.shape[1], tgt.shape[2]
        tgt[...] = np.where(arg[:, :hk, :wk, :] == k, dout[:, :hk, :wk, :], F32_ZERO)
    return din


# ---------------------------------------------------------------- im2col / col2im, 3x3 SAME
def im2col3x3(x, ldp=None, fill=0):
    """patches[m, tap * Cin + ci] = x[n, h + tap // 3 - 1, w + tap % 3 - 1, ci] (0 outside the image), m = (n H + h) W + w,
    row stride ldp >= 9 Cin; columns from 9 Cin on hold `fill` (the kernel leaves them alone).  Any dtype, bit
    patterns included: the operation only moves values."""
    x = np.asarray(x)
    N, H, W, Cin = x.shape
    ldp = ldp or 9 * Cin
    assert ldp >= 9 * Cin
    xp = np.zeros((N, H + 2, W + 2, Cin), dtype=x.dtype)
    xp[:, 1:H + 1, 1:W + 1, :] = x
    out = np.full((N * H * W, ldp), fill, dtype=x.dtype)
    for tap in range(9):
        dh, dw = tap // 3, tap % 3
        out[:, tap * Cin:(tap + 1) * Cin] = xp[:, dh:dh + H, dw:dw + W, :].reshape(N * H * W, Cin)
    return out


def col2im3x3(dpatches, N, H, W, Cin):
    """din[n, h, w, ci] = sum over taps of dpatches[pixel(h - (tap // 3 - 1), w - (tap % 3 - 1)), tap * Cin + ci] over
    the taps whose pixel exists, in float64.  -> (din, sum of |terms|), both [N,H,W,Cin]."""
    dp = np.asarray(dpatches, np.float64)
    assert dp.shape[0] == N * H * W and dp.shape[1] >= 9 * Cin
    din = np.zeros((N, H, W, Cin))
    mag = np.zeros((N, H, W, Cin))
    for tap in range(9):
        dh, dw = tap // 3 - 1, tap % 3 - 1
        t = np.zeros((N, H + 2, W + 2, Cin))              # t[n, 1 + hd + dh, 1 + wd + dw] = the term pixel (hd, wd) sends
        t[:, 1 + dh:1 + dh + H, 1 + dw:1 + dw + W, :] = dp[:, tap * Cin:(tap + 1) * Cin].reshape(N, H, W, Cin)
        din += t[:, 1:H + 1, 1:W + 1, :]
        mag += np.abs(t[:, 1:H + 1, 1:W + 1, :])
    return din, mag


# ---------------------------------------------------------------- tanh, softmax
def tanh_fwd(x):
    return np.tanh(np.asarray(x, np.float64))


def tanh_bwd(dy, y):
    dy, y = np.asarray(dy, np.float64), np.asarray(y, np.float64)
    return dy * (1.0 - y * y)


def softmax_rows(x):
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def ulp32(ref):
    """One float32 unit in the last place at the float64 value ref: 2^(floor(log2 |ref|) - 23), the binade read from ref
    itself (0.99999999 counts as below 1, not as the 1.0f it rounds to), never below the subnormal spacing 2^-149."""
    mag = np.maximum(np.abs(np.asarray(ref, np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(mag)) - 23)


# ---------------------------------------------------------------- the case lists
# The launchers' rules, as they stand in csrc/elementwise.hip and csrc/vgg.hip:
#   grid_for(n): min(ceil(n / 256), 2048) blocks of 256 -- a kernel loops over its grid when n > 2048 * 256 work items
#   gridv(n):    min(ceil(n / 256), 4096) blocks of 256 -- likewise above 4096 * 256
#   asr_dropout_mask / asr_dropout_apply / asr_relu_bwd_drop: one work item per four elements, grid_for((n + 3) / 4);
#     vec_ok = every pointer 16-byte aligned; a group takes the vector path when `vec_ok && e0 + 4 <= n`
#   asr_cast_*, asr_apply_mask, asr_tanh_*: grid_for(n);  asr_relu_bwd, asr_relu_bwd_scaled, asr_maxpool2x2_bwd,
#     asr_im2col3x3, asr_col2im3x3: gridv(work items)
#   asr_maxpool2x2_fwd: `C % 4 == 0 && 16-byte aligned` (in, out, argmax) -> maxpool_fwd_vec_kernel on
#     gridv(outputs / 4), else maxpool_fwd_kernel on gridv(outputs)
GRID_FOR_CAP = 2048 * 256
GRIDV_CAP = 4096 * 256

# (name, sizes, keep, seed, offset): one stream per row, cut at each of the sizes
DROPOUT_MASK_CASES = [
    # dropout_mask_kernel's `e < n`: words 1..3, 2..3, 3 of the only block cut; one whole block; a second block with one
    # word used; several workgroups and a three-word tail
    ('tails', (1, 2, 3, 4, 5, 4099), 0.8, 7, 0),
    ('high-words', (4096,), 0.8, (7 << 32) + 11, (5 << 32) + 17),   # key word k1 = seed >> 32 and counter word ctr >> 32
    ('counter-carry', (16,), 0.8, 3, 2 ** 32 - 2),                  # offset + i carries from c[0] into c[1] at block 2
    ('offset-2^50', (64,), 0.8, 3, 2 ** 50),       # a counter that only has a high word
    ('keep-1', (1000,), 1.0, 1, 0),                # u < 1 always: nothing dropped, inv = 1
    ('inv-inexact', (1000,), 0.9, 21, (4 << 32) + 3),               # 1 / 0.9f is rounded: inv formed as 1.f / keep
    ('keep-0.05', (100000,), 0.05, 9, 0),          # inv = 20, almost all dropped
    ('grid-stride', (2200003,), 0.8, 5, 123),      # (n + 3) / 4 = 550 001 > grid_for's 2048 * 256: the loop wraps
]
DROPOUT_STRIDE_CASES = ('grid-stride',)

# asr_cast_from_f32 / asr_cast_to_f32 F32 -> BF16: the structured set twice over, 786 432 values > grid_for's
# 2048 * 256 = 524 288 (the set alone, 393 216, stays below it), so every pattern also passes through the stride loop
CAST_REPEATS = 2

# apply_mask / dropout_apply / relu_bwd / relu_bwd_scaled sizes:
ELEMENTWISE_N = [
    1,          # dropout_apply_kernel: e0 + 4 > n in the only group; scalar tail of one
    3,          # ... n % 4 == 3: the tail one short of a vector
    4,          # exactly one vector group, no tail
    5,          # one vector group, then a tail of one
    4099,       # many vector groups over several workgroups, then a tail of three
    600001,     # more than grid_for's 2048 * 256 elements: apply_mask_kernel's loop wraps
]
ELEMENTWISE_STRIDE_N = 4 * GRID_FOR_CAP + 4 * 777 + 3   # > 4 * 2048 * 256 elements: dropout_apply_kernel's loop wraps
#                                                         (one item per 4), and > 4096 * 256: relu_bwd(_scaled)_kernel's
ELEMENTWISE_DROPS = [(0.9, 21, (4 << 32) + 3), (0.8, 7, 0)]


def elementwise_inputs(n):
    """(act, dout) float32 [n]: activations that are positive, negative, +0.0 and -0.0 for a quarter of the elements
    each (multiples of 1/8 below 16: exact in bf16), and a gradient that bf16 has to round."""
    rng = np.random.RandomState(n % (2 ** 31))
    kind = rng.permutation(n) % 4
    mag = rng.randint(1, 128, size=n) / 8.0
    act = np.where(kind == 0, mag, np.where(kind == 1, -mag, np.where(kind == 2, 0.0, -0.0))).astype(np.float32)
    return act, rng.randn(n).astype(np.float32)

# (name, (N, H, W, C), dtypes, kind, misaligned) -- kind: 'normal' | 'ties' | 'negative'
POOL_CASES = [
    ('vec-odd-odd', (2, 5, 3, 8), ('f32', 'bf16'), 'normal', False),      # maxpool_fwd_vec_kernel: H, W odd -- edge windows of 2 and 1 cells
    ('vec-even-even', (3, 6, 4, 8), ('f32', 'bf16'), 'normal', False),    # ... every window whole
    ('vec-1x1', (1, 1, 1, 4), ('f32', 'bf16'), 'normal', False),          # ... one cell, one work item
    ('vec-1xW', (2, 1, 7, 4), ('f32', 'bf16'), 'normal', False),          # ... H = 1: cells 2, 3 never exist; W odd
    ('vec-Hx1', (2, 7, 1, 4), ('f32', 'bf16'), 'normal', False),          # ... W = 1: cells 1, 3 never exist; H odd
    ('scalar-C3', (2, 5, 3, 3), ('f32', 'bf16'), 'normal', False),        # maxpool_fwd_kernel through C % 4 != 0, odd image
    ('scalar-C6', (2, 6, 4, 6), ('f32', 'bf16'), 'normal', False),        # ... C even but no multiple of 4
    ('scalar-1x1x1', (1, 1, 1, 1), ('f32', 'bf16'), 'normal', False),     # ... a single value
    ('scalar-misaligned', (2, 5, 3, 8), ('f32', 'bf16'), 'normal', True),  # maxpool_fwd_kernel through `16-byte aligned` failing, C % 4 == 0
    ('model-block1', (3, 40, 11, 64), ('f32', 'bf16'), 'normal', False),  # the VGG front-end's first pool
    ('model-block2', (3, 20, 6, 128), ('f32', 'bf16'), 'normal', False),  # ... and its second
    ('ties', (4, 6, 6, 8), ('f32', 'bf16'), 'ties', False),               # post-ReLU zeros and quantised maxima: v > best keeps the first
    ('negative', (4, 6, 6, 8), ('f32', 'bf16'), 'negative', False),       # best starts at -inf, bi at 0: padding must never win
    ('ties-scalar', (4, 5, 5, 6), ('f32', 'bf16'), 'ties', False),        # the tie rule in maxpool_fwd_kernel, odd edges included
    ('ties-misaligned', (2, 5, 3, 8), ('f32', 'bf16'), 'ties', True),     # ... and through `16-byte aligned` failing: only the scalar kernel's rule decides here
    ('negative-scalar', (2, 5, 3, 3), ('f32', 'bf16'), 'negative', False),  # -inf start in maxpool_fwd_kernel at the odd edges
    ('stride-scalar', (140, 40, 11, 66), ('f32',), 'normal', False),      # 1 108 800 outputs > gridv's 4096 * 256: maxpool_fwd_kernel wraps
    ('stride-vec', (560, 40, 11, 64), ('bf16',), 'normal', False),        # 1 075 200 groups of 4 > 4096 * 256: maxpool_fwd_vec_kernel wraps; its backward (15.8 M) wraps maxpool_bwd_kernel
]
POOL_TIE_FRACTION = 0.05


def pool_input(name, shape, kind):
    """float32 values, exact in bf16 (multiples of 1/8 or 1/2 below 16), reproducible from the case's name."""
    rng = np.random.RandomState(sum(ord(ch) for ch in name) * 7919 % (2 ** 31))
    if kind == 'ties':          # ReLU output: about half zeros, the rest multiples of 0.5 in (0, 2]
        x = np.maximum(np.round(rng.randn(*shape) * 2.0), 0.0) * 0.5
        return np.minimum(x, 2.0).astype(np.float32)
    if kind == 'negative':
        return (-(rng.randint(1, 128, size=shape)) / 8.0).astype(np.float32)
    return (rng.randint(-127, 128, size=shape) / 8.0).astype(np.float32)


def pool_work_items(shape, vec):
    N, H, W, C = shape
    outputs = N * ((H + 1) // 2) * ((W + 1) // 2) * C
    return outputs // 4 if vec else outputs


def tied_window_fraction(x):
    """Share of (window, channel) pairs whose maximum is reached by more than one existing cell."""
    best, _ = maxpool2x2_fwd(x)
    count = np.zeros(best.shape, dtype=np.int32)
    for k in range(4):
        cell = x[:, (k >> 1)::2, (k & 1)::2, :]
        hk, wk = cell.shape[1], cell.shape[2]
        count[:, :hk, :wk, :] += cell == best[:, :hk, :wk, :]
    return float((count > 1).mean())


# asr_im2col3x3 / asr_col2im3x3 (N, H, W, Cin):
IM2COL_SHAPES = [
    (2, 5, 3, 3),        # odd image, Cin = 3: every border pattern, 9 Cin = 27 is no multiple of 8
    (1, 1, 1, 1),        # one pixel: only the centre tap is inside
    (3, 40, 11, 3),      # the first VGG layer's image
    (2, 20, 6, 64),      # the third VGG layer's image; 9 Cin = 576 is a multiple of 8 already
]


def im2col_ldps(Cin):
    """ldp = 9 Cin, and 9 Cin rounded up to a multiple of 8 (the GEMM's k granule) where that differs."""
    k = 9 * Cin
    return sorted({k, (k + 7) // 8 * 8})


# asr_softmax_rows (rows, C): one wave per row, four rows per workgroup, lanes stride the row by 64
SOFTMAX_SHAPES = [
    (1, 2),          # one row, 62 idle lanes; three idle waves
    (5, 62),         # rows % 4 != 0: `row >= rows` in the last workgroup; the existing test's width
    (7, 64),         # exactly one element per lane
    (7, 65),         # one lane takes a second trip
    (3, 3387),       # a word-level vocabulary: 53 trips, the last partial
    (1030, 29),      # many workgroups
]
SOFTMAX_SPREADS = [3.0, 60.0]

# asr_tanh_fwd special points beside the 100 001 over [-20, 20]
TANH_POINTS = [0.0, -0.0, 1e-30, -1e-30, 88.0, -88.0, np.inf, -np.inf]


def as_tensor(values, torch_dtype, device, misaligned=False):
    """A contiguous tensor of `values` (numpy float array, any shape) in torch_dtype on device.  misaligned: the view
    `buf[1:]` of a flat buffer one element longer, so that its pointer sits one element (2 or 4 bytes) past an
    allocation boundary and fails every kernel's 16-byte test while staying contiguous."""
    import torch
    src = torch.from_numpy(np.array(values, order='C'))      # a copy: the callers' arrays are shared and read-only
    if not misaligned:
        return src.to(device=device, dtype=torch_dtype).contiguous()
    buf = torch.zeros(src.numel() + 1, dtype=torch_dtype, device=device)
    view = buf[1:].view(src.shape)
    view.copy_(src)
    return view
