"""TEST INFRASTRUCTURE ONLY: the numpy statement of the input augmentation (include/asr_hip.h, asr_input_augment), built on
the Philox / Box-Muller statement of tests/_weight_noise_oracle.py.  For element i = (b T + t) F + f of x [B,T,F]:
  1. t >= len_b = clamp(seq_len[b], 0, T): y[i] has the bits of x[i];
  2. v = x[i], with noise_std > 0: v = fl32(x[i] + fl32(noise_std * z_i)), z_i = z(offset + (i >> 2), seed)[i & 3];
  3. mask slot = philox_block(offset + 2^39 + 16 b + slot, seed); frequency slots 0 .. n_fmask-1, time slots 8 .. 8+n_tmask-1;
     mulhi(u, n) = (u n) >> 32; frequency: fw = mulhi(c0, min(fmask_width, n_ch) + 1), fs = mulhi(c1, n_ch - fw + 1), covers
     fs <= f mod n_ch < fs + fw; time: Tcap = min(tmask_width, floor(fl32(ratio * len_b))), tw = mulhi(c0, Tcap + 1),
     ts = mulhi(c1, len_b - tw + 1), covers ts <= t < ts + tw; a covered element is mask_value, every other one v."""
import numpy as np

import _weight_noise_oracle as own

MAX_MASKS = 8
MASK_BASE = 1 << 39
U64 = 0xFFFFFFFFFFFFFFFF


def clamp_lens(seq_len, T):
    return np.clip(np.asarray(seq_len, dtype=np.int64), 0, int(T))


def _mulhi(u, n):
    return (np.asarray(u, dtype=np.uint64) * np.asarray(n, dtype=np.uint64)) >> np.uint64(32)


def _slot_blocks(B, first_slot, n, seed, offset):
    """-> uint64 [B, n, 4]: the blocks of slots first_slot .. first_slot + n - 1 of utterances 0 .. B-1."""
    b = np.arange(B, dtype=np.uint64)[:, None]
    s = np.arange(first_slot, first_slot + n, dtype=np.uint64)[None, :]
    ctr = (np.uint64((int(offset) + MASK_BASE) & U64) + np.uint64(16) * b + s)      # uint64 arithmetic wraps like the device's
    return own.philox_blocks(ctr.reshape(-1), seed).reshape(B, n, 4)


def time_cap(lens, tmask_width, tmask_ratio):
    """min(tmask_width, (int)floorf(ratio * (float)len)) with the product in fp32."""
    r = np.floor(np.float32(tmask_ratio) * np.asarray(lens).astype(np.float32)).astype(np.int64)
    return np.minimum(np.int64(tmask_width), r)


def freq_draws(B, n_ch, n_fmask, fmask_width, seed, offset):
    """-> int64 [B, n_fmask, 2]: (width, start) of every frequency mask."""
    c = _slot_blocks(B, 0, n_fmask, seed, offset)
    cap = min(int(fmask_width), int(n_ch))
    fw = _mulhi(c[:, :, 0], cap + 1).astype(np.int64)
    fs = _mulhi(c[:, :, 1], (n_ch - fw + 1).astype(np.uint64)).astype(np.int64)
    return np.stack([fw, fs], axis=2)


def time_draws(lens, n_tmask, tmask_width, tmask_ratio, seed, offset):
    """lens: the clamped lengths [B] -> int64 [B, n_tmask, 2]: (width, start) of every time mask."""
    lens = np.asarray(lens, dtype=np.int64)
    c = _slot_blocks(len(lens), MAX_MASKS, n_tmask, seed, offset)
    cap = time_cap(lens, tmask_width, tmask_ratio)[:, None]
    tw = _mulhi(c[:, :, 0], (cap + 1).astype(np.uint64)).astype(np.int64)
    ts = _mulhi(c[:, :, 1], (lens[:, None] - tw + 1).astype(np.uint64)).astype(np.int64)
    return np.stack([tw, ts], axis=2)


def cover(shape, seq_len, n_ch, freq_masks=(0, 0), time_masks=(0, 0, 1.0), seed=0, offset=0):
    """-> (valid [B,T,1] bool: t < len_b, masked [B,T,F] bool: valid and covered by a mask, fd, td: the draws)."""
    B, T, F = shape
    assert 1 <= n_ch <= F and F % n_ch == 0
    lens = clamp_lens(seq_len, T)
    t = np.arange(T)[None, :, None]
    ch = (np.arange(F) % n_ch)[None, None, :]
    valid = t < lens[:, None, None]
    fd = freq_draws(B, n_ch, freq_masks[0], freq_masks[1], seed, offset)
    td = time_draws(lens, time_masks[0], time_masks[1], time_masks[2], seed, offset)
    masked = np.zeros((B, T, F), dtype=bool)
    for m in range(fd.shape[1]):
        w, s = fd[:, m, 0][:, None, None], fd[:, m, 1][:, None, None]
        masked |= (ch >= s) & (ch < s + w)
    for m in range(td.shape[1]):
        w, s = td[:, m, 0][:, None, None], td[:, m, 1][:, None, None]
        masked |= (t >= s) & (t < s + w)
    return valid, masked & valid, fd, td


def noise(n, seed, offset):
    """z_i of the n flat elements, float64."""
    return own.z(n, seed, offset)


def augment(x, seq_len, n_ch, noise_std=0.0, freq_masks=(0, 0), time_masks=(0, 0, 1.0), mask_value=0.0, seed=0, offset=0):
    """The statement on a float32 array x [B,T,F] -> y float32 (z taken in float64 and rounded to fp32 first)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    valid, masked, _, _ = cover(x.shape, seq_len, n_ch, freq_masks, time_masks, seed, offset)
    y = x.copy()
    if float(noise_std) > 0.0:
        z = noise(x.size, seed, offset).astype(np.float32).reshape(x.shape)
        with np.errstate(invalid='ignore'):
            v = (x + (np.float32(noise_std) * z).astype(np.float32)).astype(np.float32)
        y = np.where(valid, v, x)
    y = np.where(masked, np.float32(mask_value), y).astype(np.float32)
    # (np.where keeps the bit patterns of x, NaN payloads and -0.0 included)
    return y
