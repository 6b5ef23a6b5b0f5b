"""TEST INFRASTRUCTURE ONLY: the float64 statement of the Gaussian weight noise (include/asr_hip.h,
asr_weight_noise_perturb): z(n, seed, offset) -- element i takes the Philox4x32-10 block of counter {lo, hi, 0, 0} of
offset + (i >> 2) under key = seed; element 4q + j takes the word pair (c0, c1) for j = 0, 1 and (c2, c3) for j = 2, 3;
u_a = ((c_even >> 8) + 1) 2^-24 in (0, 1], u_b = (c_odd >> 8) 2^-24, r = sqrt(-2 ln u_a), z = r cos(2 pi u_b) for even j
and r sin(2 pi u_b) for odd j.  |z| <= sqrt(-2 ln 2^-24) = 5.768."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
Z_MAX = 5.7682           # sqrt(48 ln 2) = 5.76814..., rounded up


def philox_blocks(ctr, seed):
    """ctr: uint64 array [m] -> uint32-valued uint64 array [m, 4]: Philox4x32-10 of counter {lo, hi, 0, 0}, key = seed."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    c0, c1 = ctr & M32, ctr >> np.uint64(32)
    c2 = np.zeros_like(ctr)
    c3 = np.zeros_like(ctr)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n1 = p1 & M32
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        n3 = p0 & M32
        c0, c1, c2, c3 = n0, n1, n2, n3
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=1)


def z(n, seed, offset):
    """The n standard normal values of a buffer of n elements, float64."""
    n = int(n)
    m = (n + 3) // 4
    ctr = (np.arange(m, dtype=np.uint64) + np.uint64(int(offset) & 0xFFFFFFFFFFFFFFFF))
    c = philox_blocks(ctr, seed)
    out = np.empty((m, 4), dtype=np.float64)
    for j in (0, 2):
        ua = ((c[:, j] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
        ub = (c[:, j + 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(ua))
        out[:, j] = r * np.cos(2.0 * np.pi * ub)
        out[:, j + 1] = r * np.sin(2.0 * np.pi * ub)
    return out.reshape(-1)[:n]


def ulp32(x):
    """Spacing of float32 at |x| (float64 array)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)
