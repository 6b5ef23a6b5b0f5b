"""The launch counters on the device's handles: every public view of ops after its reset, the two native getter forms
(fixed word count / sized with zero fill) called straight on a handle, and the sum over a device's handles.  Host counters
throughout; the only device work is two 8 x 64 x 64 products.  Which kernel a call ends in is the variant tests' business."""
import ctypes as C

import pytest
import torch

from tensorflow_end2end_speech_recognition_amd import _counters, _lib, ops

pytestmark = pytest.mark.gpu

POISON = 0xDEADBEEFDEADBEEF


def _family_reset(view):
    """The ops function that zeroes the family `view` reads."""
    name = next(v.reset for v in _counters.VIEWS.values() if v.family == view.family and v.reset)
    return getattr(ops, name)


def _raw(h, fam, n_buf, *n):
    """fam's getter on handle h into a poisoned buffer of n_buf words; returns the buffer as a list."""
    out = (C.c_ulonglong * n_buf)(*([POISON] * n_buf))
    h.check(getattr(h.lib, fam.getter)(h.h, out, *n), fam.getter)
    return [int(v) for v in out]


def _two_products(cuda):
    """One tiny fp32 product on the main lane, one on side lane 1."""
    a = torch.ones(8, 64, dtype=torch.float32, device=cuda)
    b = torch.ones(64, 64, dtype=torch.float32, device=cuda)
    c0 = ops.gemm(a, b)
    with ops.side_lane(cuda, keep=[a, b]):
        c1 = ops.gemm(a, b)
    ops.join_side(cuda)
    assert float(c0.sum()) == float(c1.sum()) == 8 * 64 * 64.0


@pytest.mark.parametrize('name', list(_counters.VIEWS))
def test_view_after_reset(cuda, name):
    view = _counters.VIEWS[name]
    _family_reset(view)(cuda)
    got = getattr(ops, name)(cuda)
    assert list(got.items()) == [(k, 0) for k in view.keys]
    assert getattr(ops, name)() == got                                     # device=0 is the default


def test_sized_getters_fill_and_truncate(cuda):
    h = _lib.handle(0)
    ops.reset_gemm_path_counts(cuda)
    _two_products(cuda)                                                    # something to read on the GEMM family
    for fam in _counters.FAMILIES.values():
        if not fam.sized:
            continue
        N = len(fam.keys)
        full = _raw(h, fam, N, N)
        assert POISON not in full
        assert _raw(h, fam, N + 3, N + 2) == full + [0, 0, POISON]         # zero fill past N, nothing past n
        assert _raw(h, fam, N, N - 1) == full[:N - 1] + [POISON]           # fewer: truncated
        assert _raw(h, fam, 2, 0) == [POISON, POISON]                      # n = 0 succeeds and writes nothing
        with pytest.raises(ValueError):
            _raw(h, fam, 2, -1)
    gemm = _counters.FAMILIES['gemm_path_counts']
    assert sum(_raw(h, gemm, len(gemm.keys), len(gemm.keys))) == 1         # the main lane's product, not all zeros


def test_fixed_getters_write_their_word_count(cuda):
    h = _lib.handle(0)
    seen = set()
    for fam in _counters.FAMILIES.values():
        if fam.sized:
            continue
        N = len(fam.keys)
        seen.add(N)
        got = _raw(h, fam, N + 4)
        assert POISON not in got[:N] and got[N:] == [POISON] * 4, fam.getter
    assert seen == {3, 4, 6}


def test_sum_over_handles_and_independence(cuda):
    fam = _counters.FAMILIES['gemm_path_counts']
    gemm_views = [v for v in _counters.VIEWS.values() if v.family == 'gemm_path_counts']
    assert len(gemm_views) == 4
    ops.reset_gemm_path_counts(cuda)
    before = sum(ops.gemm_kernel_counts(cuda).values())
    _two_products(cuda)
    assert sum(ops.gemm_kernel_counts(cuda).values()) == before + 2
    # one product on each handle; the view is their sum
    lanes = [_lib.handle(0, 0), _lib.handle(0, 1)]
    assert [sum(_raw(h, fam, len(fam.keys), len(fam.keys))) for h in lanes] == [1, 1]
    ops.reset_att_beam_counts(cuda)                                        # an unrelated family's reset
    assert sum(ops.gemm_kernel_counts(cuda).values()) == before + 2
    ops.reset_gemm_path_counts(cuda)
    for v in gemm_views:
        assert getattr(ops, v.name)(cuda) == dict.fromkeys(v.keys, 0)
    assert [sum(_raw(h, fam, len(fam.keys), len(fam.keys))) for h in lanes] == [0, 0]
