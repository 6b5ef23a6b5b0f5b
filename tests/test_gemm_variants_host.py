"""Host side of tests/test_gpu_gemm_variants.py: the dispatch rule of csrc/gemm.hip as tests/_gemm_variants.py restates
it, pinned at every shape that file runs (scratch_room passed in as a number), and the properties of the integer data the
exact regime rests on, which concern the fp64 reference alone."""
import pytest

from _gemm_variants import (ALL_KEYS, CASES, GAUSSIAN, ROOM, SPLITK_S, WORKER_SHAPES, expected_gemm, gemm_plan, host_data,
                            nt_big_switch, predicted_counters)


def e(dtype, od, ta, tb, M, N, K, lda=None, ldb=None, ldc=None, a_off=0, b_off=0, c_off=None, bias=None, mul=None, ldm=None,
      drop=False, room=ROOM, tn_wgs=0, big=1):
    """expected_gemm with C in its guard frame (ldc = N + 8, two rows and four columns in) unless said otherwise."""
    lda = (M if ta else K) if lda is None else lda
    ldb = (K if tb else N) if ldb is None else ldb
    ldc = N + 8 if ldc is None else ldc
    c_off = (2 * ldc + 4) % (4 if od == 'f32' else 8) if c_off is None else c_off
    return expected_gemm(dtype, od, ta, tb, M, N, K, lda, ldb, ldc, a_off, b_off, c_off, bias, mul, N if ldm is None else ldm,
                         drop, room, tn_wgs, big)


def test_the_arena_split_is_the_library_s():
    from _conv_variants import xch_bytes_of_the_library
    from _gemm_variants import XCH_BYTES
    assert XCH_BYTES == xch_bytes_of_the_library()          # what scratch_room is taken from


def test_the_switch_is_read_as_atoi_reads_it():
    assert [nt_big_switch(dict(ASR_GEMM_NT_BIG=v)) for v in ('0', '1', '2', ' 2', 'x', '', '2x', '-1')] == [0, 1, 2, 2, 0, 0, 2, -1]
    assert nt_big_switch({}) == 1


def test_dispatch_rule_at_the_skinny_shapes():
    for s in [(17, 32, 64), (16, 32, 512), (32, 64, 576), (15, 96, 1024), (1, 32, 1088)]:
        assert e('f32', 'f32', 0, 0, *s) == ['skinny_nn32']
        assert e('f32', 'f32', 0, 1, *s) == ['skinny_nt16']              # B^T rows: narrow until N >= 6144
    for s in [(17, 48, 64), (32, 16, 576), (1, 80, 1088)]:
        assert e('f32', 'f32', 0, 0, *s) == ['skinny_nn16']
    for s in [(17, 16, 64), (32, 48, 1088)]:
        assert e('f32', 'f32', 0, 1, *s) == ['skinny_nt16']
    for s in [(17, 6144, 64), (32, 6144, 576)]:
        assert e('f32', 'f32', 0, 1, *s) == ['skinny_nt32']
        assert e('f32', 'f32', 0, 0, *s) == ['skinny_nn32']
    assert e('f32', 'f32', 0, 1, 17, 6112, 64) == ['skinny_nt16'] and e('f32', 'f32', 0, 1, 17, 6160, 64) == ['skinny_nt16']
    # a multiplier is a second pass behind the skinny kernel; a bf16 result or bf16 operands are not skinny
    assert e('f32', 'f32', 0, 0, 17, 32, 64, mul=0) == ['skinny_nn32', 'mul_pass']
    assert e('f32', 'f32', 0, 0, 17, 32, 64, drop=True, ldc=32, c_off=0) == ['skinny_nn32', 'drop_pass']
    assert e('f32', 'bf16', 0, 0, 17, 32, 64) == ['generic64'] and e('bf16', 'f32', 0, 0, 17, 32, 64) == ['generic64']
    assert e('f32', 'bf16', 0, 0, 16, 32, 512) == ['generic64_splitk']
    assert e('f32', 'bf16', 0, 1, 32, 6144, 576) == ['generic64_splitk']
    # refusals
    g = ['generic64']
    assert e('f32', 'f32', 0, 0, 33, 32, 64) == g and e('f32', 'f32', 0, 0, 17, 32, 96) == g
    assert e('f32', 'f32', 0, 0, 17, 24, 64) == g and e('f32', 'f32', 1, 0, 17, 32, 64) == g
    assert e('f32', 'f32', 0, 0, 17, 32, 64, lda=65) == g and e('f32', 'f32', 0, 0, 17, 32, 64, a_off=1) == g
    assert e('f32', 'f32', 0, 0, 17, 32, 64, b_off=1) == g and e('f32', 'f32', 0, 1, 17, 32, 64, ldb=66) == g
    assert e('f32', 'f32', 0, 0, 17, 32, 64, ldb=33) == ['skinny_nn32']    # row-major B: any row stride
    assert e('f32', 'f32', 0, 0, 17, 32, 64, a_off=4, b_off=4) == ['skinny_nn32']
    assert e('f32', 'f32', 0, 0, 17, 32, 64, a_off=1, mul=0) == ['generic64', 'mul_pass']


def test_dispatch_rule_at_the_generic_shapes():
    for dt in ('f32', 'bf16'):
        for od in ('f32', 'bf16'):
            for ta in (0, 1):
                for tb in (0, 1):
                    for s in [(1, 1, 1), (65, 67, 33), (64, 64, 64)]:
                        assert e(dt, od, ta, tb, *s) == ['generic64']
                    assert e(dt, od, ta, tb, 65, 67, 33, a_off=1) == ['generic64'] == e(dt, od, ta, tb, 65, 67, 33, b_off=1)
                    assert e(dt, od, ta, tb, 2049, 2560, 40) == ['generic128']          # 17 x 20 = 340 tiles
                    assert e(dt, od, ta, tb, 2560, 2048, 40) == ['generic128']          # 20 x 16 = 320: the threshold
                    assert e(dt, od, ta, tb, 2560, 1920, 40) == ['generic64']           # 300 tiles of 128, 1200 of 64
    # split-K: S as the rule gives it
    def plan(dt, ta, tb, K, **kw):
        lda, ldb = (64 if ta else K), (K if tb else 64)
        return gemm_plan(dt, 'f32', ta, tb, 64, 64, K, kw.get('lda', lda), kw.get('ldb', ldb), 72, 0, 0, 0, None, None, 64,
                         False, kw.get('room', ROOM), 0, 1)
    for ta in (0, 1):
        for tb in (0, 1):
            assert [plan('f32', ta, tb, K)['S'] for K in (512, 1024, 1536, 1000)] == [4, 8, 12, 7]
            assert [plan('f32', ta, tb, K)['kchunk'] for K in (512, 1024, 1536, 1000)] == [128, 128, 128, 160]
            assert all(plan('f32', ta, tb, K)['keys'] == ['generic64_splitk'] for K in (512, 1024, 1536, 1000))
            assert plan('f32', ta, tb, 511)['keys'] == ['generic64'] and plan('bf16', ta, tb, 1023)['keys'] == ['generic64']
            if (ta, tb) != (1, 0):
                assert [plan('bf16', ta, tb, K)['S'] for K in (1024, 2048, 1999)] == [4, 8, 7]
                assert [plan('bf16', ta, tb, K)['kchunk'] for K in (1024, 2048, 1999)] == [256, 256, 320]
    assert plan('bf16', 1, 0, 2048)['keys'] == ['tn_lean'] and plan('bf16', 1, 0, 1999)['keys'] == ['generic64_splitk']
    assert plan('f32', 0, 1, 1000, lda=1128, ldb=1128)['S'] == 7
    assert plan('f32', 0, 0, 1536, room=5 * 64 * 64 * 4)['S'] == 5          # the slabs must fit the scratch
    assert plan('f32', 0, 0, 1536, room=64 * 64 * 4)['keys'] == ['generic64']
    for (dt, K), S in SPLITK_S.items():
        assert plan(dt, 1, 1, K)['S'] == S


def test_dispatch_rule_at_the_lean_nt_shapes():
    nt = lambda *s, **kw: e('bf16', kw.pop('od', 'f32'), 0, 1, *s, **kw)                 # noqa: E731
    for s in [(1024, 128, 64), (1025, 128, 64), (1024, 256, 64), (1151, 256, 192), (1032, 384, 128)]:
        assert nt(*s) == ['nt128'] == nt(*s, od='bf16')
        assert nt(*s, bias=0, mul=0) == ['nt128'] == nt(*s, bias=0, drop=True, ldc=s[1], c_off=0)
        assert nt(*s, big=0) == ['nt128'] == nt(*s, big=2)
    g = ['generic64']
    assert nt(1023, 128, 64) == g and nt(1024, 192, 64) == g and nt(1024, 128, 96) == g
    assert nt(1024, 128, 64, lda=68) == g and nt(1024, 128, 64, a_off=1) == g and nt(1024, 128, 64, b_off=1) == g
    assert nt(1024, 128, 64, ldc=137) == g and nt(1024, 128, 64, c_off=2) == g
    assert nt(1024, 128, 64, bias=1) == g and nt(1024, 128, 64, bias=4) == ['nt128']
    assert nt(1023, 128, 64, mul=0) == g + ['mul_pass'] and nt(1023, 128, 64, drop=True, ldc=128, c_off=0) == g + ['drop_pass']
    assert nt(1024, 128, 64, mul=0, ldm=129) == g + ['mul_pass'] and nt(1024, 128, 64, mul=1) == g + ['mul_pass']
    assert e('bf16', 'f32', 0, 0, 1024, 128, 64) == g and e('bf16', 'f32', 1, 1, 1024, 128, 64) == g
    assert e('f32', 'f32', 0, 1, 1024, 128, 64) == g
    # the large tiles: from 512 tiles of 256 x 256 by default, from M >= 2048 with the switch at 2, never at 0
    for s in WORKER_SHAPES:
        assert nt(*s) == ['nt128'] == nt(*s, big=0) and nt(*s, big=2) == ['nt256'] == nt(*s, big=2, od='bf16')
    assert nt(2047, 256, 64, big=2) == ['nt128'] and nt(2048, 384, 64, big=2) == ['nt128']
    assert nt(66000, 512, 128) == ['nt256'] and nt(65280, 512, 128) == ['nt128'] and nt(66000, 512, 128, big=0) == ['nt128']


def test_dispatch_rule_at_the_lean_tn_shapes():
    def plan(M, N, K, **kw):
        return gemm_plan('bf16', kw.get('od', 'f32'), 1, 0, M, N, K, kw.get('lda', M), N, N + 8, 0, kw.get('b_off', 0), 0,
                         None, None, N, False, kw.get('room', ROOM), kw.get('tn_wgs', 0), 1)
    shapes = [(8, 8, 2048), (136, 264, 2048), (128, 128, 2112), (64, 64, 4099)]
    assert all(plan(*s)['keys'] == ['tn_lean'] == plan(*s, od='bf16')['keys'] for s in shapes)
    assert [plan(*s)['S'] for s in shapes] == [8, 8, 9, 17]
    assert [plan(*s)['kchunk'] for s in shapes] == [256, 256, 256, 256]
    assert [plan(*s, tn_wgs=32)['S'] for s in shapes] == [8, 6, 9, 17]
    assert plan(136, 264, 2048, tn_wgs=32)['kchunk'] == 384
    sk = ['generic64_splitk']
    assert plan(8, 8, 2047)['keys'] == sk and plan(12, 8, 2048)['keys'] == sk and plan(8, 8, 2048, lda=12)['keys'] == sk
    assert plan(8, 8, 2048, b_off=1)['keys'] == sk
    assert plan(136, 264, 2048, room=3 * 136 * 264 * 4)['S'] == 3
    assert plan(2048, 2048, 2048, room=2048 * 2048 * 4 - 1)['keys'] == ['generic64']      # no room for one slab: not lean


def test_the_case_lists_are_what_the_rule_says_of_them():
    for group, cases in CASES.items():
        for case, forms, kernel in cases:
            if kernel is None:
                continue
            for form in forms:
                keys = case.expect(form, 'f32', ROOM)
                assert keys[0] == kernel, (group, case.tag(), form, keys)
    default = predicted_counters(ROOM)
    assert default == set(ALL_KEYS) - {'nt256'}
    assert predicted_counters(ROOM, 2) == {'nt256'} and predicted_counters(ROOM, 0) == {'nt128'}
    for counter, (case, forms) in GAUSSIAN.items():
        assert any(counter in case.expect(f, 'f32', ROOM) for f in forms), counter


@pytest.mark.parametrize('group', sorted(g for g, cases in CASES.items() if any(c.K >= 512 for c, _, _ in cases)))
def test_the_integer_data_is_exact_and_large(group):
    """host_data asserts it: every partial sum below 2^24, and from K = 512 on at least half of the reference above 256
    in magnitude (a bf16 accumulator holds integers up to 256 only), with the seeds the GPU tests use."""
    seen = set()
    for case, _, _ in CASES[group]:
        if case.K >= 512 and case.seed() not in seen:
            seen.add(case.seed())
            host_data(case, 'exact')
