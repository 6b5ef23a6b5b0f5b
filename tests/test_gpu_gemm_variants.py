"""The GEMM (csrc/gemm.hip) at every kernel launch_gemm can end in, each call with the kernel that ran asserted
(ops.gemm_kernel_counts against the dispatch rule restated in tests/_gemm_variants.py) and the result compared with an
fp64 reference: bit for bit on integer data, per element on gaussian data (bounds: the docstring of _gemm_variants).

Every case runs plain, + bias, accumulating onto a non-zero C, and with bias + accumulate + ReLU (about half of the entries
negative), with an fp32 and with a bf16 result; 'mul' and 'drop' (fp32 result only) where listed.  C sits in a guard
frame.  The shapes (M, N, K), each the smallest that reaches its path (the lists: CASES of _gemm_variants):

skinny fp32 kernel (M <= 32, K % 64 == 0, no transA), K in 64-element units over eight waves: one round up to 8 units,
two rounds 9..16, 17 pads to four rounds with the fourth past the end (re-read, multiplied by keep = 0)
  NN32 (N % 32 == 0):            (17, 32, 64) 1 unit, ragged second row group; (16, 32, 512) 8 units; (32, 64, 576) 9;
                                 (15, 96, 1024) 16; (1, 32, 1088) 17
  NN16 (N % 16 == 0, not 32):    (17, 48, 64), (32, 16, 576), (1, 80, 1088)
  NT16 (transB, N < 6144):       (17, 16, 64), (32, 48, 1088)
  NT32 (transB, N >= 6144):      (17, 6144, 64), (32, 6144, 576)
  with a bf16 result the same shapes must take the generic kernel (the skinny kernel stores fp32 only)
  refused -> generic 64 x 64:    M = 33; K = 96; N = 24; transA; lda = K + 1; A one element into its buffer; B one element
                                 in; transB with ldb = K + 2
generic 64 x 64, four layouts, both operand types: (1, 1, 1); (65, 67, 33) ragged in M, N and K, ldc % 4 != 0 (scalar
  epilogue); (64, 64, 64) everything aligned (vector epilogue, the four-wide bf16 accumulate); (65, 67, 33) with A, then
  B, one element off the 16-byte boundary (the element-wise loader)
generic split-K at (64, 64, K), one output tile: fp32 K = 512 / 1024 / 1536 / 1000 -> 4 / 8 / 12 (the reducer's
  eight-at-a-time loop and its tail) / 7 slabs (last chunk 40 wide); bf16 K = 1024 / 2048 / 1999 -> 4 / 8 / 7, in the
  layouts the lean TN kernel refuses; once each with NaN behind every operand row as far as a full last chunk would
  reach (a chunk that ran past K reads them).  bias, accumulate and ReLU are the reducer's
generic 128 x 128 (>= 320 tiles): (2049, 2560, 40), 340 tiles, ragged last M tile, K below one k-tile -- fp32 and bf16,
  four layouts (bf16 NT: K % 64 != 0 keeps it off the lean kernel); (2560, 2048, 40): exactly 320 tiles
lean NT 128 x 128 (bf16, NT, M >= 1024, N % 128 == 0, K % 64 == 0): (1024, 128, 64) 8 tiles; (1025, 128, 64) 9, one row
  in the last; (1024, 256, 64) 16: the XCD remap of tile counts that are multiples of 8; (1151, 256, 192) 18 and
  (1032, 384, 128) 27: the counts that are not.  Also with a multiplier and with dropout in the epilogue
  refused -> generic 64 x 64 (+ the multiply / dropout pass): M = 1023; N = 192; K = 96; lda = K + 4; A one element in;
  ldc % 4 != 0; bias one float in; mul with ldm % 4 != 0; mul one float in.  mul / drop with a bf16 result: ValueError
lean TN (bf16, TN, K >= 2048, M and N multiples of 8), always split-K: (8, 8, 2048) one 8 x 8 corner of a tile;
  (136, 264, 2048) 2 x 3 tiles, ragged both ways; (128, 128, 2112) 9 slabs, the last 64 wide; (64, 64, 4099) odd K, 17
  slabs, the last 3 wide.  Again on a side lane asking for 32 workgroups (6 slabs instead of 8 at the second shape) and
  with the first two XCDs skipped: the same exact results
  refused -> generic split-K: K = 2047; M = 12; lda = M + 4
256 x 256 NT kernel at small shapes: fresh child processes with ASR_GEMM_NT_BIG=2 and =0 (read once per process),
  (2048, 256, 64), (2049, 512, 128), (2303, 256, 192): tests/_gemm_variant_worker.py

Left out: the fits32 fallback of the 256 x 256 kernel (an operand of 4 GiB or more: not a few-second test).  The
listed-row and tn-frames forms have files of their own (test_gpu_valid_rows.py, test_gpu_tn_frames.py)."""
import json
import os
import subprocess
import sys

import pytest
import torch

from _gemm_variants import (ALL_KEYS, CASES, GAUSSIAN, GAUSSIAN_MORE, KERNEL_KEYS, SPLITK_S, Case, Tally, check_product,
                            device_limits, nt_big_switch, predicted_counters)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = nt_big_switch(os.environ)

PARAMS = []
for _g, _cases in CASES.items():
    if _g.startswith('generic128'):                        # 21 MB results: one test per case
        PARAMS += [(_g, i) for i in range(len(_cases))]
    else:
        PARAMS.append((_g, None))


def _ops():
    from tensorflow_end2end_speech_recognition_amd import ops
    return ops


@pytest.mark.parametrize('group,index', PARAMS, ids=['%s%s' % (g, '' if i is None else '-%d' % i) for g, i in PARAMS])
def test_exact_products(cuda, group, index):
    """Integer data: every result equals the fp64 reference (its bf16 rounding for a bf16 result), every call ran the
    kernel the rule predicts, and the fp32-output calls of a case the kernel its list names."""
    room = device_limits()
    tally = Tally()
    cases = CASES[group] if index is None else [CASES[group][index]]
    for case, forms, kernel in cases:
        if kernel is not None:
            for form in forms:
                keys = case.expect(form, 'f32', room, 0, BIG)
                assert keys[0] == kernel, (case.tag(), form, keys)
                assert keys[1:] == ([] if kernel.startswith('nt') else {'mul': ['mul_pass'], 'drop': ['drop_pass']}.get(form, []))
            if kernel.startswith('skinny'):                # a bf16 result: not the skinny kernel
                assert all(case.expect(f, 'bf16', room)[0].startswith('generic64') for f in forms)
        if group.startswith('splitk'):
            assert case.plan('relu', 'bf16', room)['S'] == SPLITK_S[(case.dtype, case.K)], case.tag()
        check_product(tally, case, forms, scratch_room=room, big=BIG)
    assert _ops().check_async_errors(0) == 0


def test_partly_refused_lean_nt(cuda):
    """The lean NT conditions that concern one argument only: the calls that pass it fall to the generic kernel (+ the
    second pass), the others stay on the lean kernel."""
    room = device_limits()
    e = lambda form, **kw: Case('bf16', 0, 1, 1024, 128, 64, **kw).expect(form, 'f32', room, 0, BIG)    # noqa: E731
    assert e('plain', bias_off=1) == ['nt128'] and e('bias', bias_off=1) == ['generic64']
    assert e('mul', bias_off=1) == ['generic64', 'mul_pass'] and e('drop', bias_off=1) == ['generic64', 'drop_pass']
    for kw in (dict(ldm=129), dict(mul_off=1)):
        assert e('mul', **kw) == ['generic64', 'mul_pass'] and e('drop', **kw) == ['nt128'] and e('relu', **kw) == ['nt128']


def test_multiplier_with_a_bf16_result_is_rejected(cuda):
    ops = _ops()
    A = torch.zeros(1024, 64, dtype=torch.bfloat16, device=cuda)
    Bt = torch.zeros(128, 64, dtype=torch.bfloat16, device=cuda)
    with pytest.raises(ValueError):
        ops.gemm(A, Bt, transB=True, out_dtype='bf16', mul=torch.ones(1024, 128, device=cuda))
    with pytest.raises(ValueError):
        ops.gemm(A, Bt, transB=True, out_dtype='bf16', drop=(0.5, 1, 0))


@pytest.mark.parametrize('knob', ['workgroups_32', 'xcd_skip_2'])
def test_lean_tn_on_a_side_lane(cuda, knob):
    """The lean TN shapes on side lane 1 with asr_set_gemm_tn_workgroups = 32 (another slab count where the K bound does
    not decide it) / with the first two XCDs left alone: the same exact results.  The defaults are restored."""
    ops = _ops()
    room = device_limits()
    wgs = 32 if knob == 'workgroups_32' else 0
    plans = [(c.plan('plain', 'f32', room)['S'], c.plan('plain', 'f32', room, wgs)['S']) for c, _, _ in CASES['tn_lean']]
    assert plans == ([(8, 8), (8, 6), (9, 9), (17, 17)] if wgs else [(8, 8), (8, 8), (9, 9), (17, 17)])
    tally = Tally()
    try:
        if wgs:
            ops.set_side_gemm_workgroups(cuda, 32)
        else:
            ops.set_side_xcd_skip(cuda, 2)
        for case, forms, _ in CASES['tn_lean']:
            assert case.expect('plain', 'f32', room, wgs) == ['tn_lean']
            check_product(tally, case, forms, scratch_room=room, tn_wgs=wgs, big=BIG, side=True)
    finally:
        ops.set_side_gemm_workgroups(cuda, 0)
        ops.set_side_xcd_skip(cuda, 0)
    torch.cuda.synchronize()
    assert ops.check_async_errors(0) == 0


@pytest.mark.parametrize('counter', sorted(GAUSSIAN) + ['more'])
def test_gaussian_products(cuda, counter):
    """randn operands, once per counter (and the bf16 forms of the generic kernels): see the docstring of _gemm_variants."""
    room = device_limits()
    tally = Tally()
    for case, forms in ([GAUSSIAN[counter]] if counter != 'more' else GAUSSIAN_MORE):
        seen = check_product(tally, case, forms, regime='gaussian', scratch_room=room, big=BIG)
        assert counter == 'more' or counter in seen, (counter, seen)


# ---------------------------------------------------------------- the 256 x 256 NT kernel behind its switch
_CHILD_FAULT = []
_CHILD_RESULTS = {}


@pytest.mark.parametrize('big', ['2', '0'])
def test_switched_nt_kernels_in_a_fresh_process(cuda, big):
    """tests/_gemm_variant_worker.py under ASR_GEMM_NT_BIG = 2 (256 x 256 tiles from M >= 2048) and = 0 (128 x 128 tiles
    always): the worker checks its shapes exactly, with the counters of every call; here, that the switched kernel is the
    one that ran, and that the two processes' fp32 results are the same bits."""
    if _CHILD_FAULT:
        pytest.fail('not started: the child of ASR_GEMM_NT_BIG=%s ended on a fault or the time limit' % _CHILD_FAULT[0])
    env = dict(os.environ, ASR_GEMM_NT_BIG=big, PYTHONPATH=ROOT)
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_gemm_variant_worker.py')], env=env,
                           capture_output=True, text=True, timeout=240)
    except subprocess.TimeoutExpired as e:
        _CHILD_FAULT.append(big)
        pytest.fail('ASR_GEMM_NT_BIG=%s: the child did not finish in %d s\n%s' % (big, e.timeout, str(e.stderr)[-2000:]))
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or 'illegal memory access' in r.stderr \
            or 'HSA_STATUS_ERROR' in r.stderr:
        _CHILD_FAULT.append(big)
    assert r.returncode == 0, (big, r.returncode, r.stdout[-3000:], r.stderr[-4000:])
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith('GEMM ')][-1][len('GEMM '):])
    counts = res['counts']
    on, off = ('nt256', 'nt128') if big == '2' else ('nt128', 'nt256')
    assert counts[on] > 0 and counts[off] == 0, (big, counts)
    assert all(counts[k] == 0 for k in ALL_KEYS if k not in ('nt128', 'nt256')), (big, counts)
    _CHILD_RESULTS[big] = res['digests']
    if len(_CHILD_RESULTS) == 2:
        assert _CHILD_RESULTS['2'] == _CHILD_RESULTS['0'] and len(res['digests']) == 18


# ---------------------------------------------------------------- coverage of the counters
def test_the_cases_of_this_file_reach_every_counter(cuda):
    """Every call above is asserted against the rule, so the counters this file reaches are the ones the rule predicts for
    its case lists: in this process with the default switch, in the child with ASR_GEMM_NT_BIG=2.  They must be all."""
    room = device_limits()
    default = predicted_counters(room)
    assert default == set(ALL_KEYS) - {'nt256'}, sorted(set(ALL_KEYS) ^ default)
    assert predicted_counters(room, 2) == {'nt256'} and predicted_counters(room, 0) == {'nt128'}
    assert set(GAUSSIAN) | {'nt256'} == set(ALL_KEYS) and set(KERNEL_KEYS) < set(ALL_KEYS)
