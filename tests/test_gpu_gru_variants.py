"""The GRU recurrence (csrc/gru.hip and the two GRU cluster kernels of csrc/gru_cluster.hip) at every form asr_gru_fwd and
asr_gru_bwd can end in -- clusters of H / 32 CUs, the persistent single-CU kernel, the launch-per-step kernels -- each
device call between a reset of ops.gru_kernel_counts and an assert that exactly the counter the dispatch rule predicts
(tests/_gru_variants.py::expected_form) moved by one, and every result compared with a float64 reference written apart
from the rest of the suite (gru_reference, held against the oracle in tests/test_gru_variants_host.py).

Cases (CASES of _gru_variants, each the smallest that reaches its path; B a multiple of 16, T <= 40):
  cluster:     H = 64 / 128 / 256 / 320 x (ndir, B) = (2, 16), (1, 32), (2, 48)
  persistent:  H = 16 (one k-group of gp_tile), 48 (tail loop only), 144 (one chunk + one group; the backward gates'
               K = 2H: two chunks + two), 496 (the largest persistent backward: 159 744 bytes of LDS), 512 (forward
               persistent, backward per step on what the persistent forward saved); with ASR_GRU_CLUSTER=0 also 64, 128, 320
  per step:    asr_debug_set_gru_persistent(0) at H = 16, 48, 128, 320; the switch left on at H = 528
  mixed:       H = 128: per-step forward -> persistent / cluster backward, persistent forward -> per-step backward
  edges:       T = 1; tmax = max(seq_len) < T beside tmax = T; no final-state gradient -- on every form
  lengths:     row 0 full, row 1 of length 1, row 2 empty, the rest ragged; for B >= 32 a whole 16-row tile empty

Bounds: 8 E32 per case and tensor (E32: the float32 evaluation of the reference against the float64 one), never above 1e-5
forward / 2e-5 for gradients -- the docstring of _gru_variants.  r, u, c are compared at the frames a row worked on (past
them they are unspecified), rh, hout, dgate and dcand everywhere, and they must be exact zeros outside.

Measured worst error / E32 per form and pass, over every case and tensor (one MI355X; the tests print every figure with
-s, the last test the maxima; the bound is 8):
  cluster     forward 3.08 (c at T = 1, H = 128)          backward 2.54
  persistent  forward 2.07                                backward 1.86
  per step    forward 3.89 (r * h at H = 528)             backward 5.74 (dcand at H = 512; 4.0 - 4.8 at H = 128 .. 528)
The per-step kernels sum each product as one serial chain of K fp32 FMAs, the float32 yardstick in blocks: the widest
products sit highest, all under the margin, which therefore stands unwidened.

Left out: T >= 65536 (the clusters' 16-bit step tags hand such a call to the single-CU forms: not a few-second test), and
tile groups, which tests/test_gpu_tile_groups.py holds bit for bit against one launch."""
import contextlib
import os

import numpy as np
import pytest
import torch

from _gru_variants import (ALL_CASES, BWD_TENSORS, CASES, COUNTER_KEYS, FWD_TENSORS, SETUPS, XCH_BYTES, bound, case_data,
                           case_form, cluster_env_on)

pytestmark = pytest.mark.gpu

# worst error / E32 seen per (form, pass), over every case and tensor of that form (bound: 8)
MEASURED = {}


def _ops():
    from tensorflow_end2end_speech_recognition_amd import ops
    return ops


def _limits():
    from tensorflow_end2end_speech_recognition_amd import _lib
    h = _lib.handle(0)
    return dict(num_cu=torch.cuda.get_device_properties(0).multi_processor_count,
                scratch_room=int(h.lib.asr_scratch_bytes(h.h)) - XCH_BYTES)


@pytest.fixture
def gru(cuda, monkeypatch):
    """Runs one pass of a case under its set-up with the counter asserted; restores the switch."""
    ops = _ops()
    ops.debug_set_cluster_cu_budget(0)
    lim = _limits()

    @contextlib.contextmanager
    def counted(case, pass_):
        switch, env = SETUPS[getattr(case, pass_)]
        ops.debug_set_gru_persistent(1 if switch else 0)
        if env is None:
            monkeypatch.delenv('ASR_GRU_CLUSTER', raising=False)
        else:
            monkeypatch.setenv('ASR_GRU_CLUSTER', env)
        form = case_form(case, pass_, cluster_env_on(os.environ), **lim)
        ops.reset_gru_kernel_counts(0)
        yield form
        got = ops.gru_kernel_counts(0)
        want = {k: int(k == '%s_%s' % (pass_, form)) for k in COUNTER_KEYS}
        assert got == want, (case.name, pass_, form, got)

    class Runner(object):
        def upload(self, case):
            inp = case_data(case.name)['inp']
            dev = {k: torch.tensor(v, device=cuda) for k, v in inp.items() if v is not None}
            dev['dhf'] = dev.get('dhf')
            dev['wghT'], dev['wchT'] = dev['wgh'].transpose(1, 2).contiguous(), dev['wch'].transpose(1, 2).contiguous()
            return dev

        def fwd(self, case, dev, tmax=None):
            with counted(case, 'fwd') as form:
                out = ops.gru_fwd(dev['xg'], dev['xc'], dev['wgh'], dev['wch'], dev['sl'],
                                  case.T if tmax is None else tmax, case.H, case.ndir)
            return out, form

        def bwd(self, case, dev, saved, tmax=None):
            with counted(case, 'bwd') as form:
                dg, dc = ops.gru_bwd(dev['dout'], dev['dhf'], saved, dev['wghT'], dev['wchT'], dev['sl'],
                                     case.T if tmax is None else tmax, case.H, case.ndir)
            return dict(dgate=dg, dcand=dc), form

    yield Runner()
    ops.debug_set_gru_persistent(1)


def _check(case, got, tensors, form, pass_):
    """Every tensor within 8 E32 of the float64 reference where it is specified, exact zeros where nothing is active."""
    data = case_data(case.name)
    valid = data['valid']
    for k in tensors:
        a, ref = got[k].cpu().numpy().astype(np.float64), data['ref'][k]
        if k != 'h_final':
            if k in ('rh', 'hout', 'dgate', 'dcand'):
                assert np.abs(np.where(valid, 0.0, a)).max() == 0.0, (case.name, form, k, 'not zero past a length')
            a = np.where(valid, a, 0.0)                    # r, u, c past a row's length: unspecified
        assert np.isfinite(a).all(), (case.name, form, k)
        err, e32 = float(np.abs(a - ref).max()), data['e32'][k]
        ratio = err / e32 if e32 > 0 else 0.0
        print('GRU-VARIANT %-16s %s %-10s %-7s err %.3e E32 %.3e ratio %.2f' % (case.name, pass_, form, k, err, e32, ratio))
        MEASURED[(form, pass_)] = max(MEASURED.get((form, pass_), 0.0), ratio)
        assert err <= bound(data, k), (case.name, form, k, err, e32)
    if pass_ == 'bwd':
        assert all(np.abs(data['ref'][k]).max() > 0.1 for k in tensors)


_IDS = [c.name for c in ALL_CASES]


@pytest.mark.parametrize('case', ALL_CASES, ids=_IDS)
def test_forward_against_fp64(gru, case):
    """r, u, c, r * h at the frames a row worked on, hout everywhere, the final state; with pad > 0 also tmax =
    max(seq_len): the same bits, hout zero from tmax on."""
    dev = gru.upload(case)
    out, form = gru.fwd(case, dev)
    _check(case, out, FWD_TENSORS, form, 'fwd')
    if case.pad:
        tmax = case.T - case.pad
        short, _ = gru.fwd(case, dev, tmax)
        _check(case, short, FWD_TENSORS, form, 'fwd')
        valid = torch.tensor(case_data(case.name)['valid'], device=dev['xg'].device)
        for k in FWD_TENSORS:
            a, b = out[k], short[k]
            if k in ('r', 'u', 'c'):
                a, b = torch.where(valid, a, torch.zeros_like(a)), torch.where(valid, b, torch.zeros_like(b))
            assert torch.equal(a, b), (case.name, k)
        assert float(short['hout'][tmax:].abs().max()) == 0.0
    assert _ops().check_async_errors(0) == 0


@pytest.mark.parametrize('case', ALL_CASES, ids=_IDS)
def test_backward_against_fp64(gru, case):
    """dgate, dcand of the device backward on what the device forward saved, against the float64 gradients; exact zeros
    wherever no row is active; with pad > 0 also tmax = max(seq_len): the same bits."""
    dev = gru.upload(case)
    saved, _ = gru.fwd(case, dev)
    got, form = gru.bwd(case, dev, saved)
    _check(case, got, BWD_TENSORS, form, 'bwd')
    if case.pad:
        short, _ = gru.bwd(case, dev, saved, case.T - case.pad)
        assert all(torch.equal(got[k], short[k]) for k in BWD_TENSORS), case.name
    assert _ops().check_async_errors(0) == 0


@pytest.mark.parametrize('case', ALL_CASES, ids=_IDS)
def test_backward_never_reads_saved_activations_of_padded_frames(gru, case):
    """r, u, c at frames at or past a row's length are unspecified: with NaN there the backward of every form gives
    finite results, bit for bit those of the unpoisoned run."""
    dev = gru.upload(case)
    saved, _ = gru.fwd(case, dev)
    clean, form = gru.bwd(case, dev, saved)
    padded = ~torch.tensor(case_data(case.name)['valid'], device=dev['xg'].device)            # [T,B,1]
    assert bool(padded.any())
    poisoned = dict(saved)
    for k in ('r', 'u', 'c'):
        poisoned[k] = torch.where(padded, torch.full_like(saved[k], float('nan')), saved[k])
        assert bool(torch.isnan(poisoned[k]).any())
    got, form2 = gru.bwd(case, dev, poisoned)
    assert form2 == form
    for k in BWD_TENSORS:
        assert bool(torch.isfinite(got[k]).all()), (case.name, form, k)
        assert torch.equal(got[k], clean[k]), (case.name, form, k)
    assert _ops().check_async_errors(0) == 0


def test_cluster_launches_back_to_back(gru):
    """The cluster cases queued with no synchronisation between them, in an order that alternates width, B, T and pass
    (the two exchange areas alternate between launches and each launch zeroes what its predecessor dirtied: stale tags of
    a differently shaped predecessor are what could go wrong); results are fetched at the end and meet their bounds."""
    cases = CASES['cluster']
    order = [cases[i] for i in (0, 10, 5, 6, 2, 9, 4, 11, 1, 8, 3, 7)]           # 64 / 320 / 128 / 256 ..., B and T mixed
    assert sorted(c.name for c in order) == sorted(c.name for c in cases)
    devs = {c.name: gru.upload(c) for c in order}
    torch.cuda.synchronize()
    fwd, bwd, prev = {}, {}, None
    for c in order:                                                              # fwd(c), bwd(previous case), fwd(next) ...
        fwd[c.name], form = gru.fwd(c, devs[c.name])
        assert form == 'cluster'
        if prev is not None:
            bwd[prev.name], form = gru.bwd(prev, devs[prev.name], fwd[prev.name])
            assert form == 'cluster'
        prev = c
    bwd[prev.name], _ = gru.bwd(prev, devs[prev.name], fwd[prev.name])
    for c in order:
        _check(c, fwd[c.name], FWD_TENSORS, 'cluster', 'fwd')
        _check(c, bwd[c.name], BWD_TENSORS, 'cluster', 'bwd')
    assert _ops().check_async_errors(0) == 0


def test_the_case_lists_reach_all_six_forms(cuda):
    """From the rule, with this device's CU count and scratch: every counter of ops.gru_kernel_counts is some case's."""
    lim = _limits()
    env = cluster_env_on({k: v for k, v in os.environ.items() if k != 'ASR_GRU_CLUSTER'})
    reached = {'%s_%s' % (p, case_form(c, p, env, **lim)) for c in ALL_CASES for p in ('fwd', 'bwd')}
    assert reached == set(COUNTER_KEYS) == set(_ops().gru_kernel_counts(0)), reached
    for (form, pass_), ratio in sorted(MEASURED.items()):
        print('GRU-VARIANT worst error / E32: %-10s %s %.2f' % (form, pass_, ratio))
