"""The LSTM recurrence (csrc/lstm.hip, csrc/lstm_cluster*.hip) at every form asr_lstm_fwd and asr_lstm_bwd(_ex) can end in
-- the bf16 clusters of 16 / 32 / 64 units per CU, the fp32 three-term split, the exact fp32 clusters of 32 / 64 units per
CU, the single-CU kernels of both dtypes; fifteen counters -- each device call between a reset of ops.lstm_kernel_counts
and an assert that exactly the counter the dispatch rule predicts (tests/_lstm_variants.py::expected_form) moved by one,
and every result compared with a float64 reference written apart from the rest of the suite (lstm_forward /
lstm_backward, held against the oracle in tests/test_lstm_variants_host.py).

Cases (CASES of _lstm_variants, each the smallest that reaches its path; B in {16, 32, 48}, T <= 40, reached in-process by
asr_debug_set_lstm_flags bits 9, 13, 12, 10, 11, 5, 4, asr_debug_set_cluster_cu_budget and clip_no_grad):
  cluster:     16-CU 256; bf16 32-unit 256, 512; bf16 64-unit 256, 320, 512; split 128, 256; exact-32 128, 256, 320, 512;
               exact-64 128 -- every form at (ndir, B) = (2, 16), (1, 32), (2, 48)
  single:      both dtypes at 64, 128, 192, 256, 320, 512 (the cluster widths under a CU budget of 1), (2, 16) and (1, 32)
  ladder:      H = 256 bf16 at budgets 128, 127, 64, 63, 32, 31 (16-CU -> 32-unit -> 64-unit -> single-CU; the BPTT from the
               32-unit form down), H = 256 fp32 at 64, 63 (split -> single-CU)
  mixed:       16-CU forward -> 64-unit BPTT (-> 32-unit is the default pairing of every 16-CU case); single-CU forward ->
               cluster BPTT and the reverse in both dtypes; split forward -> exact BPTT and the reverse
  variants:    EARLY inverted, 8-byte exchange granules, the other BPTT slot layout, write-through -- one width per form
  clip_block:  clip_no_grad with 35 % of the valid states clamped, on every backward form
  edges:       T = 1, 2, 3; max(seq_len) = 37 and 36; max(seq_len) = T - 3; no peepholes; an active forward clip; no
               final-state gradients -- on every form; want_dpeep=False in every backward test (same dgates bits)
  lengths:     row 0 full, row 1 of length 1, row 2 empty, the rest ragged; for B >= 32 a whole 16-row tile empty (tmax = 0
               in its workgroups: final states, hout, dgates and its dpeep partial are exact zeros)

Bounds (the docstring of _lstm_variants).  fp32 forms: 8 E32 per case and tensor, never above 1e-5 max(1, max|ref|); the
whole chain against the reference's own forward.  bf16 forms: BF16_BOUNDS, the bounds of
test_lstm_cluster_bf16_gradient_parity_headline_shapes unchanged; the backward against lstm_backward fed the device's
saved activations, masked at padded frames.  Saved gates and cs are compared at the frames a row worked on (past them
they are unspecified), hout and dgates everywhere, and they must be exact zeros outside.

Measured on one MI355X, worst over every case of a form (the tests print every figure with -s, the last test the maxima
per form and pass).  fp32 forms, error / E32 (the bound is 8; no form needed it widened):
  split        forward 2.22   backward 2.57
  exact-32     forward 2.25   backward 2.06
  exact-64     forward 2.41   backward 2.06
  single-CU    forward 4.51 (c_final at H = 256; gates 4.07 at H = 128)   backward 3.66 (dgates at H = 192, tmax = 36)
The single-CU kernels sit highest (they sum all K = H products of a unit in one chain of MFMA accumulations, where the
clusters add per-CU partial sums of H / G products), still under the margin.  bf16 forms, worst max / mean against their bounds:
  form       hout max / mean    gates max / mean   cs max rel / mean   c_final  h_final | dgates max / mean rel  dpeep    db
  16-CU      3.9e-3 / 2.4e-6    3.9e-3 / 7.9e-6    2.4e-4 / 1.4e-5     6.1e-4   2.8e-4  | (forward only)
  32-unit    3.9e-3 / 4.4e-6    3.9e-3 / 2.6e-5    6.1e-4 / 4.7e-5     1.2e-3   7.8e-4  | 4.9e-3 / 1.7e-4        3.9e-4   2.7e-4
  64-unit    3.9e-3 / 1.7e-6    3.9e-3 / 3.3e-6    3.4e-4 / 5.7e-6     8.9e-4   6.0e-4  | 3.4e-3 / 6.8e-5        2.1e-4   1.5e-4
  single-CU  2.0e-3 / 3.6e-7    3.9e-3 / 1.0e-6    1.1e-4 / 1.3e-6     2.2e-4   1.2e-4  | 1.9e-3 / 7.5e-6        6.1e-5   5.0e-5
  bound      7.8e-3 / 2.0e-4    1.6e-2 / 3.5e-4    2.0e-2 / 8.0e-4     2.0e-2   5.0e-3  | 1.5e-2 / 2.5e-3        4.0e-3   3.0e-3
(every max on hout and gates is one bf16 ulp, 2^-8: a value on a rounding boundary that fell the other way).

Left out: T >= 65536 (the forward split's 16-bit step tags hand such a call to the exact kernel: not a few-second test),
tile groups (tests/test_gpu_tile_groups.py holds them bit for bit against one launch), the ASR_LSTM_ABLATE builds."""
import contextlib
import os

import numpy as np
import pytest
import torch

import _gru_variants as G
from _lstm_variants import (ALL_CASES, BF16_BOUNDS, BWD_TENSORS, CASES, CLUSTER_FORMS, COUNTER_KEYS, FWD_TENSORS,
                            bf16_bwd_figures, bf16_fwd_figures, bf16_round, bound, case_data, case_form, lstm_backward)

pytestmark = pytest.mark.gpu

# fp32 forms: worst error / E32 seen per (form, pass); bf16 forms: worst of each bounded figure per (form, pass)
MEASURED = {}
DIN = 16                                  # rows of the kernel above W_h (asr_lstm_prep_weights wants Din > 0): zeros


def _ops():
    from tensorflow_end2end_speech_recognition_amd import ops
    return ops


def _limits():
    from tensorflow_end2end_speech_recognition_amd import _lib
    h = _lib.handle(0)
    return dict(num_cu=torch.cuda.get_device_properties(0).multi_processor_count,
                scratch_bytes=int(h.lib.asr_scratch_bytes(h.h)))


@pytest.fixture
def lstm(cuda):
    """Runs one pass of a case under its flags and CU budget with the counter asserted; restores both."""
    ops = _ops()
    from tensorflow_end2end_speech_recognition_amd._lib import ASR_BF16, ASR_F32
    lim = _limits()

    @contextlib.contextmanager
    def counted(case, pass_):
        ops.debug_set_lstm_flags(case.fwd if pass_ == 'fwd' else case.bwd)
        ops.debug_set_cluster_cu_budget(case.fb if pass_ == 'fwd' else case.bb)
        form = case_form(case, pass_, env=os.environ, **lim)
        ops.reset_lstm_kernel_counts(0)
        yield form
        got = ops.lstm_kernel_counts(0)
        want = {k: int(k == '%s_%s' % (pass_, form)) for k in COUNTER_KEYS}
        assert got == want, (case.name, pass_, form, got)

    class Runner(object):
        def upload(self, case):
            inp = case_data(case.name)['inp']
            T, B, ndir, H = case.T, case.B, case.ndir, case.H
            dt = ASR_BF16 if case.dtype == 'bf16' else ASR_F32
            up = lambda a: None if a is None else torch.tensor(a, device=cuda)     # noqa: E731
            dev = dict(dt=dt, xproj=up(inp['xproj']).view(T, B, ndir * 4 * H), dout=up(inp['dout']).view(T, B, ndir * H),
                       peep=up(inp['peep']), dcf=up(inp['dcf']), dhf=up(inp['dhf']), sl=up(inp['sl']))
            packed = []
            for d in range(ndir):
                kernel = torch.cat([torch.zeros((DIN, 4 * H), device=cuda), up(inp['wh'][d])])
                packed.append(ops.lstm_prep_weights(kernel, torch.zeros(4 * H, device=cuda), DIN, H, dt))
            dev['pf'] = torch.stack([p['pf'] for p in packed]).contiguous()
            dev['pb'] = torch.stack([p['pb'] for p in packed]).contiguous()
            return dev

        def fwd(self, case, dev):
            with counted(case, 'fwd') as form:
                out = ops.lstm_fwd(dev['xproj'], dev['pf'], dev['peep'], dev['sl'], case.H, case.ndir, dev['dt'], 1.0, case.clip)
            return dict(zip(('gates', 'hout', 'cs', 'c_final', 'h_final'), out)), form

        def bwd(self, case, dev, saved, want_dpeep=True, ws=None):
            with counted(case, 'bwd') as form:
                dg, dp = ops.lstm_bwd(dev['dout'], saved['gates'], saved['cs'], dev['pb'], dev['peep'], dev['sl'], case.H,
                                      case.ndir, dev['dt'], dev['dcf'], dev['dhf'], want_dpeep,
                                      case.clip if case.block else 0.0, dpeep_workspace=ws)
            return dict(dgates=dg, dpeep=dp), form

    yield Runner()
    ops.debug_set_lstm_flags(0)
    ops.debug_set_cluster_cu_budget(0)


def _np(case, got):
    """Device tensors -> float64 numpy in the layouts of _lstm_variants."""
    T, B, ndir, H = case.T, case.B, case.ndir, case.H
    shapes = dict(gates=(T, B, ndir, H, 4), dgates=(T, B, ndir, H, 4), cs=(T, B, ndir, H), hout=(T, B, ndir, H))
    with np.errstate(invalid='ignore'):                      # (whatever bits the padded frames of gates and cs hold)
        return {k: v.float().cpu().numpy().astype(np.float64).reshape(shapes.get(k, tuple(v.shape)))
                for k, v in got.items() if v is not None}


def _note(form, pass_, key, val):
    m = MEASURED.setdefault((form, pass_), {})
    m[key] = max(m.get(key, 0.0), float(val))


def _check_fwd(case, got, form):
    """gates, cs at the frames a row worked on, hout everywhere and exact zeros past a length, the final states."""
    data = case_data(case.name)
    a, valid = _np(case, got), data['valid']
    assert np.abs(np.where(valid, 0.0, a['hout'])).max() == 0.0, (case.name, form, 'hout not zero past a length')
    a['gates'], a['cs'] = np.where(valid[..., None], a['gates'], 0.0), np.where(valid, a['cs'], 0.0)
    assert all(np.isfinite(a[k]).all() for k in FWD_TENSORS), (case.name, form)
    empty = [2] + (list(range(16, 32)) if case.B >= 32 else [])               # the empty row, the empty tile
    assert np.abs(a['c_final'][:, empty]).max() == 0.0 and np.abs(a['h_final'][:, empty]).max() == 0.0, (case.name, form)
    if case.clip:
        assert np.abs(a['cs']).max() == np.float32(case.clip), (case.name, form, 'the clip is not active')
    if case.dtype == 'f32':
        for k in FWD_TENSORS:
            err, e32 = float(np.abs(a[k] - data['ref'][k]).max()), data['e32'][k]
            print('LSTM-VARIANT %-28s fwd %-11s %-7s err %.3e E32 %.3e ratio %.2f' % (case.name, form, k, err, e32, err / e32))
            _note(form, 'fwd', 'ratio', err / e32)
            assert err <= bound(data, k), (case.name, form, k, err, e32)
        return
    figs = bf16_fwd_figures(a, data['refr'], valid)
    print('LSTM-VARIANT %-28s fwd %-11s %s' % (case.name, form, ' '.join('%s %.2e' % kv for kv in sorted(figs.items()))))
    for k, v in figs.items():
        _note(form, 'fwd', k, v)
    assert all(v <= BF16_BOUNDS[k] for k, v in figs.items()), (case.name, form, figs)


def _check_bwd(case, got, saved, form):
    """dgates everywhere and exact zeros past a length, the seven dpeep rows."""
    data = case_data(case.name)
    a, valid, ref, inp = _np(case, got), data['valid'], data['ref'], data['inp']
    assert np.abs(np.where(valid[..., None], 0.0, a['dgates'])).max() == 0.0, (case.name, form, 'dgates not zero past a length')
    assert all(np.isfinite(a[k]).all() for k in BWD_TENSORS), (case.name, form)
    assert np.abs(ref['dgates']).max() > 0.1 and np.abs(ref['dpeep'][:, :3]).max() > 0.1 and np.abs(ref['dpeep'][:, 3:]).max() > 0.1
    if case.dtype == 'f32':
        for k in BWD_TENSORS:
            err, e32 = float(np.abs(a[k] - ref[k]).max()), data['e32'][k]
            print('LSTM-VARIANT %-28s bwd %-11s %-7s err %.3e E32 %.3e ratio %.2f' % (case.name, form, k, err, e32, err / e32))
            _note(form, 'bwd', 'ratio', err / e32)
            assert err <= bound(data, k), (case.name, form, k, err, e32)
        return
    # dgates | device activations: the reference BPTT on what the device forward saved, padded frames masked
    s = _np(case, saved)
    r = lstm_backward(inp['dout'], np.where(valid[..., None], s['gates'], 0.0), np.where(valid, s['cs'], 0.0), inp['wh'],
                      inp['peep'], inp['sl'], case.H, case.ndir, inp['dcf'], inp['dhf'], case.clip if case.block else 0.0,
                      np.float64, bf16_round)
    figs = bf16_bwd_figures(a, r)
    print('LSTM-VARIANT %-28s bwd %-11s %s' % (case.name, form, ' '.join('%s %.2e' % kv for kv in sorted(figs.items()))))
    for k, v in figs.items():
        _note(form, 'bwd', k, v)
    assert all(v <= BF16_BOUNDS[k] for k, v in figs.items()), (case.name, form, figs)


_IDS = [c.name for c in ALL_CASES]
_POISON = CASES['cluster'] + CASES['single'] + CASES['mixed'] + [c for c in CASES['edges'] if c.pad]


@pytest.mark.parametrize('case', ALL_CASES, ids=_IDS)
def test_forward_against_fp64(lstm, case):
    dev = lstm.upload(case)
    out, form = lstm.fwd(case, dev)
    assert form == case.ff or _limits()['num_cu'] != 256
    _check_fwd(case, out, form)
    assert _ops().check_async_errors(0) == 0


@pytest.mark.parametrize('case', ALL_CASES, ids=_IDS)
def test_backward_against_fp64(lstm, case):
    """The device backward on what the device forward saved.  The per-tile dpeep partials go to a NaN-filled workspace: the
    empty tile's must come back as zeros.  Without a dpeep request the gate gradients are the same bits."""
    dev = lstm.upload(case)
    saved, _ = lstm.fwd(case, dev)
    ws = torch.full(((case.B // 16) * case.ndir * 7 * case.H,), float('nan'), device=dev['xproj'].device)
    got, form = lstm.bwd(case, dev, saved, ws=ws)
    assert form == case.bf or _limits()['num_cu'] != 256
    _check_bwd(case, got, saved, form)
    if case.B >= 32:
        part = ws.view(case.B // 16, case.ndir, 7, case.H)
        assert float(part[1].abs().max()) == 0.0 and bool(torch.isfinite(part).all()), case.name
    bare, form2 = lstm.bwd(case, dev, saved, want_dpeep=False)
    assert form2 == form and bare['dpeep'] is None and torch.equal(bare['dgates'], got['dgates']), case.name
    assert _ops().check_async_errors(0) == 0


@pytest.mark.parametrize('case', _POISON, ids=[c.name for c in _POISON])
def test_backward_never_reads_saved_activations_of_padded_frames(lstm, case):
    """Saved gates and cs at frames at or past a row's length are unspecified: with NaN there the backward of every form
    gives finite results, bit for bit those of the unpoisoned run."""
    dev = lstm.upload(case)
    saved, _ = lstm.fwd(case, dev)
    clean, form = lstm.bwd(case, dev, saved)
    T, B, ndir, H = case.T, case.B, case.ndir, case.H
    padded = ~torch.tensor(case_data(case.name)['valid'], device=dev['xproj'].device).view(T, B, 1)
    assert bool(padded.any())
    poisoned = dict(saved)
    for k in ('gates', 'cs'):
        poisoned[k] = torch.where(padded, torch.full_like(saved[k], float('nan')), saved[k])
        assert bool(torch.isnan(poisoned[k]).any())
    got, form2 = lstm.bwd(case, dev, poisoned)
    assert form2 == form
    for k in BWD_TENSORS:
        assert bool(torch.isfinite(got[k].float()).all()), (case.name, form, k)
        assert torch.equal(got[k], clean[k]), (case.name, form, k)
    assert _ops().check_async_errors(0) == 0


def test_cluster_launches_back_to_back(lstm, monkeypatch):
    """The cluster cases of all LSTM forms queued with no synchronisation between them, in an order that alternates dtype,
    width, B, T and pass, with GRU cluster launches in between (the two exchange areas alternate between launches, each
    launch zeroes what its predecessor dirtied, and every kernel family has its own bytes per cluster: stale tags of a
    differently shaped predecessor are what could go wrong); results are fetched at the end and meet their bounds."""
    ops = _ops()
    cases = CASES['cluster']
    bf, f3 = [c for c in cases if c.dtype == 'bf16'], [c for c in cases if c.dtype == 'f32']
    order = [c for pair in zip(bf, reversed(f3)) for c in pair] + f3[:len(f3) - len(bf)][::-1]
    assert sorted(c.name for c in order) == sorted(c.name for c in cases)
    assert {f for c in order for f in (c.ff, c.bf)} == set(CLUSTER_FORMS)
    gcases = [G.BY_NAME[n] for n in ('cl128_2x16', 'cl320_1x32', 'cl64_2x48')]
    monkeypatch.delenv('ASR_GRU_CLUSTER', raising=False)
    ops.debug_set_gru_persistent(1)
    devs = {c.name: lstm.upload(c) for c in order}
    gdev = {}
    for g in gcases:
        inp = G.case_data(g.name)['inp']
        gdev[g.name] = {k: torch.tensor(v, device=devs[order[0].name]['xproj'].device) for k, v in inp.items() if v is not None}
        gdev[g.name]['wghT'] = gdev[g.name]['wgh'].transpose(1, 2).contiguous()
        gdev[g.name]['wchT'] = gdev[g.name]['wch'].transpose(1, 2).contiguous()
    torch.cuda.synchronize()
    ops.reset_gru_kernel_counts(0)
    fwd, bwd, gout, prev = {}, {}, {}, None
    for i, c in enumerate(order):                                                # fwd(c), bwd(previous case), GRU, fwd(next) ...
        fwd[c.name], form = lstm.fwd(c, devs[c.name])
        assert form == c.ff or _limits()['num_cu'] != 256
        if prev is not None:
            bwd[prev.name], _ = lstm.bwd(prev, devs[prev.name], fwd[prev.name])
        prev = c
        if i % 6 == 2:
            g = gcases[i // 6]
            d = gdev[g.name]
            saved = ops.gru_fwd(d['xg'], d['xc'], d['wgh'], d['wch'], d['sl'], g.T, g.H, g.ndir)
            dg, dc = ops.gru_bwd(d['dout'], d.get('dhf'), saved, d['wghT'], d['wchT'], d['sl'], g.T, g.H, g.ndir)
            gout[g.name] = dict(saved, dgate=dg, dcand=dc)
    bwd[prev.name], _ = lstm.bwd(prev, devs[prev.name], fwd[prev.name])
    assert len(gout) == 3
    if _limits()['num_cu'] == 256:
        assert ops.gru_kernel_counts(0) == dict(fwd_cluster=3, fwd_persistent=0, fwd_per_step=0, bwd_cluster=3,
                                                bwd_persistent=0, bwd_per_step=0)
    for c in order:
        _check_fwd(c, fwd[c.name], c.ff)
        _check_bwd(c, bwd[c.name], fwd[c.name], c.bf)
    for name, out in gout.items():
        data = G.case_data(name)
        for k in G.FWD_TENSORS + G.BWD_TENSORS:
            a = out[k].cpu().numpy().astype(np.float64)
            if k != 'h_final':
                a = np.where(data['valid'], a, 0.0)
            assert float(np.abs(a - data['ref'][k]).max()) <= G.bound(data, k), (name, k)
    assert ops.check_async_errors(0) == 0


def test_the_case_lists_reach_all_fifteen_forms(cuda):
    """From the rule, with this device's CU count and scratch and a clean environment: every counter of
    ops.lstm_kernel_counts is some case's.  Prints the worst figures per (form, pass) of the tests that ran before."""
    lim = _limits()
    env = {k: v for k, v in os.environ.items() if not k.startswith('ASR_LSTM_')}
    reached = {'%s_%s' % (p, case_form(c, p, env=env, **lim)) for c in ALL_CASES for p in ('fwd', 'bwd')}
    assert reached == set(COUNTER_KEYS) == set(_ops().lstm_kernel_counts(0)), reached
    for (form, pass_), figs in sorted(MEASURED.items()):
        print('LSTM-VARIANT worst: %-11s %s %s' % (form, pass_, ' '.join('%s %.3g' % kv for kv in sorted(figs.items()))))
