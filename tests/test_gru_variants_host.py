"""CPU: the infrastructure of tests/test_gpu_gru_variants.py (tests/_gru_variants.py) held against what the repository
already has -- its float64 reference against oracle/gru.py's dynamic_rnn and against the autograd recurrence of
tests/_cpu_ops.py, the dispatch rule at its documented boundaries, the case lists, and the ceiling on the bounds."""
import numpy as np
import pytest
import torch

import _cpu_ops
from _gru_variants import (ALL_CASES, BWD_TENSORS, CASES, CEILING, CLUSTER_WIDTHS, COUNTER_KEYS, FWD_TENSORS, LDS_LIMIT,
                           MARGIN, ROOM, bound, case_data, case_form, case_lengths, cluster_env_on,
                           cluster_tiles_per_launch, expected_form, gru_reference, persistent_lds)
from oracle import gru as ogru


def _problem(rng, T, B, D, H, ndir):
    """x, full GRUCell parameters per direction, and the hoisted projections the kernels take (float64)."""
    x = rng.randn(T, B, D)
    ps = [dict(wg=rng.randn(D + H, 2 * H) * 0.2, bg=1.0 + rng.randn(2 * H) * 0.1, wc=rng.randn(D + H, H) * 0.2,
               bc=rng.randn(H) * 0.1) for _ in range(ndir)]
    xg = np.concatenate([x @ p['wg'][:D] + p['bg'] for p in ps], 2)
    xc = np.concatenate([x @ p['wc'][:D] + p['bc'] for p in ps], 2)
    wgh, wch = np.stack([p['wg'][D:] for p in ps]), np.stack([p['wc'][D:] for p in ps])
    return x, ps, xg, xc, wgh, wch


@pytest.mark.parametrize('T,B,D,H,ndir', [(9, 6, 5, 16, 2), (1, 4, 3, 16, 1), (14, 5, 7, 32, 2)])
def test_reference_forward_matches_the_oracle(T, B, D, H, ndir):
    """gru_reference against oracle.gru.dynamic_rnn (GRUCell pinned to TensorFlow's known answers): both directions,
    ragged rows, a row of length 1 and an empty one; output zero past the length, state carried.  1e-12."""
    rng = np.random.RandomState(T + B)
    x, ps, xg, xc, wgh, wch = _problem(rng, T, B, D, H, ndir)
    sl = rng.randint(1, T + 1, size=B)
    sl[0], sl[1], sl[2] = T, 1, 0
    ref = gru_reference(xg, xc, wgh, wch, sl, H, ndir)
    for d in range(ndir):
        p = {k: torch.tensor(v) for k, v in ps[d].items()}
        out, hf = ogru.dynamic_rnn(torch.tensor(x), torch.tensor(sl), p, reverse=d == 1)
        assert np.abs(ref['hout'][:, :, d * H:(d + 1) * H] - out.numpy()).max() < 1e-12
        assert np.abs(ref['h_final'][d] - hf.numpy()).max() < 1e-12
    valid = (np.arange(T)[:, None] < sl[None, :])[:, :, None]
    for k in ('r', 'u', 'c', 'rh', 'hout'):
        assert np.abs(np.where(valid, 0.0, ref[k])).max() == 0.0
    assert np.abs(ref['h_final'][:, 2]).max() == 0.0 and np.abs(ref['hout']).max() > 0.01


@pytest.mark.parametrize('T,B,H,ndir,dhf', [(9, 6, 16, 2, True), (1, 4, 16, 1, True), (13, 5, 32, 2, False)])
def test_reference_gradients_match_the_autograd_recurrence(T, B, H, ndir, dhf):
    """The hand-written backward against autograd through tests/_cpu_ops.py::_gru_fwd (the float64 graph it keeps, which
    _gru_bwd differentiates before it rounds to float32): dgate, dcand, and the forward tensors both hold.  1e-12."""
    rng = np.random.RandomState(3 * T + B)
    f = lambda *s: torch.tensor(rng.randn(*s), dtype=torch.float32)              # noqa: E731
    xg, xc, wgh, wch = f(T, B, ndir * 2 * H) * 0.5, f(T, B, ndir * H) * 0.5, f(ndir, H, 2 * H) * 0.2, f(ndir, H, H) * 0.2
    dout, d_h = f(T, B, ndir * H) * 0.3, (f(ndir, B, H) * 0.3 if dhf else None)
    sl = rng.randint(1, T + 1, size=B).astype(np.int32)
    sl[0], sl[1], sl[2] = T, 1, 0
    saved = _cpu_ops._gru_fwd(xg, xc, wgh, wch, torch.tensor(sl), T, H, ndir)
    ref = gru_reference(xg.numpy(), xc.numpy(), wgh.numpy(), wch.numpy(), sl, H, ndir, dout.numpy(),
                        None if d_h is None else d_h.numpy())
    for d, run in enumerate(saved['_runs']):
        gos = [dout[:, :, d * H:(d + 1) * H].double(), d_h[d].double() if dhf else torch.zeros_like(run['hf'])]
        ga, gb = torch.autograd.grad([run['out'], run['hf']], [run['xg'], run['xc']], grad_outputs=gos, retain_graph=True)
        assert np.abs(ref['dgate'][:, :, d * 2 * H:(d + 1) * 2 * H] - ga.numpy()).max() < 1e-12
        assert np.abs(ref['dcand'][:, :, d * H:(d + 1) * H] - gb.numpy()).max() < 1e-12
        assert np.abs(ref['hout'][:, :, d * H:(d + 1) * H] - run['out'].detach().numpy()).max() < 1e-12
        assert np.abs(ref['h_final'][d] - run['hf'].detach().numpy()).max() < 1e-12
    dg, dc = _cpu_ops._gru_bwd(dout, d_h, saved, None, None, torch.tensor(sl), T, H, ndir)   # its float32 results
    assert np.abs(ref['dgate'] - dg.numpy()).max() < 1e-7 and np.abs(ref['dcand'] - dc.numpy()).max() < 1e-7
    assert np.abs(ref['rh'] - saved['rh'].numpy()).max() < 1e-7
    valid = (np.arange(T)[:, None] < sl[None, :])[:, :, None]
    assert np.abs(np.where(valid, 0.0, ref['dgate'])).max() == 0.0 and np.abs(np.where(valid, 0.0, ref['dcand'])).max() == 0.0
    assert np.abs(ref['dgate']).max() > 0.01


def test_case_lists_are_well_formed():
    names = [c.name for c in ALL_CASES]
    assert len(set(names)) == len(names)
    for c in ALL_CASES:
        assert c.B % 16 == 0 and c.H % 16 == 0 and c.ndir in (1, 2) and 1 <= c.T <= 40 and 0 <= c.pad < c.T
        sl = case_lengths(c)
        assert sl.shape == (c.B,) and sl.min() >= 0 and sl.max() == sl[0] == c.T - c.pad and sl[1] == 1 and sl[2] == 0
        if c.B >= 32:
            assert (sl[16:32] == 0).all()
        if c.T - c.pad > 2:
            assert len(set(sl[3:16].tolist())) > 2                               # ragged
    # what the issue lists: every cluster width x (ndir, B); the widths of the persistent and per-step lists
    assert sorted((c.H, c.ndir, c.B) for c in CASES['cluster']) == sorted(
        (H, nd, B) for H in CLUSTER_WIDTHS for nd, B in ((2, 16), (1, 32), (2, 48)))
    assert [c.H for c in CASES['persistent']] == [16, 48, 144, 496, 512]
    assert [c.H for c in CASES['persistent_cluster_off']] == [64, 128, 320]
    assert [c.H for c in CASES['per_step']] == [16, 48, 128, 320, 528]
    assert {c.ndir for c in ALL_CASES} == {1, 2} and any(c.T == 1 for c in ALL_CASES)
    assert any(c.pad for c in ALL_CASES) and any(not c.dhf for c in ALL_CASES)
    # the forms the lists mean to reach (on 256 CUs with the default arena)
    f = lambda c: (case_form(c, 'fwd'), case_form(c, 'bwd'))                      # noqa: E731
    assert all(f(c) == ('cluster', 'cluster') for c in CASES['cluster'])
    assert [f(c) for c in CASES['persistent']] == [('persistent', 'persistent')] * 4 + [('persistent', 'per_step')]
    assert all(f(c) == ('persistent', 'persistent') for c in CASES['persistent_cluster_off'])
    assert all(f(c) == ('per_step', 'per_step') for c in CASES['per_step'])
    assert [f(c) for c in CASES['mixed']] == [('per_step', 'persistent'), ('per_step', 'cluster'), ('persistent', 'per_step')]
    reached = {'%s_%s' % (p, case_form(c, p)) for c in ALL_CASES for p in ('fwd', 'bwd')}
    assert reached == set(COUNTER_KEYS)


def test_expected_form_at_the_boundaries():
    e = expected_form
    # the two LDS formulas: forward 192 (H + 4) fits up to 512; backward 64 (5 H + 16) = 159 744 at 496, 164 864 at 512
    assert persistent_lds('fwd', 512) == 99072 and persistent_lds('bwd', 496) == 159744 <= LDS_LIMIT < persistent_lds('bwd', 512)
    want = {480: ('persistent', 'persistent'), 496: ('persistent', 'persistent'), 512: ('persistent', 'per_step'),
            528: ('per_step', 'per_step')}
    for H, forms in want.items():
        assert (e('fwd', H, 16, 2, 3), e('bwd', H, 16, 2, 3)) == forms, H
    # a cluster width: the switch off takes the clusters with it; the environment keeps the persistent kernel
    for H in CLUSTER_WIDTHS:
        for p in ('fwd', 'bwd'):
            assert e(p, H, 16, 2, 10) == 'cluster'
            assert e(p, H, 16, 2, 10, persistent_switch=False) == 'per_step'
            assert e(p, H, 16, 2, 10, cluster_env=False) == 'persistent'
    assert e('fwd', 96, 16, 2, 10) == 'persistent' and e('fwd', 16, 16, 1, 10, persistent_switch=False) == 'per_step'
    # 1 <= T < 65536 on the clusters
    assert e('fwd', 128, 16, 1, 0) == 'persistent' and e('fwd', 128, 16, 1, 65535) == 'cluster'
    assert e('bwd', 128, 16, 1, 65536) == 'persistent'
    # the tile plan: a budget too small for one tile of both directions (H = 256: 8 CUs per cluster, rounds of 8 clusters)
    assert cluster_tiles_per_launch('fwd', 256, 48, 2, 63, 256) == 0 and e('fwd', 256, 48, 2, 10, cu_budget=63) == 'persistent'
    assert cluster_tiles_per_launch('fwd', 256, 48, 2, 64, 256) == 3 and e('fwd', 256, 48, 2, 10, cu_budget=64) == 'cluster'
    assert cluster_tiles_per_launch('bwd', 256, 48, 2, 128, 256) == 3
    assert e('bwd', 320, 16, 2, 10, num_cu=79) == 'persistent' and e('bwd', 320, 16, 2, 10, num_cu=80) == 'cluster'
    assert e('fwd', 64, 16, 1, 10, cu_budget=1000, num_cu=8) == 'persistent'   # a budget above the chip: the chip
    # more tiles than one launch holds run as tile groups: still the clusters
    assert cluster_tiles_per_launch('fwd', 256, 512, 2, 0, 256) == 16 and e('fwd', 256, 512, 2, 10) == 'cluster'
    # packed weights ndir * 3 * H * H * 4 below the exchange area
    pk = 2 * 3 * 512 * 512 * 4
    assert e('fwd', 512, 16, 2, 3, scratch_room=pk) == 'persistent' and e('fwd', 512, 16, 2, 3, scratch_room=pk - 1) == 'per_step'
    assert e('fwd', 512, 16, 1, 3, scratch_room=pk // 2) == 'persistent'
    assert pk <= ROOM
    # the environment as the launchers read it
    assert cluster_env_on({}) and cluster_env_on({'ASR_GRU_CLUSTER': '1'}) and not cluster_env_on({'ASR_GRU_CLUSTER': '0'})
    assert not cluster_env_on({'ASR_LSTM_CLUSTER_F32': '0'}) and not cluster_env_on({'ASR_LSTM_CLUSTER': '0x'})


@pytest.mark.parametrize('group', list(CASES))
def test_bounds_stay_under_the_ceiling(group):
    """8 E32 -- the float32 evaluation of the same recurrence against the float64 one -- is under 1e-5 for every forward
    tensor and 2e-5 for every gradient of every listed case, and nonzero; the gradients are large enough that zeros
    cannot pass."""
    for c in CASES[group]:
        data = case_data(c.name)
        for k in FWD_TENSORS:
            assert bound(data, k) == MARGIN * data['e32'][k] < CEILING['fwd'], (c.name, k, data['e32'][k])
            # (zero only where the tensor is: r * h at T = 1, where h = 0 -- the device must give exact zeros too)
            assert bound(data, k) > 0.0 or np.abs(data['ref'][k]).max() == 0.0, (c.name, k)
        for k in BWD_TENSORS:
            assert 0.0 < bound(data, k) < CEILING['bwd'], (c.name, k, data['e32'][k])
            assert np.abs(data['ref'][k]).max() > 0.1, (c.name, k)
        assert np.abs(data['ref']['h_final'][:, 2]).max() == 0.0                 # the empty row
        if c.B >= 32:
            assert np.abs(data['ref']['h_final'][:, 16:32]).max() == 0.0 and np.abs(data['ref']['hout'][:, 16:32]).max() == 0.0
