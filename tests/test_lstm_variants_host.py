"""CPU: the infrastructure of tests/test_gpu_lstm_variants.py (tests/_lstm_variants.py) held against what the repository
already has -- its reference against oracle/lstm.py's explicit numpy layer (with and without the bf16 rounding points) and
against autograd through oracle.lstm.dynamic_rnn (both clip conventions), the dispatch rule at its boundaries, the case
lists, and the ceiling on the bounds."""
import numpy as np
import pytest
import torch

from _lstm_variants import (ALL_CASES, BF16_BOUNDS, BWD_TENSORS, CASES, CEILING_REL, CLIP_GAP, COUNTER_KEYS, EDGE_FORMS,
                            EDGE_KINDS, FORMS, FWD_TENSORS, F_CU16, F_EARLY, F_EXACT, F_HS64, F_WT, F_XP, F_XW8, MARGIN, NDB,
                            SCRATCH, XCH_BYTES, XCH_HALF, bf16_own_figures, bf16_round, bound, case_data, case_form,
                            case_lengths, cl_bytes, clip_gap, cluster_launch_plan, cluster_tile_plan, env_flags, expected_form, lstm_backward,
                            lstm_forward, units_per_cu)
from oracle import lstm as olstm


def _il(a, H):
    """[..., 4H] in column blocks i | g | f | o -> [..., H, 4]."""
    return np.ascontiguousarray(np.swapaxes(a.reshape(a.shape[:-1] + (4, H)), -1, -2))


def _lens(rng, T, B):
    sl = rng.randint(1, T + 1, size=B)
    sl[0], sl[1], sl[2] = T, 1, 0
    return sl


def test_bf16_round_is_round_to_nearest_even():
    rng = np.random.RandomState(0)
    a = np.concatenate([rng.randn(4096) * 3, [1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 0.0, 2.0 ** -130, 0.5]])
    assert np.array_equal(bf16_round(a).astype(np.float64), olstm.bf16_round(a))
    assert bf16_round(np.float32(1.0 + 2.0 ** -8)) == 1.0 and bf16_round(np.float32(1.0 + 3 * 2.0 ** -8)) == 1.0 + 2.0 ** -6


@pytest.mark.parametrize('rounded', [False, True])
@pytest.mark.parametrize('T,B,D,H,peep,clip', [(9, 6, 5, 16, True, 0.0), (1, 4, 3, 16, True, 0.0), (12, 5, 7, 32, False, 0.0),
                                               (10, 6, 5, 16, True, 0.4)])
def test_reference_matches_the_oracle_layer(T, B, D, H, peep, clip, rounded):
    """lstm_forward / lstm_backward against oracle.lstm.layer_forward_np / layer_backward_np on the x-projections the
    oracle forms: both directions, ragged rows, a row of length 1 and an empty one, with and without peepholes, an active
    straight-through clip, with and without the bf16 rounding points.  1e-11 (a rounding flip would show as 2^-9)."""
    rng = np.random.RandomState(T * 7 + B + H)
    sl = _lens(rng, T, B)
    scale = 3.0 if clip else 1.0
    x = rng.randn(T, B, D) * scale
    ps = [dict(w=rng.uniform(-0.3, 0.3, (D + H, 4 * H)), b=rng.uniform(-0.1, 0.1, 4 * H), wci=rng.uniform(-0.3, 0.3, H),
               wcf=rng.uniform(-0.3, 0.3, H), wco=rng.uniform(-0.3, 0.3, H)) for _ in range(2)]
    fn_o, fn = (olstm.bf16_round, bf16_round) if rounded else (None, None)
    dout, dcf, dhf = rng.randn(T, B, 2, H), rng.randn(2, B, H), rng.randn(2, B, H)
    fo = [olstm.layer_forward_np(x, sl, p, d == 1, 1.0, clip, peep, round_fn=fn_o) for d, p in enumerate(ps)]
    xproj = np.stack([_il(f['xproj'], H) for f in fo], 2)                         # [T,B,2,H,4]
    wh = np.stack([p['w'][D:] for p in ps])
    pp = np.stack([np.stack([p['wci'], p['wcf'], p['wco']]) for p in ps]) if peep else None
    ref = lstm_forward(xproj, wh, pp, sl, H, 2, 1.0, clip, np.float64, fn)
    ref.update(lstm_backward(dout, ref['gates'], ref['cs'], wh, pp, sl, H, 2, dcf, dhf, 0.0, np.float64, fn))
    valid = (np.arange(T)[:, None] < sl[None, :])[:, :, None]
    for d, f in enumerate(fo):
        assert np.abs(ref['gates'][:, :, d] - np.swapaxes(f['gates'], -1, -2)).max() < 1e-11
        for k in ('cs', 'hout'):
            assert np.abs(ref[k][:, :, d] - f[k]).max() < 1e-11, k
            assert np.abs(np.where(valid, 0.0, ref[k][:, :, d])).max() == 0.0
        assert np.abs(ref['c_final'][d] - f['c_final']).max() < 1e-11 and np.abs(ref['h_final'][d] - f['h_final']).max() < 1e-11
        bo = olstm.layer_backward_np(dout[:, :, d], f['gates'], f['cs'], sl, ps[d], d == 1, peep, dcf[d], dhf[d], round_fn=fn_o)
        assert np.abs(ref['dgates'][:, :, d] - np.swapaxes(bo['dgates'], -1, -2)).max() < 1e-11
        assert np.abs(np.where(valid[..., None], 0.0, ref['dgates'][:, :, d])).max() == 0.0
        assert np.abs(ref['dpeep'][d, :3] - bo['dpeep']).max() < 1e-10
        # (the oracle sums the rounded gate gradients into db, the kernels and this reference the unrounded ones)
        assert np.abs(ref['dpeep'][d, 3:].reshape(-1) - bo['db']).max() < (2e-2 * np.abs(bo['db']).max() if rounded else 1e-10)
    if clip:
        assert np.abs(ref['cs']).max() == clip and clip_gap(ref['cs_raw'], clip) > 0
    assert np.abs(ref['h_final'][:, 2]).max() == 0.0 and np.abs(ref['dgates']).max() > 0.01
    if not peep:
        assert np.abs(ref['dpeep'][:, :2]).max() > 0.01       # (the sums are formed all the same, as on the device)


@pytest.mark.parametrize('T,B,H,peep,clip,block,dfin', [(9, 6, 8, True, 0.0, False, True), (1, 4, 8, True, 0.0, False, True),
                                                        (11, 5, 8, False, 0.0, False, False), (10, 6, 8, True, 0.5, False, True),
                                                        (10, 6, 8, True, 0.5, True, True)])
def test_reference_gradients_match_autograd(T, B, H, peep, clip, block, dfin):
    """The hand-written BPTT against autograd through oracle.lstm.dynamic_rnn, where W_x is the identity so that x IS the
    x-projection and dL/dx the gate gradient: dgates, the three peephole gradients and the bias gradient, with gradients
    entering through the outputs, the final states or (dfin False) the outputs only; straight-through and
    gradient-blocking clip (clip_blocks_gradient), the clip active.  1e-11."""
    rng = np.random.RandomState(5 * T + B)
    sl = _lens(rng, T, B)
    x = rng.randn(T, B, 2, 4 * H) * (2.0 if clip else 1.0)
    wh = rng.uniform(-0.3, 0.3, (2, H, 4 * H))
    pp = rng.uniform(-0.3, 0.3, (2, 3, H))
    dout = rng.randn(T, B, 2, H)
    dcf, dhf = (rng.randn(2, B, H), rng.randn(2, B, H)) if dfin else (None, None)
    ref = lstm_forward(_il(x, H), wh, pp if peep else None, sl, H, 2, 1.0, clip)
    ref.update(lstm_backward(dout, ref['gates'], ref['cs'], wh, pp if peep else None, sl, H, 2, dcf, dhf, clip if block else 0.0))
    for d in range(2):
        xt = torch.tensor(x[:, :, d], requires_grad=True)
        p = dict(w=torch.tensor(np.concatenate([np.eye(4 * H), wh[d]])), b=torch.zeros(4 * H, dtype=torch.float64, requires_grad=True),
                 wci=torch.tensor(pp[d, 0], requires_grad=True), wcf=torch.tensor(pp[d, 1], requires_grad=True),
                 wco=torch.tensor(pp[d, 2], requires_grad=True))
        out, (cf, hf) = olstm.dynamic_rnn(xt, torch.tensor(sl), p, reverse=d == 1, cell_clip=clip, use_peephole=peep,
                                          clip_blocks_gradient=block)
        loss = (out * torch.tensor(dout[:, :, d])).sum()
        if dfin:
            loss = loss + (cf * torch.tensor(dcf[d])).sum() + (hf * torch.tensor(dhf[d])).sum()
        loss.backward()
        assert np.abs(ref['hout'][:, :, d] - out.detach().numpy()).max() < 1e-12
        assert np.abs(ref['c_final'][d] - cf.detach().numpy()).max() < 1e-12
        assert np.abs(ref['dgates'][:, :, d] - _il(xt.grad.numpy(), H)).max() < 1e-11
        assert np.abs(ref['dpeep'][d, 3:].reshape(-1) - p['b'].grad.numpy()).max() < 1e-11
        if peep:
            got = np.stack([p[k].grad.numpy() for k in ('wci', 'wcf', 'wco')])
            assert np.abs(ref['dpeep'][d, :3] - got).max() < 1e-11
    if clip:
        valid = np.broadcast_to((np.arange(T)[:, None] < sl[None, :])[:, :, None, None], ref['cs'].shape)
        frac = np.mean(np.abs(ref['cs'][valid]) >= clip)
        assert 0.02 < frac < 0.9 and clip_gap(ref['cs_raw'], clip) > 1e-9, frac
    assert np.abs(ref['dgates']).max() > 0.01


def test_float32_evaluation_stays_float32():
    c = CASES['edges'][5]
    d = case_data(c.name)
    r = lstm_forward(d['inp']['xproj'], d['inp']['wh'], d['inp']['peep'], d['inp']['sl'], c.H, c.ndir, dtype=np.float32)
    assert all(v.dtype == np.float32 for v in r.values())
    assert 0 < np.abs(r['hout'] - d['ref']['hout']).max() == d['e32']['hout'] < 1e-6


def test_case_lists_are_well_formed():
    names = [c.name for c in ALL_CASES]
    assert len(set(names)) == len(names)
    for c in ALL_CASES:
        assert c.B in (16, 32, 48) and c.ndir in (1, 2) and 1 <= c.T <= 40 and 0 <= c.pad < c.T and c.H in (64, 128, 192, 256, 320, 512)
        sl = case_lengths(c)
        assert sl.shape == (c.B,) and sl.min() >= 0 and sl.max() == sl[0] == c.T - c.pad and sl[1] == 1 and sl[2] == 0
        if c.B >= 32:
            assert (sl[16:32] == 0).all()
        if c.T - c.pad > 3:
            assert len(set(sl[3:16].tolist())) > 2                               # ragged
        # the forms the lists mean to reach (on 256 CUs with the default arena, a clean environment)
        assert (case_form(c, 'fwd'), case_form(c, 'bwd')) == (c.ff, c.bf), c.name
    reached = {'fwd_' + c.ff for c in ALL_CASES} | {'bwd_' + c.bf for c in ALL_CASES}
    assert reached == set(COUNTER_KEYS) and len(COUNTER_KEYS) == 15
    # every form at every width it serves; the cluster forms at the three (ndir, B); single-CU at two of them
    widths = {'bf16_cu16': {256}, 'bf16_hs32': {256, 512}, 'bf16_hs64': {256, 320, 512}, 'f32_split': {128, 256},
              'f32_hs32': {128, 256, 320, 512}, 'f32_hs64': {128}, 'single_bf16': {64, 128, 192, 256, 320, 512},
              'single_f32': {64, 128, 192, 256, 320, 512}}
    base = CASES['cluster'] + CASES['single']
    for form in FORMS:
        for attr in ('ff', 'bf')[:1 if form == 'bf16_cu16' else 2]:
            mine = [c for c in base if getattr(c, attr) == form]
            assert {c.H for c in mine} == widths[form], (form, attr)
            assert {(c.ndir, c.B) for c in mine} == set(NDB if not form.startswith('single') else NDB[:2]), (form, attr)
    # the ladder, the mixed pairings, the variants, the blocking clip and the edges the suite promises
    assert [(c.fb, c.ff, c.bf) for c in CASES['ladder']] == [
        (128, 'bf16_cu16', 'bf16_hs32'), (127, 'bf16_hs32', 'bf16_hs32'), (64, 'bf16_hs32', 'bf16_hs32'),
        (63, 'bf16_hs64', 'bf16_hs64'), (32, 'bf16_hs64', 'bf16_hs64'), (31, 'single_bf16', 'single_bf16'),
        (64, 'f32_split', 'f32_split'), (63, 'single_f32', 'single_f32')]
    assert all(c.fb == c.bb and (c.ndir, c.B) == (2, 16) for c in CASES['ladder'])
    assert {(c.ff, c.bf) for c in CASES['mixed']} == {
        ('bf16_cu16', 'bf16_hs64'), ('single_bf16', 'bf16_hs32'), ('bf16_cu16', 'single_bf16'), ('single_f32', 'f32_split'),
        ('f32_split', 'single_f32'), ('f32_split', 'f32_hs32'), ('f32_hs32', 'f32_split')}
    assert any((c.ff, c.bf) == ('bf16_cu16', 'bf16_hs32') for c in CASES['cluster'])
    v = CASES['variants']
    assert {c.ff for c in v if c.fwd & F_EARLY} == {'bf16_hs32', 'bf16_hs64', 'f32_split', 'f32_hs32', 'f32_hs64'}
    assert {c.ff for c in v if c.fwd & F_XW8} == {'bf16_hs32', 'bf16_hs64'}
    assert {c.bf for c in v if c.bwd & F_XP} == {'bf16_hs32', 'bf16_hs64'}
    assert {c.ff for c in v if c.fwd & F_WT} == set(FORMS[:6]) and {c.bf for c in v if c.bwd & F_WT} == set(FORMS[1:6])
    assert {c.bf for c in CASES['clip_block']} == set(FORMS[1:]) and all(c.block and c.clip for c in CASES['clip_block'])
    assert len(CASES['edges']) == len(EDGE_FORMS) * len(EDGE_KINDS)
    assert {c.ff for c in CASES['edges']} == set(FORMS) and {c.bf for c in CASES['edges']} == set(FORMS[1:])
    for i in range(len(EDGE_FORMS)):
        e = CASES['edges'][i * len(EDGE_KINDS):(i + 1) * len(EDGE_KINDS)]
        assert [c.T for c in e[:3]] == [1, 2, 3] and len({(c.ff, c.bf) for c in e}) == 1
        tm = sorted(c.T - c.pad for c in e[3:5])
        assert 33 <= tm[0] < tm[1] <= 40 and tm[0] % 2 != tm[1] % 2
        assert e[5].pad == 3 and not e[6].peep and e[7].clip and not e[7].block and not e[8].dfin
        assert all(c.peep and c.dfin for c in e[:6])


def test_expected_form_at_the_boundaries():
    e = expected_form
    # the budget thresholds per G at one tile of both directions: a round of 8 clusters of G CUs each
    for n, want in ((256, 'bf16_cu16'), (128, 'bf16_cu16'), (127, 'bf16_hs32'), (64, 'bf16_hs32'), (63, 'bf16_hs64'),
                    (32, 'bf16_hs64'), (31, 'single_bf16'), (1, 'single_bf16')):
        assert e('fwd', 'bf16', 256, 16, 2, 10, cu_budget=n) == want, n
    for n, want in ((64, 'bf16_hs32'), (63, 'bf16_hs64'), (32, 'bf16_hs64'), (31, 'single_bf16')):
        assert e('bwd', 'bf16', 256, 16, 2, 10, cu_budget=n) == want, n
    for n, want in ((128, 'bf16_hs32'), (127, 'bf16_hs64'), (64, 'bf16_hs64'), (63, 'single_bf16')):       # H = 512: G = 16 / 8
        assert e('fwd', 'bf16', 512, 16, 2, 10, cu_budget=n) == want and e('bwd', 'bf16', 512, 16, 2, 10, cu_budget=n) == want
    assert e('fwd', 'bf16', 320, 16, 2, 10, cu_budget=40) == 'bf16_hs64' and e('fwd', 'bf16', 320, 16, 2, 10, cu_budget=39) == 'single_bf16'
    for p in ('fwd', 'bwd'):
        assert e(p, 'f32', 128, 16, 2, 10, cu_budget=32) == 'f32_split' and e(p, 'f32', 128, 16, 2, 10, cu_budget=31) == 'single_f32'
        assert e(p, 'f32', 128, 16, 2, 10, F_HS64, 16) == 'f32_hs64' and e(p, 'f32', 128, 16, 2, 10, F_HS64, 15) == 'single_f32'
        assert e(p, 'f32', 512, 16, 2, 10, cu_budget=128) == 'f32_hs32' and e(p, 'f32', 512, 16, 2, 10, cu_budget=127) == 'single_f32'
        assert e(p, 'f32', 320, 16, 1, 10, cu_budget=80) == 'f32_hs32' and e(p, 'f32', 320, 16, 1, 10, cu_budget=79) == 'single_f32'
    # one direction needs half the round's tiles only once: per = 8 tiles per round
    assert cluster_tile_plan(8, 1, 2, 64) == (2, 1) and cluster_tile_plan(8, 2, 3, 64) == (3, 1) and cluster_tile_plan(8, 2, 5, 64) == (4, 2)
    assert cluster_tile_plan(16, 2, 1, 127) == (0, 0)
    # a budget above the chip is the chip; a small chip
    assert e('fwd', 'bf16', 256, 16, 2, 10, cu_budget=1000, num_cu=64) == 'bf16_hs32'
    assert e('fwd', 'bf16', 256, 16, 2, 10, num_cu=31) == 'single_bf16'
    # more tiles than one launch holds: the 16-CU form only as ONE launch (B = 128, two directions: 16 clusters of 16 CUs),
    # beyond it the 32-unit form as one launch up to B = 256, the 64-unit form as one launch up to B = 512 (every form as
    # ONE launch comes before any form in tile groups), and past that tile groups of the 32-unit form
    assert e('fwd', 'bf16', 256, 128, 2, 10) == 'bf16_cu16' and e('fwd', 'bf16', 256, 144, 2, 10) == 'bf16_hs32'
    assert e('fwd', 'bf16', 256, 256, 2, 10) == 'bf16_hs32' and e('fwd', 'bf16', 256, 272, 2, 10) == 'bf16_hs64'
    assert e('fwd', 'bf16', 256, 512, 2, 10) == 'bf16_hs64' and e('fwd', 'bf16', 256, 528, 2, 10) == 'bf16_hs32'
    assert e('bwd', 'bf16', 512, 512, 2, 10) == 'bf16_hs32' and e('fwd', 'f32', 256, 512, 2, 10) == 'f32_split'
    # the exchange-area cap: tiles whose clusters one area has slots for.  The largest user is the BPTT at H = 512 on 16 CUs
    # (1 MiB per cluster): one launch still holds 8 tiles of both directions, so the cap binds only on a smaller area
    assert cl_bytes('bwd', 'bf16', 512, 32) == cl_bytes('bwd', 'f32', 512, 32) == (16 + 2 * 16 * 16 * 2 * 128) * 8
    assert cl_bytes('fwd', 'bf16', 256, 16) == (16 + 2 * 16 * 16 * 8) * 8 and cl_bytes('fwd', 'f32', 128, 32) == (16 + 2 * 4 * 16 * 32) * 8
    assert cl_bytes('fwd', 'bf16', 320, 64) == (16 + 2 * 5 * 16 * 32) * 8 and cl_bytes('bwd', 'f32', 128, 64) == (16 + 2 * 2 * 2 * 4 * 128) * 8
    big = cl_bytes('bwd', 'bf16', 512, 32)
    assert XCH_HALF // (2 * big) == 15 and cluster_launch_plan(16, 2, 128, big, False, 0, 256) == 1
    assert cluster_launch_plan(16, 2, 256, big, False, 0, 512) == 0 and cluster_launch_plan(16, 2, 256, big, True, 0, 512) == 2
    assert cluster_launch_plan(16, 2, 256, big // 2, False, 0, 512) == 1
    assert e('bwd', 'bf16', 512, 256, 2, 4, num_cu=512) == 'bf16_hs64'        # (one launch of the 64-unit form is preferred to groups)
    # no exchange area at all
    assert e('fwd', 'bf16', 256, 16, 2, 10, scratch_bytes=XCH_BYTES) == 'bf16_cu16'
    assert e('fwd', 'bf16', 256, 16, 2, 10, scratch_bytes=XCH_BYTES - 1) == 'single_bf16'
    assert e('bwd', 'f32', 128, 16, 2, 10, scratch_bytes=0) == 'single_f32' and SCRATCH >= XCH_BYTES
    # the forward split's 16-bit step tags; the BPTT split has none
    assert e('fwd', 'f32', 128, 16, 1, 65535) == 'f32_split' and e('fwd', 'f32', 128, 16, 1, 65536) == 'f32_hs32'
    assert e('bwd', 'f32', 128, 16, 1, 65536) == 'f32_split' and e('fwd', 'f32', 320, 16, 1, 65536) == 'f32_hs32'
    # the 2^31 element limit of the clusters' 32-bit offsets (the single-CU kernels go on to 2^32)
    assert e('fwd', 'bf16', 256, 16, 2, 262143) == 'bf16_cu16' and e('fwd', 'bf16', 256, 16, 2, 262144) == 'single_bf16'
    assert e('bwd', 'f32', 512, 16, 2, 131071) == 'f32_hs32' and e('bwd', 'f32', 512, 16, 2, 131072) == 'single_f32'
    assert e('fwd', 'f32', 128, 16, 2, 0) is None
    # each flag
    f = lambda fl, p='fwd', dt='bf16', H=256: e(p, dt, H, 16, 2, 10, fl)          # noqa: E731
    assert f(0) == 'bf16_cu16' and f(F_CU16) == 'bf16_hs32' and f(F_HS64) == 'bf16_hs64' and f(F_HS64 | F_CU16) == 'bf16_hs64'
    assert f(F_XW8) == 'bf16_hs32' and f(F_XW8 | F_CU16) == 'bf16_hs32' and f(F_EARLY) == f(F_WT) == f(F_XP) == f(F_EXACT) == 'bf16_cu16'
    assert f(F_CU16, 'bwd') == f(F_XW8, 'bwd') == 'bf16_hs32' and f(F_HS64, 'bwd') == 'bf16_hs64'
    assert f(F_CU16, H=512) == 'bf16_hs32' and f(F_HS64, H=512) == 'bf16_hs64' and f(F_HS64, H=320) == f(0, H=320) == 'bf16_hs64'
    for p in ('fwd', 'bwd'):
        assert f(0, p, 'f32') == 'f32_split' and f(F_EXACT, p, 'f32') == 'f32_hs32' and f(F_HS64, p, 'f32') == 'single_f32'
        assert f(F_HS64, p, 'f32', 128) == f(F_HS64 | F_EXACT, p, 'f32', 128) == 'f32_hs64' and f(0, p, 'f32', 320) == 'f32_hs32'
        assert f(F_CU16 | F_XW8 | F_XP | F_EARLY | F_WT, p, 'f32') == 'f32_split'
        for H in (64, 192):
            assert f(0, p, 'f32', H) == 'single_f32' and f(0, p, 'bf16', H) == 'single_bf16'
        assert f(0, p, 'bf16', 128) == 'single_bf16'
    # each environment switch
    g = lambda env, p='fwd', dt='bf16', H=256, fl=0: e(p, dt, H, 16, 2, 10, fl, env=env)   # noqa: E731
    assert g({'ASR_LSTM_CLUSTER': '0'}) == 'single_bf16' and g({'ASR_LSTM_CLUSTER': '0'}, dt='f32') == 'single_f32'
    assert g({'ASR_LSTM_CLUSTER': '1'}) == 'bf16_cu16' and g({'ASR_LSTM_CLUSTER_F32': '0'}) == 'bf16_cu16'
    assert g({'ASR_LSTM_CLUSTER_F32': '0'}, dt='f32') == 'single_f32'
    assert g({'ASR_LSTM_CLUSTER_320': '0'}, H=320) == 'single_bf16' and g({'ASR_LSTM_CLUSTER_320': '0'}, dt='f32', H=320) == 'f32_hs32'
    assert g({'ASR_LSTM_CLUSTER_F32_WIDE': '0'}, dt='f32') == 'single_f32' and g({'ASR_LSTM_CLUSTER_F32_WIDE': '0'}, dt='f32', H=128) == 'f32_split'
    assert g({'ASR_LSTM_F32_SPLIT': '0'}, dt='f32') == g({'ASR_LSTM_F32_SPLIT': '0'}, 'bwd', 'f32') == 'f32_hs32'
    assert g({'ASR_LSTM_XW': '0'}) == 'bf16_hs32' and g({'ASR_LSTM_DBG': '1'}) == 'bf16_hs32' and g({'ASR_LSTM_DBG': '0'}) == 'bf16_cu16'
    assert g({'ASR_LSTM_HS': '64'}) == g({'ASR_LSTM_FWD_HS': '64'}) == 'bf16_hs64' and g({'ASR_LSTM_BWD_HS': '64'}) == 'bf16_cu16'
    assert g({'ASR_LSTM_BWD_HS': '64'}, 'bwd') == g({'ASR_LSTM_HS': '64'}, 'bwd') == 'bf16_hs64' and g({'ASR_LSTM_FWD_HS': '64'}, 'bwd') == 'bf16_hs32'
    assert g({'ASR_LSTM_FWD_HS': '32'}) == 'bf16_hs32' and g({'ASR_LSTM_FWD_HS': '32'}, fl=F_CU16) == 'bf16_cu16'
    assert g({'ASR_LSTM_FWD_HS': '16'}) == 'bf16_cu16' and g({'ASR_LSTM_HS': '64', 'ASR_LSTM_FWD_HS': '32'}) == 'bf16_hs32'
    assert g({'ASR_LSTM_HS': '64'}, dt='f32', H=128) == 'f32_hs64' and g({'ASR_LSTM_HS': '64'}, dt='f32') == 'single_f32'
    assert units_per_cu('fwd', 0, {}, True) == 16 and units_per_cu('fwd', 0, {}) == 32 and units_per_cu('bwd', F_HS64, {}) == 64
    assert env_flags({}) == 0 and env_flags({'ASR_LSTM_DFLAGS': '8192'}) == F_CU16 and env_flags({'ASR_LSTM_DFLAGS': '512x'}) == F_HS64


@pytest.mark.parametrize('group', list(CASES))
def test_bounds_stay_under_the_ceiling(group):
    """8 E32 -- the float32 evaluation of the same recurrence against the float64 one -- is at most 1e-5 max(1, max|ref|)
    for every tensor of every listed case, and nonzero; the gradients are large enough that zeros cannot pass; the empty
    row and tile give zeros; the clip cases have an active clip, the blocking ones 2 % .. 90 % of the valid states clamped
    and, in fp32, CLIP_GAP free on both sides of the clip.  bf16 cases: the reference's own rounding flips (the float32
    against the float64 evaluation of the rounded recurrence) use at most a third of every bf16 bound, except that one
    flipped h is one bf16 ulp, 2^-8, of the two the bound on hout allows."""
    for c in CASES[group]:
        data = case_data(c.name)
        ref = data['ref']
        for k in FWD_TENSORS + BWD_TENSORS:
            assert 0.0 < bound(data, k) == MARGIN * data['e32'][k] <= CEILING_REL * max(1.0, np.abs(ref[k]).max()), (c.name, k)
        assert np.abs(ref['dgates']).max() > 0.1 and np.abs(ref['dpeep'][:, :3]).max() > 0.1 and np.abs(ref['dpeep'][:, 3:]).max() > 0.1
        empty = [2] + (list(range(16, 32)) if c.B >= 32 else [])
        assert np.abs(ref['c_final'][:, empty]).max() == 0.0 and np.abs(ref['hout'][:, empty]).max() == 0.0
        assert np.abs(ref['dgates'][:, empty]).max() == 0.0
        valid = np.broadcast_to(data['valid'], ref['cs'].shape)
        for r in [ref] + ([data['refr']] if c.dtype == 'bf16' else []):
            if c.clip:
                assert np.abs(r['cs']).max() == c.clip, c.name
            if c.block:
                assert 0.02 < np.mean(np.abs(r['cs'][valid]) >= c.clip) < 0.9, c.name
        if c.block and c.dtype == 'f32':
            assert clip_gap(ref['cs_raw'], c.clip) >= CLIP_GAP >= 4 * bound(data, 'cs'), c.name
        if c.dtype == 'bf16':
            for k, v in bf16_own_figures(c.name).items():
                assert v <= (2.0 ** -8 if k == 'hout_max' else BF16_BOUNDS[k] / 3), (c.name, k, v)
