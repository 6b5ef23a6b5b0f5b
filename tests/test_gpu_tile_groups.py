"""GPU: cluster recurrences in tile groups.  A batch that needs more clusters than the chip has CUs for runs as several
launches over consecutive tile ranges of the same kernels (csrc/cluster_launch.h).  A cluster never talks to another
cluster, so the result must be the one-launch result BIT FOR BIT; asr_debug_set_cluster_cu_budget lowers the number of
co-resident workgroups a launch may use so that the group loop, a partial last group and every kernel family run at
B = 80 - 144 instead of B = 272+; the counters of asr_recurrence_path_counts say which path ran."""
import numpy as np
import pytest
import torch

from oracle import lstm as olstm

import test_gpu_ops as tgo

pytestmark = pytest.mark.gpu


def _ops():
    from tensorflow_end2end_speech_recognition_amd import ops
    return ops


@pytest.fixture
def budget():
    ops = _ops()
    yield ops.debug_set_cluster_cu_budget
    ops.debug_set_cluster_cu_budget(0)
    ops.debug_set_lstm_flags(0)


def _num_cu():
    from tensorflow_end2end_speech_recognition_amd import _lib
    return _lib.handle(0).info()[0]


def _counts(reset=False):
    ops = _ops()
    c = ops.recurrence_path_counts(0)
    if reset:
        ops.reset_recurrence_path_counts(0)
    return c


# ---------------------------------------------------------------- one LSTM layer through the C ABI
def _lens(rng, T, B, lo=1):
    """ragged, with a full-length and an empty row in the first AND in the last tile"""
    lens = rng.randint(lo, T + 1, size=B)
    lens[0], lens[3] = T, 0
    lens[B - 1], lens[B - 2] = T, 0
    return lens


def _case(rng, T, B, D, H, ndir, lens, bf16):
    x = rng.randn(B, T, D)
    if bf16:
        x = olstm.bf16_round(x)
    for b in range(B):
        x[b, lens[b]:] = 0
    ps = [olstm.init_lstm_params(rng, D, H, init=0.1) for _ in range(ndir)]
    for p in ps:
        p['b'] = torch.tensor(rng.uniform(-0.1, 0.1, 4 * H))
    dout = rng.randn(T, B, ndir * H)
    dfinal = (rng.randn(ndir, B, H) * 0.5, rng.randn(ndir, B, H) * 0.5)
    return x, ps, dout, dfinal


def _prep(cuda, x, ps, H, ndir, dtype):
    """x-projection, packed recurrent weights and peepholes on the device, once per case (tests/test_gpu_ops.py
    _run_hip_layer does the same in front of every run)."""
    ops = _ops()
    from tensorflow_end2end_speech_recognition_amd._lib import ASR_BF16, ASR_F32
    dt = ASR_BF16 if dtype == 'bf16' else ASR_F32
    tdt = torch.bfloat16 if dtype == 'bf16' else torch.float32
    B, T, D = x.shape
    xd = ops.bt_to_tb(torch.tensor(x, dtype=torch.float32, device=cuda), dt)
    xproj = torch.empty((T, B, ndir * 4 * H), dtype=torch.float32, device=cuda)
    whf = torch.empty((ndir, 4 * H * H), dtype=tdt, device=cuda)
    whb = torch.empty_like(whf)
    for d, p in enumerate(ps):
        kernel = torch.tensor(p['w'].detach().numpy(), dtype=torch.float32, device=cuda)
        bias = torch.tensor(p['b'].detach().numpy(), dtype=torch.float32, device=cuda)
        w = ops.lstm_prep_weights(kernel, bias, D, H, dt)
        ops.gemm(xd.view(T * B, D), w['wx_il'], bias=w['bias_il'], out=xproj.view(T * B, -1)[:, d * 4 * H:(d + 1) * 4 * H])
        whf[d].copy_(w['pf'])
        whb[d].copy_(w['pb'])
    peep = torch.tensor(np.stack([np.stack([p[k].detach().numpy() for k in ('wci', 'wcf', 'wco')]) for p in ps]),
                        dtype=torch.float32, device=cuda)
    return dict(xproj=xproj, whf=whf, whb=whb, peep=peep, dt=dt, H=H, ndir=ndir, T=T, B=B)


def _run(cuda, pr, lens, dout, dfinal, cell_clip, clip_no_grad=0.0, rows=None):
    """asr_lstm_fwd + asr_lstm_bwd_ex; rows = a slice of the batch to run on its own.  Results as _run_hip_layer gives
    them, with the saved activations of frames past a row's length (unspecified memory) set to zero."""
    ops = _ops()
    H, ndir, T = pr['H'], pr['ndir'], pr['T']
    rows = slice(0, pr['B']) if rows is None else rows
    xproj = pr['xproj'][:, rows].contiguous()
    B = xproj.shape[1]
    sl = torch.tensor(np.asarray(lens)[rows], dtype=torch.int32, device=cuda)
    gates, hout, cs, cf, hf = ops.lstm_fwd(xproj, pr['whf'], pr['peep'], sl, H, ndir, pr['dt'], 1.0, cell_clip)
    dcf = torch.tensor(dfinal[0][:, rows], dtype=torch.float32, device=cuda)
    dhf = torch.tensor(dfinal[1][:, rows], dtype=torch.float32, device=cuda)
    dg, dpeep = ops.lstm_bwd(torch.tensor(dout[:, rows], dtype=torch.float32, device=cuda), gates, cs, pr['whb'], pr['peep'],
                             sl, H, ndir, pr['dt'], dcf, dhf, clip_no_grad=clip_no_grad)
    pad = torch.arange(T, device=cuda).view(T, 1, 1) >= sl.view(1, B, 1)
    res = dict(hout=hout.float().cpu().numpy(), cs=cs.masked_fill(pad, 0.0).cpu().numpy(), cf=cf.cpu().numpy(),
               hf=hf.cpu().numpy())
    res['gates'] = gates.masked_fill(pad, 0.0).float().view(T, B, ndir, H, 4).permute(2, 0, 1, 4, 3).contiguous().cpu().numpy()
    res['dgates'] = dg.float().view(T, B, ndir, H, 4).permute(0, 1, 2, 4, 3).reshape(T, B, ndir * 4 * H).cpu().numpy()
    res['dpeep'] = dpeep.cpu().numpy()
    return res


KEYS = ('gates', 'hout', 'cs', 'cf', 'hf', 'dgates', 'dpeep')


def _same_bits(a, b, keys=KEYS):
    for k in keys:
        assert np.isfinite(a[k]).all(), k
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------- 1. forced groups: grouped == one launch, bit for bit
# (dtype, H, ndir, debug flags, G = workgroups per cluster of the form that runs, budget in units of 8 G, cell clip that
# blocks the gradient).  Flag 512: the H/64-CU forms (at fp32 H = 128: lstm_bwd_cluster8_f32_kernel); 4096: the exact-fp32
# kernels instead of the three-term split.  The bf16 launchers at H = 256 / 512 have two forms, H/32 CUs per cluster and
# then H/64, and the second holds twice the tiles in one launch: under a budget of one round of the H/32 form the batch
# has to exceed TWO of its groups before no form fits in one launch (per + per + 1 tiles).  The H/64 forms themselves
# run under flag 512, with and without the budget: the two forms sum in different orders and are not bit-identical.
FORCED = [('bf16', 256, 2, 0, 8, 1, 0.0), ('bf16', 256, 1, 0, 8, 1, 0.0), ('bf16', 256, 2, 512, 4, 1, 0.0),
          ('bf16', 320, 2, 0, 5, 1, 0.0), ('bf16', 320, 1, 0, 5, 1, 0.0),
          ('bf16', 512, 2, 512, 8, 1, 0.0), ('bf16', 512, 2, 0, 16, 1, 0.0), ('bf16', 512, 1, 512, 8, 1, 0.0),
          ('bf16', 256, 2, 0, 8, 1, 0.4),
          ('f32', 128, 2, 0, 4, 1, 0.0), ('f32', 128, 1, 4096, 4, 1, 0.0), ('f32', 128, 2, 512, 2, 1, 0.0),
          ('f32', 256, 2, 0, 8, 1, 0.0), ('f32', 256, 1, 4096, 8, 1, 0.0), ('f32', 256, 2, 4096, 8, 1, 0.4),
          ('f32', 320, 2, 0, 10, 1, 0.0), ('f32', 320, 1, 0, 10, 1, 0.0),
          ('f32', 512, 2, 0, 16, 1, 0.0), ('f32', 512, 1, 0, 16, 1, 0.0)]


@pytest.mark.parametrize('dtype,H,ndir,flags,G,rounds,clipz', FORCED)
def test_lstm_tile_groups_equal_one_launch_bit_for_bit(cuda, budget, dtype, H, ndir, flags, G, rounds, clipz):
    ops = _ops()
    bud = 8 * G * rounds
    if bud > _num_cu():
        pytest.skip('a cluster round of this form does not fit on this device')
    per = 8 * rounds // ndir                                   # tiles one launch holds under the budget
    tiles = per + 1                                            # a full group and a partial one ...
    if dtype == 'bf16' and H in (256, 512) and G == H // 32:
        tiles = 2 * per + 1                                    # ... past what the H/64 form holds in ONE launch
    B, T, D = 16 * tiles, 20, 24
    groups = ops.cluster_tile_groups(G, ndir, tiles, bud)
    assert len(groups) >= 2 and groups[-1][1] == 1
    rng = np.random.RandomState(H + 7 * ndir + flags)
    lens = _lens(rng, T, B)
    x, ps, dout, dfinal = _case(rng, T, B, D, H, ndir, lens, dtype == 'bf16')
    clip = clipz if clipz else 50.0
    ops.debug_set_lstm_flags(flags)
    pr = _prep(cuda, x, ps, H, ndir, dtype)
    res = {}
    for tag, b in (('one', 0), ('grouped', bud)):
        budget(b)
        _counts(reset=True)
        res[tag] = _run(cuda, pr, lens, dout, dfinal, clip, clipz)
        assert ops.check_async_errors(0) == 0
        c = _counts()
        n = len(groups) if b else 1
        # forward + BPTT: each call is n cluster launches, none on the single-CU kernels
        assert (c['lstm_cluster'], c['lstm_single_cu'], c['lstm_split_calls']) == (2 * n, 0, 2 if n > 1 else 0), (tag, c)
    if dtype == 'bf16' and H == 512 and G == 16:
        # without the budget this batch is ONE launch of the H/64 form (another summation order): the H/32 form's own
        # one-launch results are those of every group's utterances run alone
        assert len(ops.cluster_tile_groups(8, ndir, tiles, _num_cu())) == 1
        budget(0)
        parts = [_run(cuda, pr, lens, dout, dfinal, clip, clipz, rows=slice(16 * f, 16 * (f + n))) for f, n in groups]
        assert ops.check_async_errors(0) == 0
        axis = dict(gates=2, hout=1, cs=1, cf=1, hf=1, dgates=1)
        _same_bits(res['grouped'], {k: np.concatenate([q[k] for q in parts], axis=ax) for k, ax in axis.items()}, tuple(axis))
    else:
        _same_bits(res['grouped'], res['one'])
    assert np.abs(res['one']['dgates']).max() > 0.05 and np.abs(res['one']['dpeep'][:, :3]).max() > 0
    if clipz:
        assert np.abs(res['one']['cs']).max() == clipz        # the gradient-blocking clip is active


# ---------------------------------------------------------------- 2. GRU
@pytest.mark.parametrize('H', [64, 128, 256, 320])
@pytest.mark.parametrize('ndir', [1, 2])
def test_gru_tile_groups_equal_one_launch_bit_for_bit(cuda, budget, H, ndir):
    ops = _ops()
    G = H // 32
    bud = 8 * G
    per = 8 // ndir
    tiles = per + 1
    B, T = 16 * tiles, 20
    groups = ops.cluster_tile_groups(G, ndir, tiles, bud)
    assert groups == [(0, per), (per, 1)]
    # (inputs as in test_gru_cluster_forward_matches_the_single_cu_kernel)
    rng = np.random.RandomState(H + B + T)
    xg = torch.tensor(rng.randn(T, B, ndir * 2 * H) * 0.5, dtype=torch.float32, device=cuda)
    xc = torch.tensor(rng.randn(T, B, ndir * H) * 0.5, dtype=torch.float32, device=cuda)
    wgh = torch.tensor(rng.randn(ndir, H, 2 * H) * 0.08, dtype=torch.float32, device=cuda)
    wch = torch.tensor(rng.randn(ndir, H, H) * 0.08, dtype=torch.float32, device=cuda)
    sl_np = rng.randint(1, T + 1, size=B).astype(np.int32)
    sl_np[0], sl_np[B - 1] = T, T
    sl_np[17], sl_np[B - 2] = 0, 0
    sl = torch.tensor(sl_np, device=cuda)
    dout = torch.tensor(rng.randn(T, B, ndir * H) * 0.3, dtype=torch.float32, device=cuda)
    dhf = torch.tensor(rng.randn(ndir, B, H) * 0.3, dtype=torch.float32, device=cuda)
    wghT, wchT = wgh.transpose(1, 2).contiguous(), wch.transpose(1, 2).contiguous()
    valid = (torch.arange(T, device=cuda).view(T, 1) < sl.view(1, B)).view(T, B, 1)
    res = {}
    for tag, b in (('one', 0), ('grouped', bud)):
        budget(b)
        _counts(reset=True)
        saved = ops.gru_fwd(xg, xc, wgh, wch, sl, T, H, ndir)
        dg, dc = ops.gru_bwd(dout, dhf, saved, wghT, wchT, sl, T, H, ndir)
        assert ops.check_async_errors(0) == 0
        c = _counts()
        n = 2 if b else 1
        assert (c['gru_cluster'], c['gru_single_cu'], c['gru_split_calls']) == (2 * n, 0, 2 if n > 1 else 0), (tag, c)
        out = {k: saved[k] for k in ('hout', 'rh', 'h_final')}
        for k in ('r', 'u', 'c'):                              # (past a row's length: unspecified)
            out[k] = torch.where(valid, saved[k], torch.zeros_like(saved[k]))
        out['dgate'], out['dcand'] = dg, dc
        res[tag] = {k: v.clone() for k, v in out.items()}
    for k in res['one']:
        assert torch.isfinite(res['one'][k]).all(), k
        assert torch.equal(res['grouped'][k], res['one'][k]), k
    assert res['one']['dgate'].abs().max() > 0.05


# ---------------------------------------------------------------- 3. the real limit, no budget
def _bf16_parity(got, x, ps, lens, dout, dfinal, H, ndir, clip):
    """The checks and bounds of test_gpu_ops.test_lstm_cluster_bf16_gradient_parity_headline_shapes (oracle on the same
    bf16-rounded operands), restated on a result of _run."""
    B, T, D = x.shape
    xt = np.ascontiguousarray(np.transpose(x, (1, 0, 2)))
    R = olstm.bf16_round
    valid = (np.arange(T)[:, None] < lens[None, :])
    checks = []

    def chk(what, val, bound):
        checks.append((what, float(val), bound))
    for d in range(ndir):
        pn = {k: v.detach().numpy() for k, v in ps[d].items()}
        rev = d == 1
        tag = 'bw ' if rev else 'fw '
        f = olstm.layer_forward_np(xt, lens, pn, rev, 1.0, clip, True, round_fn=R)
        sl = slice(d * H, (d + 1) * H)
        e = np.abs(got['hout'][:, :, sl] - f['hout'])
        chk(tag + 'hout max abs', e.max(), 2 ** -7)
        chk(tag + 'hout mean abs', e.mean(), 2e-4)
        assert np.abs(got['hout'][:, :, sl][~valid]).max() == 0
        ecs = np.abs(got['cs'][:, :, sl] - f['cs'])[valid]
        chk(tag + 'cs max abs / max|cs|', ecs.max() / max(1.0, np.abs(f['cs']).max()), 2e-2)
        chk(tag + 'cs mean abs', ecs.mean(), 8e-4)
        eg = np.abs(got['gates'][d] - f['gates'])[valid]
        chk(tag + 'gates max abs', eg.max(), 2 ** -6)
        chk(tag + 'gates mean abs', eg.mean(), 3.5e-4)
        chk(tag + 'c_final max abs', np.abs(got['cf'][d] - f['c_final']).max(), 2e-2)
        chk(tag + 'h_final max abs', np.abs(got['hf'][d] - f['h_final']).max(), 5e-3)
        dg_dev = got['dgates'][:, :, d * 4 * H:(d + 1) * 4 * H].reshape(T, B, 4, H)
        g_dev = np.where(valid[:, :, None, None], got['gates'][d], 0.0)
        c_dev = np.where(valid[:, :, None], got['cs'][:, :, sl], 0.0)
        bwd = olstm.layer_backward_np(dout[:, :, sl], g_dev, c_dev, lens, pn, rev, True, dfinal[0][d], dfinal[1][d], round_fn=R)
        mx, mean = tgo._err_stats(dg_dev, bwd['dgates'])
        chk(tag + 'dgates|device activations max rel', mx, 1.5e-2)
        chk(tag + 'dgates|device activations mean rel', mean, 2.5e-3)
        assert np.abs(dg_dev[~valid]).max() == 0
        chk(tag + 'dpeep|device activations', tgo._rel(got['dpeep'][d, :3], bwd['dpeep']), 4e-3)
        chk(tag + 'db|device activations', tgo._rel(got['dpeep'][d, 3:7].reshape(-1), bwd['db']), 3e-3)
        full = olstm.layer_backward_np(dout[:, :, sl], f['gates'], f['cs'], lens, pn, rev, True, dfinal[0][d], dfinal[1][d],
                                       round_fn=R)
        mx, mean = tgo._err_stats(dg_dev, full['dgates'])
        chk(tag + 'dgates max rel', mx, 2e-2)
        chk(tag + 'dgates mean rel', mean, 6e-3)
        chk(tag + 'dpeep', tgo._rel(got['dpeep'][d, :3], full['dpeep']), 6e-3)
        chk(tag + 'db', tgo._rel(got['dpeep'][d, 3:7].reshape(-1), full['db']), 6e-3)
        dw_ref, dx_ref = olstm.layer_param_grads_np(xt, f['hout'], full['dgates'], lens, pn, rev, round_fn=R)
        dw_dev, dx_dev = olstm.layer_param_grads_np(xt, got['hout'][:, :, sl].astype(np.float64), dg_dev.astype(np.float64),
                                                    lens, pn, rev, round_fn=R)
        chk(tag + 'dW_x', tgo._rel(dw_dev[:D], dw_ref[:D]), 1e-2)
        chk(tag + 'dW_h', tgo._rel(dw_dev[D:], dw_ref[D:]), 7e-3)
        chk(tag + 'dx', tgo._rel(dx_dev, dx_ref), 1e-2)
    table = '\n'.join('%-44s %.3e  (bound %.1e)%s' % (w, v, bnd, '' if v <= bnd else '   <-- FAIL') for w, v, bnd in checks)
    print('\nH=%d B=%d T=%d\n%s' % (H, B, T, table))
    assert all(v <= bnd for _, v, bnd in checks), table


def _f32_parity(got, x, ps, lens, dout, dfinal, H, ndir, clip):
    """The checks and bounds of test_gpu_ops.test_lstm_cluster_f32_long_sequences (fp64 oracle), restated."""
    B, T, D = x.shape
    ref = tgo._oracle_layer(x, ps, lens, ndir, clip, dout, dfinal)
    assert np.abs(got['hout'] - ref['hout']).max() < 5e-5
    assert np.abs(got['cf'] - ref['cf']).max() < 2e-4
    assert np.abs(got['hf'] - ref['hf']).max() < 5e-5
    dg = got['dgates'].astype(np.float64)
    xt = np.transpose(x, (1, 0, 2))
    hout = got['hout'].astype(np.float64)
    dx = np.zeros_like(xt)
    for d, p in enumerate(ps):
        g = dg[:, :, d * 4 * H:(d + 1) * 4 * H].reshape(T * B, 4 * H)
        w = p['w'].detach().numpy()
        hp = np.zeros((T, B, H))
        if d == 0:
            hp[1:] = hout[:-1, :, :H]
        else:
            hp[:-1] = hout[1:, :, H:2 * H]
        assert tgo._rel(np.concatenate([xt.reshape(T * B, D).T @ g, hp.reshape(T * B, H).T @ g], 0), ref['dw'][d]) < 2e-4
        assert tgo._rel(got['dpeep'][d, 3:7].reshape(-1), ref['db'][d]) < 2e-4
        dx += (g @ w[:D].T).reshape(T, B, D)
    assert tgo._rel(dx, ref['dx']) < 2e-4
    assert tgo._rel(got['dpeep'][:, :3], ref['dpeep']) < 2e-4
    for b in range(B):
        if lens[b] < T:
            assert np.abs(got['hout'][lens[b]:, b]).max() == 0
            assert np.abs(got['dgates'][lens[b]:, b]).max() == 0


def _first_batch_over_the_chip(forms, ndir, num_cu):
    """Smallest B (a multiple of 16) for which no form -- workgroups per cluster, in the launchers' order of preference --
    fits in one launch, and the plan of the first form that has one: what the launchers then run."""
    ops = _ops()
    for tiles in range(1, 4096):
        plans = [ops.cluster_tile_groups(G, ndir, tiles, num_cu) for G in forms]
        if all(len(p) != 1 for p in plans):
            return 16 * tiles, next(p for p in plans if p)
    raise AssertionError('no batch exceeds the chip')


@pytest.mark.parametrize('dtype,H,forms', [('f32', 256, (8,)), ('bf16', 256, (8, 4)), ('bf16', 512, (16, 8)), ('f32', 512, (16,))])
def test_batch_one_tile_over_the_chip_runs_on_clusters_in_groups(cuda, budget, dtype, H, forms):
    """The smallest batch that no form of the launcher takes in one launch on the device the test runs on.  On 256 CUs:
    fp32 H = 256 (one form, eight CUs per cluster) B = 272, 17 tiles = 16 + 1; fp32 H = 512 B = 144 = 8 + 1; bf16 H = 512
    B = 272 -- the H/64 form holds 16 tiles in one launch, the H/32 form is the first with a plan: 8 + 8 + 1; bf16 H = 256
    B = 528 -- its H/64 form (four CUs per cluster) takes up to 32 tiles in ONE launch, as it always has, so B = 272 in
    bf16 is no split (test_bf16_256_units_at_272_utterances_stays_one_launch_of_the_64_unit_form): 16 + 16 + 1."""
    ops = _ops()
    ndir, T, D, clip = 2, 9, 24, 50.0
    B, groups = _first_batch_over_the_chip(forms, ndir, _num_cu())
    assert len(groups) >= 2
    if dtype == 'f32' and H == 256 and _num_cu() == 256:
        assert B == 272 and groups == [(0, 16), (16, 1)]
    rng = np.random.RandomState(H + B)
    lens = _lens(rng, T, B, lo=T // 3)
    x, ps, dout, dfinal = _case(rng, T, B, D, H, ndir, lens, dtype == 'bf16')
    pr = _prep(cuda, x, ps, H, ndir, dtype)
    _counts(reset=True)
    got = _run(cuda, pr, lens, dout, dfinal, clip)
    assert ops.check_async_errors(0) == 0
    c = _counts()
    # forward and BPTT: one cluster launch per group each, nothing on the single-CU kernels
    assert (c['lstm_cluster'], c['lstm_single_cu'], c['lstm_split_calls']) == (2 * len(groups), 0, 2), c
    (_bf16_parity if dtype == 'bf16' else _f32_parity)(got, x, ps, lens, dout, dfinal, H, ndir, clip)
    # the first tile of the second group against a B = 16 call on those 16 utterances alone
    t0 = groups[1][0]
    rows = slice(16 * t0, 16 * t0 + 16)
    alone = _run(cuda, pr, lens, dout, dfinal, clip, rows=rows)
    assert ops.check_async_errors(0) == 0
    for k in ('hout', 'cs', 'dgates'):
        assert np.array_equal(got[k][:, rows], alone[k]), k
    for k in ('cf', 'hf'):
        assert np.array_equal(got[k][:, rows], alone[k]), k
    assert np.array_equal(got['gates'][:, :, rows], alone['gates'])


def test_bf16_256_units_at_272_utterances_stays_one_launch_of_the_64_unit_form(cuda, budget):
    """Shapes that fit in one launch keep their form and their single launch: 17 bidirectional tiles are one more than
    the H/32 form holds on 256 CUs, and the H/64 form takes them in one launch, before and after tile groups."""
    ops = _ops()
    H, ndir, T, D, clip = 256, 2, 9, 24, 50.0
    B = 16 * (ops.cluster_tile_groups(8, ndir, 4096, _num_cu())[0][1] + 1)
    if len(ops.cluster_tile_groups(4, ndir, B // 16, _num_cu())) != 1:
        pytest.skip('the 64-unit form does not hold this batch on this device')
    rng = np.random.RandomState(B)
    lens = _lens(rng, T, B, lo=T // 3)
    x, ps, dout, dfinal = _case(rng, T, B, D, H, ndir, lens, True)
    pr = _prep(cuda, x, ps, H, ndir, 'bf16')
    _counts(reset=True)
    got = _run(cuda, pr, lens, dout, dfinal, clip)
    assert ops.check_async_errors(0) == 0
    c = _counts()
    assert (c['lstm_cluster'], c['lstm_single_cu'], c['lstm_split_calls']) == (2, 0, 0), c
    ops.debug_set_lstm_flags(512)                            # the 64-unit form by request: the same bits
    _same_bits(_run(cuda, pr, lens, dout, dfinal, clip), got)


# ---------------------------------------------------------------- 4. model level
def _batch(rng, B, T, D, C):
    x = rng.randn(B, T, D).astype(np.float32)
    sl = rng.randint(max(2, T // 2), T + 1, size=B).astype(np.int32)
    sl[0] = T
    dense = np.full((B, max(1, T // 4)), -1, dtype=np.int64)
    for b in range(B):
        x[b, sl[b]:] = 0
        n = max(1, sl[b] // 4)
        dense[b, :n] = rng.randint(0, C, size=n)
    return x, sl, dense


def _train_step(build, x, dense, sl):
    """loss, every gradient and the updated parameters of one training step of a freshly built (seeded) model"""
    model = build()
    loss, _ = model.compute_loss(x, dense, sl, keep_prob=0.9)
    opt = model._set_optimizer('adam', 1e-3)
    gv = opt.compute_gradients(loss, model=model)
    grads = {name: g.detach().clone() for g, name in gv}
    model._clip_gradients(gv)
    opt.apply_gradients(gv)
    params = {k: v.detach().clone() for k, v in model.store.state_dict().items()}
    return float(loss.item()), grads, params


@pytest.mark.parametrize('enc,H,kw,bud,B', [('blstm', 256, dict(clip_activation=50, dtype='bf16'), 64, 144),
                                              ('bgru', 128, {}, 32, 80)])
def test_training_step_in_tile_groups_is_bit_identical(cuda, budget, enc, H, kw, bud, B):
    """Clusters of a bidirectional layer come eight to a round, i.e. four tiles: B = 80 is the smallest batch a budget can
    split (4 + 1); the bf16 LSTM's second form (H/64 CUs per cluster) holds eight tiles under the same budget, so there
    the smallest batch that no form takes in one launch is B = 144 (4 + 4 + 1)."""
    ops = _ops()
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    rng = np.random.RandomState(5)
    T, D, C = 24, 24, 12
    x, sl, dense = _batch(rng, B, T, D, C)

    def build():
        return CTC(enc, D, H, 2, C, parameter_init=0.1, clip_grad_norm=5.0, seed=4, device='cuda:0', **kw)
    kind = 'gru' if enc == 'bgru' else 'lstm'
    runs = {}
    for tag, b in (('one', 0), ('grouped', bud)):
        budget(b)
        _counts(reset=True)
        runs[tag] = _train_step(build, x, dense, sl)
        assert ops.check_async_errors(0) == 0
        c = _counts()
        assert c[kind + '_single_cu'] == 0 and c[kind + '_cluster'] > 0, (tag, c)
        assert (c[kind + '_split_calls'] > 0) == (b > 0), (tag, c)
    (l0, g0, p0), (l1, g1, p1) = runs['one'], runs['grouped']
    assert np.isfinite(l0) and l1 == l0
    for n in g0:
        assert torch.equal(g1[n], g0[n]), n
    for n in p0:
        assert torch.equal(p1[n], p0[n]), n


def test_blstm_step_at_a_batch_over_the_chip(cuda, budget):
    ops = _ops()
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    B, groups = _first_batch_over_the_chip((8, 4), 2, _num_cu())          # 528 on 256 CUs
    rng = np.random.RandomState(6)
    T, D, C = 12, 24, 12
    x, sl, dense = _batch(rng, B, T, D, C)
    model = CTC('blstm', D, 256, 2, C, parameter_init=0.1, clip_grad_norm=5.0, clip_activation=50, dtype='bf16', seed=4,
                device='cuda:0')
    _counts(reset=True)
    loss, _ = model.compute_loss(x, dense, sl, keep_prob=0.9)
    model.train(loss, 'adam', 1e-3)
    assert np.isfinite(float(loss.item()))
    assert ops.check_async_errors(0) == 0
    c = _counts()
    assert c['lstm_single_cu'] == 0 and c['lstm_split_calls'] == 4 and c['lstm_cluster'] == 4 * len(groups), c


# ---------------------------------------------------------------- 5. budget hygiene
@pytest.mark.parametrize('dtype,H', [('bf16', 256), ('f32', 128)])
def test_budget_can_only_lower_the_grid(cuda, budget, dtype, H):
    """A budget above the device's CU count is the device's CU count; one below a single cluster's size leaves no plan, so
    the call takes the single-CU kernels -- the counters say so -- and meets the same bounds."""
    ops = _ops()
    ndir, T, B, D, clip = 2, 9, 32, 24, 50.0
    rng = np.random.RandomState(H)
    lens = _lens(rng, T, B, lo=T // 3)
    x, ps, dout, dfinal = _case(rng, T, B, D, H, ndir, lens, dtype == 'bf16')
    pr = _prep(cuda, x, ps, H, ndir, dtype)
    res = {}
    for tag, b in (('default', 0), ('above', _num_cu() + 100), ('below', 8)):
        budget(b)
        _counts(reset=True)
        res[tag] = _run(cuda, pr, lens, dout, dfinal, clip)
        assert ops.check_async_errors(0) == 0
        c = _counts()
        want = (0, 2, 0) if tag == 'below' else (2, 0, 0)
        assert (c['lstm_cluster'], c['lstm_single_cu'], c['lstm_split_calls']) == want, (tag, c)
    _same_bits(res['above'], res['default'])
    (_bf16_parity if dtype == 'bf16' else _f32_parity)(res['below'], x, ps, lens, dout, dfinal, H, ndir, clip)
