"""TEST INFRASTRUCTURE of tests/test_gpu_gru_variants.py and tests/test_gru_variants_host.py: the GRU recurrence of
csrc/gru.hip and of the two GRU cluster kernels of csrc/gru_cluster.hip, as

  * a plain reference (gru_reference): the recurrence of models/encoders/core/gru.py on hoisted x-projections, written
    with explicit per-frame loops and hand-written backward formulas in numpy -- float64 for the reference, float32 for
    the yardstick of the bounds.  Written apart from tests/_cpu_ops.py::_gru_fwd (torch + autograd) so that the host
    test can hold one against the other;
  * the dispatch rule (expected_form): the conditions of asr_gru_fwd / asr_gru_bwd / asr_cluster_gru_*_try /
    gru_persistent_ok restated, so that every device call of the tests can assert the one counter of
    ops.gru_kernel_counts it must move;
  * the case lists, each case the smallest that reaches its path.

Layouts (csrc/gru.hip): xg [T,B,ndir,2H] (r | u columns), xc, r, u, c, rh [T,B,ndir,H], hout [T,B,ndir*H],
h_final [ndir,B,H], wgh [ndir,H,2H], wch [ndir,H,H]; dgate like xg, dcand like xc.  Direction 1 is dynamic_rnn's reversed
pass: at step s a row of length L works on frame L - 1 - s.  Frames at or past a row's length: hout = rh = 0,
dgate = dcand = 0, the state is carried; r, u, c there are unspecified on the device (zero here).

Bounds.  E32 = the largest distance of the float32 evaluation of gru_reference from its float64 evaluation, per case and
tensor: the reference's own rounding noise at that shape and length.  A device tensor must lie within MARGIN * E32 = 8 E32
of the float64 reference (the margin: another summation order -- MFMA k-chunks, eight waves --, the three-term bf16 split
that keeps six of nine cross products, the device's exp / tanh), and, as a condition on the cases rather than a
measurement, 8 E32 may not exceed CEILING: 1e-5 for forward tensors, 2e-5 for gradients.  With these inputs a misplaced
weight element or batch row moves a value by 1e-2 or more."""
import collections
import functools

import numpy as np

XCH_BYTES = 64 << 20                      # csrc/common.h: ASR_XCH_BYTES
XCH_HALF = ((XCH_BYTES - 256) // 2) & ~255  # csrc/cluster_launch.h: one of the two exchange areas
XHDR = 16                                 # csrc/cluster_xch.h: header granules per cluster
LDS_LIMIT = 160 * 1024
ROOM = (192 << 20) - XCH_BYTES            # scratch below the exchange area of a handle with asr_create's 192 MiB arena
CLUSTER_WIDTHS = (64, 128, 256, 320)
FORMS = ('cluster', 'persistent', 'per_step')
COUNTER_KEYS = tuple('%s_%s' % (p, f) for p in ('fwd', 'bwd') for f in FORMS)   # ops.gru_kernel_counts, in its order
MARGIN = 8.0
CEILING = {'fwd': 1e-5, 'bwd': 2e-5}
FWD_TENSORS = ('r', 'u', 'c', 'rh', 'hout', 'h_final')
BWD_TENSORS = ('dgate', 'dcand')


# ---------------------------------------------------------------- the dispatch rule
def persistent_lds(pass_, H):
    """Dynamic LDS of the persistent kernels: three 16 x (H + 4) images forward; dc_pre, [dr_pre | du_pre], dh_rec and
    dh u backward."""
    return 3 * 16 * (H + 4) * 4 if pass_ == 'fwd' else 16 * (3 * (H + 4) + 2 * H + 4) * 4


def cluster_env_on(env):
    """What the cluster launchers read from the environment: ASR_GRU_CLUSTER per call; ASR_LSTM_CLUSTER and
    ASR_LSTM_CLUSTER_F32 once per process."""
    return not any(env.get(k, '')[:1] == '0' for k in ('ASR_GRU_CLUSTER', 'ASR_LSTM_CLUSTER', 'ASR_LSTM_CLUSTER_F32'))


def cluster_tiles_per_launch(pass_, H, B, ndir, cu_budget, num_cu):
    """cluster_launch_plan for the GRU clusters (G = H / 32 CUs each): tiles of 16 rows one launch holds; 0 = no plan."""
    G, tiles = H // 32, B // 16
    budget = num_cu if (cu_budget <= 0 or cu_budget > num_cu) else cu_budget
    per = (budget // (8 * G)) * 8 // ndir
    if per < 1 or tiles < 1:
        return 0
    per = min(per, tiles)
    cl_bytes = (XHDR + (4 if pass_ == 'fwd' else 6) * G * 16 * 32) * 8
    return min(per, XCH_HALF // (ndir * cl_bytes))


def expected_form(pass_, H, B, ndir, T, persistent_switch=True, cluster_env=True, cu_budget=0, num_cu=256,
                  scratch_room=ROOM):
    """The form asr_gru_fwd (pass_ 'fwd') / asr_gru_bwd ('bwd') ends in.  persistent_switch: asr_debug_set_gru_persistent
    (off = launch per step, the clusters too); cluster_env: cluster_env_on; cu_budget: asr_debug_set_cluster_cu_budget
    (0 = the device's num_cu); scratch_room: the handle's scratch less the exchange area (negative: none at all)."""
    assert pass_ in ('fwd', 'bwd') and B > 0 and B % 16 == 0 and H > 0 and H % 16 == 0 and ndir in (1, 2) and T >= 0
    if (persistent_switch and cluster_env and H in CLUSTER_WIDTHS and 1 <= T < 65536
            and T * B * ndir * 2 * H < (1 << 31) and scratch_room >= 0
            and cluster_tiles_per_launch(pass_, H, B, ndir, cu_budget, num_cu) >= 1):
        return 'cluster'
    if (persistent_switch and H <= 512 and persistent_lds(pass_, H) <= LDS_LIMIT and scratch_room > 0
            and ndir * 3 * H * H * 4 <= scratch_room):
        return 'persistent'
    return 'per_step'


# ---------------------------------------------------------------- the reference
def _sigmoid(x):
    return 1 / (1 + np.exp(-x))


def gru_reference(xg, xc, wgh, wch, seq_len, H, ndir, dout=None, d_h_final=None, dtype=np.float64):
    """The recurrence in `dtype`, frame by frame.  Returns dict(r, u, c, rh [T,B,ndir*H], hout [T,B,ndir*H],
    h_final [ndir,B,H]) and, given dout [T,B,ndir*H] (d_h_final [ndir,B,H] or None = zeros), dgate [T,B,ndir*2H] and
    dcand [T,B,ndir*H]: the gradients at the pre-activations of [r | u] and of c.  Nothing at or past a row's length is
    read."""
    T, B = xg.shape[0], xg.shape[1]
    xg = np.asarray(xg, dtype).reshape(T, B, ndir, 2 * H)
    xc = np.asarray(xc, dtype).reshape(T, B, ndir, H)
    wgh, wch = np.asarray(wgh, dtype), np.asarray(wch, dtype)
    lens = np.clip(np.asarray(seq_len).astype(np.int64), 0, T)
    z = lambda *s: np.zeros(s, dtype)                                            # noqa: E731
    r, u, c, rh, hout = (z(T, B, ndir, H) for _ in range(5))
    h_final = z(ndir, B, H)
    hprev = z(ndir, T, B, H)                                                     # the state a row entered step s with
    steps = []                                                                   # (d, s, rows, frames) of the forward
    for d in range(ndir):
        h = z(B, H)
        for s in range(T):
            a = np.nonzero(s < lens)[0]
            if a.size == 0:
                break
            f = lens[a] - 1 - s if d == 1 else np.full(a.size, s)
            hp = h[a]
            hprev[d, s, a] = hp
            g = _sigmoid(xg[f, a, d] + hp @ wgh[d])
            rr, uu = g[:, :H], g[:, H:]
            rhh = rr * hp
            cc = np.tanh(xc[f, a, d] + rhh @ wch[d])
            hn = uu * hp + (1 - uu) * cc
            r[f, a, d], u[f, a, d], c[f, a, d], rh[f, a, d], hout[f, a, d] = rr, uu, cc, rhh, hn
            h[a] = hn
            steps.append((d, s, a, f))
        h_final[d] = h
    res = dict(r=r.reshape(T, B, ndir * H), u=u.reshape(T, B, ndir * H), c=c.reshape(T, B, ndir * H),
               rh=rh.reshape(T, B, ndir * H), hout=hout.reshape(T, B, ndir * H), h_final=h_final)
    if dout is None:
        return res
    dout = np.asarray(dout, dtype).reshape(T, B, ndir, H)
    dgate, dcand = z(T, B, ndir, 2 * H), z(T, B, ndir, H)
    dh_rec = z(ndir, B, H) if d_h_final is None else np.array(d_h_final, dtype)
    for d, s, a, f in reversed(steps):                                           # each direction's steps run backwards
        hp, rr, uu, cc = hprev[d, s, a], r[f, a, d], u[f, a, d], c[f, a, d]
        dh = dout[f, a, d] + dh_rec[d, a]
        du_pre = dh * (hp - cc) * uu * (1 - uu)
        dc_pre = dh * (1 - uu) * (1 - cc * cc)
        drh = dc_pre @ wch[d].T
        dr_pre = drh * hp * rr * (1 - rr)
        dg = np.concatenate([dr_pre, du_pre], 1)
        dgate[f, a, d], dcand[f, a, d] = dg, dc_pre
        dh_rec[d, a] = dh * uu + drh * rr + dg @ wgh[d].T
    res['dgate'], res['dcand'] = dgate.reshape(T, B, ndir * 2 * H), dcand.reshape(T, B, ndir * H)
    return res


# ---------------------------------------------------------------- the cases
# fwd / bwd: how the pass is set up -- 'default' (switch on, ASR_GRU_CLUSTER unset), 'cluster_off' (ASR_GRU_CLUSTER=0),
# 'switch_off' (asr_debug_set_gru_persistent(0)).  T frames are allocated, row 0 has T - pad of them (pad > 0: tmax =
# max(seq_len) < T beside tmax = T).  dhf: whether a final-state gradient is fed in.
Case = collections.namedtuple('Case', 'name H B ndir T fwd bwd pad dhf')
SETUPS = {'default': (True, None), 'cluster_off': (True, '0'), 'switch_off': (False, None)}   # (switch, ASR_GRU_CLUSTER)


def _case(name, H, B, ndir, T, fwd='default', bwd=None, pad=0, dhf=True):
    return Case(name, H, B, ndir, T, fwd, bwd or fwd, pad, dhf)


CASES = collections.OrderedDict()
# clusters of H / 32 CUs per (direction, 16-row tile): every width x one tile both directions, two tiles one direction
# (the second of zero length), three tiles both directions
CASES['cluster'] = [_case('cl%d_%dx%d' % (H, ndir, B), H, B, ndir, T)
                    for H, Ts in ((64, (23, 31, 14)), (128, (19, 12, 27)), (256, (17, 21, 9)), (320, (13, 16, 11)))
                    for (ndir, B), T in zip(((2, 16), (1, 32), (2, 48)), Ts)]
# widths the clusters never take.  gp_tile walks k in chunks of eight 16-wide groups plus a tail: H = 16 one group, 48 tail
# only, 144 one chunk + one group (backward gates, K = 2H: two chunks + two), 496 the largest persistent backward
# (159 744 bytes of LDS), 512 forward persistent and backward per step on the persistent forward's activations
CASES['persistent'] = [_case('p16', 16, 16, 2, 21), _case('p48', 48, 32, 1, 18), _case('p144', 144, 16, 2, 15),
                       _case('p496', 496, 16, 2, 3), _case('p512', 512, 16, 2, 3)]
# the clusters' widths on one CU: 64 half a chunk, 128 exactly one chunk forward and two backward, 320 two chunks + four
CASES['persistent_cluster_off'] = [_case('p64', 64, 32, 2, 22, 'cluster_off'), _case('p128', 128, 16, 2, 16, 'cluster_off'),
                                   _case('p320', 320, 16, 1, 9, 'cluster_off')]
CASES['per_step'] = [_case('s16', 16, 16, 2, 20, 'switch_off'), _case('s48', 48, 32, 1, 17, 'switch_off'),
                     _case('s128', 128, 32, 2, 11, 'switch_off'), _case('s320', 320, 16, 1, 7, 'switch_off'),
                     _case('s528', 528, 16, 2, 3)]
# a backward form on another forward form's saved tensors (p512 above: per-step backward after the persistent forward)
CASES['mixed'] = [_case('m128_step_pers', 128, 16, 2, 10, 'switch_off', 'cluster_off'),
                  _case('m128_step_cl', 128, 16, 2, 10, 'switch_off', 'default'),
                  _case('m128_pers_step', 128, 16, 2, 10, 'cluster_off', 'switch_off')]
# T = 1; tmax = max(seq_len) < T; no final-state gradient -- each on every form
CASES['edges'] = [_case('%s_%s' % (tag, en), H, B, ndir, T, setup, pad=pad, dhf=dhf)
                  for tag, H, B, ndir, setup in (('cl128', 128, 16, 2, 'default'), ('p48', 48, 16, 1, 'default'),
                                                 ('p64', 64, 16, 2, 'cluster_off'), ('s48', 48, 16, 2, 'switch_off'))
                  for en, T, pad, dhf in (('t1', 1, 0, True), ('pad3', 12, 3, True), ('nodhf', 8, 0, False))]
ALL_CASES = [c for cs in CASES.values() for c in cs]
BY_NAME = {c.name: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)


def case_lengths(case):
    """Row 0 full (T - pad), row 1 of length 1, row 2 empty, the rest ragged in [1, T - pad]; for B >= 32 the whole
    second 16-row tile is empty."""
    rng = np.random.RandomState(case.H * 7 + case.B + case.T)
    full = case.T - case.pad
    sl = rng.randint(1, full + 1, size=case.B).astype(np.int32)
    sl[0], sl[1], sl[2] = full, 1, 0
    if case.B >= 32:
        sl[16:32] = 0
    return sl


def case_form(case, pass_, cluster_env=True, num_cu=256, scratch_room=ROOM):
    return expected_form(pass_, case.H, case.B, case.ndir, case.T, SETUPS[getattr(case, pass_)][0],
                         cluster_env and SETUPS[getattr(case, pass_)][1] != '0', 0, num_cu, scratch_room)


@functools.lru_cache(maxsize=None)
def case_data(name):
    """Inputs (float32), the float64 reference, and E32 per tensor -- computed once per case and shared; treat as
    read-only."""
    case = BY_NAME[name]
    H, B, ndir, T = case.H, case.B, case.ndir, case.T
    rng = np.random.RandomState(1000 + sum(ord(ch) for ch in name) + H + T)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)                           # noqa: E731
    inp = dict(xg=f32(rng.randn(T, B, ndir * 2 * H) * 0.5), xc=f32(rng.randn(T, B, ndir * H) * 0.5),
               wgh=f32(rng.randn(ndir, H, 2 * H) * 0.08), wch=f32(rng.randn(ndir, H, H) * 0.08),
               dout=f32(rng.randn(T, B, ndir * H) * 0.3), dhf=f32(rng.randn(ndir, B, H) * 0.3) if case.dhf else None,
               sl=case_lengths(case))
    args = (inp['xg'], inp['xc'], inp['wgh'], inp['wch'], inp['sl'], H, ndir, inp['dout'], inp['dhf'])
    ref = gru_reference(*args, dtype=np.float64)
    r32 = gru_reference(*args, dtype=np.float32)
    assert all(v.dtype == np.float32 for v in r32.values())
    e32 = {k: float(np.abs(r32[k].astype(np.float64) - ref[k]).max()) for k in ref}
    valid = (np.arange(T)[:, None] < inp['sl'][None, :])[:, :, None]               # [T,B,1]: the row works on the frame
    for v in list(inp.values()) + list(ref.values()) + [valid]:
        if v is not None:
            v.setflags(write=False)
    return dict(case=case, inp=inp, ref=ref, e32=e32, valid=valid)


def bound(data, tensor):
    return MARGIN * data['e32'][tensor]
