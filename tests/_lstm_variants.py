"""TEST INFRASTRUCTURE of tests/test_gpu_lstm_variants.py and tests/test_lstm_variants_host.py: the LSTM recurrence of
csrc/lstm.hip (single-CU kernels) and csrc/lstm_cluster.hip / csrc/lstm_cluster_f32.hip (the cluster forms), as

  * a plain reference (lstm_forward / lstm_backward): LSTMBlockCell under dynamic_rnn on hoisted x-projections, written
    with explicit per-frame loops and hand-written BPTT in numpy -- float64 for the reference, float32 for the yardstick
    of the fp32 bounds, and with round_fn = bf16_round the rounding points of the bf16 kernels (W_h, the fed-back and
    emitted h, the saved gates, dG entering dG W_h^T: the list of oracle/lstm.py).  Written apart from oracle/lstm.py and
    tests/_cpu_ops.py so that the host test can hold them against each other;
  * the dispatch rule (expected_form): every condition of asr_lstm_fwd / lstm_bwd_impl, asr_cluster_fwd_try /
    asr_cluster_bwd_try, their _f32_ forms, cluster_launch_plan / cluster_tile_plan, units_per_cu and the forward split's
    T < 65536 restated, so that every device call of the tests can assert the one counter of ops.lstm_kernel_counts it
    must move;
  * the case lists, each case the smallest that reaches its path.

Layouts (csrc/lstm.hip): xproj, gates, dgates [T,B,ndir,H,4] with the four of a unit in the order i, g (candidate), f, o;
cs, hout, dout [T,B,ndir,H]; c_final, h_final and their gradients [ndir,B,H]; W_h [ndir,H,4H] with TensorFlow's column
blocks i | g | f | o; peep [ndir,3,H] = w_ci, w_cf, w_co; dpeep [ndir,7,H] = the three peephole gradients, then the bias
gradients of i, g, f, o.  Direction 1 is dynamic_rnn's reversed pass: at step s a row of length L works on frame
L - 1 - s.  Frames at or past a row's length: hout = 0, dgates = 0, the state is carried; gates and cs there are
unspecified on the device (zero here).

Bounds.  fp32 forms: E32 = the largest distance of the float32 evaluation of the reference from its float64 evaluation,
per case and tensor; a device tensor must lie within MARGIN * E32 = 8 E32 of the float64 reference (the margin: another
summation order -- MFMA k-chunks, partial sums of several CUs --, the three-term bf16 split, the device's exp / rcp gate
functions), and as a condition on the cases 8 E32 <= 1e-5 max(1, max|ref|).  bf16 forms: the project's bounds of
test_lstm_cluster_bf16_gradient_parity_headline_shapes, unchanged (BF16_BOUNDS), against the reference with round_fn; the
backward against lstm_backward fed the device's own saved activations.

Left out: T >= 65536 (where the forward split hands over to the exact kernel: not a few-second test), tile groups
(tests/test_gpu_tile_groups.py holds them bit for bit against one launch), and the ASR_LSTM_ABLATE builds."""
import collections
import functools

import numpy as np

XCH_BYTES = 64 << 20                        # csrc/common.h: ASR_XCH_BYTES
XCH_HALF = ((XCH_BYTES - 256) // 2) & ~255  # csrc/cluster_launch.h: one of the two exchange areas
XHDR = 16                                   # csrc/cluster_xch.h: header granules per cluster
SCRATCH = 192 << 20                         # asr_create's arena
LSTM_UNITS = (64, 128, 192, 256, 320, 512)  # ASR_H_DISPATCH
FORMS = ('bf16_cu16', 'bf16_hs32', 'bf16_hs64', 'f32_split', 'f32_hs32', 'f32_hs64', 'single_bf16', 'single_f32')
# ops.lstm_kernel_counts, in its order (the 16-CU form is forward only)
COUNTER_KEYS = tuple('fwd_' + f for f in FORMS) + tuple('bwd_' + f for f in FORMS[1:])
CLUSTER_FORMS = FORMS[:6]
# ASR_LSTM_DFLAGS / asr_debug_set_lstm_flags
F_WT, F_EARLY, F_HS64, F_XW8, F_XP, F_EXACT, F_CU16 = 16, 32, 512, 1024, 2048, 4096, 8192
MARGIN = 8.0
CEILING_REL = 1e-5
FWD_TENSORS = ('gates', 'cs', 'hout', 'c_final', 'h_final')
BWD_TENSORS = ('dgates', 'dpeep')
# bf16 operands: the bounds of test_lstm_cluster_bf16_gradient_parity_headline_shapes (tests/test_gpu_ops.py)
BF16_BOUNDS = {'hout_max': 2.0 ** -7, 'hout_mean': 2e-4, 'gates_max': 2.0 ** -6, 'gates_mean': 3.5e-4, 'cs_max_rel': 2e-2,
               'cs_mean': 8e-4, 'c_final': 2e-2, 'h_final': 5e-3, 'dgates_max_rel': 1.5e-2, 'dgates_mean_rel': 2.5e-3,
               'dpeep_rel': 4e-3, 'db_rel': 3e-3}


# ---------------------------------------------------------------- the dispatch rule
def _atoi(s):
    s, n, i = s.strip(), 0, 0
    neg = s[:1] == '-'
    i = 1 if s[:1] in ('-', '+') else 0
    while i < len(s) and s[i].isdigit():
        n, i = n * 10 + int(s[i]), i + 1
    return -n if neg else n


def _on(env, key):
    """A switch that is on unless the variable starts with '0'."""
    return env.get(key, '')[:1] != '0'


def env_flags(env):
    """The flags a process starts with: ASR_LSTM_DFLAGS, until asr_debug_set_lstm_flags replaces them."""
    return _atoi(env['ASR_LSTM_DFLAGS']) if 'ASR_LSTM_DFLAGS' in env else 0


def units_per_cu(pass_, flags, env, allow16=False):
    """units_per_cu of cluster_host.hip: 64 with flag bit 9 or ASR_LSTM_{FWD,BWD}_HS / ASR_LSTM_HS = 64, else 32; with
    allow16 (the bf16 forward at H = 256) 16 by default or when the variable says 16, inverted by flag bit 13."""
    if flags & F_HS64:
        return 64
    e = env.get('ASR_LSTM_FWD_HS' if pass_ == 'fwd' else 'ASR_LSTM_BWD_HS', env.get('ASR_LSTM_HS'))
    v = _atoi(e) if e is not None else 0
    if v == 64:
        return 64
    if not allow16:
        return 32
    cu16 = (v == 16) if e is not None else True
    return 16 if cu16 != bool(flags & F_CU16) else 32


def cluster_tile_plan(G, ndir, tiles, budget):
    """(tiles per full group, groups); (0, 0) = not even one tile of every direction fits."""
    if G < 1 or ndir < 1 or ndir > 8 or tiles < 1 or budget < 1:
        return 0, 0
    per = (budget // (8 * G)) * 8 // ndir
    if per < 1:
        return 0, 0
    per = min(per, tiles)
    return per, (tiles + per - 1) // per


def cluster_launch_plan(G, ndir, B, cl_bytes, grouped, cu_budget, num_cu):
    """Launches of one launcher call: 0 = the form does not apply; without `grouped` only a single launch counts."""
    tiles = B // 16
    budget = num_cu if (cu_budget <= 0 or cu_budget > num_cu) else cu_budget
    per, n = cluster_tile_plan(G, ndir, tiles, budget)
    area_tiles = XCH_HALF // (ndir * cl_bytes)
    if n and per > area_tiles:
        per = area_tiles
        n = (tiles + per - 1) // per if per else 0
    if n != 1 and not grouped:
        n = 0
    return n


def cl_bytes(pass_, dtype, H, hsu):
    """Exchange bytes per cluster: the five formulas of the launchers (bf16 forward incl. the 16-CU form, fp32 forward,
    and the BPTT kernels of both dtypes, which share one)."""
    G = H // hsu
    if pass_ == 'bwd':
        return (XHDR + 2 * G * G * (hsu // 16) * 64 * 2) * 8
    return (XHDR + 2 * G * 16 * (hsu // 2 if dtype == 'bf16' else hsu)) * 8


def expected_form(pass_, dtype, H, B, ndir, T, flags=0, cu_budget=0, num_cu=256, scratch_bytes=SCRATCH, env=None):
    """The form asr_lstm_fwd (pass_ 'fwd') / asr_lstm_bwd(_ex) ('bwd') ends in, one of FORMS; None for T = 0 (nothing is
    launched).  flags: what asr_debug_set_lstm_flags last set (env_flags(env) before the first call); cu_budget:
    asr_debug_set_cluster_cu_budget (0 or above num_cu = the device); scratch_bytes: asr_scratch_bytes; env: the
    ASR_LSTM_* variables, most of them read once per process."""
    env = {} if env is None else env
    assert pass_ in ('fwd', 'bwd') and dtype in ('bf16', 'f32') and B > 0 and B % 16 == 0 and ndir in (1, 2) and T >= 0
    assert T * B * ndir * H < 4294967295 and H in LSTM_UNITS
    if T == 0:
        return None
    cluster_on = _on(env, 'ASR_LSTM_CLUSTER')
    dbg = env.get('ASR_LSTM_DBG', '')[:1] == '1'            # the phase timers: their buffer exists

    def fits(hsu, grouped):
        if T * B * ndir * H >= (1 << 31) or scratch_bytes < XCH_BYTES:
            return False
        return cluster_launch_plan(H // hsu, ndir, B, cl_bytes(pass_, dtype, H, hsu), grouped, cu_budget, num_cu) >= 1

    hs = units_per_cu(pass_, flags, env)
    if dtype == 'bf16':
        if cluster_on and (H in (256, 512) or (H == 320 and _on(env, 'ASR_LSTM_CLUSTER_320'))):
            for grouped in (False, True):
                if H == 320:
                    if fits(64, grouped):
                        return 'bf16_hs64'
                    continue
                if (pass_ == 'fwd' and H == 256 and not grouped and units_per_cu('fwd', flags, env, True) == 16
                        and _on(env, 'ASR_LSTM_XW') and not (flags & F_XW8) and not dbg and fits(16, False)):
                    return 'bf16_cu16'
                if hs == 32 and fits(32, grouped):
                    return 'bf16_hs32'
                if fits(64, grouped):
                    return 'bf16_hs64'
        return 'single_bf16'
    if cluster_on and _on(env, 'ASR_LSTM_CLUSTER_F32'):
        split = _on(env, 'ASR_LSTM_F32_SPLIT') and not (flags & F_EXACT)
        for grouped in (False, True):
            if hs == 32:
                if H != 128 and not (_on(env, 'ASR_LSTM_CLUSTER_F32_WIDE') and H in (256, 320, 512)):
                    break
                if fits(32, grouped):
                    # (the BPTT split carries no 16-bit step tags: only the forward hands T >= 65536 to the exact kernel)
                    if H in (128, 256) and split and (pass_ == 'bwd' or T < 65536):
                        return 'f32_split'
                    return 'f32_hs32'
            elif H == 128 and fits(64, grouped):
                return 'f32_hs64'
    return 'single_f32'


# ---------------------------------------------------------------- the reference
def bf16_round(a):
    """Nearest-even bfloat16 of the float32 nearest to `a` (what a kernel that computes in fp32 stores), as float32."""
    x = np.ascontiguousarray(a, np.float32).view(np.uint32)
    r = (x + np.uint32(0x7fff) + ((x >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)
    return r.view(np.float32)


def _sigmoid(x):
    return 1 / (1 + np.exp(-x))


def _prep(wh, peep, H, ndir, dtype, round_fn):
    rnd = (lambda a: a) if round_fn is None else (lambda a: np.asarray(round_fn(a), dtype))
    wh = rnd(np.asarray(wh, dtype).reshape(ndir, H, 4 * H))
    pp = np.zeros((ndir, 3, H), dtype) if peep is None else np.asarray(peep, dtype).reshape(ndir, 3, H)
    return rnd, wh, pp


def lstm_forward(xproj, wh, peep, seq_len, H, ndir, forget_bias=1.0, cell_clip=0.0, dtype=np.float64, round_fn=None):
    """The recurrence in `dtype`, frame by frame.  Returns dict(gates [T,B,ndir,H,4] (rounded), cs [T,B,ndir,H],
    hout [T,B,ndir,H] (rounded), c_final, h_final [ndir,B,H] (unrounded, as the device keeps them), cs_raw).  cs holds the
    clipped state, cs_raw the state before the clip (the device does not save it).  Nothing at or past a row's length is
    read."""
    T, B = xproj.shape[0], xproj.shape[1]
    xp = np.asarray(xproj, dtype).reshape(T, B, ndir, H, 4)
    rnd, wh, pp = _prep(wh, peep, H, ndir, dtype, round_fn)
    lens = np.clip(np.asarray(seq_len).astype(np.int64), 0, T)
    fb, clip = dtype(forget_bias), dtype(cell_clip or 0.0)
    gates, cs, hout = np.zeros((T, B, ndir, H, 4), dtype), np.zeros((T, B, ndir, H), dtype), np.zeros((T, B, ndir, H), dtype)
    cs_raw = np.zeros((T, B, ndir, H), dtype)
    c_final, h_final = np.zeros((ndir, B, H), dtype), np.zeros((ndir, B, H), dtype)
    for d in range(ndir):
        c, h, hb = np.zeros((B, H), dtype), np.zeros((B, H), dtype), np.zeros((B, H), dtype)
        for s in range(T):
            a = np.nonzero(s < lens)[0]
            if a.size == 0:
                break
            f = lens[a] - 1 - s if d == 1 else np.full(a.size, s)
            z = xp[f, a, d] + (hb[a] @ wh[d]).reshape(a.size, 4, H).transpose(0, 2, 1)      # [n,H,4]: i, g, f, o
            cp = c[a]
            gi = _sigmoid(z[..., 0] + pp[d, 0] * cp)
            gg = np.tanh(z[..., 1])
            gf = _sigmoid(z[..., 2] + fb + pp[d, 1] * cp)
            cn = cs_raw[f, a, d] = gg * gi + cp * gf
            if clip > 0:
                cn = np.clip(cn, -clip, clip)
            go = _sigmoid(z[..., 3] + pp[d, 2] * cn)
            hn = np.tanh(cn) * go
            gates[f, a, d] = rnd(np.stack([gi, gg, gf, go], -1))
            cs[f, a, d] = cn
            hout[f, a, d] = hb[a] = rnd(hn)
            c[a], h[a] = cn, hn
        c_final[d], h_final[d] = c, h
    return dict(gates=gates, cs=cs, hout=hout, c_final=c_final, h_final=h_final, cs_raw=cs_raw)


def lstm_backward(dout, gates, cs, wh, peep, seq_len, H, ndir, d_c_final=None, d_h_final=None, clip_no_grad=0.0,
                  dtype=np.float64, round_fn=None):
    """BPTT by hand on saved gates [T,B,ndir,H,4] and cs.  The cell clip is straight-through (LSTMBlockCellGrad) unless
    clip_no_grad > 0: then a state with |cs| >= clip_no_grad passes nothing to its gates or to c_prev (tf.clip_by_value).
    Returns dgates [T,B,ndir,H,4] (rounded; zero at or past a length) and dpeep [ndir,7,H] (sums of the unrounded gate
    gradients, as the kernels form them).  Nothing at or past a row's length is read."""
    T, B = dout.shape[0], dout.shape[1]
    dout = np.asarray(dout, dtype).reshape(T, B, ndir, H)
    gates, cs = np.asarray(gates, dtype).reshape(T, B, ndir, H, 4), np.asarray(cs, dtype).reshape(T, B, ndir, H)
    rnd, wh, pp = _prep(wh, peep, H, ndir, dtype, round_fn)
    lens = np.clip(np.asarray(seq_len).astype(np.int64), 0, T)
    block = dtype(clip_no_grad or 0.0)
    dgates, dpeep = np.zeros((T, B, ndir, H, 4), dtype), np.zeros((ndir, 7, H), dtype)
    dh_rec = np.zeros((ndir, B, H), dtype) if d_h_final is None else np.array(d_h_final, dtype)
    dc_car = np.zeros((ndir, B, H), dtype) if d_c_final is None else np.array(d_c_final, dtype)
    for d in range(ndir):
        for s in range(int(lens.max()) - 1 if B else -1, -1, -1):
            a = np.nonzero(s < lens)[0]
            f = lens[a] - 1 - s if d == 1 else np.full(a.size, s)
            g4, c = gates[f, a, d], cs[f, a, d]
            gi, gg, gf, go = g4[..., 0], g4[..., 1], g4[..., 2], g4[..., 3]
            cp = cs[f + 1 if d == 1 else f - 1, a, d] if s > 0 else np.zeros_like(c)    # the frame of step s - 1
            dh = dout[f, a, d] + dh_rec[d, a]
            tc = np.tanh(c)
            d_o = dh * tc * go * (1 - go)
            dc = dc_car[d, a] + dh * go * (1 - tc * tc) + d_o * pp[d, 2]
            if block > 0:
                dc = np.where(np.abs(c) >= block, dtype(0), dc)
            d_g = dc * gi * (1 - gg * gg)
            d_i = dc * gg * gi * (1 - gi)
            d_f = dc * cp * gf * (1 - gf)
            dpeep[d] += np.stack([(d_i * cp).sum(0), (d_f * cp).sum(0), (d_o * c).sum(0), d_i.sum(0), d_g.sum(0), d_f.sum(0),
                                  d_o.sum(0)])
            dG = rnd(np.stack([d_i, d_g, d_f, d_o], -1))                                    # [n,H,4]
            dgates[f, a, d] = dG
            dc_car[d, a] = dc * gf + d_i * pp[d, 0] + d_f * pp[d, 1]
            dh_rec[d, a] = dG.transpose(0, 2, 1).reshape(a.size, 4 * H) @ wh[d].T
    return dict(dgates=dgates, dpeep=dpeep)


# ---------------------------------------------------------------- the cases
# fwd / bwd: the flags of asr_debug_set_lstm_flags for that pass; fb / bb: asr_debug_set_cluster_cu_budget for it
# (0 = the device).  T frames are allocated, row 0 has T - pad of them.  scale multiplies xproj (a driven cell for the clip
# cases); clip: the forward's cell clip; block: the backward gets clip_no_grad = clip; dfin: final-state gradients fed in.
# ff / bf: the form the case is written for (on 256 CUs with the default arena; the host test checks it).
Case = collections.namedtuple('Case', 'name dtype H B ndir T fwd bwd fb bb pad peep clip scale block dfin ff bf')
NDB = ((2, 16), (1, 32), (2, 48))
NONE = 1                                  # a CU budget under which no cluster form fits: the single-CU kernels

# how a (dtype, form family, H) is reached in-process: (forward flags, backward flags, budget, forward form, backward form)
_SETUP = {
    ('bf16', 'cu16', 256): (0, 0, 0, 'bf16_cu16', 'bf16_hs32'),                 # the default pairing at H = 256
    ('bf16', 'hs32', 256): (F_CU16, 0, 0, 'bf16_hs32', 'bf16_hs32'),
    ('bf16', 'hs32', 512): (0, 0, 0, 'bf16_hs32', 'bf16_hs32'),
    ('bf16', 'hs64', 256): (F_HS64, F_HS64, 0, 'bf16_hs64', 'bf16_hs64'),
    ('bf16', 'hs64', 320): (0, 0, 0, 'bf16_hs64', 'bf16_hs64'),
    ('bf16', 'hs64', 512): (F_HS64, F_HS64, 0, 'bf16_hs64', 'bf16_hs64'),
    ('f32', 'split', 128): (0, 0, 0, 'f32_split', 'f32_split'),
    ('f32', 'split', 256): (0, 0, 0, 'f32_split', 'f32_split'),
    ('f32', 'hs32', 128): (F_EXACT, F_EXACT, 0, 'f32_hs32', 'f32_hs32'),
    ('f32', 'hs32', 256): (F_EXACT, F_EXACT, 0, 'f32_hs32', 'f32_hs32'),
    ('f32', 'hs32', 320): (0, 0, 0, 'f32_hs32', 'f32_hs32'),
    ('f32', 'hs32', 512): (0, 0, 0, 'f32_hs32', 'f32_hs32'),
    ('f32', 'hs64', 128): (F_HS64, F_HS64, 0, 'f32_hs64', 'f32_hs64'),
}
for _dt in ('bf16', 'f32'):
    for _H in LSTM_UNITS:
        _SETUP[(_dt, 'single', _H)] = (0, 0, NONE, 'single_' + _dt, 'single_' + _dt)


def _case(name, dtype, fam, H, ndb, T, pad=0, peep=True, clip=0.0, scale=1.0, block=False, dfin=True, xf=0, xb=0,
          bwd_of=None, fb=None, bb=None, ff=None, bf=None):
    """fam: the family of _SETUP; xf / xb: flag bits added to the forward / backward; bwd_of: another (fam) whose backward
    set-up is used (mixed pairings); fb / bb / ff / bf override the budgets and the claimed forms."""
    f = _SETUP[(dtype, fam, H)]
    b = _SETUP[(dtype, bwd_of, H)] if bwd_of else f
    return Case(name, dtype, H, ndb[1], ndb[0], T, f[0] | xf, b[1] | xb, f[2] if fb is None else fb,
                b[2] if bb is None else bb, pad, peep, clip, scale, block, dfin, ff or f[3], bf or b[4])


CASES = collections.OrderedDict()
# every cluster form at every width it serves, and at one tile both directions, two tiles one direction (the second of
# zero length), three tiles both directions
CASES['cluster'] = [_case('%s_%s%d_%dx%d' % (dt, fam, H, nd, B), dt, fam, H, (nd, B), T)
                    for dt, fam, H, nd, B, T in (
    ('bf16', 'cu16', 256, 2, 16, 17), ('bf16', 'cu16', 256, 1, 32, 12), ('bf16', 'cu16', 256, 2, 48, 9),
    ('bf16', 'hs32', 256, 2, 16, 14), ('bf16', 'hs32', 256, 1, 32, 11), ('bf16', 'hs32', 512, 2, 48, 8),
    ('bf16', 'hs64', 256, 2, 48, 10), ('bf16', 'hs64', 320, 2, 16, 13), ('bf16', 'hs64', 512, 1, 32, 9),
    ('f32', 'split', 128, 2, 16, 19), ('f32', 'split', 128, 1, 32, 12), ('f32', 'split', 256, 2, 48, 9),
    ('f32', 'hs32', 128, 2, 48, 11), ('f32', 'hs32', 256, 2, 16, 13), ('f32', 'hs32', 320, 1, 32, 10),
    ('f32', 'hs32', 512, 2, 16, 8),
    ('f32', 'hs64', 128, 2, 16, 16), ('f32', 'hs64', 128, 1, 32, 13), ('f32', 'hs64', 128, 2, 48, 10))]
# the single-CU kernels at every width of the dispatch, in both dtypes: each (dtype, H) is its own instantiation (waves
# 4 / 8 / 12 / 16 / 10 / 16, LDS-resident chunk counts fwd_ksl / bwd_ksl, the double-buffered dG image up to H = 128 fp32 /
# 256 bf16).  64 and 192 (bf16 also 128) have no cluster form; the others are reached under a CU budget of 1
CASES['single'] = [_case('%s_single%d_%dx%d' % (dt, H, nd, B), dt, 'single', H, (nd, B), T)
                   for dt in ('bf16', 'f32')
                   for H, (nd, B), T in zip(LSTM_UNITS, (NDB[0], NDB[1]) * 3, (15, 12, 11, 10, 9, 7))]
# the fall-through ladder by CU budget at ndir = 2, B = 16 (cluster_tile_plan: a round of 8 clusters of G CUs must fit):
# H = 256 bf16, G = 16 / 8 / 4: 16-CU form >= 128, 32-unit form 64 .. 127, 64-unit form 32 .. 63, single-CU < 32 (the BPTT
# has no 16-CU form); H = 256 fp32, G = 8: split >= 64, no 64-unit form to fall to
CASES['ladder'] = [_case('bf16_256_budget%d' % n, 'bf16', 'cu16', 256, NDB[0], 6, fb=n, bb=n, ff=ff, bf=bf)
                   for n, ff, bf in ((128, 'bf16_cu16', 'bf16_hs32'), (127, 'bf16_hs32', 'bf16_hs32'),
                                     (64, 'bf16_hs32', 'bf16_hs32'), (63, 'bf16_hs64', 'bf16_hs64'),
                                     (32, 'bf16_hs64', 'bf16_hs64'), (31, 'single_bf16', 'single_bf16'))]
CASES['ladder'] += [_case('f32_256_budget%d' % n, 'f32', 'split', 256, NDB[0], 6, fb=n, bb=n, ff=ff, bf=ff)
                    for n, ff in ((64, 'f32_split'), (63, 'single_f32'))]
# a backward form on another forward form's saved gates and cs: every form saves them in the same layout
CASES['mixed'] = [
    _case('bf16_cu16_then_hs64', 'bf16', 'cu16', 256, NDB[0], 11, bwd_of='hs64'),
    _case('bf16_single_then_cluster', 'bf16', 'single', 256, NDB[1], 10, bwd_of='hs32'),
    _case('bf16_cluster_then_single', 'bf16', 'cu16', 256, NDB[1], 10, bwd_of='single'),
    _case('f32_single_then_cluster', 'f32', 'single', 128, NDB[0], 12, bwd_of='split'),
    _case('f32_cluster_then_single', 'f32', 'split', 128, NDB[0], 12, bwd_of='single'),
    _case('f32_split_then_exact', 'f32', 'split', 256, NDB[1], 9, bwd_of='hs32'),
    _case('f32_exact_then_split', 'f32', 'hs32', 256, NDB[1], 9, bwd_of='split')]
# template choices inside a form, each at one width per form it applies to: EARLY inverted (forward, not the 16-CU form);
# 8-byte exchange granules (bf16 forward; the 16-CU form has none and hands over to the 32-unit form); the other
# reduce-scatter slot layout (bf16 BPTT); the write-through exchange (every cluster kernel)
CASES['variants'] = [
    _case('early_bf16_hs32', 'bf16', 'hs32', 256, NDB[0], 9, xf=F_EARLY),
    _case('early_bf16_hs64', 'bf16', 'hs64', 320, NDB[0], 9, xf=F_EARLY),
    _case('early_f32_split', 'f32', 'split', 128, NDB[0], 9, xf=F_EARLY),
    _case('early_f32_hs32', 'f32', 'hs32', 320, NDB[0], 9, xf=F_EARLY),
    _case('early_f32_hs64', 'f32', 'hs64', 128, NDB[0], 9, xf=F_EARLY),
    _case('xw8_bf16_hs32', 'bf16', 'cu16', 256, NDB[0], 9, xf=F_XW8, ff='bf16_hs32'),
    _case('xw8_bf16_hs64', 'bf16', 'hs64', 512, NDB[0], 7, xf=F_XW8),
    _case('xp_bf16_hs32', 'bf16', 'cu16', 256, NDB[0], 9, xb=F_XP),
    _case('xp_bf16_hs64', 'bf16', 'hs64', 320, NDB[0], 9, xb=F_XP),
    _case('wt_bf16_cu16', 'bf16', 'cu16', 256, NDB[0], 8, xf=F_WT, xb=F_WT),
    _case('wt_bf16_hs32', 'bf16', 'hs32', 512, NDB[0], 7, xf=F_WT, xb=F_WT),
    _case('wt_bf16_hs64', 'bf16', 'hs64', 256, NDB[0], 8, xf=F_WT, xb=F_WT),
    _case('wt_f32_split', 'f32', 'split', 256, NDB[0], 8, xf=F_WT, xb=F_WT),
    _case('wt_f32_hs32', 'f32', 'hs32', 512, NDB[0], 7, xf=F_WT, xb=F_WT),
    _case('wt_f32_hs64', 'f32', 'hs64', 128, NDB[0], 8, xf=F_WT, xb=F_WT)]
# the gradient-blocking clip of asr_lstm_bwd_ex on every backward form, with an active clip (2 % .. 90 % of the valid
# states clamped).  fp32: the clamped set must be the same on the device as in the float64 reference, so the host test
# requires a gap on both sides of the clip that no state falls into before it is clamped (CLIP_GAP, at least four times
# the bound on cs; case_data draws the inputs again until the reference has it)
CASES['clip_block'] = [_case('block_%s_%s%d' % (dt, fam, H), dt, fam, H, NDB[0], 6, clip=0.5, scale=2.0, block=True)
                       for dt, fam, H in (('bf16', 'cu16', 256), ('bf16', 'hs64', 320), ('f32', 'split', 128),
                                          ('f32', 'hs32', 320), ('f32', 'hs64', 128), ('bf16', 'single', 192),
                                          ('f32', 'single', 64))]
CLIP_GAP = 2e-5
# edges, on every form (the eight pairings below reach all fifteen counters): T = 1, 2, 3; an odd and an even
# max(seq_len) in 33 .. 40 (the two-step unrolled loops); max(seq_len) = T - 3 (the zero-fill of the common padded tail);
# no peepholes; an active forward clip (max |cs| = clip exactly); no final-state gradients
EDGE_FORMS = (('bf16', 'cu16', 256), ('bf16', 'hs32', 512), ('bf16', 'hs64', 320), ('f32', 'split', 128),
              ('f32', 'hs32', 320), ('f32', 'hs64', 128), ('bf16', 'single', 128), ('f32', 'single', 192))
EDGE_KINDS = (('t1', dict(T=1)), ('t2', dict(T=2)), ('t3', dict(T=3)), ('odd', dict(T=37)), ('even', dict(T=36)),
              ('pad3', dict(T=12, pad=3)), ('nopeep', dict(T=7, peep=False)), ('clip', dict(T=8, clip=0.5, scale=4.0)),
              ('nodfin', dict(T=7, dfin=False)))
CASES['edges'] = [_case('%s_%s_%s%d' % (kind, dt, fam, H), dt, fam, H, NDB[i % 2], **kw)
                  for i, (dt, fam, H) in enumerate(EDGE_FORMS) for kind, kw in EDGE_KINDS]
ALL_CASES = [c for cs_ in CASES.values() for c in cs_]
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


def case_form(case, pass_, num_cu=256, scratch_bytes=SCRATCH, env=None):
    return expected_form(pass_, case.dtype, case.H, case.B, case.ndir, case.T, case.fwd if pass_ == 'fwd' else case.bwd,
                         case.fb if pass_ == 'fwd' else case.bb, num_cu, scratch_bytes, env)


def clip_gap(cs_raw, clip):
    """The least distance of a state before the clip from +-clip (padded frames hold zeros: `clip` itself)."""
    return float(np.abs(np.abs(cs_raw) - clip).min())


@functools.lru_cache(maxsize=None)
def case_data(name):
    """Inputs (float32), the float64 reference of both passes, E32 per tensor and, for a bf16 case, the float64 forward
    with the kernels' rounding points (`refr`) -- computed once per case and shared; treat as read-only."""
    case = BY_NAME[name]
    H, B, ndir, T = case.H, case.B, case.ndir, case.T
    f32 = lambda a: np.ascontiguousarray(a, np.float32)                           # noqa: E731
    block = case.clip if case.block else 0.0

    def run(dtype, round_fn=None):
        r = lstm_forward(inp['xproj'], inp['wh'], inp['peep'], inp['sl'], H, ndir, 1.0, case.clip, dtype, round_fn)
        r.update(lstm_backward(inp['dout'], r['gates'], r['cs'], inp['wh'], inp['peep'], inp['sl'], H, ndir, inp['dcf'],
                               inp['dhf'], block, dtype, round_fn))
        return r
    for attempt in range(32):
        rng = np.random.RandomState(2000 + sum(ord(ch) for ch in name) + H + T + 100000 * attempt)
        inp = dict(xproj=f32(rng.randn(T, B, ndir, H, 4) * case.scale), wh=f32(rng.uniform(-0.1, 0.1, (ndir, H, 4 * H))),
                   peep=f32(rng.uniform(-0.3, 0.3, (ndir, 3, H))) if case.peep else None,
                   dout=f32(rng.randn(T, B, ndir, H)), dcf=f32(rng.randn(ndir, B, H) * 0.5) if case.dfin else None,
                   dhf=f32(rng.randn(ndir, B, H) * 0.5) if case.dfin else None, sl=case_lengths(case))
        if case.dtype == 'bf16':
            inp['wh'] = bf16_round(inp['wh'])                # (what asr_lstm_prep_weights keeps of it)
        ref = run(np.float64)
        # fp32 with the gradient-blocking clip: inputs whose float64 states leave CLIP_GAP free below the clip, so that
        # the set of clamped states cannot depend on fp32 rounding (a condition on the reference alone; see CLIP_GAP)
        if not (block and case.dtype == 'f32') or clip_gap(ref['cs_raw'], case.clip) >= CLIP_GAP:
            break
    r32 = run(np.float32)
    assert all(v.dtype == np.float32 for v in r32.values())
    e32 = {k: float(np.abs(r32[k].astype(np.float64) - ref[k]).max()) for k in ref}
    out = dict(case=case, inp=inp, ref=ref, e32=e32)
    if case.dtype == 'bf16':
        out['refr'] = run(np.float64, bf16_round)
    out['valid'] = (np.arange(T)[:, None] < inp['sl'][None, :])[:, :, None, None]       # [T,B,1,1]: the row works on the frame
    for v in list(inp.values()) + list(ref.values()) + list(out.get('refr', {}).values()) + [out['valid']]:
        if v is not None:
            v.setflags(write=False)
    return out


def bound(data, tensor):
    return MARGIN * data['e32'][tensor]


def bf16_fwd_figures(a, ref, valid):
    """The forward figures BF16_BOUNDS bounds, of tensors `a` (gates and cs zeroed outside `valid`) against `ref`, as
    test_lstm_cluster_bf16_gradient_parity_headline_shapes forms them: hout over all frames, gates and cs over valid ones."""
    eh, eg, ec = np.abs(a['hout'] - ref['hout']), np.abs(a['gates'] - ref['gates']), np.abs(a['cs'] - ref['cs'])
    nv = max(int(np.broadcast_to(valid, eh.shape).sum()), 1)
    return dict(hout_max=eh.max(), hout_mean=eh.mean(), gates_max=eg.max(), gates_mean=eg.sum() / (4 * nv),
                cs_max_rel=ec.max() / max(1.0, np.abs(ref['cs']).max()), cs_mean=ec.sum() / nv,
                c_final=np.abs(a['c_final'] - ref['c_final']).max(), h_final=np.abs(a['h_final'] - ref['h_final']).max())


def bf16_bwd_figures(a, ref):
    """The backward figures BF16_BOUNDS bounds: dgates max / mean relative (tests/test_gpu_ops.py::_err_stats), the
    peephole and the bias gradients relative to their largest entry."""
    d = np.abs(a['dgates'] - ref['dgates'])
    rel = lambda x, y: np.abs(x - y).max() / max(np.abs(y).max(), 1e-30)           # noqa: E731
    return dict(dgates_max_rel=d.max() / max(np.abs(ref['dgates']).max(), 1e-30),
                dgates_mean_rel=d.mean() / max(np.abs(ref['dgates']).mean(), 1e-30),
                dpeep_rel=rel(a['dpeep'][:, :3], ref['dpeep'][:, :3]), db_rel=rel(a['dpeep'][:, 3:], ref['dpeep'][:, 3:]))


def bf16_own_figures(name):
    """The same figures between the float32 and the float64 evaluation of the ROUNDED reference of a bf16 case: what the
    reference's own rounding flips use of the bounds."""
    data = case_data(name)
    case, inp, rr = data['case'], data['inp'], data['refr']
    block = case.clip if case.block else 0.0
    f = lstm_forward(inp['xproj'], inp['wh'], inp['peep'], inp['sl'], case.H, case.ndir, 1.0, case.clip, np.float32, bf16_round)
    b = lstm_backward(inp['dout'], rr['gates'], rr['cs'], inp['wh'], inp['peep'], inp['sl'], case.H, case.ndir, inp['dcf'],
                      inp['dhf'], block, np.float32, bf16_round)
    figs = bf16_fwd_figures(f, rr, data['valid'])
    figs.update(bf16_bwd_figures(b, rr))
    return figs
