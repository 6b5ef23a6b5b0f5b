"""TEST INFRASTRUCTURE of tests/test_gpu_conv3x3_variants.py and of its child-process worker
(tests/_conv_variant_worker.py): the dispatch rule of csrc/conv3x3.hip restated in plain Python, the list of kernel
instantiations that rule can reach, and the checks of one 3x3 layer shape against fp64 references with the path counters
(ops.conv_path_counts) asserted launch by launch.

Bounds (none of them measured on the code under test): a bf16 result within one bf16 ulp of the fp64 reference
(+ 1e-5 max|ref| where values cancel) -- the criterion tests/test_gpu_cnn_zhang.py holds the same tiled kernel to at
K = 3840; fp32 results (data gradient, weight and bias gradient) within 1e-5 max|ref|; everything the library documents
as the same arithmetic in another launch shape, bit for bit."""
import hashlib
import os
import re

import torch

from _bf16_ulp import within_bf16_ulp

DROP = (0.9, 21, (4 << 32) + 3)          # keep_prob (1 / 0.9 is not exact: the scale must be formed alike), seed, offset
XCH_BYTES = 64 << 20                     # csrc/common.h: ASR_XCH_BYTES (xch_bytes_of_the_library reads it from there)
PAIRS = {(64, 64): (14, 16), (64, 128): (4, 16), (128, 128): (8, 16), (128, 64): (8, 16)}    # -> the MAXV instantiated


def xch_bytes_of_the_library():
    """ASR_XCH_BYTES as csrc/common.h defines it: the top of the scratch arena the weight-gradient slabs must leave alone."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'tensorflow_end2end_speech_recognition_amd', 'csrc', 'common.h')) as f:
        m = re.search(r'ASR_XCH_BYTES\s*=\s*\(size_t\)\s*(\d+)\s*<<\s*(\d+)\s*;', f.read())
    assert m, 'csrc/common.h no longer defines ASR_XCH_BYTES as (size_t)A << B'
    return int(m.group(1)) << int(m.group(2))


# ---------------------------------------------------------------- the dispatch rule
def switches(env=None):
    """The ASR_CONV_* switches as csrc/conv3x3.hip reads them: on unless the value starts with '0'; BN64 off unless '1'."""
    env = os.environ if env is None else env

    def on(name):
        return not env.get(name, '').startswith('0')
    return dict(img=on('ASR_CONV_IMG'), stream=on('ASR_CONV_STREAM'), w8=on('ASR_CONV_IMG_W8'),
                wgrad_img=on('ASR_CONV_WGRAD_IMG'), wgrad_tr=on('ASR_CONV_WGRAD_TR'),
                bn64=env.get('ASR_CONV_WGRAD_BN64', '').startswith('1'), wgrad_bias=on('ASR_CONV_WGRAD_BIAS'),
                split=on('ASR_CONV_WGRAD_SPLIT'))


def expected_conv(N, H, W, Cin, Cout, act, use_drop, sw=None, f32_out=False):
    """conv3x3_launch for one Cin -> Cout product over N images of H x W (the data gradient of a layer is the Cout -> Cin
    product): form, MAXV, nbuf, stream, w8, tile width -> the counters one launch bumps.
    act: 0 none, 1 ReLU, 2 gated data gradient (use_drop 0 / 1 / 2), 3 forward ReLU + dropout."""
    sw = sw or switches({})
    pair = 'pair_%d_%d' % (Cin, Cout) if (Cin, Cout) in PAIRS else 'pair_other'
    img_bytes = (H + 2) * (W + 2) * (2 * Cin + 16)
    nvec = H * W * Cin // 8
    if sw['img'] and pair != 'pair_other' and nvec <= 16 * 256 and img_bytes <= 156 * 1024 and N >= 64:
        nbuf = 2 if 2 * img_bytes <= 158 * 1024 else 1
        mv = -(-nvec // 256)
        actc = 0 if f32_out else ((4 if use_drop == 1 else 2) if act == 2 else act)
        w8 = (not f32_out) and Cin == 64 and sw['w8'] and mv <= 4 and actc == 3
        small, large = PAIRS[(Cin, Cout)]
        maxv = 2 if w8 else small if mv <= small else large
        stream = (not w8) and sw['stream'] and nbuf == 2 and (Cin, Cout) == (64, 64) and actc in (1, 3)
        keys = ['img', pair, 'maxv_%d' % maxv, 'act_%d' % actc, 'nbuf_%d' % nbuf]
        return keys + (['stream'] if stream else []) + (['w8'] if w8 else [])
    return ['tiled', pair, 'tiled_bn128' if Cout % 128 == 0 else 'tiled_bn64']


def expected_wgrad(N, H, W, Cin, Cout, bias, aligned, num_cu, scratch_room, sw=None):
    """conv3x3_bwd_weight_impl: the counters one weight-gradient call bumps (bias: asr_conv3x3_bwd_weight_bias; aligned:
    dw on a 16-byte boundary; scratch_room: the handle's scratch less the exchange area)."""
    sw = sw or switches({})
    HW = H * W
    nchunk = -(-HW // 32)
    lds = (H + 2) * (W + 2) * (2 * Cin + 16) + nchunk * 32 * (64 * 2 + 16)
    nth = Cin * 4
    mvx, mvy = -(-(HW * Cin // 8) // nth), -(-(HW * 8) // nth)
    mv = max(mvx, mvy)
    inb = bias and sw['wgrad_bias']
    slab = (9 * Cin + (Cin // 16 if inb else 0)) * Cout * 4
    wgs, cols = scratch_room // slab, Cout // 64
    if wgs * cols > num_cu:
        wgs = num_cu // cols
    wgs = min(wgs, N)
    if (sw['wgrad_img'] and (Cin == 64 or (Cin == 128 and mvx <= 4 and mvy <= 2)) and Cout % 64 == 0 and N >= 64
            and lds <= 158 * 1024 and mv <= 14 and nchunk * 2 >= mv and wgs >= 32):
        keys = ['wgrad_img_128' if Cin == 128 else 'wgrad_img_64_small' if mv <= 4 else 'wgrad_img_64_large']
        if Cin == 64 and sw['split']:
            keys.append('split')
        if inb:
            keys += ['bias_in_kernel', 'reduce_vec' if aligned else 'reduce_scalar']
        return keys
    if sw['wgrad_tr']:
        return ['wgrad_tr_64' if sw['bn64'] and Cout % 128 == 64 else 'wgrad_tr_128']
    return ['wgrad_colpix']


def family_launches(N, H, W, Cin, Cout, sw=None):
    """The launches check_forward_family makes for one layer shape, in its order: name -> (predicted counters, fp32 output)."""
    e = expected_conv
    return {'forward': (e(N, H, W, Cin, Cout, 1, 0, sw), False),
            'forward, no epilogue': (e(N, H, W, Cin, Cout, 0, 0, sw), False),
            'forward + dropout': (e(N, H, W, Cin, Cout, 3, 1, sw), False),
            'data gradient': (e(N, H, W, Cout, Cin, 0, 0, sw, f32_out=True), True),
            'ReLU gate': (e(N, H, W, Cout, Cin, 2, 0, sw), False),
            'Philox gate': (e(N, H, W, Cout, Cin, 2, 1, sw), False),
            'dropped gate': (e(N, H, W, Cout, Cin, 2, 2, sw), False)}


def wgrad_launches(N, H, W, Cin, Cout, aligned, num_cu, scratch_room, sw=None):
    """The two kinds of call check_weight_gradient makes: name -> predicted counters."""
    return {'plain': expected_wgrad(N, H, W, Cin, Cout, False, aligned, num_cu, scratch_room, sw),
            'bias': expected_wgrad(N, H, W, Cin, Cout, True, aligned, num_cu, scratch_room, sw)}


# ---------------------------------------------------------------- the instantiations behind the counters
def conv_instantiation(keys, f32_out):
    """The template instantiation a forward / data-gradient launch with these counters ran.  The counters are marginals
    (pair, MAXV and ACT each on its own); one launch bumps one of each, so its keys name the instantiation:
    ('img', fp32 output, pair, MAXV, ACT, stream, w8) or ('tiled', fp32 output, tile width).  nbuf is a run-time argument."""
    if keys[0] == 'tiled':
        return ('tiled', f32_out, keys[2])
    return ('img', f32_out, keys[1], keys[2], keys[3], 'stream' in keys, 'w8' in keys)


def all_conv_instantiations():
    """Every instantiation conv3x3_launch can start (the ASR_CONV_DBG=1 cycle-counter builds of the ReLU forms apart):
    per channel pair two MAXV, each with the fp32 output and the five bf16 epilogues; the streamed 64 -> 64 ReLU / ReLU +
    dropout forms; the two eight-wave forms; conv_nt_kernel<Taps33> with either output type and tile width."""
    out = set()
    for (ci, co), maxvs in PAIRS.items():
        pair = 'pair_%d_%d' % (ci, co)
        for mv in maxvs:
            out.add(('img', True, pair, 'maxv_%d' % mv, 'act_0', False, False))
            for act in range(5):
                out.add(('img', False, pair, 'maxv_%d' % mv, 'act_%d' % act, False, False))
            if (ci, co) == (64, 64):
                out |= {('img', False, pair, 'maxv_%d' % mv, 'act_%d' % act, True, False) for act in (1, 3)}
        if ci == 64:
            out.add(('img', False, pair, 'maxv_2', 'act_3', False, True))
    return out | {('tiled', f32, bn) for f32 in (False, True) for bn in ('tiled_bn128', 'tiled_bn64')}


def wgrad_instantiations(keys):
    """The kernels one weight-gradient call with these counters ran: the main kernel (form, split, bias in kernel) and,
    with the bias in the kernel, the reduce kernel."""
    out = {(keys[0], 'split' in keys, 'bias_in_kernel' in keys)}
    return out | {(k,) for k in keys if k.startswith('reduce')}


def all_wgrad_instantiations():
    out = {(form, split, inb) for form in ('wgrad_img_64_small', 'wgrad_img_64_large') for split in (False, True)
           for inb in (False, True)}
    out |= {('wgrad_img_128', False, inb) for inb in (False, True)}
    return out | {('reduce_vec',), ('reduce_scalar',), ('wgrad_tr_128', False, False), ('wgrad_tr_64', False, False),
                  ('wgrad_colpix', False, False)}


# ---------------------------------------------------------------- checks
def _ops():
    from tensorflow_end2end_speech_recognition_amd import ops
    return ops


def device_limits():
    """(num_cu, scratch_room) of the main handle of device 0, from the library."""
    from tensorflow_end2end_speech_recognition_amd import _lib
    h = _lib.handle(0)
    return h.info()[0], int(h.lib.asr_scratch_bytes(h.h)) - XCH_BYTES


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:24]


class Tally(object):
    """Runs one group of launches between a reset and a read of the path counters and demands exactly the predicted
    counters -- every other key zero, so a launch that fell to another kernel fails here; sums what it saw."""

    def __init__(self):
        self.total = {}

    def run(self, expect_keys, fn, what):
        ops = _ops()
        ops.reset_conv_path_counts(0)
        res = fn()
        got = ops.conv_path_counts(0)
        want = dict.fromkeys(got, 0)
        for k in expect_keys:
            want[k] += 1
        assert got == want, '%s: counters %s, predicted %s' % (
            what, {k: v for k, v in got.items() if v}, {k: v for k, v in want.items() if v})
        for k, v in got.items():
            self.total[k] = self.total.get(k, 0) + v
        return res


def _conv_ref(x_nhwc, w_hwio64, bias=None):
    """fp64 SAME 3x3 convolution on the CPU: x [n,H,W,Cin], w [3,3,Cin,Cout] -> [n,H,W,Cout]."""
    y = torch.nn.functional.conv2d(x_nhwc.double().cpu().permute(0, 3, 1, 2), w_hwio64.permute(3, 2, 0, 1),
                                   None if bias is None else bias.double().cpu(), padding=1)
    return y.permute(0, 2, 3, 1)


def check_forward_family(tally, N, H, W, Cin, Cout, pick=None, sw=None, dev='cuda:0'):
    """Forward (ReLU and no epilogue), forward + dropout, data gradient (fp32) and the three gated data gradients of one
    layer shape.  pick: the images compared with the fp64 reference (None = all); the bitwise statements cover every image.
    Returns {'fused_drop': digest, 'separate_drop': digest}."""
    ops = _ops()
    tag = '%dx%dx%d -> %d, N = %d' % (H, W, Cin, Cout, N)
    plan = family_launches(N, H, W, Cin, Cout, sw)
    g = torch.Generator().manual_seed(1000 * H + 10 * W + Cin + Cout + N)
    x = torch.randn(N, H, W, Cin, generator=g).to(torch.bfloat16)
    w = torch.randn(3, 3, Cin, Cout, generator=g) * 0.05
    b = torch.randn(Cout, generator=g) * 0.1
    dy = torch.randn(N, H, W, Cout, generator=g).to(torch.bfloat16)
    below = torch.randn(N, H, W, Cin, generator=g).clamp_min(0).to(torch.bfloat16)
    xd, bd, dyd, belowd = x.to(dev), b.to(dev), dy.to(dev), below.to(dev)
    wf, wb = ops.conv3x3_prep_weights(w.to(dev))
    wq = wf.float().cpu().view(Cout, 3, 3, Cin).permute(1, 2, 3, 0).double()      # the bf16-rounded weights, HWIO
    sel = list(range(N)) if pick is None else sorted(set(pick))
    ref = _conv_ref(x[sel], wq, b)

    out = tally.run(plan['forward'][0], lambda: ops.conv3x3_fwd(xd, wf, bd, relu=True), tag + ' forward')
    ok, worst = within_bf16_ulp(out[sel], torch.relu(ref))
    print('%s forward: worst %.3f bf16 ulp' % (tag, worst))
    assert ok, (tag, 'forward', worst)

    lin = tally.run(plan['forward, no epilogue'][0], lambda: ops.conv3x3_fwd(xd, wf, bd, relu=False),
                    tag + ' forward, no epilogue')
    ok, worst = within_bf16_ulp(lin[sel], ref)
    print('%s forward, no epilogue: worst %.3f bf16 ulp' % (tag, worst))
    assert ok, (tag, 'forward, no epilogue', worst)

    want = ops.dropout_apply(out, *DROP)
    got = tally.run(plan['forward + dropout'][0], lambda: ops.conv3x3_fwd_drop(xd, wf, bd, DROP),
                    tag + ' forward + dropout')
    assert torch.equal(got, want), (tag, 'fused dropout differs from the separate pass')
    assert float(got.float().abs().sum()) > 0

    dx = tally.run(plan['data gradient'][0], lambda: ops.conv3x3_bwd_data(dyd, wb), tag + ' data gradient')
    ref = _conv_ref(dy[sel], wq.flip(0, 1).permute(0, 1, 3, 2))                 # flipped taps, swapped channels: the adjoint
    err, mag = float((dx[sel].cpu().double() - ref).abs().max()), float(ref.abs().max())
    print('%s data gradient: max error %.3e of max|ref| %.3e (%.2e)' % (tag, err, mag, err / mag))
    assert err <= 1e-5 * mag, (tag, 'data gradient', err, mag)

    dropped = ops.dropout_apply(belowd, *DROP)
    for name, act_t, kw in (('ReLU gate', belowd, dict(drop=None)), ('Philox gate', belowd, dict(drop=DROP)),
                            ('dropped gate', dropped, dict(drop=DROP, dropped=True))):
        refg = ops.relu_bwd(dx, belowd, drop=kw['drop'])
        gotg = tally.run(plan[name][0], lambda: ops.conv3x3_bwd_data_relu(dyd, wb, act_t, **kw), '%s %s' % (tag, name))
        assert torch.equal(gotg, refg), (tag, name)
        assert float(gotg.float().abs().sum()) > 0, (tag, name)
    return dict(fused_drop=digest(got), separate_drop=digest(want))


def check_weight_gradient(tally, N, H, W, Cin, Cout, offset_view=False, sw=None, dev='cuda:0'):
    """asr_conv3x3_bwd_weight (twice, then accumulating) and asr_conv3x3_bwd_weight_bias (twice) against an fp64 einsum
    over the padded input.  offset_view: dw starts one float into a larger buffer (not 16-byte aligned); the floats on
    either side of it must survive.  Returns {'dw': digest, 'dw_bias': digest}."""
    ops = _ops()
    num_cu, room = device_limits()
    tag = 'weight gradient %dx%dx%d -> %d, N = %d%s' % (H, W, Cin, Cout, N, ', offset dw' if offset_view else '')
    g = torch.Generator().manual_seed(77 * H + 7 * W + Cin + Cout + N)
    xd = torch.randn(N, H, W, Cin, generator=g).to(torch.bfloat16).to(dev)
    dyd = torch.randn(N, H, W, Cout, generator=g).to(torch.bfloat16).to(dev)
    xp = torch.nn.functional.pad(xd.double(), (0, 0, 1, 1, 1, 1))
    ref = torch.cat([torch.einsum('nhwc,nhwo->co', xp[:, ty:ty + H, tx:tx + W], dyd.double())
                     for ty in range(3) for tx in range(3)], 0)
    refb = dyd.double().sum(dim=(0, 1, 2))
    mag, magb = float(ref.abs().max()), float(refb.abs().max())
    M = 9 * Cin

    def fresh(fill):
        buf = torch.full((M * Cout + 8,), fill, device=dev)
        lo = 1 if offset_view else 4                          # torch allocations are 16-byte aligned (and far more)
        dw = buf[lo:lo + M * Cout].view(M, Cout)
        assert (dw.data_ptr() % 16 == 0) != offset_view
        return buf, lo, dw

    def guards_ok(buf, lo, fill):
        return float(buf[lo - 1]) == fill and float(buf[lo + M * Cout]) == fill

    plan = wgrad_launches(N, H, W, Cin, Cout, not offset_view, num_cu, room, sw)
    plain, withb = plan['plain'], plan['bias']
    buf, lo, dw = fresh(7.0)
    tally.run(plain, lambda: ops.conv3x3_bwd_weight(xd, dyd, dw), tag)
    err = float((dw.double() - ref).abs().max())
    print('%s: max error %.3e of max|ref| %.3e (%.2e)' % (tag, err, mag, err / mag))
    assert err <= 1e-5 * mag, (tag, err, mag)
    assert guards_ok(buf, lo, 7.0), (tag, 'wrote outside dw')
    buf2, lo2, dw2 = fresh(-3.0)
    tally.run(plain, lambda: ops.conv3x3_bwd_weight(xd, dyd, dw2), tag + ' (again)')
    assert torch.equal(dw, dw2), (tag, 'two calls differ')
    tally.run(plain, lambda: ops.conv3x3_bwd_weight(xd, dyd, dw2, accumulate=True), tag + ' (accumulate)')
    err2 = float((dw2.double() - 2 * ref).abs().max())
    assert err2 <= 1e-5 * 2 * mag, (tag, 'accumulate', err2, mag)
    assert guards_ok(buf2, lo2, -3.0), (tag, 'accumulate wrote outside dw')

    res = []
    for fill in (5.0, -9.0):
        bufb, lob, dwb = fresh(fill)
        db = torch.full((Cout,), fill, device=dev)
        tally.run(withb, lambda: ops.conv3x3_bwd_weight_bias(xd, dyd, dwb, db), tag + ' + bias')
        assert guards_ok(bufb, lob, fill), (tag, 'the bias form wrote outside dw')
        res.append((dwb, db))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), (tag, 'two bias calls differ')
    dwb, db = res[0]
    errw, errb = float((dwb.double() - ref).abs().max()), float((db.double() - refb).abs().max())
    print('%s + bias: dw %.2e, db max error %.3e of max|ref| %.3e (%.2e)' % (tag, errw / mag, errb, magb, errb / magb))
    assert errw <= 1e-5 * mag, (tag, 'bias form dw', errw, mag)
    assert errb <= 1e-5 * magb, (tag, 'db', errb, magb)
    assert torch.equal(dwb, dw), (tag, 'the weight gradient with the bias differs from the one without')
    return dict(dw=digest(dw), dw_bias=digest(dwb))


# ---------------------------------------------------------------- what the child-process worker runs
WORKER_FORWARD = [(67, 40, 11, 64, 64), (67, 20, 6, 64, 64), (67, 20, 6, 64, 128), (67, 20, 6, 128, 128)]
WORKER_WGRAD = WORKER_FORWARD + [(67, 20, 6, 64, 192)]
