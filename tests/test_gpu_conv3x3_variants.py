"""GPU: every kernel instantiation that csrc/conv3x3.hip dispatches, each asserted through the host path counters
(ops.conv_path_counts) and checked against fp64 references at the smallest shape that reaches it.

The dispatch rule is restated in tests/_conv_variants.py (expected_conv / expected_wgrad); every launch of every case
resets the counters, runs, and demands exactly the counters the rule predicts, so a shape that silently falls to another
kernel fails.  The CU count and the scratch size come from the library.  The counters are marginals (pair, MAXV and ACT
each on its own), but one launch bumps one of each, so the counters of a single launch name its instantiation:
test_the_cases_of_this_file_reach_every_instantiation holds the cases below against the full list of instantiations.

What each shape is for (image-resident forward / data gradient, conv3x3_img_kernel; staged vectors mv = ceil(H W Cin / 2048)):
  64 ch 45 x 11   mv 16 -> MAXV 16; 87 984 bytes with the border: one LDS buffer; 495 pixels leave a 15-pixel tail tile
  64 ch 41 x 11   mv 15 -> MAXV 16, two buffers, STREAM for 64 -> 64 ReLU / ReLU + dropout
  64 ch 1 x 300   mv 10 -> MAXV 14 (64 -> 64) / 16 (64 -> 128), one buffer, every pixel on the top and bottom border
  128 ch 20 x 12  mv 15 -> MAXV 16, one buffer;  128 ch 16 x 13  mv 13 -> MAXV 16, two buffers; both also as the data
                  gradient of a 64 -> 128 layer (the 128 -> 64 product with the fp32 output and the gated epilogues) and, for
                  128 -> 64 layers, with a 64 -> 128 product at MAXV 16 as the data gradient
  20 x 6 128 -> 64  the MAXV 8 forward of that pair and the MAXV 4 data gradient of 64 -> 128
  N = num_cu + 37 at the one-buffer images: a workgroup multiplies a second image out of the buffer it staged the first in
  128 ch 40 x 11  7040 vectors: too big for the image form at an image-resident channel pair -> tiled at N >= 64
  64 -> 192 / 256 the tiled forward with 64- and 128-column tiles, the data gradient with 192 / 256 input channels
Weight gradient: 3 and 4 column groups (Cout 192 / 256), the 128-channel form, mv 16 -> the tiled fallback at N >= 64,
channels that are multiples of 8 only, dw off a 16-byte boundary (wgrad_img_reduce_kernel<0>).
The kernels behind the ASR_CONV_* switches run in fresh child processes (test_switched_kernels_in_a_fresh_process)."""
import json
import os
import subprocess
import sys

import pytest

from _conv_variants import (WORKER_FORWARD, WORKER_WGRAD, XCH_BYTES, Tally, all_conv_instantiations,
                            all_wgrad_instantiations, check_forward_family, check_weight_gradient, conv_instantiation,
                            device_limits, expected_conv, expected_wgrad, family_launches, switches, wgrad_instantiations,
                            wgrad_launches, xch_bytes_of_the_library)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N0 = 64 + 3

# (H, W, Cin, Couts, one LDS buffer)
IMAGES = [(45, 11, 64, (64, 128), True), (41, 11, 64, (64, 128), False), (1, 300, 64, (64, 128), True),
          (20, 12, 128, (128, 64), True), (16, 13, 128, (128, 64), False)]
LAYERS = [(H, W, Cin, Cout) for H, W, Cin, couts, _ in IMAGES for Cout in couts]
# 64 -> 128 at the 128-channel images: the data gradient is the 128 -> 64 product at mv 15 (one buffer) / 13 (two), the
# only way to its fp32, ACT 2 and ACT 4 forms at MAXV 16 (at the 64-channel images above that product exceeds 4096 vectors
# and is tiled); 128 -> 64 at 20 x 6: that pair's MAXV 8 forward, and the 64 -> 128 product at MAXV 4 as a data gradient
LAYERS += [(20, 12, 64, 128), (16, 13, 64, 128), (20, 6, 128, 64)]
ONE_BUFFER = [(H, W, Cin, Cout) for H, W, Cin, couts, one in IMAGES if one for Cout in couts]
TILED = [(40, 11, 128, 128), (20, 6, 64, 192), (20, 6, 64, 256)]


def _ops():
    from tensorflow_end2end_speech_recognition_amd import ops
    return ops


# ---------------------------------------------------------------- the rule itself, at the shapes this file relies on
def test_dispatch_rule_at_the_shapes_of_this_file(cuda):
    num_cu, room = device_limits()
    assert XCH_BYTES == xch_bytes_of_the_library()          # the arena split expected_wgrad's scratch_room is taken from
    e = expected_conv
    assert e(N0, 45, 11, 64, 64, 1, 0) == ['img', 'pair_64_64', 'maxv_16', 'act_1', 'nbuf_1']
    assert e(N0, 41, 11, 64, 64, 1, 0) == ['img', 'pair_64_64', 'maxv_16', 'act_1', 'nbuf_2', 'stream']
    assert e(N0, 41, 11, 64, 64, 3, 1) == ['img', 'pair_64_64', 'maxv_16', 'act_3', 'nbuf_2', 'stream']
    assert e(N0, 41, 11, 64, 128, 1, 0) == ['img', 'pair_64_128', 'maxv_16', 'act_1', 'nbuf_2']
    assert e(N0, 1, 300, 64, 64, 2, 1) == ['img', 'pair_64_64', 'maxv_14', 'act_4', 'nbuf_1']
    assert e(N0, 1, 300, 64, 128, 1, 0) == ['img', 'pair_64_128', 'maxv_16', 'act_1', 'nbuf_1']
    assert e(N0, 20, 12, 128, 128, 2, 2) == ['img', 'pair_128_128', 'maxv_16', 'act_2', 'nbuf_1']
    assert e(N0, 16, 13, 128, 64, 0, 0, f32_out=True) == ['img', 'pair_128_64', 'maxv_16', 'act_0', 'nbuf_2']
    # the data gradients of 64 -> 128 layers: 128 -> 64 products
    assert e(N0, 16, 13, 128, 64, 2, 0) == ['img', 'pair_128_64', 'maxv_16', 'act_2', 'nbuf_2']
    assert e(N0, 20, 12, 128, 64, 2, 1) == ['img', 'pair_128_64', 'maxv_16', 'act_4', 'nbuf_1']
    assert e(N0, 16, 13, 64, 128, 1, 0) == ['img', 'pair_64_128', 'maxv_16', 'act_1', 'nbuf_2']
    assert e(N0, 45, 11, 128, 64, 0, 0, f32_out=True) == ['tiled', 'pair_128_64', 'tiled_bn64']      # 7920 vectors
    assert e(N0, 20, 6, 128, 64, 1, 0) == ['img', 'pair_128_64', 'maxv_8', 'act_1', 'nbuf_2']
    assert e(N0, 20, 6, 64, 128, 2, 2) == ['img', 'pair_64_128', 'maxv_4', 'act_2', 'nbuf_2']
    assert e(N0, 20, 6, 64, 128, 3, 1) == ['img', 'pair_64_128', 'maxv_2', 'act_3', 'nbuf_2', 'w8']
    assert e(N0, 40, 11, 128, 128, 1, 0) == ['tiled', 'pair_128_128', 'tiled_bn128']
    assert e(63, 20, 6, 64, 64, 1, 0) == ['tiled', 'pair_64_64', 'tiled_bn64']
    assert e(N0, 20, 6, 64, 192, 1, 0) == ['tiled', 'pair_other', 'tiled_bn64']
    assert e(N0, 20, 6, 256, 64, 0, 0, f32_out=True) == ['tiled', 'pair_other', 'tiled_bn64']
    g = lambda *a: expected_wgrad(*a, num_cu, room)                                      # noqa: E731
    assert g(N0, 20, 6, 64, 192, True, True) == ['wgrad_img_64_small', 'split', 'bias_in_kernel', 'reduce_vec']
    assert g(N0, 20, 6, 64, 128, True, False) == ['wgrad_img_64_small', 'split', 'bias_in_kernel', 'reduce_scalar']
    assert g(N0, 40, 11, 64, 64, False, True) == ['wgrad_img_64_large', 'split']
    assert g(N0, 20, 6, 128, 128, False, True) == ['wgrad_img_128']
    assert g(N0, 45, 11, 64, 64, True, True) == ['wgrad_tr_128']
    assert g(5, 7, 5, 8, 24, True, True) == ['wgrad_tr_128']
    off = switches({'ASR_CONV_WGRAD_IMG': '0', 'ASR_CONV_WGRAD_TR': '0', 'ASR_CONV_WGRAD_BN64': '1'})
    assert expected_wgrad(N0, 20, 6, 64, 192, True, True, num_cu, room, off) == ['wgrad_colpix']


# ---------------------------------------------------------------- image-resident forward / data gradient
@pytest.mark.parametrize('H,W,Cin,Cout', LAYERS)
def test_image_resident_variants(cuda, H, W, Cin, Cout):
    """Every launch is held to the counters family_launches predicts (Tally.run) and to its reference."""
    check_forward_family(Tally(), N0, H, W, Cin, Cout)


@pytest.mark.parametrize('H,W,Cin,Cout', ONE_BUFFER)
def test_one_buffer_workgroup_walks_two_images(cuda, H, W, Cin, Cout):
    """More images than CUs on the single-buffer path: a workgroup must finish multiplying image i before it stores image
    i + num_cu over it.  fp64 comparison on the images around the wrap; the bitwise statements cover all of them."""
    num_cu, _ = device_limits()
    N = num_cu + 37
    assert any('nbuf_1' in keys for keys, _ in family_launches(N, H, W, Cin, Cout).values())
    check_forward_family(Tally(), N, H, W, Cin, Cout, pick=[0, 1, num_cu - 1, num_cu, num_cu + 1, N - 1])


@pytest.mark.parametrize('H,W,Cin,Cout', TILED)
def test_tiled_kernel_on_the_3x3_geometry(cuda, H, W, Cin, Cout):
    """conv_nt_kernel<Taps33> at N >= 64: an image-resident channel pair whose image is too big for LDS (7040 vectors), and
    64- / 128-column tiles at 192 / 256 output channels (the data gradients: 192 / 256 input channels, 64-column tiles)."""
    assert all(keys[0] == 'tiled' for keys, _ in family_launches(N0, H, W, Cin, Cout).values())
    check_forward_family(Tally(), N0, H, W, Cin, Cout)


# ---------------------------------------------------------------- weight gradient
WGRADS = [(N0, 20, 6, 64, 192, 'wgrad_img_64_small'), (N0, 20, 6, 64, 256, 'wgrad_img_64_small'),
          (N0, 40, 11, 64, 64, 'wgrad_img_64_large'), (N0, 45, 11, 64, 64, 'wgrad_tr_128'),
          (N0, 20, 6, 128, 128, 'wgrad_img_128'), (5, 7, 5, 8, 24, 'wgrad_tr_128'), (3, 9, 4, 72, 40, 'wgrad_tr_128')]
WGRAD_UNALIGNED = (N0, 20, 6, 64, 128)


@pytest.mark.parametrize('N,H,W,Cin,Cout,form', WGRADS)
def test_weight_gradient_variants(cuda, N, H, W, Cin, Cout, form):
    tally = Tally()
    check_weight_gradient(tally, N, H, W, Cin, Cout)
    assert tally.total[form] == 5
    img = form.startswith('wgrad_img')
    assert tally.total['bias_in_kernel'] == tally.total['reduce_vec'] == (2 if img else 0)
    assert tally.total['reduce_scalar'] == 0


def test_weight_gradient_into_an_unaligned_view(cuda):
    tally = Tally()
    check_weight_gradient(tally, *WGRAD_UNALIGNED, offset_view=True)
    assert tally.total['wgrad_img_64_small'] == 5 and tally.total['reduce_scalar'] == 2 and tally.total['reduce_vec'] == 0


# ---------------------------------------------------------------- the switches, each in a fresh child process
_CHILD_FAULT = []            # set by the first child that ends on a signal, a fault or the time limit: nothing more is started

# switches -> what the counters of the worker's fixed case list must then show
SWITCH_CASES = {
    'IMG=0': dict(env={'ASR_CONV_IMG': '0'}, zero=['img', 'stream', 'w8', 'nbuf_1', 'nbuf_2'],
                  nonzero=['tiled', 'tiled_bn128', 'tiled_bn64']),
    'STREAM=0': dict(env={'ASR_CONV_STREAM': '0'}, zero=['stream', 'tiled'], nonzero=['img', 'maxv_14', 'w8']),
    'IMG_W8=0': dict(env={'ASR_CONV_IMG_W8': '0'}, zero=['w8', 'maxv_2', 'tiled'], nonzero=['act_3', 'maxv_4', 'stream']),
    'WGRAD_IMG=0': dict(env={'ASR_CONV_WGRAD_IMG': '0'},
                        zero=['wgrad_img_64_small', 'wgrad_img_64_large', 'wgrad_img_128', 'split', 'bias_in_kernel',
                              'reduce_vec', 'wgrad_tr_64', 'wgrad_colpix'], nonzero=['wgrad_tr_128']),
    'WGRAD_IMG=0,WGRAD_TR=0': dict(env={'ASR_CONV_WGRAD_IMG': '0', 'ASR_CONV_WGRAD_TR': '0'},
                                   zero=['wgrad_img_64_small', 'wgrad_img_64_large', 'wgrad_img_128', 'wgrad_tr_128',
                                         'wgrad_tr_64'], nonzero=['wgrad_colpix']),
    'WGRAD_IMG=0,WGRAD_BN64=1': dict(env={'ASR_CONV_WGRAD_IMG': '0', 'ASR_CONV_WGRAD_BN64': '1'},
                                     zero=['wgrad_img_64_small', 'wgrad_img_64_large', 'wgrad_img_128', 'wgrad_colpix'],
                                     nonzero=['wgrad_tr_64', 'wgrad_tr_128']),
    'WGRAD_BIAS=0': dict(env={'ASR_CONV_WGRAD_BIAS': '0'}, zero=['bias_in_kernel', 'reduce_vec', 'reduce_scalar'],
                         nonzero=['wgrad_img_64_small', 'wgrad_img_64_large', 'wgrad_img_128', 'split']),
    'WGRAD_SPLIT=0': dict(env={'ASR_CONV_WGRAD_SPLIT': '0'}, zero=['split'],
                          nonzero=['wgrad_img_64_small', 'wgrad_img_64_large', 'wgrad_img_128', 'bias_in_kernel']),
}
_SWITCH_NAMES = ('ASR_CONV_IMG', 'ASR_CONV_STREAM', 'ASR_CONV_IMG_W8', 'ASR_CONV_WGRAD_IMG', 'ASR_CONV_WGRAD_TR',
                 'ASR_CONV_WGRAD_BN64', 'ASR_CONV_WGRAD_BIAS', 'ASR_CONV_WGRAD_SPLIT', 'ASR_CONV_DBG')


@pytest.mark.parametrize('case', sorted(SWITCH_CASES))
def test_switched_kernels_in_a_fresh_process(cuda, case):
    """tests/_conv_variant_worker.py with the switches of `case`: the worker checks its shapes against the fp64 references
    with the bounds of this file and asserts the counters of every launch against the rule under those switches; here, that
    the switched kernel is the one that ran and that what the default build states as bit-identical stays so."""
    if _CHILD_FAULT:
        pytest.fail('not started: the child of %s ended on a fault or the time limit' % _CHILD_FAULT[0])
    spec = SWITCH_CASES[case]
    env = {k: v for k, v in os.environ.items() if k not in _SWITCH_NAMES}
    env.update(spec['env'], PYTHONPATH=ROOT)
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_conv_variant_worker.py')], env=env,
                           capture_output=True, text=True, timeout=240)
    except subprocess.TimeoutExpired as e:
        _CHILD_FAULT.append(case)
        pytest.fail('%s: the child did not finish in %d s\n%s' % (case, e.timeout, str(e.stderr)[-2000:]))
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or 'illegal memory access' in r.stderr \
            or 'HSA_STATUS_ERROR' in r.stderr:
        _CHILD_FAULT.append(case)
    assert r.returncode == 0, (case, r.returncode, r.stdout[-3000:], r.stderr[-4000:])
    line = [l for l in r.stdout.splitlines() if l.startswith('CONV ')][-1]
    res = json.loads(line[len('CONV '):])
    counts = res['counts']
    for k in spec['zero']:
        assert counts[k] == 0, (case, k, counts)
    for k in spec['nonzero']:
        assert counts[k] > 0, (case, k, counts)
    for name, d in res['digests'].items():
        if name.startswith('wgrad'):
            assert d['dw'] == d['dw_bias'], (case, name)
        else:
            assert d['fused_drop'] == d['separate_drop'], (case, name)


# ---------------------------------------------------------------- coverage of the instantiations
def test_the_cases_of_this_file_reach_every_instantiation(cuda):
    """The counters are marginals: pair_128_64, maxv_16 and act_4 can each turn non-zero from a different launch.  A single
    launch bumps one of each, and every launch of the cases above is asserted against family_launches / wgrad_launches, so
    the instantiations this file runs are the ones those predict for its case lists: in this process with the default
    switches, in the children with the switches of SWITCH_CASES.  They must be all there are."""
    num_cu, room = device_limits()
    conv, wgrad = set(), set()

    def collect(forward, weight, sw):
        for N, H, W, Cin, Cout in forward:
            conv.update(conv_instantiation(keys, f32) for keys, f32 in family_launches(N, H, W, Cin, Cout, sw).values())
        for N, H, W, Cin, Cout, aligned in weight:
            for keys in wgrad_launches(N, H, W, Cin, Cout, aligned, num_cu, room, sw).values():
                wgrad.update(wgrad_instantiations(keys))

    collect([(N0,) + c for c in LAYERS + TILED] + [(num_cu + 37,) + c for c in ONE_BUFFER],
            [c[:5] + (True,) for c in WGRADS] + [WGRAD_UNALIGNED + (False,)], switches({}))
    # (the children with a weight-gradient switch run the forward kernels by the default rule, and the other way round)
    collect(WORKER_FORWARD, [c + (True,) for c in WORKER_WGRAD], switches({}))
    by_default = set(conv), set(wgrad)
    for spec in SWITCH_CASES.values():
        collect(WORKER_FORWARD, [c + (True,) for c in WORKER_WGRAD], switches(spec['env']))
    assert conv == all_conv_instantiations(), (sorted(all_conv_instantiations() - conv), sorted(conv - all_conv_instantiations()))
    assert wgrad == all_wgrad_instantiations(), sorted(all_wgrad_instantiations() ^ wgrad)
    # what only a flipped switch reaches: the four-wave ReLU + dropout of small 64-channel images (ASR_CONV_IMG_W8=0), the
    # one-group weight-gradient forms (ASR_CONV_WGRAD_SPLIT=0) and the two tiled weight-gradient kernels behind switches
    assert sorted(all_conv_instantiations() - by_default[0]) == [
        ('img', False, 'pair_64_128', 'maxv_4', 'act_3', False, False)]
    assert sorted(all_wgrad_instantiations() - by_default[1]) == sorted(
        [(f, False, b) for f in ('wgrad_img_64_small', 'wgrad_img_64_large') for b in (False, True)]
        + [('wgrad_tr_64', False, False), ('wgrad_colpix', False, False)])


# ---------------------------------------------------------------- coverage of the enum
# keys no in-process launch can reach, and the child case that asserts each
SWITCH_ONLY = {'wgrad_tr_64': 'WGRAD_IMG=0,WGRAD_BN64=1', 'wgrad_colpix': 'WGRAD_IMG=0,WGRAD_TR=0'}


def test_every_counter_is_reached(cuda):
    """One minimal launch per variant in this process: no key of the enum but the two behind a switch stays zero (those two
    are asserted non-zero by the child cases named in SWITCH_ONLY)."""
    import torch
    ops = _ops()
    assert all(k in SWITCH_CASES and k2 in SWITCH_CASES[k]['nonzero'] for k2, k in SWITCH_ONLY.items())
    if any(not v for k, v in switches().items() if k != 'bn64') or switches()['bn64']:
        pytest.fail('an ASR_CONV_* switch is set in the environment of the test run')
    dev = 'cuda:0'
    ops.reset_conv_path_counts(0)
    N = 64

    def layer(H, W, Cin, Cout, gates=(None,)):
        x = torch.randn(N, H, W, Cin).to(torch.bfloat16).to(dev)
        wf, wb = ops.conv3x3_prep_weights((torch.randn(3, 3, Cin, Cout) * 0.05).to(dev))
        b = torch.zeros(Cout, device=dev)
        ops.conv3x3_fwd(x, wf, b, relu=True)
        ops.conv3x3_fwd(x, wf, b, relu=False)
        ops.conv3x3_fwd_drop(x, wf, b, DROP)
        dy = torch.randn(N, H, W, Cout).to(torch.bfloat16).to(dev)
        ops.conv3x3_bwd_data(dy, wb)
        ops.conv3x3_bwd_data_relu(dy, wb, x)
        ops.conv3x3_bwd_data_relu(dy, wb, x, drop=DROP)
        return x, dy

    DROP = (0.9, 3, 1 << 32)
    layer(45, 11, 64, 64)                                 # maxv_16, nbuf_1, act 0 - 4
    layer(40, 11, 64, 64)                                 # maxv_14, stream
    layer(20, 6, 64, 128)                                 # maxv_4, maxv_2 + w8; the data gradient: 128 -> 64, maxv_8
    layer(20, 6, 128, 128)
    x, dy = layer(20, 6, 64, 192)                         # tiled, 64-column tiles, pair_other
    layer(4, 4, 128, 256)                                 # tiled, 128-column tiles

    def wgrad(x, dy, unaligned=False):
        M, Cout = 9 * x.shape[3], dy.shape[3]
        buf = torch.zeros(M * Cout + 8, device=dev)
        lo = 1 if unaligned else 4
        dw = buf[lo:lo + M * Cout].view(M, Cout)
        ops.conv3x3_bwd_weight_bias(x, dy, dw, torch.zeros(Cout, device=dev))

    wgrad(x, dy)                                          # wgrad_img_64_small, split, bias_in_kernel, reduce_vec
    wgrad(x, dy, unaligned=True)                          # reduce_scalar
    r = lambda *s: torch.randn(*s).to(torch.bfloat16).to(dev)                           # noqa: E731
    wgrad(r(N, 40, 11, 64), r(N, 40, 11, 64))             # wgrad_img_64_large
    wgrad(r(N, 20, 6, 128), r(N, 20, 6, 128))             # wgrad_img_128
    wgrad(r(2, 5, 3, 8), r(2, 5, 3, 16))                  # wgrad_tr_128
    torch.cuda.synchronize()
    counts = ops.conv_path_counts(0)
    assert sorted(k for k, v in counts.items() if v == 0) == sorted(SWITCH_ONLY), counts
