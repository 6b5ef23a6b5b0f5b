"""GPU: the cnn_zhang kernels (asr_conv3x5_*, asr_maxpool3x1_*) against torch fp64 on the same bf16 operands, and the
cnn_zhang CTC model against what the reference's own code computes (tests/golden/cnn_zhang_v1.npz)."""
import numpy as np
import pytest
import torch

from _bf16_ulp import within_bf16_ulp as _within_bf16_ulp
from test_cnn_zhang_host import check_against_fixture, fixture_batch, fixture_model

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _ops():
    from tensorflow_end2end_speech_recognition_amd import ops
    return ops


def _conv_ref(x, w_hwio, bias=None, relu=False):
    """fp64 SAME 3x5 convolution on the CPU: x [N,H,W,Cin], w [3,5,Cin,Cout] -> [N,H,W,Cout]."""
    y = torch.nn.functional.conv2d(x.double().cpu().permute(0, 3, 1, 2), w_hwio.double().cpu().permute(3, 2, 0, 1),
                                   None if bias is None else bias.double().cpu(), padding=(1, 2))
    y = y.permute(0, 2, 3, 1)
    return torch.relu(y) if relu else y


def _operands(N, H, W, cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, W, cin, generator=g).to(torch.bfloat16)
    w = (torch.randn(3, 5, cin, cout, generator=g) * 0.05)
    b = torch.randn(cout, generator=g) * 0.1
    return x, w, b


SHAPES = [(128, 128), (128, 256), (256, 256)]


@pytest.mark.parametrize('cin,cout', SHAPES + [(128, 192)])        # 192: the 64-column tiles (Cout % 128 == 64)
@pytest.mark.parametrize('W', [1, 11, 22])
@pytest.mark.parametrize('N', [1, 37])
def test_conv3x5_fwd_and_data_gradient(cin, cout, W, N):
    ops = _ops()
    H = 14
    x, w, b = _operands(N, H, W, cin, cout, seed=cin + cout + W + N)
    wq = w.to(torch.bfloat16).float()                    # the kernels multiply the bf16-rounded weights
    wf, wb = ops.conv3x5_prep_weights(w.to(DEV))
    out = ops.conv3x5_fwd(x.to(DEV), wf, b.to(DEV), relu=True)
    ok, worst = _within_bf16_ulp(out, _conv_ref(x, wq, b, relu=True))
    assert ok, worst
    # data gradient: conv with the flipped taps / swapped channels = the adjoint of the forward
    dy = torch.randn(N, H, W, cout).to(torch.bfloat16)
    dx = ops.conv3x5_bwd_data(dy.to(DEV), wb).cpu().double()
    ref = _conv_ref(dy, wq.flip(0, 1).permute(0, 1, 3, 2))
    assert float((dx - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    # ... gated by the ReLU of the layer below (bf16 output)
    below = torch.randn(N, H, W, cin).to(torch.bfloat16)
    dpre = ops.conv3x5_bwd_data_relu(dy.to(DEV), wb, below.to(DEV))
    ok, worst = _within_bf16_ulp(dpre, ref * (below.double() > 0))
    assert ok, worst


@pytest.mark.parametrize('cin,cout', SHAPES)
def test_conv3x5_many_images(cin, cout):
    """Several thousand images in one launch: images checked at the start, middle and end of the grid."""
    ops = _ops()
    N, H, W = 3001, 14, 11
    x, w, b = _operands(N, H, W, cin, cout, seed=7)
    wq = w.to(torch.bfloat16).float()
    wf, wb = ops.conv3x5_prep_weights(w.to(DEV))
    out = ops.conv3x5_fwd(x.to(DEV), wf, b.to(DEV), relu=True).cpu()
    pick = [0, 1, 1500, 2999, 3000]
    ok, worst = _within_bf16_ulp(out[pick], _conv_ref(x[pick], wq, b, relu=True))
    assert ok, worst


@pytest.mark.parametrize('cin,cout', SHAPES)
def test_conv3x5_fused_dropout_equals_separate_pass(cin, cout):
    ops = _ops()
    N, H, W = 37, 14, 11
    x, w, b = _operands(N, H, W, cin, cout, seed=3)
    wf, wb = ops.conv3x5_prep_weights(w.to(DEV))
    drop = (0.8, 1234, 5 << 32)
    fused = ops.conv3x5_fwd_drop(x.to(DEV), wf, b.to(DEV), drop)
    sep = ops.dropout_apply(ops.conv3x5_fwd(x.to(DEV), wf, b.to(DEV), relu=True), *drop)
    assert torch.equal(fused, sep)
    # backward gate from the dropped tensor (use_drop 2) == the mask formed from (keep, seed, offset) over the undropped one
    undropped = ops.conv3x5_fwd(x.to(DEV), wf, b.to(DEV), relu=True)
    _, wb2 = ops.conv3x5_prep_weights((torch.randn(3, 5, cout, 128) * 0.05).to(DEV))     # a layer above: cout -> 128
    dy = torch.randn(N, H, W, 128).to(torch.bfloat16).to(DEV)
    g_dropped = ops.conv3x5_bwd_data_relu(dy, wb2, fused, drop=drop, dropped=True)
    g_mask = ops.conv3x5_bwd_data_relu(dy, wb2, undropped, drop=drop, dropped=False)
    assert torch.equal(g_dropped, g_mask)


@pytest.mark.parametrize('cin,cout', SHAPES)
@pytest.mark.parametrize('N,W', [(1, 1), (37, 11), (300, 22)])
def test_conv3x5_weight_gradient(cin, cout, N, W):
    ops = _ops()
    H = 14
    x, _, _ = _operands(N, H, W, cin, cout, seed=N + W)
    dy = torch.randn(N, H, W, cout).to(torch.bfloat16)
    xd, dyd = x.to(DEV), dy.to(DEV)
    dw = torch.empty(15 * cin, cout, device=DEV)
    db = torch.empty(cout, device=DEV)
    ops.conv3x5_bwd_weight_bias(xd, dyd, dw, db)
    xp = torch.nn.functional.pad(xd.double(), (0, 0, 2, 2, 1, 1))
    ref = torch.cat([torch.einsum('nhwc,nhwo->co', xp[:, ty:ty + H, tx:tx + W], dyd.double())
                     for ty in range(3) for tx in range(5)], 0)
    assert float((dw.double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    rb = dyd.double().sum(dim=(0, 1, 2))
    assert float((db.double() - rb).abs().max()) <= 1e-5 * float(rb.abs().max())
    dw2 = torch.empty_like(dw)
    db2 = torch.empty_like(db)
    ops.conv3x5_bwd_weight_bias(xd, dyd, dw2, db2)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


def test_conv3x5_weight_gradient_bitwise_many_images():
    ops = _ops()
    N, H, W, cin, cout = 3001, 14, 11, 256, 256
    x = torch.randn(N, H, W, cin, device=DEV).to(torch.bfloat16)
    dy = torch.randn(N, H, W, cout, device=DEV).to(torch.bfloat16)
    res = []
    for _ in range(2):
        dw = torch.empty(15 * cin, cout, device=DEV)
        db = torch.empty(cout, device=DEV)
        ops.conv3x5_bwd_weight_bias(x, dy, dw, db)
        res.append((dw, db))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


@pytest.mark.parametrize('F', [40, 41])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_maxpool3x1_forward_backward_with_ties(F, dtype):
    ops = _ops()
    g = torch.Generator().manual_seed(F)
    N, W, C = 5, 11, 128
    x = torch.randint(0, 3, (N, F, W, C), generator=g).to(dtype)          # exact ties everywhere
    out, arg = ops.maxpool3x1_fwd(x.to(DEV))
    Ho = (F + 2) // 3
    pt = (3 * Ho - F) // 2
    xp = torch.full((N, 3 * Ho, W, C), float('-inf'), dtype=torch.float64)
    xp[:, pt:pt + F] = x.double()
    win = xp.view(N, Ho, 3, W, C)
    best = win.max(2)[0]
    first = (win == best.unsqueeze(2)).double().argmax(2)                   # first maximal row of the window
    assert torch.equal(out.cpu().double(), best)
    assert torch.equal(arg.cpu().long(), first)
    d = torch.randn(N, Ho, W, C).to(dtype)
    din = ops.maxpool3x1_bwd(d.to(DEV), arg, F).cpu()
    full = torch.zeros(N, Ho, 3, W, C, dtype=dtype)
    full.scatter_(2, first.unsqueeze(2), d.unsqueeze(2))
    assert torch.equal(din, full.view(N, 3 * Ho, W, C)[:, pt:pt + F])
    drop = (0.7, 99, 3 << 32)
    o2, a2 = ops.maxpool3x1_fwd(x.to(DEV), drop=drop)
    assert torch.equal(o2, ops.dropout_apply(out, *drop)) and torch.equal(a2, arg)


# ---------------------------------------------------------------- the model
def _model(dtype, F=40, W=11, seed=0):
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    return CTC('cnn_zhang', 3 * F, 256, 10, 61, splice=11, num_stack=W // 11, parameter_init=0.03, dtype=dtype,
               device=DEV, seed=seed)                  # W = splice * num_stack (11 or 22, as the reference's test_ctc.py)


@pytest.mark.parametrize('case', ['cnn_zhang_F40_W11', 'cnn_zhang_F41_W11', 'cnn_zhang_F40_W22', 'cnn_zhang_F41_W22'])
def test_fp32_model_against_reference_fixture(case):
    """The reference's own code on the fp64 stand-in (tests/golden/cnn_zhang_v1.npz).  fp32 accumulation order flips the
    ReLU gate of the few pre-activations within an ulp of 0 among ~1e6 units per layer, which moves the gradients of the
    lowest layers by up to ~1e-3 relative L2 (measured 1.4e-3 at CNN1, F = 41, W = 22); the head holds 1e-4."""
    m = fixture_model(case, 'f32', DEV)
    check_against_fixture(m, case, 1e-5, 5e-3, head_tol=1e-4)
    assert set(m.encoder.conv_path.values()) == {'im2col'}


def test_bf16_model_against_reference_fixture_on_the_implicit_path():
    case = 'cnn_zhang_F40_W11'
    m = fixture_model(case, 'bf16', DEV)
    check_against_fixture(m, case, 2e-3, 0.6, head_tol=2e-2)
    path = m.encoder.conv_path
    assert path['CNN1/conv'] == 'im2col' and all(path['CNN%d/conv' % i] == 'implicit' for i in range(2, 11))


def test_implicit_path_at_cfg_c_geometry_and_bitwise_steps():
    """cfg C geometry (F = 40, splice 11, B = 16, dropout): the implicit kernels run, and two training steps from the
    same state are bitwise reproducible."""
    rng = np.random.RandomState(1)
    B, T = 16, 40
    sl = rng.randint(20, T + 1, size=B).astype(np.int32)
    x = rng.randn(B, T, 40 * 11 * 3).astype(np.float32)
    dense = rng.randint(0, 61, size=(B, 8)).astype(np.int64)
    res = []
    for _ in range(2):
        m = _model('bf16', seed=4)
        for _step in range(2):
            loss, _ = m.compute_loss(x, dense, sl, keep_prob=0.8)
            m.train(loss, 'adam', 1e-4)
        assert all(m.encoder.conv_path['CNN%d/conv' % i] == 'implicit' for i in range(2, 11))
        torch.cuda.synchronize()
        res.append((loss.item(), m.store.flat.clone(), m.store.grad.clone()))
    assert res[0][0] == res[1][0]
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
    assert np.isfinite(res[0][0])
    from tensorflow_end2end_speech_recognition_amd import ops
    assert ops.check_async_errors(0) == 0
