"""TEST INFRASTRUCTURE ONLY: torch-CPU stand-ins for the cnn_zhang kernels (asr_conv3x5_*, asr_maxpool3x1_*), layered
over _cpu_ops.install, so that the host logic of models/encoders/core/cnn_zhang.py runs in the `-m "not gpu"` suite.
Values are rounded where the device rounds (bf16 stored activations and pre-activation gradients); products
accumulate in fp64.  Kernel numerics are tested on the GPU (tests/test_gpu_cnn_zhang.py)."""
import torch

import _cpu_ops


def _bf(t):
    return t.to(torch.bfloat16)


def _conv35(x, w_oihw, bias=None):
    """SAME 3x5 convolution of NHWC x with OIHW weights, fp64 -> NHWC fp64."""
    y = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), w_oihw.double(),
                                   None if bias is None else bias.double(), padding=(1, 2))
    return y.permute(0, 2, 3, 1).contiguous()


def _conv3x5_prep_weights(w_hwio):
    _, _, Cin, Cout = w_hwio.shape
    wq = w_hwio.to(torch.bfloat16)          # the images are bf16 whatever the activations' rounding
    wf = wq.permute(3, 0, 1, 2).reshape(Cout, 15 * Cin).contiguous()
    wb = wq.flip(0, 1).permute(2, 0, 1, 3).reshape(Cin, 15 * Cout).contiguous()
    return wf, wb


def _conv3x5_fwd(x, wt_fwd, bias, relu=True, out=None):
    Cout, Cin = wt_fwd.shape[0], x.shape[3]
    y = _conv35(x, wt_fwd.view(Cout, 3, 5, Cin).permute(0, 3, 1, 2), bias)
    return _bf(torch.relu(y) if relu else y)


def _conv3x5_fwd_drop(x, wt_fwd, bias, drop, out=None):
    return _bf(_cpu_ops._dropout_apply(_conv3x5_fwd(x, wt_fwd, bias, True).float(), *drop))


def _conv3x5_bwd_data(dy, wt_bwd):
    Cin, Cout = wt_bwd.shape[0], dy.shape[3]
    return _conv35(dy, wt_bwd.view(Cin, 3, 5, Cout).permute(0, 3, 1, 2)).float()   # the image holds the flipped taps


def _conv3x5_bwd_data_relu(dy, wt_bwd, act_below, drop=None, dropped=False):
    dx = _conv3x5_bwd_data(dy, wt_bwd)
    if drop is None:
        return _bf(dx * (act_below > 0))
    if dropped:
        return _bf(dx * (act_below > 0) * (1.0 / drop[0]))
    return _bf(_cpu_ops._relu_bwd(dx, act_below, drop=drop))


def _conv3x5_bwd_weight_bias(x, dy, dw, dbias=None):
    N, H, W, Cin = x.shape
    xp = torch.nn.functional.pad(x.double(), (0, 0, 2, 2, 1, 1))
    rows = [torch.einsum('nhwc,nhwo->co', xp[:, ty:ty + H, tx:tx + W], dy.double())
            for ty in range(3) for tx in range(5)]
    dw.copy_(torch.cat(rows, 0).float().view(dw.shape))
    if dbias is not None:
        dbias.copy_(dy.double().sum(dim=(0, 1, 2)).float())
    return dw, dbias


def _maxpool3x1_fwd(x, drop=None):
    N, H, W, Cc = x.shape
    Ho = (H + 2) // 3
    pt = (3 * Ho - H) // 2
    xp = torch.full((N, 3 * Ho, W, Cc), float('-inf'), dtype=x.dtype)
    xp[:, pt:pt + H] = x
    win = xp.view(N, Ho, 3, W, Cc)
    out = win.max(dim=2)[0].contiguous()
    arg = (win == out.unsqueeze(2)).to(torch.uint8).argmax(dim=2)     # the first of equal values, as the kernel
    if drop is not None:
        out = _cpu_ops._dropout_apply(out.float(), *drop).to(x.dtype)
    return out, arg.to(torch.uint8).contiguous()


def _maxpool3x1_bwd(dout, arg, H):
    N, Ho, W, Cc = dout.shape
    pt = (3 * Ho - H) // 2
    g = torch.zeros((N, Ho, 3, W, Cc), dtype=dout.dtype)
    g.scatter_(2, arg.long().unsqueeze(2), dout.unsqueeze(2))
    return g.view(N, 3 * Ho, W, Cc)[:, pt:pt + H].contiguous()


STAND_INS = dict(
    conv3x5_prep_weights=_conv3x5_prep_weights, conv3x5_fwd=_conv3x5_fwd, conv3x5_fwd_drop=_conv3x5_fwd_drop,
    conv3x5_bwd_data=_conv3x5_bwd_data, conv3x5_bwd_data_relu=_conv3x5_bwd_data_relu,
    conv3x5_bwd_weight_bias=_conv3x5_bwd_weight_bias, maxpool3x1_fwd=_maxpool3x1_fwd, maxpool3x1_bwd=_maxpool3x1_bwd,
)


def install(monkeypatch):
    ops = _cpu_ops.install(monkeypatch)
    for name, fn in STAND_INS.items():
        assert hasattr(ops, name), name
        monkeypatch.setattr(ops, name, fn)
    return ops
