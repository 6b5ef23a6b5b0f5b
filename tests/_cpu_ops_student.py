"""TEST INFRASTRUCTURE ONLY: torch-CPU stand-ins for the student-CNN kernels (asr_conv3x4_*, asr_bn_*,
asr_softmax_xent_soft), layered over _cpu_ops_cnn.install, so that the host logic of models/ctc/student_ctc.py and
models/encoders/core/student_cnn.py runs in the `-m "not gpu"` suite.  Arithmetic in fp64, results in the kernels' output
dtypes (bf16 where the device rounds to bf16).  Kernel numerics are tested on the GPU (tests/test_gpu_student.py)."""
import torch

import _cpu_ops_cnn

F64 = torch.float64
_TD = {0: torch.float32, 1: torch.bfloat16}


def _td(dtype):
    return dtype if isinstance(dtype, torch.dtype) else _TD[int(dtype)]


def _conv34(x, w_oihw, bias=None):
    """SAME 3x4 convolution of NHWC x (TensorFlow's padding: rows 1 / 1, columns 1 before and 2 after), fp64."""
    xp = torch.nn.functional.pad(x.double().permute(0, 3, 1, 2), (1, 2, 1, 1))
    y = torch.nn.functional.conv2d(xp, w_oihw.double(), None if bias is None else bias.double())
    return y.permute(0, 2, 3, 1).contiguous()


def _conv3x4_prep_weights(w_hwio):
    _, _, Cin, Cout = w_hwio.shape
    wq = w_hwio.to(torch.bfloat16)
    wf = wq.permute(3, 0, 1, 2).reshape(Cout, 12 * Cin).contiguous()
    wb = wq.flip(0, 1).permute(2, 0, 1, 3).reshape(Cin, 12 * Cout).contiguous()
    return wf, wb


def _conv3x4_fwd(x, wt_fwd, bias, relu=True, out_dtype=1):
    Cout, Cin = wt_fwd.shape[0], x.shape[3]
    y = _conv34(x, wt_fwd.view(Cout, 3, 4, Cin).permute(0, 3, 1, 2), bias)
    return (torch.relu(y) if relu else y).to(_td(out_dtype))


def _conv3x4_bwd_data(dy, wt_bwd):
    """the flipped image is a 3x4 correlation padded 1 / 1 rows and 2 before / 1 after columns"""
    Cin, Cout = wt_bwd.shape[0], dy.shape[3]
    w = wt_bwd.view(Cin, 3, 4, Cout).permute(0, 3, 1, 2)
    xp = torch.nn.functional.pad(dy.double().permute(0, 3, 1, 2), (2, 1, 1, 1))
    y = torch.nn.functional.conv2d(xp, w.double())
    return y.permute(0, 2, 3, 1).float().contiguous()


def _conv3x4_bwd_weight_bias(x, dy, dw, dbias=None):
    N, H, W, Cin = x.shape
    xp = torch.nn.functional.pad(x.double(), (0, 0, 1, 2, 1, 1))
    rows = [torch.einsum('nhwc,nhwo->co', xp[:, ty:ty + H, tx:tx + W], dy.double())
            for ty in range(3) for tx in range(4)]
    dw.copy_(torch.cat(rows, 0).float().view(dw.shape))
    if dbias is not None:
        dbias.copy_(dy.double().sum(dim=(0, 1, 2)).float())
    return dw, dbias


def _bn_stats(x, eps, momentum, avg_mean=None, avg_var=None):
    Cc = x.shape[-1]
    y = x.double().reshape(-1, Cc)
    mean = y.mean(0)
    var = ((y - mean) ** 2).mean(0)
    out = torch.zeros((5, Cc), dtype=F64)
    out[0], out[1], out[2] = mean, var, 1.0 / torch.sqrt(var.float().double() + eps)
    if avg_mean is not None:
        out[3] = avg_mean.double() * momentum + mean * (1.0 - momentum)
        out[4] = avg_var.double() * momentum + var * (1.0 - momentum)
    return out.float()


def _bn_apply(x, mean, var, gamma, beta, eps, pool, out_dtype):
    inv = torch.rsqrt(var.double() + eps) * gamma.double()
    y = x.double() * inv + (beta.double() - mean.double() * inv)
    if pool:
        out, arg = _cpu_ops_cnn._maxpool3x1_fwd(y)
        return out.to(_td(out_dtype)), arg
    return y.to(_td(out_dtype)), None


def _bn_bwd(dz, arg, x, stats, gamma, dgamma, dbeta, out_dtype, relu_gate=True):
    N, H, W, Cc = x.shape
    dy = _cpu_ops_cnn._maxpool3x1_bwd(dz.double(), arg, H) if arg is not None else dz.double().view(x.shape)
    mean, rstd = stats[0].double(), stats[2].double()
    xh = (x.double() - mean) * rstd
    M = N * H * W
    sdy = dy.reshape(-1, Cc).sum(0)
    sdyx = (dy * xh).reshape(-1, Cc).sum(0)
    dbeta.copy_(sdy.float())
    dgamma.copy_(sdyx.float())
    dx = gamma.double() * rstd * (dy - sdy / M - xh * sdyx / M)
    if relu_gate:
        dx = dx * (x > 0).double()
    return dx.to(_td(out_dtype)).contiguous()


def _softmax_xent_soft(logits, targets, grad_scale=1.0, want_grad=True):
    z, p = logits.double(), targets.double()
    ls = torch.log_softmax(z, dim=1)
    loss = -(p * ls).sum(1)
    dl = ((ls.exp() - p) * grad_scale).float() if want_grad else None
    return loss.float(), dl


STAND_INS = dict(
    conv3x4_prep_weights=_conv3x4_prep_weights, conv3x4_fwd=_conv3x4_fwd, conv3x4_bwd_data=_conv3x4_bwd_data,
    conv3x4_bwd_weight_bias=_conv3x4_bwd_weight_bias, bn_stats=_bn_stats, bn_apply=_bn_apply, bn_bwd=_bn_bwd,
    softmax_xent_soft=_softmax_xent_soft,
)


def install(monkeypatch):
    ops = _cpu_ops_cnn.install(monkeypatch)
    for name, fn in STAND_INS.items():
        assert hasattr(ops, name), name
        monkeypatch.setattr(ops, name, fn)
    return ops
