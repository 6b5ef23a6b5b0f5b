"""Host code shared by the convolution-only encoders (cnn_zhang.py, student_cnn.py): variable declaration as in the
reference's models/encoders/core/cnn_util.py:66-69, the asr_im2col + GEMM convolution (the fp32 parity path and the
3-channel first layers), the fully connected stack, and the gather back to the time-major padded grid.

Every kernel wrapper is looked up as ops.<name> when it is called.  Nothing here knows which encoder calls it: the
filter size, the weight / bias / gradient views and the dropout descriptors are arguments.
"""
import numpy as np
import torch

from .... import ops
from ...._lib import ASR_F32

PATCH_BYTES = 1 << 30        # im2col chunks: the patch matrix of one chunk stays under 1 GiB


def _trunc_normal(rng, std, shape):
    x = rng.normal(0.0, std, size=shape)
    bad = np.abs(x) > 2 * std
    while bad.any():
        x[bad] = rng.normal(0.0, std, size=int(bad.sum()))
        bad = np.abs(x) > 2 * std
    return x


# ---------------------------------------------------------------------- variables
def declare_conv(store, name, kh, kw, cin, cout, rng, std):
    """name/{weight,bias}: tf.Variable(truncated_normal(stddev=parameter_init)) and zeros (cnn_util.py:66-69)."""
    store.declare(name + '/weight', (kh, kw, cin, cout), _trunc_normal(rng, std, (kh, kw, cin, cout)))
    store.declare(name + '/bias', (cout,), np.zeros(cout))


def declare_fc(store, name, din, dout, rng, std):
    """name/{weights,biases} of one fully connected layer."""
    store.declare(name + '/weights', (din, dout), _trunc_normal(rng, std, (din, dout)))
    store.declare(name + '/biases', (dout,), np.zeros(dout))


# ---------------------------------------------------------------------- convolution through asr_im2col + GEMM
def _chunk(pix, cols, elem):
    """images per im2col chunk"""
    return max(1, PATCH_BYTES // (pix * cols * elem))


def conv_im2col(x, kh, kw, w2d, b, out_dtype):
    """relu(conv kh x kw SAME(x) + b) through asr_im2col + GEMM, chunked over images: x [N,H,W,Cin], w2d the
    [kh*kw*Cin, Cout] view of the HWIO weight in the operand dtype -> [N,H,W,Cout] in out_dtype (a torch dtype)."""
    N, H, W, _ = x.shape
    K, cout = w2d.shape
    ldp = (K + 7) // 8 * 8
    out = torch.empty((N, H, W, cout), dtype=out_dtype, device=x.device)
    step = _chunk(H * W, ldp, x.element_size())
    for c0 in range(0, N, step):
        pat = ops.im2col(x[c0:c0 + step], kh, kw, 1, 1, ldp=ldp)
        ops.gemm(pat[:, :K], w2d, bias=b, relu=True, out=out[c0:c0 + step].view(-1, cout))
    return out


def wgrad_im2col(x_in, dpre, kh, kw, gw, gb):
    """Weight and bias gradients of that convolution into gw ([kh*kw*Cin, Cout] view of the HWIO gradient) and gb."""
    N, H, W, _ = x_in.shape
    K, cout = gw.shape
    ldp = (K + 7) // 8 * 8
    step = _chunk(H * W, ldp, x_in.element_size())
    d2 = dpre.view(N * H * W, cout)
    for ci, c0 in enumerate(range(0, N, step)):
        pat = ops.im2col(x_in[c0:c0 + step], kh, kw, 1, 1, ldp=ldp)
        ops.gemm(pat[:, :K], d2[c0 * H * W:(c0 + step) * H * W], transA=True, out=gw, accumulate=(ci > 0))
    ops.colsum(d2, out=gb)


def dgrad_im2col(dpre, kh, kw, w2d):
    """fp32 data gradient of that convolution through GEMM + asr_col2im, chunked."""
    N, H, W, cout = dpre.shape
    K = w2d.shape[0]
    cin = K // (kh * kw)
    din = torch.empty((N, H, W, cin), dtype=torch.float32, device=dpre.device)
    step = _chunk(H * W, K, 4)
    for c0 in range(0, N, step):
        dc = dpre[c0:c0 + step]
        n = dc.shape[0]
        dpat = ops.gemm(dc.reshape(n * H * W, cout), w2d, transB=True, out_dtype=ASR_F32)
        din[c0:c0 + n] = ops.col2im(dpat, n, H, W, cin, kh, kw, 1, 1)
    return din


# ---------------------------------------------------------------------- fully connected stack
def fc_forward(store, sh, names, h_in, drops, out=None):
    """relu(h @ weights + biases) for each layer of `names`, followed by dropout where drops[k] = (keep, seed, offset)
    is not None.  `sh` is the store's shadow in the operand dtype; `out`, if given, receives the last layer's ReLU
    output.  Returns (the stack's output, [(h_in, a, drop)] per layer for fc_backward)."""
    saved = []
    for k, name in enumerate(names):
        a = ops.gemm(h_in, sh[name + '/weights'], bias=store[name + '/biases'], relu=True,
                     out=out if k == len(names) - 1 else None)
        d = drops[k]
        ad = ops.dropout_apply(a, *d) if d is not None else a
        saved.append((h_in, a, d))
        h_in = ad
    return h_in, saved


def fc_backward(store, sh, names, saved, d):
    """d fp32: the gradient at the stack's output.  Fills the gradients of every layer, returns the fp32 gradient at the
    stack's input."""
    for k in reversed(range(len(names))):
        name = names[k]
        h_in, a, dr = saved[k]
        dpre = ops.relu_bwd(d, a, drop=dr)
        ops.gemm(h_in, dpre, transA=True, out=store.g(name + '/weights'))
        ops.colsum(dpre, out=store.g(name + '/biases'))
        d = ops.gemm(dpre, sh[name + '/weights'], transB=True, out_dtype=ASR_F32)
    return d


# ---------------------------------------------------------------------- back to the time-major padded grid
def gather_time_major(table, inv):
    """table [N + 1, U] whose last row is zeros, inv int32 [T * Bp]: for every row t*Bp + b of the time-major padded
    grid its row of `table`, N at padded positions (they read the zero row) -> [T * Bp, U].  A row copy: a bf16 table
    moves as fp32 words, two values each."""
    bf = table.dtype == torch.bfloat16
    out = ops.embedding_gather(table.view(torch.float32) if bf else table, inv)
    return out.view(torch.bfloat16) if bf else out
