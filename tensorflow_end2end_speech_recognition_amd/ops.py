"""Thin torch-tensor front end of the C ABI (include/asr_hip.h).

torch owns device memory and the stream; every function below hands raw device
pointers + shapes to libasr_hip.so.  No arithmetic happens in torch here and
there is no CPU fallback: non-CUDA tensors raise.
"""
import ctypes as C
import math
import os
import time as _time

import numpy as np
import torch

from . import _counters, _lib
from ._lib import ASR_BF16, ASR_F32

TORCH_DTYPE = {ASR_F32: torch.float32, ASR_BF16: torch.bfloat16}


def dtype_id(dtype):
    if dtype in (ASR_F32, 'f32', 'fp32', 'float32', torch.float32):
        return ASR_F32
    if dtype in (ASR_BF16, 'bf16', 'bfloat16', torch.bfloat16):
        return ASR_BF16
    raise ValueError('dtype must be f32 or bf16, got %r' % (dtype,))


_lane = 0            # 0: main stream / handle, 1: side stream / second handle (side_lane)
_side = {}           # device index -> dict(stream, keep)


def _h(t):
    if not t.is_cuda:
        raise RuntimeError('HIP path needs a CUDA(ROCm) tensor; there is no CPU fallback')
    return _lib.handle(t.device.index or 0, _lane)


def debug_placement(nblocks, stream=None, spin_cycles=200000, device=0):
    """[nblocks, 2] int32 (XCC id, HW_ID) of a probe grid launched on `stream` (default: current)."""
    h = _lib.handle(device, 0)
    out = torch.zeros((nblocks, 2), dtype=torch.int32, device='cuda:%d' % device)
    sp = C.c_void_p(stream.cuda_stream) if stream is not None else _s()
    h.check(h.lib.asr_debug_placement(h.h, _p(out), nblocks, spin_cycles, sp), 'asr_debug_placement')
    return out


class side_lane(object):
    """Issue the enclosed launches on a side HIP stream (with its own handle, i.e. its own
    split-K scratch) ordered after everything already on the main stream.  Used for work
    nothing downstream waits on until later (weight images of the layers ahead, weight-gradient
    GEMMs), so it overlaps with the recurrence kernels, which only occupy a handful of CUs.
    `lane` 1, 2, ...: independent side streams (the two directions of a layer's weight gradients
    run side by side on lanes 1 and 2).
    `keep`: tensors the side work reads/writes -- held until join_side() so the caching
    allocator cannot hand their memory to later main-stream allocations."""

    def __init__(self, device, keep=(), lane=1, after=None):
        self.dev = device.index or 0
        self.keep = list(keep)
        self.lane = int(lane)
        # after: an event already recorded on the main stream (stream_event()): the lane starts behind THAT point and
        # nothing new is put on the main stream (every marker there costs ~6 us of an in-order queue's time: measured
        # 25 us between a layer's dx GEMM and the next BPTT kernel with four lane entries in between)
        self.after = after

    def __enter__(self):
        global _lane
        st = _side.get((self.dev, self.lane))
        if st is None:
            st = _side[(self.dev, self.lane)] = dict(stream=torch.cuda.Stream(device=self.dev), keep=[])
        st['keep'].extend(self.keep)
        if self.after is not None:
            st['stream'].wait_event(self.after)
        else:
            st['stream'].wait_stream(_cur_stream(self.dev))
        self._ctx = torch.cuda.stream(st['stream'])
        self._ctx.__enter__()
        self._prev = _lane
        _lane = self.lane
        return self

    def __exit__(self, *exc):
        global _lane
        _lane = self._prev
        self._ctx.__exit__(*exc)
        return False


def set_side_xcd_skip(device, n):
    """The side lanes' reduction-major GEMMs leave the first n XCDs alone (asr_set_xcd_skip).  An experiment knob, off
    by default: keeping the weight-gradient GEMMs off the recurrence clusters' XCDs (their L2s carry the per-step
    hand-off) was measured on the headline step -- BPTT launch 1321 us (n = 0), 1314 us (n = 2), 1362 us (n = 4) -- so
    whatever stretches the recurrence beside the side GEMMs (1.19 ms alone) is not L2 sharing."""
    dev = device.index or 0
    for lane in (1, 2):
        h = _lib.handle(dev, lane)
        if getattr(h, '_xcd_skip', None) != n:
            h.check(h.lib.asr_set_xcd_skip(h.h, int(n)), 'asr_set_xcd_skip')
            h._xcd_skip = n


def set_side_gemm_workgroups(device, n):
    """Workgroups the side lanes' reduction-major (weight-gradient) GEMMs aim at (asr_set_gemm_tn_workgroups): 32 for
    GEMMs that run beside a recurrence kernel, 0 (default, ~2 per CU) for exposed ones."""
    dev = device.index or 0
    for lane in (1, 2):
        h = _lib.handle(dev, lane)
        if getattr(h, '_tn_wgs', None) != n:
            h.check(h.lib.asr_set_gemm_tn_workgroups(h.h, int(n)), 'asr_set_gemm_tn_workgroups')
            h._tn_wgs = n


def keep_on_lane(device, lane, tensors):
    """Hold `tensors` until join_side(): work already issued on side lane `lane` reads or writes them."""
    st = _side.get((device.index or 0, int(lane)))
    if st is not None:
        st['keep'].extend(tensors)


def join_side(device):
    """Main stream waits for all side-lane work; releases the tensors held for it."""
    dev = device.index or 0
    for (d, lane), st in _side.items():
        if d != dev:
            continue
        _cur_stream(dev).wait_stream(st['stream'])
        st['keep'] = []


def stream_event():
    """Event recorded on the CURRENT stream (inside a side_lane block: on that lane).  wait_event(ev) makes the
    then-current stream wait for exactly this point instead of for everything on the other stream."""
    ev = torch.cuda.Event()
    ev.record(_cur_stream())
    return ev


def wait_event(ev):
    if ev is not None:
        _cur_stream().wait_event(ev)


_stream_objs = {}


def _raw_stream(dev=None):
    """Raw hipStream_t of torch's current stream (torch.cuda.current_stream() resolves the device through four Python
    layers every time: 1.1 ms of a 3.8 ms step issue at ~160 calls per step)."""
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice() if dev is None else dev)


def _cur_stream(dev=None):
    """torch.cuda.current_stream(dev) as a cached Stream object, looked up by its raw handle."""
    # the default stream's raw handle is 0 on EVERY device: the key must carry the resolved device index, or a process
    # that touches a second GPU would be handed the first one's stream object
    d = torch._C._cuda_getDevice() if dev is None else (dev.index if isinstance(dev, torch.device) else dev)
    if d is None:
        d = torch._C._cuda_getDevice()
    raw = torch._C._cuda_getCurrentRawStream(d)
    key = (d, raw)
    so = _stream_objs.get(key)
    if so is None:
        so = _stream_objs[key] = torch.cuda.current_stream(dev)
    return so


def _s():
    return C.c_void_p(_raw_stream())


def to_device(x, dtype, dev):
    """Host array / list / CPU tensor -> device tensor WITHOUT draining the stream: staged in pinned memory and copied
    with non_blocking=True (a pageable `torch.as_tensor(x, device=dev)` waits for everything enqueued before it -- one
    such call per training step makes the whole step host-synchronous).  Device tensors pass through (dtype converted on
    the device).  torch's caching host allocator keeps the pinned block alive until the copy has run."""
    if torch.is_tensor(x) and x.is_cuda:
        return x if x.dtype == dtype else x.to(dtype)
    t = torch.as_tensor(x) if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    if t.dtype != dtype:
        t = t.to(dtype)
    t = t.contiguous()
    if torch.device(dev).type != 'cuda':
        return t.to(dev)
    return t.pin_memory().to(dev, non_blocking=True)


_upload_streams = {}


def upload_ints(dev, vectors):
    """Host int vectors -> int32 device vectors through ONE pinned staging buffer and ONE asynchronous copy, issued on
    an upload stream of its own and joined to the current stream by an event.  A CTC step hands over three such vectors
    (frame counts, label offsets, labels); as three copies on the main stream they and the queue gaps between them held
    the first kernel of the step back by 50 us behind the previous step's optimizer (profiles/r06_step_timeline.md); on
    the upload stream the copy runs as soon as the host has issued it, beside whatever the main stream is still doing.
    (Step time of the headline bench is unchanged by it, 8.90 ms: without the profiler the host runs steps ahead and the
    copies' gaps were the profiler's; what remains is two packets fewer on the main stream.)
    Device vectors pass through (converted to int32 on the device).  Each result starts on a 16-byte boundary."""
    d = torch.device(dev)
    out, host = [None] * len(vectors), []
    for i, v in enumerate(vectors):
        if torch.is_tensor(v) and v.is_cuda:
            out[i] = v if v.dtype == torch.int32 else v.to(torch.int32)
        else:
            a = v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)
            host.append((i, np.ascontiguousarray(a, dtype=np.int32).ravel()))
    if not host:
        return out
    if d.type != 'cuda':
        for i, a in host:
            out[i] = torch.from_numpy(a.copy()).to(d)
        return out
    starts, n = [], 0
    for _, a in host:
        starts.append(n)
        n += max(4, a.size + (-a.size) % 4)
    stage = torch.zeros(n, dtype=torch.int32).pin_memory()
    sv = stage.numpy()
    for (_, a), s0 in zip(host, starts):
        sv[s0:s0 + a.size] = a
    idx = d.index if d.index is not None else torch._C._cuda_getDevice()
    up = _upload_streams.get(idx)
    if up is None:
        up = _upload_streams[idx] = torch.cuda.Stream(device=idx)
    with torch.cuda.stream(up):
        buf = stage.to(d, non_blocking=True)      # allocated in the upload stream's pool: no wait for the main stream
    ev = torch.cuda.Event()
    ev.record(up)
    cur = _cur_stream(idx)
    cur.wait_event(ev)
    buf.record_stream(cur)                        # side lanes fork from / join into this stream within the step
    for (i, a), s0 in zip(host, starts):
        out[i] = buf[s0:s0 + a.size]
    return out


_host_copies = {}


def host_ints(x):
    """Host numpy view of an integer vector the caller may hand over on the host (the reference feeds seq_len as numpy,
    examples/timit/training/train_ctc.py:134-144) or on the device.  A device tensor costs ONE synchronising copy the
    first time it is seen; the copy is remembered for that tensor OBJECT (weak reference + version counter: a new tensor
    that merely reuses the address, or an in-place update, is read again), so a batch object reused across steps (bench
    loops, an epoch cached on the device) never drains the stream a second time."""
    if not torch.is_tensor(x):
        return np.asarray(x)
    if not x.is_cuda:
        return x.detach().numpy()
    import weakref
    hit = _host_copies.get(id(x))
    if hit is not None and hit[0]() is x and hit[1] == x._version:
        return hit[2]
    if len(_host_copies) > 64:
        for k in [k for k, v in _host_copies.items() if v[0]() is None]:
            del _host_copies[k]
        if len(_host_copies) > 64:
            _host_copies.clear()
    host = x.detach().cpu().numpy()
    _host_copies[id(x)] = (weakref.ref(x), x._version, host)
    return host


def invalidate_host_ints(x=None):
    """Forget the remembered host copy of device vector `x` (all of them when None).  The version counter host_ints keys
    on does not move for writes torch does not see -- `x.data.copy_()`, a kernel launched on `x.data_ptr()` through ctypes
    (this library's own calls), DLPack consumers: a caller that rewrites a length vector that way, in place, says so here
    (or, simpler, hands the lengths over on the host, as the reference's feed_dict does)."""
    if x is None:
        _host_copies.clear()
    else:
        _host_copies.pop(id(x), None)


def _p(t):
    if t is None:
        return None
    if not t.is_contiguous():
        raise ValueError('tensor must be contiguous')
    return C.c_void_p(t.data_ptr())


def _chk(t, dtype, name):
    if t.dtype != dtype:
        raise ValueError('%s must be %s, got %s' % (name, dtype, t.dtype))


# ---------------------------------------------------------------- layout / casts
def bt_to_tb(x_btd, dtype=ASR_F32, ld=None):
    """[B,T,D] fp32 -> [T,B,ld] in `dtype`; columns D..ld-1 (ld defaults to D) are zero -- the reduction width the
    lean GEMM wants (a multiple of 64) when D is not one."""
    h = _h(x_btd)
    _chk(x_btd, torch.float32, 'inputs')
    B, T, D = x_btd.shape
    ld = D if ld is None else int(ld)
    out = torch.empty((T, B, ld), dtype=TORCH_DTYPE[dtype], device=x_btd.device)
    h.check(h.lib.asr_bt_to_tb_ld(h.h, dtype, _p(x_btd), _p(out), B, T, D, ld, _s()), 'asr_bt_to_tb')
    return out


SUBSAMPLE_TYPES = {'drop': 0, 'concat': 1}     # asr_subsample_type


def _subsample_type(kind):
    if kind not in SUBSAMPLE_TYPES:
        raise ValueError('subsample_type is "drop" or "concat", got %r' % (kind,))
    return SUBSAMPLE_TYPES[kind]


def time_subsample_fwd(x_tb, seq_len, batch, kind='drop'):
    """One 2x reduction in time of a recurrence's time-major output x [T,Bp,W] (fp32 or bf16) with lengths seq_len [Bp]
    (asr_time_subsample_fwd): returns (y [batch, T//2, W'] fp32 batch-major -- 'drop': frame 2t'+1, W' = W; 'concat':
    frames 2t', 2t'+1 side by side, W' = 2W; zero from seq_len >> 1 on -- and the halved lengths [Bp] int32)."""
    h = _h(x_tb)
    typ = _subsample_type(kind)
    _chk(seq_len, torch.int32, 'seq_len')
    T, Bp, W = x_tb.shape
    dtype = dtype_id(x_tb.dtype)
    if seq_len.shape[0] != Bp or not 0 <= batch <= Bp:
        raise ValueError('time_subsample_fwd: %d lengths, batch %d for a padded batch of %d' % (seq_len.shape[0], batch, Bp))
    y = torch.empty((batch, T // 2, W * (2 if typ else 1)), dtype=torch.float32, device=x_tb.device)
    len_out = torch.empty((Bp,), dtype=torch.int32, device=x_tb.device)
    h.check(h.lib.asr_time_subsample_fwd(h.h, dtype, typ, _p(x_tb), _p(seq_len), T, Bp, int(batch), W, _p(y),
                                         _p(len_out), _s()), 'asr_time_subsample_fwd')
    return y, len_out


def time_subsample_bwd(dy_tb, len_out, T, kind='drop', out=None):
    """The transpose of time_subsample_fwd: dy [T//2,Bp,W'] fp32 time-major and the halved lengths [Bp] ->
    dx [T,Bp,W] fp32 (`out` or a new tensor), every element written (asr_time_subsample_bwd)."""
    h = _h(dy_tb)
    typ = _subsample_type(kind)
    _chk(dy_tb, torch.float32, 'dy')
    _chk(len_out, torch.int32, 'len_out')
    T2, Bp, Wo = dy_tb.shape
    if T2 != int(T) // 2 or len_out.shape[0] != Bp or (typ and Wo % 2):
        raise ValueError('time_subsample_bwd: dy %s does not belong to T = %d / %d lengths'
                         % (tuple(dy_tb.shape), T, len_out.shape[0]))
    W = Wo // 2 if typ else Wo
    dx = out if out is not None else torch.empty((int(T), Bp, W), dtype=torch.float32, device=dy_tb.device)
    if out is not None and (tuple(out.shape) != (int(T), Bp, W) or out.dtype != torch.float32):
        raise ValueError('time_subsample_bwd: out must be fp32 %s' % ((int(T), Bp, W),))
    h.check(h.lib.asr_time_subsample_bwd(h.h, typ, _p(dy_tb), _p(len_out), int(T), Bp, W, _p(dx), _s()),
            'asr_time_subsample_bwd')
    return dx


def _drop_args(drop):
    """(keep_prob, seed, offset) of a dropout descriptor; None: no dropout (keep_prob 1)."""
    if drop is None:
        return 1.0, 0, 0
    keep, seed, offset = drop
    if not 0.0 < float(keep) <= 1.0:
        raise ValueError('dropout descriptor: keep_prob must be in (0, 1], got %r' % (keep,))
    return float(keep), int(seed), int(offset)


def residual_fwd(h_tb, skip, seq_len, drop=None, sum_out=None, out=None):
    """A skip connection behind a recurrent layer (asr_residual_fwd; encoder_residual / encoder_dense_residual):
    out = round(m * h + skip) [T,Bp,W] in h's dtype for the layer's output h (fp32 or bf16), skip in h's dtype or fp32,
    lengths seq_len [Bp] and drop = (keep_prob, seed, offset) -- the mask dropout_mask(h.shape, ...) would hold -- or
    None.  sum_out: None, True (a new fp32 tensor) or an fp32 [T,Bp,W] tensor, which may be an fp32 `skip` itself
    (updated in place), receives skip + out.  Frames t >= seq_len[b] are not read and come back zero.
    Returns out (`out` or a new tensor), or (out, sum_out) when sum_out was asked for."""
    h = _h(h_tb)
    _chk(seq_len, torch.int32, 'seq_len')
    dtype = dtype_id(h_tb.dtype)
    if h_tb.dim() != 3 or tuple(skip.shape) != tuple(h_tb.shape) or seq_len.shape[0] != h_tb.shape[1]:
        raise ValueError('residual_fwd: h %s, skip %s, %d lengths' % (tuple(h_tb.shape), tuple(skip.shape),
                                                                      seq_len.shape[0]))
    if skip.dtype != h_tb.dtype and skip.dtype != torch.float32:
        raise ValueError('residual_fwd: skip must be %s or fp32, got %s' % (h_tb.dtype, skip.dtype))
    if not skip.is_cuda or not seq_len.is_cuda:
        raise RuntimeError('HIP path needs a CUDA(ROCm) tensor; there is no CPU fallback')
    keep, seed, offset = _drop_args(drop)
    T, Bp, W = h_tb.shape
    if sum_out is True:
        sum_out = torch.empty((T, Bp, W), dtype=torch.float32, device=h_tb.device)
    if sum_out is not None and (tuple(sum_out.shape) != (T, Bp, W) or sum_out.dtype != torch.float32
                                or not sum_out.is_cuda):
        raise ValueError('residual_fwd: sum_out must be a device fp32 %s' % ((T, Bp, W),))
    if out is None:
        out = torch.empty_like(h_tb, memory_format=torch.contiguous_format)
    elif tuple(out.shape) != (T, Bp, W) or out.dtype != h_tb.dtype or not out.is_cuda:
        raise ValueError('residual_fwd: out must be a device %s %s' % (h_tb.dtype, (T, Bp, W)))
    h.check(h.lib.asr_residual_fwd(h.h, dtype, dtype_id(skip.dtype), _p(h_tb), _p(skip), _p(seq_len), T, Bp, W, keep,
                                   seed, offset, _p(out), _p(sum_out), _s()), 'asr_residual_fwd')
    return out if sum_out is None else (out, sum_out)


def residual_bwd(dx_raw, carry, seq_len, drop=None, dense=False, dout=None, carry_out=None):
    """The backward pass at a skip connection (asr_residual_bwd), all fp32 [T,Bp,W]: g = dx_raw + carry, returns
    (dout = m * g, carry_out = g, or g + carry with dense) -- new tensors, or the ones handed in: `dout` may be dx_raw
    itself and `carry_out` may be carry itself.  Frames t >= seq_len[b] are not read (dx_raw may be unwritten there) and come back zero in both."""
    h = _h(dx_raw)
    _chk(dx_raw, torch.float32, 'dx_raw')
    _chk(carry, torch.float32, 'carry')
    _chk(seq_len, torch.int32, 'seq_len')
    if dx_raw.dim() != 3 or tuple(carry.shape) != tuple(dx_raw.shape) or seq_len.shape[0] != dx_raw.shape[1]:
        raise ValueError('residual_bwd: dx_raw %s, carry %s, %d lengths' % (tuple(dx_raw.shape), tuple(carry.shape),
                                                                            seq_len.shape[0]))
    if not carry.is_cuda or not seq_len.is_cuda:
        raise RuntimeError('HIP path needs a CUDA(ROCm) tensor; there is no CPU fallback')
    keep, seed, offset = _drop_args(drop)
    T, Bp, W = dx_raw.shape
    for name, t in (('dout', dout), ('carry_out', carry_out)):
        if t is not None and (tuple(t.shape) != (T, Bp, W) or t.dtype != torch.float32 or not t.is_cuda):
            raise ValueError('residual_bwd: %s must be a device fp32 %s' % (name, (T, Bp, W)))
    dout = dout if dout is not None else torch.empty_like(dx_raw, memory_format=torch.contiguous_format)
    carry_out = carry_out if carry_out is not None else torch.empty_like(carry, memory_format=torch.contiguous_format)
    h.check(h.lib.asr_residual_bwd(h.h, _p(dx_raw), _p(carry), _p(seq_len), T, Bp, W, keep, seed, offset,
                                   1 if dense else 0, _p(dout), _p(carry_out), _s()), 'asr_residual_bwd')
    return dout, carry_out


def stack_frames(x_btf, seq_len, num_stack, num_skip):
    """Zero-padded batch [B,T,F] fp32 + seq_len [B] int32 -> ([B, ceil(T/num_skip), F*num_stack], new seq_len)."""
    h = _h(x_btf)
    _chk(x_btf, torch.float32, 'inputs')
    _chk(seq_len, torch.int32, 'seq_len')
    if num_stack < num_skip:
        raise ValueError('num_skip must be less than num_stack.')
    B, T, F = x_btf.shape
    Tn = (T + num_skip - 1) // num_skip
    out = torch.empty((B, Tn, F * num_stack), dtype=torch.float32, device=x_btf.device)
    out_len = torch.empty((B,), dtype=torch.int32, device=x_btf.device)
    h.check(h.lib.asr_stack_frames(h.h, _p(x_btf), _p(seq_len), B, T, F, int(num_stack), int(num_skip), _p(out),
                                   _p(out_len), _s()), 'asr_stack_frames')
    return out, out_len


def splice(x_btd, seq_len, splice, num_stack=1):
    """Zero-padded batch [B,T,D] fp32 -> [B,T,D*splice], spliced per utterance over its own seq_len frames."""
    h = _h(x_btd)
    _chk(x_btd, torch.float32, 'inputs')
    _chk(seq_len, torch.int32, 'seq_len')
    B, T, D = x_btd.shape
    if D % (3 * num_stack) != 0:
        raise ValueError('frame width must be channels*3*num_stack')
    out = torch.empty((B, T, D * splice), dtype=torch.float32, device=x_btd.device)
    h.check(h.lib.asr_splice(h.h, _p(x_btd), _p(seq_len), B, T, D, int(splice), int(num_stack), _p(out), _s()),
            'asr_splice')
    return out


def transpose2d(x, out=None):
    """out[c, r] = x[r, c] for a 2-D tensor with unit inner stride."""
    h = _h(x)
    dt = dtype_id(x.dtype)
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError('transpose2d: 2-D tensor with unit inner stride expected')
    R, Cc = x.shape
    if out is None:
        out = torch.empty((Cc, R), dtype=x.dtype, device=x.device)
    h.check(h.lib.asr_transpose2d(h.h, dt, C.c_void_p(x.data_ptr()), R, Cc, x.stride(0),
                                  C.c_void_p(out.data_ptr()), out.stride(0), _s()), 'asr_transpose2d')
    return out


def cast_from_f32(x, dtype, out=None):
    h = _h(x)
    _chk(x, torch.float32, 'x')
    if out is None:
        out = torch.empty(x.shape, dtype=TORCH_DTYPE[dtype], device=x.device)
    h.check(h.lib.asr_cast_from_f32(h.h, dtype, _p(x), _p(out), x.numel(), _s()), 'asr_cast_from_f32')
    return out


def cast_to_f32(x, out=None):
    h = _h(x)
    dt = dtype_id(x.dtype)
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    h.check(h.lib.asr_cast_to_f32(h.h, dt, _p(x), _p(out), x.numel(), _s()), 'asr_cast_to_f32')
    return out


def apply_mask(x, mask, out=None):
    h = _h(x)
    dt = dtype_id(x.dtype)
    _chk(mask, torch.float32, 'mask')
    if out is None:
        out = torch.empty_like(x)
    h.check(h.lib.asr_apply_mask(h.h, dt, _p(x), _p(mask), _p(out), x.numel(), _s()), 'asr_apply_mask')
    return out


def dropout_mask(shape, keep_prob, seed, offset, device):
    mask = torch.empty(shape, dtype=torch.float32, device=device)
    h = _h(mask)
    h.check(h.lib.asr_dropout_mask(h.h, _p(mask), mask.numel(), float(keep_prob), int(seed),
                                   int(offset), _s()), 'asr_dropout_mask')
    return mask


def touch(t):
    """Read pass over a tensor (asr_touch): into the memory-side cache ahead of a latency-critical consumer."""
    h = _h(t)
    h.check(h.lib.asr_touch(h.h, _p(t), t.numel() * t.element_size(), _s()), 'asr_touch')


def dropout_apply(x, keep_prob, seed, offset):
    """x * dropout mask(seed, offset) without a mask tensor (== apply_mask(x, dropout_mask(x.shape, ...)) bit for bit)."""
    h = _h(x)
    out = torch.empty_like(x)
    h.check(h.lib.asr_dropout_apply(h.h, dtype_id(x.dtype), _p(x), _p(out), x.numel(), float(keep_prob), int(seed),
                                    int(offset), _s()), 'asr_dropout_apply')
    return out


def colsum(a, out=None):
    """sum over rows of a [M,N] (last-dim contiguous 2-D view) -> fp32 [N]."""
    h = _h(a)
    dt = dtype_id(a.dtype)
    M, N = a.shape
    if a.stride(1) != 1:
        raise ValueError('colsum: inner stride must be 1')
    if out is None:
        out = torch.empty((N,), dtype=torch.float32, device=a.device)
    h.check(h.lib.asr_colsum(h.h, dt, C.c_void_p(a.data_ptr()), M, N, a.stride(0), _p(out), _s()),
            'asr_colsum')
    return out


# ---------------------------------------------------------------- GEMM
def gemm(A, B, transA=False, transB=False, bias=None, out=None, out_dtype=None, accumulate=False, relu=False,
         mul=None, drop=None, rows=None):
    """C = op(A) @ op(B) (+bias) (+C).  A, B 2-D, same dtype (f32 or bf16), row stride = ld.
    mul: fp32 [M,N] multiplier of the result (a dropout mask); drop = (keep_prob, seed, offset): the same multiplier
    formed from the dropout generator's counter in the epilogue -- dropout_mask((M, N), ...) without the tensor.
    rows = (int32 device vector, count): only the rows of the result that the ASCENDING list names have to be right
    (asr_gemm_rows: fp32 output; the others are left as they were or written, the caller must not care which)."""
    h = _h(A)
    dt = dtype_id(A.dtype)
    if B.dtype != A.dtype:
        raise ValueError('gemm: A and B dtypes differ')
    for t, n in ((A, 'A'), (B, 'B')):
        if t.dim() != 2 or t.stride(1) != 1:
            raise ValueError('gemm: %s must be 2-D with unit inner stride' % n)
    M, K = (A.shape[1], A.shape[0]) if transA else (A.shape[0], A.shape[1])
    Kb, N = (B.shape[1], B.shape[0]) if transB else (B.shape[0], B.shape[1])
    if K != Kb:
        raise ValueError('gemm: inner dimensions differ (%d vs %d)' % (K, Kb))
    odt = dt if out_dtype is None else dtype_id(out_dtype)
    if out is None:
        out = torch.empty((M, N), dtype=TORCH_DTYPE[odt], device=A.device)
    else:
        odt = dtype_id(out.dtype)
        if out.shape != (M, N) or out.stride(1) != 1:
            raise ValueError('gemm: bad out shape %s' % (tuple(out.shape),))
    if bias is not None:
        _chk(bias, torch.float32, 'bias')
    if rows is not None:
        rt, nr = rows
        nr = int(nr)
        _chk(rt, torch.int32, 'rows')
        if odt != ASR_F32 or rt.dim() != 1 or not rt.is_contiguous() or not 0 <= nr <= min(rt.numel(), M):
            raise ValueError('gemm: rows needs an fp32 output and a contiguous int32 vector of at least `count` <= M rows')
        if mul is not None and drop is not None:
            raise ValueError('gemm: rows takes mul or drop, not both')
        if drop is not None and (not out.is_contiguous() or N % 4):
            raise ValueError('gemm: drop needs a contiguous fp32 output with N % 4 == 0')
        if mul is not None:
            _chk(mul, torch.float32, 'mul')
            if mul.dim() != 2 or mul.shape != (M, N) or mul.stride(1) != 1:
                raise ValueError('gemm: mul needs an fp32 output and an fp32 [M,N] multiplier')
        keep, seed, off = (float(drop[0]), int(drop[1]), int(drop[2])) if drop is not None else (0.0, 0, 0)
        h.check(h.lib.asr_gemm_rows(h.h, dt, int(transA), int(transB), M, N, K,
                                    C.c_void_p(A.data_ptr()), A.stride(0), C.c_void_p(B.data_ptr()), B.stride(0),
                                    C.c_void_p(out.data_ptr()), out.stride(0), _p(bias), int(accumulate),
                                    1 if relu else 0, C.c_void_p(mul.data_ptr()) if mul is not None else None,
                                    mul.stride(0) if mul is not None else 0,
                                    keep, seed, off, C.c_void_p(rt.data_ptr()), nr, _s()), 'asr_gemm_rows')
        return out
    if drop is not None:
        if odt != ASR_F32 or not out.is_contiguous() or N % 4:
            raise ValueError('gemm: drop needs a contiguous fp32 output with N % 4 == 0')
        h.check(h.lib.asr_gemm_drop(h.h, dt, int(transA), int(transB), M, N, K,
                                    C.c_void_p(A.data_ptr()), A.stride(0), C.c_void_p(B.data_ptr()), B.stride(0),
                                    C.c_void_p(out.data_ptr()), out.stride(0), _p(bias), int(accumulate),
                                    1 if relu else 0, float(drop[0]), int(drop[1]), int(drop[2]), _s()), 'asr_gemm_drop')
        return out
    if mul is not None:   # fp32 output times an elementwise fp32 multiplier [M,N] (a dropout mask), in the epilogue
        _chk(mul, torch.float32, 'mul')
        if odt != ASR_F32 or mul.dim() != 2 or mul.shape != (M, N) or mul.stride(1) != 1:
            raise ValueError('gemm: mul needs an fp32 output and an fp32 [M,N] multiplier')
        h.check(h.lib.asr_gemm_mul(h.h, dt, int(transA), int(transB), M, N, K,
                                   C.c_void_p(A.data_ptr()), A.stride(0), C.c_void_p(B.data_ptr()), B.stride(0),
                                   C.c_void_p(out.data_ptr()), out.stride(0), _p(bias), int(accumulate),
                                   1 if relu else 0, C.c_void_p(mul.data_ptr()), mul.stride(0), _s()), 'asr_gemm_mul')
        return out
    h.check(h.lib.asr_gemm_act(h.h, dt, odt, int(transA), int(transB), M, N, K,
                               C.c_void_p(A.data_ptr()), A.stride(0), C.c_void_p(B.data_ptr()), B.stride(0),
                               C.c_void_p(out.data_ptr()), out.stride(0), _p(bias), int(accumulate),
                               1 if relu else 0, _s()), 'asr_gemm')
    return out


def gemm_tn_frames(A, B, seq_len, Bp, frame0=0, out=None, accumulate=False):
    """C [M,N] fp32 = A^T @ B for bf16 A [K,M], B [K,N] whose rows are the frames of a time-major [T,Bp] batch: row k is
    utterance k % Bp at frame frame0 + k // Bp.  B must be exactly zero in the rows of padded frames (frame >=
    seq_len[utterance]: the BPTT kernels' dgates); those rows are then loaded from neither operand and the result has
    the bits of gemm(A, B, transA=True) (asr_gemm_tn_frames).  seq_len: int32 device vector of at least Bp lengths."""
    h = _h(A)
    for t, n in ((A, 'A'), (B, 'B')):
        if t.dtype != torch.bfloat16 or t.dim() != 2 or t.stride(1) != 1:
            raise ValueError('gemm_tn_frames: %s must be 2-D bf16 with unit inner stride' % n)
    K, M = A.shape
    N = B.shape[1]
    Bp, frame0 = int(Bp), int(frame0)
    _chk(seq_len, torch.int32, 'seq_len')
    if B.shape[0] != K or Bp < 1 or K % Bp or frame0 < 0 or seq_len.dim() != 1 or not seq_len.is_contiguous() \
            or seq_len.numel() < Bp:
        raise ValueError('gemm_tn_frames: K = %d / %d rows, Bp = %d, %d lengths' % (K, B.shape[0], Bp, seq_len.numel()))
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    elif out.dtype != torch.float32 or out.shape != (M, N) or out.stride(1) != 1:
        raise ValueError('gemm_tn_frames: bad out %s' % (tuple(out.shape),))
    h.check(h.lib.asr_gemm_tn_frames(h.h, M, N, K, C.c_void_p(A.data_ptr()), A.stride(0), C.c_void_p(B.data_ptr()),
                                     B.stride(0), C.c_void_p(out.data_ptr()), out.stride(0), int(accumulate),
                                     _p(seq_len), Bp, frame0, _s()), 'asr_gemm_tn_frames')
    return out


def _out_like(out, shape, dtype, device, what):
    """`out` (a contiguous tensor of exactly this shape / dtype, e.g. a slice of a larger one along the first axis) or a fresh one."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or not out.is_contiguous():
        raise ValueError('%s: out must be a contiguous %s tensor of shape %s' % (what, dtype, tuple(shape)))
    return out


# ---------------------------------------------------------------- 3xK implicit-GEMM convolutions (VGG 3x3, cnn_zhang 3x5, students 3x4)
# One implementation per wrapper, parameterised by the filter and the C symbol prefix (csrc/conv.hip is templated on the
# tap geometry; csrc/conv3x3.hip adds the image-resident 3x3 forms behind the same signatures); the public conv3x3_* /
# conv3x5_* / conv3x4_* names are bound below with their own signatures.
_K3X3 = (3, 3, 'conv3x3')
_K3X5 = (3, 5, 'conv3x5')
_K3X4 = (3, 4, 'conv3x4')


def _conv3xk_prep_weights(geom, w_hwio):
    kh, kw, pre = geom
    fn = pre + '_prep_weights'
    h = _h(w_hwio)
    _chk(w_hwio, torch.float32, 'w')
    fh, fw, Cin, Cout = w_hwio.shape
    if (fh, fw) != (kh, kw):
        raise ValueError('%s: filter is %dx%d' % (fn, fh, fw))
    wf = torch.empty((Cout, kh * kw * Cin), dtype=torch.bfloat16, device=w_hwio.device)
    wb = torch.empty((Cin, kh * kw * Cout), dtype=torch.bfloat16, device=w_hwio.device)
    h.check(getattr(h.lib, 'asr_' + fn)(h.h, _p(w_hwio.contiguous()), Cin, Cout, _p(wf), _p(wb), _s()), 'asr_' + fn)
    return wf, wb


def _conv3xk_fwd(geom, x_nhwc, wt_fwd, bias, relu, out, f32_out=None):
    """f32_out: None for asr_conv3x3_fwd / asr_conv3x5_fwd (bf16 output only); asr_conv3x4_fwd takes it as one more argument."""
    fn = geom[2] + '_fwd'
    h = _h(x_nhwc)
    _chk(x_nhwc, torch.bfloat16, 'x')
    N, H, W, Cin = x_nhwc.shape
    Cout = wt_fwd.shape[0]
    out = _out_like(out, (N, H, W, Cout), torch.float32 if f32_out else torch.bfloat16, x_nhwc.device, fn)
    extra = () if f32_out is None else (int(f32_out),)
    h.check(getattr(h.lib, 'asr_' + fn)(h.h, _p(x_nhwc), N, H, W, Cin, _p(wt_fwd), _p(bias), Cout, 1 if relu else 0,
                                        *extra, _p(out), _s()), 'asr_' + fn)
    return out


def _conv3xk_fwd_drop(geom, x_nhwc, wt_fwd, bias, drop, out):
    fn = geom[2] + '_fwd_drop'
    h = _h(x_nhwc)
    _chk(x_nhwc, torch.bfloat16, 'x')
    N, H, W, Cin = x_nhwc.shape
    Cout = wt_fwd.shape[0]
    out = _out_like(out, (N, H, W, Cout), torch.bfloat16, x_nhwc.device, fn)
    h.check(getattr(h.lib, 'asr_' + fn)(h.h, _p(x_nhwc), N, H, W, Cin, _p(wt_fwd), _p(bias), Cout, float(drop[0]),
                                        int(drop[1]), int(drop[2]), _p(out), _s()), 'asr_' + fn)
    return out


def _conv3xk_bwd_data(geom, dy_nhwc, wt_bwd):
    fn = geom[2] + '_bwd_data'
    h = _h(dy_nhwc)
    _chk(dy_nhwc, torch.bfloat16, 'dy')
    N, H, W, Cout = dy_nhwc.shape
    Cin = wt_bwd.shape[0]
    dx = torch.empty((N, H, W, Cin), dtype=torch.float32, device=dy_nhwc.device)
    h.check(getattr(h.lib, 'asr_' + fn)(h.h, _p(dy_nhwc), N, H, W, Cout, _p(wt_bwd), Cin, _p(dx), _s()), 'asr_' + fn)
    return dx


def _conv3xk_bwd_data_relu(geom, dy_nhwc, wt_bwd, act_below, drop, dropped):
    fn = geom[2] + '_bwd_data_relu'
    h = _h(dy_nhwc)
    _chk(dy_nhwc, torch.bfloat16, 'dy')
    _chk(act_below, torch.bfloat16, 'act_below')
    N, H, W, Cout = dy_nhwc.shape
    Cin = wt_bwd.shape[0]
    if tuple(act_below.shape) != (N, H, W, Cin):
        raise ValueError('%s: act_below has shape %s' % (fn, tuple(act_below.shape)))
    dpre = torch.empty((N, H, W, Cin), dtype=torch.bfloat16, device=dy_nhwc.device)
    k, sd, off = drop if drop is not None else (1.0, 0, 0)
    # dropped=True: act_below is the DROPPED activation (*_fwd_drop): no mask is formed, dx * (1 / keep) where it is > 0
    mode = 0 if drop is None else (2 if dropped else 1)
    h.check(getattr(h.lib, 'asr_' + fn)(h.h, _p(dy_nhwc), N, H, W, Cout, _p(wt_bwd), Cin, _p(act_below), float(k), int(sd),
                                        int(off), mode, _p(dpre), _s()), 'asr_' + fn)
    return dpre


def _conv3xk_bwd_weight_bias(geom, x_nhwc, dy_nhwc, dw, dbias):
    kh, kw, pre = geom
    taps, fn = kh * kw, pre + '_bwd_weight_bias'
    h = _h(x_nhwc)
    _chk(x_nhwc, torch.bfloat16, 'x')
    _chk(dy_nhwc, torch.bfloat16, 'dy')
    if dbias is not None:
        _chk(dbias, torch.float32, 'dbias')
    N, H, W, Cin = x_nhwc.shape
    Cout = dy_nhwc.shape[3]
    if dw.numel() != taps * Cin * Cout or not dw.is_contiguous():
        raise ValueError('%s: dw must be a contiguous [%d*Cin, Cout] fp32 tensor' % (fn, taps))
    if dbias is not None and dbias.numel() != Cout:
        raise ValueError('%s: dbias has %d elements, Cout = %d' % (fn, dbias.numel(), Cout))
    h.check(getattr(h.lib, 'asr_' + fn)(h.h, _p(x_nhwc), _p(dy_nhwc), N, H, W, Cin, Cout, _p(dw), _p(dbias), _s()),
            'asr_' + fn)
    return dw, dbias


# ---------------------------------------------------------------- VGG front-end
def conv3x3_prep_weights(w_hwio):
    """fp32 [3,3,Cin,Cout] -> (wt_fwd bf16 [Cout, 9*Cin], wt_bwd bf16 [Cin, 9*Cout]: the flipped-tap image)."""
    return _conv3xk_prep_weights(_K3X3, w_hwio)


def conv3x3_fwd(x_nhwc, wt_fwd, bias, relu=True, out=None):
    """relu?(conv3x3 SAME(x) + bias): x bf16 [N,H,W,Cin] -> bf16 [N,H,W,Cout] (implicit GEMM, image-resident where it fits)."""
    return _conv3xk_fwd(_K3X3, x_nhwc, wt_fwd, bias, relu, out)


def conv3x3_fwd_drop(x_nhwc, wt_fwd, bias, drop, out=None):
    """dropout_apply(conv3x3_fwd(x, ..., relu=True), *drop) in one launch (the undropped activation is never written)."""
    return _conv3xk_fwd_drop(_K3X3, x_nhwc, wt_fwd, bias, drop, out)


def conv3x3_bwd_data(dy_nhwc, wt_bwd):
    """dx fp32 [N,H,W,Cin] = data gradient of the 3x3 convolution (dy bf16 [N,H,W,Cout])."""
    return _conv3xk_bwd_data(_K3X3, dy_nhwc, wt_bwd)


def conv3x3_smallc_fwd(x_nhwc, w2d, bias, relu=True):
    """Direct 3x3 SAME convolution for 9*Cin <= 32, Cout == 64 (bf16): x [N,H,W,Cin], w2d [9*Cin, 64] bf16 -> [N,H,W,64]."""
    h = _h(x_nhwc)
    _chk(x_nhwc, torch.bfloat16, 'x')
    _chk(w2d, torch.bfloat16, 'w2d')
    N, H, W, Cin = x_nhwc.shape
    out = torch.empty((N, H, W, w2d.shape[1]), dtype=torch.bfloat16, device=x_nhwc.device)
    h.check(h.lib.asr_conv3x3_smallc_fwd(h.h, _p(x_nhwc), N, H, W, Cin, _p(w2d), _p(bias), w2d.shape[1], int(relu),
                                         _p(out), _s()), 'asr_conv3x3_smallc_fwd')
    return out


def conv3x3_smallc_fwd_drop(x_nhwc, w2d, bias, drop, out=None):
    """dropout_apply(conv3x3_smallc_fwd(x, ..., relu=True), *drop) in one launch."""
    h = _h(x_nhwc)
    _chk(x_nhwc, torch.bfloat16, 'x')
    _chk(w2d, torch.bfloat16, 'w2d')
    N, H, W, Cin = x_nhwc.shape
    out = _out_like(out, (N, H, W, w2d.shape[1]), torch.bfloat16, x_nhwc.device, 'conv3x3_smallc_fwd_drop')
    h.check(h.lib.asr_conv3x3_smallc_fwd_drop(h.h, _p(x_nhwc), N, H, W, Cin, _p(w2d), _p(bias), w2d.shape[1],
                                              float(drop[0]), int(drop[1]), int(drop[2]), _p(out), _s()),
            'asr_conv3x3_smallc_fwd_drop')
    return out


def conv3x3_smallc_bwd_weight(x_nhwc, dpre_nhwc, dw):
    """dw fp32 [9*Cin, 64] = patches(x)^T dpre (both bf16), no patch matrix."""
    h = _h(x_nhwc)
    _chk(x_nhwc, torch.bfloat16, 'x')
    _chk(dpre_nhwc, torch.bfloat16, 'dpre')
    N, H, W, Cin = x_nhwc.shape
    h.check(h.lib.asr_conv3x3_smallc_bwd_weight(h.h, _p(x_nhwc), _p(dpre_nhwc), N, H, W, Cin, dpre_nhwc.shape[-1],
                                                _p(dw), _s()), 'asr_conv3x3_smallc_bwd_weight')
    return dw


def conv3x3_smallc_bwd_weight_bias(x_nhwc, dpre_nhwc, dw, dbias):
    """conv3x3_smallc_bwd_weight + dbias fp32 [64] = column sums of dpre, in the same two launches."""
    h = _h(x_nhwc)
    _chk(x_nhwc, torch.bfloat16, 'x')
    _chk(dpre_nhwc, torch.bfloat16, 'dpre')
    _chk(dbias, torch.float32, 'dbias')
    N, H, W, Cin = x_nhwc.shape
    if dbias.numel() != dpre_nhwc.shape[-1]:
        raise ValueError('conv3x3_smallc_bwd_weight_bias: dbias has %d elements' % dbias.numel())
    h.check(h.lib.asr_conv3x3_smallc_bwd_weight_bias(h.h, _p(x_nhwc), _p(dpre_nhwc), N, H, W, Cin, dpre_nhwc.shape[-1],
                                                     _p(dw), _p(dbias), _s()), 'asr_conv3x3_smallc_bwd_weight_bias')
    return dw, dbias


def conv3x3_bwd_data_relu(dy_nhwc, wt_bwd, act_below, drop=None, dropped=False):
    """relu_bwd(conv3x3_bwd_data(dy, wt_bwd), act_below, drop=drop) without the fp32 gradient in between -> bf16."""
    return _conv3xk_bwd_data_relu(_K3X3, dy_nhwc, wt_bwd, act_below, drop, dropped)


def conv3x3_bwd_weight(x_nhwc, dy_nhwc, dw, accumulate=False):
    """dw: fp32 [9*Cin, Cout] view of the HWIO gradient."""
    h = _h(x_nhwc)
    _chk(x_nhwc, torch.bfloat16, 'x')
    _chk(dy_nhwc, torch.bfloat16, 'dy')
    N, H, W, Cin = x_nhwc.shape
    Cout = dy_nhwc.shape[3]
    h.check(h.lib.asr_conv3x3_bwd_weight(h.h, _p(x_nhwc), _p(dy_nhwc), N, H, W, Cin, Cout, _p(dw),
                                         int(accumulate), _s()), 'asr_conv3x3_bwd_weight')
    return dw


def conv3x3_bwd_weight_bias(x_nhwc, dy_nhwc, dw, dbias):
    """dw: fp32 [9*Cin, Cout] view of the HWIO gradient, dbias: fp32 [Cout] = column sums of dy -- one call, the bias sums
    from the dy images the weight-gradient kernel stages anyway (asr_conv3x3_bwd_weight_bias)."""
    return _conv3xk_bwd_weight_bias(_K3X3, x_nhwc, dy_nhwc, dw, dbias)


def im2col3x3(x_nhwc, ldp=None, out=None):
    h = _h(x_nhwc)
    dt = dtype_id(x_nhwc.dtype)
    N, H, W, Cin = x_nhwc.shape
    ldp = ldp or 9 * Cin
    if out is None:
        out = torch.zeros((N * H * W, ldp), dtype=x_nhwc.dtype, device=x_nhwc.device)
    h.check(h.lib.asr_im2col3x3(h.h, dt, _p(x_nhwc), N, H, W, Cin, ldp, _p(out), _s()), 'asr_im2col3x3')
    return out


def col2im3x3(dpatches, N, H, W, Cin):
    h = _h(dpatches)
    _chk(dpatches, torch.float32, 'dpatches')
    din = torch.empty((N, H, W, Cin), dtype=torch.float32, device=dpatches.device)
    h.check(h.lib.asr_col2im3x3(h.h, _p(dpatches), N, H, W, Cin, dpatches.stride(0), _p(din), _s()), 'asr_col2im3x3')
    return din


def conv_out_hw(H, W, sh, sw):
    return (H + sh - 1) // sh, (W + sw - 1) // sw


def im2col(x_nhwc, kh, kw, sh, sw, ldp=None):
    """[N,H,W,Cin] -> patches [N*Ho*Wo, ldp] of a SAME convolution with any kernel / stride (columns past
    kh*kw*Cin zero)."""
    h = _h(x_nhwc)
    dt = dtype_id(x_nhwc.dtype)
    N, H, W, Cin = x_nhwc.shape
    Ho, Wo = conv_out_hw(H, W, sh, sw)
    K = kh * kw * Cin
    ldp = ldp or K
    out = torch.zeros((N * Ho * Wo, ldp), dtype=x_nhwc.dtype, device=x_nhwc.device) if ldp > K else \
        torch.empty((N * Ho * Wo, ldp), dtype=x_nhwc.dtype, device=x_nhwc.device)
    h.check(h.lib.asr_im2col(h.h, dt, _p(x_nhwc), N, H, W, Cin, kh, kw, sh, sw, ldp, _p(out), _s()), 'asr_im2col')
    return out


def col2im(dpatches, N, H, W, Cin, kh, kw, sh, sw):
    h = _h(dpatches)
    _chk(dpatches, torch.float32, 'dpatches')
    din = torch.empty((N, H, W, Cin), dtype=torch.float32, device=dpatches.device)
    h.check(h.lib.asr_col2im(h.h, _p(dpatches), N, H, W, Cin, kh, kw, sh, sw, dpatches.stride(0), _p(din), _s()),
            'asr_col2im')
    return din


def maxpool2x2_fwd(x_nhwc):
    h = _h(x_nhwc)
    dt = dtype_id(x_nhwc.dtype)
    N, H, W, Cc = x_nhwc.shape
    out = torch.empty((N, (H + 1) // 2, (W + 1) // 2, Cc), dtype=x_nhwc.dtype, device=x_nhwc.device)
    arg = torch.empty(out.shape, dtype=torch.uint8, device=x_nhwc.device)
    h.check(h.lib.asr_maxpool2x2_fwd(h.h, dt, _p(x_nhwc), N, H, W, Cc, _p(out), _p(arg), _s()), 'asr_maxpool2x2_fwd')
    return out, arg


def maxpool2x2_fwd_drop(x_nhwc, drop, out=None, arg=None):
    """dropout_apply(maxpool2x2_fwd(x)[0], *drop) and the argmax in one launch."""
    h = _h(x_nhwc)
    dt = dtype_id(x_nhwc.dtype)
    N, H, W, Cc = x_nhwc.shape
    out = _out_like(out, (N, (H + 1) // 2, (W + 1) // 2, Cc), x_nhwc.dtype, x_nhwc.device, 'maxpool2x2_fwd_drop')
    arg = _out_like(arg, tuple(out.shape), torch.uint8, x_nhwc.device, 'maxpool2x2_fwd_drop(arg)')
    h.check(h.lib.asr_maxpool2x2_fwd_drop(h.h, dt, _p(x_nhwc), N, H, W, Cc, _p(out), _p(arg), float(drop[0]), int(drop[1]),
                                          int(drop[2]), _s()), 'asr_maxpool2x2_fwd_drop')
    return out, arg


def maxpool2x2_bwd(dout, arg, H, W):
    h = _h(dout)
    N, _, _, Cc = dout.shape
    din = torch.empty((N, H, W, Cc), dtype=torch.float32, device=dout.device)
    h.check(h.lib.asr_maxpool2x2_bwd(h.h, _p(dout), _p(arg), N, H, W, Cc, _p(din), _s()), 'asr_maxpool2x2_bwd')
    return din


def maxpool2x2_relu_bwd(dout, arg, act, drop=None, pooled=None, hw=None):
    """relu_bwd(maxpool2x2_bwd(dropout_apply(dout, *drop)), act) in one pass: dout [N,Ho,Wo,C] fp32 pooled gradient,
    arg the pool's argmax, act [N,H,W,C] the ReLU output under the pool (operand dtype) -> dpre like act.
    pooled (with hw = (H, W)): the POOLED activation after its dropout (maxpool2x2_fwd_drop; or the plain pooled output when
    drop is None) instead of act -- it is > 0 exactly where the window's maximum was active and kept, so neither the
    full-resolution activation is read nor a mask formed."""
    h = _h(dout)
    k, sd, off = drop if drop is not None else (1.0, 0, 0)
    if pooled is not None:
        N, _, _, Cc = pooled.shape
        H, W = hw
        dpre = torch.empty((N, H, W, Cc), dtype=pooled.dtype, device=pooled.device)
        h.check(h.lib.asr_maxpool2x2_relu_bwd(h.h, dtype_id(pooled.dtype), _p(dout), _p(arg), _p(pooled), N, H, W, Cc, _p(dpre),
                                              float(k), 0, 0, 2, _s()), 'asr_maxpool2x2_relu_bwd')
        return dpre
    N, H, W, Cc = act.shape
    dpre = torch.empty_like(act)
    h.check(h.lib.asr_maxpool2x2_relu_bwd(h.h, dtype_id(act.dtype), _p(dout), _p(arg), _p(act), N, H, W, Cc, _p(dpre),
                                          float(k), int(sd), int(off), int(drop is not None), _s()),
            'asr_maxpool2x2_relu_bwd')
    return dpre


def relu_bwd_scaled(dout, out_dropped, keep):
    """dpre = (out_dropped > 0) ? dout * (1 / keep) : 0 (out_dropped: a ReLU output after its dropout with keep_prob keep)."""
    h = _h(dout)
    dpre = torch.empty_like(out_dropped)
    h.check(h.lib.asr_relu_bwd_scaled(h.h, dtype_id(out_dropped.dtype), _p(dout), _p(out_dropped), out_dropped.numel(),
                                      float(keep), _p(dpre), _s()), 'asr_relu_bwd_scaled')
    return dpre


def relu_bwd(dout, out, mask=None, drop=None):
    """dout fp32, out in the operand dtype -> dpre (operand dtype) = dout * (out>0) (* mask).
    drop = (keep_prob, seed, offset): the mask of dropout_apply with those arguments, formed in the kernel."""
    h = _h(dout)
    dt = dtype_id(out.dtype)
    dpre = torch.empty_like(out)
    if drop is not None:
        h.check(h.lib.asr_relu_bwd_drop(h.h, dt, _p(dout), _p(out), out.numel(), float(drop[0]), int(drop[1]),
                                        int(drop[2]), _p(dpre), _s()), 'asr_relu_bwd_drop')
        return dpre
    h.check(h.lib.asr_relu_bwd(h.h, dt, _p(dout), _p(out), _p(mask), out.numel(), _p(dpre), _s()), 'asr_relu_bwd')
    return dpre


# ---------------------------------------------------------------- cnn_zhang convolution stack (3x5 convolutions, 3x1 pool)
def conv3x5_prep_weights(w_hwio):
    """fp32 [3,5,Cin,Cout] -> (wt_fwd bf16 [Cout, 15*Cin], wt_bwd bf16 [Cin, 15*Cout]: the flipped-tap image)."""
    return _conv3xk_prep_weights(_K3X5, w_hwio)


def conv3x5_fwd(x_nhwc, wt_fwd, bias, relu=True, out=None):
    """relu?(conv3x5 SAME(x) + bias): x bf16 [N,H,W,Cin] -> bf16 [N,H,W,Cout] (implicit GEMM)."""
    return _conv3xk_fwd(_K3X5, x_nhwc, wt_fwd, bias, relu, out)


def conv3x5_fwd_drop(x_nhwc, wt_fwd, bias, drop, out=None):
    """dropout_apply(conv3x5_fwd(x, ..., relu=True), *drop) in one launch."""
    return _conv3xk_fwd_drop(_K3X5, x_nhwc, wt_fwd, bias, drop, out)


def conv3x5_bwd_data(dy_nhwc, wt_bwd):
    """dx fp32 [N,H,W,Cin] = data gradient of the 3x5 convolution (dy bf16 [N,H,W,Cout])."""
    return _conv3xk_bwd_data(_K3X5, dy_nhwc, wt_bwd)


def conv3x5_bwd_data_relu(dy_nhwc, wt_bwd, act_below, drop=None, dropped=False):
    """relu_bwd(conv3x5_bwd_data(dy, wt_bwd), act_below, drop=drop) in one launch -> bf16 (as conv3x3_bwd_data_relu)."""
    return _conv3xk_bwd_data_relu(_K3X5, dy_nhwc, wt_bwd, act_below, drop, dropped)


def conv3x5_bwd_weight_bias(x_nhwc, dy_nhwc, dw, dbias=None):
    """dw fp32 [15*Cin, Cout] view of the HWIO gradient, dbias fp32 [Cout] (both overwritten; deterministic)."""
    return _conv3xk_bwd_weight_bias(_K3X5, x_nhwc, dy_nhwc, dw, dbias)


def maxpool3x1_fwd(x_nhwc, drop=None):
    """max_pool [3,1] / [3,1] SAME over H (+ dropout of the pooled output when drop = (keep, seed, offset)) ->
    (out [N, ceil(H/3), W, C], argmax uint8)."""
    h = _h(x_nhwc)
    dt = dtype_id(x_nhwc.dtype)
    N, H, W, Cc = x_nhwc.shape
    out = torch.empty((N, (H + 2) // 3, W, Cc), dtype=x_nhwc.dtype, device=x_nhwc.device)
    arg = torch.empty(out.shape, dtype=torch.uint8, device=x_nhwc.device)
    k, sd, off = drop if drop is not None else (1.0, 0, 0)
    h.check(h.lib.asr_maxpool3x1_fwd(h.h, dt, _p(x_nhwc), N, H, W, Cc, _p(out), _p(arg), float(k), int(sd), int(off),
                                     int(drop is not None), _s()), 'asr_maxpool3x1_fwd')
    return out, arg


def maxpool3x1_bwd(dout, arg, H):
    """Gather-form backward of maxpool3x1_fwd: dout [N, ceil(H/3), W, C] -> din [N, H, W, C] (same dtype)."""
    h = _h(dout)
    N, _, W, Cc = dout.shape
    din = torch.empty((N, H, W, Cc), dtype=dout.dtype, device=dout.device)
    h.check(h.lib.asr_maxpool3x1_bwd(h.h, dtype_id(dout.dtype), _p(dout), _p(arg), N, H, W, Cc, _p(din), _s()),
            'asr_maxpool3x1_bwd')
    return din


# ---------------------------------------------------------------- student CNNs (3x4 convolutions, batch normalization)
def conv3x4_prep_weights(w_hwio):
    """fp32 [3,4,Cin,Cout] -> (wt_fwd bf16 [Cout, 12*Cin], wt_bwd bf16 [Cin, 12*Cout]: the flipped-tap image)."""
    return _conv3xk_prep_weights(_K3X4, w_hwio)


def conv3x4_fwd(x_nhwc, wt_fwd, bias, relu=True, out_dtype=ASR_BF16):
    """relu?(conv3x4 SAME(x) + bias): x bf16 [N,H,W,Cin] -> [N,H,W,Cout] in out_dtype (implicit GEMM)."""
    return _conv3xk_fwd(_K3X4, x_nhwc, wt_fwd, bias, relu, None, f32_out=dtype_id(out_dtype) == ASR_F32)


def conv3x4_bwd_data(dy_nhwc, wt_bwd):
    """dx fp32 [N,H,W,Cin] = data gradient of the 3x4 convolution (dy bf16 [N,H,W,Cout])."""
    return _conv3xk_bwd_data(_K3X4, dy_nhwc, wt_bwd)


def conv3x4_bwd_weight_bias(x_nhwc, dy_nhwc, dw, dbias=None):
    """dw fp32 [12*Cin, Cout] view of the HWIO gradient, dbias fp32 [Cout] (both overwritten; deterministic)."""
    return _conv3xk_bwd_weight_bias(_K3X4, x_nhwc, dy_nhwc, dw, dbias)


def _bn_ws(M, Cc, dev):
    n = int(_lib.load().asr_bn_workspace_bytes(int(M), int(Cc)))
    return torch.empty((max(n, 4) // 4,), dtype=torch.float32, device=dev)


def bn_stats(x_nhwc, eps, momentum, avg_mean=None, avg_var=None):
    """Batch statistics of fp32 NHWC activations over all N*H*W rows -> fp32 [5, C]: mean, biased variance,
    rsqrt(var + eps), and (with the moving averages given) the pending averages avg * momentum + stat * (1 - momentum)."""
    h = _h(x_nhwc)
    _chk(x_nhwc, torch.float32, 'x')
    Cc = x_nhwc.shape[-1]
    M = x_nhwc.numel() // Cc
    stats = torch.empty((5, Cc), dtype=torch.float32, device=x_nhwc.device)
    if avg_mean is None:
        stats[3:].zero_()
    h.check(h.lib.asr_bn_stats(h.h, _p(x_nhwc), M, Cc, float(eps), float(momentum), _p(avg_mean), _p(avg_var),
                               _p(stats), _p(_bn_ws(M, Cc, x_nhwc.device)), _s()), 'asr_bn_stats')
    return stats


def bn_apply(x_nhwc, mean, var, gamma, beta, eps, pool, out_dtype):
    """tf.nn.batch_normalization(x, mean, var, beta, gamma, eps) then max_pool [3,1]/[3,1] SAME (pool=True, with its
    uint8 argmax) or the identity -> (out [N, Ho, W, C] in out_dtype, argmax or None)."""
    h = _h(x_nhwc)
    _chk(x_nhwc, torch.float32, 'x')
    N, H, W, Cc = x_nhwc.shape
    Ho = (H + 2) // 3 if pool else H
    odt = dtype_id(out_dtype)
    out = torch.empty((N, Ho, W, Cc), dtype=TORCH_DTYPE[odt], device=x_nhwc.device)
    arg = torch.empty((N, Ho, W, Cc), dtype=torch.uint8, device=x_nhwc.device) if pool else None
    h.check(h.lib.asr_bn_apply(h.h, odt, _p(x_nhwc), N, H, W, Cc, _p(mean), _p(var), _p(gamma), _p(beta), float(eps),
                               int(bool(pool)), _p(out), _p(arg), _s()), 'asr_bn_apply')
    return out, arg


def bn_bwd(dz, arg, x_nhwc, stats, gamma, dgamma, dbeta, out_dtype, relu_gate=True):
    """Backward of bn_apply (+ pool when arg is given) and of the ReLU in front of it: dz fp32 = gradient at the pooled
    output; writes dgamma = sum(dy * xhat), dbeta = sum(dy); returns dx [N,H,W,C] in out_dtype."""
    h = _h(x_nhwc)
    _chk(dz, torch.float32, 'dz')
    _chk(x_nhwc, torch.float32, 'x')
    N, H, W, Cc = x_nhwc.shape
    pool = arg is not None
    want = (N, (H + 2) // 3 if pool else H, W, Cc)
    if dz.numel() != int(np.prod(want)):
        raise ValueError('bn_bwd: dz has %d elements, expected %s' % (dz.numel(), want))
    odt = dtype_id(out_dtype)
    dx = torch.empty((N, H, W, Cc), dtype=TORCH_DTYPE[odt], device=x_nhwc.device)
    h.check(h.lib.asr_bn_bwd(h.h, odt, _p(dz), _p(arg), int(pool), _p(x_nhwc), N, H, W, Cc, _p(stats), _p(gamma),
                             int(bool(relu_gate)), _p(dgamma), _p(dbeta), _p(dx),
                             _p(_bn_ws(N * H * W, Cc, x_nhwc.device)), _s()), 'asr_bn_bwd')
    return dx


def softmax_xent_soft(logits2d, targets2d, grad_scale=1.0, want_grad=True):
    """tf.nn.softmax_cross_entropy_with_logits(labels=targets, logits) per row -> (row_loss fp32 [rows], TF's gradient
    (softmax(logits) - targets) * grad_scale or None)."""
    h = _h(logits2d)
    _chk(logits2d, torch.float32, 'logits')
    _chk(targets2d, torch.float32, 'targets')
    rows, Cc = logits2d.shape
    if tuple(targets2d.shape) != (rows, Cc):
        raise ValueError('softmax_xent_soft: targets have shape %s, logits %s' % (tuple(targets2d.shape), (rows, Cc)))
    loss = _f32((rows,), logits2d.device)
    dl = torch.empty_like(logits2d) if want_grad else None
    h.check(h.lib.asr_softmax_xent_soft(h.h, _p(logits2d), _p(targets2d), rows, Cc, float(grad_scale), _p(loss), _p(dl),
                                        _s()), 'asr_softmax_xent_soft')
    return loss, dl


# ---------------------------------------------------------------- LSTM
def lstm_prep_weights(kernel, bias, din, H, dtype, out=None):
    """kernel [Din+H,4H] fp32 (TF layout), bias [4H] -> dict(wx_il [Din,4H] dtype, bias_il [4H] fp32,
    pf, pb packed W_h fragments)."""
    h = _h(kernel)
    _chk(kernel, torch.float32, 'kernel')
    if kernel.shape != (din + H, 4 * H):
        raise ValueError('kernel must be [Din+H,4H]')
    dev, tdt = kernel.device, TORCH_DTYPE[dtype]
    if out is None:
        out = dict(wx_il=torch.empty((din, 4 * H), dtype=tdt, device=dev),
                   bias_il=torch.empty((4 * H,), dtype=torch.float32, device=dev),
                   pf=torch.empty((H * 4 * H,), dtype=tdt, device=dev),
                   pb=torch.empty((H * 4 * H,), dtype=tdt, device=dev))
    h.check(h.lib.asr_lstm_prep_weights(h.h, dtype, _p(kernel), _p(bias), din, H, _p(out['wx_il']),
                                        _p(out['bias_il']), _p(out['pf']), _p(out['pb']), _s()),
            'asr_lstm_prep_weights')
    return out


def gate_deinterleave(src, dst, H):
    """src [R,4H] fp32 interleaved columns -> dst [R,4H] gate-major (row strides honoured)."""
    h = _h(src)
    h.check(h.lib.asr_gate_deinterleave(h.h, C.c_void_p(src.data_ptr()), src.stride(0),
                                        C.c_void_p(dst.data_ptr()), dst.stride(0), src.shape[0], H, _s()),
            'asr_gate_deinterleave')
    return dst


def _ptr_table(rows):
    """ndir x 5 device pointers (kernel, bias, w_i_diag, w_f_diag, w_o_diag per direction) as a C array."""
    flat = []
    for r in rows:
        r = list(r) + [None] * (5 - len(r))
        flat.extend(t.data_ptr() if t is not None else None for t in r)
    return (C.c_void_p * len(flat))(*flat)


def _prep_layer_args(variables, din, H, dtype, ldk, out=None):
    """The checks of lstm_prep_layer and its six images (allocated here, or `out` when the caller owns them)."""
    k0 = variables[0][0]
    ndir = len(variables)
    ldk = din if ldk is None else int(ldk)
    for v in variables:
        _chk(v[0], torch.float32, 'kernel')
        if v[0].shape != (din + H, 4 * H):
            raise ValueError('kernel must be [Din+H,4H]')
    has_peep = len(variables[0]) >= 5 and variables[0][2] is not None
    dev, tdt = k0.device, TORCH_DTYPE[dtype]
    shapes = dict(wxT=((ndir * 4 * H, ldk), tdt), wx_cat=((din, ndir * 4 * H), tdt),
                  bias=((ndir * 4 * H,), torch.float32), whf=((ndir, H * 4 * H), tdt), whb=((ndir, H * 4 * H), tdt),
                  peep=((ndir, 3, H), torch.float32))
    if out is None:
        out = dict((k, torch.empty(sh, dtype=dt, device=dev)) for k, (sh, dt) in shapes.items())
        if not has_peep:
            out['peep'] = None
    else:
        for k, (sh, dt) in shapes.items():
            t = out.get(k)
            if k == 'peep' and not has_peep:
                if t is not None:
                    raise ValueError('lstm_prep_layers: out has a peephole image for a layer without peepholes')
                continue
            if t is None or tuple(t.shape) != sh or t.dtype != dt or t.device != dev or not t.is_contiguous():
                raise ValueError('lstm_prep_layers: out[%r] must be a contiguous %s tensor of shape %s on %s'
                                 % (k, dt, sh, dev))
    return ndir, ldk, out


def lstm_prep_layer(variables, din, H, dtype, ldk=None):
    """variables: per direction (kernel [Din+H,4H], bias [4H], w_i_diag, w_f_diag, w_o_diag [H] or None) fp32 views.
    One launch -> dict(wxT [ndir*4H, ldk], wx_cat [Din, ndir*4H], bias [ndir*4H] fp32, whf / whb [ndir, H*4H] packed
    W_h, peep [ndir,3,H] fp32 or None) in the operand dtype (include/asr_hip.h asr_lstm_prep_layer)."""
    h = _h(variables[0][0])
    ndir, ldk, out = _prep_layer_args(variables, din, H, dtype, ldk)
    h.check(h.lib.asr_lstm_prep_layer(h.h, dtype, ndir, _ptr_table(variables), din, ldk, H, _p(out['wxT']),
                                      _p(out['wx_cat']), _p(out['bias']), _p(out['whf']), _p(out['whb']),
                                      _p(out['peep']), _s()), 'asr_lstm_prep_layer')
    _count_prep(variables[0][0].device, per_layer=1)
    return out


_lstm_prep_layer_native = lstm_prep_layer
_prep_counts = {}      # device index (-1: host) -> [grouped, per_layer]


def _prep_key(device):
    if isinstance(device, torch.device):
        return (device.index or 0) if device.type == 'cuda' else -1
    return -1 if device in ('cpu', None) else int(device)


def _count_prep(device, grouped=0, per_layer=0):
    c = _prep_counts.setdefault(_prep_key(device), [0, 0])
    c[0] += grouped
    c[1] += per_layer


def prep_counts(device=0):
    """Weight-image launches on `device` ('cpu': the per-layer stand-ins of a host run) since the last
    reset_prep_counts: `grouped` = asr_lstm_prep_layers launches (one per lstm_prep_layers call of up to 16 layers),
    `per_layer` = asr_lstm_prep_layer launches.  Host counters: no device work, no synchronisation."""
    c = _prep_counts.get(_prep_key(device), (0, 0))
    return dict(grouped=int(c[0]), per_layer=int(c[1]))


def reset_prep_counts(device=0):
    _prep_counts.pop(_prep_key(device), None)


def lstm_prep_layers(specs, out=None):
    """lstm_prep_layer for a stack of layers in ONE launch (include/asr_hip.h asr_lstm_prep_layers).  specs: per layer a
    dict(variables, din, H, dtype, ldk=None) -- the arguments of lstm_prep_layer; one dtype for all.  Returns the list
    of dicts lstm_prep_layer would return, byte for byte; out (a list of such dicts): caller-owned images to write into.
    Non-CUDA tensors (host runs that put stand-ins into this module): lstm_prep_layer once per layer, looked up in the
    module at call time."""
    specs = list(specs)
    if out is not None and len(out) != len(specs):
        raise ValueError('lstm_prep_layers: %d output dicts for %d layers' % (len(out), len(specs)))
    if not specs:
        return []
    k0 = specs[0]['variables'][0][0]
    if not k0.is_cuda:
        per_layer = globals()['lstm_prep_layer']
        if per_layer is _lstm_prep_layer_native:
            _h(k0)      # raises: the device path has no CPU fallback
        res = []
        for i, sp in enumerate(specs):
            w = per_layer(sp['variables'], sp['din'], sp['H'], sp['dtype'], ldk=sp.get('ldk'))
            _count_prep(k0.device, per_layer=1)
            if out is not None:
                for k, t in w.items():
                    if t is not None:
                        out[i][k].copy_(t)
                w = out[i]
            res.append(w)
        return res
    h = _h(k0)
    dtype = specs[0]['dtype']
    descs = (_lib.LstmPrepDesc * len(specs))()
    res, tables = [], []
    for i, sp in enumerate(specs):
        if sp['dtype'] != dtype:
            raise ValueError('lstm_prep_layers: one operand dtype for all layers')
        if sp['variables'][0][0].device != k0.device:
            raise ValueError('lstm_prep_layers: all layers on one device')
        ndir, ldk, o = _prep_layer_args(sp['variables'], sp['din'], sp['H'], dtype, sp.get('ldk'),
                                        out[i] if out is not None else None)
        tab = _ptr_table(sp['variables'])
        tables.append(tab)
        d = descs[i]
        d.ndir, d.vars, d.Din, d.ldk, d.H = ndir, C.addressof(tab), sp['din'], ldk, sp['H']
        d.wxT, d.wx_cat, d.bias_cat = o['wxT'].data_ptr(), o['wx_cat'].data_ptr(), o['bias'].data_ptr()
        d.packed_fwd, d.packed_bwd = o['whf'].data_ptr(), o['whb'].data_ptr()
        d.peep_out = o['peep'].data_ptr() if o.get('peep') is not None else None
        res.append(o)
    h.check(h.lib.asr_lstm_prep_layers(h.h, dtype, len(specs), C.addressof(descs), _s()), 'asr_lstm_prep_layers')
    _count_prep(k0.device, grouped=(len(specs) + 15) // 16)
    return res


def lstm_grad_finish(grads, dw_il, dpeep, H):
    """dw_il [ndir, Din+H, 4H] fp32 (interleaved columns) + dpeep [ndir,7,H] -> the gradient views `grads`
    (per direction: kernel, bias, w_i_diag, w_f_diag, w_o_diag or None), TF layouts, one launch."""
    h = _h(dw_il)
    ndir, rows, _ = dw_il.shape
    has_peep = len(grads[0]) >= 5 and grads[0][2] is not None
    h.check(h.lib.asr_lstm_grad_finish(h.h, ndir, _ptr_table(grads), rows, H, _p(dw_il), _p(dpeep),
                                       1 if has_peep else 0, _s()), 'asr_lstm_grad_finish')


LSTM_UNITS = (64, 128, 192, 256, 320, 512)   # include/asr_hip.h asr_lstm_fwd


def lstm_units_supported(H):
    """Whether asr_lstm_fwd / asr_lstm_bwd take num_units = H (callers with a step-by-step alternative ask first)."""
    return int(H) in LSTM_UNITS


def lstm_fwd(xproj, wh_packed, peep, seq_len, H, ndir, dtype, forget_bias=1.0, cell_clip=0.0,
             want_final=True):
    """xproj [T,B,ndir*4H] fp32 (interleaved gate layout [T,B,ndir,H,4]).
    Returns gates, hout, cs, c_final, h_final."""
    h = _h(xproj)
    _chk(xproj, torch.float32, 'xproj')
    _chk(seq_len, torch.int32, 'seq_len')
    T, B, G = xproj.shape
    if G != ndir * 4 * H:
        raise ValueError('xproj last dim %d != ndir*4H' % G)
    dev = xproj.device
    gates = torch.empty((T, B, ndir * 4 * H), dtype=TORCH_DTYPE[dtype], device=dev)
    hout = torch.empty((T, B, ndir * H), dtype=TORCH_DTYPE[dtype], device=dev)
    cs = torch.empty((T, B, ndir * H), dtype=torch.float32, device=dev)
    cf = torch.empty((ndir, B, H), dtype=torch.float32, device=dev) if want_final else None
    hf = torch.empty((ndir, B, H), dtype=torch.float32, device=dev) if want_final else None
    h.check(h.lib.asr_lstm_fwd(h.h, dtype, T, B, H, ndir, _p(xproj), _p(wh_packed), _p(peep),
                               _p(seq_len), float(forget_bias), float(cell_clip or 0.0), _p(gates),
                               _p(hout), _p(cs), _p(cf), _p(hf), _s()), 'asr_lstm_fwd')
    return gates, hout, cs, cf, hf


def lstm_bwd(dhout, gates, cs, wh_packed_bwd, peep, seq_len, H, ndir, dtype, d_c_final=None,
             d_h_final=None, want_dpeep=True, clip_no_grad=0.0, dpeep_workspace=None):
    """clip_no_grad > 0: the forward's cell_clip, for a cell whose clamp passes no gradient (LSTMCell's
    tf.clip_by_value; LSTMBlockCell's clip is straight-through: 0).  dpeep_workspace (tests): a caller's fp32 tensor of
    (B/16)*ndir*7*H elements for the per-tile partials [tile, ndir, 7, H] (written for B > 16 only)."""
    h = _h(dhout)
    _chk(dhout, torch.float32, 'dhout')
    T, B, _ = dhout.shape
    dev = dhout.device
    dgates = torch.empty((T, B, ndir * 4 * H), dtype=TORCH_DTYPE[dtype], device=dev)
    dpeep = ws = None
    if want_dpeep:
        dpeep = torch.empty((ndir, 7, H), dtype=torch.float32, device=dev)   # 3 peephole + 4 bias rows
        ws = dpeep_workspace
        if ws is None:
            ws = torch.empty(((B // 16) * ndir * 7 * H,), dtype=torch.float32, device=dev)
        elif ws.dtype != torch.float32 or ws.numel() < (B // 16) * ndir * 7 * H or not ws.is_contiguous():
            raise ValueError('lstm_bwd: dpeep_workspace must be contiguous fp32 with (B/16)*ndir*7*H elements')
    h.check(h.lib.asr_lstm_bwd_ex(h.h, dtype, T, B, H, ndir, _p(dhout), _p(gates), _p(cs),
                                  _p(wh_packed_bwd), _p(peep), _p(seq_len), _p(d_c_final), _p(d_h_final),
                                  float(clip_no_grad or 0.0), _p(dgates), _p(dpeep), _p(ws), _s()), 'asr_lstm_bwd')
    return dgates, dpeep


def gru_fwd(xg, xc, wgh, wch, seq_len, tmax, H, ndir):
    """xg [T,B,ndir*2H], xc [T,B,ndir*H] fp32 (hoisted x-projections + biases); wgh [ndir,H,2H], wch [ndir,H,H].
    Returns dict(r, u, c, rh [T,B,ndir*H] each, hout [T,B,ndir*H], h_final [ndir,B,H])."""
    h = _h(xg)
    _chk(xg, torch.float32, 'xg')
    _chk(seq_len, torch.int32, 'seq_len')
    T, B, G = xg.shape
    if G != ndir * 2 * H or tuple(xc.shape) != (T, B, ndir * H):
        raise ValueError('gru_fwd: xg / xc shapes do not match ndir, H')
    dev = xg.device
    out = {k: torch.empty((T, B, ndir * H), dtype=torch.float32, device=dev) for k in ('r', 'u', 'c', 'hout')}
    # rh is contracted over ALL T*B rows into the candidate kernel's recurrent gradient (with dcand = 0 at padded frames):
    # the kernel skips inactive rows, so they must hold zeros, not allocator leftovers (0 * NaN = NaN)
    out['rh'] = torch.zeros((T, B, ndir * H), dtype=torch.float32, device=dev)
    hs = torch.empty((2, ndir, B, H), dtype=torch.float32, device=dev)
    h.check(h.lib.asr_gru_fwd(h.h, T, B, H, ndir, _p(xg), _p(xc), _p(wgh), _p(wch), _p(seq_len), int(tmax),
                              _p(out['r']), _p(out['u']), _p(out['c']), _p(out['rh']), _p(out['hout']), _p(hs), _s()),
            'asr_gru_fwd')
    out['h_final'] = hs[0]
    return out


def gru_bwd(dout, d_h_final, saved, wghT, wchT, seq_len, tmax, H, ndir):
    """dout [T,B,ndir*H] fp32 -> (dgate [T,B,ndir*2H], dcand [T,B,ndir*H]) pre-activation gradients."""
    h = _h(dout)
    _chk(dout, torch.float32, 'dout')
    T, B, _ = dout.shape
    dev = dout.device
    dgate = torch.empty((T, B, ndir * 2 * H), dtype=torch.float32, device=dev)
    dcand = torch.empty((T, B, ndir * H), dtype=torch.float32, device=dev)
    work = torch.empty((2, ndir, B, H), dtype=torch.float32, device=dev)
    h.check(h.lib.asr_gru_bwd(h.h, T, B, H, ndir, _p(dout), _p(d_h_final), _p(saved['hout']), _p(saved['r']),
                              _p(saved['u']), _p(saved['c']), _p(wghT), _p(wchT), _p(seq_len), int(tmax), _p(dgate),
                              _p(dcand), _p(work), _s()), 'asr_gru_bwd')
    return dgate, dcand


def check_async_errors(device=0, flush_deferred=True):
    """Device sync + sticky error word of the multi-CU LSTM kernels (raises on a hand-off timeout).
    The blocking form: call at sync points (evaluation, checkpoint, end of an epoch)."""
    h = _lib.handle(device)
    flags = C.c_uint(0)
    rc = h.lib.asr_check_async_errors(h.h, C.byref(flags))
    dkey = device.index or 0 if isinstance(device, torch.device) else int(device)
    for (d, lane), h2 in list(_lib._handles.items()):
        # recurrences also run on the second pipeline's lane (models/encoders/core/blstm.py PIPE_LANE): its handle has
        # its own exchange areas and its own error word
        if d == dkey and lane == WATCHED_SIDE_LANE:
            f2 = C.c_uint(0)
            rc2 = h2.lib.asr_check_async_errors(h2.h, C.byref(f2))
            if f2.value:
                h2.lib.asr_clear_async_errors(h2.h, _s())
                flags.value |= f2.value
                rc = rc or rc2
                h = h2 if rc2 else h
    if flags.value:
        h0 = _lib.handle(device)
        h0.lib.asr_clear_async_errors(h0.h, _s())     # sticky until reported once
        # ... and once only: the non-blocking watch may still hold copies of the same word armed before this point (the
        # device has been drained, they have all landed); left in its ring they would raise the error a second time up to
        # DEPTH optimizer steps later -- after the caller has restored its checkpoint
        w = _watches.get(device.index or 0 if isinstance(device, torch.device) else int(device))
        if w is not None:
            w.events = [None] * w.DEPTH
    h.check(rc, 'asr_check_async_errors')
    if flush_deferred:
        _deferred_for(device).flush()                # the device is idle: every counter armed on it has landed
    return flags.value


WATCHED_SIDE_LANE = 6     # == blstm.PIPE_LANE: the one side lane recurrence kernels are issued on


class ErrorWatch(object):
    """Non-blocking watch on the sticky error word of the cluster recurrence kernels.

    poll() is called once per optimizer step (models/model_base.py Optimizer.apply_gradients): it enqueues a 4-byte
    device->host copy of the word behind the step's kernels and inspects the copy armed DEPTH polls earlier (its event
    has long completed, so the host never stalls in steady state).  A hand-off timeout therefore raises AsrError at
    most DEPTH steps after it happened instead of silently corrupting the weights."""
    DEPTH = 3

    def __init__(self, device):
        self.dev = device
        self.host = torch.zeros(2 * self.DEPTH, dtype=torch.int32).pin_memory()   # [slot] main handle, [DEPTH + slot] side lane's
        self.events = [None] * self.DEPTH
        self.i = 0
        self.waited_s = 0.0   # host time spent blocked on a step armed DEPTH polls ago (bench.py subtracts it)

    def poll(self):
        slot = self.i % self.DEPTH
        ev = self.events[slot]
        if ev is not None:
            if not ev.query():
                # the host is DEPTH steps ahead of the device: this wait is the throttle of the issue loop, not issue work
                t0 = _time.perf_counter()
                ev.synchronize()
                self.waited_s += _time.perf_counter() - t0
            flags = int(self.host[slot]) | int(self.host[self.DEPTH + slot])
            if flags:
                h = _lib.handle(self.dev)
                h.lib.asr_clear_async_errors(h.h, _s())
                h2 = _lib._handles.get((self.dev, WATCHED_SIDE_LANE))
                if h2 is not None:
                    h2.lib.asr_clear_async_errors(h2.h, _s())
                self.events = [None] * self.DEPTH
                if flags & 3:
                    raise _lib.AsrError('LSTM cluster hand-off timed out (flags 0x%x): the recurrent state of a recent '
                                        'step is garbage -- restore the last checkpoint' % flags)
                # not a hand-off fault: the MODEL diverged.  The reference would carry a NaN loss on (and its learning-rate
                # controller / early stop would react); the bf16 cluster exchange cannot represent a non-finite h (its tag
                # bits would launder it into a finite value for the peers), so this path stops instead (INTEGRATION.md,
                # "Deviations"; bf16 self-tagged exchange only -- the fp32 paths propagate NaN like the reference)
                raise _lib.AsrError('LSTM recurrence produced a non-finite hidden state (flags 0x%x): the model diverged '
                                    '(learning rate / clipping); weights of the last %d steps are NaN-contaminated'
                                    % (flags, self.DEPTH))
        h = _lib.handle(self.dev)
        h.check(h.lib.asr_peek_async_errors(h.h, C.c_void_p(self.host.data_ptr() + 4 * slot), _s()),
                'asr_peek_async_errors')
        self.host[self.DEPTH + slot] = 0
        h2 = _lib._handles.get((self.dev, WATCHED_SIDE_LANE))
        if h2 is not None:       # the second pipeline's handle (its work has been joined into this stream by now)
            h2.check(h2.lib.asr_peek_async_errors(h2.h, C.c_void_p(self.host.data_ptr() + 4 * (self.DEPTH + slot)), _s()),
                     'asr_peek_async_errors')
        ev = torch.cuda.Event()
        ev.record(_cur_stream())
        self.events[slot] = ev
        self.i += 1


_watches = {}


class DeferredCheck(object):
    """A device-side counter that must be zero (tf.nn.ctc_loss's "Not enough time for target transition sequence"
    InvalidArgumentError, ctc.py:289 with ignore_longer_outputs_than_inputs=False), checked WITHOUT stalling the training
    step: arm() copies the counter to pinned memory behind the step's kernels -- on the counter's OWN device and that
    device's current stream (one DeferredCheck per device) -- and every earlier copy that has landed is inspected then.
    Lateness: the reference raises inside the sess.run of the offending step; here the error surfaces at a later arm() --
    in steady state within ErrorWatch.DEPTH (3) optimizer steps, because that is how far the issue loop may run ahead of
    the device, and NEVER more than DEPTH (4) optimizer STEPS late, however many CTC heads arm a counter per step
    (MultitaskCTC arms two): a copy armed DEPTH steps ago is waited for (the device's ErrorWatch counts the steps:
    note_step()); without optimizer steps in between (a loop of compute_loss calls) at most RING - 1 copies are pending.
    The optimizer has applied the updates of the steps in between.  An error DROPS every other pending copy (another
    head's, the later steps' -- which ran on the state the failing step left and would only repeat the report while the
    caller restores its checkpoint): one exception per incident.  flush() is the blocking form; it runs at every sync point: evaluation (is_training=False), Saver.save / check_async_errors (checkpoints), the
    end of the recipes' epochs, and at interpreter exit (a pending error is printed, it cannot be raised any more)."""
    DEPTH = 4          # optimizer steps
    RING = 16          # pinned slots: >= DEPTH x the heads of any model here, and the cap when no optimizer steps run

    def __init__(self, device=None):
        self.device = device
        self.slots = []          # (pinned host tensor, event, exception factory, step it was armed in)
        self.waited_s = 0.0
        self.ring = None
        self.n = 0
        self.step = 0

    def note_step(self):
        """One optimizer step has been issued on this device (watch_async_errors)."""
        self.step += 1

    def _inspect(self, host, ev, make_exc, step, block):
        if not ev.query():
            if not block:
                return False
            t0 = _time.perf_counter()
            ev.synchronize()
            self.waited_s += _time.perf_counter() - t0
        n = int(host[0])
        if n:
            self.slots = []
            # a timed-out cluster hand-off leaves NaN activations, which the CTC kernels count as infeasible rows: report the
            # root cause (AsrError from the sticky error word) rather than its symptom
            check_async_errors(self.device if self.device is not None else torch.cuda.current_device(), flush_deferred=False)
            raise make_exc(n)
        return True

    def arm(self, counter, make_exc):
        if self.ring is None:        # one pinned block for the life of the process: no pinned allocation per step
            self.ring = torch.zeros(self.RING, dtype=torch.int32).pin_memory()
        self.n += 1
        host = self.ring[self.n % self.RING:][:1]
        host.copy_(counter.view(-1)[:1].to(torch.int32), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(_cur_stream(counter.device))       # the stream the copy was enqueued on: the counter's device
        self.slots.append((host, ev, make_exc, self.step))
        while self.slots:
            block = self.step - self.slots[0][3] >= self.DEPTH or len(self.slots) >= self.RING - 1
            if not self._inspect(*self.slots[0], block=block):
                break
            self.slots.pop(0)

    def flush(self):
        while self.slots:
            slot = self.slots.pop(0)
            self._inspect(*slot, block=True)


_deferred_by_dev = {}


def _deferred_for(device):
    d = device.index if isinstance(device, torch.device) else device
    d = torch.cuda.current_device() if d is None else int(d)
    w = _deferred_by_dev.get(d)
    if w is None:
        w = _deferred_by_dev[d] = DeferredCheck(d)
    return w


def defer_zero_check(counter, make_exc, blocking=False):
    """counter: device int tensor that must be 0; make_exc(n) builds the exception.  blocking=True checks now."""
    if not counter.is_cuda:
        if int(counter.view(-1)[0]):
            raise make_exc(int(counter.view(-1)[0]))
        return
    w = _deferred_for(counter.device)
    with torch.cuda.device(counter.device):
        w.arm(counter, make_exc)
        if blocking:
            w.flush()


def flush_deferred_checks():
    """Blocking inspection of every armed counter on every device (end of an epoch / of training)."""
    for w in list(_deferred_by_dev.values()):
        w.flush()


def _flush_deferred_at_exit():
    try:
        flush_deferred_checks()
    except Exception as e:       # too late to raise into the training loop: say so
        import sys
        sys.stderr.write('tensorflow_end2end_speech_recognition_amd: an error of one of the LAST training steps was still '
                         'pending at exit: %r\n' % (e,))


import atexit as _atexit      # noqa: E402
_atexit.register(_flush_deferred_at_exit)


def watch_waited_seconds(device=0):
    """Cumulative host time the device's ErrorWatch spent blocked behind the GPU (0 if none exists yet)."""
    w = _watches.get(device.index or 0 if isinstance(device, torch.device) else int(device))
    return (w.waited_s if w is not None else 0.0) + sum(d.waited_s for d in _deferred_by_dev.values())


def watch_async_errors(device):
    """One ErrorWatch per device; see ErrorWatch.poll."""
    dev = device.index or 0 if isinstance(device, torch.device) else int(device)
    w = _watches.get(dev)
    if w is None:
        w = _watches[dev] = ErrorWatch(dev)
    d = _deferred_by_dev.get(dev)
    if d is not None:
        d.note_step()
    w.poll()


def debug_set_lstm_flags(flags):
    """ASR_LSTM_DFLAGS at run time (tests): 16 = write-through exchange, 64 = force hand-off timeouts."""
    _lib.load().asr_debug_set_lstm_flags(int(flags))


def debug_set_gru_persistent(on):
    """asr_debug_set_gru_persistent: 1 = one persistent launch per GRU layer call (default), 0 = launch per step."""
    _lib.load().asr_debug_set_gru_persistent(int(bool(on)))


def debug_set_cluster_cu_budget(n):
    """TEST ONLY: co-resident workgroups a cluster launch may use (0 = the device's CU count; never more than that)."""
    _lib.load().asr_debug_set_cluster_cu_budget(int(n))


def cluster_tile_groups(G, ndir, tiles, cu_budget):
    """asr_cluster_tile_groups: the [(first_tile, ntiles), ...] launches of a cluster recurrence with G workgroups per
    cluster over `tiles` 16-utterance tiles when at most cu_budget workgroups are resident at once; [] = no plan.
    Host arithmetic only (no GPU)."""
    lib = _lib.load()
    first, cnt = (C.c_int * max(int(tiles), 1))(), (C.c_int * max(int(tiles), 1))()
    n = lib.asr_cluster_tile_groups(int(G), int(ndir), int(tiles), int(cu_budget), first, cnt, max(int(tiles), 1))
    if n < 0:
        raise ValueError('asr_cluster_tile_groups: bad arguments')
    return [(first[i], cnt[i]) for i in range(n)]


# ---------------------------------------------------------------- launch counters
# Every native kernel family counts on its handle which path its calls took (plain host integers: no device work, no
# synchronisation).  _counters holds the table of families, keys and public views; the views are built here.
def _device_handles(device):
    dev = device.index or 0 if isinstance(device, torch.device) else int(device)
    _lib.handle(dev)
    return [h for (d, _lane), h in list(_lib._handles.items()) if d == dev]


def _read_counts(family, device):
    """The words of _counters.FAMILIES[family], summed over the handles of `device`: one native call per handle."""
    fam = _counters.FAMILIES[family]
    n = len(fam.keys)
    tot = [0] * n
    for h in _device_handles(device):
        out = (C.c_ulonglong * n)()
        get = getattr(h.lib, fam.getter)
        h.check(get(h.h, out, n) if fam.sized else get(h.h, out), fam.getter)
        tot = [a + int(b) for a, b in zip(tot, out)]
    return tot


def _reset_counts(family, device):
    fam = _counters.FAMILIES[family]
    for h in _device_handles(device):
        h.check(getattr(h.lib, fam.reset)(h.h), fam.reset)


def _counter_fns(name):
    """(counts, reset) of the public view `name` of _counters.VIEWS, each taking (device=0): counts returns the view's keys
    in table order; reset zeroes the view's whole family, and is None for a view that shares another view's reset."""
    view = _counters.VIEWS[name]
    end = view.offset + len(view.keys)

    def counts(device=0):
        return dict(zip(view.keys, _read_counts(view.family, device)[view.offset:end]))

    def reset(device=0):
        _reset_counts(view.family, device)

    counts.__name__ = counts.__qualname__ = view.name
    counts.__doc__ = view.doc
    if view.reset is None:
        return counts, None
    reset.__name__ = reset.__qualname__ = view.reset
    return counts, reset


recurrence_path_counts, reset_recurrence_path_counts = _counter_fns('recurrence_path_counts')
gru_kernel_counts, reset_gru_kernel_counts = _counter_fns('gru_kernel_counts')
lstm_kernel_counts, reset_lstm_kernel_counts = _counter_fns('lstm_kernel_counts')
att_path_counts, reset_att_path_counts = _counter_fns('att_path_counts')
conv_path_counts, reset_conv_path_counts = _counter_fns('conv_path_counts')
gemm_path_counts, reset_gemm_path_counts = _counter_fns('gemm_path_counts')
tn_frames_path_counts = _counter_fns('tn_frames_path_counts')[0]       # these three: reset_gemm_path_counts
ctc_head_bwd_counts = _counter_fns('ctc_head_bwd_counts')[0]
gemm_kernel_counts = _counter_fns('gemm_kernel_counts')[0]
ctc_head_counts, reset_ctc_head_counts = _counter_fns('ctc_head_counts')
ctc_ls_counts, reset_ctc_ls_counts = _counter_fns('ctc_ls_counts')
att_beam_counts, reset_att_beam_counts = _counter_fns('att_beam_counts')
att_joint_counts, reset_att_joint_counts = _counter_fns('att_joint_counts')
att_gru_counts, reset_att_gru_counts = _counter_fns('att_gru_counts')
att_stack_counts, reset_att_stack_counts = _counter_fns('att_stack_counts')
att_lm_counts, reset_att_lm_counts = _counter_fns('att_lm_counts')
ctc_beam_lm_counts, reset_ctc_beam_lm_counts = _counter_fns('ctc_beam_lm_counts')
weight_noise_counts, reset_weight_noise_counts = _counter_fns('weight_noise_counts')
input_augment_counts, reset_input_augment_counts = _counter_fns('input_augment_counts')


# ---------------------------------------------------------------- CTC
def ctc_loss(logits, labels_flat, label_offsets, seq_len, max_label_len, grad_scale=1.0,
             want_grad=True):
    """logits [T,B,C] fp32; returns (loss [B], grad [T,B,C] or None, num_infeasible [1] int32)."""
    h = _h(logits)
    _chk(logits, torch.float32, 'logits')
    _chk(labels_flat, torch.int32, 'labels_flat')
    _chk(label_offsets, torch.int32, 'label_offsets')
    _chk(seq_len, torch.int32, 'seq_len')
    T, B, Cc = logits.shape
    dev = logits.device
    nbytes = h.lib.asr_ctc_workspace_bytes(T, B, int(max_label_len))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    loss = torch.empty((B,), dtype=torch.float32, device=dev)
    grad = torch.empty_like(logits) if want_grad else None
    ninf = torch.empty((1,), dtype=torch.int32, device=dev)     # zeroed by the call
    h.check(h.lib.asr_ctc_loss(h.h, _p(logits), T, B, Cc, _p(labels_flat), _p(label_offsets),
                               _p(seq_len), int(max_label_len), float(grad_scale), _p(loss), _p(grad),
                               _p(ninf), _p(ws), nbytes, _s()), 'asr_ctc_loss')
    return loss, grad, ninf


def ctc_head_ok(rows, E, Cc):
    """Whether ctc_head_fwd takes a [rows, E] x [E, Cc] head (asr_ctc_head_ok): bf16 operands, E % 64 == 0, Cc <= 64, and
    a logits product that ops.gemm runs in one pass over E."""
    return bool(_lib.load().asr_ctc_head_ok(int(rows), int(E), int(Cc)))


def ctc_head_prep(W, out=None):
    """Operand images of a CTC head's weights W [E, Cc] fp32 (asr_ctc_head_prep): (Wt [64, E] bf16 class-major for
    ctc_head_fwd, or None for Cc > 64; Wp [E, Kp] bf16, Kp = Cc rounded up to 64, columns >= Cc zero, for the product
    dlogits W^T on ctc_loss_ex's bf16 image)."""
    h = _h(W)
    _chk(W, torch.float32, 'W')
    E, Cc = W.shape
    Kp = (Cc + 63) // 64 * 64
    if out is not None:
        Wt, Wp = out
        if (Cc <= 64 and (Wt is None or Wt.shape != (64, E) or Wt.dtype != torch.bfloat16)) or Wp.shape != (E, Kp) \
                or Wp.dtype != torch.bfloat16:
            raise ValueError('ctc_head_prep: bad out images for W %s' % (tuple(W.shape),))
    else:
        Wt = torch.empty((64, E), dtype=torch.bfloat16, device=W.device) if Cc <= 64 else None
        Wp = torch.empty((E, Kp), dtype=torch.bfloat16, device=W.device)
    h.check(h.lib.asr_ctc_head_prep(h.h, _p(W), E, Cc, _p(Wt), _p(Wp), _s()), 'asr_ctc_head_prep')
    return Wt, Wp


def ctc_workspace(T, B, max_label_len, device):
    nbytes = _lib.load().asr_ctc_workspace_bytes(int(T), int(B), int(max_label_len))
    return torch.empty((nbytes,), dtype=torch.uint8, device=device)


def ctc_head_fwd(hout, drop, Wt, bias, Cc, labels_flat, label_offsets, seq_len, max_label_len, ws):
    """The CTC head's forward in one launch (asr_ctc_head_fwd).  hout [T,B,E] bf16: the top layer's output BEFORE its
    dropout; drop = (keep_prob, seed, offset) or None.  Returns (x_op [T,B,E] bf16 -- dropout_apply(hout, *drop), or hout
    itself without dropout --, logits [T,B,Cc] fp32, num_infeasible [1] int32, cleared); `ws` (ctc_workspace) then holds
    what ctc_loss_ex(lse_done=True) continues from."""
    h = _h(hout)
    _chk(hout, torch.bfloat16, 'hout')
    _chk(Wt, torch.bfloat16, 'Wt')
    _chk(bias, torch.float32, 'bias')
    T, B, E = hout.shape
    if Wt.shape != (64, E) or bias.numel() != Cc:
        raise ValueError('ctc_head_fwd: weight image %s / bias %d for E = %d, C = %d' % (tuple(Wt.shape), bias.numel(), E, Cc))
    dev = hout.device
    x_op = torch.empty_like(hout) if drop is not None else hout
    logits = torch.empty((T, B, Cc), dtype=torch.float32, device=dev)
    ninf = torch.empty((1,), dtype=torch.int32, device=dev)     # zeroed by the call
    keep, seed, off = (float(drop[0]), int(drop[1]), int(drop[2])) if drop is not None else (0.0, 0, 0)
    h.check(h.lib.asr_ctc_head_fwd(h.h, _p(hout), T, B, E, keep, seed, off, _p(Wt), _p(bias), int(Cc), _p(labels_flat),
                                   _p(label_offsets), _p(seq_len), int(max_label_len),
                                   _p(x_op) if drop is not None else None, _p(logits), _p(ninf), _p(ws), ws.numel(), _s()),
            'asr_ctc_head_fwd')
    return x_op, logits, ninf


def ctc_head_bwd(img, Wp, out, drop=None, rows=None):
    """d(encoder output) of a CTC head into `out` [M,E] fp32 (asr_ctc_head_bwd): img [M,Kp] bf16 (ctc_loss_ex's image of
    dlogits) x Wp [E,Kp]^T (ctc_head_prep), times the dropout mask drop = (keep_prob, seed, offset) of the top layer in
    the epilogue.  rows = (int32 device vector, count): only the listed rows have to be right, as for gemm(rows=...)."""
    h = _h(img)
    _chk(img, torch.bfloat16, 'img')
    _chk(Wp, torch.bfloat16, 'Wp')
    _chk(out, torch.float32, 'out')
    M, Kp = img.shape
    E = Wp.shape[0]
    if Wp.shape != (E, Kp) or out.shape != (M, E) or E % 4:
        raise ValueError('ctc_head_bwd: img %s, Wp %s, out %s' % (tuple(img.shape), tuple(Wp.shape), tuple(out.shape)))
    rt, nr = (rows[0], int(rows[1])) if rows is not None else (None, 0)
    if rt is not None:
        _chk(rt, torch.int32, 'rows')
        if rt.dim() != 1 or not 0 <= nr <= min(rt.numel(), M):
            raise ValueError('ctc_head_bwd: bad row list')
    keep, seed, off = (float(drop[0]), int(drop[1]), int(drop[2])) if drop is not None else (0.0, 0, 0)
    h.check(h.lib.asr_ctc_head_bwd(h.h, M, E, Kp, _p(img), _p(Wp), _p(out), keep, seed, off, _p(rt), nr, _s()),
            'asr_ctc_head_bwd')
    return out


def ctc_loss_ex(logits, labels_flat, label_offsets, seq_len, max_label_len, grad_scale=1.0, ws=None, ninf=None,
                lse_done=False, want_image=True):
    """ctc_loss through asr_ctc_loss_ex: continues from ctc_head_fwd's workspace (lse_done) and also returns the bf16
    image [T*B, Kp] of the gradient (Kp = C rounded up to 64, zero columns behind C).
    Returns (loss [B], grad [T,B,C] fp32, grad image or None, num_infeasible)."""
    h = _h(logits)
    _chk(logits, torch.float32, 'logits')
    T, B, Cc = logits.shape
    dev = logits.device
    if ws is None:
        if lse_done:
            raise ValueError('ctc_loss_ex: lse_done needs the workspace of ctc_head_fwd')
        ws = ctc_workspace(T, B, max_label_len, dev)
    if ninf is None:
        ninf = torch.empty((1,), dtype=torch.int32, device=dev)
    loss = torch.empty((B,), dtype=torch.float32, device=dev)
    grad = torch.empty_like(logits)
    Kp = (Cc + 63) // 64 * 64
    img = torch.empty((T * B, Kp), dtype=torch.bfloat16, device=dev) if want_image else None
    h.check(h.lib.asr_ctc_loss_ex(h.h, _p(logits), T, B, Cc, _p(labels_flat), _p(label_offsets), _p(seq_len),
                                  int(max_label_len), float(grad_scale), _p(loss), _p(grad), _p(ninf), _p(ws),
                                  ws.numel(), 1 if lse_done else 0, _p(img), Kp if want_image else 0, _s()),
            'asr_ctc_loss_ex')
    return loss, grad, img, ninf


def ctc_ls_workspace(T, B, max_label_len, device):
    """The workspace of ctc_loss_ls (asr_ctc_ls_workspace_bytes): ctc_workspace's layout and behind it the KL row terms,
    so ctc_head_fwd can fill it for ctc_loss_ls(lse_done=True)."""
    nbytes = _lib.load().asr_ctc_ls_workspace_bytes(int(T), int(B), int(max_label_len))
    return torch.empty((nbytes,), dtype=torch.uint8, device=device)


def ctc_loss_ls(logits, labels_flat, label_offsets, seq_len, max_label_len, smoothing, grad_scale=1.0, ws=None, ninf=None,
                lse_done=False, want_grad=True, want_image=False):
    """EXTENSION: CTC loss with label smoothing towards the uniform distribution over all classes (asr_ctc_loss_ls).
    Returns (loss [B] -- the UNSMOOTHED CTC loss, ctc_loss's bits --, kl [B] = sum_t KL(uniform || softmax(logits[t,b])),
    grad [T,B,C] = grad_scale * d((1 - smoothing) loss + smoothing kl) / d logits or None, its bf16 image [T*B, Kp] or None,
    num_infeasible).  0 < smoothing < 1; finite logits; ws: ctc_ls_workspace (needed with lse_done, after ctc_head_fwd)."""
    eps = float(smoothing)
    if not 0.0 < eps < 1.0:
        raise ValueError('ctc_loss_ls: smoothing must be in (0, 1), got %r' % (smoothing,))
    if want_image and not want_grad:
        raise ValueError('ctc_loss_ls: the image is the image of the gradient (want_grad)')
    h = _h(logits)
    _chk(logits, torch.float32, 'logits')
    _chk(labels_flat, torch.int32, 'labels_flat')
    _chk(label_offsets, torch.int32, 'label_offsets')
    _chk(seq_len, torch.int32, 'seq_len')
    T, B, Cc = logits.shape
    dev = logits.device
    if ws is None:
        if lse_done:
            raise ValueError('ctc_loss_ls: lse_done needs the workspace of ctc_head_fwd (ctc_ls_workspace)')
        ws = ctc_ls_workspace(T, B, max_label_len, dev)
    if ninf is None:
        ninf = torch.empty((1,), dtype=torch.int32, device=dev)
    loss = torch.empty((B,), dtype=torch.float32, device=dev)
    kl = torch.empty((B,), dtype=torch.float32, device=dev)
    grad = torch.empty_like(logits) if want_grad else None
    Kp = (Cc + 63) // 64 * 64
    img = torch.empty((T * B, Kp), dtype=torch.bfloat16, device=dev) if want_image else None
    h.check(h.lib.asr_ctc_loss_ls(h.h, _p(logits), T, B, Cc, _p(labels_flat), _p(label_offsets), _p(seq_len),
                                  int(max_label_len), float(grad_scale), eps, _p(loss), _p(kl), _p(grad), _p(ninf),
                                  _p(ws), ws.numel(), 1 if lse_done else 0, _p(img), Kp if want_image else 0, _s()),
            'asr_ctc_loss_ls')
    return loss, kl, grad, img, ninf


def ctc_greedy_decode(logits, seq_len, blank=None):
    h = _h(logits)
    _chk(logits, torch.float32, 'logits')
    _chk(seq_len, torch.int32, 'seq_len')
    T, B, Cc = logits.shape
    if blank is None:
        blank = Cc - 1
    out = torch.empty((B, T), dtype=torch.int32, device=logits.device)
    n = torch.empty((B,), dtype=torch.int32, device=logits.device)
    h.check(h.lib.asr_ctc_greedy_decode(h.h, _p(logits), T, B, Cc, _p(seq_len), int(blank), _p(out),
                                        _p(n), _s()), 'asr_ctc_greedy_decode')
    return out, n


def ctc_beam_decode(logits, seq_len, beam_width, blank=None):
    """Prefix beam search.  logits [T,B,C] fp32 -> (labels [B,T] int32 padded -1, lengths [B],
    scores [B] float64 = -log p of the best prefix)."""
    h = _h(logits)
    _chk(logits, torch.float32, 'logits')
    _chk(seq_len, torch.int32, 'seq_len')
    T, B, Cc = logits.shape
    if blank is None:
        blank = Cc - 1
    dev = logits.device
    nbytes = h.lib.asr_ctc_beam_workspace_bytes(T, B, Cc, int(beam_width))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    out = torch.empty((B, T), dtype=torch.int32, device=dev)
    n = torch.empty((B,), dtype=torch.int32, device=dev)
    score = torch.empty((B,), dtype=torch.float64, device=dev)
    h.check(h.lib.asr_ctc_beam_decode(h.h, _p(logits), T, B, Cc, _p(seq_len), int(blank), int(beam_width),
                                      _p(out), _p(n), _p(score), _p(ws), nbytes, _s()), 'asr_ctc_beam_decode')
    return out, n, score


def softmax_rows(x2d):
    h = _h(x2d)
    _chk(x2d, torch.float32, 'x')
    out = torch.empty_like(x2d)
    h.check(h.lib.asr_softmax_rows(h.h, _p(x2d), _p(out), x2d.shape[0], x2d.shape[1], _s()),
            'asr_softmax_rows')
    return out


# ---------------------------------------------------------------- attention decoder
def _f32(shape, dev):
    return torch.empty(shape, dtype=torch.float32, device=dev)


def _col_block(t, B, W, name):
    """(pointer, row stride) of a [B, W] column block of a row-major array (unit inner stride)."""
    if t is None:
        return None, 0
    if t.dim() != 2 or tuple(t.shape) != (B, W) or t.stride(1) != 1 or t.dtype != torch.float32:
        raise ValueError('%s must be an fp32 [B,%d] column block with unit inner stride' % (name, W))
    return C.c_void_p(t.data_ptr()), t.stride(0)


def lstm_cell_fwd(pre, c_prev, h_prev, peep, live, forget_bias=1.0, cell_clip=0.0, out_mask=None, want_cell_out=False,
                  h_also=None, cell_out_also=None):
    """One decoder cell step.  Returns (gates, c_raw, c_out, h_out, h_raw) -- plus cell_out = h_raw * out_mask as a
    sixth element when want_cell_out.  h_also / cell_out_also: [B,U] column blocks of wider arrays (the next step's
    cell input, the attentional vector's input) that receive h_out / cell_out as well, inside the same launch."""
    h = _h(pre)
    B, U4 = pre.shape
    U = U4 // 4
    dev = pre.device
    gates, c_raw, c_out, h_out, h_raw = _f32((B, U4), dev), _f32((B, U), dev), _f32((B, U), dev), \
        _f32((B, U), dev), _f32((B, U), dev)
    cell_out = _f32((B, U), dev) if want_cell_out else None
    hp, hld = _col_block(h_also, B, U, 'h_also')
    cp, cld = _col_block(cell_out_also, B, U, 'cell_out_also')
    h.check(h.lib.asr_lstm_cell_fwd_ex(h.h, _p(pre), _p(c_prev), _p(h_prev), _p(peep), _p(live), B, U,
                                       float(forget_bias), float(cell_clip or 0.0), _p(gates), _p(c_raw), _p(c_out),
                                       _p(h_out), _p(h_raw), _p(out_mask), _p(cell_out), hp, hld, cp, cld, _s()),
            'asr_lstm_cell_fwd')
    if want_cell_out:
        return gates, c_raw, c_out, h_out, h_raw, cell_out
    return gates, c_raw, c_out, h_out, h_raw


def lstm_cell_gemm_prep(W, bias):
    """Gate-interleaved image [(K + 1), 4U] of a decoder cell's kernel [K,4U] and bias [4U] (asr_lstm_cell_gemm_prep)."""
    h = _h(W)
    K, U4 = W.shape
    out = _f32(((K + (1 if bias is not None else 0)), U4), W.device)
    h.check(h.lib.asr_lstm_cell_gemm_prep(h.h, _p(W), _p(bias), K, U4 // 4, _p(out), _s()), 'asr_lstm_cell_gemm_prep')
    return out


def lstm_cell_gemm_fwd(x, W_il, has_bias, c_prev, h_prev, peep, live, forget_bias=1.0, cell_clip=0.0, out_mask=None,
                       h_also=None, cell_out_also=None):
    """lstm_cell_fwd(gemm(x, W) + b, ...) as one launch on the interleaved image; x [B,K] (a row block of a wider array is
    fine).  Returns (gates, c_raw, c_out, h_out, h_raw, cell_out)."""
    h = _h(x)
    B, K = x.shape
    U = W_il.shape[1] // 4
    dev = x.device
    gates, c_raw, c_out, h_out, h_raw, cell_out = _f32((B, 4 * U), dev), _f32((B, U), dev), _f32((B, U), dev), \
        _f32((B, U), dev), _f32((B, U), dev), _f32((B, U), dev)
    hp, hld = _col_block(h_also, B, U, 'h_also')
    cp, cld = _col_block(cell_out_also, B, U, 'cell_out_also')
    if x.dtype != torch.float32 or x.stride(1) != 1:
        raise ValueError('lstm_cell_gemm_fwd: x must be fp32 with unit inner stride')
    h.check(h.lib.asr_lstm_cell_gemm_fwd(h.h, C.c_void_p(x.data_ptr()), int(x.stride(0)), K, _p(W_il), int(bool(has_bias)), _p(c_prev), _p(h_prev),
                                         _p(peep), _p(live), B, U, float(forget_bias), float(cell_clip or 0.0), _p(gates),
                                         _p(c_raw), _p(c_out), _p(h_out), _p(h_raw), _p(out_mask), _p(cell_out), hp, hld, cp,
                                         cld, _s()), 'asr_lstm_cell_gemm_fwd')
    return gates, c_raw, c_out, h_out, h_raw, cell_out


def lstm_cell_gemm_prep_h(W, bias):
    """The bf16 images of a decoder cell's kernel [K,4U] (+ bias) for lstm_cell_gemm_fwd_h / _bwd_h: one opaque buffer."""
    h = _h(W)
    K, U4 = W.shape
    nbytes = int(h.lib.asr_lstm_cell_gemm_h_bytes(K, U4 // 4))
    img = torch.empty((nbytes // 4,), dtype=torch.float32, device=W.device)
    h.check(h.lib.asr_lstm_cell_gemm_prep_h(h.h, _p(W), _p(bias), K, U4 // 4, _p(img), _s()), 'asr_lstm_cell_gemm_prep_h')
    return img


def lstm_cell_gemm_fwd_h(x, img, U, c_prev, h_prev, peep, live, forget_bias=1.0, cell_clip=0.0, out_mask=None,
                         h_also=None, cell_out_also=None):
    """lstm_cell_gemm_fwd with bf16 weights (the image of lstm_cell_gemm_prep_h)."""
    h = _h(x)
    B, K = x.shape
    dev = x.device
    if x.dtype != torch.float32 or x.stride(1) != 1:
        raise ValueError('lstm_cell_gemm_fwd_h: x must be fp32 with unit inner stride')
    gates, c_raw, c_out, h_out, h_raw, cell_out = _f32((B, 4 * U), dev), _f32((B, U), dev), _f32((B, U), dev), \
        _f32((B, U), dev), _f32((B, U), dev), _f32((B, U), dev)
    hp, hld = _col_block(h_also, B, U, 'h_also')
    cp, cld = _col_block(cell_out_also, B, U, 'cell_out_also')
    h.check(h.lib.asr_lstm_cell_gemm_fwd_h(h.h, C.c_void_p(x.data_ptr()), int(x.stride(0)), K, _p(img), _p(c_prev), _p(h_prev),
                                           _p(peep), _p(live), B, U, float(forget_bias), float(cell_clip or 0.0), _p(gates),
                                           _p(c_raw), _p(c_out), _p(h_out), _p(h_raw), _p(out_mask), _p(cell_out), hp, hld,
                                           cp, cld, _s()), 'asr_lstm_cell_gemm_fwd_h')
    return gates, c_raw, c_out, h_out, h_raw, cell_out


def lstm_cell_gemm_bwd_h(dpre, img, K):
    """dx [B,K] = dpre [B,4U] W^T on the bf16 copy of W inside the image."""
    h = _h(dpre)
    B, U4 = dpre.shape
    dx = _f32((B, K), dpre.device)
    h.check(h.lib.asr_lstm_cell_gemm_bwd_h(h.h, _p(dpre), B, K, U4 // 4, _p(img), _p(dx), K, _s()), 'asr_lstm_cell_gemm_bwd_h')
    return dx


def lstm_cell_bwd(dh_use, dc_next, dh_next, gates, c_raw, c_prev, peep, live, want_dpeep=True, dpre_out=None,
                  dpeep_out=None, cell_clip=0.0):
    """dpre_out [B,4U] / dpeep_out [B,3U] (contiguous rows of the caller's per-step arrays): written in place.
    cell_clip: the clip the forward applied to the new cell state (0: none) -- a clamped state passes no gradient."""
    h = _h(dh_use)
    B, U = dh_use.shape
    dev = dh_use.device
    dpre = dpre_out if dpre_out is not None else _f32((B, 4 * U), dev)
    dc_prev, dh_carry = _f32((B, U), dev), _f32((B, U), dev)
    dpeep = (dpeep_out if dpeep_out is not None else _f32((B, 3, U), dev)) if want_dpeep else None
    h.check(h.lib.asr_lstm_cell_bwd_ex(h.h, _p(dh_use), _p(dc_next), _p(dh_next), _p(gates), _p(c_raw), _p(c_prev),
                                       _p(peep), _p(live), B, U, float(cell_clip or 0.0), _p(dpre), _p(dc_prev),
                                       _p(dh_carry), _p(dpeep), _s()), 'asr_lstm_cell_bwd')
    return dpre, dc_prev, dh_carry, dpeep


def att_energy_fwd(keys, qz, v, T, mode):
    h = _h(qz)
    B, A = qz.shape
    energy = _f32((B, T), qz.device)
    h.check(h.lib.asr_att_energy_fwd(h.h, _p(keys), _p(qz), _p(v), T, B, A, int(mode), _p(energy), _s()),
            'asr_att_energy_fwd')
    return energy


def att_energy_bwd(denergy, keys, qz, v, mode, dkeys=None, want_dv=True, dqz_out=None, dv_out=None):
    h = _h(qz)
    B, A = qz.shape
    T = denergy.shape[1]
    dqz = dqz_out if dqz_out is not None else _f32((B, A), qz.device)
    dv = (dv_out if dv_out is not None else _f32((B, A), qz.device)) if want_dv else None
    h.check(h.lib.asr_att_energy_bwd(h.h, _p(denergy), _p(keys), _p(qz), _p(v), T, B, A, int(mode), _p(dkeys),
                                     _p(dqz), _p(dv), _s()), 'asr_att_energy_bwd')
    return dqz, dv


def att_softmax_ctx_fwd(energy, seq_len, sharpening, enc, alpha_out=None, sigmoid_norm=None, ctx_also=()):
    """sigmoid_norm: None = softmax; a [B] fp32 tensor = sigmoid smoothing (receives sum_t sigmoid(e)).
    ctx_also: up to two [B,E] column blocks of wider arrays that receive the context as well (same launch)."""
    h = _h(energy)
    B, T = energy.shape
    E = enc.shape[2]
    alpha = alpha_out if alpha_out is not None else _f32((B, T), energy.device)
    ctx = _f32((B, E), energy.device)
    if sigmoid_norm is not None and (sigmoid_norm.dtype != torch.float32 or sigmoid_norm.numel() != B):
        raise ValueError('sigmoid_norm must be fp32 [B]')
    also = [t for t in ctx_also if t is not None]
    if len(also) > 2:
        raise ValueError('att_softmax_ctx_fwd: at most two extra destinations')
    p2, l2 = _col_block(also[0] if len(also) > 0 else None, B, E, 'ctx_also')
    p3, l3 = _col_block(also[1] if len(also) > 1 else None, B, E, 'ctx_also')
    h.check(h.lib.asr_att_softmax_ctx_fwd_ex(h.h, _p(energy), _p(seq_len), float(sharpening), _p(enc),
                                             dtype_id(enc.dtype), T, B, E, _p(alpha), _p(ctx), _p(sigmoid_norm),
                                             p2, l2, p3, l3, _s()), 'asr_att_softmax_ctx_fwd')
    return alpha, ctx


def att_loc_energy_fwd(alpha_prev, filt, wfil, keys, qz, v, T):
    """Location / hybrid energies with the previous step's weights carried through conv1d -> W_filter
    (attention_layer.py:191-265).  alpha_prev [B,T]; filt [taps,1,10]; wfil [10,A]; keys [T,B,A] or None."""
    h = _h(qz)
    B, A = qz.shape
    taps = filt.shape[0]
    energy = _f32((B, T), qz.device)
    h.check(h.lib.asr_att_loc_energy_fwd(h.h, _p(alpha_prev), _p(filt), _p(wfil), _p(keys), _p(qz), _p(v), T, B, A,
                                         taps, _p(energy), _s()), 'asr_att_loc_energy_fwd')
    return energy


def att_loc_energy_bwd(denergy, alpha_prev, filt, wfil, keys, qz, v, dwfil_rows, dfilt_rows, accumulate, dkeys=None,
                       dqz_out=None, dv_out=None):
    """-> (dqz [B,A], dv_rows [B,A], dalpha_prev [B,T]); dwfil_rows [B,10,A] / dfilt_rows [B,taps,10] are
    overwritten (accumulate False) or added to (True); dkeys += in place when given."""
    h = _h(qz)
    B, A = qz.shape
    T = denergy.shape[1]
    taps = filt.shape[0]
    dqz = dqz_out if dqz_out is not None else _f32((B, A), qz.device)
    dv = dv_out if dv_out is not None else _f32((B, A), qz.device)
    dap = _f32((B, T), qz.device)
    h.check(h.lib.asr_att_loc_energy_bwd(h.h, _p(denergy), _p(alpha_prev), _p(filt), _p(wfil), _p(keys), _p(qz), _p(v),
                                         T, B, A, taps, _p(dkeys), _p(dqz), _p(dv), _p(dwfil_rows), _p(dfilt_rows),
                                         _p(dap), 1 if accumulate else 0, _s()), 'asr_att_loc_energy_bwd')
    return dqz, dv, dap


def att_softmax_ctx_bwd(dctx, alpha, seq_len, sharpening, enc, denc=None, sigmoid_norm=None, dalpha_extra=None):
    """denc None: only denergy is produced; the caller accumulates d_enc = sum_steps alpha (x) dctx itself.
    sigmoid_norm: the tensor the forward filled (sigmoid smoothing), or None (softmax).
    dalpha_extra [B,T]: gradient w.r.t. alpha from the next step's carried location features, or None."""
    h = _h(dctx)
    B, T = alpha.shape
    E = enc.shape[2]
    denergy = _f32((B, T), dctx.device)
    if sigmoid_norm is not None and (sigmoid_norm.dtype != torch.float32 or sigmoid_norm.numel() != B):
        raise ValueError('sigmoid_norm must be fp32 [B]')
    h.check(h.lib.asr_att_softmax_ctx_bwd(h.h, _p(dctx), _p(alpha), _p(seq_len), float(sharpening), _p(enc),
                                          dtype_id(enc.dtype), T, B, E, _p(denergy), _p(denc), _p(sigmoid_norm),
                                          _p(dalpha_extra), _s()),
            'asr_att_softmax_ctx_bwd')
    return denergy


class _AttDecoder(C.Structure):
    """struct asr_att_decoder (include/asr_hip.h), field for field."""
    _INTS = ['To', 'B', 'T', 'U', 'Em', 'E2', 'A', 'att_mode', 'has_query_fc', 'carry_alpha', 'taps', 'enc_dtype']
    _FLOATS = ['forget_bias', 'cell_clip', 'sharpening']
    _PTRS1 = ['W_cell', 'b_cell', 'peep', 'W_q', 'b_q', 'v']
    _PTRS2 = ['keys', 'enc', 'seq_len', 'filt', 'wfil', 'alpha_zero', 'live', 'dmask', 'dec_in', 'av_in', 'alpha_all',
              'snorm_all', 'gates_all', 'craw_all', 'c_all', 'h_all', 'qz_all', 'work', 'dav_cell', 'dav_ctx', 'dctx_all',
              'dpre_all', 'dqz_all', 'dv_all', 'dpeep_all', 'd_in_all', 'dkeys', 'dwfil_rows', 'dfilt_rows', 'dc0', 'dh0',
              'W_cell_il', 'W_cell_h']
    _fields_ = ([(n, C.c_int) for n in _INTS] + [(n, C.c_float) for n in _FLOATS] +
                [(n, C.c_void_p) for n in _PTRS1] + [('ld_wq', C.c_int)] + [(n, C.c_void_p) for n in _PTRS2])


def _att_decoder_struct(a):
    st = _AttDecoder()
    for n in _AttDecoder._INTS:
        setattr(st, n, int(a.get(n, 0) or 0))
    for n in _AttDecoder._FLOATS:
        setattr(st, n, float(a.get(n, 0.0) or 0.0))
    for n in _AttDecoder._PTRS1 + _AttDecoder._PTRS2:
        t = a.get(n)
        if t is not None and not t.is_cuda:
            raise RuntimeError('HIP path needs a CUDA(ROCm) tensor; there is no CPU fallback')
        if t is not None and n != 'W_q' and not t.is_contiguous():
            raise ValueError('att_decoder: %s must be contiguous' % n)
        setattr(st, n, t.data_ptr() if t is not None else None)
    wq = a.get('W_q')
    st.ld_wq = int(wq.stride(0)) if wq is not None else 0
    return st


FUSED_CELL_GEMM = os.environ.get('ASR_DEC_CELL_GEMM', '1') != '0'   # A/B: 0 keeps product and cell as two launches


BF16_CELL_WEIGHTS = os.environ.get('ASR_DEC_CELL_BF16', '1') != '0'   # A/B: 0 keeps fp32 decoder weights in bf16 models


def _cell_gemm_image(h, a):
    """Work space for the gate-interleaved image of W_cell | b_cell (the loops fill it): with it a decoder step's cell-input
    product and LSTM cell are one launch (asr_lstm_cell_gemm_fwd).  a['cell_bf16'] (bf16-operand models): the bf16 images
    instead (asr_lstm_cell_gemm_*_h: forward product + cell, backward product)."""
    Din = a['Em'] + a['E2'] + a['U']
    if a.get('gru') is not None:          # the GRU cell has its own image (_att_gru_struct)
        return
    if not (FUSED_CELL_GEMM and h.lib.asr_lstm_cell_gemm_ok(int(a['B']), Din, int(a['U']), Din)):
        return
    if a.get('cell_bf16') and BF16_CELL_WEIGHTS and a['U'] % 16 == 0:
        if a.get('W_cell_h') is None:
            nbytes = int(h.lib.asr_lstm_cell_gemm_h_bytes(Din, int(a['U'])))
            a['W_cell_h'] = torch.empty((nbytes // 4,), dtype=torch.float32, device=a['dec_in'].device)
    elif a.get('W_cell_il') is None:
        a['W_cell_il'] = _f32(((Din + 1) * 4 * a['U'],), a['dec_in'].device)


def _dec_work_floats(a, bwd):
    """Floats of a loop's work space (forward: pre-activations, raw h, energies, context; backward: 2 x dc, dh, d-alpha)."""
    return a['B'] * (5 * a['U'] + (3 if bwd else 1) * a['T'] + a['E2'])


def _dec_loop_call(h, base_name, a, st, *extra, bwd=False):
    """Call loop entry point `base_name` for the cell of `a`: + '_gru' with the GRU block, + '_stack' with the upper layers'
    block, else as it is.  st: the filled asr_att_decoder; extra: the arguments between the cell block and the stream."""
    if a.get('gru') is not None:
        name, blocks = base_name + '_gru', (C.byref(st), C.byref(_att_gru_struct(a)))
    elif a.get('stack') is not None:
        name, blocks = base_name + '_stack', (C.byref(st), C.byref(_att_stack_struct(a, bwd=bwd)))
    else:
        name, blocks = base_name, (C.byref(st),)
    h.check(getattr(h.lib, name)(h.h, *blocks, *extra, _s()), name)


def att_decoder_fwd(a):
    """All To steps of the attention decoder's forward pass from one call (asr_att_decoder_fwd).  `a`: dict of the
    struct's fields (ints / floats / cuda tensors or None); the per-step arrays are filled in place."""
    h = _h(a['dec_in'])
    if a.get('work') is None:
        a['work'] = _f32((_dec_work_floats(a, False),), a['dec_in'].device)
    _cell_gemm_image(h, a)
    _dec_loop_call(h, 'asr_att_decoder_fwd', a, _att_decoder_struct(a))


class _AttDecoderSS(C.Structure):
    """struct asr_att_decoder_ss (include/asr_hip.h), field for field."""
    _fields_ = [('W_av', C.c_void_p), ('W_out', C.c_void_p), ('b_out', C.c_void_p), ('embedding', C.c_void_p),
                ('C2', C.c_int), ('teacher_ids', C.c_void_p), ('draw', C.c_void_p), ('emb_mask', C.c_void_p),
                ('av_all', C.c_void_p), ('logits_all', C.c_void_p), ('ids_fed', C.c_void_p)]


def att_decoder_fwd_ss(a, W_av, W_out, b_out, embedding, teacher_ids, draw, emb_mask, out=None):
    """The training loop with scheduled sampling (asr_att_decoder_fwd_ss): `a` as for att_decoder_fwd (row 0 of dec_in
    filled by the caller), teacher_ids [To,B] int32, draw [To,B] float (non-zero: feed the previous step's argmax where the
    row is live), emb_mask [To,B,Em] or None.  Returns (av [To,B,U], logits [To,B,C2], ids_fed [To,B] int32), not imputed;
    the per-step arrays of `a` are filled in place.  out: the three result tensors, when the caller brings its own."""
    h = _h(a['dec_in'])
    dev = a['dec_in'].device
    To, B, U, Em = int(a['To']), int(a['B']), int(a['U']), int(a['Em'])
    C2 = int(W_out.shape[1])
    _chk(teacher_ids, torch.int32, 'teacher_ids')
    _chk(draw, torch.float32, 'draw')
    if tuple(teacher_ids.shape) != (To, B) or tuple(draw.shape) != (To, B):
        raise ValueError('att_decoder_fwd_ss: teacher_ids and draw are [To,B] = [%d,%d]' % (To, B))
    if emb_mask is not None and tuple(emb_mask.shape) != (To, B, Em):
        raise ValueError('att_decoder_fwd_ss: emb_mask is [To,B,Em] = [%d,%d,%d]' % (To, B, Em))
    if tuple(W_av.shape) != (U + int(a['E2']), U) or W_out.shape[0] != U or tuple(embedding.shape) != (C2, Em) or \
            (b_out is not None and tuple(b_out.shape) != (C2,)):
        raise ValueError('att_decoder_fwd_ss: W_av [U+E2,U], W_out [U,C2], b_out [C2], embedding [C2,Em]')
    if a.get('work') is None:
        a['work'] = _f32((_dec_work_floats(a, False),), dev)
    _cell_gemm_image(h, a)
    if out is not None:
        av, logits, ids_fed = out
        if tuple(av.shape) != (To, B, U) or tuple(logits.shape) != (To, B, C2) or tuple(ids_fed.shape) != (To, B) or \
                ids_fed.dtype != torch.int32:
            raise ValueError('att_decoder_fwd_ss: out is (av [To,B,U], logits [To,B,C2], ids_fed [To,B] int32)')
    else:
        av, logits = _f32((To, B, U), dev), _f32((To, B, C2), dev)
        ids_fed = torch.empty((To, B), dtype=torch.int32, device=dev)
    ids_fed[0].copy_(teacher_ids[0])
    st = _att_decoder_struct(a)
    f = _AttDecoderSS()
    for n, t in (('W_av', W_av), ('W_out', W_out), ('b_out', b_out), ('embedding', embedding), ('teacher_ids', teacher_ids),
                 ('draw', draw), ('emb_mask', emb_mask), ('av_all', av), ('logits_all', logits), ('ids_fed', ids_fed)):
        if t is not None and (not t.is_cuda or not t.is_contiguous()):
            raise ValueError('att_decoder_fwd_ss: %s must be a contiguous device tensor' % n)
        if t is not None and n not in ('teacher_ids', 'ids_fed') and t.dtype != torch.float32:
            raise ValueError('att_decoder_fwd_ss: %s must be float32' % n)
        setattr(f, n, t.data_ptr() if t is not None else None)
    f.C2 = C2
    h.check(h.lib.asr_att_decoder_fwd_ss(h.h, C.byref(st), C.byref(f), _s()), 'asr_att_decoder_fwd_ss')
    return av, logits, ids_fed


def att_decoder_bwd(a):
    """The reverse loop (asr_att_decoder_bwd): fills dctx_all, dpre_all, dqz_all, dv_all, dpeep_all, d_in_all, dc0, dh0
    (and adds into dkeys / the filter gradients)."""
    h = _h(a['dec_in'])
    a['work'] = _f32((_dec_work_floats(a, True),), a['dec_in'].device)
    _cell_gemm_image(h, a)
    # (GRU: dpre_all is [To,B,3U] = dr | du | dp and dc0 is not written; stack: the upper layers' dpre / d_hin / dpeep /
    # dc0 / dh0 are in the stack block)
    _dec_loop_call(h, 'asr_att_decoder_bwd', a, _att_decoder_struct(a), bwd=True)


class _AttInfer(C.Structure):
    """struct asr_att_infer (include/asr_hip.h), field for field."""
    _fields_ = [('W_av', C.c_void_p), ('W_out', C.c_void_p), ('b_out', C.c_void_p), ('embedding', C.c_void_p),
                ('C2', C.c_int), ('eos', C.c_int), ('live', C.c_void_p), ('av_all', C.c_void_p), ('logits_all', C.c_void_p),
                ('ids_all', C.c_void_p), ('live_count', C.c_void_p), ('host_live_count', C.c_void_p), ('check_every', C.c_int)]


def _att_infer_struct(what, To, C2, eos, check_every, **tensors):
    """struct asr_att_infer for a decode loop of at most To steps, with the pinned words its early exit reads (None with
    check_every 0; the caller keeps them alive until it has synchronised)."""
    host = torch.ones((To + 1,), dtype=torch.int32).pin_memory() if check_every else None
    f = _AttInfer()
    for n, t in tensors.items():
        if t is not None and (not t.is_cuda or not t.is_contiguous()):
            raise ValueError('%s: %s must be a contiguous device tensor' % (what, n))
        setattr(f, n, t.data_ptr() if t is not None else None)
    f.C2, f.eos, f.check_every = int(C2), int(eos), int(check_every or 0)
    f.host_live_count = host.data_ptr() if host is not None else None
    return f, host


def att_decoder_infer(a, W_av, W_out, b_out, embedding, eos, n_live, check_every=8):
    """Greedy inference loop (asr_att_decoder_infer): `a` as for att_decoder_fwd with To = max_decode_length and
    a['live'] a [To+1,B] tensor whose row 0 marks the rows that decode.  Returns a dict: ids [To,B] int32 (imputed),
    logits [To,B,C2], av [To,B,U], live [To+1,B], live_count [To+1] int32 (all on the device, nothing synchronised) and
    steps_issued (host int)."""
    h = _h(a['dec_in'])
    dev = a['dec_in'].device
    To, B, U = a['To'], a['B'], a['U']
    C2 = W_out.shape[1]
    if a.get('work') is None:
        a['work'] = _f32((_dec_work_floats(a, False),), dev)
    _cell_gemm_image(h, a)
    out = dict(ids=torch.empty((To, B), dtype=torch.int32, device=dev), logits=_f32((To, B, C2), dev), av=_f32((To, B, U), dev),
               live=a['live'], live_count=torch.empty((To + 1,), dtype=torch.int32, device=dev))
    out['live_count'][:1].fill_(int(n_live))
    st = _att_decoder_struct(a)
    f, host = _att_infer_struct('att_decoder_infer', To, C2, eos, check_every, W_av=W_av, W_out=W_out, b_out=b_out,
                                embedding=embedding, live=a['live'], av_all=out['av'], logits_all=out['logits'],
                                ids_all=out['ids'], live_count=out['live_count'])
    issued = C.c_int(0)
    _dec_loop_call(h, 'asr_att_decoder_infer', a, st, C.byref(f), C.byref(issued))
    out['steps_issued'] = issued.value
    out['_host'] = host                      # keeps the pinned words alive until the caller has synchronised
    return out


# ---------------------------------------------------------------- beam search over the attention decoder
MAX_BEAM_WIDTH = 32


def _beam_width(beam_width, C2):
    W = int(beam_width)
    if W < 1 or W > MAX_BEAM_WIDTH:
        raise ValueError('beam_width must be in 1 .. %d, got %d' % (MAX_BEAM_WIDTH, W))
    if W > int(C2):
        raise ValueError('beam_width %d exceeds the %d classes step 0 selects among' % (W, int(C2)))
    return W


def _i32(shape, dev):
    return torch.empty(shape, dtype=torch.int32, device=dev)


def att_beam_select(logits, beam_width, eos, length_penalty_weight, first_step, log_probs, finished, lengths,
                    unfinished=None):
    """One beam search selection per utterance (asr_att_beam_select; beam_search_step, beam_search_decoder.py:234-332).
    logits [B*W,C2]; log_probs [B*W] fp32, finished / lengths [B*W] int32: the state before the step (left unchanged).
    Returns word, parent [B,W] int32, score [B,W], and the next state log_probs, finished, lengths [B*W].
    length_penalty_weight None is 0.0; unfinished: an int32 word the count of unfinished slots is added to."""
    h = _h(logits)
    R, C2 = logits.shape
    W = _beam_width(beam_width, C2)
    if R % W:
        raise ValueError('att_beam_select: %d rows are not a multiple of beam_width %d' % (R, W))
    B, dev = R // W, logits.device
    _chk(logits, torch.float32, 'logits')
    _chk(log_probs, torch.float32, 'log_probs')
    _chk(finished, torch.int32, 'finished')
    _chk(lengths, torch.int32, 'lengths')
    word, parent, score = _i32((B, W), dev), _i32((B, W), dev), _f32((B, W), dev)
    lp, fin, ln = _f32((R,), dev), _i32((R,), dev), _i32((R,), dev)
    a = 0.0 if length_penalty_weight is None else float(length_penalty_weight)
    h.check(h.lib.asr_att_beam_select(h.h, _p(logits), B, W, int(C2), int(eos), a, int(bool(first_step)), _p(log_probs),
                                      _p(finished), _p(lengths), _p(word), _p(parent), _p(score), _p(lp), _p(fin), _p(ln),
                                      _p(unfinished), _s()), 'asr_att_beam_select')
    return word, parent, score, lp, fin, ln


def att_beam_reorder(parent, word, c_src, h_src, din_src, alpha_src, embedding):
    """What the next decoder step reads, gathered by parent within each utterance (asr_att_beam_reorder): parent / word
    [B,W] int32; c_src / h_src [B*W,U], din_src [B*W,Em+E2+U], alpha_src [B*W,T] or None.  Returns new c, h, din (its
    embedding columns = embedding[word]) and alpha (None without alpha_src)."""
    h = _h(c_src)
    B, W = parent.shape
    R, U = c_src.shape
    Em = int(embedding.shape[1])
    E2 = din_src.shape[1] - Em - U
    T = int(alpha_src.shape[1]) if alpha_src is not None else 0
    for t, dt, n in ((parent, torch.int32, 'parent'), (word, torch.int32, 'word'), (c_src, torch.float32, 'c_src'),
                     (h_src, torch.float32, 'h_src'), (din_src, torch.float32, 'din_src'), (embedding, torch.float32, 'embedding')):
        _chk(t, dt, n)
    if R != B * W or h_src.shape != c_src.shape or din_src.shape[0] != R or E2 < 1 or (alpha_src is not None and alpha_src.shape[0] != R):
        raise ValueError('att_beam_reorder: shapes disagree')
    c, hh, din = torch.empty_like(c_src), torch.empty_like(h_src), torch.empty_like(din_src)
    alpha = torch.empty_like(alpha_src) if alpha_src is not None else None
    h.check(h.lib.asr_att_beam_reorder(h.h, _p(parent), _p(word), B, W, U, Em, E2, T, int(embedding.shape[0]), _p(c_src),
                                       _p(h_src), _p(din_src), _p(alpha_src), _p(embedding), _p(c), _p(hh), _p(din),
                                       _p(alpha), _s()), 'asr_att_beam_reorder')
    return c, hh, din, alpha


def att_beam_backtrace(word, parent, score, steps, eos):
    """gather_tree_py over the first `steps` rows of word / parent [To,B,W] int32, cut behind the first <EOS>
    (asr_att_beam_backtrace).  Returns ids [B,W,To] int32, hyp_len [B,W] int32, final_score [B,W]."""
    h = _h(word)
    To, B, W = word.shape
    _chk(word, torch.int32, 'word')
    _chk(parent, torch.int32, 'parent')
    _chk(score, torch.float32, 'score')
    ids, n, fs = _i32((B, W, To), word.device), _i32((B, W), word.device), _f32((B, W), word.device)
    h.check(h.lib.asr_att_beam_backtrace(h.h, _p(word), _p(parent), _p(score), int(steps), To, B, W, int(eos), _p(ids), _p(n),
                                         _p(fs), _s()), 'asr_att_beam_backtrace')
    return ids, n, fs


class _AttBeam(C.Structure):
    """struct asr_att_beam (include/asr_hip.h), field for field."""
    _PTRS = ['word', 'parent', 'score', 'log_probs', 'finished', 'lengths', 'alpha_prev', 'av', 'logits', 'unfinished', 'ids',
             'hyp_len', 'final_score']
    _fields_ = [('W', C.c_int), ('length_penalty_weight', C.c_float)] + [(n, C.c_void_p) for n in _PTRS]


def _beam_loop_call(what, a, W_av, W_out, b_out, embedding, eos, W, length_penalty_weight, check_every, extra_out=None,
                    extra_scratch=None):
    """What att_decoder_beam and att_decoder_beam_joint share: the loop's work space, its outputs and scratch, and the three
    structs.  Returns (h, st, f, m, out, scratch, host); the caller issues the native call and finishes `out` with
    _beam_loop_done."""
    h = _h(a['dec_in'])
    dev = a['dec_in'].device
    To, R, U = a['To'], a['B'], a['U']
    C2 = W_out.shape[1]
    if R % W:
        raise ValueError('%s: %d rows are not a multiple of beam_width %d' % (what, R, W))
    B = R // W
    if a.get('work') is None:
        a['work'] = _f32((_dec_work_floats(a, False),), dev)
    _cell_gemm_image(h, a)
    out = dict(word=_i32((To, B, W), dev), parent=_i32((To, B, W), dev), score=_f32((To, B, W), dev),
               log_probs=torch.zeros((B, W), dtype=torch.float32, device=dev),
               finished=torch.zeros((B, W), dtype=torch.int32, device=dev),
               lengths=torch.zeros((B, W), dtype=torch.int32, device=dev), unfinished=_i32((To + 1,), dev),
               ids=_i32((B, W, To), dev), hyp_len=_i32((B, W), dev), final_score=_f32((B, W), dev))
    out.update(extra_out or {})
    scratch = dict(av=_f32((R, U), dev), logits=_f32((R, C2), dev),
                   alpha_prev=torch.zeros((R, a['T']), dtype=torch.float32, device=dev) if a.get('carry_alpha') else None)
    scratch.update(extra_scratch or {})
    if a.get('carry_alpha') and a.get('alpha_zero') is None:
        a['alpha_zero'] = scratch['alpha_prev']
    st = _att_decoder_struct(a)
    f, host = _att_infer_struct(what, To, C2, eos, check_every, W_av=W_av, W_out=W_out, b_out=b_out, embedding=embedding)
    m = _AttBeam()
    m.W = W
    m.length_penalty_weight = 0.0 if length_penalty_weight is None else float(length_penalty_weight)
    for n in _AttBeam._PTRS:
        t = out.get(n, scratch.get(n))
        setattr(m, n, t.data_ptr() if t is not None else None)
    return h, st, f, m, out, scratch, host


def _beam_loop_done(out, issued, host, scratch):
    out['steps_issued'] = issued.value
    out['_host'] = host                      # keeps the pinned words (and the scratch) alive until the caller has synchronised
    out['_scratch'] = scratch
    return out


def att_decoder_beam(a, W_av, W_out, b_out, embedding, eos, beam_width, length_penalty_weight=0.0, check_every=8):
    """Beam search decode from one call (asr_att_decoder_beam).  `a`: the struct's fields as for att_decoder_fwd with
    B = utterances * beam_width rows (row b*W + w; encoder arrays tiled by the caller), To = max_decode_length, live [R]
    ones, and ONE step of state: dec_in [2,R,Din], c_all / h_all [2,R,U] (block 0 filled by the caller), av_in [1,R,U+E2],
    alpha_all [1,R,T], gates_all / craw_all / qz_all one step.  Returns a dict, everything on the device and nothing
    synchronised: word, parent [To,B,W] int32 and score [To,B,W] per step; ids [B,W,To] (0 behind the first <EOS>),
    hyp_len [B,W], final_score [B,W] (slot 0 is the best hypothesis); the final state log_probs, finished, lengths
    [B,W]; unfinished [To+1]; and steps_issued (host int)."""
    W = _beam_width(beam_width, W_out.shape[1])
    h, st, f, m, out, scratch, host = _beam_loop_call('att_decoder_beam', a, W_av, W_out, b_out, embedding, eos, W,
                                                      length_penalty_weight, check_every)
    issued = C.c_int(0)
    # (GRU: c_all is zeros [2,R,U], gathered by the re-ordering as ever; stack: the upper layers' in [2,R,2U] and c / h
    # [2,R,U] are re-ordered by asr_att_stack_reorder)
    _dec_loop_call(h, 'asr_att_decoder_beam', a, st, C.byref(f), C.byref(m), C.byref(issued))
    return _beam_loop_done(out, issued, host, scratch)


# ---------------------------------------------------------------- joint CTC / attention beam search (an extension)
def log_softmax_rows(x2d, out=None):
    """x - logsumexp(x) per row of an fp32 [rows, cols] array (asr_log_softmax_rows)."""
    h = _h(x2d)
    _chk(x2d, torch.float32, 'x')
    if x2d.dim() != 2 or x2d.shape[0] < 1 or x2d.shape[1] < 1:
        raise ValueError('log_softmax_rows: x must be a non-empty [rows, cols] array')
    out = _out_like(out, tuple(x2d.shape), torch.float32, x2d.device, 'log_softmax_rows')
    h.check(h.lib.asr_log_softmax_rows(h.h, _p(x2d), _p(out), x2d.shape[0], x2d.shape[1], _s()), 'asr_log_softmax_rows')
    return out


def _joint_shapes(what, y, seq_len, R, n_labels=None, blank=None):
    """(B, W, T, By, Cc, blank) of a joint-search call on R device rows; y [T,By,Cc] fp32, seq_len [B] int32."""
    _chk(y, torch.float32, 'y')
    _chk(seq_len, torch.int32, 'seq_len')
    if y.dim() != 3 or seq_len.dim() != 1:
        raise ValueError('%s: y must be [T,By,Cc] and seq_len [B]' % what)
    T, By, Cc = (int(v) for v in y.shape)
    B = int(seq_len.shape[0])
    if B < 1 or B > By or R < B or R % B:
        raise ValueError('%s: %d rows for %d utterances (y holds %d)' % (what, R, B, By))
    W = R // B
    if W > MAX_BEAM_WIDTH:
        raise ValueError('beam_width must be in 1 .. %d, got %d' % (MAX_BEAM_WIDTH, W))
    blank = Cc - 1 if blank is None else int(blank)
    if n_labels is not None and not (1 <= int(n_labels) < Cc and int(n_labels) <= blank < Cc):
        raise ValueError('%s: %d labels, blank %d, %d CTC classes' % (what, int(n_labels), blank, Cc))
    if not 0 <= blank < Cc:
        raise ValueError('%s: blank %d outside the %d CTC classes' % (what, blank, Cc))
    return B, W, T, By, Cc, blank


def _check_ctc_weight(ctc_weight):
    lam = float(ctc_weight)
    if not 0.0 < lam <= 1.0:
        raise ValueError('ctc_weight must be in (0, 1] here (0 is the attention-only beam search), got %r' % (ctc_weight,))
    return lam


def ctc_prefix_init(y, seq_len, beam_width, blank=None):
    """The prefix state of the empty hypothesis in each of the B * beam_width rows (asr_ctc_prefix_init): y [T,By,Cc] CTC
    log-posteriors, seq_len [B] int32.  Returns r [R,2,T] (entries at t >= seq_len[b] are not written), last [R] int32
    (-1) and ctc_score [R] (0)."""
    h = _h(y)
    W = int(beam_width)
    if W < 1 or W > MAX_BEAM_WIDTH:
        raise ValueError('beam_width must be in 1 .. %d, got %d' % (MAX_BEAM_WIDTH, W))
    B, W, T, By, Cc, blank = _joint_shapes('ctc_prefix_init', y, seq_len, int(seq_len.numel()) * W, blank=blank)
    R, dev = B * W, y.device
    r, last, score = _f32((R, 2, T), dev), _i32((R,), dev), _f32((R,), dev)
    h.check(h.lib.asr_ctc_prefix_init(h.h, _p(y), _p(seq_len), B, W, T, By, Cc, blank, _p(r), _p(last), _p(score), _s()),
            'asr_ctc_prefix_init')
    return r, last, score


def _chk_state(what, r, last, T):
    _chk(r, torch.float32, 'r')
    _chk(last, torch.int32, 'last')
    if r.dim() != 3 or r.shape[1] != 2 or r.shape[2] != T or tuple(last.shape) != (r.shape[0],):
        raise ValueError('%s: r must be [R,2,%d] and last [R]' % (what, T))


def ctc_prefix_score(y, seq_len, r, last, finished, cand, n_labels, blank=None):
    """CTC prefix scores psi [R,K] of the candidates cand [R,K] (int32 attention class ids: labels, <SOS> = n_labels,
    <EOS> = n_labels + 1) of the hypotheses whose state is r [R,2,T] / last [R] (asr_ctc_prefix_score); finished [R] int32
    or None: a finished row scores its <EOS> alone.  An infeasible prefix and <SOS> are exactly -inf."""
    h = _h(y)
    _chk(cand, torch.int32, 'cand')
    if cand.dim() != 2 or not 1 <= cand.shape[1] <= 64:
        raise ValueError('ctc_prefix_score: cand must be [R, 1 .. 64]')
    R, K = (int(v) for v in cand.shape)
    B, W, T, By, Cc, blank = _joint_shapes('ctc_prefix_score', y, seq_len, R, n_labels, blank)
    _chk_state('ctc_prefix_score', r, last, T)
    if r.shape[0] != R or (finished is not None and tuple(finished.shape) != (R,)):
        raise ValueError('ctc_prefix_score: state and candidates disagree on the number of rows')
    if finished is not None:
        _chk(finished, torch.int32, 'finished')
    psi = _f32((R, K), y.device)
    h.check(h.lib.asr_ctc_prefix_score(h.h, _p(y), _p(seq_len), B, W, T, By, Cc, blank, int(n_labels), _p(r), _p(last),
                                       _p(finished), _p(cand), K, _p(psi), _s()), 'asr_ctc_prefix_score')
    return psi


def ctc_prefix_advance(y, seq_len, r, last, parent, word, n_labels, blank=None):
    """The prefix state of the selected hypotheses (asr_ctc_prefix_advance): new row b*W + w extends the hypothesis of row
    b*W + parent[b,w] (state r [R,2,T], last [R]: the parents') by word[b,w]; <EOS> copies.  Returns the new r (out of
    place: the sources are untouched)."""
    h = _h(y)
    _chk(parent, torch.int32, 'parent')
    _chk(word, torch.int32, 'word')
    if parent.dim() != 2 or parent.shape != word.shape:
        raise ValueError('ctc_prefix_advance: parent and word must be [B,W]')
    R = int(parent.numel())
    B, W, T, By, Cc, blank = _joint_shapes('ctc_prefix_advance', y, seq_len, R, n_labels, blank)
    _chk_state('ctc_prefix_advance', r, last, T)
    if r.shape[0] != R or tuple(parent.shape) != (B, W):
        raise ValueError('ctc_prefix_advance: state and selection disagree on the number of rows')
    out = torch.empty_like(r)
    h.check(h.lib.asr_ctc_prefix_advance(h.h, _p(y), _p(seq_len), B, W, T, By, Cc, blank, int(n_labels), _p(r), _p(last),
                                         _p(parent), _p(word), _p(out), _s()), 'asr_ctc_prefix_advance')
    return out


def _select_streams(what, h, logits, lm_logits, N, W, lam, mu, length_penalty_weight, first_step, state, ctc, unfinished):
    """What att_beam_select_joint and att_beam_select_fused share behind their own argument checks: the checks of the [R]
    state arrays `state` ((tensor, dtype, name) of log_probs, finished, lengths and, per stream, ctc_score / lm_score), the
    outputs and the native call -- asr_att_beam_select_joint without lm_logits, asr_att_beam_select_fused with.  ctc: None
    or (y, seq_len, r, last, T, By, Cc, blank).  Returns word, parent, score, log_probs, finished, lengths, lm_score, last,
    ctc_score (None for a stream that is off)."""
    R, dev = int(logits.shape[0]), logits.device
    B = R // W
    _beam_width(W, N + 1)
    for t, dt, n in state:
        _chk(t, dt, n)
        if tuple(t.shape) != (R,):
            raise ValueError('%s: %s must be [%d]' % (what, n, R))
    st = {n: _p(t) for t, _, n in state}
    y, seq_len, r, last, T, By, Cc, blank = ctc if ctc is not None else (None, None, None, None, 0, 0, 0, 0)
    word, parent, score = _i32((B, W), dev), _i32((B, W), dev), _f32((B, W), dev)
    lp, fin, ln = _f32((R,), dev), _i32((R,), dev), _i32((R,), dev)
    cand, tot = _i32((R, W + 1), dev), _f32((R, W + 1), dev)
    psi, lst, cs = (_f32((R, W + 1), dev), _i32((R,), dev), _f32((R,), dev)) if ctc is not None else (None, None, None)
    clm, ls = (_f32((R, W + 1), dev), _f32((R,), dev)) if lm_logits is not None else (None, None)
    a = 0.0 if length_penalty_weight is None else float(length_penalty_weight)
    state_in = (int(bool(first_step)), _p(y), _p(seq_len), T, By, Cc, blank, _p(r), st['log_probs'], st['finished'],
                st['lengths'], _p(last), st.get('ctc_score'))
    out = (_p(word), _p(parent), _p(score), _p(lp), _p(fin), _p(ln), _p(lst), _p(cs))
    if lm_logits is None:
        rc = h.lib.asr_att_beam_select_joint(h.h, _p(logits), B, W, N, a, lam, *state_in, _p(cand), _p(tot), _p(psi), *out,
                                             _p(unfinished), _s())
    else:
        rc = h.lib.asr_att_beam_select_fused(h.h, _p(logits), _p(lm_logits), B, W, N, a, lam, mu, *state_in, st['lm_score'],
                                             _p(cand), _p(tot), _p(clm), _p(psi), *out, _p(ls), _p(unfinished), _s())
    h.check(rc, 'asr_' + what)
    return word, parent, score, lp, fin, ln, ls, lst, cs


def att_beam_select_joint(logits, y, seq_len, r, last, ctc_score, n_labels, ctc_weight, length_penalty_weight, first_step,
                          log_probs, finished, lengths, unfinished=None, blank=None):
    """One joint CTC / attention selection per utterance (asr_att_beam_select_joint): att_beam_select on
    ((1 - ctc_weight) * total_att + ctc_weight * ctc) / penalty over the preselected W + 1 classes of every slot.
    logits [B*W, n_labels + 2]; y / seq_len / r / last as ctc_prefix_score; ctc_score [B*W] fp32.  Nothing is changed in
    place.  Returns word, parent [B,W] int32, score [B,W] and the next state log_probs (attention totals), finished,
    lengths, last, ctc_score [B*W] -- the next r is ctc_prefix_advance(y, seq_len, r, last, parent, word, n_labels)."""
    h = _h(logits)
    _chk(logits, torch.float32, 'logits')
    R, C2 = (int(v) for v in logits.shape)
    N = int(n_labels)
    if C2 != N + 2:
        raise ValueError('att_beam_select_joint: %d attention classes for %d labels' % (C2, N))
    lam = _check_ctc_weight(ctc_weight)
    B, W, T, By, Cc, blank = _joint_shapes('att_beam_select_joint', y, seq_len, R, N, blank)
    _chk_state('att_beam_select_joint', r, last, T)
    if r.shape[0] != R:
        raise ValueError('att_beam_select_joint: r must have %d rows' % R)
    state = [(log_probs, torch.float32, 'log_probs'), (ctc_score, torch.float32, 'ctc_score'),
             (finished, torch.int32, 'finished'), (lengths, torch.int32, 'lengths')]
    out = _select_streams('att_beam_select_joint', h, logits, None, N, W, lam, 0.0, length_penalty_weight, first_step, state,
                          (y, seq_len, r, last, T, By, Cc, blank), unfinished)
    return out[:6] + out[7:]


class _AttBeamCtc(C.Structure):
    """struct asr_att_beam_ctc (include/asr_hip.h), field for field."""
    _fields_ = [('y', C.c_void_p), ('seq_len', C.c_void_p), ('By', C.c_int), ('Cc', C.c_int), ('blank', C.c_int),
                ('n_labels', C.c_int), ('ctc_weight', C.c_float), ('r', C.c_void_p), ('last', C.c_void_p),
                ('ctc_score', C.c_void_p), ('cand', C.c_void_p), ('cand_total', C.c_void_p), ('psi', C.c_void_p)]


def _beam_ctc(what, a, y, seq_len, W, N, lam, blank):
    """The CTC part of att_decoder_beam_joint / att_decoder_beam_lm: y / seq_len checked against the loop's R rows of
    a['T'] frames.  Returns the loop's extra scratch (prefix state r / last in two blocks, candidates, their totals and
    psi; y and seq_len kept alive), its ctc_score [B,W] output and struct asr_att_beam_ctc over them."""
    dev, R = a['dec_in'].device, a['B']
    B, W2, T, By, Cc, blank = _joint_shapes(what, y, seq_len, R, N, blank)
    if W2 != W or T != a['T']:
        raise ValueError('%s: y [%d,%d,%d] / seq_len [%d] do not fit %d rows of %d frames' % (what, T, By, Cc, B, R, a['T']))
    t = dict(r=_f32((2, R, 2, T), dev), last=_i32((2, R), dev), cand=_i32((R, W + 1), dev),
             cand_total=_f32((R, W + 1), dev), psi=_f32((R, W + 1), dev), y=y, seq_len=seq_len)
    ctc_score = _f32((B, W), dev)
    j = _AttBeamCtc()
    j.By, j.Cc, j.blank, j.n_labels, j.ctc_weight = By, Cc, blank, N, lam
    for n, v in list(t.items()) + [('ctc_score', ctc_score)]:
        setattr(j, n, v.data_ptr())
    return t, ctc_score, j


def att_decoder_beam_joint(a, W_av, W_out, b_out, embedding, eos, beam_width, y, seq_len, ctc_weight,
                           length_penalty_weight=0.0, check_every=8, blank=None):
    """Joint CTC / attention beam search decode from one call (asr_att_decoder_beam_joint): att_decoder_beam with
    y [T,By,Cc], the CTC log-posteriors of the B utterances (NOT tiled; T = a['T']), seq_len [B] int32 and
    0 < ctc_weight <= 1.  Returns att_decoder_beam's dict (log_probs are the attention totals, score / final_score the
    fused, length-normalised scores) and ctc_score [B,W].
    Every seq_len must be >= 1 (not checked here: that would read the device; JointCTCAttention.infer checks its host
    copy).  An utterance of 0 frames has the empty hypothesis alone: places no candidate with a finite CTC score reaches
    come out as finished <EOS> slots with score -inf."""
    R = a['B']
    C2 = int(W_out.shape[1])
    N = C2 - 2
    if int(eos) != N + 1:
        raise ValueError('att_decoder_beam_joint: <EOS> must be the last of the %d attention classes' % C2)
    W = _beam_width(beam_width, N + 1)
    lam = _check_ctc_weight(ctc_weight)
    if R % W:
        raise ValueError('att_decoder_beam_joint: %d rows are not a multiple of beam_width %d' % (R, W))
    extra, ctc_score, j = _beam_ctc('att_decoder_beam_joint', a, y, seq_len, W, N, lam, blank)
    h, st, f, m, out, scratch, host = _beam_loop_call('att_decoder_beam_joint', a, W_av, W_out, b_out, embedding, eos, W,
                                                      length_penalty_weight, check_every,
                                                      extra_out=dict(ctc_score=ctc_score), extra_scratch=extra)
    issued = C.c_int(0)
    h.check(h.lib.asr_att_decoder_beam_joint(h.h, C.byref(st), C.byref(f), C.byref(m), C.byref(j), C.byref(issued), _s()),
            'asr_att_decoder_beam_joint')
    return _beam_loop_done(out, issued, host, scratch)


# ---------------------------------------------------------------- GRU decoder cell (decoder_type 'gru')
GRU_CELL_GEMM = os.environ.get('ASR_DEC_GRU_GEMM', '1') != '0'   # A/B: 0 keeps every step on the four-launch form


class _AttGru(C.Structure):
    """struct asr_att_gru (include/asr_hip.h), field for field."""
    _PTRS = ['W_g', 'b_g', 'W_c', 'b_c', 'W3']
    _fields_ = [(n, C.c_void_p) for n in _PTRS] + [('fused', C.c_int)]


def _att_gru_struct(a):
    """The GRU block of a loop dict: a['gru'] = dict(W_g [Din,2U], b_g [2U], W_c [Din,U], b_c [U]) and, optional, W3 (the
    image work space, made here when missing) and fused (False: the four-launch form at every shape)."""
    gd = a['gru']
    U, Din = int(a['U']), int(a['Em'] + a['E2'] + a['U'])
    for n, shape in (('W_g', (Din, 2 * U)), ('b_g', (2 * U,)), ('W_c', (Din, U)), ('b_c', (U,))):
        t = gd.get(n)
        if t is None or not t.is_cuda or not t.is_contiguous() or t.dtype != torch.float32 or tuple(t.shape) != shape:
            raise ValueError('att_decoder (gru): %s must be a contiguous fp32 device tensor of shape %r' % (n, shape))
    if gd.get('W3') is None:
        gd['W3'] = _f32(((Din + 1), 3 * U), a['dec_in'].device)
    g = _AttGru()
    for n in _AttGru._PTRS:
        setattr(g, n, gd[n].data_ptr())
    g.fused = int(bool(gd.get('fused', True)) and GRU_CELL_GEMM)
    return g


def gru_cell_prep(W_g, b_g, W_c, b_c):
    """The image W3 [(Din + 1), 3U] the GRU cell's products read (asr_gru_cell_prep): W_g | W_c with its h-rows zeroed,
    bias row last."""
    h = _h(W_g)
    Din, U = W_c.shape
    for t, n in ((W_g, 'W_g'), (b_g, 'b_g'), (W_c, 'W_c'), (b_c, 'b_c')):
        _chk(t, torch.float32, n)
    if tuple(W_g.shape) != (Din, 2 * U) or tuple(b_g.shape) != (2 * U,) or tuple(b_c.shape) != (U,) or Din <= U:
        raise ValueError('gru_cell_prep: W_g [Din,2U], b_g [2U], W_c [Din,U], b_c [U], Din > U')
    out = _f32((Din + 1, 3 * U), W_g.device)
    h.check(h.lib.asr_gru_cell_prep(h.h, _p(W_g), _p(b_g), _p(W_c), _p(b_c), Din, U, _p(out), _s()), 'asr_gru_cell_prep')
    return out


def gru_cell_gemm_ok(B, Din, U, ldx=None):
    """Whether the two-launch form covers the shape (asr_gru_cell_gemm_ok): B <= 32, Din % 64 == 0, U % 16 == 0."""
    from . import _lib
    return bool(_lib.load().asr_gru_cell_gemm_ok(int(B), int(Din), int(U), int(Din if ldx is None else ldx)))


def gru_cell_fwd(x, W3, W_c, h_prev, live, out_mask=None, fused=False, h_also=None, cell_out_also=None, out=None):
    """One GRU decoder cell step (asr_gru_cell_fwd_ex, or asr_gru_cell_gemm_fwd when fused): x [B,Din] = input | h_prev (a
    row block of a wider array is fine), W3 from gru_cell_prep, W_c the candidate kernel itself (its h-rows are read).
    Returns (gates [B,4U] = r | u | c | r*h, h_out [B,U], cell_out [B,U]); h_also / cell_out_also / cell_out_also2: [B,U]
    column blocks of wider arrays that receive h_out / cell_out as well.  out: the three result tensors, when the caller
    brings its own (cell_out may itself be a column block of a wider array: the loops write it into av_in)."""
    h = _h(x)
    B, Din = x.shape
    U = W_c.shape[1]
    dev = x.device
    if x.dtype != torch.float32 or x.stride(1) != 1:
        raise ValueError('gru_cell_fwd: x must be fp32 with unit inner stride')
    for t, n in ((W3, 'W3'), (W_c, 'W_c'), (h_prev, 'h_prev'), (live, 'live')):
        _chk(t, torch.float32, n)
    if tuple(W3.shape) != (Din + 1, 3 * U) or tuple(W_c.shape) != (Din, U) or tuple(h_prev.shape) != (B, U):
        raise ValueError('gru_cell_fwd: shapes disagree')
    gates, h_out, cell_out = out if out is not None else (_f32((B, 4 * U), dev), _f32((B, U), dev), _f32((B, U), dev))
    hp, hld = _col_block(h_also, B, U, 'h_also')
    cp, cld = _col_block(cell_out_also, B, U, 'cell_out_also')
    op, old = _col_block(cell_out, B, U, 'cell_out')
    W_ch = C.c_void_p(W_c.data_ptr() + (Din - U) * U * 4)
    xp = C.c_void_p(x.data_ptr())
    if fused:
        h.check(h.lib.asr_gru_cell_gemm_fwd(h.h, xp, int(x.stride(0)), Din, _p(W3), W_ch, _p(h_prev), _p(live), _p(out_mask),
                                            B, U, _p(gates), _p(h_out), op, old, hp, hld, cp, cld, _s()),
                'asr_gru_cell_gemm_fwd')
    else:
        work = _f32((B, 4 * U), dev)
        h.check(h.lib.asr_gru_cell_fwd_ex(h.h, xp, int(x.stride(0)), Din, _p(W3), W_ch, _p(h_prev), _p(live), _p(out_mask),
                                          B, U, _p(gates), _p(h_out), op, old, hp, hld, cp, cld, _p(work), _s()),
                'asr_gru_cell_fwd_ex')
    return gates, h_out, cell_out


def gru_cell_bwd(dcell, dh_c, gates, h_prev, W3, W_c, live, out_mask=None, dh_c2=None):
    """One GRU decoder cell step backwards (asr_gru_cell_bwd).  Returns (dpre [B,3U] = dr | du | dp pre-activation
    gradients, dh_prev_carry [B,U] -- WITHOUT d_in's h-columns --, d_in [B,Din])."""
    h = _h(dcell)
    B, U = dcell.shape
    Din = W_c.shape[0]
    dev = dcell.device
    for t, n in ((dcell, 'dcell'), (dh_c, 'dh_c'), (gates, 'gates'), (h_prev, 'h_prev'), (W3, 'W3'), (W_c, 'W_c'), (live, 'live')):
        _chk(t, torch.float32, n)
    p2, ld2 = _col_block(dh_c2, B, U, 'dh_c2')
    dpre, carry, d_in, work = _f32((B, 3 * U), dev), _f32((B, U), dev), _f32((B, Din), dev), _f32((2, B, U), dev)
    W_ch = C.c_void_p(W_c.data_ptr() + (Din - U) * U * 4)
    h.check(h.lib.asr_gru_cell_bwd(h.h, _p(dcell), _p(dh_c), p2, ld2, _p(out_mask), _p(live), _p(gates), _p(h_prev), _p(W3),
                                   W_ch, B, Din, U, _p(dpre), _p(carry), _p(d_in), Din, _p(work), _s()), 'asr_gru_cell_bwd')
    return dpre, carry, d_in


# ---------------------------------------------------------------- multi-layer LSTM decoder (decoder_num_layers > 1)
STACK_BWD_FUSED = os.environ.get('ASR_DEC_STACK_FUSED', '1') != '0'   # A/B: 0 keeps every backward step on the generic form
ATT_STACK_MAX = 7                                                     # upper layers (ASR_ATT_STACK_MAX)


class _AttStackLayer(C.Structure):
    """struct asr_att_stack_layer (include/asr_hip.h), field for field."""
    _PTRS = ['W', 'b', 'peep', 'dmask', 'in', 'c', 'h', 'gates', 'craw', 'W_il', 'dpre', 'd_hin', 'dpeep', 'dc0', 'dh0']
    _fields_ = [(n, C.c_void_p) for n in _PTRS]


class _AttStack(C.Structure):
    """struct asr_att_stack (include/asr_hip.h), field for field."""
    _fields_ = [('L', C.c_int), ('fused', C.c_int), ('up', _AttStackLayer * ATT_STACK_MAX), ('work', C.c_void_p)]


def _att_stack_struct(a, bwd=False):
    """The stack block of a loop dict: a['stack'] = dict(layers=[one dict per upper layer, layer 1 first, with the fields of
    asr_att_stack_layer as contiguous fp32 device tensors or None], fused (optional; False: the generic backward form at
    every shape), work (made here for the backward when missing)).  W_il, the work space of a layer's interleaved image,
    is made here where the one-launch forward covers the shape."""
    sd = a['stack']
    layers = sd['layers']
    U, B, To = int(a['U']), int(a['B']), int(a['To'])
    if not 1 <= len(layers) <= ATT_STACK_MAX:
        raise ValueError('att_decoder (stack): 1 .. %d upper layers, got %d' % (ATT_STACK_MAX, len(layers)))
    dev = a['dec_in'].device
    h = _h(a['dec_in'])
    need = ['W', 'b', 'in', 'c', 'h', 'gates', 'craw'] + (['dpre', 'd_hin', 'dc0', 'dh0'] if bwd else [])
    k = _AttStack()
    k.L = len(layers) + 1
    k.fused = int(bool(sd.get('fused', True)) and STACK_BWD_FUSED)
    for i, ld in enumerate(layers):
        if tuple(ld['W'].shape) != (2 * U, 4 * U) or tuple(ld['b'].shape) != (4 * U,):
            raise ValueError('att_decoder (stack): layer %d: W [2U,4U], b [4U]' % (i + 1))
        if bwd and ld.get('peep') is not None and ld.get('dpeep') is None:
            raise ValueError('att_decoder (stack): layer %d: dpeep is needed with peepholes' % (i + 1))
        if ld.get('W_il') is None and FUSED_CELL_GEMM and h.lib.asr_lstm_cell_gemm_ok(B, 2 * U, U, 2 * U):
            ld['W_il'] = _f32(((2 * U + 1) * 4 * U,), dev)
        for n in _AttStackLayer._PTRS:
            t = ld.get(n)
            if t is None:
                if n in need:
                    raise ValueError('att_decoder (stack): layer %d: %s is missing' % (i + 1, n))
                continue
            if not t.is_cuda or not t.is_contiguous() or t.dtype != torch.float32:
                raise ValueError('att_decoder (stack): layer %d: %s must be a contiguous fp32 device tensor' % (i + 1, n))
            setattr(k.up[i], n, t.data_ptr())
    if bwd:
        if sd.get('work') is None:
            sd['work'] = _f32((len(layers) * 4 * B * U + B * U,), dev)
        k.work = sd['work'].data_ptr()
    return k


def att_stack_bwd_ok(B, U):
    """Whether the one-launch backward of a lower layer (dx product + cell backward) covers the shape
    (asr_att_stack_bwd_ok): B <= 32, U % 16 == 0."""
    from . import _lib
    return bool(_lib.load().asr_att_stack_bwd_ok(int(B), int(U)))


def att_stack_bwd_step(dpre_up, W_up, dc_next, dh_next, gates, c_raw, c_prev, live, peep=None, use_mask=None, dh_next2=None,
                       fused=True, want_dpeep=None):
    """The backward of one lower layer of a decoder stack at one step (asr_att_stack_bwd_step): dx = dpre_up [B,4U] W_up^T
    ([2U,4U]); the cell backward on dx[:, :U] * use_mask with the carried dc_next / dh_next (+ dh_next2 [B,U]).  Returns
    (dpre [B,4U], dc_prev, dh_prev_carry, d_hin_up = dx[:, U:], dpeep_rows [B,3U] or None), every output prefilled with
    NaN.  fused: the one-launch form where att_stack_bwd_ok."""
    h = _h(dpre_up)
    B, U = dc_next.shape
    dev = dpre_up.device
    for t, n in ((dpre_up, 'dpre_up'), (W_up, 'W_up'), (dc_next, 'dc_next'), (dh_next, 'dh_next'), (gates, 'gates'),
                 (c_raw, 'c_raw'), (c_prev, 'c_prev'), (live, 'live')):
        _chk(t, torch.float32, n)
    if tuple(dpre_up.shape) != (B, 4 * U) or tuple(W_up.shape) != (2 * U, 4 * U) or tuple(gates.shape) != (B, 4 * U):
        raise ValueError('att_stack_bwd_step: shapes disagree')
    nan = lambda *shape: torch.full(shape, float('nan'), dtype=torch.float32, device=dev)   # noqa: E731
    dpre, dc_prev, carry, d_hin = nan(B, 4 * U), nan(B, U), nan(B, U), nan(B, U)
    want = (peep is not None) if want_dpeep is None else want_dpeep
    dpeep = nan(B, 3 * U) if want else None
    work = _f32((B, U), dev)
    p2, ld2 = _col_block(dh_next2, B, U, 'dh_next2')
    h.check(h.lib.asr_att_stack_bwd_step(h.h, _p(dpre_up), _p(W_up), B, U, _p(dc_next), _p(dh_next), p2, ld2, _p(gates),
                                         _p(c_raw), _p(c_prev), _p(peep), _p(live), _p(use_mask), _p(dpre), _p(dc_prev),
                                         _p(carry), _p(dpeep), _p(d_hin), _p(work), int(bool(fused) and STACK_BWD_FUSED),
                                         _s()), 'asr_att_stack_bwd_step')
    return dpre, dc_prev, carry, d_hin, dpeep


def att_stack_reorder(parent, c, h, in_):
    """Beam re-ordering of a stack's upper layers in one launch (asr_att_stack_reorder): c / h: lists of [2,R,U], in_: list of
    [2,R,2U]; parent [B,W] int32.  Block 0 row b*W + w (of in_: its columns [U,2U)) becomes block 1 row b*W + parent[b,w]."""
    hd = _h(c[0])
    B, W = parent.shape
    U = c[0].shape[2]
    _chk(parent, torch.int32, 'parent')
    k = _AttStack()
    k.L = len(c) + 1
    for i, (ci, hi, xi) in enumerate(zip(c, h, in_)):
        for t, shape, n in ((ci, (2, B * W, U), 'c'), (hi, (2, B * W, U), 'h'), (xi, (2, B * W, 2 * U), 'in')):
            _chk(t, torch.float32, n)
            if tuple(t.shape) != shape:
                raise ValueError('att_stack_reorder: %s must be %r' % (n, shape))
        k.up[i].c, k.up[i].h = ci.data_ptr(), hi.data_ptr()
        setattr(k.up[i], 'in', xi.data_ptr())
    hd.check(hd.lib.asr_att_stack_reorder(hd.h, C.byref(k), _p(parent), B, W, U, _s()), 'asr_att_stack_reorder')


# ---------------------------------------------------------------- shallow fusion with an RNN language model (an extension)
def _check_lm_weight(lm_weight):
    mu = float(lm_weight)
    if not (mu > 0.0 and mu != float('inf')):
        raise ValueError('lm_weight must be a finite number > 0 here (0 is the search without a language model), got %r'
                         % (lm_weight,))
    return mu


class _AttLm(C.Structure):
    """struct asr_att_lm (include/asr_hip.h), field for field."""
    _INTS = ['L', 'H', 'Em_lm', 'R', 'C2']
    _PTRS = ['emb', 'W', 'b', 'W_out', 'b_out', 'W_il', 'c', 'h', 'in', 'live', 'work', 'lm_logits', 'lm_score', 'cand',
             'cand_total', 'cand_lm']
    _fields_ = ([(n, C.c_int) for n in _INTS] + [('cell_clip', C.c_float), ('lm_weight', C.c_float)] +
                [(n, C.c_void_p) for n in _PTRS])


def lm_in_layers(flat, R, Em_lm, H, L):
    """The per-layer views [R, Din_l + H] (x | h_prev) of a language model's cell-input rows (struct asr_att_lm's `in`)."""
    views, o = [], 0
    for l in range(L):
        wdt = (Em_lm if l == 0 else H) + H
        views.append(flat[o:o + R * wdt].view(R, wdt))
        o += R * wdt
    return views


def _lm_struct(lm, R, W, lm_weight):
    """struct asr_att_lm and the tensors behind it for R device rows.  `lm`: dict(emb [C2,Em_lm], kernels = L tensors
    [Din_l + H, 4H], biases = L tensors [4H], W_out [H,C2], b_out [C2], cell_clip) -- RNNLM.decode_weights().  The state is
    that of the empty history: c, h zeros, the layer-0 input the embedding of lm['sos'] (when given)."""
    emb, kernels, biases = lm['emb'], list(lm['kernels']), list(lm['biases'])
    dev = emb.device
    L, H = len(kernels), int(biases[0].numel()) // 4
    C2, Em = (int(v) for v in emb.shape)
    for t, n in [(emb, 'emb'), (lm['W_out'], 'W_out'), (lm['b_out'], 'b_out')] + [(k, 'kernel') for k in kernels] + \
            [(b, 'bias') for b in biases]:
        _chk(t, torch.float32, 'lm ' + n)
    for l, k in enumerate(kernels):
        if tuple(k.shape) != ((Em if l == 0 else H) + H, 4 * H):
            raise ValueError('language model: kernel of layer %d is %s' % (l, tuple(k.shape)))
    if tuple(lm['W_out'].shape) != (H, C2) or tuple(lm['b_out'].shape) != (C2,):
        raise ValueError('language model: the output layer does not fit [%d,%d]' % (H, C2))
    n_in = R * (Em + H) + (L - 1) * R * 2 * H
    n_il = (Em + H + 1) * 4 * H + (L - 1) * (2 * H + 1) * 4 * H
    t = dict(emb=emb, W=torch.cat([k.reshape(-1) for k in kernels]), b=torch.stack(biases).contiguous(), W_out=lm['W_out'],
             b_out=lm['b_out'], W_il=_f32((n_il,), dev) if FUSED_CELL_GEMM else None,
             c=torch.zeros((2, L, R, H), dtype=torch.float32, device=dev),
             h=torch.zeros((2, L, R, H), dtype=torch.float32, device=dev),
             live=torch.ones((R,), dtype=torch.float32, device=dev), work=_f32((R * 10 * H,), dev),
             lm_logits=_f32((R, C2), dev), lm_score=torch.zeros((R,), dtype=torch.float32, device=dev),
             cand=_i32((R, W + 1), dev), cand_total=_f32((R, W + 1), dev), cand_lm=_f32((R, W + 1), dev))
    t['in'] = torch.zeros((n_in,), dtype=torch.float32, device=dev)
    if lm.get('sos') is not None:
        lm_in_layers(t['in'], R, Em, H, L)[0][:, :Em] = emb[int(lm['sos'])]
    st = _AttLm()
    st.L, st.H, st.Em_lm, st.R, st.C2 = L, H, Em, R, C2
    st.cell_clip, st.lm_weight = float(lm.get('cell_clip') or 0.0), float(lm_weight)
    for n in _AttLm._PTRS:
        setattr(st, n, t[n].data_ptr() if t[n] is not None else None)
    return st, t


def lm_step(lm, words, c, h):
    """One language model step on R rows (asr_lm_prep + asr_lm_step): words [R] int32 (each row's last word), c / h
    [L,R,H] the state before the step.  Returns (lm_logits [R,C2] raw, c_new, h_new [L,R,H])."""
    hd = _h(c)
    _chk(words, torch.int32, 'words')
    _chk(c, torch.float32, 'c')
    _chk(h, torch.float32, 'h')
    L, R, H = (int(v) for v in c.shape)
    st, t = _lm_struct(lm, R, 1, 1.0)
    if st.L != L or st.H != H or tuple(h.shape) != tuple(c.shape) or tuple(words.shape) != (R,):
        raise ValueError('lm_step: state [%d,%d,%d] does not fit the language model' % (L, R, H))
    t['c'][0].copy_(c)
    t['h'][0].copy_(h)
    ins = lm_in_layers(t['in'], R, st.Em_lm, H, L)
    ins[0][:, :st.Em_lm] = lm['emb'].index_select(0, words.long().clamp(0, st.C2 - 1))
    for l in range(L):
        ins[l][:, -H:] = h[l]
    hd.check(hd.lib.asr_lm_prep(hd.h, C.byref(st), _s()), 'asr_lm_prep')
    hd.check(hd.lib.asr_lm_step(hd.h, C.byref(st), _s()), 'asr_lm_step')
    return t['lm_logits'], t['c'][1], t['h'][1]


def att_beam_select_fused(logits, lm_logits, n_labels, lm_weight, length_penalty_weight, first_step, log_probs, finished,
                          lengths, lm_score, beam_width=None, ctc_weight=0.0, y=None, seq_len=None, r=None, last=None,
                          ctc_score=None, unfinished=None, blank=None):
    """One selection per utterance on fused attention / LM (/ CTC prefix) scores (asr_att_beam_select_fused):
    ((1 - ctc_weight) * total_att + ctc_weight * ctc + lm_weight * lm_total) / penalty over the W + 1 classes per slot that
    p_att + lm_weight * p_lm preselects.  logits / lm_logits [B*W, n_labels + 2] raw; log_probs, lm_score [B*W] fp32,
    finished, lengths [B*W] int32; beam_width W (needed without CTC; with it W = rows / utterances); with ctc_weight > 0
    also y / seq_len / r / last / ctc_score as att_beam_select_joint.
    Nothing is changed in place.  Returns word, parent [B,W] int32, score [B,W], and the next state log_probs, finished,
    lengths, lm_score [B*W], last, ctc_score [B*W] (None, None without CTC)."""
    h = _h(logits)
    _chk(logits, torch.float32, 'logits')
    _chk(lm_logits, torch.float32, 'lm_logits')
    R, C2 = (int(v) for v in logits.shape)
    N = int(n_labels)
    if C2 != N + 2 or tuple(lm_logits.shape) != (R, C2):
        raise ValueError('att_beam_select_fused: logits %s / lm_logits %s for %d labels' % (tuple(logits.shape),
                                                                                        tuple(lm_logits.shape), N))
    mu = _check_lm_weight(lm_weight)
    lam = float(ctc_weight)
    if not 0.0 <= lam <= 1.0:
        raise ValueError('ctc_weight must be in [0, 1], got %r' % (ctc_weight,))
    state = [(log_probs, torch.float32, 'log_probs'), (lm_score, torch.float32, 'lm_score'), (finished, torch.int32, 'finished'),
             (lengths, torch.int32, 'lengths')]
    ctc = None
    if lam > 0.0:
        B, W, T, By, Cc, blank = _joint_shapes('att_beam_select_fused', y, seq_len, R, N, blank)
        _chk_state('att_beam_select_fused', r, last, T)
        if r.shape[0] != R or (beam_width is not None and int(beam_width) != W):
            raise ValueError('att_beam_select_fused: r must have %d rows' % R)
        state.append((ctc_score, torch.float32, 'ctc_score'))
        ctc = (y, seq_len, r, last, T, By, Cc, blank)
    else:
        if beam_width is None:
            raise ValueError('att_beam_select_fused: without CTC posteriors beam_width must be given')
        W = int(beam_width)
        if W < 1 or R % W:
            raise ValueError('att_beam_select_fused: %d rows are not a multiple of beam_width %d' % (R, W))
    return _select_streams('att_beam_select_fused', h, logits, lm_logits, N, W, lam, mu, length_penalty_weight, first_step,
                           state, ctc, unfinished)


def lm_beam_reorder(parent, word, c_src, h_src, emb):
    """The language model state the next step reads, gathered by parent within each utterance (asr_lm_beam_reorder): parent /
    word [B,W] int32, c_src / h_src [L,B*W,H], emb [C2,Em_lm].  Returns new c, h [L,B*W,H] and the per-layer cell-input
    rows [B*W, Din_l + H] (x | h_prev; x of layer 0 = emb[word], x of the layers above is not written here: zeros)."""
    hd = _h(c_src)
    for t, dt, n in ((parent, torch.int32, 'parent'), (word, torch.int32, 'word'), (c_src, torch.float32, 'c_src'),
                     (h_src, torch.float32, 'h_src'), (emb, torch.float32, 'emb')):
        _chk(t, dt, n)
    B, W = (int(v) for v in parent.shape)
    L, R, H = (int(v) for v in c_src.shape)
    Em = int(emb.shape[1])
    if R != B * W or tuple(h_src.shape) != tuple(c_src.shape) or tuple(word.shape) != (B, W):
        raise ValueError('lm_beam_reorder: shapes disagree')
    c, hh = torch.empty_like(c_src), torch.empty_like(h_src)
    flat = torch.zeros((R * (Em + H) + (L - 1) * R * 2 * H,), dtype=torch.float32, device=c_src.device)
    hd.check(hd.lib.asr_lm_beam_reorder(hd.h, _p(parent), _p(word), B, W, L, H, Em, int(emb.shape[0]), _p(c_src), _p(h_src),
                                        _p(emb), _p(c), _p(hh), _p(flat), _s()), 'asr_lm_beam_reorder')
    return c, hh, lm_in_layers(flat, R, Em, H, L)


def att_decoder_beam_lm(a, W_av, W_out, b_out, embedding, eos, beam_width, lm, lm_weight, length_penalty_weight=0.0,
                        check_every=8, y=None, seq_len=None, ctc_weight=0.0, blank=None):
    """Beam search decode with shallow LM fusion from one call (asr_att_decoder_beam_lm): att_decoder_beam -- or, with
    ctc_weight > 0 and y / seq_len, att_decoder_beam_joint -- whose every step also runs one step of the language model
    `lm` (dict: see RNNLM.decode_weights; its images are prepared once, before the first step) and selects on the fused
    score.  Returns that loop's dict and lm_score [B,W], the hypotheses' LM log-probabilities."""
    R = a['B']
    C2 = int(W_out.shape[1])
    N = C2 - 2
    if int(eos) != N + 1:
        raise ValueError('att_decoder_beam_lm: <EOS> must be the last of the %d attention classes' % C2)
    W = _beam_width(beam_width, N + 1)
    mu = _check_lm_weight(lm_weight)
    lam = float(ctc_weight)
    if not 0.0 <= lam <= 1.0:
        raise ValueError('ctc_weight must be in [0, 1], got %r' % (ctc_weight,))
    if R % W:
        raise ValueError('att_decoder_beam_lm: %d rows are not a multiple of beam_width %d' % (R, W))
    if int(lm['emb'].shape[0]) != C2:
        raise ValueError('att_decoder_beam_lm: the language model has %d classes, the decoder %d' % (int(lm['emb'].shape[0]), C2))
    B = R // W
    lst, lt = _lm_struct(dict(lm, sos=N), R, W, mu)
    extra_out = dict(lm_score=lt['lm_score'].view(B, W))
    extra = dict(lm=lt)
    j = None
    if lam > 0.0:
        ctc_scratch, extra_out['ctc_score'], j = _beam_ctc('att_decoder_beam_lm', a, y, seq_len, W, N, lam, blank)
        extra.update(ctc_scratch)
    h, st, f, m, out, scratch, host = _beam_loop_call('att_decoder_beam_lm', a, W_av, W_out, b_out, embedding, eos, W,
                                                      length_penalty_weight, check_every, extra_out=extra_out,
                                                      extra_scratch=extra)
    issued = C.c_int(0)
    h.check(h.lib.asr_att_decoder_beam_lm(h.h, C.byref(st), C.byref(f), C.byref(m), C.byref(j) if j is not None else None,
                                          C.byref(lst), C.byref(issued), _s()), 'asr_att_decoder_beam_lm')
    return _beam_loop_done(out, issued, host, scratch)


# ------------------------------------------------- CTC prefix beam search with LM fusion / insertion bonus (an extension)
def _ctc_lm_args(who, logits, seq_len, beam_width, lm_weight, insertion_bonus, blank):
    _chk(logits, torch.float32, 'logits')
    _chk(seq_len, torch.int32, 'seq_len')
    T, B, Cc = (int(v) for v in logits.shape)
    W = int(beam_width)
    if W < 1 or W > MAX_BEAM_WIDTH or W > Cc - 1:
        raise ValueError('%s: beam_width must be in 1 .. min(%d, C - 1 = %d), got %d' % (who, MAX_BEAM_WIDTH, Cc - 1, W))
    alpha, beta = float(lm_weight), float(insertion_bonus)
    if not (math.isfinite(alpha) and math.isfinite(beta)):
        raise ValueError('%s: lm_weight / insertion_bonus must be finite, got %r / %r' % (who, lm_weight, insertion_bonus))
    return T, B, Cc, W, alpha, beta, Cc - 1 if blank is None else int(blank)


def _ctc_lm_check(lm, Cc):
    """The LM must be fp32, have V >= C + 1 classes and keep <SOS> / <EOS> out of the CTC labels 0 .. C-2."""
    if lm['emb'].dtype != torch.float32:
        raise ValueError('ctc_beam_decode_lm: the language model must be fp32, got %s' % lm['emb'].dtype)
    V = int(lm['emb'].shape[0])
    if V < Cc + 1:
        raise ValueError('ctc_beam_decode_lm: the language model has %d classes, a CTC model of %d classes needs >= %d'
                         % (V, Cc, Cc + 1))
    if lm.get('sos') is None:
        raise ValueError("ctc_beam_decode_lm: the language model dict needs 'sos'")
    for k in ('sos', 'eos'):
        if lm.get(k) is not None and not Cc - 1 <= int(lm[k]) < V:
            raise ValueError('ctc_beam_decode_lm: <%s> = %d of the language model lies inside the CTC labels 0 .. %d'
                             % (k.upper(), int(lm[k]), Cc - 2))
    return V


def ctc_beam_decode_lm(logits, seq_len, beam_width, lm=None, lm_weight=0.0, insertion_bonus=0.0, blank=None, _poison=False):
    """Prefix beam search with shallow LM fusion and an insertion bonus from one call (asr_ctc_beam_decode_lm; the float64
    statement is models/ctc/decoders/charlm_beam_search_decoder.py): every extension of a prefix by a label c uses
    p_t + lm_weight * log p_lm(c | <SOS>, prefix) + insertion_bonus in place of p_t.  logits [T,B,C] fp32; lm:
    RNNLM.decode_weights() (fp32, V >= C + 1 classes, 'sos' -- and 'eos' when given -- outside the CTC labels) or None
    (lm_weight must then be 0).  1 <= beam_width <= 32, <= C - 1.  Returns (labels [B,T] int32 padded -1, lengths [B],
    scores [B] float64 = -log of the best prefix' fused total, lm_score [B] fp32 = its sum of log p_lm).
    _poison (tests): the workspace starts as NaN bit patterns."""
    T, B, Cc, W, alpha, beta, blank = _ctc_lm_args('ctc_beam_decode_lm', logits, seq_len, beam_width, lm_weight,
                                                   insertion_bonus, blank)
    if lm is None and alpha != 0.0:
        raise ValueError('ctc_beam_decode_lm: lm_weight = %r needs a language model' % (lm_weight,))
    V = _ctc_lm_check(lm, Cc) if lm is not None else 0
    h = _h(logits)                                              # (after the argument checks: they hold without a device)
    dev = logits.device
    lst, keep = _lm_struct(lm, B * W, W, 1.0) if lm is not None else (None, None)
    nbytes = h.lib.asr_ctc_beam_lm_workspace_bytes(T, B, Cc, W, V)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    if _poison:
        ws.fill_(0xFF)
    out, n = _i32((B, T), dev), _i32((B,), dev)
    score = torch.empty((B,), dtype=torch.float64, device=dev)
    lm_score = _f32((B,), dev)
    h.check(h.lib.asr_ctc_beam_decode_lm(h.h, _p(logits), T, B, Cc, _p(seq_len), blank, W, alpha, beta,
                                         C.byref(lst) if lst is not None else None, _p(out), _p(n), _p(score), _p(lm_score),
                                         _p(ws), nbytes, _s()), 'asr_ctc_beam_decode_lm')
    return out, n, score, lm_score


class CtcBeamLmFrames(object):
    """The one-frame form of ctc_beam_decode_lm (asr_ctc_beam_lm_frame), for tests and probes: the caller supplies each
    slot's LM logits row.  frame(t, lm_logits [B*W,V] fp32 or None) must be called for t = 0, 1, ... in order; returns
    (parent [B,W], word [B,W] int32, p_b, p_nb [B,W] float64, lm_total [B,W] fp32, entries [B] int32) of the new beam
    (state rows of an utterance past its seq_len, and slots >= entries, are not written)."""

    def __init__(self, logits, seq_len, beam_width, lm_weight=0.0, insertion_bonus=0.0, blank=None):
        self.h = _h(logits)
        self.logits, self.seq_len = logits, seq_len
        self.T, self.B, self.C, self.W, self.alpha, self.beta, self.blank = _ctc_lm_args(
            'CtcBeamLmFrames', logits, seq_len, beam_width, lm_weight, insertion_bonus, blank)
        self.nbytes = self.h.lib.asr_ctc_beam_lm_workspace_bytes(self.T, self.B, self.C, self.W, 0)
        self.ws = torch.empty((self.nbytes,), dtype=torch.uint8, device=logits.device)

    def frame(self, t, lm_logits=None):
        B, W, dev = self.B, self.W, self.logits.device
        V = 0
        if lm_logits is not None:
            _chk(lm_logits, torch.float32, 'lm_logits')
            V = int(lm_logits.shape[1])
            if tuple(lm_logits.shape) != (B * W, V) or V < self.C:
                raise ValueError('CtcBeamLmFrames: lm_logits must be [%d, V >= %d]' % (B * W, self.C))
        elif self.alpha != 0.0:
            raise ValueError('CtcBeamLmFrames: lm_weight = %r needs LM logits' % (self.alpha,))
        parent, word, nb = _i32((B, W), dev), _i32((B, W), dev), torch.zeros((B,), dtype=torch.int32, device=dev)
        pb = torch.zeros((B, W), dtype=torch.float64, device=dev)
        pnb = torch.zeros((B, W), dtype=torch.float64, device=dev)
        lmt = torch.zeros((B, W), dtype=torch.float32, device=dev)
        h = self.h
        h.check(h.lib.asr_ctc_beam_lm_frame(h.h, _p(self.logits), int(t), self.T, B, self.C, _p(self.seq_len), self.blank, W,
                                            self.alpha, self.beta, _p(lm_logits), V, _p(parent), _p(word), _p(pb), _p(pnb),
                                            _p(lmt), _p(nb), _p(self.ws), self.nbytes, _s()), 'asr_ctc_beam_lm_frame')
        return parent, word, pb, pnb, lmt, nb


def tanh_fwd(x):
    h = _h(x)
    y = torch.empty_like(x)
    h.check(h.lib.asr_tanh_fwd(h.h, _p(x), _p(y), x.numel(), _s()), 'asr_tanh_fwd')
    return y


def tanh_bwd(dy, y):
    h = _h(dy)
    dx = torch.empty_like(dy)
    h.check(h.lib.asr_tanh_bwd(h.h, _p(dy), _p(y), _p(dx), dy.numel(), _s()), 'asr_tanh_bwd')
    return dx


def embedding_gather(W, ids):
    h = _h(W)
    _chk(ids, torch.int32, 'ids')
    out = _f32(tuple(ids.shape) + (W.shape[1],), W.device)
    h.check(h.lib.asr_embedding_gather(h.h, _p(W), _p(ids), ids.numel(), W.shape[1], _p(out), _s()),
            'asr_embedding_gather')
    return out


def embedding_scatter(dout, ids, vocab, out):
    h = _h(dout)
    E = dout.shape[-1]
    h.check(h.lib.asr_embedding_scatter(h.h, _p(dout), _p(ids), ids.numel(), E, int(vocab), _p(out), _s()),
            'asr_embedding_scatter')
    return out


def seq_xent(logits2d, targets, weights, eps, dscale, want_grad=True, smoothing=0.0):
    """smoothing > 0 (label_smoothing_prob): the target is (1 - smoothing) * onehot + smoothing / C (asr_seq_xent_ls);
    0 is asr_seq_xent, untouched."""
    if float(smoothing) > 0.0:
        return seq_xent_ls(logits2d, targets, weights, eps, smoothing, dscale, want_grad=want_grad)
    if float(smoothing) != 0.0:
        raise ValueError('smoothing must be in [0, 1), got %r' % (smoothing,))
    h = _h(logits2d)
    rows, Cc = logits2d.shape
    row_loss = _f32((rows,), logits2d.device)
    dl = torch.empty_like(logits2d) if want_grad else None
    h.check(h.lib.asr_seq_xent(h.h, _p(logits2d), _p(targets), _p(weights), rows, Cc, float(eps), float(dscale),
                               _p(row_loss), _p(dl), _s()), 'asr_seq_xent')
    return row_loss, dl


def seq_xent_ls(logits2d, targets, weights, eps, smoothing, dscale, want_grad=True):
    """asr_seq_xent_ls: the masked sequence cross-entropy against (1 - smoothing) * onehot + smoothing / C, 0 <= smoothing < 1."""
    smoothing = float(smoothing)
    if not 0.0 <= smoothing < 1.0:
        raise ValueError('smoothing must be in [0, 1), got %r' % (smoothing,))
    h = _h(logits2d)
    rows, Cc = logits2d.shape
    row_loss = _f32((rows,), logits2d.device)
    dl = torch.empty_like(logits2d) if want_grad else None
    h.check(h.lib.asr_seq_xent_ls(h.h, _p(logits2d), _p(targets), _p(weights), rows, Cc, float(eps), smoothing,
                                  float(dscale), _p(row_loss), _p(dl), _s()), 'asr_seq_xent_ls')
    return row_loss, dl


def argmax_rows(x2d):
    h = _h(x2d)
    out = torch.empty((x2d.shape[0],), dtype=torch.int32, device=x2d.device)
    h.check(h.lib.asr_argmax_rows(h.h, _p(x2d), x2d.shape[0], x2d.shape[1], _p(out), _s()), 'asr_argmax_rows')
    return out


# ---------------------------------------------------------------- clip / decay / optimizers
class ClipPlan(object):
    """Device-side description of a flat fp32 parameter buffer split into tensors."""

    NORM_CHUNK = 4096   # == NORM_CHUNK in csrc/elementwise.hip (asr_clip_plan computes the same table)

    def __init__(self, offsets_host, device):
        off = np.asarray(offsets_host, dtype=np.int64)
        self.num_tensors = len(off) - 1
        cs = np.zeros(self.num_tensors + 1, dtype=np.int64)
        device = torch.device(device)
        if device.type == 'cuda':
            lib = _lib.load()
            hd = _lib.handle(device.index or 0)
            hd.check(lib.asr_clip_plan(hd.h, off.ctypes.data_as(C.c_void_p), self.num_tensors,
                                       cs.ctypes.data_as(C.c_void_p)), 'asr_clip_plan')
        else:   # host-only bookkeeping (CPU tests of the data-parallel logic); kernels still need a GPU
            cs[1:] = np.cumsum((np.diff(off) + self.NORM_CHUNK - 1) // self.NORM_CHUNK)
        self.total_chunks = int(cs[-1])
        self.offsets = torch.from_numpy(off).to(device)
        self.chunk_start = torch.from_numpy(cs).to(device)
        self.partial = torch.empty((max(self.total_chunks, 1),), dtype=torch.float32, device=device)


def clip_by_norm_multi(flat_grads, plan, clip_norm):
    h = _h(flat_grads)
    _chk(flat_grads, torch.float32, 'grads')
    h.check(h.lib.asr_clip_by_norm_multi(h.h, _p(flat_grads), _p(plan.offsets), _p(plan.chunk_start),
                                         plan.num_tensors, plan.total_chunks, float(clip_norm),
                                         _p(plan.partial), _s()), 'asr_clip_by_norm_multi')


def weight_decay(flat_grads, flat_params, plan, decay_mask, wd, l2_out=None):
    h = _h(flat_params)
    h.check(h.lib.asr_weight_decay(h.h, _p(flat_grads), _p(flat_params), _p(plan.offsets),
                                   _p(decay_mask), plan.num_tensors, float(wd), _p(l2_out), _s()),
            'asr_weight_decay')


def weight_noise_perturb(flat, backup, std, seed, offset):
    """EXTENSION: Gaussian weight noise for one training step (asr_weight_noise_perturb), in place and in one pass:
    backup[i] = flat[i], flat[i] += std * z[i] with z the standard normal values of the Philox blocks offset + i / 4 under
    key `seed` (the statement: include/asr_hip.h).  flat / backup: contiguous fp32 of one size that do not overlap; a view
    that starts at a multiple of 4 elements, with offset + start / 4, gets the bits of those elements of a whole-buffer
    call.  std >= 0 (0: the backup alone).  The clean weights come back with flat.copy_(backup)."""
    sd = float(std)
    if not (0.0 <= sd < float('inf')):
        raise ValueError('weight_noise_perturb: std must be finite and >= 0, got %r' % (std,))
    _chk(flat, torch.float32, 'flat')
    _chk(backup, torch.float32, 'backup')
    if backup.numel() != flat.numel():
        raise ValueError('weight_noise_perturb: backup has %d elements, flat %d' % (backup.numel(), flat.numel()))
    h = _h(flat)
    h.check(h.lib.asr_weight_noise_perturb(h.h, _p(flat), _p(backup), flat.numel(), sd, int(seed), int(offset), _s()),
            'asr_weight_noise_perturb')
    return flat


def input_augment(x, seq_len, n_ch, noise_std=0.0, freq_masks=(0, 0), time_masks=(0, 0, 1.0), mask_value=0.0, seed=0,
                  offset=0, out=None):
    """EXTENSION: input augmentation of one training step (asr_input_augment), one pass, x untouched: y = x with Gaussian
    noise of `noise_std` on every valid element, `freq_masks = (number, max width)` bands of the `n_ch` base channels
    (the same band in every group of n_ch columns) and `time_masks = (number, max width, max share of the utterance)`
    runs of frames per utterance set to `mask_value`; padded frames (t >= seq_len[b]) keep x's bits.  x [B,T,F] fp32
    contiguous, seq_len [B] int32 on the device; noise blocks offset + i / 4 and mask slots offset + 2^39 + 16 b + slot
    under key `seed` (the statement: include/asr_hip.h).  `out`: a [B,T,F] fp32 tensor that does not overlap x (default:
    a fresh one).  Everything off: a device copy.  Returns y."""
    _chk(x, torch.float32, 'x')
    if x.dim() != 3:
        raise ValueError('input_augment: x must be [B,T,F], got %s' % (tuple(x.shape),))
    B, T, F = x.shape
    h = _h(x)
    seq_len = to_device(seq_len, torch.int32, x.device)
    if seq_len.numel() != B:
        raise ValueError('input_augment: seq_len has %d entries for a batch of %d' % (seq_len.numel(), B))
    if out is None:
        out = torch.empty_like(x, memory_format=torch.contiguous_format)
    _chk(out, torch.float32, 'out')
    if tuple(out.shape) != tuple(x.shape):
        raise ValueError('input_augment: out is %s, x %s' % (tuple(out.shape), tuple(x.shape)))
    nf, fw = freq_masks
    nt, tw, tr = time_masks
    h.check(h.lib.asr_input_augment(h.h, _p(x), _p(out), _p(seq_len), B, T, F, int(n_ch), float(noise_std), int(nf),
                                    int(fw), int(nt), int(tw), float(tr), float(mask_value),
                                    int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF, _s()),
            'asr_input_augment')
    return out


def optimizer_step(opt_id, params, grads, slot0, slot1, lr, step):
    h = _h(params)
    h.check(h.lib.asr_optimizer_step(h.h, int(opt_id), _p(params), _p(grads), _p(slot0), _p(slot1),
                                     params.numel(), float(lr), int(step), _s()), 'asr_optimizer_step')


def scale_(x, s):
    h = _h(x)
    _chk(x, torch.float32, 'x')
    h.check(h.lib.asr_scale(h.h, _p(x), x.numel(), float(s), _s()), 'asr_scale')
    return x


# ---------------------------------------------------------------- data-parallel collective (RCCL through the C ABI)
class NativeComm(object):
    """asr_comm_* : one RCCL communicator per process / GPU, created from a 128-byte unique id that rank 0 generates
    (NativeComm.unique_id()) and the host program distributes.  allreduce_mean works in place on a flat fp32 cuda
    tensor, asynchronously on the current stream."""

    @staticmethod
    def _bind_library():
        import os
        lib = _lib.load()
        path = os.path.join(os.path.dirname(torch.__file__), 'lib', 'librccl.so')
        if os.path.exists(path):        # share the instance PyTorch has loaded
            lib.asr_comm_set_library(path.encode())
        return lib

    @staticmethod
    def unique_id():
        lib = NativeComm._bind_library()
        buf = C.create_string_buffer(128)
        rc = lib.asr_comm_unique_id(buf)
        if rc != 0:
            raise _lib.AsrError('asr_comm_unique_id failed (%d)' % rc)
        return bytes(buf.raw)

    def __init__(self, device, rank, world, unique_id):
        self._bind_library()
        self.h = _lib.handle(device)
        self.rank, self.world = int(rank), int(world)
        c = C.c_void_p()
        idbuf = C.create_string_buffer(bytes(unique_id), 128)
        self.h.check(self.h.lib.asr_comm_init(C.byref(c), self.h.h, self.rank, self.world, idbuf), 'asr_comm_init')
        self.c = c

    def allreduce_mean(self, flat):
        _chk(flat, torch.float32, 'buffer')
        if not flat.is_cuda or not flat.is_contiguous():
            raise ValueError('allreduce_mean: contiguous cuda tensor expected')
        self.h.check(self.h.lib.asr_allreduce_mean(self.c, _p(flat), flat.numel(), _s()), 'asr_allreduce_mean')
        return flat

    def close(self):
        if getattr(self, 'c', None):
            self.h.lib.asr_comm_destroy(self.c)
            self.c = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
