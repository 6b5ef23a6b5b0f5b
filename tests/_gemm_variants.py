"""TEST INFRASTRUCTURE of tests/test_gpu_gemm_variants.py, of its child-process worker (tests/_gemm_variant_worker.py) and
of the host test of the rule (tests/test_gemm_variants_host.py): the dispatch rule of csrc/gemm.hip (launch_gemm and the
try_gemm_* functions it asks first) restated in plain Python, and the check of one product against an fp64 reference
with the kernel counters (ops.gemm_kernel_counts) asserted call by call.

Two data regimes.
  exact:    A, B, bias and the prior C hold integers of [-8, 8], multipliers are 0 or 2 (keep probability 0.5).  Every
            partial sum in every accumulation order is an integer below 2^24 (K <= 262144), so an fp32 result EQUALS the
            fp64 reference and a bf16 result equals its round-to-nearest-even: tolerance zero, a dropped, doubled or
            misplaced k-term anywhere changes an integer.
  gaussian: randn operands (bf16 operands rounded first, the reference taken on the rounded values in fp64): what integer
            data cannot show, an operand that silently lost precision.  Bounds, per element against
            |A| @ |B| + |bias| + |C0|: 2e-6 (fp32 operands) and 1e-5 (bf16 operands, fp32 result) -- the figures
            tests/test_gpu_ops.py holds the same kernels to, there against the largest reference value; a bf16 result
            within one bf16 ulp (tests/_bf16_ulp.py), the convolution tests' criterion.

Every result is written into a guard-framed C: two rows above and below, four columns on either side (ldc = N + 8 or
more), filled with a sentinel that must survive.  gemm(drop=...) takes a contiguous C only: its frame is the rows.
The padding behind the rows of A and B (lda, ldb larger than the row) and the elements in front of an offset view hold
NaN: an operand element read from outside the matrix and used shows in the result."""
import hashlib

import torch

from _bf16_ulp import within_bf16_ulp

XCH_BYTES = 64 << 20                     # csrc/common.h: ASR_XCH_BYTES (tests/_conv_variants.py reads it back from there)
KERNEL_KEYS = ('skinny_nn16', 'skinny_nn32', 'skinny_nt16', 'skinny_nt32', 'nt128', 'nt256', 'tn_lean', 'generic128',
               'generic64', 'generic64_splitk')
PASS_KEYS = ('mul_pass', 'drop_pass')
ALL_KEYS = KERNEL_KEYS + PASS_KEYS
DROP = (0.5, 29, (3 << 32) + 5)          # keep_prob (scale 1 / 0.5 = 2, exact), seed, offset
SENTINEL = 12345.0                       # exact in bf16 and fp32
FORMS = ('plain', 'bias', 'accumulate', 'relu')
ROOM = (192 << 20) - XCH_BYTES           # scratch_room of a handle with asr_create's 192 MiB arena (the host test's figure)
TOL = {'f32': 2e-6, 'bf16': 1e-5}        # gaussian regime, fp32 result, per element of |A| @ |B| + |bias| + |C0|


# ---------------------------------------------------------------- the dispatch rule
def nt_big_switch(env):
    """ASR_GEMM_NT_BIG as try_gemm_nt_bf16 reads it (atoi; unset = 1)."""
    v = env.get('ASR_GEMM_NT_BIG')
    if v is None:
        return 1
    s = v.strip()
    sign, i = 1, 0
    if s[:1] in '+-' and s:
        sign, i = (-1 if s[0] == '-' else 1), 1
    j = i
    while j < len(s) and s[j].isdigit():
        j += 1
    return sign * int(s[i:j]) if j > i else 0


def _cdiv(a, b):
    return -(-a // b)


def gemm_plan(dtype, out_dtype, ta, tb, M, N, K, lda, ldb, ldc, a_off, b_off, c_off, bias, mul, ldm, drop, scratch_room,
              tn_wgs, big):
    """launch_gemm step by step.  dtype / out_dtype: 'f32' or 'bf16'; a_off, b_off, c_off: elements between a 16-byte
    boundary and the first element of A, B, C; bias, mul: None, or the same offset (in floats) of the vector / of the
    multiplier, whose row stride is ldm; drop: gemm(drop=...); scratch_room: the handle's scratch less the exchange area;
    tn_wgs: asr_set_gemm_tn_workgroups of the handle (0 = default); big: nt_big_switch.
    -> dict(keys = the counters the call bumps, S = split-K slabs (1: one pass), kchunk)."""
    es, eo = (4 if dtype == 'f32' else 2), (4 if out_dtype == 'f32' else 2)
    a16, b16 = (a_off * es) % 16 == 0, (b_off * es) % 16 == 0
    passes = (['mul_pass'] if mul is not None else []) + (['drop_pass'] if drop else [])
    assert not (passes and out_dtype != 'f32'), 'gemm(mul / drop) is an fp32-output entry point'
    if dtype == 'f32' and out_dtype == 'f32':
        if (not ta and 1 <= M <= 32 and K % 64 == 0 and N % 16 == 0 and K >= 64 and lda % 4 == 0 and a16 and b16
                and (not tb or ldb % 4 == 0)):
            wide = N % 32 == 0 and (not tb or N >= 32 * 192)
            key = 'skinny_n%s%d' % ('t' if tb else 'n', 32 if wide else 16)
            return dict(keys=[key] + passes, S=1, kchunk=K)
    if dtype == 'bf16':
        nt = not ta and tb and K % 64 == 0 and N % 128 == 0 and M >= 1024
        nt = nt and not (drop and eo != 4)
        nt = nt and (mul is None or (eo == 4 and ldm % 4 == 0 and (mul * 4) % 16 == 0))
        nt = nt and lda % 8 == 0 and ldb % 8 == 0 and a16 and b16
        nt = nt and ldc % 4 == 0 and (c_off * eo) % (4 * eo) == 0 and (bias is None or (bias * 4) % 16 == 0)
        if nt:
            assert ((M - 1) * lda + K) * 2 < 0xFFFFFFFF and ((N - 1) * ldb + K) * 2 < 0xFFFFFFFF   # fits32: not modelled
            tiles256 = (N // 256) * _cdiv(M, 256)
            use_big = bool(big) and N % 256 == 0 and (M >= 2048 if big == 2 else tiles256 >= 512)
            return dict(keys=['nt256' if use_big else 'nt128'], S=1, kchunk=K)     # multiplier / dropout in the epilogue
        if ta and not tb and K >= 2048 and M % 8 == 0 and N % 8 == 0 and lda % 8 == 0 and ldb % 8 == 0 and a16 and b16:
            tiles = _cdiv(M, 128) * _cdiv(N, 128)
            S = min(_cdiv(tn_wgs if tn_wgs > 0 else 512, tiles), _cdiv(K, 256), 256)
            while S > 1 and S * M * N * 4 > scratch_room:
                S -= 1
            if S * M * N * 4 <= scratch_room:
                kchunk = _cdiv(_cdiv(K, S), 64) * 64
                return dict(keys=['tn_lean'] + passes, S=_cdiv(K, kchunk), kchunk=kchunk)
    if _cdiv(M, 128) * _cdiv(N, 128) >= 320:
        return dict(keys=['generic128'] + passes, S=1, kchunk=K)
    BK = 32 if dtype == 'f32' else 64
    tiles64 = _cdiv(M, 64) * _cdiv(N, 64)
    S = 1
    if tiles64 < 256 and K >= 16 * BK:
        S = min(_cdiv(512, tiles64), K // (4 * BK), 64)
        while S > 1 and S * M * N * 4 > scratch_room:
            S -= 1
    if S <= 1:
        return dict(keys=['generic64'] + passes, S=1, kchunk=K)
    kchunk = _cdiv(_cdiv(K, S), BK) * BK
    return dict(keys=['generic64_splitk'] + passes, S=_cdiv(K, kchunk), kchunk=kchunk)


def expected_gemm(*args, **kw):
    """The counters one ops.gemm call bumps (gemm_plan's arguments)."""
    return gemm_plan(*args, **kw)['keys']


# ---------------------------------------------------------------- one product and its operands
class Case(object):
    """One product: dtype 'f32' / 'bf16' operands, layout (ta, tb), shape, and where the operands sit in memory.
    lda / ldb / ldm: None = the row itself; ldc_extra: columns added to the right guard (ldc = N + 8 + ldc_extra);
    a_off / b_off / bias_off / mul_off: elements the view starts into its (aligned) buffer."""

    def __init__(self, dtype, ta, tb, M, N, K, lda=None, ldb=None, a_off=0, b_off=0, ldc_extra=0, bias_off=0, ldm=None,
                 mul_off=0, note=''):
        self.dtype, self.ta, self.tb, self.M, self.N, self.K = dtype, int(ta), int(tb), M, N, K
        self.a_shape = (K, M) if ta else (M, K)
        self.b_shape = (N, K) if tb else (K, N)
        self.lda = self.a_shape[1] if lda is None else lda
        self.ldb = self.b_shape[1] if ldb is None else ldb
        self.a_off, self.b_off, self.ldc_extra, self.bias_off = a_off, b_off, ldc_extra, bias_off
        self.ldm = N if ldm is None else ldm
        self.mul_off, self.note = mul_off, note

    def tag(self):
        extra = [n for n in ('lda=%d' % self.lda if self.lda != self.a_shape[1] else '',
                             'ldb=%d' % self.ldb if self.ldb != self.b_shape[1] else '',
                             'A+%d' % self.a_off if self.a_off else '', 'B+%d' % self.b_off if self.b_off else '',
                             'ldc+%d' % self.ldc_extra if self.ldc_extra else '',
                             'bias+%d' % self.bias_off if self.bias_off else '',
                             'ldm=%d' % self.ldm if self.ldm != self.N else '',
                             'mul+%d' % self.mul_off if self.mul_off else '') if n]
        return '%s %s%s (%d, %d, %d)%s' % (self.dtype, 'T' if self.ta else 'N', 'T' if self.tb else 'N', self.M, self.N,
                                           self.K, ' ' + ' '.join(extra) if extra else '')

    def seed(self):
        return (self.M * 1000003 + self.N * 10007 + self.K * 101 + self.ta * 2 + self.tb + (self.dtype == 'bf16') * 4) % (1 << 31)

    def ldc(self, form):
        return self.N if form == 'drop' else self.N + 8 + self.ldc_extra

    def c_off(self, form, out_dtype):
        """Elements between a 16-byte boundary and C[0][0] inside its frame (buffers start on such a boundary)."""
        per16 = 4 if out_dtype == 'f32' else 8
        return (2 * self.ldc(form) + (0 if form == 'drop' else 4)) % per16

    def plan(self, form, out_dtype, scratch_room, tn_wgs=0, big=1):
        return gemm_plan(self.dtype, out_dtype, self.ta, self.tb, self.M, self.N, self.K, self.lda, self.ldb,
                         self.ldc(form), self.a_off, self.b_off, self.c_off(form, out_dtype),
                         self.bias_off if form in ('bias', 'relu', 'mul', 'drop') else None,
                         self.mul_off if form == 'mul' else None, self.ldm, form == 'drop', scratch_room, tn_wgs, big)

    def expect(self, form, out_dtype, scratch_room, tn_wgs=0, big=1):
        return self.plan(form, out_dtype, scratch_room, tn_wgs, big)['keys']


TDT = {'f32': torch.float32, 'bf16': torch.bfloat16}


def _view(values, ld, off):
    """`values` [R, C] as a view with row stride ld that starts `off` elements into a buffer of NaN."""
    R, Cc = values.shape
    buf = torch.full((off + R * ld,), float('nan'), dtype=values.dtype)
    v = buf[off:].view(R, ld)[:, :Cc]
    v.copy_(values)
    return buf, v


def host_data(case, regime):
    """The operands of `case` on the CPU (fp64 values that the operand type holds exactly) and the fp64 pieces of every
    form's reference.  exact regime: asserts what makes it exact, on the reference alone."""
    g = torch.Generator().manual_seed(case.seed() + (regime == 'gaussian'))
    M, N, K = case.M, case.N, case.K
    t = TDT[case.dtype]
    if regime == 'exact':
        def draw(*shape):
            return torch.randint(-8, 9, shape, generator=g).double()
    else:
        def draw(*shape):
            return torch.randn(*shape, generator=g).double()
    A = draw(*case.a_shape).to(t).double()
    B = draw(*case.b_shape).to(t).double()
    bias = draw(N).float().double()
    c0 = draw(M, N).to(torch.bfloat16).double()               # the prior C: exact in either output type
    mul = (torch.rand(M, N, generator=g) < 0.5).double() * 2.0
    opA, opB = (A.t() if case.ta else A), (B.t() if case.tb else B)
    P = opA @ opB
    env = opA.abs() @ opB.abs()
    if regime == 'exact':
        assert float(env.max()) + 16 < 2 ** 24, (case.tag(), 'partial sums leave the integers fp32 holds')
        if K >= 512:
            for pre in (P, P + bias, P + c0, P + bias + c0):
                frac = float((pre.abs() > 256).double().mean())
                assert frac >= 0.5, (case.tag(), 'only %.2f of the reference above 256: a bf16 accumulator could pass' % frac)
    return dict(A=A, B=B, bias=bias, c0=c0, mul=mul, P=P, env=env)


def reference(d, form, dropmask=None):
    """fp64 reference of one form and the magnitude its gaussian bound is taken against."""
    ref, env = d['P'].clone(), d['env'].clone()
    if form in ('bias', 'relu', 'mul', 'drop'):
        ref, env = ref + d['bias'], env + d['bias'].abs()
    if form in ('accumulate', 'relu'):
        ref, env = ref + d['c0'], env + d['c0'].abs()
    if form == 'relu':
        ref = ref.clamp_min(0)
    if form == 'mul':
        ref, env = ref * d['mul'], env * 2
    if form == 'drop':
        ref, env = ref * dropmask, env * 2
    return ref, env


def _ops():
    from tensorflow_end2end_speech_recognition_amd import ops
    return ops


def device_limits():
    """scratch_room of the main handle of device 0, from the library (every handle's arena has that size)."""
    from tensorflow_end2end_speech_recognition_amd import _lib
    h = _lib.handle(0)
    return int(h.lib.asr_scratch_bytes(h.h)) - XCH_BYTES


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:24]


class Tally(object):
    """Runs one call between a reset and a read of the kernel counters and demands exactly the predicted ones -- every
    other key zero, so a product that fell to another kernel, or took a second pass it should not, fails here; sums what
    it saw and what was predicted."""

    def __init__(self):
        self.total = dict.fromkeys(ALL_KEYS, 0)

    def run(self, expect_keys, fn, what):
        ops = _ops()
        ops.reset_gemm_path_counts(0)
        res = fn()
        got = ops.gemm_kernel_counts(0)
        assert tuple(got) == ALL_KEYS, sorted(got)
        want = dict.fromkeys(got, 0)
        for k in expect_keys:
            want[k] += 1
        assert got == want, '%s: counters %s, predicted %s' % (
            what, {k: v for k, v in got.items() if v}, {k: v for k, v in want.items() if v})
        for k, v in got.items():
            self.total[k] += v
        return res


def _aligned(t):
    return t.data_ptr() % 16 == 0


def check_product(tally, case, forms=FORMS, out_dtypes=('f32', 'bf16'), regime='exact', scratch_room=None, tn_wgs=0,
                  big=1, side=False, dev='cuda:0', results=None):
    """ops.gemm on `case` in each of `forms` ('plain', 'bias', 'accumulate', 'relu' = bias + accumulate + ReLU, 'mul' = bias
    + multiplier, 'drop' = bias + dropout) and output types, every call under the tally with the counters gemm_plan
    predicts, every result against the fp64 reference (see the module docstring) inside an untouched guard frame.
    side: issue the calls on side lane 1 (its own handle: tn_wgs and the XCD skip are set there by the caller).
    results: dict that receives {tag: digest} of the fp32 results.  -> the union of the counters predicted."""
    ops = _ops()
    room = device_limits() if scratch_room is None else scratch_room
    d = host_data(case, regime)
    M, N = case.M, case.N
    t = TDT[case.dtype]
    bufA, Av = _view(d['A'].to(t), case.lda, case.a_off)
    bufB, Bv = _view(d['B'].to(t), case.ldb, case.b_off)
    bufA, bufB = bufA.to(dev), bufB.to(dev)
    assert _aligned(bufA) and _aligned(bufB)
    Ad = bufA[case.a_off:].view(case.a_shape[0], case.lda)[:, :case.a_shape[1]]
    Bd = bufB[case.b_off:].view(case.b_shape[0], case.ldb)[:, :case.b_shape[1]]
    bias_buf = torch.full((case.bias_off + N,), float('nan'))
    bias_buf[case.bias_off:] = d['bias'].float()
    bias_buf = bias_buf.to(dev)
    bias_d = bias_buf[case.bias_off:]
    mul_buf, _ = _view(d['mul'].float(), case.ldm, case.mul_off)
    mul_buf = mul_buf.to(dev)
    mul_d = mul_buf[case.mul_off:].view(M, case.ldm)[:, :N]
    assert _aligned(bias_buf) and _aligned(mul_buf)
    dropmask = None
    if 'drop' in forms:
        dropmask = ops.dropout_mask((M, N), *DROP, dev).double().cpu()
        vals = set(dropmask.unique().tolist())
        assert vals <= {0.0, 2.0} and (M * N < 64 or 0.3 < float((dropmask > 0).double().mean()) < 0.7), vals
    seen = set()
    for form in forms:
        ref, env = reference(d, form, dropmask)
        for od in out_dtypes:
            if form in ('mul', 'drop') and od != 'f32':
                continue
            tag = '%s, %s -> %s, %s' % (case.tag(), form, od, regime)
            ldc = case.ldc(form)
            left = 0 if form == 'drop' else 4
            frame = torch.full((M + 4, ldc), SENTINEL, dtype=TDT[od])
            if form in ('accumulate', 'relu'):
                frame[2:2 + M, left:left + N] = d['c0'].to(TDT[od])
            frame = frame.to(dev)
            assert _aligned(frame)
            out = frame[2:2 + M, left:left + N]
            assert (out.data_ptr() % 16) // out.element_size() == case.c_off(form, od), tag
            kw = dict(transA=bool(case.ta), transB=bool(case.tb), out=out)
            if form in ('bias', 'relu', 'mul', 'drop'):
                kw['bias'] = bias_d
            if form in ('accumulate', 'relu'):
                kw['accumulate'] = True
            if form == 'relu':
                kw['relu'] = True
            if form == 'mul':
                kw['mul'] = mul_d
            if form == 'drop':
                kw['drop'] = DROP
            keys = case.expect(form, od, room, tn_wgs, big)
            seen.update(keys)

            def call():
                if side:
                    with ops.side_lane(torch.device(dev)):
                        ops.gemm(Ad, Bd, **kw)
                    ops.join_side(torch.device(dev))
                else:
                    ops.gemm(Ad, Bd, **kw)
            tally.run(keys, call, tag)
            got = frame.cpu()
            inner = got[2:2 + M, left:left + N]
            hole = torch.ones(M + 4, ldc, dtype=torch.bool)
            hole[2:2 + M, left:left + N] = False
            assert bool((got[hole] == SENTINEL).all()), (tag, 'wrote outside C')
            if regime == 'exact':
                assert float(ref.abs().max()) < 2 ** 24
                want = ref.to(torch.float32).to(TDT[od])
                if not torch.equal(inner, want):
                    bad = (inner.double() != want.double()).nonzero()
                    i, j = [int(x) for x in bad[0]]
                    raise AssertionError('%s: %d of %d elements differ from the exact result, first at [%d, %d]: got %r, '
                                         'exact %r' % (tag, len(bad), M * N, i, j, float(inner[i, j]), float(want[i, j])))
            elif od == 'f32':
                ratio = float(((inner.double() - ref).abs() / env.clamp_min(1e-30)).max())
                print('%s: worst error %.3e of |A| @ |B| + |bias| + |C0| (bound %.0e)' % (tag, ratio, TOL[case.dtype]))
                assert ratio <= TOL[case.dtype], (tag, ratio)
            else:
                ok, worst = within_bf16_ulp(inner, ref)
                print('%s: worst %.3f bf16 ulp' % (tag, worst))
                assert ok, (tag, worst)
            if results is not None and od == 'f32':
                results['%s, %s' % (case.tag(), form)] = digest(inner)
    return seen


# ---------------------------------------------------------------- the cases of tests/test_gpu_gemm_variants.py
# (what each shape is for: the docstring of that file).  group -> [(Case, forms, the kernel counter every fp32-output call
# of the case must bump, or None where the forms differ)]
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]
MULDROP = FORMS + ('mul', 'drop')


def _f32(ta, tb, M, N, K, **kw):
    return Case('f32', ta, tb, M, N, K, **kw)


def _bf16(ta, tb, M, N, K, **kw):
    return Case('bf16', ta, tb, M, N, K, **kw)


CASES = {
    'skinny_nn32': [(_f32(0, 0, *s), FORMS, 'skinny_nn32')
                    for s in [(17, 32, 64), (16, 32, 512), (32, 64, 576), (15, 96, 1024), (1, 32, 1088)]],
    'skinny_nn16': [(_f32(0, 0, *s), FORMS, 'skinny_nn16') for s in [(17, 48, 64), (32, 16, 576), (1, 80, 1088)]],
    'skinny_nt16': [(_f32(0, 1, *s), FORMS, 'skinny_nt16') for s in [(17, 16, 64), (32, 48, 1088)]],
    'skinny_nt32': [(_f32(0, 1, *s), FORMS, 'skinny_nt32') for s in [(17, 6144, 64), (32, 6144, 576)]],
    'skinny_refused': [(c, MULDROP, 'generic64') for c in [
        _f32(0, 0, 33, 32, 64), _f32(0, 0, 17, 32, 96), _f32(0, 0, 17, 24, 64), _f32(1, 0, 17, 32, 64),
        _f32(0, 0, 17, 32, 64, lda=65), _f32(0, 0, 17, 32, 64, a_off=1), _f32(0, 0, 17, 32, 64, b_off=1),
        _f32(0, 1, 17, 32, 64, ldb=66)]],
    'generic128_f32': [(_f32(ta, tb, 2049, 2560, 40), FORMS, 'generic128') for ta, tb in LAYOUTS]
    + [(_f32(0, 0, 2560, 2048, 40), ('relu',), 'generic128')],             # exactly 320 tiles: the threshold itself
    'generic128_bf16': [(_bf16(ta, tb, 2049, 2560, 40), FORMS, 'generic128') for ta, tb in LAYOUTS],
    'nt128': [(_bf16(0, 1, *s), MULDROP, 'nt128')
              for s in [(1024, 128, 64), (1025, 128, 64), (1024, 256, 64), (1151, 256, 192), (1032, 384, 128)]],
    'nt128_refused': [(c, MULDROP, 'generic64') for c in [
        _bf16(0, 1, 1023, 128, 64), _bf16(0, 1, 1024, 192, 64), _bf16(0, 1, 1024, 128, 96),
        _bf16(0, 1, 1024, 128, 64, lda=68), _bf16(0, 1, 1024, 128, 64, a_off=1)]]
    + [(_bf16(0, 1, 1024, 128, 64, ldc_extra=1), FORMS + ('mul',), 'generic64'),   # (drop: a contiguous C, ldc == N, only)
       (_bf16(0, 1, 1024, 128, 64, bias_off=1), MULDROP, None), (_bf16(0, 1, 1024, 128, 64, ldm=129), MULDROP, None),
       (_bf16(0, 1, 1024, 128, 64, mul_off=1), MULDROP, None)],
    'tn_lean': [(_bf16(1, 0, *s), FORMS, 'tn_lean')
                for s in [(8, 8, 2048), (136, 264, 2048), (128, 128, 2112), (64, 64, 4099)]],
    'tn_refused': [(c, FORMS, 'generic64_splitk') for c in [
        _bf16(1, 0, 8, 8, 2047), _bf16(1, 0, 12, 8, 2048), _bf16(1, 0, 8, 8, 2048, lda=12)]],
}
for _dt, _mk in (('f32', _f32), ('bf16', _bf16)):
    CASES['generic64_' + _dt] = (
        [(_mk(ta, tb, *s), FORMS, 'generic64') for ta, tb in LAYOUTS for s in [(1, 1, 1), (65, 67, 33), (64, 64, 64)]]
        # the element-wise loader behind a base pointer off the 16-byte boundary, either operand, every layout
        + [(_mk(ta, tb, 65, 67, 33, **kw), FORMS, 'generic64') for ta, tb in LAYOUTS for kw in (dict(a_off=1), dict(b_off=1))])
CASES['splitk_f32'] = [(_f32(ta, tb, 64, 64, K), FORMS, 'generic64_splitk') for ta, tb in LAYOUTS
                       for K in (512, 1024, 1536, 1000)]
# rows with NaN behind them, as far as the last chunk would reach if it ran to its full width (7 x 160 = 1120,
# 7 x 320 = 2240): a k range that ran past K would read them
CASES['splitk_f32'] += [(_f32(0, 1, 64, 64, 1000, lda=1128, ldb=1128), FORMS, 'generic64_splitk')]
CASES['splitk_bf16'] = [(_bf16(ta, tb, 64, 64, K), FORMS, 'generic64_splitk') for ta, tb in LAYOUTS
                        for K in (1024, 2048, 1999) if not ((ta, tb) == (1, 0) and K == 2048)]   # (that one: the lean TN kernel)
CASES['splitk_bf16'] += [(_bf16(0, 1, 64, 64, 1999, lda=2248, ldb=2248), FORMS, 'generic64_splitk')]

# the split-K slab counts the rule gives (S is not observable from outside: pinned here and in the host test)
SPLITK_S = {('f32', 512): 4, ('f32', 1024): 8, ('f32', 1536): 12, ('f32', 1000): 7,
            ('bf16', 1024): 4, ('bf16', 2048): 8, ('bf16', 1999): 7}

# gaussian regime, once per counter: counter -> (Case, forms)
GAUSSIAN = {
    'skinny_nn32': (_f32(0, 0, 32, 64, 576), FORMS), 'skinny_nn16': (_f32(0, 0, 32, 16, 576), FORMS),
    'skinny_nt16': (_f32(0, 1, 32, 48, 1088), FORMS), 'skinny_nt32': (_f32(0, 1, 32, 6144, 576), FORMS),
    'nt128': (_bf16(0, 1, 1151, 256, 192), MULDROP), 'tn_lean': (_bf16(1, 0, 136, 264, 2048), FORMS),
    'generic128': (_bf16(1, 1, 2049, 2560, 40), FORMS), 'generic64': (_f32(1, 0, 65, 67, 33), FORMS),
    'generic64_splitk': (_f32(1, 1, 64, 64, 1000), FORMS),
    'mul_pass': (_bf16(0, 1, 1023, 128, 64), ('mul',)), 'drop_pass': (_bf16(0, 1, 1023, 128, 64), ('drop',)),
    # (nt256: in the child process, WORKER_GAUSSIAN)
}
GAUSSIAN_MORE = [(_bf16(0, 0, 65, 67, 33), FORMS), (_bf16(0, 0, 64, 64, 1999), FORMS), (_f32(0, 0, 2049, 2560, 40), ('relu',))]

# ---------------------------------------------------------------- what the child-process worker runs
WORKER_SHAPES = [(2048, 256, 64), (2049, 512, 128), (2303, 256, 192)]
WORKER_FORMS = MULDROP
WORKER_GAUSSIAN = (2303, 256, 192)


def predicted_counters(scratch_room, big=1):
    """The union of the counters gemm_plan predicts over CASES (both output types, default switches) -- and over the
    worker's shapes under ASR_GEMM_NT_BIG = `big` where that is not the default."""
    seen = set()
    if big != 1:
        for s in WORKER_SHAPES:
            for form in WORKER_FORMS:
                for od in ('f32', 'bf16'):
                    if not (form in ('mul', 'drop') and od == 'bf16'):
                        seen.update(_bf16(0, 1, *s).expect(form, od, scratch_room, 0, big))
        return seen
    for group in CASES.values():
        for case, forms, _ in group:
            for form in forms:
                for od in ('f32', 'bf16'):
                    if not (form in ('mul', 'drop') and od == 'bf16'):
                        seen.update(case.expect(form, od, scratch_room))
    return seen
