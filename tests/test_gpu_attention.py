"""GPU parity: attention encoder-decoder and joint CTC-attention (class surface of
models/attention/*.py) vs the oracle -- loss within 1e-4 relative (fp32), every parameter gradient,
teacher-forced logits, greedy inference ids bit-exact."""
import numpy as np
import pytest
import torch

from oracle import attention as oatt

pytestmark = pytest.mark.gpu


def _batch(rng, B, T, D, C):
    x = rng.randn(B, T, D).astype(np.float32)
    sl = rng.randint(max(2, T // 2), T + 1, size=B).astype(np.int32)
    sl[0] = T
    lens = rng.randint(1, 6, size=B)
    lens[0] = 5
    Lmax = int(lens.max()) + 2
    sos, eos = C, C + 1
    labels = np.full((B, Lmax), eos, dtype=np.int64)
    ctc_labels = np.full((B, int(lens.max())), -1, dtype=np.int64)
    for b in range(B):
        x[b, sl[b]:] = 0
        y = rng.randint(0, C, size=lens[b])
        labels[b, 0] = sos
        labels[b, 1:1 + lens[b]] = y
        ctc_labels[b, :lens[b]] = y
    return x, sl, labels, lens + 2, ctc_labels


def _mk(cls, att, D, H, L, U, A, Em, C, **kw):
    return cls(input_size=D, encoder_type='blstm', encoder_num_units=H, encoder_num_layers=L,
               encoder_num_proj=None, attention_type=att, attention_dim=A, decoder_type='lstm',
               decoder_num_units=U, decoder_num_layers=1, embedding_dim=Em, num_classes=C, sos_index=C,
               eos_index=C + 1, max_decode_length=12, parameter_init=0.1, clip_grad_norm=5.0,
               clip_activation_encoder=50, clip_activation_decoder=50, dtype='f32', seed=5, **kw)


@pytest.mark.parametrize('att', ['bahdanau_content', 'location', 'hybrid', 'dot_product', 'luong_dot', 'luong_general',
                                 'luong_concat'])
def test_attention_model_parity(cuda, att):
    from tensorflow_end2end_speech_recognition_amd.models.attention.attention_seq2seq import AttentionSeq2Seq
    rng = np.random.RandomState(11)
    B, T, D, H, L, U, A, Em, C = 5, 17, 12, 64, 1, 128, 32, 8, 9
    x, sl, labels, lsl, _ = _batch(rng, B, T, D, C)
    model = _mk(AttentionSeq2Seq, att, D, H, L, U, A, Em, C, sharpening_factor=1.5, logits_temperature=2.0)
    sd = {k: v.cpu().numpy() for k, v in model.store.state_dict().items()}
    ref = oatt.attention_model_forward(sd, x, labels, sl, lsl, L, att, clip_enc=50.0, clip_dec=50.0,
                                       sharpening=1.5, temperature=2.0)
    loss, logits, out_train, out_infer = model.compute_loss(x, labels, sl, lsl, 1.0, 1.0, 1.0)
    assert abs(loss.item() - ref['total_loss']) / abs(ref['total_loss']) < 1e-4
    assert np.abs(logits.cpu().numpy() * 1.0 - ref['logits'] * 2.0).max() < 2e-4      # ref logits are /temperature
    assert np.abs(out_train.attention_weights.cpu().numpy() - ref['alphas']).max() < 1e-5
    assert np.array_equal(out_train.predicted_ids.cpu().numpy(), ref['predicted_ids'])
    opt = model._set_optimizer('adam', 1e-3)
    gv = opt.compute_gradients(loss, model=model)
    for g, name in gv:
        r = ref['grads'][name]
        err = np.abs(g.cpu().numpy() - r).max()
        assert err < 2e-3 * max(np.abs(r).max(), 1e-3) + 1e-7, (name, err, np.abs(r).max())
    # greedy inference
    ids = out_infer.predicted_ids.cpu().numpy()
    ref_ids = oatt.attention_model_infer(sd, x, sl, L, att, C, C + 1, 12, clip_enc=50.0, clip_dec=50.0, sharpening=1.5)
    assert np.array_equal(ids, ref_ids)
    dtr, dinf = model.decode(out_train, out_infer)
    assert dtr.shape[0] == B and dinf.shape[0] == B


@pytest.mark.parametrize('att', ['bahdanau_content', 'luong_dot'])
def test_attention_sigmoid_smoothing(cuda, att):
    """sigmoid_smoothing=True (attention_layer.py:92-96): alpha = sigmoid(e) / sum sigmoid(e); loss, weights,
    every gradient and the greedy decode against the fp64 oracle."""
    from tensorflow_end2end_speech_recognition_amd.models.attention.attention_seq2seq import AttentionSeq2Seq
    rng = np.random.RandomState(21)
    B, T, D, H, L, U, A, Em, C = 5, 19, 12, 64, 1, 128, 32, 8, 9
    x, sl, labels, lsl, _ = _batch(rng, B, T, D, C)
    model = _mk(AttentionSeq2Seq, att, D, H, L, U, A, Em, C, sharpening_factor=2.0, sigmoid_smoothing=True)
    sd = {k: v.cpu().numpy() for k, v in model.store.state_dict().items()}
    ref = oatt.attention_model_forward(sd, x, labels, sl, lsl, L, att, clip_enc=50.0, clip_dec=50.0, sharpening=2.0,
                                       sigmoid_smoothing=True)
    loss, logits, out_train, out_infer = model.compute_loss(x, labels, sl, lsl, 1.0, 1.0, 1.0)
    assert abs(loss.item() - ref['total_loss']) / abs(ref['total_loss']) < 1e-4
    al = out_train.attention_weights.cpu().numpy()
    assert np.abs(al - ref['alphas']).max() < 1e-5
    opt = model._set_optimizer('adam', 1e-3)
    for g, name in opt.compute_gradients(loss, model=model):
        r = ref['grads'][name]
        err = np.abs(g.cpu().numpy() - r).max()
        assert err < 2e-3 * max(np.abs(r).max(), 1e-3) + 1e-7, (name, err, np.abs(r).max())
    ref_ids = oatt.attention_model_infer(sd, x, sl, L, att, C, C + 1, 12, clip_enc=50.0, clip_dec=50.0, sharpening=2.0,
                                         sigmoid_smoothing=True)
    assert np.array_equal(out_infer.predicted_ids.cpu().numpy(), ref_ids)


def test_joint_ctc_attention_parity_and_training(cuda):
    from tensorflow_end2end_speech_recognition_amd.models.attention.joint_ctc_attention import JointCTCAttention
    from tensorflow_end2end_speech_recognition_amd.utils.io.labels.sparsetensor import list2sparsetensor
    rng = np.random.RandomState(3)
    B, T, D, H, L, U, A, Em, C = 6, 20, 12, 64, 2, 64, 32, 8, 7
    x, sl, labels, lsl, ctc_labels = _batch(rng, B, T, D, C)
    model = _mk(JointCTCAttention, 'bahdanau_content', D, H, L, U, A, Em, C, lambda_weight=0.5)
    sd = {k: v.cpu().numpy() for k, v in model.store.state_dict().items()}
    ctc_list = [[int(v) for v in row if v >= 0] for row in ctc_labels]
    ref = oatt.attention_model_forward(sd, x, labels, sl, lsl, L, 'bahdanau_content', clip_enc=50.0, clip_dec=50.0,
                                       ctc_labels=ctc_list, lambda_weight=0.5)
    loss, logits, ctc_logits, otr, oinf = model.compute_loss(x, labels, list2sparsetensor(ctc_labels, -1), sl, lsl,
                                                             1.0, 1.0, 1.0)
    assert abs(loss.item() - ref['total_loss']) / abs(ref['total_loss']) < 1e-4
    assert np.abs(ctc_logits.cpu().numpy() - ref['ctc_logits']).max() < 1e-4
    assert np.abs(model.ctc_losses.cpu().numpy() - ref['ctc_losses']).max() / ref['ctc_losses'].max() < 1e-4
    opt = model._set_optimizer('adam', 1e-3)
    for g, name in opt.compute_gradients(loss, model=model):
        r = ref['grads'][name]
        err = np.abs(g.cpu().numpy() - r).max()
        assert err < 2e-3 * max(np.abs(r).max(), 1e-3) + 1e-7, (name, err)
    # overfit the batch (the reference's own test strategy) incl. dropout paths
    first = last = None
    for step in range(40):
        loss, *_ = model.compute_loss(x, labels, ctc_labels, sl, lsl, 0.9, 0.9, 0.9)
        model.train(loss, 'adam', 2e-3)
        first = loss.item() if first is None else first
        last = loss.item()
    assert last < 0.6 * first, (first, last)


def test_attention_bf16_operands(cuda):
    """bf16-operand model (encoder MFMA operands, per-step context / d-alpha streams over the bf16 encoder
    copy): loss within bf16 rounding of the fp64 oracle, and it trains."""
    from tensorflow_end2end_speech_recognition_amd.models.attention.attention_seq2seq import AttentionSeq2Seq
    rng = np.random.RandomState(8)
    B, T, D, H, L, U, A, Em, C = 6, 20, 12, 64, 2, 64, 32, 8, 7
    x, sl, labels, lsl, _ = _batch(rng, B, T, D, C)
    for att in ('bahdanau_content', 'luong_dot'):
        kw = dict(input_size=D, encoder_type='blstm', encoder_num_units=H, encoder_num_layers=L, encoder_num_proj=None,
                  attention_type=att, attention_dim=A, decoder_type='lstm', decoder_num_units=2 * H if att == 'luong_dot' else U,
                  decoder_num_layers=1, embedding_dim=Em, num_classes=C, sos_index=C, eos_index=C + 1,
                  max_decode_length=12, parameter_init=0.1, clip_grad_norm=5.0, clip_activation_encoder=50,
                  clip_activation_decoder=50, seed=5)
        model = AttentionSeq2Seq(dtype='bf16', **kw)
        sd = {k: v.cpu().numpy() for k, v in model.store.state_dict().items()}
        ref = oatt.attention_model_forward(sd, x, labels, sl, lsl, L, att, clip_enc=50.0, clip_dec=50.0)
        loss, *_ = model.compute_loss(x, labels, sl, lsl, 1.0, 1.0, 1.0)
        assert abs(loss.item() - ref['total_loss']) / abs(ref['total_loss']) < 3e-2, att
        first = None
        for step in range(30):
            loss, *_ = model.compute_loss(x, labels, sl, lsl, 0.9, 0.9, 0.9)
            model.train(loss, 'adam', 3e-3)
            first = loss.item() if first is None else first
        assert loss.item() < 0.7 * first, att


# ------------------------------------------------------------------------------------------------------------------
# Kernel-level parity at cfg-D / cfg-E sequence lengths (T up to 1600, A = 128, 2H = 1024): the scoring /
# softmax / context kernels work on 64-frame chunks with per-chunk partials reduced in a fixed order, so every
# T > 64 exercises the multi-chunk path the small model tests never reach.
def _ragged(rng, B, T):
    sl = rng.randint(max(1, T // 3), T + 1, size=B).astype(np.int32)
    sl[0] = T
    if B > 2:
        sl[2] = min(T, 3)
    return sl


@pytest.mark.parametrize('T', [65, 200, 1600])
@pytest.mark.parametrize('mode,with_keys', [(0, True), (0, False), (1, True)])
def test_att_energy_kernels_multi_chunk(cuda, T, mode, with_keys):
    """asr_att_energy_fwd / _bwd (attention_layer.py:162-186, 262): additive with keys (bahdanau / hybrid), additive
    without keys (location, Q6) and dot-product energies, vs fp64 autograd."""
    from tensorflow_end2end_speech_recognition_amd import ops
    rng = np.random.RandomState(T + mode)
    B, A = 3, 128
    keys = torch.tensor(rng.randn(T, B, A) * 0.5, dtype=torch.float32) if with_keys else None
    qz = torch.tensor(rng.randn(B, A) * 0.5, dtype=torch.float32)
    v = torch.tensor(rng.randn(A), dtype=torch.float32)
    de = torch.tensor(rng.randn(B, T), dtype=torch.float32)
    k64 = keys.double().clone().requires_grad_(True) if with_keys else None
    q64, v64 = qz.double().clone().requires_grad_(True), v.double().clone().requires_grad_(True)
    if mode == 0:
        z = q64.unsqueeze(0) + (k64 if with_keys else torch.zeros(T, B, A, dtype=torch.float64))
        ref = (v64 * torch.tanh(z)).sum(2).t()
    else:
        ref = (k64 * q64.unsqueeze(0)).sum(2).t()
    (ref * de.double()).sum().backward()
    kd = keys.to(cuda) if with_keys else None
    got = ops.att_energy_fwd(kd, qz.to(cuda), v.to(cuda) if mode == 0 else None, T, mode)
    assert np.abs(got.cpu().numpy() - ref.detach().numpy()).max() < 2e-5 * max(1.0, float(ref.abs().max()))
    dkeys = torch.zeros(T, B, A, device=cuda) if with_keys else None
    dqz, dv = ops.att_energy_bwd(de.to(cuda), kd, qz.to(cuda), v.to(cuda) if mode == 0 else None, mode, dkeys=dkeys,
                                 want_dv=mode == 0)
    rel = lambda a, b: np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)
    assert rel(dqz.cpu().numpy(), q64.grad.numpy()) < 1e-5
    if mode == 0:
        assert rel(dv.sum(0).cpu().numpy(), v64.grad.numpy()) < 1e-5
    if with_keys:
        assert rel(dkeys.cpu().numpy(), k64.grad.numpy()) < 1e-5


@pytest.mark.parametrize('T', [65, 200, 1600])
@pytest.mark.parametrize('enc_dtype,sigmoid', [('f32', False), ('bf16', False), ('f32', True)])
def test_att_softmax_context_kernels_multi_chunk(cuda, T, enc_dtype, sigmoid):
    """asr_att_softmax_ctx_fwd / _bwd (attention_layer.py:75-111): mask, sharpening, softmax / sigmoid smoothing,
    context, and the gradients w.r.t. the energies and (per-step form) the encoder outputs, incl. an external
    gradient w.r.t. alpha (carried location features), vs fp64 autograd on the operands the kernel reads."""
    rng = np.random.RandomState(T + 7)
    _softmax_context_case(cuda, T, 1024, enc_dtype, sigmoid, _ragged(rng, 4, T), rng)


def _softmax_context_case(cuda, T, E, enc_dtype, sigmoid, sl, rng=None):
    from tensorflow_end2end_speech_recognition_amd import ops
    rng = rng if rng is not None else np.random.RandomState(T + E)
    B, sharp = len(sl), 1.5
    enc = torch.tensor(rng.randn(T, B, E), dtype=torch.float32)
    if enc_dtype == 'bf16':
        enc = enc.to(torch.bfloat16)
    energy = torch.tensor(rng.randn(B, T) * 2, dtype=torch.float32)
    dctx = torch.tensor(rng.randn(B, E), dtype=torch.float32)
    dextra = torch.tensor(rng.randn(B, T), dtype=torch.float32)
    e64 = energy.double().clone().requires_grad_(True)
    enc64 = enc.double().clone().requires_grad_(True)
    mask = torch.arange(T).unsqueeze(0) < torch.tensor(sl).long().unsqueeze(1)
    em = torch.where(mask, e64, torch.full_like(e64, float(np.finfo(np.float32).min))) * sharp
    if sigmoid:
        sg = torch.sigmoid(em) * mask
        alpha = sg / sg.sum(1, keepdim=True)
    else:
        alpha = torch.softmax(em, 1)
    ctx = torch.einsum('bt,tbe->be', alpha, enc64)
    ((ctx * dctx.double()).sum() + (alpha * dextra.double() * mask).sum()).backward()
    sld = torch.tensor(sl, device=cuda)
    snorm = torch.empty(B, device=cuda) if sigmoid else None
    a_dev, c_dev = ops.att_softmax_ctx_fwd(energy.to(cuda), sld, sharp, enc.to(cuda), sigmoid_norm=snorm)
    assert np.abs(a_dev.cpu().numpy() - alpha.detach().numpy()).max() < 2e-6
    assert np.abs(c_dev.cpu().numpy() - ctx.detach().numpy()).max() < 2e-5 * max(1.0, float(ctx.abs().max()))
    denc = torch.zeros(T, B, E, device=cuda)
    de_dev = ops.att_softmax_ctx_bwd(dctx.to(cuda), a_dev, sld, sharp, enc.to(cuda), denc, sigmoid_norm=snorm,
                                     dalpha_extra=dextra.to(cuda))
    rel = lambda a, b: np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)
    assert rel(de_dev.cpu().numpy(), e64.grad.numpy()) < 2e-5
    assert rel(denc.cpu().numpy(), enc64.grad.numpy()) < 2e-5


@pytest.mark.parametrize('T', [30, 65, 200, 1600])
@pytest.mark.parametrize('taps,with_keys', [(201, False), (200, True)])
def test_att_location_feature_kernels(cuda, T, taps, with_keys):
    """asr_att_loc_energy_fwd / _bwd: conv1d(alpha_prev, filter [taps,1,10], SAME) -> W_filter inside the energy
    (attention_layer.py:200-229 hybrid, 200 taps, pad 99 / 100; :239-265 location, 201 taps), two consecutive
    steps' accumulation of the per-utterance filter / W_filter gradients, vs fp64 autograd of the torch statement."""
    from tensorflow_end2end_speech_recognition_amd import ops
    from _cpu_ops import _loc_energy
    rng = np.random.RandomState(T + taps)
    B, A = 3, 128
    keys = torch.tensor(rng.randn(T, B, A) * 0.5, dtype=torch.float32) if with_keys else None
    qz = torch.tensor(rng.randn(B, A) * 0.5, dtype=torch.float32)
    v = torch.tensor(rng.randn(A), dtype=torch.float32)
    filt = torch.tensor(rng.randn(taps, 1, 10) * 0.3, dtype=torch.float32)
    wfil = torch.tensor(rng.randn(10, A) * 0.3, dtype=torch.float32)
    sl = _ragged(rng, B, T)
    ap = torch.tensor(rng.rand(B, T), dtype=torch.float32)
    ap = ap * (torch.arange(T).unsqueeze(0) < torch.tensor(sl).long().unsqueeze(1))
    ap = ap / ap.sum(1, keepdim=True)                       # a softmax-like previous weight vector, zero past len
    de = [torch.tensor(rng.randn(B, T), dtype=torch.float32) for _ in range(2)]
    leaves = [t.double().clone().requires_grad_(True) for t in (ap, filt, wfil, qz, v)]
    k64 = keys.double().clone().requires_grad_(True) if with_keys else None
    ref = _loc_energy(leaves[0], leaves[1], leaves[2], k64, leaves[3], leaves[4], T)
    dev = lambda t: None if t is None else t.to(cuda)
    got = ops.att_loc_energy_fwd(dev(ap), dev(filt), dev(wfil), dev(keys), dev(qz), dev(v), T)
    assert np.abs(got.cpu().numpy() - ref.detach().numpy()).max() < 3e-5 * max(1.0, float(ref.abs().max()))
    (ref * (de[0] + de[1]).double()).sum().backward()       # two "steps" with the same operands: grads add up
    dw = torch.empty(B, 10, A, device=cuda)
    df = torch.empty(B, taps, 10, device=cuda)
    dkeys = torch.zeros(T, B, A, device=cuda) if with_keys else None
    dq = dv = dap = 0
    for i in range(2):
        a, b_, c = ops.att_loc_energy_bwd(dev(de[i]), dev(ap), dev(filt), dev(wfil), dev(keys), dev(qz), dev(v), dw, df,
                                          accumulate=(i == 1), dkeys=dkeys)
        dq, dv, dap = dq + a, dv + b_, dap + c
    rel = lambda a, b: np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)
    assert rel(dq.cpu().numpy(), leaves[3].grad.numpy()) < 2e-5
    assert rel(dv.sum(0).cpu().numpy(), leaves[4].grad.numpy()) < 2e-5
    assert rel(dw.sum(0).cpu().numpy(), leaves[2].grad.numpy()) < 2e-5
    assert rel(df.sum(0).cpu().numpy().reshape(taps, 1, 10), leaves[1].grad.numpy()) < 2e-5
    assert rel(dap.cpu().numpy(), leaves[0].grad.numpy()) < 2e-5
    if with_keys:
        assert rel(dkeys.cpu().numpy(), k64.grad.numpy()) < 2e-5


# ------------------------------------------------------------------------------------------------------------------
# The same kernels across the lane shapes their launchers pick from the attention width (energy_vec_shape /
# loc_vec_shape in csrc/attention.hip), with ops.att_path_counts saying which one ran.
def _energy_lanes(A, aligned=True):
    """energy_vec_shape: float4 lanes per frame (x 2 vectors per lane above 256 columns), else the general kernel."""
    if A % 4 or A > 512 or not aligned:
        return 'general'
    return '16' if A <= 64 else '32' if A <= 128 else '64' if A <= 256 else '64x2'


def _loc_lanes(A, aligned=True):
    """loc_vec_shape: as above, no two-vector form."""
    if A % 4 or A > 256 or not aligned:
        return 'general'
    return '16' if A <= 64 else '32' if A <= 128 else '64'


def _counted(ops):
    """The non-zero attention path counters since the last reset."""
    return {k: v for k, v in ops.att_path_counts(0).items() if v}


def _lane_lengths(rng, T):
    """B = 5: a full row, one frame, exactly one 64-frame chunk, one frame more, a random length."""
    return np.array([T, 1, 64, 65, rng.randint(66, T)], dtype=np.int32)


def _misaligned(t, dev):
    """`t` on `dev` at an address that is 4 but not 16 bytes aligned: a view into a buffer one float larger."""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=dev)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


@pytest.mark.parametrize('A', [4, 36, 64, 100, 130, 256, 260, 512, 516, 'qz+4B', 'keys+4B'])
@pytest.mark.parametrize('mode,with_keys', [(0, True), (0, False), (1, True)])
def test_att_energy_kernels_lane_shapes(cuda, A, mode, with_keys):
    """asr_att_energy_fwd / _bwd at every lane shape of energy_vec_shape: 16 lanes (A = 4: one live lane, 36: tail lanes
    idle, 64: all), 32 (100: tail idle), 64 (256), 64 x 2 vectors (260: one live lane in the second vector, 512: all) and
    the general kernels (130: A % 4 != 0, 516: A > 512, and A = 128 with qz or keys 4 bytes off a 16-byte boundary), vs
    fp64 autograd.  T = 200 (four chunks), B = 5; the entry points take no lengths, so the ragged batch (full, 1, 64, 65,
    random frames) is expressed the way the decoder loop does it: the energy gradient is zero from a row's length on.
    Bounds: those of test_att_energy_kernels_multi_chunk (they do not depend on A: relative to the largest entry)."""
    from tensorflow_end2end_speech_recognition_amd import ops
    off = A if isinstance(A, str) else None
    if off == 'keys+4B' and not with_keys:
        off = 'qz+4B'                                          # (no keys to misplace: the query again)
    A = 128 if off else A
    rng = np.random.RandomState(1000 * mode + A + (7 if with_keys else 0))
    B, T = 5, 200
    sl = _lane_lengths(rng, T)
    keys = torch.tensor(rng.randn(T, B, A) * 0.5, dtype=torch.float32) if with_keys else None
    qz = torch.tensor(rng.randn(B, A) * 0.5, dtype=torch.float32)
    v = torch.tensor(rng.randn(A), dtype=torch.float32)
    de = torch.tensor(rng.randn(B, T), dtype=torch.float32) * (torch.arange(T).unsqueeze(0) < torch.tensor(sl).long().unsqueeze(1))
    k64 = keys.double().clone().requires_grad_(True) if with_keys else None
    q64, v64 = qz.double().clone().requires_grad_(True), v.double().clone().requires_grad_(True)
    if mode == 0:
        z = q64.unsqueeze(0) + (k64 if with_keys else torch.zeros(T, B, A, dtype=torch.float64))
        ref = (v64 * torch.tanh(z)).sum(2).t()
    else:
        ref = (k64 * q64.unsqueeze(0)).sum(2).t()
    (ref * de.double()).sum().backward()
    kd = None if not with_keys else _misaligned(keys, cuda) if off == 'keys+4B' else keys.to(cuda)
    qd = _misaligned(qz, cuda) if off == 'qz+4B' else qz.to(cuda)
    vd = v.to(cuda) if mode == 0 else None
    lanes = _energy_lanes(A, aligned=not off)
    ops.reset_att_path_counts(0)
    got = ops.att_energy_fwd(kd, qd, vd, T, mode)
    assert _counted(ops) == {'energy_fwd_' + lanes: 1}
    assert np.abs(got.cpu().numpy() - ref.detach().numpy()).max() < 2e-5 * max(1.0, float(ref.abs().max()))
    dkeys = torch.zeros(T, B, A, device=cuda) if with_keys else None
    ops.reset_att_path_counts(0)
    dqz, dv = ops.att_energy_bwd(de.to(cuda), kd, qd, vd, mode, dkeys=dkeys, want_dv=mode == 0)
    assert _counted(ops) == {'energy_bwd_' + lanes: 1}
    rel = lambda a, b: np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)
    assert rel(dqz.cpu().numpy(), q64.grad.numpy()) < 1e-5
    if mode == 0:
        assert rel(dv.sum(0).cpu().numpy(), v64.grad.numpy()) < 1e-5
    if with_keys:
        assert rel(dkeys.cpu().numpy(), k64.grad.numpy()) < 1e-5
    assert ops.check_async_errors(0) == 0


@pytest.mark.parametrize('A', [4, 36, 64, 100, 256, 260, 'qz+4B'])
@pytest.mark.parametrize('taps,with_keys', [(201, False), (200, True)])
def test_att_location_feature_kernels_lane_shapes(cuda, A, taps, with_keys):
    """asr_att_loc_energy_fwd / _bwd at every lane shape of loc_vec_shape: 16 lanes (A = 4, 36, 64), 32 (100), 64 (256:
    the backward's four-wave partial sums then need more than 64 KB of LDS) and the general kernels (260: A > 256; A = 128
    with a misaligned query), two accumulating backward calls, vs fp64 autograd of _cpu_ops._loc_energy.  T = 200, B = 5,
    ragged as the loop has it: the previous weights and the energy gradient are zero from a row's length on.  Bounds:
    those of test_att_location_feature_kernels."""
    from tensorflow_end2end_speech_recognition_amd import ops
    from _cpu_ops import _loc_energy
    off = isinstance(A, str)
    A = 128 if off else A
    rng = np.random.RandomState(taps + A)
    B, T = 5, 200
    sl = _lane_lengths(rng, T)
    inside = torch.arange(T).unsqueeze(0) < torch.tensor(sl).long().unsqueeze(1)
    keys = torch.tensor(rng.randn(T, B, A) * 0.5, dtype=torch.float32) if with_keys else None
    qz = torch.tensor(rng.randn(B, A) * 0.5, dtype=torch.float32)
    v = torch.tensor(rng.randn(A), dtype=torch.float32)
    filt = torch.tensor(rng.randn(taps, 1, 10) * 0.3, dtype=torch.float32)
    wfil = torch.tensor(rng.randn(10, A) * 0.3, dtype=torch.float32)
    ap = torch.tensor(rng.rand(B, T), dtype=torch.float32) * inside
    ap = ap / ap.sum(1, keepdim=True)
    de = [torch.tensor(rng.randn(B, T), dtype=torch.float32) * inside for _ in range(2)]
    leaves = [t.double().clone().requires_grad_(True) for t in (ap, filt, wfil, qz, v)]
    k64 = keys.double().clone().requires_grad_(True) if with_keys else None
    ref = _loc_energy(leaves[0], leaves[1], leaves[2], k64, leaves[3], leaves[4], T)
    dev = lambda t: None if t is None else t.to(cuda)
    qd = _misaligned(qz, cuda) if off else qz.to(cuda)
    lanes = _loc_lanes(A, aligned=not off)
    ops.reset_att_path_counts(0)
    got = ops.att_loc_energy_fwd(dev(ap), dev(filt), dev(wfil), dev(keys), qd, dev(v), T)
    assert _counted(ops) == {'loc_fwd_' + lanes: 1}
    assert np.abs(got.cpu().numpy() - ref.detach().numpy()).max() < 3e-5 * max(1.0, float(ref.abs().max()))
    (ref * (de[0] + de[1]).double()).sum().backward()
    dw = torch.empty(B, 10, A, device=cuda)
    df = torch.empty(B, taps, 10, device=cuda)
    dkeys = torch.zeros(T, B, A, device=cuda) if with_keys else None
    dq = dv = dap = 0
    ops.reset_att_path_counts(0)
    for i in range(2):
        a, b_, c = ops.att_loc_energy_bwd(dev(de[i]), dev(ap), dev(filt), dev(wfil), dev(keys), qd, dev(v), dw, df,
                                          accumulate=(i == 1), dkeys=dkeys)
        dq, dv, dap = dq + a, dv + b_, dap + c
    assert _counted(ops) == {'loc_bwd_' + lanes: 2}
    rel = lambda a, b: np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)
    assert rel(dq.cpu().numpy(), leaves[3].grad.numpy()) < 2e-5
    assert rel(dv.sum(0).cpu().numpy(), leaves[4].grad.numpy()) < 2e-5
    assert rel(dw.sum(0).cpu().numpy(), leaves[2].grad.numpy()) < 2e-5
    assert rel(df.sum(0).cpu().numpy().reshape(taps, 1, 10), leaves[1].grad.numpy()) < 2e-5
    assert rel(dap.cpu().numpy(), leaves[0].grad.numpy()) < 2e-5
    if with_keys:
        assert rel(dkeys.cpu().numpy(), k64.grad.numpy()) < 2e-5
    assert ops.check_async_errors(0) == 0


@pytest.mark.parametrize('E', [64, 256, 320])
@pytest.mark.parametrize('enc_dtype', ['f32', 'bf16'])
def test_att_softmax_context_kernels_encoder_widths(cuda, E, enc_dtype):
    """asr_att_softmax_ctx_fwd / _bwd at encoder widths beside 1024: 64 (a quarter of a 256-thread row), 256 and 320
    (a partial second trip), fp32 and bf16, T = 200, on the ragged batch full / 1 / 64 / 65 / random; same statement
    and bounds as test_att_softmax_context_kernels_multi_chunk."""
    _softmax_context_case(cuda, 200, E, enc_dtype, False, _lane_lengths(np.random.RandomState(E), 200))


@pytest.mark.parametrize('att,sig,B,T', [('location', False, 5, 17), ('hybrid', False, 5, 17), ('hybrid', True, 4, 150),
                                         ('location', False, 4, 150), ('bahdanau_content', False, 4, 150)])
def test_attention_model_parity_carried_alpha_and_long_inputs(cuda, att, sig, B, T):
    """prev_alpha='carry' (the recurrence attention_layer.py:191-265 was written to express):
    loss, weights, EVERY gradient (incl. `filter`, W_filter/weights, which are dead under the reference's effective
    graph) and greedy inference vs the oracle; T = 150 spans three 64-frame chunks of the scoring kernels and the
    per-utterance alpha^T dctx contraction of the encoder gradient."""
    from tensorflow_end2end_speech_recognition_amd.models.attention.attention_seq2seq import AttentionSeq2Seq
    rng = np.random.RandomState(31 + T)
    D, H, L, U, A, Em, C = 12, 64, 1, 128, 32, 8, 9
    x, sl, labels, lsl, _ = _batch(rng, B, T, D, C)
    model = _mk(AttentionSeq2Seq, att, D, H, L, U, A, Em, C, sharpening_factor=1.5, sigmoid_smoothing=sig,
                prev_alpha='carry')
    sd = {k: v.cpu().numpy() for k, v in model.store.state_dict().items()}
    ref = oatt.attention_model_forward(sd, x, labels, sl, lsl, L, att, clip_enc=50.0, clip_dec=50.0, sharpening=1.5,
                                       sigmoid_smoothing=sig, prev_alpha='carry')
    loss, logits, out_train, out_infer = model.compute_loss(x, labels, sl, lsl, 1.0, 1.0, 1.0)
    assert abs(loss.item() - ref['total_loss']) / abs(ref['total_loss']) < 1e-4
    assert np.abs(out_train.attention_weights.cpu().numpy() - ref['alphas']).max() < 1e-5
    opt = model._set_optimizer('adam', 1e-3)
    A_ = 'attention_decoder/decoder/attention_layer/'
    for g, name in opt.compute_gradients(loss, model=model):
        r = ref['grads'][name]
        err = np.abs(g.cpu().numpy() - r).max()
        assert err < 2e-3 * max(np.abs(r).max(), 1e-3) + 1e-7, (name, err, np.abs(r).max())
        if att != 'bahdanau_content' and name in (A_ + 'filter', A_ + 'W_filter/weights'):
            assert np.abs(r).max() > 0          # the location path is live
    ref_ids = oatt.attention_model_infer(sd, x, sl, L, att, C, C + 1, 12, clip_enc=50.0, clip_dec=50.0, sharpening=1.5,
                                         sigmoid_smoothing=sig, prev_alpha='carry')
    assert np.array_equal(out_infer.predicted_ids.cpu().numpy(), ref_ids)


@pytest.mark.parametrize('B,K,U,peep,bias,mask', [(32, 1600, 512, True, True, True), (5, 192, 64, False, True, False),
                                                  (17, 640, 128, True, False, True), (1, 64, 8, False, False, False)])
def test_cell_product_and_cell_in_one_launch(cuda, B, K, U, peep, bias, mask):
    """asr_lstm_cell_gemm_fwd on the gate-interleaved image (asr_lstm_cell_gemm_prep) == asr_gemm_act -> asr_lstm_cell_fwd_ex,
    bit for bit: every output, the copies into column blocks of wider arrays included; finished rows (live = 0) copy their
    state through; the cfg D decoder's own shape (B = 32, 1600 -> 4 x 512) and ragged ones.  Reference:
    attention_decoder.py:142-229 (LSTMBlockCell of the decoder)."""
    from tensorflow_end2end_speech_recognition_amd import ops
    rng = np.random.RandomState(B + K + U)
    f = lambda *s, sc=1.0: torch.tensor(rng.randn(*s) * sc, dtype=torch.float32, device=cuda)
    wide = f(B, K + 8, sc=0.5)                               # x as a row block of a wider array
    x = wide[:, :K]
    W, b = f(K, 4 * U, sc=0.06), (f(4 * U, sc=0.2) if bias else None)
    pp = f(3, U, sc=0.3) if peep else None
    cp, hp = f(B, U, sc=2.0), f(B, U, sc=0.5)
    live = torch.tensor((rng.rand(B) < 0.7).astype(np.float32), device=cuda)
    live[0] = 1.0
    om = torch.tensor((rng.rand(B, U) < 0.8) / 0.8, dtype=torch.float32, device=cuda) if mask else None
    next_in, av = torch.zeros(B, K, device=cuda), torch.zeros(B, U + 24, device=cuda)
    next_in2, av2 = torch.zeros_like(next_in), torch.zeros_like(av)
    pre = ops.gemm(x, W, bias=b)
    want = ops.lstm_cell_fwd(pre, cp, hp, pp, live, 1.0, 3.0, out_mask=om, want_cell_out=True,
                             h_also=next_in[:, K - U:], cell_out_also=av[:, :U])
    W_il = ops.lstm_cell_gemm_prep(W, b)
    assert torch.equal(W_il[:K].view(K, U, 4), W.view(K, 4, U).transpose(1, 2))
    got = ops.lstm_cell_gemm_fwd(x, W_il, bias, cp, hp, pp, live, 1.0, 3.0, out_mask=om, h_also=next_in2[:, K - U:],
                                 cell_out_also=av2[:, :U])
    for name, g, w in zip(('gates', 'c_raw', 'c_out', 'h_out', 'h_raw', 'cell_out'), got, want):
        assert torch.equal(g, w), (name, float((g - w).abs().max()))
    assert torch.equal(next_in2, next_in) and torch.equal(av2, av)
    assert float(want[0].abs().sum()) > 0 and float((want[2] - cp).abs().max()) > 0     # the clip (3.0) and live rows are exercised
    assert float(want[1].abs().max()) <= 3.0


@pytest.mark.parametrize('B,K,U', [(32, 1600, 512), (5, 192, 64), (17, 640, 128), (1, 64, 16)])
def test_cell_products_with_bf16_weight_images(cuda, B, K, U):
    """asr_lstm_cell_gemm_fwd_h / _bwd_h (bf16 weight images: fragment-ordered, gate-interleaved for the forward product +
    cell; plain rows for dpre W^T) against the fp32 kernels on the same weights rounded to bf16 -- the activations stay
    fp32 and the products are exact, so only the summation order differs: 1e-5 of the largest entry."""
    from tensorflow_end2end_speech_recognition_amd import ops
    rng = np.random.RandomState(B + K + U + 1)
    f = lambda *s, sc=1.0: torch.tensor(rng.randn(*s) * sc, dtype=torch.float32, device=cuda)
    x, W, b, pp = f(B, K, sc=0.5), f(K, 4 * U, sc=0.06), f(4 * U, sc=0.2), f(3, U, sc=0.3)
    cp, hp = f(B, U, sc=2.0), f(B, U, sc=0.5)
    live = torch.ones(B, device=cuda)
    live[B // 2:] = torch.tensor((rng.rand(B - B // 2) < 0.6).astype(np.float32), device=cuda)
    om = torch.tensor((rng.rand(B, U) < 0.8) / 0.8, dtype=torch.float32, device=cuda)
    Wr = W.to(torch.bfloat16).float()
    img = ops.lstm_cell_gemm_prep_h(W, b)
    nxt, av = torch.zeros(B, K, device=cuda), torch.zeros(B, U + 8, device=cuda)
    nxt2, av2 = torch.zeros_like(nxt), torch.zeros_like(av)
    want = ops.lstm_cell_fwd(ops.gemm(x, Wr, bias=b), cp, hp, pp, live, 1.0, 3.0, out_mask=om, want_cell_out=True,
                             h_also=nxt[:, K - U:], cell_out_also=av[:, :U])
    got = ops.lstm_cell_gemm_fwd_h(x, img, U, cp, hp, pp, live, 1.0, 3.0, out_mask=om, h_also=nxt2[:, K - U:],
                                   cell_out_also=av2[:, :U])
    rel = lambda g, w: float((g - w).abs().max() / w.abs().max().clamp_min(1e-6))
    for name, g, w in zip(('gates', 'c_raw', 'c_out', 'h_out', 'h_raw', 'cell_out'), got, want):
        assert rel(g, w) < 1e-5, (name, rel(g, w))
    assert rel(nxt2, nxt) < 1e-5 and rel(av2, av) < 1e-5
    dpre = f(B, 4 * U, sc=0.3)
    assert rel(ops.lstm_cell_gemm_bwd_h(dpre, img, K), ops.gemm(dpre, Wr, transB=True)) < 1e-5


@pytest.mark.parametrize('att,prev,sig,dtype', [('location', 'carry', False, 'f32'), ('hybrid', 'zeros', False, 'bf16'),
                                               ('bahdanau_content', 'zeros', True, 'f32'), ('luong_dot', 'zeros', False, 'f32')])
def test_native_greedy_inference_loop(cuda, att, prev, sig, dtype):
    """asr_att_decoder_infer (every decoder step, the output head, argmax, the embedding of the chosen id and the
    per-row finished flags issued from one call; one read-back at the end) against the class-surface path
    (AttentionDecoder.step under dynamic_decode, a device sync per token) and against oracle.attention: ids identical,
    same number of emitted steps.  The end-of-sequence bias is set so that (a) no row ever finishes (all 40 steps), (b) rows
    finish at different steps (imputed zeros behind the first EOS, state copy-through, zeroed context input), (c) every
    row finishes at once (one step; the early exit must not change the result).  Reference:
    models/attention/attention_seq2seq.py:462-509, decoders/dynamic_decoder.py:148-197."""
    from tensorflow_end2end_speech_recognition_amd.models.attention.attention_seq2seq import AttentionSeq2Seq
    rng = np.random.RandomState(5)
    B, T, D, H, L, U, A, Em, C = 5, 70, 12, 64, 1, 128, 32, 8, 9
    if att == 'luong_dot':
        U = 2 * H
    x, sl, labels, lsl, _ = _batch(rng, B, T, D, C)
    model = AttentionSeq2Seq(input_size=D, encoder_type='blstm', encoder_num_units=H, encoder_num_layers=L,
                             encoder_num_proj=None, attention_type=att, attention_dim=A, decoder_type='lstm',
                             decoder_num_units=U, decoder_num_layers=1, embedding_dim=Em, num_classes=C, sos_index=C,
                             eos_index=C + 1, max_decode_length=40, parameter_init=0.1, clip_grad_norm=5.0,
                             clip_activation_encoder=50, clip_activation_decoder=50, dtype=dtype, seed=5,
                             sharpening_factor=1.5, sigmoid_smoothing=sig, prev_alpha=prev)
    lens = []
    for eos_bias in (-50.0, 0.35, 50.0):
        sd = {k: v.clone() for k, v in model.store.state_dict().items()}
        sd['attention_decoder/decoder/output_layer/biases'][C + 1] = eos_bias
        model.store.load_state_dict(sd)
        ids_native = model.infer(x, sl, native=True)
        raw = model._infer_raw
        ids_class = model.infer(x, sl, native=False)
        assert ids_native.shape == ids_class.shape and np.array_equal(ids_native, ids_class), (eos_bias, ids_native, ids_class)
        assert raw['steps'] == ids_native.shape[1] and raw['steps_issued'] >= raw['steps']
        lens.append(ids_native.shape[1])
        if dtype == 'f32':
            sdn = {k: v.cpu().numpy() for k, v in sd.items()}
            ref_ids = oatt.attention_model_infer(sdn, x, sl, L, att, C, C + 1, 40, clip_enc=50.0, clip_dec=50.0,
                                                 sharpening=1.5, sigmoid_smoothing=sig, prev_alpha=prev)
            assert np.array_equal(ids_native, ref_ids), eos_bias
    assert lens[0] == 40 and lens[2] == 1 and 1 <= lens[1] <= 40


# The decoder-loop matrix.  Per case: the scoring configuration, the shape (defaults B = 3, T = 200, U = 64, To = 5,
# Em = 8) and `path`, the kernels every step of the case is MEANT to run -- asserted through ops.att_path_counts:
#   fwd   'fused' (att_fused_fwd_kernel + combine) | '4launch'        cell  'bf16' | 'f32img' | 'gemm' (product, then cell)
#   bwd   'fused_q' (att_dq_cell_bwd_kernel) | 'unfused'              bwd_cell  'bf16' (asr_lstm_cell_gemm_bwd_h) | 'gemm'
#   fold  softmax backward inside the energy backward                 lanes  lane shape of the energy / location kernels
# The first five (and their /one_step and /em64 forms) are the cases this test has had from the start.
_P = lambda fwd, cell, bwd, bwd_cell, fold, lanes: dict(fwd=fwd, cell=cell, bwd=bwd, bwd_cell=bwd_cell, fold=fold, lanes=lanes)
_LOOP_CASES = dict(
    location_zeros_bf16=dict(keys=False, carry=0, sig=False, bf16=True, A=128, E2=512, mode=0, hasq=1, taps=0,
                             path=_P('fused', 'gemm', 'fused_q', 'gemm', True, '32')),
    bahdanau_sigmoid_f32=dict(keys=True, carry=0, sig=True, bf16=False, A=128, E2=256, mode=0, hasq=1, taps=0,
                              path=_P('4launch', 'gemm', 'fused_q', 'gemm', True, '32')),
    location_carry_bf16=dict(keys=False, carry=1, sig=False, bf16=True, A=128, E2=512, mode=0, hasq=1, taps=201,
                             path=_P('4launch', 'gemm', 'unfused', 'gemm', False, '32')),
    hybrid_carry_f32=dict(keys=True, carry=1, sig=True, bf16=False, A=32, E2=256, mode=0, hasq=1, taps=200,
                          path=_P('4launch', 'gemm', 'unfused', 'gemm', False, '16')),
    # (2H = 64 fp32 is below the 16-byte-vector context / d-alpha kernels: general ones, hence no fold)
    luong_dot_small=dict(keys=True, carry=0, sig=False, bf16=False, A=64, E2=64, mode=1, hasq=0, taps=0,
                         path=_P('4launch', 'gemm', 'unfused', 'gemm', False, '16')),
    # ---- att_dq_cell_bwd_kernel's wave layouts (wpu = 8 / A x 64 waves per 64-column slice) and chunk-loop trips
    # wpu = 8; fused forward <16,1,float>; U not a multiple of 64 (three column blocks)
    A64=dict(keys=False, carry=0, sig=False, bf16=False, A=64, E2=256, mode=0, hasq=1, taps=0, U=48,
             path=_P('fused', 'gemm', 'fused_q', 'gemm', True, '16')),
    # wpu = 2; fused forward <64,1,bf16>.  (No fold: the 16-byte-vector d-alpha kernel wants 2H % 512 == 0 in bf16.)
    A256=dict(keys=True, carry=0, sig=False, bf16=True, A=256, E2=256, mode=0, hasq=1, taps=0, B=5, T=300,
              path=_P('fused', 'gemm', 'fused_q', 'gemm', False, '64')),
    # wpu = 1: 10 chunks = a second trip of the chunk loop with a partial tail; <64,2,float>
    A512_long=dict(keys=True, carry=0, sig=False, bf16=False, A=512, E2=512, mode=0, hasq=1, taps=0, T=600,
                   path=_P('fused', 'gemm', 'fused_q', 'gemm', True, '64x2')),
    # wpu = 4: 33 chunks = a second trip of one chunk; a single column block
    A128_chunks33=dict(keys=False, carry=0, sig=False, bf16=True, A=128, E2=256, mode=0, hasq=1, taps=0, U=16, B=2, T=2110,
                       path=_P('fused', 'gemm', 'fused_q', 'gemm', False, '32')),
    # ---- batch: a second row group with clamped rows in the backward kernel, the second MFMA row tile of the one-launch
    # cell (17, 32), and past asr_lstm_cell_gemm_ok's B <= 32 the product + cell pair while fused_q stays on (35)
    B17=dict(keys=True, carry=0, sig=False, bf16=False, A=128, E2=256, mode=0, hasq=1, taps=0, B=17, T=130, Em=64,
             path=_P('fused', 'f32img', 'fused_q', 'gemm', True, '32')),
    B32=dict(keys=True, carry=0, sig=False, bf16=False, A=128, E2=256, mode=0, hasq=1, taps=0, B=32, T=130, Em=64,
             path=_P('fused', 'f32img', 'fused_q', 'gemm', True, '32')),
    B35=dict(keys=True, carry=0, sig=False, bf16=False, A=128, E2=256, mode=0, hasq=1, taps=0, B=35, T=130, Em=64,
             path=_P('fused', 'gemm', 'fused_q', 'gemm', True, '32')),
    # the benchmarked decoder width: 34 workgroups x 2 row groups in the backward kernel
    cfgD_narrow=dict(keys=True, carry=0, sig=False, bf16=True, A=128, E2=512, mode=0, hasq=1, taps=0, B=32, U=512, Em=64, To=3,
                     path=_P('fused', 'f32img', 'fused_q', 'gemm', True, '32')),
    # U % 16 != 0: the fp32 image although the model is bf16 (40 + 512 + 24 = 9 x 64 input columns), no fused_q
    cell_bf16_U24=dict(keys=False, carry=0, sig=False, bf16=True, A=128, E2=512, mode=0, hasq=1, taps=0, U=24, Em=40,
                       cell_bf16=True, path=_P('fused', 'f32img', 'unfused', 'gemm', True, '32')),
    # fused_q off (A = 36), four-launch forward (2H = 64), vectorised 16-lane energies with idle tail lanes
    A36_general_q=dict(keys=True, carry=0, sig=False, bf16=False, A=36, E2=64, mode=0, hasq=1, taps=0,
                       path=_P('4launch', 'gemm', 'unfused', 'gemm', False, '16')),
    # A % 4 != 0: everything general
    A130=dict(keys=True, carry=0, sig=False, bf16=False, A=130, E2=64, mode=0, hasq=1, taps=0,
              path=_P('4launch', 'gemm', 'unfused', 'gemm', False, 'general')),
    # T > 64 chunks: the fused forward is refused; 65 chunks = a second trip at wpu = 8 in the backward kernel
    T4100=dict(keys=False, carry=0, sig=False, bf16=False, A=64, E2=256, mode=0, hasq=1, taps=0, B=1, T=4100, To=2,
               path=_P('4launch', 'gemm', 'fused_q', 'gemm', True, '16')),
    # sigmoid smoothing refuses the fused forward, the fold stays on
    sigmoid_E256=dict(keys=False, carry=0, sig=True, bf16=False, A=128, E2=256, mode=0, hasq=1, taps=0, Em=64,
                      path=_P('4launch', 'f32img', 'fused_q', 'gemm', True, '32')),
    # W_q as a column slice of a [U, A + 1] array: rows 4 bytes off 16-byte alignment refuse fused_q
    unaligned_Wq=dict(keys=False, carry=0, sig=False, bf16=False, A=128, E2=256, mode=0, hasq=1, taps=0, wq_slice=True,
                      path=_P('fused', 'gemm', 'unfused', 'gemm', True, '32')))
_LOOP_ORIGINAL = ['location_zeros_bf16', 'bahdanau_sigmoid_f32', 'location_carry_bf16', 'hybrid_carry_f32',
                  'luong_dot_small', 'bahdanau_sigmoid_f32/one_step', 'location_carry_bf16/one_step',
                  'location_zeros_bf16/em64', 'hybrid_carry_f32/em64']
_LOOP_NEW = ['A64', 'A256', 'A512_long', 'A128_chunks33', 'B17', 'B32', 'B35', 'cfgD_narrow',
             'cell_bf16/location_zeros_bf16/em64', 'cell_bf16/location_carry_bf16/em64', 'cell_bf16/B17', 'cell_bf16_U24',
             'A36_general_q', 'A130', 'T4100', 'sigmoid_E256', 'unaligned_Wq', 'B17/one_step',
             'cell_bf16/location_zeros_bf16/em64/one_step']


def _loop_config(case):
    """case = ['cell_bf16/'] name ['/em64'] ['/one_step'] -> the configuration dict of the loop test (B, T, U, To, Em,
    cell_bf16, seq_len, live and the intended path included)."""
    parts = case.split('/')
    cell_bf16 = parts[0] == 'cell_bf16'
    name = parts[1] if cell_bf16 else parts[0]
    cfg = dict(_LOOP_CASES[name])
    cfg['path'] = dict(cfg['path'])
    cfg.update(name=name, original=case in _LOOP_ORIGINAL, one_step='one_step' in parts, em64='em64' in parts)
    cfg['cell_bf16'] = bool(cfg.get('cell_bf16') or cell_bf16)
    cfg['Em'] = 64 if cfg['em64'] else cfg.get('Em', 8)
    cfg['To'] = 1 if cfg['one_step'] else cfg.get('To', 5)
    cfg.setdefault('B', 3)
    cfg.setdefault('T', 200)
    cfg.setdefault('U', cfg['A'] if not cfg['hasq'] else 64)
    B, T, To = cfg['B'], cfg['T'], cfg['To']
    if cfg['em64'] and cfg['path']['cell'] == 'gemm':
        cfg['path']['cell'] = 'f32img'                       # (Em = 64 makes the first cases' input width a multiple of 64)
    if cell_bf16:
        cfg['path'].update(cell='bf16', bwd_cell='bf16')
    if cfg['original']:
        cfg['seq_len'] = [T, 77, 130]
        cfg['live'] = [[1, 1, 1], [1, 1, 1], [1, 0, 1], [1, 0, 1], [1, 0, 0]][:To]
    else:
        # a full row, a row that ends on a chunk boundary, a one-frame row, the rest anywhere from a third of T on
        sl = np.random.RandomState(B + T).randint(max(1, T // 3), T + 1, size=B)
        sl[0] = T
        if B >= 2:
            sl[1] = 128 if T > 128 else 64
        if B >= 3:
            sl[2] = 1
        cfg['seq_len'] = [int(x) for x in sl]
        # row b finishes at step b % (To + 1): live there for the last time (so step 0 has every row, and with B <= To
        # the last steps have none)
        cfg['live'] = [[1.0 if k <= b % (To + 1) else 0.0 for b in range(B)] for k in range(To)]
    return cfg


def _loop_expected_counts(cfg):
    """The path counters after one forward / one backward loop of To steps on the intended path."""
    p, To = cfg['path'], cfg['To']
    fwd = {'fwd_step_' + p['fwd']: To, 'fwd_cell_' + p['cell']: To}
    if p['fwd'] == 'fused':
        fwd['fused_fwd_' + p['lanes']] = To
    else:
        fwd[('loc_fwd_' if cfg['carry'] else 'energy_fwd_') + p['lanes']] = To
    bwd = {'bwd_step_' + p['bwd']: To, 'bwd_cell_' + p['bwd_cell']: To,
           'bwd_softmax_' + ('folded' if p['fold'] else 'separate'): To,
           ('loc_bwd_' if cfg['carry'] else 'energy_bwd_') + p['lanes']: To}
    return fwd, bwd


def _loop_arrays(cfg):
    """The loop's operands on the CPU (fp32 tensors; ints / floats as they are) and the shapes of the backward's outputs."""
    rng = np.random.RandomState(len(cfg['name']))
    B, T, To, Em, A, E2, U = cfg['B'], cfg['T'], cfg['To'], cfg['Em'], cfg['A'], cfg['E2'], cfg['U']
    Din = Em + E2 + U
    f = lambda *s, sc=1.0: torch.tensor(rng.randn(*s) * sc, dtype=torch.float32)
    seq_len = torch.tensor(cfg['seq_len'], dtype=torch.int32)
    live = torch.tensor(cfg['live'], dtype=torch.float32).contiguous()   # [To,B]
    enc = f(T, B, E2, sc=0.5)
    enc = enc * (torch.arange(T).view(T, 1, 1) < seq_len.view(1, B, 1))
    if cfg['bf16']:
        enc = enc.to(torch.bfloat16)
    a = dict(To=To, B=B, T=T, U=U, Em=Em, E2=E2, A=A, att_mode=cfg['mode'], has_query_fc=cfg['hasq'],
             carry_alpha=cfg['carry'], taps=cfg['taps'], enc_dtype=1 if cfg['bf16'] else 0, forget_bias=1.0,
             cell_clip=3.0, sharpening=1.5,
             W_cell=f(Din, 4 * U, sc=0.08), b_cell=f(4 * U, sc=0.1), peep=f(3, U, sc=0.1),
             W_q=f(U, A, sc=0.1) if cfg['hasq'] else None, b_q=f(A, sc=0.1) if (cfg['hasq'] and cfg['carry']) else None,
             v=f(A, sc=0.5) if cfg['mode'] == 0 else None,
             keys=(enc.float() if cfg['name'] == 'luong_dot_small' else f(T, B, A, sc=0.5)) if cfg['keys'] else None,
             enc=enc, seq_len=seq_len,
             filt=f(cfg['taps'], 1, 10, sc=0.3) if cfg['carry'] else None, wfil=f(10, A, sc=0.3) if cfg['carry'] else None,
             alpha_zero=torch.zeros(B, T) if cfg['carry'] else None, live=live,
             dmask=(torch.tensor(rng.rand(To, B, U) < 0.8, dtype=torch.float32) / 0.8),
             dec_in=f(To, B, Din, sc=0.5), av_in=torch.zeros(To, B, U + E2), alpha_all=torch.zeros(To, B, T),
             snorm_all=torch.zeros(To, B) if cfg['sig'] else None, gates_all=torch.zeros(To, B, 4 * U),
             craw_all=torch.zeros(To, B, U), c_all=torch.zeros(To + 1, B, U), h_all=torch.zeros(To + 1, B, U),
             qz_all=torch.zeros(To, B, A))
    a['c_all'][0] = f(B, U, sc=0.3)
    a['h_all'][0] = f(B, U, sc=0.3)
    a['dec_in'][0, :, Em:Em + E2] = 0.0                      # no context before the first step
    a['dec_in'][0, :, Em + E2:] = a['h_all'][0]
    if cfg['cell_bf16']:
        # both sides get weights that ARE bf16 values: the device's rounding into its bf16 images is then the identity
        # and the float64 statement applies unchanged
        a['W_cell'] = a['W_cell'].to(torch.bfloat16).float()
        a['cell_bf16'] = True
    bwd_in = dict(dav_cell=f(To, B, U, sc=0.3), dav_ctx=f(To, B, E2, sc=0.3))
    bwd_out = dict(dctx_all=(To, B, E2), dpre_all=(To, B, 4 * U), dqz_all=(To, B, A),
                   dv_all=(To, B, A) if cfg['mode'] == 0 else None, dpeep_all=(To, B, 3 * U), d_in_all=(To, B, Din),
                   dkeys=(T, B, A) if cfg['keys'] else None, dwfil_rows=(B, 10, A) if cfg['carry'] else None,
                   dfilt_rows=(B, cfg['taps'], 10) if cfg['carry'] else None, dc0=(B, U), dh0=(B, U))
    return a, bwd_in, bwd_out


def _loop_clone(cfg, a, bwd_in, bwd_out, dev):
    d = {k: (v.clone().to(dev) if torch.is_tensor(v) else v) for k, v in a.items()}
    d.update({k: v.clone().to(dev) for k, v in bwd_in.items()})
    d.update({k: (torch.zeros(s, device=dev) if s is not None else None) for k, s in bwd_out.items()})
    if cfg.get('wq_slice'):            # the same values as the first A columns of a [U, A + 1] array: row stride A + 1
        wide = torch.zeros(cfg['U'], cfg['A'] + 1, device=dev)
        wide[:, :cfg['A']] = d['W_q']
        d['W_q'] = wide[:, :cfg['A']]
        assert d['W_q'].stride(0) % 4 != 0
    return d


_LOOP_FWD = ('alpha_all', 'av_in', 'dec_in', 'c_all', 'h_all', 'qz_all', 'gates_all', 'craw_all')


@pytest.mark.parametrize('case', _LOOP_ORIGINAL + _LOOP_NEW)
def test_native_decoder_loop_against_the_step_by_step_statement(cuda, monkeypatch, case):
    """asr_att_decoder_fwd / _bwd (all To steps from one call, with the fused kernels the loop uses: dctx add inside the
    4-frame d-alpha kernel, softmax backward folded into the energy backward through partial alpha.dalpha sums, dropout
    mask and carried-dh add inside the cell backward, length-limited vectorised energy / location kernels with exp2-rcp
    tanh, skinny MFMA products) against tests/_cpu_ops.py's step-by-step float64 statement of the same loop -- at
    widths that select those kernels (A = 128 -> 32 lanes x float4 per frame, 2H = 512 bf16 / 256 fp32 -> 16-byte
    encoder vectors, T = 200 -> four 64-frame chunks), which the small model-level parity tests do not reach.  The
    luong_dot_small case (A = U = 2H = 64, dot-product scoring without a query FC) takes the general context kernels.
    The cases behind the first nine walk the loop's dispatch (_LOOP_CASES says what each one reaches): every layout of
    att_dq_cell_bwd_kernel, both trips of its chunk loop, B past one row group and past the one-launch cell, the bf16
    cell-weight images inside both loops, every refusal of the fused forward step and of fused_q.  Every case asserts the
    kernels it ran through ops.att_path_counts."""
    import _cpu_ops as cpu
    from tensorflow_end2end_speech_recognition_amd import ops
    cfg = _loop_config(case)
    em64 = cfg['em64'] and cfg['original']   # cell input width % 64 == 0: product + cell as ONE launch (asr_lstm_cell_gemm_fwd)
    a, bwd_in, bwd_out = _loop_arrays(cfg)
    clone_to = lambda dev: _loop_clone(cfg, a, bwd_in, bwd_out, dev)
    want_fwd, want_bwd = _loop_expected_counts(cfg)
    ref, got = clone_to('cpu'), clone_to(cuda)
    cpu._att_decoder_fwd(ref)
    ops.reset_att_path_counts(0)
    ops.att_decoder_fwd(got)
    assert _counted(ops) == want_fwd
    assert (got.get('W_cell_il') is not None) == (cfg['path']['cell'] == 'f32img')
    assert (got.get('W_cell_h') is not None) == (cfg['path']['cell'] == 'bf16')
    if em64:       # the one-launch product + cell against the two launches it replaces: the whole loop bit for bit
        two = clone_to(cuda)
        monkeypatch.setattr(ops, 'FUSED_CELL_GEMM', False)
        ops.att_decoder_fwd(two)
        monkeypatch.setattr(ops, 'FUSED_CELL_GEMM', True)
        assert two.get('W_cell_il') is None
        for name in _LOOP_FWD:
            assert torch.equal(got[name], two[name]), name
    # relative to the array's largest entry, with a floor: without keys and without carried location features every frame
    # has the same energy, so dqz / dv are (sum_t denergy) x const = rounding noise around zero (1e-7) on both sides
    rel = lambda x, y: float(np.abs(x.cpu().double().numpy() - y.double().numpy()).max() / max(np.abs(y.double().numpy()).max(), 1e-2))
    for name in _LOOP_FWD + (('snorm_all',) if cfg['sig'] else ()):
        err = rel(got[name], ref[name])
        print('%s fwd %s %.3g' % (case, name, err))
        assert err < 2e-5, (name, err)
    # the backward of both sides starts from the SAME saved forward (the reference's), so the comparison is per kernel
    for name in _LOOP_FWD + ('snorm_all',):
        if ref.get(name) is not None:
            got[name].copy_(ref[name].to(cuda))
    cpu._att_decoder_bwd(ref)
    ops.reset_att_path_counts(0)
    ops.att_decoder_bwd(got)
    assert _counted(ops) == want_bwd
    for name, shape in bwd_out.items():
        if shape is not None:
            err = rel(got[name], ref[name])
            print('%s bwd %s %.3g' % (case, name, err))
            assert err < 5e-5, (name, err)
    assert ops.check_async_errors(0) == 0


# the greedy loop at the widths of the one-launch cell: seed under which the float64 statement's top-2 logit margin
# is above 1e-3 at every (step, row) -- asserted below, so the exact id comparison cannot be excused by a near-tie
_INFER_SEED = 5


def _infer_arrays(cell_bf16, seed=_INFER_SEED):
    rng = np.random.RandomState(seed)
    B, T, To, Em, E2, U, A, C2 = 32, 130, 12, 64, 256, 64, 128, 40
    Din = Em + E2 + U
    f = lambda *s, sc=1.0: torch.tensor(rng.randn(*s) * sc, dtype=torch.float32)
    seq_len = torch.tensor(rng.randint(T // 3, T + 1, size=B), dtype=torch.int32)
    seq_len[0], seq_len[1], seq_len[2] = T, 128, 1
    enc = f(T, B, E2, sc=0.5) * (torch.arange(T).view(T, 1, 1) < seq_len.view(1, B, 1))
    W_cell = f(Din, 4 * U, sc=0.08)
    emb = f(C2, Em, sc=0.5)
    live = torch.zeros(To + 1, B)
    live[0] = 1.0
    a = dict(To=To, B=B, T=T, U=U, Em=Em, E2=E2, A=A, att_mode=0, has_query_fc=1, carry_alpha=0, taps=0, enc_dtype=0,
             forget_bias=1.0, cell_clip=3.0, sharpening=1.5,
             W_cell=W_cell.to(torch.bfloat16).float() if cell_bf16 else W_cell, b_cell=f(4 * U, sc=0.1),
             peep=f(3, U, sc=0.1), W_q=f(U, A, sc=0.1), v=f(A, sc=0.5), keys=f(T, B, A, sc=0.5), enc=enc, seq_len=seq_len,
             live=live, dec_in=torch.zeros(To, B, Din), av_in=torch.zeros(To, B, U + E2), alpha_all=torch.zeros(To, B, T),
             gates_all=torch.zeros(To, B, 4 * U), craw_all=torch.zeros(To, B, U), c_all=torch.zeros(To + 1, B, U),
             h_all=torch.zeros(To + 1, B, U), qz_all=torch.zeros(To, B, A))
    if cell_bf16:
        a['cell_bf16'] = True
    a['c_all'][0] = f(B, U, sc=0.3)
    a['h_all'][0] = f(B, U, sc=0.3)
    a['dec_in'][0, :, :Em] = emb[C2 - 2]                     # <SOS>
    a['dec_in'][0, :, Em + E2:] = a['h_all'][0]
    head = dict(W_av=f(U + E2, U, sc=0.15), W_out=f(U, C2, sc=0.6), b_out=f(C2, sc=0.3), embedding=emb)
    head['b_out'][C2 - 1] = 2.0                              # <EOS>: rows finish at different steps
    return a, head, C2 - 1


@pytest.mark.parametrize('cell_bf16', [False, True])
def test_native_inference_loop_at_the_fused_cell_widths(cuda, cell_bf16):
    """asr_att_decoder_infer against _cpu_ops._att_decoder_infer at B = 32, Em = 64, 2H = 256, U = 64 (384 input
    columns: product + cell in one launch, two MFMA row tiles), A = 128, 12 steps, 40 classes, on the fp32 image and on
    the bf16 images (weights that are bf16 values on both sides).  The end-of-sequence bias makes rows finish at
    different steps.  Logits and attentional vectors within the loop test's forward bound; ids, finished flags and live
    counts exactly -- legitimate because the statement's top-2 logit margin is above 1e-3 everywhere (asserted first)."""
    import _cpu_ops as cpu
    from tensorflow_end2end_speech_recognition_amd import ops
    a, head, eos = _infer_arrays(cell_bf16)
    To, B = a['To'], a['B']
    dev = lambda d: {k: (v.clone().to(cuda) if torch.is_tensor(v) else v) for k, v in d.items()}
    cl = lambda d: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in d.items()}
    ra = cl(a)
    ref = cpu._att_decoder_infer(ra, head['W_av'], head['W_out'], head['b_out'], head['embedding'], eos, B, check_every=0)
    top2 = ref['logits'].double().topk(2, dim=2).values
    assert float((top2[..., 0] - top2[..., 1]).min()) > 1e-3
    fin = (ref['live'][:To].sum(0)).numpy()                  # steps each row was live for
    assert len(set(fin.tolist())) >= 4 and fin.min() < To and ref['steps_issued'] == To
    ga, gh = dev(a), dev(head)
    ops.reset_att_path_counts(0)
    got = ops.att_decoder_infer(ga, gh['W_av'], gh['W_out'], gh['b_out'], gh['embedding'], eos, B, check_every=0)
    torch.cuda.synchronize()
    assert got['steps_issued'] == To
    assert _counted(ops) == {'fwd_step_fused': To, 'fused_fwd_32': To, ('fwd_cell_bf16' if cell_bf16 else 'fwd_cell_f32img'): To}
    rel = lambda x, y: float(np.abs(x.cpu().double().numpy() - y.double().numpy()).max() / max(np.abs(y.double().numpy()).max(), 1e-2))
    for name in ('logits', 'av'):
        err = rel(got[name], ref[name])
        print('infer %s %s %.3g' % ('bf16' if cell_bf16 else 'f32', name, err))
        assert err < 2e-5, (name, err)
    assert torch.equal(got['ids'].cpu(), ref['ids'])
    assert torch.equal(got['live'].cpu(), ref['live'])
    assert torch.equal(got['live_count'].cpu(), ref['live_count'])
    assert ops.check_async_errors(0) == 0


def test_first_maximum_of_tied_logits_in_the_loops_and_argmax_rows(cuda):
    """The one first-maximum argmax behind asr_argmax_rows, the greedy loop's selection and the scheduled-sampling loop's:
    on logits that tie EXACTLY at the row maximum, all three give numpy's answer (the first index) on the very logits the
    loops returned -- no tolerance.  C2 = 300 > 256, so a thread of the 256-wide scan meets a second column (261 = 5 + 256).
    Row 0 ties at columns 5, 70 and 261 (-> 5), row 1 at 261 and 299 (-> 261), row 2 has its maximum at 261 alone.
    How the ties come about: columns 5 and 70 of the output layer are duplicates, 261 and 299 differ from them (and from
    each other) only in the weights of the attentional units 0 and 1, and those units are exactly 0 for row 0 / row 1:
    their only input is a context column in which that row's encoder frames are zero, tanh(0) = 0, and a product with an
    exact zero adds nothing to a column's sum.  (Four identical columns would tie in every row alike and could not tell
    the rows apart.)  The ties are asserted before anything is concluded from them.  <EOS> is none of these columns and
    far below them, so every row stays live for all four steps."""
    from tensorflow_end2end_speech_recognition_amd import ops
    rng = np.random.RandomState(11)
    B, T, U, E2, Em, A, To, C2 = 3, 8, 16, 16, 8, 16, 4, 300
    Din, eos = Em + E2 + U, 298
    f = lambda *s, sc=1.0: torch.tensor(rng.randn(*s) * sc, dtype=torch.float32)
    seq_len = torch.tensor([8, 5, 1], dtype=torch.int32)
    enc = f(T, B, E2, sc=0.5)
    enc[:, :, 0] = torch.tensor([0.0, 1.0, 1.0])             # row 0: context column 0 is zero -> attentional unit 0 is
    enc[:, :, 1] = torch.tensor([1.0, 0.0, 1.0])             # row 1: context column 1                  -> unit 1
    enc[:, :, 2] = 1.0                                       # every row: unit 2 is tanh(2 x 1), the tied columns' lead
    enc = enc * (torch.arange(T).view(T, 1, 1) < seq_len.view(1, B, 1))
    W_av = f(U + E2, U, sc=0.15)
    W_av[:, :3] = 0.0
    W_av[U, 0] = W_av[U + 1, 1] = W_av[U + 2, 2] = 2.0
    W_out, b_out = f(U, C2, sc=0.05), f(C2, sc=0.05)
    for col, (x, y) in {5: (0.0, 1.0), 70: (0.0, 1.0), 261: (1.0, 1.0), 299: (1.0, 0.0)}.items():
        W_out[:, col] = W_out[:, 5]
        W_out[0, col], W_out[1, col], W_out[2, col] = x, y, 5.0
        b_out[col] = b_out[5]
    b_out[eos] = -10.0
    emb = f(C2, Em, sc=0.5)

    def loop_dict(n_live_rows):
        a = dict(To=To, B=B, T=T, U=U, Em=Em, E2=E2, A=A, att_mode=0, has_query_fc=1, carry_alpha=0, taps=0, enc_dtype=0,
                 forget_bias=1.0, cell_clip=3.0, sharpening=1.5, W_cell=f(Din, 4 * U, sc=0.08), b_cell=f(4 * U, sc=0.1),
                 peep=f(3, U, sc=0.1), W_q=f(U, A, sc=0.1), v=f(A, sc=0.5), keys=f(T, B, A, sc=0.5), enc=enc, seq_len=seq_len,
                 live=torch.ones(n_live_rows, B), dec_in=torch.zeros(To, B, Din), av_in=torch.zeros(To, B, U + E2),
                 alpha_all=torch.zeros(To, B, T), gates_all=torch.zeros(To, B, 4 * U), craw_all=torch.zeros(To, B, U),
                 c_all=torch.zeros(To + 1, B, U), h_all=torch.zeros(To + 1, B, U), qz_all=torch.zeros(To, B, A))
        a['c_all'][0], a['h_all'][0] = f(B, U, sc=0.3), f(B, U, sc=0.3)
        a['dec_in'][0, :, :Em] = emb[7]
        a['dec_in'][0, :, Em + E2:] = a['h_all'][0]
        return {k: (v.to(cuda) if torch.is_tensor(v) else v) for k, v in a.items()}

    def first_maxima(logits):
        """numpy's argmax of the loop's own logits [To,B,C2], after checking that the ties are there."""
        lg = logits.cpu().numpy()
        for k in range(To):
            top = lg[k].max(axis=1)
            assert [sorted(np.flatnonzero(lg[k, b] == top[b]).tolist()) for b in range(B)] == [[5, 70, 261], [261, 299], [261]]
        want = lg.argmax(axis=2)
        assert (want == np.array([5, 261, 261])).all()
        assert np.array_equal(ops.argmax_rows(logits.view(To * B, C2)).cpu().numpy().reshape(To, B), want)
        return want

    head = [t.to(cuda) for t in (W_av, W_out, b_out, emb)]
    a = loop_dict(To + 1)
    a['live'][1:] = 0.0                                      # (the loop writes rows 1 ..)
    got = ops.att_decoder_infer(a, *head, eos, B, check_every=0)
    torch.cuda.synchronize()
    want = first_maxima(got['logits'])
    assert bool((got['live'][:To] == 1.0).all()) and got['steps_issued'] == To
    assert np.array_equal(got['ids'].cpu().numpy(), want)
    teacher = torch.full((To, B), 7, dtype=torch.int32, device=cuda)
    _, logits, ids_fed = ops.att_decoder_fwd_ss(loop_dict(To), *head, teacher, torch.ones(To, B, device=cuda), None)
    torch.cuda.synchronize()
    want = first_maxima(logits)
    assert np.array_equal(ids_fed.cpu().numpy()[1:], want[:To - 1])
    assert ops.check_async_errors(0) == 0


@pytest.mark.parametrize('att,prev,sig', [('bahdanau_content', 'zeros', False), ('location', 'carry', False),
                                          ('hybrid', 'carry', True), ('luong_dot', 'zeros', False),
                                          ('luong_concat', 'zeros', False)])
def test_attention_class_surface(cuda, att, prev, sig):
    """AttentionLayer / LSTMDecoderCell / AttentionDecoder under dynamic_decode with a TrainingHelper, and
    InitialStateBridge (models/attention/decoders/*.py, bridge.py) on the HIP kernels: teacher-forced logits / weights /
    ids equal the oracle's and the model's own fused loop (asr_att_decoder_fwd); a standalone AttentionLayer equals
    oracle.attention.attention_step.  (Greedy inference -- the path these classes serve in the model -- is checked
    bit-exact against the oracle by every test_attention_model_parity case.)"""
    import _config_parity as cp
    r = cp.run_class_surface('cuda:0', att, prev, sig, B=5, T=70, To=6, D=12, H=64, L=1, U=128, A=32, Em=8, C=9)
    assert r['loss_rel'] < 1e-4, r['report']
    assert r['class_logits_vs_oracle'] < 2e-4 and r['class_alpha_vs_oracle'] < 1e-5 and r['class_ids_vs_oracle'] == 0, r['report']
    assert r['class_logits_vs_fused'] < 2e-4 and r['class_alpha_vs_fused'] < 1e-5, r['report']
    assert r['layer_alpha'] < 1e-5 and r['layer_ctx'] < 2e-4, r['report']


def test_bridge_classes(cuda):
    import _config_parity as cp
    r = cp.run_bridges('cuda:0')
    assert r['fc_err'] < 1e-5 and r['ok_zero'] and r['ok_pass'] and r['raised'], r
