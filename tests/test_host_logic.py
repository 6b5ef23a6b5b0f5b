"""Host logic above the kernels, on the CPU: the models are run with the kernel front end (`ops`) swapped for the
torch/oracle stand-ins of tests/_cpu_ops.py, and compared with the oracle's end-to-end models.  What this pins is
the Python side -- which tensors are fed to which GEMM, how weight / bias / peephole gradients are assembled from
the BPTT output, the head and loss composition, the clip -> optimizer sequence -- not kernel numerics (GPU tests)."""
import os
import sys

import numpy as np
import pytest
import torch

import _cpu_ops
from oracle import model as omodel
from oracle import optim as oopt


def _batch(rng, B, T, D, C, div=4):
    x = rng.randn(B, T, D).astype(np.float32)
    sl = rng.randint(max(2, T // 2), T + 1, size=B).astype(np.int32)
    sl[0] = T
    labs = []
    for b in range(B):
        x[b, sl[b]:] = 0
        labs.append([int(v) for v in rng.randint(0, C, size=max(1, sl[b] // div))])
    dense = np.full((B, max(len(l) for l in labs)), -1, dtype=np.int64)
    for b, l in enumerate(labs):
        dense[b, :len(l)] = l
    return x, sl, labs, dense


def _check_grads(opt, loss, model, ref, tol=1e-4):
    seen = set()
    for g, name in opt.compute_gradients(loss, model=model):
        r = ref['grads'][name]
        seen.add(name)
        err = np.abs(g.numpy() - r).max()
        assert err < tol * max(np.abs(r).max(), 1e-3) + 1e-7, (name, err, np.abs(r).max())
    assert seen == set(ref['grads'])


@pytest.mark.parametrize('enc,L,bn,wd', [('blstm', 2, None, 0.0), ('lstm', 2, None, 0.0), ('blstm', 1, 12, 1e-3)])
def test_ctc_model_host_logic(monkeypatch, enc, L, bn, wd):
    _cpu_ops.install(monkeypatch)
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    rng = np.random.RandomState(5)
    B, T, D, H, C = 5, 11, 6, 8, 6                    # B is padded to 16 utterances inside the encoder
    x, sl, labs, dense = _batch(rng, B, T, D, C)
    model = CTC(encoder_type=enc, input_size=D, num_units=H, num_layers=L, num_classes=C, parameter_init=0.1,
                clip_grad_norm=0.05, clip_activation=50, bottleneck_dim=bn, weight_decay=wd, dtype='f32', seed=3,
                device='cpu')
    sd = {k: v.numpy().copy() for k, v in model.store.state_dict().items()}
    for k in sd:
        if k.endswith('/bias') or k.endswith('/biases'):
            sd[k] = (rng.randn(*sd[k].shape) * 0.05).astype(np.float32)
    model.store.load_state_dict({k: torch.tensor(v) for k, v in sd.items()})
    ref = omodel.ctc_model_forward(sd, x, labs, sl, L, ndir=2 if enc == 'blstm' else 1, cell_clip=50.0,
                                   weight_decay=wd, bottleneck=bn is not None)
    loss, logits = model.compute_loss(x, dense, sl, keep_prob=1.0)
    assert abs(loss.item() - ref['total_loss']) / abs(ref['total_loss']) < 1e-5
    assert np.abs(logits.numpy() - ref['logits']).max() < 1e-5
    opt = model._set_optimizer('sgd', 0.1)
    _check_grads(opt, loss, model, ref)
    # one full training step: per-variable clip, then the update (model_base.py:97-152)
    before = {k: v.numpy().copy() for k, v in model.store.state_dict().items()}
    loss, _ = model.compute_loss(x, dense, sl, keep_prob=1.0)
    model.train(loss, 'momentum', 0.1)
    after = model.store.state_dict()
    for name, r in ref['grads'].items():
        want = before[name] - 0.1 * oopt.clip_by_norm(r, 0.05)          # first momentum step: v = g
        assert np.abs(after[name].numpy() - want).max() < 1e-5, name
    # decode / LER plumbing
    dec = model.decoder(logits, sl, beam_width=1)
    from tensorflow_end2end_speech_recognition_amd.utils.io.labels.sparsetensor import list2sparsetensor
    assert 0.0 <= model.compute_ler(dec, list2sparsetensor(dense, -1))


@pytest.mark.parametrize('enc,L', [('bgru', 2), ('gru', 2), ('bgru', 1)])
def test_gru_ctc_model_host_logic(monkeypatch, enc, L):
    """CTC(encoder_type='gru' | 'bgru') (models/ctc/ctc.py:150-155, models/encoders/core/gru.py) on the CPU stand-ins
    against the oracle's GRU model: loss, logits, every gradient (the hoisted x-projections, the shifted h_prev /
    same-frame r*h weight-gradient products, bias column sums, dx through both kernels), final states, one step."""
    _cpu_ops.install(monkeypatch)
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    rng = np.random.RandomState(6)
    B, T, D, H, C = 5, 10, 6, 16, 6
    x, sl, labs, dense = _batch(rng, B, T, D, C)
    ndir = 2 if enc == 'bgru' else 1
    model = CTC(encoder_type=enc, input_size=D, num_units=H, num_layers=L, num_classes=C, parameter_init=0.3,
                clip_grad_norm=5.0, dtype='bf16', seed=3, device='cpu')      # dtype request falls back to fp32
    sd = {k: v.numpy().copy() for k, v in model.store.state_dict().items()}
    assert all(np.all(sd[k] == 1.0) for k in sd if k.endswith('gates/bias'))   # GRUCell: gate bias starts at one
    for k in sd:
        if k.endswith('/bias') or k.endswith('/biases'):
            sd[k] = sd[k] + (rng.randn(*sd[k].shape) * 0.05).astype(np.float32)
    model.store.load_state_dict({k: torch.tensor(v) for k, v in sd.items()})
    ref = omodel.gru_ctc_model_forward(sd, x, labs, sl, L, ndir=ndir)
    loss, logits = model.compute_loss(x, dense, sl, keep_prob=1.0)
    assert abs(loss.item() - ref['total_loss']) / abs(ref['total_loss']) < 1e-5
    assert np.abs(logits.numpy() - ref['logits']).max() < 1e-5
    fin = model.encoder._finals[-1]
    want = ref['final'] if ndir == 2 else (ref['final'],)
    for d in range(ndir):
        assert np.abs(fin[d, :B].numpy() - want[d].detach().numpy()).max() < 1e-5
    opt = model._set_optimizer('sgd', 0.1)
    _check_grads(opt, loss, model, ref)
    # dropout masks (given explicitly) and one optimizer step
    masks = [torch.tensor((rng.rand(T, 16, ndir * H) < 0.8) / 0.8, dtype=torch.float32) for _ in range(L)]
    refd = omodel.gru_ctc_model_forward(sd, x, labs, sl, L, ndir=ndir,
                                        drop_masks=[m[:, :B].double() for m in masks])
    model.encoder(torch.tensor(x), torch.tensor(sl), 0.8, True, drop_masks=masks)
    assert np.abs(model.encoder._out_tm[:, :B].numpy() - refd['enc']).max() < 1e-5
    loss, _ = model.compute_loss(x, dense, sl, keep_prob=1.0)
    model.train(loss, 'adam', 1e-2)
    loss2, _ = model.compute_loss(x, dense, sl, keep_prob=1.0)
    assert loss2.item() < loss.item()


@pytest.mark.parametrize('proj', [None, 5])
def test_cldnn_ctc_model_host_logic(monkeypatch, proj):
    """CTC(encoder_type='cldnn_wang') (models/encoders/core/cldnn_wang.py) on the CPU stand-ins against the oracle:
    the three strided SAME convolutions as im2col + GEMM (chunked over frames), the BLSTM stack on their flattened
    output, fc1 / fc2, and every gradient back through col2im.  proj: lstm_impl='LSTMCell' with num_proj (cldnn_wang.py:202)."""
    _cpu_ops.install(monkeypatch)
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    from tensorflow_end2end_speech_recognition_amd.models.encoders.core import cldnn_wang
    monkeypatch.setattr(cldnn_wang, 'CHUNK_FRAMES', 7)              # several chunks, the last one partial
    rng = np.random.RandomState(9)
    B, T, F, W, H, L, C = 3, 6, 7, 5, 8, 1, 5
    D = F * W * 3
    x, sl, labs, dense = _batch(rng, B, T, D, C, div=3)
    model = CTC(encoder_type='cldnn_wang', input_size=3 * F, splice=W, num_units=H, num_layers=L, num_classes=C,
                parameter_init=0.1, clip_grad_norm=5.0, clip_activation=50, dtype='f32', seed=4, device='cpu',
                **(dict(lstm_impl='LSTMCell', num_proj=proj) if proj else {}))
    sd = {k: v.numpy().copy() for k, v in model.store.state_dict().items()}
    assert sd['CNN1/conv/weight'].shape == (11, 21, 3, 32) and sd['CNN2/conv/weight'].shape == (11, 11, 32, 32)
    assert sd['CNN3/conv/weight'].shape == (3, 3, 32, 96) and sd['fc1/weights'].shape == (2 * (proj or H), 896)
    assert sd['fc2/weights'].shape == (896, 74) and sd['output/weights'].shape == (74, C + 1)
    for k in sd:
        if k.endswith('/bias') or k.endswith('/biases'):
            sd[k] = (rng.randn(*sd[k].shape) * 0.05 + 0.02).astype(np.float32)
    model.store.load_state_dict({k: torch.tensor(v) for k, v in sd.items()})
    ref = omodel.cldnn_ctc_model_forward(sd, x, labs, sl, L, F, W, cell_clip=50.0, proj=bool(proj))
    loss, logits = model.compute_loss(x, dense, sl, keep_prob=1.0)
    assert abs(loss.item() - ref['total_loss']) / abs(ref['total_loss']) < 1e-5
    assert np.abs(logits.numpy() - ref['logits']).max() < 1e-5
    assert np.abs(model.encoder._out_tm[:, :B].numpy() - ref['enc']).max() < 1e-5
    opt = model._set_optimizer('sgd', 0.1)
    _check_grads(opt, loss, model, ref)
    # dropout path runs and a training step lowers the loss
    l0 = None
    for it in range(6):
        l, _ = model.compute_loss(x, dense, sl, keep_prob=0.9)
        model.train(l, 'adam', 2e-3)
        l0 = l.item() if l0 is None else l0
    assert l.item() < l0


@pytest.mark.parametrize('enc,L,bn,bucket_mb', [('blstm', 3, None, '0'), ('lstm', 2, 12, '0'), ('blstm', 3, None, '6'),
                                                ('blstm', 4, None, '0.008')])
def test_bucketed_gradient_averaging_is_the_single_bucket_arithmetic(monkeypatch, enc, L, bn, bucket_mb):
    """utils/training/multi_gpu.BucketedAverager (clip + tower mean per encoder layer as soon as the layer's gradients
    are issued, the rest after the backward pass): its buckets partition the flat gradient buffer, the hook fires for
    every layer top-down, and the clipped gradients equal those of the single-bucket path bit for bit (one rank: the
    mean is the identity; N ranks are covered by the gloo tests of the recipes, which run this path)."""
    _cpu_ops.install(monkeypatch)
    # ASR_DP_BUCKET_MB: consecutive layers (top down) share a collective until the group holds that many MB;
    # 0 = every layer alone, 6 (default) = one group at these toy widths, 0.008 = two groups of two ~6 KB layers
    monkeypatch.setenv('ASR_DP_BUCKET_MB', bucket_mb)
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    from tensorflow_end2end_speech_recognition_amd.utils.training import multi_gpu
    rng = np.random.RandomState(8)
    B, T, D, H, C = 4, 9, 6, 8, 5
    x, sl, labs, dense = _batch(rng, B, T, D, C)
    model = CTC(encoder_type=enc, input_size=D, num_units=H, num_layers=L, num_classes=C, parameter_init=0.3,
                clip_grad_norm=0.02, clip_activation=50, bottleneck_dim=bn, dtype='f32', seed=3, device='cpu')
    opt = model._set_optimizer('sgd', 0.1)
    loss, _ = model.compute_loss(x, dense, sl, keep_prob=1.0)
    gv = opt.compute_gradients(loss, model=model)
    model._clip_gradients(gv)
    want = model.store.grad.clone()
    avg = multi_gpu.averager_for(model)
    groups = [b['layers'] for b in avg.buckets]
    assert avg.ok and len(avg.buckets) == {'0': L, '6': 1, '0.008': 2}[bucket_mb], groups
    assert groups[0][1] == L - 1 and groups[-1][0] == 0 and all(a[0] == b[1] + 1 for a, b in zip(groups, groups[1:]))
    spans = sorted((b['start'], b['end']) for b in avg.buckets + avg.rest)
    assert spans[0][0] == 0 and spans[-1][1] == model.store.total
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    order = []
    orig = avg.layer_ready
    monkeypatch.setattr(avg, 'layer_ready', lambda li, layer: (order.append(li), orig(li, layer)))
    avg.force = True
    loss, _ = model.compute_loss(x, dense, sl, keep_prob=1.0)
    multi_gpu.clip_and_average(model, opt, loss)
    assert order == list(reversed(range(L)))
    assert torch.equal(model.store.grad, want)
    assert model.encoder.grad_ready_hook is None
    # a rank with an empty shard: zero gradients through the same sequence of buckets
    multi_gpu.clip_and_average(model, opt, None)
    assert float(model.store.grad.abs().sum()) == 0.0
    # weight decay adds its gradient term over the whole buffer after the backward pass: single bucket
    m2 = CTC(encoder_type=enc, input_size=D, num_units=H, num_layers=L, num_classes=C, weight_decay=1e-3,
             dtype='f32', seed=3, device='cpu')
    assert not multi_gpu.averager_for(m2).ok


@pytest.mark.parametrize('enc,Lm,Ls,bn,proj', [('multitask_blstm', 3, 2, None, None), ('multitask_blstm', 2, 2, 10, None),
                                               ('multitask_blstm', 3, 1, None, None), ('multitask_lstm', 3, 1, None, None),
                                               ('multitask_blstm', 3, 2, None, 5), ('multitask_blstm', 2, 1, 10, 4)])
def test_multitask_ctc_host_logic(monkeypatch, enc, Lm, Ls, bn, proj):
    """The second head and the join of its gradient inside the encoder stack (models/ctc/multitask_ctc.py,
    models/encoders/core/multitask_blstm.py) against the oracle's multitask model.  proj: lstm_impl='LSTMCell' with
    num_proj (multitask_blstm.py:95 hands it to the cell builder of blstm.py:187-230) -- the sub head on the projected
    outputs of layer num_layers_sub, its gradient joined there."""
    _cpu_ops.install(monkeypatch)
    from tensorflow_end2end_speech_recognition_amd.models.ctc.multitask_ctc import MultitaskCTC
    from tensorflow_end2end_speech_recognition_amd.utils.io.labels.sparsetensor import list2sparsetensor
    rng = np.random.RandomState(17)
    B, T, D, H, Cm, Cs, w = 4, 10, 6, 8, 7, 3, 0.7
    x, sl, labs_m, dense_m = _batch(rng, B, T, D, Cm)
    labs_s = [[int(v) for v in rng.randint(0, Cs, size=max(1, int(sl[b]) // 5))] for b in range(B)]
    dense_s = np.full((B, max(len(l) for l in labs_s)), -1, dtype=np.int64)
    for b, l in enumerate(labs_s):
        dense_s[b, :len(l)] = l
    model = MultitaskCTC(encoder_type=enc, input_size=D, num_units=H, num_layers_main=Lm, num_layers_sub=Ls,
                         num_classes_main=Cm, num_classes_sub=Cs, main_task_weight=w, parameter_init=0.1,
                         clip_grad_norm=5.0, clip_activation=50, bottleneck_dim=bn, dtype='f32', seed=9, device='cpu',
                         **(dict(lstm_impl='LSTMCell', num_proj=proj) if proj else {}))
    ndir = 2 if enc == 'multitask_blstm' else 1
    sd = {k: v.numpy().copy() for k, v in model.store.state_dict().items()}
    for k in sd:
        if k.endswith('/biases'):
            sd[k] = (rng.randn(*sd[k].shape) * 0.05).astype(np.float32)
    model.store.load_state_dict({k: torch.tensor(v) for k, v in sd.items()})
    ref = omodel.multitask_ctc_model_forward(sd, x, labs_m, labs_s, sl, Lm, Ls if ndir == 2 else Lm, w, ndir=ndir,
                                             cell_clip=50.0, bottleneck=bn is not None, proj=bool(proj))
    if proj:
        assert 'blstm_hidden1/fw/lstm_cell/projection/kernel' in sd and model.encoder.output_dim == 2 * proj
    loss, lg_m, lg_s = model.compute_loss(x, dense_m, list2sparsetensor(dense_s, -1), sl, keep_prob=1.0)
    assert abs(loss.item() - ref['total_loss']) / abs(ref['total_loss']) < 1e-5
    assert np.abs(lg_m.numpy() - ref['logits_main']).max() < 1e-5
    assert np.abs(lg_s.numpy() - ref['logits_sub']).max() < 1e-5
    assert np.abs(model.ctc_losses_sub.numpy() - ref['ctc_losses_sub']).max() < 1e-4
    _check_grads(model._set_optimizer('sgd', 0.1), loss, model, ref)
    # dropout path runs, trains, decodes and scores both tasks
    first = last = None
    for it in range(6):
        l, lm_, ls_ = model.compute_loss(x, dense_m, dense_s, sl, keep_prob=0.9)
        model.train(l, 'adam', 1e-2)
        first = l.item() if first is None else first
        last = l.item()
    assert last < first
    dm, ds = model.decoder(lm_, ls_, sl, beam_width=1)
    ler_m, ler_s = model.compute_ler(dm, ds, list2sparsetensor(dense_m, -1), list2sparsetensor(dense_s, -1))
    assert 0.0 <= ler_m and 0.0 <= ler_s
    pm, ps = model.posteriors(lm_, ls_)
    assert pm.shape == (B * T, Cm + 1) and ps.shape == (B * T, Cs + 1)


def _att_batch(rng, B, T, D, C):
    x = rng.randn(B, T, D).astype(np.float32)
    sl = rng.randint(max(2, T // 2), T + 1, size=B).astype(np.int32)
    sl[0] = T
    lens = rng.randint(1, 5, size=B)
    lens[0] = 4
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


def _mk_att(cls, att, D, H, L, U, A, Em, C, **kw):
    return cls(input_size=D, encoder_type='blstm', encoder_num_units=H, encoder_num_layers=L,
               encoder_num_proj=None, attention_type=att, attention_dim=A, decoder_type='lstm',
               decoder_num_units=U, decoder_num_layers=1, embedding_dim=Em, num_classes=C, sos_index=C,
               eos_index=C + 1, max_decode_length=8, parameter_init=0.1, clip_grad_norm=5.0,
               clip_activation_encoder=50, clip_activation_decoder=50, dtype='f32', seed=5, device='cpu', **kw)


@pytest.mark.parametrize('att,sig,prev', [
    ('bahdanau_content', False, 'zeros'), ('location', False, 'zeros'), ('hybrid', False, 'zeros'),
    ('dot_product', False, 'zeros'), ('luong_dot', False, 'zeros'), ('luong_general', False, 'zeros'),
    ('luong_concat', False, 'zeros'), ('bahdanau_content', True, 'zeros'), ('luong_dot', True, 'zeros'),
    ('location', False, 'carry'), ('hybrid', False, 'carry'), ('hybrid', True, 'carry'),
    ('bahdanau_content', False, 'carry')])
def test_attention_model_host_logic(monkeypatch, att, sig, prev):
    """Decoder loop, bridge, per-type query / key wiring, deferred d_enc, sigmoid-smoothing plumbing
    (models/attention/attention_seq2seq.py) against the oracle's attention model.  prev='carry': the previous
    step's weights feed the location features (conv1d -> W_filter) and gradients flow back through them into
    `filter`, W_filter/weights and the earlier steps (a no-op for types without location features)."""
    _cpu_ops.install(monkeypatch)
    from oracle import attention as oatt
    from tensorflow_end2end_speech_recognition_amd.models.attention.attention_seq2seq import AttentionSeq2Seq
    rng = np.random.RandomState(11)
    B, T, D, H, L, A, Em, C = 3, 9, 6, 8, 1, 10, 4, 6
    U = 2 * H if att == 'luong_dot' else 12
    x, sl, labels, lsl, _ = _att_batch(rng, B, T, D, C)
    model = _mk_att(AttentionSeq2Seq, att, D, H, L, U, A, Em, C, sharpening_factor=1.5, logits_temperature=2.0,
                    sigmoid_smoothing=sig, prev_alpha=prev)
    sd = {k: v.numpy().copy() for k, v in model.store.state_dict().items()}
    ref = oatt.attention_model_forward(sd, x, labels, sl, lsl, L, att, clip_enc=50.0, clip_dec=50.0, sharpening=1.5,
                                       temperature=2.0, sigmoid_smoothing=sig, prev_alpha=prev)
    if prev == 'carry' and att in ('location', 'hybrid'):   # the location path is live: its variables get gradient
        A_ = 'attention_decoder/decoder/attention_layer/'
        assert np.abs(ref['grads'][A_ + 'filter']).max() > 0 and np.abs(ref['grads'][A_ + 'W_filter/weights']).max() > 0
    loss, logits, out_train, out_infer = model.compute_loss(x, labels, sl, lsl, 1.0, 1.0, 1.0)
    assert abs(loss.item() - ref['total_loss']) / abs(ref['total_loss']) < 1e-5
    assert np.abs(out_train.attention_weights.numpy() - ref['alphas']).max() < 1e-5
    assert np.array_equal(out_train.predicted_ids.numpy(), ref['predicted_ids'])
    opt = model._set_optimizer('adam', 1e-3)
    for g, name in opt.compute_gradients(loss, model=model):
        r = ref['grads'][name]
        err = np.abs(g.numpy() - r).max()
        assert err < 1e-4 * max(np.abs(r).max(), 1e-3) + 1e-7, (name, err, np.abs(r).max())
    ref_ids = oatt.attention_model_infer(sd, x, sl, L, att, C, C + 1, 8, clip_enc=50.0, clip_dec=50.0, sharpening=1.5,
                                         sigmoid_smoothing=sig, prev_alpha=prev)
    assert np.array_equal(out_infer.predicted_ids.numpy(), ref_ids)


@pytest.mark.parametrize('enc', ['vgg_blstm', 'vgg_lstm'])
def test_vgg_bf16_path_dropout_bookkeeping_fused_equals_separate(monkeypatch, enc):
    """The bf16 (implicit-GEMM) path of the VGG front-end on the CPU stand-ins: with tf.nn.dropout applied inside the
    producing kernels (conv / pool epilogues; the backward reads "active and kept" off the dropped tensors) and with every
    dropout as its own pass over the stored activation (front.fused_drop = False) the step is the same step -- loss,
    logits and every gradient -- for the same dropout counters; and the dropout is live (keep_prob 1.0 gives another loss).
    Host bookkeeping of models/encoders/core/vgg_blstm.py forward() / backward(); the kernels themselves are compared bit
    for bit on the GPU (tests/test_gpu_ops.py, test_gpu_model.py)."""
    _cpu_ops.install(monkeypatch)
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    rng = np.random.RandomState(3)
    B, T, F, W, H, C = 3, 8, 4, 3, 8, 5
    x = rng.randn(B, T, F * W * 3).astype(np.float32)
    sl = np.array([8, 6, 3], dtype=np.int32)
    for b in range(B):
        x[b, sl[b]:] = 0
    dense = np.array([[1, 2, -1], [3, -1, -1], [0, -1, -1]], dtype=np.int64)
    model = CTC(encoder_type=enc, input_size=3 * F, splice=W, num_units=H, num_layers=1, num_classes=C, parameter_init=0.1,
                clip_grad_norm=5.0, clip_activation=50, dtype='bf16', seed=1, device='cpu')
    opt = model._set_optimizer('sgd', 0.1)
    runs = {}
    for fused in (True, False):
        model.encoder.front.fused_drop = fused
        calls = model._dropout_calls
        loss, logits = model.compute_loss(x, dense, sl, keep_prob=0.8)
        assert model.encoder.front.ctx['fused_drop'] == fused
        opt.compute_gradients(loss, model=model)
        runs[fused] = (loss.item(), logits.clone(), model.store.grad.clone())
        model._dropout_calls = calls                          # replay the same masks
    assert runs[True][0] == runs[False][0] and torch.equal(runs[True][1], runs[False][1])
    g1, g0 = runs[True][2], runs[False][2]
    assert float(g0.abs().max()) > 0 and float((g1 - g0).abs().max()) <= 1e-6 * float(g0.abs().max())
    plain, _ = model.compute_loss(x, dense, sl, keep_prob=1.0)
    assert abs(plain.item() - runs[True][0]) > 1e-4


def test_bf16_model_multiplies_with_the_rounded_decoder_kernel_everywhere(monkeypatch):
    """A bf16-operand attention model streams its decoder cell's kernel as bf16 (asr_lstm_cell_gemm_*_h) -- one more
    rounding point, straight-through (AttentionSeq2Seq._w_cell, oracle.attention's operand_round set).  On the CPU
    stand-ins nothing else rounds, so the point can be isolated: loss, logits and EVERY gradient equal the oracle's for the
    same weights with ONLY that kernel rounded to bf16 (1e-6), and differ measurably from the oracle on the stored kernel."""
    _cpu_ops.install(monkeypatch)
    from oracle import attention as oatt
    from oracle import lstm as olstm
    from tensorflow_end2end_speech_recognition_amd.models.attention import attention_seq2seq as S
    from tensorflow_end2end_speech_recognition_amd.models.attention.attention_seq2seq import AttentionSeq2Seq
    # (ASR_ATT_BWD_BF16 off for this check: with the backward's batched products on bf16 operands -- the device default
    # for a bf16 model since round 5 -- the gradients differ from the oracle by bf16 rounding, 7e-3, like the encoder's; the
    # statement below isolates the FORWARD rounding point)
    monkeypatch.setattr(S, 'ATT_BWD_BF16', False)
    rng = np.random.RandomState(11)
    B, T, D, H, L, A, Em, C, U = 3, 9, 6, 8, 1, 10, 4, 6, 12
    x, sl, labels, lsl, _ = _att_batch(rng, B, T, D, C)
    model = AttentionSeq2Seq(input_size=D, encoder_type='blstm', encoder_num_units=H, encoder_num_layers=L,
                             encoder_num_proj=None, attention_type='location', attention_dim=A, decoder_type='lstm',
                             decoder_num_units=U, decoder_num_layers=1, embedding_dim=Em, num_classes=C, sos_index=C,
                             eos_index=C + 1, max_decode_length=8, parameter_init=0.5, clip_grad_norm=5.0,
                             clip_activation_encoder=50, clip_activation_decoder=50, dtype='bf16', seed=5, device='cpu',
                             sharpening_factor=1.5, logits_temperature=2.0)
    key = 'attention_decoder/decoder/lstm_cell/kernel'
    sd = {k: v.numpy().copy() for k, v in model.store.state_dict().items()}
    rounded = dict(sd)
    rounded[key] = olstm.bf16_round_t(torch.tensor(sd[key], dtype=torch.float64)).numpy()
    assert np.abs(rounded[key] - sd[key]).max() > 1e-4                    # the rounding is not a no-op on these weights
    assert torch.equal(model._w_cell(), torch.tensor(rounded[key], dtype=torch.float32))
    loss, logits, _, _ = model.compute_loss(x, labels, sl, lsl, 1.0, 1.0, 1.0)
    opt = model._set_optimizer('adam', 1e-3)
    grads = {name: g.numpy() for g, name in opt.compute_gradients(loss, model=model)}
    gap = {}
    for tag, weights in (('rounded', rounded), ('stored', sd)):
        ref = oatt.attention_model_forward(weights, x, labels, sl, lsl, L, 'location', clip_enc=50.0, clip_dec=50.0,
                                           sharpening=1.5, temperature=2.0)
        gap[tag] = (abs(loss.item() - ref['total_loss']) / abs(ref['total_loss']),
                    np.abs(logits.numpy() - ref['logits'] * 2.0).max(),
                    max(np.abs(grads[n] - ref['grads'][n]).max() / max(np.abs(ref['grads'][n]).max(), 1e-3) for n in grads))
    assert gap['rounded'][0] < 1e-6 and gap['rounded'][1] < 1e-6 and gap['rounded'][2] < 1e-5, gap
    assert gap['stored'][1] > 1e-4 and gap['stored'][2] > 1e-4, gap       # ... and the test can tell the two apart


@pytest.mark.parametrize('att', ['location', 'hybrid', 'bahdanau_content', 'luong_general'])
def test_bf16_attention_backward_rounding_points_are_the_oracles(monkeypatch, att):
    """a bf16-operand attention model rounds the operands of its backward pass's batched products to bf16
    (ASR_ATT_BWD_BF16, the device default).  oracle.attention models those points (bwd_round: d W_av and d av_in, alpha^T .
    dctx into d enc, both gradients of the key projection, d W_cell).  On the CPU stand-ins the only FORWARD rounding point
    of a bf16 model is the decoder cell's kernel (the test above), so the oracle gets that kernel rounded, no operand_round,
    and the backward points: with the flag ON the model agrees with it to 1e-5 of every gradient's maximum -- and does NOT
    agree with the oracle without the backward points (the test sees them)."""
    _cpu_ops.install(monkeypatch)
    from oracle import attention as oatt
    from oracle import lstm as olstm
    from tensorflow_end2end_speech_recognition_amd.models.attention import attention_seq2seq as S
    from tensorflow_end2end_speech_recognition_amd.models.attention.attention_seq2seq import AttentionSeq2Seq
    monkeypatch.setattr(S, 'ATT_BWD_BF16', True)
    rng = np.random.RandomState(13)
    B, T, D, H, L, A, Em, C, U = 3, 9, 6, 8, 1, 10, 4, 6, 12
    if att == 'luong_general':
        A = U
    x, sl, labels, lsl, _ = _att_batch(rng, B, T, D, C)
    prev = 'carry' if att in ('location', 'hybrid') else 'zeros'
    model = AttentionSeq2Seq(input_size=D, encoder_type='blstm', encoder_num_units=H, encoder_num_layers=L,
                             encoder_num_proj=None, attention_type=att, attention_dim=A, decoder_type='lstm',
                             decoder_num_units=U, decoder_num_layers=1, embedding_dim=Em, num_classes=C, sos_index=C,
                             eos_index=C + 1, max_decode_length=8, parameter_init=0.5, clip_grad_norm=5.0,
                             clip_activation_encoder=50, clip_activation_decoder=50, dtype='bf16', seed=5, device='cpu',
                             prev_alpha=prev)
    sd = {k: v.numpy().copy() for k, v in model.store.state_dict().items()}
    key = 'attention_decoder/decoder/lstm_cell/kernel'
    sd[key] = olstm.bf16_round_t(torch.tensor(sd[key], dtype=torch.float64)).numpy()
    loss, logits, *_ = model.compute_loss(x, labels, sl, lsl, 1.0, 1.0, 1.0)
    opt = model._set_optimizer('adam', 1e-3)
    grads = {name: g.numpy() for g, name in opt.compute_gradients(loss, model=model)}
    gap = {}
    for tag, br in (('with', olstm.bf16_round_t), ('without', None)):
        ref = oatt.attention_model_forward(sd, x, labels, sl, lsl, L, att, clip_enc=50.0, clip_dec=50.0, prev_alpha=prev,
                                           bwd_round=br)
        gap[tag] = (abs(loss.item() - ref['total_loss']) / abs(ref['total_loss']),
                    {n: np.abs(grads[n] - ref['grads'][n]).max() / max(np.abs(ref['grads'][n]).max(), 1e-3) for n in grads})
    worst = max(gap['with'][1].values())
    assert gap['with'][0] < 1e-6 and worst < 1e-5, (gap['with'][0], sorted(gap['with'][1].items(), key=lambda kv: -kv[1])[:4])
    assert max(gap['without'][1].values()) > 1e-3            # without the backward points the difference is bf16-sized


def test_joint_ctc_attention_host_logic(monkeypatch):
    _cpu_ops.install(monkeypatch)
    from oracle import attention as oatt
    from tensorflow_end2end_speech_recognition_amd.models.attention.joint_ctc_attention import JointCTCAttention
    from tensorflow_end2end_speech_recognition_amd.utils.io.labels.sparsetensor import list2sparsetensor
    rng = np.random.RandomState(3)
    B, T, D, H, L, U, A, Em, C = 4, 10, 6, 8, 2, 12, 10, 4, 5
    x, sl, labels, lsl, ctc_labels = _att_batch(rng, B, T, D, C)
    model = _mk_att(JointCTCAttention, 'bahdanau_content', D, H, L, U, A, Em, C, lambda_weight=0.5)
    sd = {k: v.numpy().copy() for k, v in model.store.state_dict().items()}
    ctc_list = [[int(v) for v in row if v >= 0] for row in ctc_labels]
    ref = oatt.attention_model_forward(sd, x, labels, sl, lsl, L, 'bahdanau_content', clip_enc=50.0, clip_dec=50.0,
                                       ctc_labels=ctc_list, lambda_weight=0.5)
    loss, logits, ctc_logits, otr, oinf = model.compute_loss(x, labels, list2sparsetensor(ctc_labels, -1), sl, lsl,
                                                             1.0, 1.0, 1.0)
    assert abs(loss.item() - ref['total_loss']) / abs(ref['total_loss']) < 1e-5
    assert np.abs(ctc_logits.numpy() - ref['ctc_logits']).max() < 1e-5
    opt = model._set_optimizer('adam', 1e-3)
    for g, name in opt.compute_gradients(loss, model=model):
        r = ref['grads'][name]
        err = np.abs(g.numpy() - r).max()
        assert err < 1e-4 * max(np.abs(r).max(), 1e-3) + 1e-7, (name, err)
    first = last = None
    for step in range(5):                                 # dropout paths + optimizer sequencing run
        loss, *_ = model.compute_loss(x, labels, ctc_labels, sl, lsl, 0.9, 0.9, 0.9)
        model.train(loss, 'adam', 5e-3)
        first = loss.item() if first is None else first
        last = loss.item()
    assert last < first


from _corpus import make_timit_like as _make_timit_like          # noqa: E402


def test_timit_recipe_end_to_end_on_cpu_stand_ins(monkeypatch, tmp_path):
    """examples/timit/training/train_ctc.py + evaluation/eval_ctc.py on a generated corpus in the reference's
    directory layout: dataset -> train -> print_step logging -> per-epoch PER on 39 phones -> checkpoint on a new
    best -> test-set PER -> LR controller -> run-directory bookkeeping; then the evaluation script restores the
    checkpoint and reproduces the test PER."""
    import os
    import sys
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    _cpu_ops.install(monkeypatch)
    from examples.timit.training import train_ctc
    from examples.timit.evaluation import eval_ctc
    corpus = str(tmp_path / 'corpus')
    _make_timit_like(corpus, np.random.RandomState(0))
    with open(os.path.join(root, 'examples/timit/config/ctc/blstm_ctc_phone61.yml')) as f:
        cfg = yaml.safe_load(f)
    cfg['param'].update(input_size=6, num_units=8, num_layers=1, batch_size=8, num_epoch=14, eval_start_epoch=1,
                        print_step=5, optimizer='adam', learning_rate=0.05, dropout=0.0, weight_decay=0,
                        decay_start_epoch=2, dtype='f32', device='cpu', dataset_root=corpus, sort_stop_epoch=2)
    cfg_path = str(tmp_path / 'cfg.yml')
    with open(cfg_path, 'w') as f:
        yaml.safe_dump(cfg, f)
    import random
    random.seed(0)                    # the iterators draw from the global generator, as the reference's do
    res = train_ctc.main(cfg_path, str(tmp_path / 'runs'))
    run = res['save_path']
    assert run.endswith(os.path.join('ctc', 'phone61', 'blstm_ctc_8_1_adam_lr0.05'))
    for name in ('config.yml', 'train.log', 'complete.txt', 'loss.csv', 'ler.csv', 'checkpoint',
                 os.path.join('mapping_files', 'phone2phone.txt')):
        assert os.path.isfile(os.path.join(run, name)), name
    assert len(res['ler_dev']) == 14 and res['checkpoints'] and res['ler_test'] is not None
    assert all(0.0 <= v for v in res['ler_dev']) and min(res['ler_dev']) < 0.5
    log = open(os.path.join(run, 'train.log')).read()
    assert 'Total 12 variables' in log and '-----EPOCH:14' in log and 'PER:' in log and 'Model saved in file' in log
    # a second run never reuses the directory
    cfg['param']['num_epoch'] = 1
    with open(cfg_path, 'w') as f:
        yaml.safe_dump(cfg, f)
    res2 = train_ctc.main(cfg_path, str(tmp_path / 'runs'))
    assert res2['save_path'] == run + '_1'
    # evaluation script: latest checkpoint of the first run == its last best epoch
    per = eval_ctc.main([run, '--beam_width', '1', '--device', 'cpu'])
    assert abs(per - res['ler_test']) < 1e-9
    # visualization script: Ref / Hyp pairs of the test set
    from examples.timit.visualization import decode_ctc
    pairs = decode_ctc.main([run, '--beam_width', '1', '--device', 'cpu'])
    assert len(pairs) == 4 and all(isinstance(r, str) and isinstance(h, str) for _, r, h in pairs)


def _recipe_cfg(root, rel, tmp_path, **upd):
    import yaml
    with open(os.path.join(root, rel)) as f:
        cfg = yaml.safe_load(f)
    cfg['param'].update(upd)
    path = str(tmp_path / ('cfg_%s' % os.path.basename(rel)))
    with open(path, 'w') as f:
        yaml.safe_dump(cfg, f)
    return path


@pytest.mark.parametrize('family', ['attention', 'joint', 'multitask'])
def test_timit_attention_joint_multitask_recipes_on_cpu_stand_ins(monkeypatch, tmp_path, family):
    """examples/timit/training/train_{attention,joint_ctc_attention,multitask_ctc}.py on a generated corpus: the
    family-specific dataset, loss call, inference-decoder monitoring and PER / CER evaluation, through the shared
    loop (checkpoint on a new best, test evaluation, run-directory files)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    _cpu_ops.install(monkeypatch)
    corpus = str(tmp_path / 'corpus')
    _make_timit_like(corpus, np.random.RandomState(0), n_train=16, n_dev=4, n_test=3, multitask=family == 'multitask')
    common = dict(input_size=6, batch_size=8, num_epoch=3, eval_start_epoch=1, print_step=2, optimizer='adam',
                  learning_rate=0.02, weight_decay=0, decay_start_epoch=2, dtype='f32', device='cpu',
                  dataset_root=corpus, sort_stop_epoch=2)
    if family == 'multitask':
        from examples.timit.training import train_multitask_ctc as drv
        cfg = _recipe_cfg(root, 'examples/timit/config/ctc/multitask_blstm_ctc_char_phone61.yml', tmp_path,
                          num_units=8, num_layers_main=2, num_layers_sub=1, dropout=0.0, **common)
    else:
        from examples.timit.training import train_attention, train_joint_ctc_attention
        drv = train_attention if family == 'attention' else train_joint_ctc_attention
        cfg = _recipe_cfg(root, 'examples/timit/config/attention/blstm_attention_phone61.yml', tmp_path,
                          encoder_num_units=8, encoder_num_layers=1, attention_dim=6, decoder_num_units=8,
                          embedding_dim=4, max_decode_length=10, dropout_encoder=0.0, dropout_decoder=0.1,
                          dropout_embedding=0.1, **common)
    res = drv.main(cfg, str(tmp_path / 'runs'))
    run = res['save_path']
    assert res['steps'] == 6 and len(res['ler_dev']) == 3 and all(v >= 0 for v in res['ler_dev'])
    for name in ('config.yml', 'train.log', 'complete.txt', 'loss_ler.csv', os.path.join('mapping_files', 'phone61.txt')):
        assert os.path.isfile(os.path.join(run, name)), name
    log = open(os.path.join(run, 'train.log')).read()
    assert '-----EPOCH:3' in log and 'Step 6' in log and ('PER' in log or 'CER' in log)
    if res['checkpoints']:
        assert res['ler_test'] is not None and os.path.isfile(os.path.join(run, 'checkpoint'))
    if family == 'multitask':
        from examples.timit.evaluation import eval_multitask_ctc
        from tensorflow_end2end_speech_recognition_amd.utils.training.checkpoint import Saver
        Saver().save(res['model'], os.path.join(run, 'model.ckpt'), global_step=99)
        cer, wer, per = eval_multitask_ctc.main([run, '--beam_width', '1', '--device', 'cpu'])
        assert cer >= 0 and wer >= 0 and per >= 0
    if family != 'multitask':
        # the evaluation script: rebuild the model from the run's config.yml, restore a checkpoint of the trained
        # parameters, score the test set -- must equal scoring the trained model object directly
        from examples.timit.evaluation import eval_attention
        from examples.timit.metrics.attention import do_eval_per
        from examples.timit.training.train_attention import make_datasets
        from tensorflow_end2end_speech_recognition_amd.utils.training.checkpoint import Saver
        model = res['model']
        Saver().save(model, os.path.join(run, 'model.ckpt'), global_step=99)
        map_dir = os.path.join(run, 'mapping_files')
        params = dict(label_type='phone61', splice=1, num_stack=1, num_skip=1, batch_size=8, num_epoch=1,
                      sort_stop_epoch=1, dataset_root=corpus)
        test_data = make_datasets(drv.Dataset, params, map_dir)[2]
        want = do_eval_per(None, None, None, model, test_data, 'phone61', is_test=True, eval_batch_size=1,
                           map_dir=map_dir, is_jointctcatt=family == 'joint')
        got = eval_attention.main([run, '--device', 'cpu'] + (['--joint'] if family == 'joint' else []))
        assert abs(got - want) < 1e-9


@pytest.mark.parametrize('encoder_type', ['blstm', 'lstm', 'multitask_blstm', 'multitask_lstm'])
def test_encoder_shape_table(monkeypatch, encoder_type):
    """The reference's own encoder test (models/test/test_encoder.py:258-314): for every lstm_impl and both
    time_major settings, outputs are (B, T, ndir*H) -- (T, B, ndir*H) when time_major -- and the final state is
    (LSTMStateTuple fw, LSTMStateTuple bw) of the last layer, or one LSTMStateTuple per layer for the
    unidirectional stack, each (B, H); the multitask encoders add the sub-task outputs / state."""
    _cpu_ops.install(monkeypatch)
    from tensorflow_end2end_speech_recognition_amd.models.encoders.load_encoder import load
    from tensorflow_end2end_speech_recognition_amd.models.encoders.core.blstm import LSTM_IMPLS
    rng = np.random.RandomState(0)
    B, T, D, H, L = 3, 7, 6, 8, 3
    x = torch.tensor(rng.randn(B, T, D).astype(np.float32))
    sl = torch.tensor([7, 5, 2], dtype=torch.int32)
    bidir = 'blstm' in encoder_type
    multi = encoder_type.startswith('multitask')
    for lstm_impl in LSTM_IMPLS:
        for time_major in (True, False):
            kw = dict(num_units=H, num_proj=None, lstm_impl=lstm_impl, use_peephole=True, parameter_init=0.1,
                      clip_activation=50, time_major=time_major)
            if multi:
                kw.update(num_layers_main=L, num_layers_sub=2)
            else:
                kw.update(num_layers=L)
            enc = load(encoder_type)(**kw)
            res = enc(x, sl, 0.9, True)
            outs, final = res[0], res[1]
            want = (T, B, H * (2 if bidir else 1)) if time_major else (B, T, H * (2 if bidir else 1))
            assert tuple(outs.shape) == want
            assert len(final) == (2 if bidir else L)
            for st in final:
                assert tuple(st.c.shape) == (B, H) and tuple(st.h.shape) == (B, H)
            if multi:
                outs_sub, final_sub = res[2], res[3]
                assert tuple(outs_sub.shape) == want
                assert len(final_sub) == (2 if bidir else L)          # lstm.py:271-272: the sub stack is the full stack
                for st in final_sub:
                    assert tuple(st.c.shape) == (B, H) and tuple(st.h.shape) == (B, H)
            # frames past an utterance's length are zero
            o = outs if not time_major else outs.transpose(0, 1)
            assert float(o[2, 2:].abs().max()) == 0.0 and float(o[1, 5:].abs().max()) == 0.0


@pytest.mark.parametrize('encoder_type', ['gru', 'bgru', 'cldnn_wang'])
def test_encoder_shape_table_gru_and_cldnn(monkeypatch, encoder_type):
    """models/test/test_encoder.py:130-314 for the remaining registry keys: GRU / BGRU outputs (B, T, ndir*H) with one
    state per layer (MultiRNNCell) / (fw, bw) of the last layer, each (B, H); CLDNN outputs (B, T, 74)."""
    _cpu_ops.install(monkeypatch)
    from tensorflow_end2end_speech_recognition_amd.models.encoders.load_encoder import load
    rng = np.random.RandomState(0)
    B, T, H, L = 3, 7, 16, 2
    sl = torch.tensor([7, 5, 2], dtype=torch.int32)
    for time_major in (True, False):
        if encoder_type == 'cldnn_wang':
            F, W = 7, 5
            x = torch.tensor(rng.randn(B, T, F * W * 3).astype(np.float32))
            enc = load(encoder_type)(input_size=3 * F, splice=W, num_stack=1, num_units=H, num_proj=None, num_layers=L,
                                     lstm_impl='LSTMBlockCell', use_peephole=True, parameter_init=0.1,
                                     clip_activation=50, time_major=time_major)
            width = 74
        else:
            x = torch.tensor(rng.randn(B, T, 6).astype(np.float32))
            enc = load(encoder_type)(num_units=H, num_layers=L, parameter_init=0.1, time_major=time_major)
            width = H * (2 if encoder_type == 'bgru' else 1)
        outs, final = enc(x, sl, 0.9, True)
        assert tuple(outs.shape) == ((T, B, width) if time_major else (B, T, width))
        if encoder_type == 'gru':
            assert len(final) == L and all(tuple(f.shape) == (B, H) for f in final)
        elif encoder_type == 'bgru':
            assert len(final) == 2 and all(tuple(f.shape) == (B, H) for f in final)
        else:
            assert len(final) == 2 and all(tuple(f.c.shape) == (B, H) for f in final)
        if encoder_type != 'cldnn_wang':          # the DNN on top of the CLDNN stack maps a zero frame to relu(bias)
            o = outs if not time_major else outs.transpose(0, 1)
            assert float(o[2, 2:].abs().max()) == 0.0 and float(o[1, 5:].abs().max()) == 0.0
    with pytest.raises(ValueError):
        load('pyramid_blstm')


def test_overfit_one_utterance_like_the_reference_model_tests(monkeypatch):
    """models/test/test_ctc.py:170-233 and test_attention.py:107-226: one utterance repeated B times, train until
    the label error rate of the decode drops below 0.1 (the reference's only pass criterion; it allows 1000 steps).
    CTC (greedy decode) and attention (inference decoder) on the CPU stand-ins."""
    _cpu_ops.install(monkeypatch)
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    from tensorflow_end2end_speech_recognition_amd.models.attention.attention_seq2seq import AttentionSeq2Seq
    from tensorflow_end2end_speech_recognition_amd.utils.io.labels.sparsetensor import list2sparsetensor
    rng = np.random.RandomState(0)
    B, T, D, C = 2, 24, 6, 8
    x = np.repeat(rng.randn(1, T, D).astype(np.float32), B, 0)
    sl = np.array([T] * B, np.int32)
    lab = rng.randint(0, C, size=6)
    st = list2sparsetensor(np.repeat(lab[None], B, 0), -1)
    model = CTC('blstm', D, 16, 1, C, parameter_init=0.1, clip_grad_norm=5.0, clip_activation=50, dtype='f32',
                device='cpu', seed=1)
    ler = 1.0
    for step in range(1000):
        loss, logits = model.compute_loss(x, st, sl, 1.0)
        model.train(loss, 'adam', 1e-2)
        if (step + 1) % 10 == 0:
            ler = model.compute_ler(model.decoder(logits, sl, 1), st)
            if ler < 0.1:
                break
    assert ler < 0.1, (step, ler)

    labels = np.concatenate([[C], lab, [C + 1]])[None].repeat(B, 0)
    lsl = np.array([len(lab) + 2] * B)
    att = AttentionSeq2Seq(input_size=D, encoder_type='blstm', encoder_num_units=16, encoder_num_layers=1,
                           encoder_num_proj=None, attention_type='bahdanau_content', attention_dim=8,
                           decoder_type='lstm', decoder_num_units=16, decoder_num_layers=1, embedding_dim=6,
                           num_classes=C, sos_index=C, eos_index=C + 1, max_decode_length=12, parameter_init=0.1,
                           clip_grad_norm=5.0, clip_activation_encoder=50, clip_activation_decoder=50, dtype='f32',
                           device='cpu', seed=1)
    ler = 1.0
    for step in range(1000):
        loss, _, out_train, out_infer = att.compute_loss(x, labels, sl, lsl, 1.0, 1.0, 1.0)
        att.train(loss, 'adam', 1e-2)
        if (step + 1) % 10 == 0:
            ids = np.asarray(out_infer.predicted_ids)
            pred = [[int(v) for v in row[:list(row).index(C + 1)]] if (C + 1) in row else [int(v) for v in row]
                    for row in ids]
            ler = att.compute_ler([list(lab)] * B, pred)
            if ler < 0.1:
                break
    assert ler < 0.1, (step, ler)


@pytest.mark.parametrize('enc', ['vgg_blstm', 'vgg_lstm'])
def test_vgg_front_end_host_logic(monkeypatch, enc):
    """VGG front-end + recurrent stack + CTC (models/encoders/core/vgg_blstm.py): valid-frame packing of the padded
    batch, the im2col form of the four convolutions, pooling with odd edges, the bridge, and every gradient, against
    the oracle's VGG model (oracle/vgg.py)."""
    _cpu_ops.install(monkeypatch)
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    rng = np.random.RandomState(2)
    B, T, F, W, H, C = 3, 7, 5, 3, 8, 5               # 5 x 3 images: both pooling stages see an odd edge
    D = F * W * 3
    x, sl, labs, dense = _batch(rng, B, T, D, C, div=3)
    model = CTC(encoder_type=enc, input_size=3 * F, splice=W, num_units=H, num_layers=1, num_classes=C,
                parameter_init=0.1, clip_grad_norm=5.0, clip_activation=50, dtype='f32', seed=4, device='cpu')
    sd = {k: v.numpy().copy() for k, v in model.store.state_dict().items()}
    for k in sd:
        if k.endswith('/bias') or k.endswith('/biases'):
            sd[k] = (rng.randn(*sd[k].shape) * 0.05).astype(np.float32)
    model.store.load_state_dict({k: torch.tensor(v) for k, v in sd.items()})
    ref = omodel.ctc_model_forward(sd, x, labs, sl, 1, ndir=2 if enc == 'vgg_blstm' else 1, cell_clip=50.0, vgg=(F, W))
    loss, logits = model.compute_loss(x, dense, sl, keep_prob=1.0)
    assert abs(loss.item() - ref['total_loss']) / abs(ref['total_loss']) < 1e-5
    valid = np.arange(T)[:, None] < sl[None, :]
    assert np.abs((logits.numpy() - ref['logits'])[valid]).max() < 1e-4
    _check_grads(model._set_optimizer('sgd', 0.1), loss, model, ref, tol=2e-4)
    # dropout path runs and trains
    first = last = None
    for it in range(4):
        l, _ = model.compute_loss(x, dense, sl, keep_prob=0.8)
        model.train(l, 'adam', 5e-3)
        first = l.item() if first is None else first
        last = l.item()
    assert np.isfinite(last)


@pytest.mark.parametrize('B,T,D,C,L,enc,bn,wd,temp', [
    (1, 1, 3, 4, 1, 'blstm', None, 0.0, 1),          # one utterance, one frame (no h_prev term in dW_h)
    (1, 5, 3, 4, 2, 'lstm', None, 1e-3, 1),
    (17, 4, 6, 5, 1, 'blstm', 7, 0.0, 2),            # batch padded 17 -> 32, bottleneck, softmax temperature
    (16, 3, 3, 2, 3, 'lstm', None, 0.0, 1),
    (33, 2, 3, 6, 1, 'blstm', None, 1e-2, 3),
])
def test_ctc_host_logic_edge_shapes(monkeypatch, B, T, D, C, L, enc, bn, wd, temp):
    _cpu_ops.install(monkeypatch)
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    rng = np.random.RandomState(B * 7 + T)
    x = rng.randn(B, T, D).astype(np.float32)
    sl = rng.randint(1, T + 1, size=B).astype(np.int32)
    sl[0] = T
    labs = []
    for b in range(B):
        x[b, sl[b]:] = 0
        labs.append([int(v) for v in rng.randint(0, C, size=max(1, sl[b] // 3))])
    dense = np.full((B, max(len(l) for l in labs)), -1, dtype=np.int64)
    for b, l in enumerate(labs):
        dense[b, :len(l)] = l
    model = CTC(enc, D, 8, L, C, parameter_init=0.2, clip_grad_norm=5.0, clip_activation=50, bottleneck_dim=bn,
                weight_decay=wd, dtype='f32', device='cpu', seed=B)
    sd = {k: v.numpy().copy() for k, v in model.store.state_dict().items()}
    ref = omodel.ctc_model_forward(sd, x, labs, sl, L, ndir=2 if enc == 'blstm' else 1, cell_clip=50.0,
                                   weight_decay=wd, bottleneck=bn is not None, temperature=float(temp))
    loss, logits = model.compute_loss(x, dense, sl, 1.0, softmax_temperature=temp)
    assert logits.shape == (T, B, C + 1)
    assert abs(loss.item() - ref['total_loss']) / max(abs(ref['total_loss']), 1e-6) < 1e-5
    _check_grads(model._set_optimizer('sgd', 0.1), loss, model, ref)


@pytest.mark.parametrize('B,T,D,C,L,att,sig,lam', [
    (1, 1, 3, 4, 1, 'bahdanau_content', False, None),     # one frame to attend over
    (1, 6, 3, 4, 1, 'location', True, None),
    (17, 3, 6, 5, 2, 'hybrid', False, None),              # batch padded 17 -> 32
    (3, 5, 6, 4, 1, 'dot_product', True, 0.3),            # joint, sigmoid smoothing
    (2, 7, 3, 4, 2, 'luong_concat', False, 0.9),
])
def test_attention_host_logic_edge_shapes(monkeypatch, B, T, D, C, L, att, sig, lam):
    _cpu_ops.install(monkeypatch)
    from oracle import attention as oatt
    from tensorflow_end2end_speech_recognition_amd.models.attention.attention_seq2seq import AttentionSeq2Seq
    from tensorflow_end2end_speech_recognition_amd.models.attention.joint_ctc_attention import JointCTCAttention
    from tensorflow_end2end_speech_recognition_amd.utils.io.labels.sparsetensor import list2sparsetensor
    rng = np.random.RandomState(B * 11 + T)
    x = rng.randn(B, T, D).astype(np.float32)
    sl = rng.randint(1, T + 1, size=B).astype(np.int32)
    sl[0] = T
    lens = np.array([max(1, min(3, int(n) // 2)) for n in sl])          # CTC head: 2L <= T keeps every row feasible
    labels = np.full((B, int(lens.max()) + 2), C + 1, dtype=np.int64)
    ctc = np.full((B, int(lens.max())), -1, dtype=np.int64)
    for b in range(B):
        x[b, sl[b]:] = 0
        y = rng.randint(0, C, size=lens[b])
        if sl[b] < 2 * lens[b] + 1 and lens[b] > 1:
            y[1:] = (y[:-1] + 1) % C                                     # no repeats where frames are scarce
        labels[b, 0] = C
        labels[b, 1:1 + lens[b]] = y
        ctc[b, :lens[b]] = y
    kw = dict(input_size=D, encoder_type='blstm', encoder_num_units=8, encoder_num_layers=L, encoder_num_proj=None,
              attention_type=att, attention_dim=5, decoder_type='lstm', decoder_num_units=6, decoder_num_layers=1,
              embedding_dim=3, num_classes=C, sos_index=C, eos_index=C + 1, max_decode_length=6, parameter_init=0.2,
              clip_grad_norm=5.0, clip_activation_encoder=50, clip_activation_decoder=50, dtype='f32', device='cpu',
              seed=B, sharpening_factor=1.3, sigmoid_smoothing=sig)
    if lam is None:
        model, sharp = AttentionSeq2Seq(**kw), 1.3
    elif B % 2:
        # the reference's JointCTCAttention hands sharpening_factor=1.0 (and four more literals) to its base class
        # whatever the caller passed (joint_ctc_attention.py:133-137, quirk Q15): reproduced, with a warning
        with pytest.warns(UserWarning, match='sharpening_factor=1.3'):
            model = JointCTCAttention(lambda_weight=lam, **kw)
        sharp = 1.0
    else:
        model, sharp = JointCTCAttention(lambda_weight=lam, honour_ctor_args=True, **kw), 1.3
    assert model.sharpening_factor == sharp
    sd = {k: v.numpy().copy() for k, v in model.store.state_dict().items()}
    ctc_list = [[int(v) for v in row if v >= 0] for row in ctc] if lam is not None else None
    ref = oatt.attention_model_forward(sd, x, labels, sl, lens + 2, L, att, clip_enc=50.0, clip_dec=50.0,
                                       sharpening=sharp, sigmoid_smoothing=sig, ctc_labels=ctc_list, lambda_weight=lam)
    if lam is None:
        loss = model.compute_loss(x, labels, sl, lens + 2, 1.0, 1.0, 1.0)[0]
    else:
        loss = model.compute_loss(x, labels, list2sparsetensor(ctc, -1), sl, lens + 2, 1.0, 1.0, 1.0)[0]
    assert abs(loss.item() - ref['total_loss']) / max(abs(ref['total_loss']), 1e-6) < 1e-5
    for g, name in model._set_optimizer('sgd', 0.1).compute_gradients(loss, model=model):
        r = ref['grads'][name]
        assert np.abs(g.numpy() - r).max() < 3e-4 * max(np.abs(r).max(), 1e-3) + 1e-7, name
    ref_ids = oatt.attention_model_infer(sd, x, sl, L, att, C, C + 1, 6, clip_enc=50.0, clip_dec=50.0, sharpening=sharp,
                                         sigmoid_smoothing=sig)
    assert np.array_equal(np.asarray(model.infer(x, sl)), ref_ids)


@pytest.mark.parametrize('enc', ['blstm', 'vgg_blstm'])
def test_dropout_descriptors_give_the_gradient_of_the_loss_they_produce(monkeypatch, enc):
    """Dropout ON, masks described by (keep_prob, seed, offset) instead of stored: the analytic gradient must be the
    derivative of the very loss the forward pass computed, i.e. forward and backward have to form the SAME masks at
    every site -- the recurrent layers' outputs (asr_dropout_apply forward, the dx GEMM's epilogue backward), the VGG
    activations (asr_dropout_apply / asr_relu_bwd_drop, the first layer's backward chunk by chunk with shifted
    counters: the chunk size is forced below the batch's frame count) and the pooled tensors.  Central differences on
    the largest-gradient entry of every variable, dropout stream re-wound for every evaluation."""
    _cpu_ops.install(monkeypatch)
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    from tensorflow_end2end_speech_recognition_amd.models.encoders.core import vgg_blstm as vb
    monkeypatch.setattr(vb, 'CHUNK_FRAMES', 4)
    rng = np.random.RandomState(11)
    if enc == 'vgg_blstm':
        B, T, F, W, H, C, L = 3, 6, 4, 3, 6, 5, 1
        x, sl, labs, dense = _batch(rng, B, T, F * W * 3, C, div=3)
        kw = dict(encoder_type=enc, input_size=3 * F, splice=W, num_units=H, num_layers=L)
    else:
        B, T, D, H, C, L = 4, 9, 6, 6, 5, 3
        x, sl, labs, dense = _batch(rng, B, T, D, C, div=3)
        kw = dict(encoder_type=enc, input_size=D, num_units=H, num_layers=L)
    model = CTC(num_classes=C, parameter_init=0.3, clip_grad_norm=1e9, clip_activation=50, dtype='f32', seed=2,
                device='cpu', **kw)

    def loss_now():
        model._dropout_calls = 0                      # the same dropout stream for every evaluation
        if hasattr(model.encoder, '_dropout_calls'):
            model.encoder._dropout_calls = 0
        loss, _ = model.compute_loss(x, dense, sl, keep_prob=0.7)
        return loss

    loss = loss_now()
    grads = {name: g.numpy().copy() for g, name in model._set_optimizer('sgd', 0.1).compute_gradients(loss, model=model)}
    assert any(np.abs(g).max() > 0 for g in grads.values())
    if enc == 'vgg_blstm':      # the chunked first-layer backward must not depend on where the chunks are cut
        monkeypatch.setattr(vb, 'CHUNK_FRAMES', 4096)
        whole = {name: g.numpy().copy() for g, name in
                 model._set_optimizer('sgd', 0.1).compute_gradients(loss_now(), model=model)}
        monkeypatch.setattr(vb, 'CHUNK_FRAMES', 4)
        for name in grads:
            assert np.abs(grads[name] - whole[name]).max() <= 1e-5 * max(1.0, np.abs(whole[name]).max()), name
    # eps: with weights of +-0.3 the loss is strongly curved (an LSTM kernel entry with gradient -18.86: central
    # differences -1.48 / -12.64 / -18.00 / -18.76 at eps 1e-2 / 1e-3 / 3e-4 / 1e-4); the fp32 storage of the stand-ins
    # puts ~2.5e-3 of noise on a difference quotient at 1e-4, below the 8e-3 the assertion allows at least
    eps, checked = 1e-4, 0
    for name, g in grads.items():
        if np.abs(g).max() < 5e-2:
            continue
        idx = np.unravel_index(np.abs(g).argmax(), g.shape)
        p = model.store[name]
        old = float(p[idx])
        p[idx] = old + eps
        lp = float(loss_now().item())
        p[idx] = old - eps
        lm = float(loss_now().item())
        p[idx] = old
        fd = (lp - lm) / (2 * eps)
        assert abs(fd - g[idx]) < 8e-2 * max(abs(g[idx]), 0.1), (name, idx, fd, g[idx])
        checked += 1
    assert checked >= 4


@pytest.mark.parametrize('which', ['cfgC', 'cfgD_location_carry', 'cfgD_location_zeros', 'cfgE_hybrid', 'cfgD_two_tiles_carry'])
def test_config_parity_runs_on_cpu_stand_ins(monkeypatch, which):
    """tests/_config_parity.py -- the model-level parity runs the `-m gpu` suite does at the widths of BASELINE
    configs[2..4] (tests/test_gpu_configs.py) -- at toy widths on the torch stand-ins: the same batch makers, model
    construction, oracle calls (with and without the bf16 rounding points) and error reports, so the host wiring
    they exercise (ragged two-tile VGG batch, joint location / hybrid attention with a wide CTC head) is pinned here."""
    import _config_parity as cp
    _cpu_ops.install(monkeypatch)
    if which == 'cfgC':
        r = cp.run_cfgC('cpu', 'f32', B=18, T=7, F=5, W=3, H=8, L=2, C=6, halves=True)
        assert r['loss_rel'] < 1e-5 and r['per_utt_rel'] < 1e-5 and r['logits_abs'] < 1e-4, r['report']
    else:
        att = 'hybrid' if which == 'cfgE_hybrid' else 'location'
        prev = 'zeros' if which.endswith('zeros') else 'carry'
        C = 37 if which == 'cfgE_hybrid' else 6
        # (two tiles: the encoder's two half-batch pipelines under the joint model -- final states into the bridge, the
        # decoder's and the CTC head's gradients back into both parts)
        r = cp.run_attention('cpu', 'f32', att, B=19 if 'two_tiles' in which else 3, T=12, To=5, D=6, H=8, L=2, U=12, A=10,
                             Em=4, C=C, lam=0.5, prev_alpha=prev, halves='two_tiles' in which)
        assert r['loss_rel'] < 1e-5 and r['alpha_abs'] < 1e-5 and r['ids_mismatch'] == 0, r['report']
        assert r['ctc_logits_abs'] < 1e-4 and r['ctc_losses_rel'] < 1e-5, r['report']
    assert r['grad_worst'] < 2e-4, r['report']


@pytest.mark.parametrize('att,prev,sig', [('bahdanau_content', 'zeros', False), ('location', 'zeros', False),
                                          ('location', 'carry', False), ('hybrid', 'carry', True), ('dot_product', 'zeros', False),
                                          ('luong_dot', 'zeros', False), ('luong_general', 'zeros', True),
                                          ('luong_concat', 'zeros', False)])
def test_attention_class_surface_on_cpu_stand_ins(monkeypatch, att, prev, sig):
    """models/attention/decoders/{attention_layer,attention_decoder,dynamic_decoder}.py and bridge.py: AttentionDecoder
    stepped by dynamic_decode under a TrainingHelper reproduces the oracle's teacher-forced logits / weights / ids and
    the model's own fused loop; a standalone AttentionLayer reproduces oracle.attention.attention_step."""
    import _config_parity as cp
    _cpu_ops.install(monkeypatch)
    r = cp.run_class_surface('cpu', att, prev, sig)
    assert r['loss_rel'] < 1e-5, r['report']
    assert r['class_logits_vs_oracle'] < 1e-4 and r['class_alpha_vs_oracle'] < 1e-5 and r['class_ids_vs_oracle'] == 0, r['report']
    assert r['class_logits_vs_fused'] < 1e-4 and r['class_alpha_vs_fused'] < 1e-5, r['report']
    assert r['layer_alpha'] < 1e-5 and r['layer_ctx'] < 1e-4, r['report']


def test_bridge_classes_on_cpu_stand_ins(monkeypatch):
    import _config_parity as cp
    _cpu_ops.install(monkeypatch)
    r = cp.run_bridges('cpu')
    assert r['fc_err'] < 1e-5 and r['ok_zero'] and r['ok_pass'] and r['raised'], r


@pytest.mark.parametrize('ndir,fused', [(2, '1'), (1, '1'), (2, '0'), (1, '0')])
def test_lstmcell_projection_host_logic(monkeypatch, ndir, fused):
    """lstm_impl='LSTMCell' with num_proj (models/encoders/core/blstm.py:187-230, lstm.py): the projected cells of
    rnn_util.LSTMPLayer (recurrent input and output = m W_proj) against the oracle's LSTMP model -- loss, logits, every
    gradient incl. projection/kernel -- with TF's variable names; so does the VGG front-end over projected cells.
    fused: the layer's two forms (the whole-sequence recurrence on W_p W_h with its batched products and the padded
    16-utterance tile; the step-by-step loop), the host logic of both."""
    import _config_parity as cp
    _cpu_ops.install(monkeypatch)
    monkeypatch.setenv('ASR_LSTMP_FUSED', fused)
    r = cp.run_lstmp('cpu', B=5, T=9, D=6, H=8, P=5, L=2, C=6, ndir=ndir)
    assert r['trained']
    if ndir == 2:
        assert r['loss_rel'] < 1e-5 and r['logits_abs'] < 1e-4 and r['grad_worst'] < 2e-4, r['report']
        # an ACTIVE cell clip: tf.contrib.rnn.LSTMCell clamps with tf.clip_by_value, so a clamped state passes no gradient
        # to its gates or to c_prev (the fused LSTMBlockCell of the other paths is straight-through) -- ADVICE r03
        rc = cp.run_lstmp('cpu', B=5, T=9, D=6, H=8, P=5, L=2, C=6, ndir=2, clip=0.15)
        assert rc['loss_rel'] < 1e-5 and rc['grad_worst'] < 2e-4, rc['report']
        assert 'blstm_hidden2/bw/lstm_cell/projection/kernel' in r['names']
    else:
        assert 'multi_lstm/multi_rnn_cell/cell_1/lstm_cell/projection/kernel' in r['names']
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    if ndir == 2:   # the VGG front-end in front of the projected cells (vgg_blstm.py:107-190 passes num_proj on)
        rv = cp.run_vgg_lstmp('cpu', B=3, T=7, F=4, W=3, H=8, P=5, L=1, C=6)
        assert rv['loss_rel'] < 1e-5 and rv['grad_worst'] < 2e-4 and rv['finite'], rv['report']
    # without lstm_impl='LSTMCell' num_proj is dropped, as in the reference (blstm.py:49-52)
    m = CTC(encoder_type='blstm', input_size=6, num_units=8, num_layers=1, num_classes=5, num_proj=4, device='cpu')
    assert m.encoder.num_proj is None and m.encoder.output_dim == 16


def _load_bench_module():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('bench_for_test', os.path.join(root, 'bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, root


def test_bench_compact_line_fits_the_drivers_window():
    """bench.py's last stdout line is built by compact_line(): from a canned FULL result (round 3's 20.7 KB object, which
    the driver's 8 000-byte stdout window cut the head off) it must stay under 6 000 bytes, keep every contract key and
    the roofline / cpu_baseline objects, and hold no prose notes; an 8-rank line (per_rank + comm) obeys the same limit,
    and an over-long object sheds auxiliary entries rather than overflow."""
    import json
    bench, root = _load_bench_module()
    full = json.load(open(os.path.join(root, 'profiles', 'r03_bench_steps20_warmup5.json')))
    assert len(json.dumps(full)) > 15000
    line = bench.compact_line(dict(full, full='bench_full.json'))
    assert len(line) < 6000 and '\n' not in line
    d = json.loads(line)
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
              'vs_baseline', 'dtype', 'data', 'config', 'step_ms', 'parity', 'kernels', 'roofline', 'cpu_baseline'):
        assert k in d, k
    assert abs(d['value'] - full['value']) < 1e-4 * full['value'] and d['config']['workload'] == full['config']['workload']
    rf = d['roofline']
    assert set(('bound', 'achieved', 'peak', 'unit', 'frac', 'traffic')) <= set(rf) and 'note' not in rf
    assert rf['traffic_file'] == 'profiles/r03_pmc_hbm.md' and abs(rf['frac'] - full['roofline']['frac']) < 1e-6
    cb = d['cpu_baseline']
    assert set(('value', 'unit', 'cores', 'kind', 'sample')) <= set(cb) and len(cb['sample']) <= 160
    for k in ('cfgA', 'cfgC', 'cfgD', 'cfgE'):
        e = d[k]
        assert abs(e['value'] - full[k]['value']) < 1e-4 * e['value'] and e['roofline']['frac'] > 0
        assert e['cpu_baseline']['value'] > 0 and e['cpu_baseline']['cores'] >= 1 and 'workload' not in e
    assert d['decode']['kanji3387_beam100']['beam']['ms_per_call'] > 0 and d['full'] == 'bench_full.json'

    def strings(o):
        if isinstance(o, dict):
            for v in o.values():
                yield from strings(v)
        elif isinstance(o, list):
            for v in o:
                yield from strings(v)
        elif isinstance(o, str):
            yield o
    assert max(len(s) for s in strings(d)) <= 160
    # round 6's object with the fp32 run of the headline shard added: the new entry keeps its value and parity numbers, the
    # decode figures stay on the line (the input-width / batch-size extras are what gives way first)
    r6 = json.load(open(os.path.join(root, 'profiles', 'r06_bench_default.json')))
    r6['headline_f32'] = dict(r6['cfgA'], workload='the headline shard with fp32 operands', value=5.1e5, ms_per_step=12.5)
    r6['blstmp'] = dict(workload='blstm 5x256 LSTMCell num_proj 128', value=3.02e5, ms_per_step=21.2, unit='frames/s',
                        cluster_handoff_flags=0, final_loss=1000.0)
    l6 = bench.compact_line(dict(r6, full='bench_full.json'))
    d6 = json.loads(l6)
    assert len(l6) < 6000 and d6['headline_f32']['value'] == 5.1e5
    assert d6['blstmp'] in ('see full', dict(value=3.02e5, ms_per_step=21.2, cluster_handoff_flags=0))
    assert d6['headline_f32']['parity']['greedy_label_mismatch'] == r6['cfgA']['parity']['greedy_label_mismatch']
    assert d6['decode']['kanji3387_beam100']['beam']['ms_per_call'] > 0 and d6['cfgE']['value'] > 0
    # N = 8: per-rank tables and the communication summary ride on the same line
    multi = dict(full, n_gpus=8, per_rank=dict(step_median_ms=[9.31] * 8, frames=[6400.0 + i for i in range(8)],
                                               elapsed_s=[0.1871234] * 8, comm_stream_allreduce_ms_per_step=[0.71] * 8),
                 comm=dict(allreduce_calls_per_step=3.0, allreduce_ms_per_step=0.7, bytes_per_step=2.2e7, bucket_min_mb=4.0,
                           buckets=[dict(layers=[4, 3], mbytes=8.0)] * 3, note='x' * 300))
    l8 = bench.compact_line(multi)
    d8 = json.loads(l8)
    assert len(l8) < 6000 and len(d8['per_rank']['frames']) == 8 and 'buckets' not in d8['comm']
    # pathological growth (many more kernels per auxiliary entry): entries are shed, the headline never is
    fat = json.loads(json.dumps(full))
    for k in ('cfgA', 'cfgC', 'cfgD', 'cfgE', 'input_width_D39'):
        fat[k]['kernels'] = {'kernel_%03d' % i: dict(calls=5, total_ms=1.0, avg_us=200.0 + i) for i in range(60)}
    lf = bench.compact_line(fat)
    df = json.loads(lf)
    assert len(lf) <= 6000 and df['roofline']['frac'] > 0 and df['cpu_baseline']['value'] > 0 and df['cfgC']['value'] > 0


def test_bench_compact_line_of_a_plain_run():
    """A plain `bench.py` run (no --full) times the headline only: its object has no h2d leg, parity, CPU baseline,
    auxiliary entries or full-result file.  compact_line must still carry every contract key, and the entries that
    were not run are null or absent, never invented."""
    import json
    bench, root = _load_bench_module()
    r6 = json.load(open(os.path.join(root, 'profiles', 'r06_bench_default.json')))
    keep = ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
            'vs_baseline', 'dtype', 'data', 'config', 'step_ms', 'final_loss', 'cluster_handoff_flags', 'kernels', 'roofline')
    plain = {k: r6[k] for k in keep}
    plain.update(h2d_inclusive=None, parity=None, cpu_baseline=None, cfgA=None, full=None)
    line = bench.compact_line(plain)
    d = json.loads(line)
    for k in keep:
        assert k in d, k
    assert d['metric'] == r6['metric'] and d['unit'] == 'frames/s' and d['higher_is_better'] is True
    assert abs(d['value'] - r6['value']) < 1e-4 * r6['value'] and abs(d['ms_per_step'] - r6['ms_per_step']) < 1e-4 * r6['ms_per_step']
    assert d['parity'] is None and d['cpu_baseline'] is None and d['full'] is None and d['h2d_inclusive'] == {}
    for k in ('cfgA', 'cfgC', 'cfgD', 'cfgE', 'decode', 'bgru', 'blstmp', 'batch_scaling', 'headline_f32'):
        assert k not in d, k
    assert d['roofline']['frac'] > 0 and len(line) < 6000


def test_bench_conv_roofline_credits_chunked_calls_with_their_own_images():
    """VERDICT r05 weak 3 / ADVICE r05: with the VGG forward going through in runs of images a step makes several calls
    per convolution kernel, each on PART of the batch; bench.conv_roofline must credit every timed call with the images
    it processed and take the step count from the timed loop.  A canned record of 5 steps x 2 runs (the shape of
    profiles/r05_bench_steps20_warmup5.json: conv3x3_fwd.calls 20, conv3x3_fwd_drop.calls 10) must give the rate of
    the WHOLE batch over the summed event time -- half of what counting calls as steps reported -- and the same figure
    as the unchunked record of the same work; a record whose work does not add up to the batch is refused."""
    bench, _ = _load_bench_module()
    F, W, frames, steps, runs = 40, 11, 57600, 5, 2
    p1, p2 = F * W, ((F + 1) // 2) * ((W + 1) // 2)
    f64, f128a, f128b = 2.0 * 9 * p1 * 64 * 64, 2.0 * 9 * p2 * 64 * 128, 2.0 * 9 * p2 * 128 * 128
    per_frame = f64 + f128a + f128b
    ms = dict(fwd=(2.559 + 1.960) / runs, drop=1.9 / runs)               # event time of one call on half the images
    ks = dict(conv3x3_fwd=dict(calls=2 * runs * steps, total_ms=ms['fwd'] * runs * steps, avg_us=1e3 * ms['fwd'] / 2,
                               work=(f64 + f128b) * frames * steps),
              conv3x3_fwd_drop=dict(calls=runs * steps, total_ms=ms['drop'] * runs * steps, avg_us=1e3 * ms['drop'],
                                    work=f128a * frames * steps))
    r = bench.conv_roofline(F, W, frames, steps, ks)
    want = per_frame * frames / ((2.559 + 1.960 + 1.9) * 1e-3) / 1e12
    assert abs(r['achieved'] - want) < 1e-9 * want and abs(r['frac'] - want / 2500.0) < 1e-12
    assert r['calls_per_step'] == 3 * runs and abs(r['ms_per_step'] - (2.559 + 1.960 + 1.9)) < 1e-9
    # what round 5 printed for such a record (steps := calls of conv3x3_fwd_drop) was exactly twice this
    r05 = per_frame * frames * ks['conv3x3_fwd_drop']['calls'] / ((ks['conv3x3_fwd']['total_ms'] + ks['conv3x3_fwd_drop']['total_ms']) * 1e-3) / 1e12
    assert abs(r05 / r['achieved'] - runs) < 1e-9
    one = dict(conv3x3_fwd=dict(calls=2 * steps, total_ms=(2.559 + 1.960) * steps, avg_us=0.0, work=(f64 + f128b) * frames * steps),
               conv3x3_fwd_drop=dict(calls=steps, total_ms=1.9 * steps, avg_us=0.0, work=f128a * frames * steps))
    assert abs(bench.conv_roofline(F, W, frames, steps, one)['achieved'] - r['achieved']) < 1e-9 * want
    bad = {k: dict(v) for k, v in ks.items()}
    bad['conv3x3_fwd']['work'] *= 0.5                                      # calls that saw half the images
    with pytest.raises(AssertionError):
        bench.conv_roofline(F, W, frames, steps, bad)
    with pytest.raises(AssertionError):
        bench.conv_roofline(F, W, frames, 3, ks)                           # calls not a multiple of the steps
    # per-call work of the timer's own accounting: [n, H, W, Cin] against a [Cout, 9 Cin] weight image; gemm by layout
    x = torch.empty((7, 20, 6, 64)); w = torch.empty((128, 9 * 64))
    assert bench._conv_work((x, w), {}) == 2.0 * 7 * 20 * 6 * 9 * 64 * 128
    A = torch.empty((300, 64)); B = torch.empty((300, 32))
    assert bench._gemm_work((A, B), dict(transA=True)) == ('gemm_tn', 2.0 * 64 * 32 * 300)
    assert bench._gemm_work((A, B.t().contiguous(), False, False), {})[0] == 'gemm_nn'
    assert bench._gemm_work((A, torch.empty((48, 64))), dict(transB=True)) == ('gemm_nt', 2.0 * 300 * 48 * 64)
    # the dominant entry is the group with the most event time per step, whatever its bound
    g = dict(a=dict(kernel='a', ms_per_step=3.0, frac=0.4), b=dict(kernel='b', ms_per_step=9.5, frac=0.01), c=None)
    assert bench.dominant_roofline(g)['kernel'] == 'b'


@pytest.mark.parametrize('enc,L,B', [('blstm', 2, 37), ('lstm', 2, 20), ('blstm', 1, 33)])
def test_encoder_half_batch_pipelines_against_the_oracle(monkeypatch, enc, L, B):
    """models/encoders/core/blstm.py ENC_HALVES: with at least two 16-utterance tiles the padded batch goes through the
    layer stack as two independent pipelines (B = 37 -> 48 rows -> 32 + 16; B = 20 -> 32 rows -> 16 + 16) whose weight
    gradients meet in the second part's accumulating products.  On the CPU stand-ins: loss, logits, EVERY gradient and
    the final states against the oracle, and against the single pipeline of the same model (halves switched off)."""
    _cpu_ops.install(monkeypatch)
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    rng = np.random.RandomState(15)
    T, D, H, C = 9, 6, 8, 6
    x, sl, labs, dense = _batch(rng, B, T, D, C)
    model = CTC(encoder_type=enc, input_size=D, num_units=H, num_layers=L, num_classes=C, parameter_init=0.1,
                clip_grad_norm=5.0, clip_activation=50, dtype='f32', seed=3, device='cpu')
    sd = {k: v.numpy().copy() for k, v in model.store.state_dict().items()}
    for k in sd:
        if k.endswith('/bias') or k.endswith('/biases'):
            sd[k] = (rng.randn(*sd[k].shape) * 0.05).astype(np.float32)
    model.store.load_state_dict({k: torch.tensor(v) for k, v in sd.items()})
    ref = omodel.ctc_model_forward(sd, x, labs, sl, L, ndir=2 if enc == 'blstm' else 1, cell_clip=50.0)
    model.encoder.halves = True           # (measured slower on the device than one pipeline: off by default)
    loss, logits = model.compute_loss(x, dense, sl, keep_prob=1.0)
    assert model.encoder._split == ((((B + 15) // 16) + 1) // 2) * 16 and model.encoder.layers_b is not None
    assert abs(loss.item() - ref['total_loss']) / abs(ref['total_loss']) < 1e-5
    assert np.abs(logits.numpy() - ref['logits']).max() < 1e-5
    fs_two = [np.stack([t.numpy() for t in st]) for st in model.encoder._state_tuple(model.encoder._finals, L)]
    opt = model._set_optimizer('sgd', 0.1)
    _check_grads(opt, loss, model, ref)
    g_two = {n: g.numpy().copy() for g, n in opt.compute_gradients(model.compute_loss(x, dense, sl, keep_prob=1.0)[0], model=model)}
    # the single pipeline of the same model
    model.encoder.halves = False
    loss1, logits1 = model.compute_loss(x, dense, sl, keep_prob=1.0)
    assert model.encoder._split == 0
    assert abs(loss1.item() - loss.item()) < 1e-6 * abs(loss.item()) and np.abs(logits1.numpy() - logits.numpy()).max() < 1e-6
    fs_one = [np.stack([t.numpy() for t in st]) for st in model.encoder._state_tuple(model.encoder._finals, L)]
    for a, b in zip(fs_one, fs_two):
        assert np.abs(a - b).max() < 1e-6
    for g, n in opt.compute_gradients(loss1, model=model):
        assert np.abs(g.numpy() - g_two[n]).max() < 1e-5 * max(1e-3, np.abs(g_two[n]).max()), n
    # dropout: the two parts draw from disjoint stretches of the layer's stream, a training step stays finite
    model.encoder.halves = True
    l2, _ = model.compute_loss(x, dense, sl, keep_prob=0.7)
    model.train(l2, 'adam', 1e-3)
    assert np.isfinite(l2.item()) and all(np.isfinite(v.numpy()).all() for v in model.store.state_dict().values())


def test_upload_ints_host_path_keeps_values_and_dtypes():
    """ops.upload_ints without a GPU device: plain int32 tensors, one per vector, input arrays left alone."""
    import torch
    from tensorflow_end2end_speech_recognition_amd import ops
    lens = np.array([5, 7, 9], np.int64)
    flat = [1, 2, 3, 4, 5]
    a, b, c = ops.upload_ints('cpu', [lens, flat, torch.tensor([3, 1], dtype=torch.int64)])
    assert a.dtype == b.dtype == c.dtype == torch.int32
    assert a.tolist() == [5, 7, 9] and b.tolist() == flat and c.tolist() == [3, 1]
    a[0] = 99
    assert lens[0] == 5
