"""Host logic of time subsampling (subsample_list / subsample_type) on the CPU stand-ins: the statement's own properties,
the segment wiring of models/encoders/core/subsample.py under CTC / AttentionSeq2Seq / JointCTCAttention against the
float64 statement (tests/_cpu_ops_subsample.py), the keyword contract of the models, and the TIMIT recipe."""
import os
import sys

import numpy as np
import pytest
import torch

import _cpu_ops_subsample as sub
from _corpus import make_timit_like
from oracle import attention as oatt
from oracle import optim as oopt

KINDS = ('drop', 'concat')
PKG = 'tensorflow_end2end_speech_recognition_amd'


# ---------------------------------------------------------------- the statement itself
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('T', [9, 8, 1])
def test_statement_backward_is_the_transpose_of_the_forward(kind, T):
    rng = np.random.RandomState(T)
    Bp, W = 6, 5
    lens = np.minimum(np.array([T, 8, 1, 2, 5, 0], dtype=np.int32), T)
    x = rng.randn(T, Bp, W)
    y, lo = sub.subsample_fwd_np(x, lens, kind)
    assert np.array_equal(lo, lens >> 1) and y.shape == (Bp, T // 2, W * (2 if kind == 'concat' else 1))
    dy = rng.randn(T // 2, Bp, y.shape[2])
    dx = sub.subsample_bwd_np(dy, lo, T, kind)
    assert dx.shape == x.shape
    # <y, dy> = <x, dx>, with dy restricted to the rows the forward defines (the others are zero in y)
    lhs = float((y.transpose(1, 0, 2).astype(np.float64) * dy).sum())
    assert abs(lhs - float((x * dx).sum())) < 1e-5 * max(1.0, abs(lhs))
    # the torch form of the statement is the numpy one
    yt, lt = sub.reduce_torch(torch.tensor(x), torch.tensor(lens.astype(np.int64)), kind)
    assert np.array_equal(lt.numpy(), lo) and np.array_equal(yt.numpy().transpose(1, 0, 2).astype(np.float32), y)


def test_drop_at_the_last_layer_is_the_plain_encoder_at_odd_frames(monkeypatch):
    sub.install(monkeypatch)
    from tensorflow_end2end_speech_recognition_amd.models.encoders.core.blstm import BLSTMEncoder
    from tensorflow_end2end_speech_recognition_amd.models.encoders.core.subsample import SubsampledBLSTMEncoder
    rng = np.random.RandomState(1)
    B, T, D, H, L = 3, 9, 6, 8, 2
    x = torch.tensor(rng.randn(B, T, D).astype(np.float32))
    sl = torch.tensor([9, 6, 3], dtype=torch.int32)
    kw = dict(num_units=H, num_proj=None, num_layers=L, lstm_impl='LSTMBlockCell', use_peephole=True, parameter_init=0.1,
              clip_activation=50, seed=4)
    plain = BLSTMEncoder(**kw)
    out_p, fin_p = plain(x, sl, 1.0, False)
    enc = SubsampledBLSTMEncoder(subsample_list=[False, True], subsample_type='drop', **kw)
    out_s, fin_s = enc(x, sl, 1.0, False)
    assert list(enc.store.names) == list(plain.store.names)
    want = out_p[1:2 * (T // 2):2].clone()
    for b in range(B):
        want[int(sl[b]) // 2:, b] = 0
    assert out_s.shape == (T // 2, B, 2 * H) and torch.equal(out_s, want)
    assert np.array_equal(enc.seq_len_padded[:B].numpy(), sl.numpy() >> 1)
    for d in range(2):
        assert torch.equal(fin_s[d].c, fin_p[d].c) and torch.equal(fin_s[d].h, fin_p[d].h)
    assert np.array_equal(enc.output_seq_len(sl.numpy()), sl.numpy() >> 1)


# ---------------------------------------------------------------- CTC
def _batch(rng, B, T, D, C, k):
    x = rng.randn(B, T, D).astype(np.float32)
    sl = rng.randint(max(2 << k, T // 2), T + 1, size=B).astype(np.int32)
    sl[0] = T
    labs = []
    for b in range(B):
        x[b, sl[b]:] = 0
        labs.append([int(v) for v in rng.randint(0, C, size=max(1, (int(sl[b]) >> k) // 2))])
    dense = np.full((B, max(len(l) for l in labs)), -1, dtype=np.int64)
    for b, l in enumerate(labs):
        dense[b, :len(l)] = l
    return x, sl, labs, dense


def _ctc(enc, D, H, L, C, **kw):
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    return CTC(encoder_type=enc, input_size=D, num_units=H, num_layers=L, num_classes=C, parameter_init=0.1,
               clip_grad_norm=0.05, clip_activation=50, dtype='f32', seed=3, device='cpu', **kw)


@pytest.mark.parametrize('lst,kind', [((False, True, False), 'drop'), ((True, False, True), 'concat')])
@pytest.mark.parametrize('enc', ['blstm', 'lstm'])
def test_subsampled_ctc_model_host_logic(monkeypatch, enc, lst, kind):
    sub.install(monkeypatch)
    rng = np.random.RandomState(5)
    B, T, D, H, L, C = 5, 13, 6, 8, 3, 6                # B is padded to 16 utterances inside every segment
    k, ndir = sum(lst), 2 if enc == 'blstm' else 1
    x, sl, labs, dense = _batch(rng, B, T, D, C, k)
    model = _ctc(enc, D, H, L, C, subsample_list=list(lst), subsample_type=kind)
    plain = _ctc(enc, D, H, L, C)
    # variable names and creation order are the plain model's; a drop model is checkpoint-compatible, a concat model
    # differs only in the input height of the kernels that follow a reduction
    assert list(model.store.names) == list(plain.store.names)
    for li in range(1, L + 1):
        for name in model.encoder.layers[li - 1].var_names():
            a, b = tuple(model.store[name].shape), tuple(plain.store[name].shape)
            if kind == 'concat' and name.endswith('/kernel') and li >= 2 and lst[li - 2]:
                assert a == (b[0] + ndir * H, b[1]), name
            else:
                assert a == b, name
    if kind == 'drop':
        for name in plain.store.names:
            assert torch.equal(model.store[name], plain.store[name]), name
    assert tuple(model.store['output/weights'].shape) == (ndir * H * (2 if kind == 'concat' and lst[-1] else 1), C + 1)
    sd = {n: v.numpy().copy() for n, v in model.store.state_dict().items()}
    for n in sd:
        if n.endswith('/bias') or n.endswith('/biases'):
            sd[n] = (rng.randn(*sd[n].shape) * 0.05).astype(np.float32)
    model.store.load_state_dict({n: torch.tensor(v) for n, v in sd.items()})
    ref = sub.ctc_model_forward(sd, x, labs, sl, L, ndir, lst, kind, cell_clip=50.0)
    loss, logits = model.compute_loss(x, dense, sl, keep_prob=1.0)
    assert logits.shape == (T >> k, B, C + 1)
    assert abs(loss.item() - ref['total_loss']) / abs(ref['total_loss']) < 1e-5
    assert np.abs(logits.numpy() - ref['logits']).max() < 1e-5
    # output_seq_len: numpy, list, tensor
    assert np.array_equal(model.output_seq_len(sl), sl >> k)
    assert np.array_equal(model.output_seq_len([int(v) for v in sl]), sl >> k)
    assert torch.equal(model.output_seq_len(torch.tensor(sl)), torch.tensor(sl >> k))
    assert plain.output_seq_len(sl) is sl
    assert np.array_equal(model.encoder.seq_len_padded[:B].numpy(), sl >> k)
    # every gradient; the hook fires once per layer, global indices, top layer first
    fired = []
    model.encoder.grad_ready_hook = lambda li, layer: fired.append((li, layer))
    opt = model._set_optimizer('sgd', 0.1)
    seen = set()
    for g, name in opt.compute_gradients(loss, model=model):
        r = ref['grads'][name]
        seen.add(name)
        err = np.abs(g.numpy() - r).max()
        assert err < 1e-4 * max(np.abs(r).max(), 1e-3) + 1e-7, (name, err, np.abs(r).max())
    assert seen == set(ref['grads'])
    assert [li for li, _ in fired] == list(reversed(range(L)))
    assert all(layer is model.encoder.layers[li] for li, layer in fired)
    model.encoder.grad_ready_hook = None
    # one full training step: per-variable clip, then the update
    before = {n: v.numpy().copy() for n, v in model.store.state_dict().items()}
    loss, _ = model.compute_loss(x, dense, sl, keep_prob=1.0)
    model.train(loss, 'momentum', 0.1)
    after = model.store.state_dict()
    for name, r in ref['grads'].items():
        want = before[name] - 0.1 * oopt.clip_by_norm(r, 0.05)
        assert np.abs(after[name].numpy() - want).max() < 1e-5, name
    # decode plumbing on the reduced lengths
    from tensorflow_end2end_speech_recognition_amd.utils.io.labels.sparsetensor import list2sparsetensor
    dec = model.decoder(logits, model.output_seq_len(sl), beam_width=1)
    assert 0.0 <= model.compute_ler(dec, list2sparsetensor(dense, -1))


@pytest.mark.parametrize('enc', ['blstm', 'lstm'])
def test_all_false_list_builds_exactly_the_plain_model(monkeypatch, enc):
    sub.install(monkeypatch)
    rng = np.random.RandomState(6)
    B, T, D, H, L, C = 4, 11, 6, 8, 2, 6
    x, sl, labs, dense = _batch(rng, B, T, D, C, 0)
    plain = _ctc(enc, D, H, L, C)
    for lst in (None, [False, False]):
        model = _ctc(enc, D, H, L, C, subsample_list=lst, subsample_type='concat')
        assert type(model.encoder) is type(plain.encoder)
        assert list(model.store.names) == list(plain.store.names)
        a, la = model.compute_loss(x, dense, sl, keep_prob=1.0)
        b, lb = plain.compute_loss(x, dense, sl, keep_prob=1.0)
        assert a.numpy().tobytes() == b.numpy().tobytes() and torch.equal(la, lb)


def test_dropout_counters_stay_indexed_by_the_global_layer(monkeypatch):
    """Layer li of a subsampled stack draws its mask at rng_state[1] + li * 2^32, as the plain stack does."""
    ops = sub.install(monkeypatch)
    from tensorflow_end2end_speech_recognition_amd.models.encoders.core.subsample import SubsampledBLSTMEncoder
    seen = []
    real = ops.dropout_apply
    monkeypatch.setattr(ops, 'dropout_apply', lambda t, keep, seed, offset: (seen.append((seed, offset)), real(t, keep, seed, offset))[1])
    enc = SubsampledBLSTMEncoder(num_units=8, num_proj=None, num_layers=3, lstm_impl='LSTMBlockCell', use_peephole=True,
                                 parameter_init=0.1, clip_activation=50, seed=2, subsample_list=[True, False, True],
                                 subsample_type='drop')
    x = torch.tensor(np.random.RandomState(0).randn(2, 8, 6).astype(np.float32))
    enc(x, torch.tensor([8, 5], dtype=torch.int32), 0.8, True, rng_state=(9, 1 << 40))
    assert seen == [(9, (1 << 40) + li * (1 << 32)) for li in range(3)]


def test_value_errors(monkeypatch):
    sub.install(monkeypatch)
    from tensorflow_end2end_speech_recognition_amd.models.ctc.multitask_ctc import MultitaskCTC
    from tensorflow_end2end_speech_recognition_amd.models.ctc.student_ctc import StudentCTC
    with pytest.raises(ValueError):
        _ctc('blstm', 6, 8, 3, 6, subsample_list=[True, False])                     # one entry per layer
    with pytest.raises(ValueError):
        _ctc('blstm', 6, 8, 2, 6, subsample_list=[True, False], subsample_type='max')
    with pytest.raises(ValueError):
        _ctc('blstm', 6, 8, 2, 6, subsample_list=None, subsample_type='max')
    for enc in ('gru', 'bgru', 'vgg_blstm', 'vgg_lstm', 'cldnn_wang', 'cnn_zhang'):
        with pytest.raises(ValueError):
            _ctc(enc, 6, 8, 2, 6, subsample_list=[True, False])
    with pytest.raises(ValueError):
        _ctc('blstm', 6, 8, 2, 6, subsample_list=[True, False], lstm_impl='LSTMCell', num_proj=4)
    with pytest.raises(ValueError):
        MultitaskCTC(encoder_type='multitask_blstm', input_size=6, num_units=8, num_layers_main=2, num_layers_sub=1,
                     num_classes_main=6, num_classes_sub=3, main_task_weight=0.5, device='cpu',
                     subsample_list=[True, False])
    with pytest.raises(ValueError):
        StudentCTC(encoder_type='student_cnn_ctc', input_size=120, num_classes=6, device='cpu', subsample_list=[True])
    # a real utterance that reduces to zero frames: from the host lengths, before anything runs
    model = _ctc('blstm', 6, 8, 2, 6, subsample_list=[True, True])
    x = np.zeros((2, 9, 6), dtype=np.float32)
    with pytest.raises(ValueError):
        model.compute_loss(x, np.zeros((2, 1), dtype=np.int64), np.array([9, 3], dtype=np.int32), keep_prob=1.0)
    # no new registry key: the function of pyramid_blstm is subsample_type='concat'
    from tensorflow_end2end_speech_recognition_amd.models.encoders.load_encoder import load
    with pytest.raises(ValueError):
        load('pyramid_blstm')


# ---------------------------------------------------------------- attention / joint
def _att_batch(rng, B, T, D, C, k):
    x = rng.randn(B, T, D).astype(np.float32)
    sl = rng.randint(max(2 << k, T // 2), T + 1, size=B).astype(np.int32)
    sl[0] = T
    lens = np.array([max(1, min(4, (int(s) >> k) // 2)) for s in sl])
    sos, eos = C, C + 1
    labels = np.full((B, int(lens.max()) + 2), eos, dtype=np.int64)
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


@pytest.mark.parametrize('joint,att,lst,kind', [(False, 'location', (True, False), 'drop'),
                                                (True, 'bahdanau_content', (False, True), 'concat')])
def test_subsampled_attention_models_host_logic(monkeypatch, joint, att, lst, kind):
    sub.install(monkeypatch)
    from tensorflow_end2end_speech_recognition_amd.models.attention.attention_seq2seq import AttentionSeq2Seq
    from tensorflow_end2end_speech_recognition_amd.models.attention.joint_ctc_attention import JointCTCAttention
    rng = np.random.RandomState(11)
    B, T, D, H, L, U, A, Em, C = 3, 11, 6, 8, 2, 12, 10, 4, 6
    x, sl, labels, lsl, ctc_labels = _att_batch(rng, B, T, D, C, 1)
    kw = dict(subsample_list=list(lst), subsample_type=kind)
    model = _mk_att(JointCTCAttention, att, D, H, L, U, A, Em, C, lambda_weight=0.5, **kw) if joint else \
        _mk_att(AttentionSeq2Seq, att, D, H, L, U, A, Em, C, **kw)
    plain = _mk_att(JointCTCAttention, att, D, H, L, U, A, Em, C, lambda_weight=0.5) if joint else \
        _mk_att(AttentionSeq2Seq, att, D, H, L, U, A, Em, C)
    assert list(model.store.names) == list(plain.store.names)
    sd = {n: v.numpy().copy() for n, v in model.store.state_dict().items()}
    sl_out = model.output_seq_len(sl)
    assert np.array_equal(sl_out, sl >> 1) and plain.output_seq_len(sl) is sl
    sub.patch_oracle_blstm_encoder(monkeypatch, sl, lst, kind)
    okw = dict(clip_enc=50.0, clip_dec=50.0)
    if joint:
        ctc_list = [[int(v) for v in row if v >= 0] for row in ctc_labels]
        ref = oatt.attention_model_forward(sd, x, labels, sl_out, lsl, L, att, ctc_labels=ctc_list, lambda_weight=0.5,
                                           **okw)
        loss, logits, ctc_logits, out_train, out_infer = model.compute_loss(x, labels, ctc_labels, sl, lsl, 1.0, 1.0, 1.0)
        assert ctc_logits.shape == (T // 2, B, C + 1)
        assert np.abs(ctc_logits.numpy() - ref['ctc_logits']).max() < 1e-5
    else:
        ref = oatt.attention_model_forward(sd, x, labels, sl_out, lsl, L, att, **okw)
        loss, logits, out_train, out_infer = model.compute_loss(x, labels, sl, lsl, 1.0, 1.0, 1.0)
    assert abs(loss.item() - ref['total_loss']) / abs(ref['total_loss']) < 1e-5
    assert out_train.attention_weights.shape[2] == T // 2
    assert np.abs(out_train.attention_weights.numpy() - ref['alphas']).max() < 1e-5
    opt = model._set_optimizer('adam', 1e-3)
    seen = set()
    for g, name in opt.compute_gradients(loss, model=model):
        r = ref['grads'][name]
        seen.add(name)
        err = np.abs(g.numpy() - r).max()
        assert err < 1e-4 * max(np.abs(r).max(), 1e-3) + 1e-7, (name, err, np.abs(r).max())
    assert seen == set(ref['grads'])
    ref_ids = oatt.attention_model_infer(sd, x, sl_out, L, att, C, C + 1, 8, **okw)
    assert np.array_equal(model.infer(x, sl), ref_ids)
    short = sl.copy()
    short[1] = 1
    with pytest.raises(ValueError):
        model.infer(x, short)


# ---------------------------------------------------------------- the recipe
def test_timit_subsample_recipe_on_cpu_stand_ins(monkeypatch, tmp_path):
    """examples/timit/config/ctc/blstm_ctc_phone61_subsample.yml through train_ctc.py and eval_ctc.py on a generated
    corpus (every frame held twice, so that the 2x reduction leaves room for the transcripts)."""
    import pickle
    import random
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    sub.install(monkeypatch)
    from examples.timit.training import train_ctc
    from examples.timit.evaluation import eval_ctc
    corpus = str(tmp_path / 'corpus')
    make_timit_like(corpus, np.random.RandomState(0))
    for data_type in ('train', 'dev', 'test'):
        d = os.path.join(corpus, 'inputs', data_type)
        with open(os.path.join(d, 'frame_num.pickle'), 'rb') as f:
            frame_num = pickle.load(f)
        for name in frame_num:
            path = os.path.join(d, name + '.npy')
            np.save(path, np.repeat(np.load(path), 2, axis=0))
            frame_num[name] *= 2
        with open(os.path.join(d, 'frame_num.pickle'), 'wb') as f:
            pickle.dump(frame_num, f)
    with open(os.path.join(root, 'examples/timit/config/ctc/blstm_ctc_phone61_subsample.yml')) as f:
        cfg = yaml.safe_load(f)
    assert cfg['param']['subsample_list'] == [False, True, False, False, False]
    assert cfg['param']['subsample_type'] == 'drop' and cfg['param']['num_layers'] == 5
    # the topology shrunk as the plain recipe test shrinks it: two layers, the list cut to them (layer 1 reduced)
    cfg['param'].update(num_layers=2, subsample_list=cfg['param']['subsample_list'][1:3])
    cfg['param'].update(input_size=6, num_units=8, batch_size=8, num_epoch=30, eval_start_epoch=1, print_step=3,
                        optimizer='adam', learning_rate=0.05, dropout=0.0, weight_decay=0, decay_start_epoch=2,
                        dtype='f32', device='cpu', dataset_root=corpus, sort_stop_epoch=2, not_improved_patient_epoch=100)
    cfg_path = str(tmp_path / 'cfg.yml')
    with open(cfg_path, 'w') as f:
        yaml.safe_dump(cfg, f)
    random.seed(0)
    res = train_ctc.main(cfg_path, str(tmp_path / 'runs'))
    run = res['save_path']
    assert run.endswith(os.path.join('ctc', 'phone61', 'blstm_ctc_8_2_adam_lr0.05_subdrop1'))
    assert len(res['ler_dev']) == 30 and res['checkpoints'] and res['ler_test'] is not None
    assert min(res['ler_dev']) < 0.9
    log = open(os.path.join(run, 'train.log')).read()
    assert 'Total 22 variables' in log and '-----EPOCH:30' in log and 'PER:' in log
    per = eval_ctc.main([run, '--beam_width', '1', '--device', 'cpu'])
    assert abs(per - res['ler_test']) < 1e-9
