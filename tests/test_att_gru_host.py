"""CPU: the GRU decoder of the attention models (decoder_type='gru') -- variables, bridge, rng stream, the three refusals,
the recipe, and the host logic of AttentionSeq2Seq / JointCTCAttention on the stand-ins of tests/_cpu_ops_att_gru.py against
the float64 statement of tests/_att_gru_oracle.py (loss, logits, every gradient, greedy and beam decode)."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

import _att_gru_oracle as go
import _cpu_ops_att_gru as cg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

D = 'attention_decoder/decoder/'


def _mk(cls, att, Din, H, L, U, A, Em, C, decoder_type='gru', **kw):
    kw.setdefault('max_decode_length', 10)
    kw.setdefault('seed', 5)
    return cls(input_size=Din, encoder_type='blstm', encoder_num_units=H, encoder_num_layers=L, encoder_num_proj=None,
               attention_type=att, attention_dim=A, decoder_type=decoder_type, decoder_num_units=U, decoder_num_layers=1,
               embedding_dim=Em, num_classes=C, sos_index=C, eos_index=C + 1, parameter_init=0.1, clip_grad_norm=5.0,
               clip_activation_encoder=50, clip_activation_decoder=50, dtype='f32', device='cpu', **kw)


def _models():
    from tensorflow_end2end_speech_recognition_amd.models.attention.attention_seq2seq import AttentionSeq2Seq
    from tensorflow_end2end_speech_recognition_amd.models.attention.joint_ctc_attention import JointCTCAttention
    return AttentionSeq2Seq, JointCTCAttention


def _batch(rng, B, T, Din, C, lens):
    """Ragged inputs and <SOS> y <EOS> labels padded with <EOS>, y of the given lengths."""
    x = rng.randn(B, T, Din).astype(np.float32)
    sl = rng.randint(max(2, T // 2), T + 1, size=B).astype(np.int32)
    sl[0] = T
    lens = np.asarray(lens)
    sos, eos = C, C + 1
    labels = np.full((B, int(lens.max()) + 2), eos, dtype=np.int64)
    ctc = np.full((B, int(lens.max())), -1, dtype=np.int64)
    for b in range(B):
        x[b, sl[b]:] = 0
        y = rng.randint(0, C, size=lens[b])
        labels[b, 0] = sos
        labels[b, 1:1 + lens[b]] = y
        ctc[b, :lens[b]] = y
    return x, sl, labels, lens + 2, ctc


def test_variables_bridge_and_creation_order(monkeypatch):
    cg.install(monkeypatch)
    Att, _ = _models()
    Din, H, L, U, A, Em, C = 6, 8, 1, 12, 10, 4, 6
    gru = _mk(Att, 'location', Din, H, L, U, A, Em, C)
    lstm = _mk(Att, 'location', Din, H, L, U, A, Em, C, decoder_type='lstm')
    sd = gru.store.state_dict()
    E2 = 2 * H
    want = {D + 'gru_cell/gates/kernel': (Em + E2 + U, 2 * U), D + 'gru_cell/gates/bias': (2 * U,),
            D + 'gru_cell/candidate/kernel': (Em + E2 + U, U), D + 'gru_cell/candidate/bias': (U,),
            'bridge/fully_connected/weights': (4 * H, U), 'bridge/fully_connected/biases': (U,)}
    for name, shape in want.items():
        assert tuple(sd[name].shape) == shape, name
    assert not any('lstm_cell' in k for k in sd if k.startswith(D))
    assert float(sd[D + 'gru_cell/gates/bias'].min()) == 1.0 == float(sd[D + 'gru_cell/gates/bias'].max())
    assert float(sd[D + 'gru_cell/candidate/bias'].abs().max()) == 0.0
    assert float(sd[D + 'gru_cell/gates/kernel'].abs().max()) <= 0.1 and float(sd[D + 'gru_cell/gates/kernel'].std()) > 0.03
    # creation order: the four cell variables stand where lstm_cell/{kernel,bias,w_*_diag} stand in an LSTM model
    gn, ln = list(sd), list(lstm.store.state_dict())
    cell = [D + 'gru_cell/gates/kernel', D + 'gru_cell/gates/bias', D + 'gru_cell/candidate/kernel',
            D + 'gru_cell/candidate/bias']
    i = gn.index(cell[0])
    assert gn[i:i + 4] == cell
    j = ln.index(D + 'lstm_cell/kernel')
    assert i == j and gn[:i] == ln[:j] and gn[i + 4:] == ln[j + 5:]        # (kernel, bias, three peepholes)
    # everything drawn before the bridge is the same stream; the kernels are drawn where lstm_cell/kernel is
    lsd = lstm.store.state_dict()
    for k in gn[:gn.index('bridge/fully_connected/weights')]:
        assert torch.equal(sd[k], lsd[k]), k
    assert tuple(lsd['bridge/fully_connected/weights'].shape) == (4 * H, 2 * U)
    with pytest.raises(TypeError):
        _mk(Att, 'location', Din, H, L, U, A, Em, C, decoder_type='rnn')


def _digest(model):
    h = hashlib.sha256()
    for k, v in model.store.state_dict().items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v.cpu().numpy()).tobytes())
    return h.hexdigest()


# sha256 over (name, fp32 bytes) of every variable of the two LSTM-decoder models below, taken on the commit before the GRU
# decoder existed
_LSTM_DIGESTS = {'location': '56e12e0b36deb939c74f79502aa3026e8ec9908178b804d3cb73ccc0c454a7b2', 'joint': 'bf7759845a7e26e3d35c2a91e208249ddd2504067751f71da4e3f55ef02cb4db'}


def test_lstm_model_rng_draws_are_unchanged(monkeypatch):
    cg.install(monkeypatch)
    Att, Joint = _models()
    Din, H, L, U, A, Em, C = 6, 8, 2, 12, 10, 4, 6
    assert _digest(_mk(Att, 'location', Din, H, L, U, A, Em, C, decoder_type='lstm')) == _LSTM_DIGESTS['location']
    assert _digest(_mk(Joint, 'hybrid', Din, H, L, U, A, Em, C, decoder_type='lstm', lambda_weight=0.3,
                       prev_alpha='carry')) == _LSTM_DIGESTS['joint']


def test_the_three_refusals(monkeypatch):
    cg.install(monkeypatch)
    Att, Joint = _models()
    B, T, Din, H, L, U, A, Em, C = 3, 16, 6, 8, 1, 12, 10, 4, 6
    x, sl, labels, lsl, ctc = _batch(np.random.RandomState(0), B, T, Din, C, [4, 2, 3])
    model = _mk(Att, 'location', Din, H, L, U, A, Em, C)
    with pytest.raises(ValueError, match='scheduled_sampling_prob.*decoder_type="gru"'):
        model.compute_loss(x, labels, sl, lsl, 1.0, 1.0, 1.0, scheduled_sampling_prob=0.3)
    joint = _mk(Joint, 'location', Din, H, L, U, A, Em, C, lambda_weight=0.5)
    with pytest.raises(ValueError, match='ctc_weight.*decoder_type="gru"'):
        joint.infer(x, sl, beam_width=2, ctc_weight=0.3)
    for kw in (dict(lm=object()), dict(lm_weight=0.3), dict(lm=object(), lm_weight=0.3)):
        with pytest.raises(ValueError, match='decoder_type="gru"'):
            model.infer(x, sl, beam_width=2, **kw)
    with pytest.raises(ValueError, match='native'):
        model.infer(x, sl, native=False)
    # scheduled_sampling_prob = 0 is the teacher-forced GRU path; evaluation ignores the keyword's value only at 0
    model.compute_loss(x, labels, sl, lsl, 1.0, 1.0, 1.0, scheduled_sampling_prob=0.0)


@pytest.mark.parametrize('att,joint,prev', [('location', False, 'zeros'), ('location', False, 'carry'),
                                            ('luong_dot', False, 'zeros'), ('bahdanau_content', True, 'zeros')])
def test_model_host_logic_against_the_statement(monkeypatch, att, joint, prev):
    """One training step with decoder and embedding dropout on the stand-ins: loss, logits and every gradient against the
    float64 statement fed the step's masks, at the plain attention model's bars (loss 1e-4 relative, logits 2e-4, gradients
    2e-3 of their largest entry).  Label lengths 1 / 5 / 3 / 5: a row finishes at step 1, two at the last step -- the
    host-side recursion (dh0 into the [4H, U] bridge, no dc0; the cell's weight gradients batched over the steps) against
    autograd.  Greedy infer and infer(beam_width=...) run through the GRU loops and equal the statement's decode."""
    import _cpu_ops_att_ss as ss
    from tensorflow_end2end_speech_recognition_amd.utils.io.labels.sparsetensor import list2sparsetensor
    ops = cg.install(monkeypatch)
    Att, Joint = _models()
    B, T, Din, H, L, A, Em, C = 4, 18, 6, 8, 1, 10, 4, 6
    U = 2 * H if att == 'luong_dot' else 12
    x, sl, labels, lsl, ctc = _batch(np.random.RandomState(11), B, T, Din, C, [1, 5, 3, 5])
    kw = dict(sharpening_factor=1.5, logits_temperature=2.0, prev_alpha=prev)
    model = _mk(Joint, att, Din, H, L, U, A, Em, C, lambda_weight=0.5, honour_ctor_args=True, **kw) if joint else \
        _mk(Att, att, Din, H, L, U, A, Em, C, **kw)
    masks = ss.spy_dropout_masks(monkeypatch, ops)
    before = dict(cg.CALLS)
    if joint:
        loss, logits, _, otr, _ = model.compute_loss(x, labels, list2sparsetensor(ctc, -1), sl, lsl, 1.0, 0.8, 0.8)
    else:
        loss, logits, otr, _ = model.compute_loss(x, labels, sl, lsl, 1.0, 0.8, 0.8)
    by_seed = {m[2]: m for m in masks}
    demb = by_seed[model.seed + 1][4][:, :B].transpose(0, 1).numpy()
    ddec = by_seed[model.seed + 2][4][:, :B].numpy()
    sd = {k: v.numpy().copy() for k, v in model.store.state_dict().items()}
    ref = go.gru_model_forward(sd, x, labels, sl, lsl, L, att, clip_enc=50.0, sharpening=1.5, temperature=2.0,
                               drop_emb=demb, drop_dec=ddec, prev_alpha=prev,
                               ctc_labels=[[int(v) for v in r if v >= 0] for r in ctc] if joint else None,
                               lambda_weight=0.5 if joint else None)
    assert abs(loss.item() - ref['total_loss']) / abs(ref['total_loss']) < 1e-4
    assert np.abs(logits.numpy() - ref['logits'] * 2.0).max() < 2e-4
    assert np.abs(otr.attention_weights.numpy() - ref['alphas']).max() < 1e-5
    gv = model._set_optimizer('sgd', 0.1).compute_gradients(loss, model=model)
    names = set()
    for g, name in gv:
        r = ref['grads'][name]
        err = np.abs(g.numpy() - r).max()
        assert err < 2e-3 * max(np.abs(r).max(), 1e-3) + 1e-7, (name, err, np.abs(r).max())
        names.add(name)
    for name in ('gru_cell/gates/kernel', 'gru_cell/gates/bias', 'gru_cell/candidate/kernel', 'gru_cell/candidate/bias'):
        assert D + name in names and np.abs(ref['grads'][D + name]).max() > 0
    assert np.abs(ref['grads']['bridge/fully_connected/weights']).max() > 0
    assert cg.CALLS['fwd'] == before['fwd'] + 1 and cg.CALLS['bwd'] == before['bwd'] + 1
    # decoding (the output layer's weights times 40, as tests/test_gpu_att_beam.py does: at parameter_init = 0.1 the logits
    # of an untrained model are too flat for any margin)
    tsd = {k: v.clone() for k, v in model.store.state_dict().items()}
    tsd[D + 'output_layer/weights'] *= 40.0
    tsd[D + 'output_layer/biases'][C + 1] = 0.35
    model.store.load_state_dict(tsd)
    sd = {k: v.numpy().copy() for k, v in tsd.items()}
    ids, margin, lmax = go.gru_model_infer(sd, x, sl, L, att, C, C + 1, 10, clip_enc=50.0, sharpening=1.5, prev_alpha=prev)
    got = model.infer(x, sl)
    assert cg.CALLS['infer'] == before['infer'] + 1
    sure = margin > 10 * 2e-4
    n = min(got.shape[1], ids.shape[1])
    assert sure.mean() >= 0.9 and (got.shape[1] == ids.shape[1] or not sure.all())
    assert np.array_equal(got[:, :n][sure[:, :n]], ids[:, :n][sure[:, :n]])
    assert np.array_equal(model.infer(x, sl, beam_width=1), got)               # (width 1 IS the greedy loop)
    one = model._decode_beam(ops.to_device(x, torch.float32, model.device), ops.to_device(sl, torch.int32, model.device), 1)
    assert cg.CALLS['beam'] == before['beam'] + 1
    from tensorflow_end2end_speech_recognition_amd.models.attention.decoders.beam_search.beam_search_decoder import cut_at_eos
    if sure.all():
        for b in range(B):
            assert cut_at_eos(one[b], C + 1) == cut_at_eos(got[b], C + 1), b
    want = go.gru_beam_infer(sd, x, sl, L, att, C, C + 1, 10, 3, 0.6, clip_enc=50.0, sharpening=1.5, prev_alpha=prev)
    best = model.infer(x, sl, beam_width=3, length_penalty_weight=0.6)
    raw = model._beam_raw
    for b, r in enumerate(want):
        if not r['margin'] > 1e-3:
            continue
        for w in range(3):
            k = int(raw['hyp_len'][b, w])
            assert raw['ids'][b, w, :k].tolist() == r['ids'][w], (b, w)
        assert np.abs(raw['scores'][b] - r['scores']).max() < 1e-3
        assert best[b, :len(r['ids'][0])].tolist() == r['ids'][0]


def test_lstm_models_never_reach_the_gru_loops(monkeypatch):
    ops = cg.install(monkeypatch)
    Att, _ = _models()
    B, T, Din, H, L, U, A, Em, C = 3, 16, 6, 8, 1, 12, 10, 4, 6
    x, sl, labels, lsl, _ = _batch(np.random.RandomState(1), B, T, Din, C, [4, 2, 3])
    model = _mk(Att, 'location', Din, H, L, U, A, Em, C, decoder_type='lstm')
    before = dict(cg.CALLS)
    seen = []
    for name in ('att_decoder_fwd', 'att_decoder_bwd', 'att_decoder_infer', 'att_decoder_beam'):
        def wrap(a, *p, _f=getattr(ops, name), **k):
            seen.append('gru' in a)
            return _f(a, *p, **k)
        monkeypatch.setattr(ops, name, wrap)
    loss, *_ = model.compute_loss(x, labels, sl, lsl, 1.0, 0.8, 0.8)
    model._set_optimizer('sgd', 0.1).compute_gradients(loss, model=model)
    model.infer(x, sl)
    model.infer(x, sl, beam_width=2)
    assert cg.CALLS == before and seen == [False] * 4


def test_recipe_and_run_name():
    import yaml
    from examples.timit.training.train_attention import model_kwargs, run_name
    with open(os.path.join(ROOT, 'examples/timit/config/attention/blstm_attention_phone61_gru_decoder.yml')) as f:
        params = yaml.safe_load(f)['param']
    with open(os.path.join(ROOT, 'examples/timit/config/attention/blstm_attention_phone61.yml')) as f:
        base = yaml.safe_load(f)['param']
    assert params == dict(base, decoder_type='gru')
    assert run_name(params) == run_name(base) + '_grudec'
    assert run_name(dict(params, label_smoothing_prob=0.1)) == run_name(base) + '_grudec_ls0.1'
    assert model_kwargs(dict(params, num_classes=61))['decoder_type'] == 'gru'


@pytest.mark.parametrize('family', ['attention', 'joint'])
def test_timit_recipe_with_a_gru_decoder(monkeypatch, tmp_path, family):
    """examples/timit/training/train_{attention,joint_ctc_attention}.py on the synthetic corpus with the GRU decoder recipe:
    training steps and dev decodes go through the GRU loops, the run is tagged _grudec, and eval_attention.py rebuilds the
    model from the run's config.yml, restores a checkpoint and scores what the trained object scores."""
    import test_host_logic as thl
    cg.install(monkeypatch)
    corpus = str(tmp_path / 'corpus')
    thl._make_timit_like(corpus, np.random.RandomState(0), n_train=16, n_dev=4, n_test=3, multitask=False)
    from examples.timit.training import train_attention, train_joint_ctc_attention
    drv = train_attention if family == 'attention' else train_joint_ctc_attention
    cfg = thl._recipe_cfg(ROOT, 'examples/timit/config/attention/blstm_attention_phone61_gru_decoder.yml', tmp_path,
                          encoder_num_units=8, encoder_num_layers=1, attention_dim=6, decoder_num_units=8, embedding_dim=4,
                          max_decode_length=10, dropout_encoder=0.0, dropout_decoder=0.1, dropout_embedding=0.1,
                          input_size=6, batch_size=8, num_epoch=2, eval_start_epoch=1, print_step=2, optimizer='adam',
                          learning_rate=0.02, weight_decay=0, decay_start_epoch=2, dtype='f32', device='cpu',
                          dataset_root=corpus, sort_stop_epoch=2)
    before = dict(cg.CALLS)
    res = drv.main(cfg, str(tmp_path / 'runs'))
    run = res['save_path']
    assert res['steps'] == 4 and all(np.isfinite(v) for v in res['ler_dev'])
    assert '_grudec' in os.path.basename(run) and res['model'].gru_decoder
    assert cg.CALLS['fwd'] >= before['fwd'] + 4 and cg.CALLS['bwd'] == before['bwd'] + 4 and cg.CALLS['infer'] > before['infer']
    from examples.timit.evaluation import eval_attention
    from examples.timit.metrics.attention import do_eval_per
    from examples.timit.training.train_attention import make_datasets
    from tensorflow_end2end_speech_recognition_amd.utils.training.checkpoint import Saver
    model = res['model']
    Saver().save(model, os.path.join(run, 'model.ckpt'), global_step=99)
    map_dir = os.path.join(run, 'mapping_files')
    params = dict(label_type='phone61', splice=1, num_stack=1, num_skip=1, batch_size=8, num_epoch=1, sort_stop_epoch=1,
                  dataset_root=corpus)
    test_data = make_datasets(drv.Dataset, params, map_dir)[2]
    want = do_eval_per(None, None, None, model, test_data, 'phone61', is_test=True, eval_batch_size=1, map_dir=map_dir,
                       is_jointctcatt=family == 'joint')
    got = eval_attention.main([run, '--device', 'cpu'] + (['--joint'] if family == 'joint' else []))
    assert abs(got - want) < 1e-9
