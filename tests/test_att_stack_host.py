"""CPU: the multi-layer LSTM decoder of the attention models (decoder_num_layers > 1) -- variables, bridge split, rng stream,
mask draws, every refusal, the recipe, a checkpoint round trip, and the host logic of AttentionSeq2Seq / JointCTCAttention on
the stand-ins of tests/_cpu_ops_att_stack.py against the float64 statement of tests/_att_stack_oracle.py (loss, logits,
every gradient, greedy and beam decode)."""
import os
import sys

import numpy as np
import pytest
import torch

import _att_stack_oracle as so
import _cpu_ops_att_stack as cs
from test_att_gru_host import _LSTM_DIGESTS, _batch, _digest, _models

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

D = 'attention_decoder/decoder/'


def _mk(cls, att, Din, H, L, U, A, Em, C, layers, **kw):
    kw.setdefault('max_decode_length', 10)
    kw.setdefault('seed', 5)
    kw.setdefault('decoder_type', 'lstm')
    return cls(input_size=Din, encoder_type='blstm', encoder_num_units=H, encoder_num_layers=L, encoder_num_proj=None,
               attention_type=att, attention_dim=A, decoder_num_units=U, decoder_num_layers=layers,
               embedding_dim=Em, num_classes=C, sos_index=C, eos_index=C + 1, parameter_init=0.1, clip_grad_norm=5.0,
               clip_activation_encoder=50, clip_activation_decoder=50, dtype='f32', device='cpu', **kw)


@pytest.mark.parametrize('peep', [True, False])
def test_variables_and_creation_order(monkeypatch, peep):
    cs.install(monkeypatch)
    Att, _ = _models()
    Din, H, L, U, A, Em, C = 6, 8, 1, 12, 10, 4, 6
    sds = {n: _mk(Att, 'location', Din, H, L, U, A, Em, C, n, use_peephole=peep).store.state_dict() for n in (1, 2, 3)}
    per_cell = ['kernel', 'bias'] + (['w_i_diag', 'w_f_diag', 'w_o_diag'] if peep else [])
    base = list(sds[1])
    for n in (1, 2, 3):
        sd, names = sds[n], list(sds[n])
        assert tuple(sd['bridge/fully_connected/weights'].shape) == (4 * H, 2 * U * n)
        assert tuple(sd['bridge/fully_connected/biases'].shape) == (2 * U * n,)
        upper = [D + 'lstm_cell_%d/%s' % (l, v) for l in range(1, n) for v in per_cell]
        # the new variables stand directly behind layer 0's; everything else is the one-layer model's sequence
        i = names.index(D + 'lstm_cell/' + per_cell[-1]) + 1
        assert names[i:i + len(upper)] == upper
        assert names[:i] + names[i + len(upper):] == base
        assert not any(k.startswith(D + 'lstm_cell_%d/' % n) for k in names)
        for l in range(1, n):
            cell = D + 'lstm_cell_%d/' % l
            assert tuple(sd[cell + 'kernel'].shape) == (2 * U, 4 * U) and tuple(sd[cell + 'bias'].shape) == (4 * U,)
            assert float(sd[cell + 'bias'].abs().max()) == 0.0
            assert float(sd[cell + 'kernel'].abs().max()) <= 0.1 and float(sd[cell + 'kernel'].std()) > 0.03
            for v in per_cell[2:]:
                assert tuple(sd[cell + v].shape) == (U,) and float(sd[cell + v].abs().max()) <= 0.1
        # everything drawn before the bridge is the same stream at every depth
        for k in names[:names.index('bridge/fully_connected/weights')]:
            assert torch.equal(sd[k], sds[1][k]), k


def test_one_layer_model_is_the_model_of_before(monkeypatch):
    """sha256 over (name, fp32 bytes) of every variable of two one-layer models, taken on the commit before the GRU decoder
    existed (tests/test_att_gru_host.py): names, shapes and values of decoder_num_layers = 1 are what they were."""
    cs.install(monkeypatch)
    Att, Joint = _models()
    Din, H, L, U, A, Em, C = 6, 8, 2, 12, 10, 4, 6
    m = _mk(Att, 'location', Din, H, L, U, A, Em, C, 1)
    assert _digest(m) == _LSTM_DIGESTS['location']
    assert m.decoder_num_layers == 1 == m.decdoder_num_layers
    assert _digest(_mk(Joint, 'hybrid', Din, H, L, U, A, Em, C, 1, lambda_weight=0.3,
                       prev_alpha='carry')) == _LSTM_DIGESTS['joint']
    m3 = _mk(Att, 'location', Din, H, L, U, A, Em, C, 3)
    assert m3.decoder_num_layers == 3 == m3.decdoder_num_layers


def test_bridge_width_and_split_order(monkeypatch):
    cs.install(monkeypatch)
    Att, _ = _models()
    Din, H, L, U, A, Em, C, B = 6, 8, 1, 12, 10, 4, 6, 5
    model = _mk(Att, 'location', Din, H, L, U, A, Em, C, 3)
    rng = np.random.RandomState(3)
    cf, hf = torch.tensor(rng.randn(2, B, H), dtype=torch.float32), torch.tensor(rng.randn(2, B, H), dtype=torch.float32)
    bi, c0, h0 = model._bridge(cf, hf, B)
    assert torch.equal(bi, torch.cat([cf[0], hf[0], cf[1], hf[1]], 1))
    st = model.store
    init = bi.double() @ st['bridge/fully_connected/weights'].double() + st['bridge/fully_connected/biases'].double()
    flat = [c0, h0] + [t for ch in model._init_up for t in ch]              # c_0, h_0, c_1, h_1, c_2, h_2
    assert len(flat) == 6
    for i, t in enumerate(flat):
        assert tuple(t.shape) == (B, U)
        assert float((t.double() - init[:, i * U:(i + 1) * U]).abs().max()) < 1e-5, i


@pytest.mark.parametrize('layers,calls', [(1, 2), (2, 3), (3, 3)])
def test_mask_draws(monkeypatch, layers, calls):
    """decoder_num_layers = 1 draws what it always drew (embedding mask, decoder mask: two increments of _calls); L > 1 adds
    ONE draw [(L-1),To,Bp,U] with a further increment, made only with dropout on."""
    import _cpu_ops_att_ss as ss
    ops = cs.install(monkeypatch)
    Att, _ = _models()
    B, T, Din, H, L, U, A, Em, C = 3, 16, 6, 8, 1, 12, 10, 4, 6
    x, sl, labels, lsl, _ = _batch(np.random.RandomState(0), B, T, Din, C, [4, 2, 3])
    model = _mk(Att, 'location', Din, H, L, U, A, Em, C, layers)
    masks = ss.spy_dropout_masks(monkeypatch, ops)
    model.compute_loss(x, labels, sl, lsl, 1.0, 0.8, 0.8)
    assert model._calls == calls and len(masks) == calls
    To = 5                                   # label lengths 4 / 2 / 3: <SOS> y <EOS> gives max + 1 decoder steps
    Bp = masks[1][0][1]
    assert masks[0][2] == model.seed + 1 and masks[0][3] == 1 << 40
    assert masks[1][0] == (To, Bp, U) and masks[1][2] == model.seed + 2 and masks[1][3] == 2 << 40
    if layers > 1:
        assert masks[2][0] == (layers - 1, To, Bp, U) and masks[2][2] == model.seed + 2 and masks[2][3] == 3 << 40
    del masks[:]
    model.compute_loss(x, labels, sl, lsl, 1.0, 1.0, 1.0)
    assert model._calls == calls and not masks                               # no dropout: no draw at any depth


def test_refusals(monkeypatch):
    cs.install(monkeypatch)
    Att, Joint = _models()
    B, T, Din, H, L, U, A, Em, C = 3, 16, 6, 8, 1, 12, 10, 4, 6
    for bad in (0, -1, 9, 1.5):
        with pytest.raises(ValueError, match='decoder_num_layers'):
            _mk(Att, 'location', Din, H, L, U, A, Em, C, bad)
    _mk(Att, 'location', Din, H, L, U, A, Em, C, 8)
    with pytest.raises(ValueError, match='decoder_num_layers > 1.*decoder_type="gru"'):
        _mk(Att, 'location', Din, H, L, U, A, Em, C, 2, decoder_type='gru')
    x, sl, labels, lsl, ctc = _batch(np.random.RandomState(0), B, T, Din, C, [4, 2, 3])
    model = _mk(Att, 'location', Din, H, L, U, A, Em, C, 2)
    with pytest.raises(ValueError, match='scheduled_sampling_prob.*decoder_num_layers > 1'):
        model.compute_loss(x, labels, sl, lsl, 1.0, 1.0, 1.0, scheduled_sampling_prob=0.3)
    joint = _mk(Joint, 'location', Din, H, L, U, A, Em, C, 2, lambda_weight=0.5)
    with pytest.raises(ValueError, match='ctc_weight.*decoder_num_layers > 1'):
        joint.infer(x, sl, beam_width=2, ctc_weight=0.3)
    for kw in (dict(lm=object()), dict(lm_weight=0.3), dict(lm=object(), lm_weight=0.3)):
        with pytest.raises(ValueError, match='decoder_num_layers > 1'):
            model.infer(x, sl, beam_width=2, **kw)
    model.compute_loss(x, labels, sl, lsl, 1.0, 1.0, 1.0, scheduled_sampling_prob=0.0)


@pytest.mark.parametrize('att,joint,prev,layers,peep', [('location', False, 'carry', 2, True),
                                                        ('luong_dot', False, 'zeros', 2, True),
                                                        ('bahdanau_content', True, 'zeros', 2, True),
                                                        ('location', False, 'zeros', 3, False)])
def test_model_host_logic_against_the_statement(monkeypatch, att, joint, prev, layers, peep):
    """One training step with decoder and embedding dropout on the stand-ins: loss, logits and every gradient against the
    float64 statement fed the step's masks, at the plain attention model's bars (loss 1e-4 relative, logits 2e-4, gradients
    2e-3 of their largest entry).  Label lengths 1 / 5 / 3 / 5: a row finishes at step 1, two at the last step -- the
    host-side recursion (every layer's dc0 / dh0 into the [4H, 2UL] bridge, the upper layers' weight, bias and peephole
    gradients batched over the steps) against autograd.  Greedy infer (native and class surface) and
    infer(beam_width=...) run through the stack loops and equal the statement's decode."""
    import _cpu_ops_att_ss as ss
    from tensorflow_end2end_speech_recognition_amd.utils.io.labels.sparsetensor import list2sparsetensor
    ops = cs.install(monkeypatch)
    Att, Joint = _models()
    B, T, Din, H, L, A, Em, C = 4, 18, 6, 8, 1, 10, 4, 6
    U = 2 * H if att == 'luong_dot' else 12
    x, sl, labels, lsl, ctc = _batch(np.random.RandomState(11), B, T, Din, C, [1, 5, 3, 5])
    kw = dict(sharpening_factor=1.5, logits_temperature=2.0, prev_alpha=prev, use_peephole=peep)
    model = _mk(Joint, att, Din, H, L, U, A, Em, C, layers, lambda_weight=0.5, honour_ctor_args=True, **kw) if joint else \
        _mk(Att, att, Din, H, L, U, A, Em, C, layers, **kw)
    masks = ss.spy_dropout_masks(monkeypatch, ops)
    before = dict(cs.CALLS)
    if joint:
        loss, logits, _, otr, _ = model.compute_loss(x, labels, list2sparsetensor(ctc, -1), sl, lsl, 1.0, 0.8, 0.8)
    else:
        loss, logits, otr, _ = model.compute_loss(x, labels, sl, lsl, 1.0, 0.8, 0.8)
    demb = [m for m in masks if m[2] == model.seed + 1][0][4][:, :B].transpose(0, 1).numpy()
    d0 = [m for m in masks if m[2] == model.seed + 2 and len(m[0]) == 3][0][4]
    dup = [m for m in masks if m[2] == model.seed + 2 and len(m[0]) == 4][0][4]
    ddec = torch.cat([d0.unsqueeze(0), dup], 0)[:, :, :B].numpy()             # [L,To,B,U]
    sd = {k: v.numpy().copy() for k, v in model.store.state_dict().items()}
    ref = so.stack_model_forward(sd, x, labels, sl, lsl, L, att, clip_enc=50.0, clip_dec=50.0, sharpening=1.5,
                                 temperature=2.0, drop_emb=demb, drop_dec=ddec, prev_alpha=prev,
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
    for l in range(1, layers):
        for v in ['kernel', 'bias'] + (['w_i_diag', 'w_f_diag', 'w_o_diag'] if peep else []):
            name = D + 'lstm_cell_%d/%s' % (l, v)
            assert name in names and np.abs(ref['grads'][name]).max() > 0, name
    gb = ref['grads']['bridge/fully_connected/weights']
    for i in range(2 * layers):                                             # every layer's c0 and h0 columns see a gradient
        assert np.abs(gb[:, i * U:(i + 1) * U]).max() > 0, i
    assert cs.CALLS['fwd'] == before['fwd'] + 1 and cs.CALLS['bwd'] == before['bwd'] + 1
    # decoding (the output layer's weights times 40, as tests/test_gpu_att_beam.py does: at parameter_init = 0.1 the logits
    # of an untrained model are too flat for any margin)
    tsd = {k: v.clone() for k, v in model.store.state_dict().items()}
    tsd[D + 'output_layer/weights'] *= 40.0
    tsd[D + 'output_layer/biases'][C + 1] = 0.35
    model.store.load_state_dict(tsd)
    sd = {k: v.numpy().copy() for k, v in tsd.items()}
    ids, margin, lmax = so.stack_model_infer(sd, x, sl, L, att, C, C + 1, 10, clip_enc=50.0, clip_dec=50.0, sharpening=1.5,
                                             prev_alpha=prev)
    got = model.infer(x, sl)
    assert cs.CALLS['infer'] == before['infer'] + 1
    sure = margin > 10 * 2e-4
    n = min(got.shape[1], ids.shape[1])
    assert sure.mean() >= 0.9 and (got.shape[1] == ids.shape[1] or not sure.all())
    assert np.array_equal(got[:, :n][sure[:, :n]], ids[:, :n][sure[:, :n]])
    surf = model.infer(x, sl, native=False)                                    # AttentionDecoder.step over the stacked cell
    m = min(surf.shape[1], n)
    assert np.array_equal(surf[:, :m][sure[:, :m]], ids[:, :m][sure[:, :m]])
    one = model._decode_beam(ops.to_device(x, torch.float32, model.device), ops.to_device(sl, torch.int32, model.device), 1)
    assert cs.CALLS['beam'] == before['beam'] + 1
    from tensorflow_end2end_speech_recognition_amd.models.attention.decoders.beam_search.beam_search_decoder import cut_at_eos
    if sure.all():
        for b in range(B):
            assert cut_at_eos(one[b], C + 1) == cut_at_eos(got[b], C + 1), b
    want = so.stack_beam_infer(sd, x, sl, L, att, C, C + 1, 10, 3, 0.6, clip_enc=50.0, clip_dec=50.0, sharpening=1.5,
                               prev_alpha=prev)
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


def test_one_layer_models_never_reach_the_stack_loops(monkeypatch):
    ops = cs.install(monkeypatch)
    Att, _ = _models()
    B, T, Din, H, L, U, A, Em, C = 3, 16, 6, 8, 1, 12, 10, 4, 6
    x, sl, labels, lsl, _ = _batch(np.random.RandomState(1), B, T, Din, C, [4, 2, 3])
    model = _mk(Att, 'location', Din, H, L, U, A, Em, C, 1)
    before = dict(cs.CALLS)
    seen = []
    for name in ('att_decoder_fwd', 'att_decoder_bwd', 'att_decoder_infer', 'att_decoder_beam'):
        def wrap(a, *p, _f=getattr(ops, name), **k):
            seen.append('stack' in a)
            return _f(a, *p, **k)
        monkeypatch.setattr(ops, name, wrap)
    loss, *_ = model.compute_loss(x, labels, sl, lsl, 1.0, 0.8, 0.8)
    model._set_optimizer('sgd', 0.1).compute_gradients(loss, model=model)
    model.infer(x, sl)
    model.infer(x, sl, beam_width=2)
    assert cs.CALLS == before and seen == [False] * 4


def test_checkpoint_round_trip(monkeypatch, tmp_path):
    from tensorflow_end2end_speech_recognition_amd.utils.training.checkpoint import Saver
    cs.install(monkeypatch)
    Att, _ = _models()
    B, T, Din, H, L, U, A, Em, C = 3, 16, 6, 8, 1, 12, 10, 4, 6
    x, sl, labels, lsl, _ = _batch(np.random.RandomState(2), B, T, Din, C, [4, 2, 3])
    a = _mk(Att, 'location', Din, H, L, U, A, Em, C, 2, seed=5)
    loss, *_ = a.compute_loss(x, labels, sl, lsl, 1.0, 1.0, 1.0)
    a.train(loss, 'momentum', 0.05)
    Saver().save(a, str(tmp_path / 'model.ckpt'), global_step=7)
    b = _mk(Att, 'location', Din, H, L, U, A, Em, C, 2, seed=6)
    Saver().restore(b, str(tmp_path / 'model.ckpt-7'))
    sa, sb = a.store.state_dict(), b.store.state_dict()
    assert list(sa) == list(sb) and D + 'lstm_cell_1/kernel' in sa
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert np.array_equal(a.infer(x, sl), b.infer(x, sl))
    one = _mk(Att, 'location', Din, H, L, U, A, Em, C, 1)
    with pytest.raises(Exception):                                             # a two-layer checkpoint is not a one-layer model's
        Saver().restore(one, str(tmp_path / 'model.ckpt-7'))


def test_recipe_builds_a_two_layer_decoder(monkeypatch):
    import yaml
    from examples.timit.training.train_attention import model_kwargs, run_name
    cs.install(monkeypatch)
    Att, _ = _models()
    with open(os.path.join(ROOT, 'examples/timit/config/attention/blstm_attention_phone61_2layer_decoder.yml')) as f:
        params = yaml.safe_load(f)['param']
    with open(os.path.join(ROOT, 'examples/timit/config/attention/blstm_attention_phone61.yml')) as f:
        base = yaml.safe_load(f)['param']
    assert params == dict(base, decoder_num_layers=2)
    assert '_de256_2' in run_name(params) and '_de256_1' in run_name(base)
    kw = model_kwargs(dict(params, num_classes=61, encoder_num_units=8, encoder_num_layers=1, decoder_num_units=8,
                           attention_dim=6, embedding_dim=4, input_size=6))
    assert kw['decoder_num_layers'] == 2
    kw.update(device='cpu', dtype='f32')
    model = Att(**kw)
    sd = model.store.state_dict()
    assert tuple(sd[D + 'lstm_cell_1/kernel'].shape) == (16, 32)
    assert tuple(sd['bridge/fully_connected/weights'].shape) == (32, 32)


@pytest.mark.parametrize('family', ['attention', 'joint'])
def test_timit_recipe_with_a_two_layer_decoder(monkeypatch, tmp_path, family):
    """examples/timit/training/train_{attention,joint_ctc_attention}.py on the synthetic corpus with the two-layer recipe:
    training steps and dev decodes go through the stack loops, and eval_attention.py rebuilds the model from the run's
    config.yml (decoder_num_layers reaches the constructor), restores a checkpoint and scores what the trained object
    scores."""
    import test_host_logic as thl
    cs.install(monkeypatch)
    corpus = str(tmp_path / 'corpus')
    thl._make_timit_like(corpus, np.random.RandomState(0), n_train=16, n_dev=4, n_test=3, multitask=False)
    from examples.timit.training import train_attention, train_joint_ctc_attention
    drv = train_attention if family == 'attention' else train_joint_ctc_attention
    cfg = thl._recipe_cfg(ROOT, 'examples/timit/config/attention/blstm_attention_phone61_2layer_decoder.yml', tmp_path,
                          encoder_num_units=8, encoder_num_layers=1, attention_dim=6, decoder_num_units=8, embedding_dim=4,
                          max_decode_length=10, dropout_encoder=0.0, dropout_decoder=0.1, dropout_embedding=0.1,
                          input_size=6, batch_size=8, num_epoch=2, eval_start_epoch=1, print_step=2, optimizer='adam',
                          learning_rate=0.02, weight_decay=0, decay_start_epoch=2, dtype='f32', device='cpu',
                          dataset_root=corpus, sort_stop_epoch=2)
    before = dict(cs.CALLS)
    res = drv.main(cfg, str(tmp_path / 'runs'))
    run = res['save_path']
    assert res['steps'] == 4 and all(np.isfinite(v) for v in res['ler_dev'])
    assert '_de8_2' in os.path.basename(run) and res['model'].decoder_num_layers == 2
    assert cs.CALLS['fwd'] >= before['fwd'] + 4 and cs.CALLS['bwd'] == before['bwd'] + 4 and cs.CALLS['infer'] > before['infer']
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
