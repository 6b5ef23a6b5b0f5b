"""CPU: scheduled sampling and label smoothing for the attention decoder -- keyword contract, the untouched p = 0 / eps = 0
path, the recipes' ramp and run names, one recipe run, and the host logic of the new path (AttentionSeq2Seq and
JointCTCAttention on the stand-ins of tests/_cpu_ops_att_ss.py) against the float64 statement of the whole loss."""
import os
import sys

import numpy as np
import pytest
import torch

import _cpu_ops_att_ss as ss
from oracle import attention as oatt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _mk(cls, att, D, H, L, U, A, Em, C, **kw):
    return cls(input_size=D, encoder_type='blstm', encoder_num_units=H, encoder_num_layers=L, encoder_num_proj=None,
               attention_type=att, attention_dim=A, decoder_type='lstm', decoder_num_units=U, decoder_num_layers=1,
               embedding_dim=Em, num_classes=C, sos_index=C, eos_index=C + 1, max_decode_length=10, parameter_init=0.1,
               clip_grad_norm=5.0, clip_activation_encoder=50, clip_activation_decoder=50, dtype='f32', seed=5, device='cpu',
               **kw)


def _models():
    from tensorflow_end2end_speech_recognition_amd.models.attention.attention_seq2seq import AttentionSeq2Seq
    from tensorflow_end2end_speech_recognition_amd.models.attention.joint_ctc_attention import JointCTCAttention
    return AttentionSeq2Seq, JointCTCAttention


def test_keyword_contract(monkeypatch):
    ops = ss.install(monkeypatch)
    Att, Joint = _models()
    B, T, D, H, L, U, A, Em, C = 3, 16, 6, 8, 1, 12, 10, 4, 6
    for bad in (-0.1, 1.0, 1.5, float('nan')):
        with pytest.raises(ValueError):
            _mk(Att, 'location', D, H, L, U, A, Em, C, label_smoothing_prob=bad)
        with pytest.raises(ValueError):
            _mk(Joint, 'location', D, H, L, U, A, Em, C, lambda_weight=0.5, label_smoothing_prob=bad)
    assert _mk(Att, 'location', D, H, L, U, A, Em, C).label_smoothing_prob == 0.0
    assert _mk(Joint, 'location', D, H, L, U, A, Em, C, lambda_weight=0.5, label_smoothing_prob=0.25).label_smoothing_prob == 0.25
    x, sl, labels, lsl, ctc = ss.batch(np.random.RandomState(0), B, T, D, C, 4)
    model = _mk(Att, 'location', D, H, L, U, A, Em, C)
    for bad in (-0.01, 1.01, float('nan')):
        with pytest.raises(ValueError):
            model.compute_loss(x, labels, sl, lsl, 1.0, 1.0, 1.0, scheduled_sampling_prob=bad)
    model.compute_loss(x, labels, sl, lsl, 1.0, 1.0, 1.0, scheduled_sampling_prob=1.0)        # 1 is allowed
    # the kernel front end: smoothing outside [0, 1) is refused before anything is launched
    lg = torch.zeros(2, 5)
    for bad in (-0.1, 1.0, float('nan')):
        with pytest.raises(ValueError):
            ops.seq_xent(lg, torch.zeros(2, dtype=torch.int32), torch.ones(2), 1e-10, 1.0, smoothing=bad)
        with pytest.raises(ValueError):
            ops.seq_xent_ls(lg, torch.zeros(2, dtype=torch.int32), torch.ones(2), 1e-10, bad, 1.0)


def test_product_front_end_routes_and_refuses_without_a_device():
    """The real ops (no stand-ins): smoothing is validated on the host, and both new entry points refuse CPU tensors."""
    from tensorflow_end2end_speech_recognition_amd import ops
    lg, tg, w = torch.zeros(2, 5), torch.zeros(2, dtype=torch.int32), torch.ones(2)
    for bad in (-0.1, 1.0, float('nan')):
        with pytest.raises(ValueError):
            ops.seq_xent(lg, tg, w, 1e-10, 1.0, smoothing=bad)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            ops.seq_xent(lg, tg, w, 1e-10, 1.0, smoothing=0.1)
        with pytest.raises(RuntimeError):
            ops.att_decoder_fwd_ss(dict(dec_in=torch.zeros(1, 1, 3), To=1, B=1, U=1, Em=1, E2=1, T=1), torch.zeros(2, 1),
                                   torch.zeros(1, 3), None, torch.zeros(3, 1), torch.zeros(1, 1, dtype=torch.int32),
                                   torch.zeros(1, 1), None)


@pytest.mark.parametrize('joint', [False, True])
def test_zero_probabilities_are_todays_model(monkeypatch, joint):
    """p = 0 and eps = 0: the calls compute_loss has always made (one att_decoder_fwd, seq_xent without a smoothing
    argument, no draw), and the numbers of a model built and called without the new keywords, bit for bit -- also when not
    training, whatever p says; they are the oracle's."""
    ops = ss.install(monkeypatch)
    Att, Joint = _models()
    B, T, D, H, L, U, A, Em, C = 3, 16, 6, 8, 1, 12, 10, 4, 6
    x, sl, labels, lsl, ctc = ss.batch(np.random.RandomState(1), B, T, D, C, 4)
    cls, kw = (Joint, dict(lambda_weight=0.5)) if joint else (Att, {})
    head = (x, labels, ctc, sl, lsl) if joint else (x, labels, sl, lsl)
    log = []
    for name in ('att_decoder_fwd', 'att_decoder_fwd_ss', 'seq_xent', 'seq_xent_ls', 'dropout_mask'):
        def wrap(*a, _f=getattr(ops, name), _n=name, **k):
            log.append((_n, sorted(k)))
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, wrap)
    results = []
    for ctor_kw, call_kw in (({}, {}), (dict(label_smoothing_prob=0.0), dict(scheduled_sampling_prob=0.0))):
        model = _mk(cls, 'location', D, H, L, U, A, Em, C, **kw, **ctor_kw)
        del log[:]
        out = model.compute_loss(*head, 1.0, 0.8, 0.8, **call_kw)
        calls = list(log)
        grads = [g.clone() for g, _ in model._set_optimizer('sgd', 0.1).compute_gradients(out[0], model=model)]
        results.append((out[0].item(), out[1].clone(), grads, calls))
    assert results[0][3] == results[1][3]
    names = [c[0] for c in results[0][3]]
    assert names.count('att_decoder_fwd') == 1 and 'att_decoder_fwd_ss' not in names and 'seq_xent_ls' not in names
    assert names.count('dropout_mask') == 2                               # embedding and decoder masks, no draw
    assert [c for c in results[0][3] if c[0] == 'seq_xent'] == [('seq_xent', ['want_grad'])]
    assert results[0][0] == results[1][0] and torch.equal(results[0][1], results[1][1])
    assert all(torch.equal(a, b) for a, b in zip(results[0][2], results[1][2]))
    # not training: a smoothing model with p > 0 evaluates the plain teacher-forced cross-entropy
    plain = _mk(cls, 'location', D, H, L, U, A, Em, C, **kw)
    smooth = _mk(cls, 'location', D, H, L, U, A, Em, C, label_smoothing_prob=0.3, **kw)
    del log[:]
    a = plain.compute_loss(*head, 1.0, 1.0, 1.0, is_training=False)
    b = smooth.compute_loss(*head, 1.0, 1.0, 1.0, is_training=False, scheduled_sampling_prob=0.7)
    assert a[0].item() == b[0].item() and torch.equal(a[1], b[1])
    assert all(n not in ('att_decoder_fwd_ss', 'seq_xent_ls', 'dropout_mask') for n, _ in log)
    sd = {k: v.numpy().copy() for k, v in plain.store.state_dict().items()}
    ref = oatt.attention_model_forward(sd, x, labels, sl, lsl, L, 'location', clip_enc=50.0, clip_dec=50.0,
                                       ctc_labels=[[int(v) for v in r if v >= 0] for r in ctc] if joint else None,
                                       lambda_weight=0.5 if joint else None)
    assert abs(a[0].item() - ref['total_loss']) / abs(ref['total_loss']) < 1e-5


def test_statement_with_teacher_tokens_is_the_oracle():
    """fed = the labels and eps = 0: the float64 statement is oracle.attention.attention_model_forward, loss and gradients."""
    B, T, D, H, L, U, A, Em, C = 3, 16, 6, 8, 1, 12, 10, 4, 6
    ops_free = _mk(_models()[0], 'hybrid', D, H, L, U, A, Em, C)        # (parameters only: no kernel is called)
    x, sl, labels, lsl, _ = ss.batch(np.random.RandomState(2), B, T, D, C, 4)
    sd = {k: v.numpy().copy() for k, v in ops_free.store.state_dict().items()}
    kw = dict(clip_enc=50.0, clip_dec=50.0, sharpening=1.5, temperature=2.0, prev_alpha='carry')
    ref = oatt.attention_model_forward(sd, x, labels, sl, lsl, L, 'hybrid', **kw)
    To = int(lsl.max()) - 1
    got = ss.ss_model_forward(sd, x, labels, sl, lsl, L, 'hybrid', fed=labels[:, :To], **kw)
    assert abs(got['total_loss'] - ref['total_loss']) < 1e-12 and np.abs(got['logits'] - ref['logits']).max() < 1e-12
    for name, r in ref['grads'].items():
        assert np.abs(got['grads'][name] - r).max() < 1e-12, name
    # the roll-out form with no draw set feeds the labels too; with every draw set it feeds its own argmax where live
    none = ss.ss_model_forward(sd, x, labels, sl, lsl, L, 'hybrid', draw=np.zeros((B, To)), **kw)
    assert np.array_equal(none['fed'], labels[:, :To]) and abs(none['total_loss'] - ref['total_loss']) < 1e-12
    full = ss.ss_model_forward(sd, x, labels, sl, lsl, L, 'hybrid', draw=np.ones((B, To)), **kw)
    live = full['live']
    assert np.array_equal(full['fed'][:, 0], labels[:, 0]) and np.array_equal(full['fed'][~live], labels[:, :To][~live])
    for k in range(1, To):
        assert np.array_equal(full['fed'][live[:, k], k], np.argmax(full['raw_logits'][live[:, k], k - 1], axis=1))
    # smoothing: against torch's own label-smoothed cross-entropy
    sm = ss.ss_model_forward(sd, x, labels, sl, lsl, L, 'hybrid', fed=labels[:, :To], smoothing=0.2, **kw)
    lg = torch.tensor(ref['logits']) + 1e-10
    w = torch.tensor(live, dtype=torch.float64)
    ce = torch.nn.functional.cross_entropy(lg.reshape(B * To, -1), torch.tensor(labels[:, 1:To + 1]).reshape(-1),
                                           reduction='none', label_smoothing=0.2).view(B, To)
    assert abs(sm['sequence_loss'] - float((ce * w).sum() / w.sum())) < 1e-12


def test_smoothed_cross_entropy_stand_in():
    """The stand-in of asr_seq_xent_ls: torch's label-smoothed cross-entropy and its autograd gradient; masked rows are
    exact zeros over NaN logits; eps = 0 is the plain stand-in."""
    import _cpu_ops
    rng = np.random.RandomState(3)
    rows, Cc = 9, 7
    x = torch.tensor(rng.randn(rows, Cc) * 3, dtype=torch.float32)
    tg = torch.tensor(rng.randint(0, Cc, size=rows), dtype=torch.int32)
    w = torch.tensor([1, 0, 1, 1, 0, 1, 1, 0, 1], dtype=torch.float32)
    x[w == 0] = float('nan')
    row, dl = ss._seq_xent_ls(x, tg, w, 1e-10, 0.2, 0.5)
    assert torch.equal(row[w == 0], torch.zeros(3)) and torch.equal(dl[w == 0], torch.zeros(3, Cc))
    x64 = torch.nan_to_num(x.double()).requires_grad_(True)
    ce = torch.nn.functional.cross_entropy(x64 + 1e-10, tg.long(), reduction='none', label_smoothing=0.2) * w.double()
    (ce.sum() * 0.5).backward()
    assert np.abs(row.numpy() - ce.detach().numpy()).max() < 1e-6 and np.abs(dl.numpy() - x64.grad.numpy()).max() < 1e-7
    x0 = torch.nan_to_num(x)
    a, b = ss._seq_xent_ls(x0, tg, w, 1e-10, 0.0, 0.5), _cpu_ops._seq_xent(x0, tg, w, 1e-10, 0.5)
    assert (a[0] - b[0]).abs().max() < 1e-6 and (a[1] - b[1]).abs().max() < 1e-7


def test_recipe_ramp_and_run_name():
    from examples.timit.training.train_attention import model_kwargs, run_name, scheduled_sampling_prob
    import yaml
    with open(os.path.join(ROOT, 'examples/timit/config/attention/blstm_attention_phone61_ss_ls.yml')) as f:
        params = yaml.safe_load(f)['param']
    assert params['scheduled_sampling_prob'] == 0.2 and params['scheduled_sampling_ramp_max_step'] == 4000
    assert params['label_smoothing_prob'] == 0.2
    ramp = 4000
    got = [scheduled_sampling_prob(params, s) for s in (0, ramp // 2, ramp, 2 * ramp)]
    assert got == [0.0, 0.1, 0.2, 0.2]
    no_ramp = {k: v for k, v in params.items() if k != 'scheduled_sampling_ramp_max_step'}
    assert [scheduled_sampling_prob(no_ramp, s) for s in (0, 1, 10 ** 6)] == [0.2, 0.2, 0.2]
    with open(os.path.join(ROOT, 'examples/timit/config/attention/blstm_attention_phone61.yml')) as f:
        base = yaml.safe_load(f)['param']
    assert [scheduled_sampling_prob(base, s) for s in (0, 5000)] == [0.0, 0.0]
    assert run_name(params) == run_name(base) + '_ss0.2_ls0.2'
    assert run_name(dict(base, label_smoothing_prob=0.1)) == run_name(base) + '_ls0.1'
    assert run_name(dict(base, scheduled_sampling_prob=0.3, label_smoothing_prob=0)) == run_name(base) + '_ss0.3'
    kw = model_kwargs(dict(params, num_classes=61))
    assert kw['label_smoothing_prob'] == 0.2 and model_kwargs(dict(base, num_classes=61))['label_smoothing_prob'] == 0.0


def test_timit_attention_recipe_with_both_keys(monkeypatch, tmp_path):
    """examples/timit/training/train_attention.py on the synthetic corpus with scheduled sampling (ramped) and label
    smoothing: the training steps go through the new loop with the ramp's probabilities, the dev loss through the old."""
    import test_host_logic as thl
    ops = ss.install(monkeypatch)
    corpus = str(tmp_path / 'corpus')
    thl._make_timit_like(corpus, np.random.RandomState(0), n_train=16, n_dev=4, n_test=3, multitask=False)
    from examples.timit.training import train_attention as drv
    cfg = thl._recipe_cfg(ROOT, 'examples/timit/config/attention/blstm_attention_phone61_ss_ls.yml', tmp_path,
                          encoder_num_units=8, encoder_num_layers=1, attention_dim=6, decoder_num_units=8, embedding_dim=4,
                          max_decode_length=10, dropout_encoder=0.0, dropout_decoder=0.1, dropout_embedding=0.1,
                          scheduled_sampling_prob=0.5, scheduled_sampling_ramp_max_step=4, label_smoothing_prob=0.1,
                          input_size=6, batch_size=8, num_epoch=3, eval_start_epoch=1, print_step=2, optimizer='adam',
                          learning_rate=0.02, weight_decay=0, decay_start_epoch=2, dtype='f32', device='cpu',
                          dataset_root=corpus, sort_stop_epoch=2)
    seen = dict(ss=[], plain=0, ls=[])
    real_ss, real_fwd, real_xent = ops.att_decoder_fwd_ss, ops.att_decoder_fwd, ops.seq_xent

    def spy_ss(a, W_av, W_out, b_out, embedding, teacher_ids, draw, emb_mask):
        seen['ss'].append(float((draw != 0).float().mean()))
        return real_ss(a, W_av, W_out, b_out, embedding, teacher_ids, draw, emb_mask)

    def spy_fwd(a):
        seen['plain'] += 1
        return real_fwd(a)

    def spy_xent(*a, **k):
        seen['ls'].append(k.get('smoothing', 0.0))
        return real_xent(*a, **k)
    monkeypatch.setattr(ops, 'att_decoder_fwd_ss', spy_ss)
    monkeypatch.setattr(ops, 'att_decoder_fwd', spy_fwd)
    monkeypatch.setattr(ops, 'seq_xent', spy_xent)
    probs = []
    real_loss = drv.AttentionSeq2Seq.compute_loss

    def spy_loss(self, *a, **k):
        if k.get('is_training', True):
            probs.append(k.get('scheduled_sampling_prob', 0.0))
        return real_loss(self, *a, **k)
    monkeypatch.setattr(drv.AttentionSeq2Seq, 'compute_loss', spy_loss)
    res = drv.main(cfg, str(tmp_path / 'runs'))
    assert res['steps'] == 6 and probs == [0.0, 0.125, 0.25, 0.375, 0.5, 0.5]
    assert len(seen['ss']) == 5 and seen['plain'] >= 1                     # step 0 (p = 0) and every dev loss: the old loop
    assert seen['ls'].count(0.1) == 6 and set(seen['ls']) == {0.0, 0.1}
    assert res['save_path'].endswith('_ss0.5_ls0.1') and res['model'].label_smoothing_prob == 0.1
    assert all(np.isfinite(v) for v in res['ler_dev'])


@pytest.mark.parametrize('att,joint,prev', [('location', False, 'zeros'), ('luong_dot', False, 'zeros'),
                                            ('hybrid', False, 'carry'), ('location', True, 'zeros')])
def test_model_host_logic_against_the_statement(monkeypatch, att, joint, prev):
    """p = 0.5, eps = 0.1, decoder and embedding dropout on, on the stand-ins: loss, logits and every gradient against the
    float64 statement fed the step's draws, masks and fed ids (bars of test_host_logic's attention parity); the fed ids are
    the statement's own argmax wherever its margin exceeds 10 x the logits bar, the labels wherever nothing was sampled;
    the embedding gradient lands on the fed rows."""
    ops = ss.install(monkeypatch)
    Att, Joint = _models()
    B, T, D, H, L, A, Em, C = 4, 18, 6, 8, 1, 10, 4, 6
    U = 2 * H if att == 'luong_dot' else 12
    x, sl, labels, lsl, ctc = ss.batch(np.random.RandomState(11), B, T, D, C, 7)
    kw = dict(sharpening_factor=1.5, logits_temperature=2.0, prev_alpha=prev, label_smoothing_prob=0.1)
    if joint:
        model = _mk(Joint, att, D, H, L, U, A, Em, C, lambda_weight=0.5, honour_ctor_args=True, **kw)
    else:
        model = _mk(Att, att, D, H, L, U, A, Em, C, **kw)
    r = ss.model_step_against_statement(monkeypatch, ops, model, x, labels, sl, lsl, L, att, 0.5, (1.0, 0.8, 0.8), 1e-4,
                                        ctc_labels=ctc if joint else None, clip_enc=50.0, clip_dec=50.0, sharpening=1.5,
                                        temperature=2.0, prev_alpha=prev)
    print('loss rel %.2e  logits abs %.2e  sampled %d  excluded %d  wrong %d' %
          (r['loss_rel'], r['logits_abs'], r['n_sampled'], r['n_excluded'], r['n_wrong']))
    assert r['loss_rel'] < 1e-5 and r['logits_abs'] < 1e-5
    assert r['n_sampled'] >= 4 and r['n_wrong'] == 0 and r['teacher_ok'] and r['n_excluded'] <= 0.1 * r['n_sampled']
    assert (r['fed'] != labels[:, :r['fed'].shape[1]]).any()              # something other than the label was fed
    for name, (err, mag) in r['grads'].items():
        assert err < 1e-4 * max(mag, 1e-3) + 1e-7, (name, err, mag)
    # the embedding gradient lands on what was fed: a class that was fed and is no label of the batch has a non-zero row
    only_fed = sorted(set(r['fed'].ravel().tolist()) - set(labels[:, :r['fed'].shape[1]].ravel().tolist()))
    demb = dict((n, g) for g, n in r['gv'])['output_embedding/W_embedding']
    for c in only_fed:
        assert demb[c].abs().max() > 0, c
