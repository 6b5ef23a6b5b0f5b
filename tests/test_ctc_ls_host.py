"""Label smoothing for the CTC heads (label_smoothing_prob / ctc_label_smoothing_prob, an extension) on the host: the
float64 statement (tests/_ctc_ls_oracle.py) against central differences of its own loss, and CTC / MultitaskCTC /
JointCTCAttention on the CPU stand-ins (tests/_cpu_ops_ctc_ls.py) against that statement composed with the model
statements of oracle.model / oracle.attention; the keyword contract and the TIMIT recipes."""
import os
import random
import sys

import numpy as np
import pytest
import torch

import _cpu_ops_ctc_ls as cls_ops
import _ctc_ls_oracle as ols
import test_host_logic as thl
from oracle import attention as oatt
from oracle import ctc as octc
from oracle import model as omodel
from oracle import optim as oopt

EPS = 0.2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def edge_case(rng=None):
    """The lengths and labels of test_gpu_ops.py::test_ctc_edge_cases: an empty row, an exact-fit row, an infeasible row,
    a zero-length row."""
    rng = rng or np.random.RandomState(0)
    T, B, C = 12, 5, 7
    logits = rng.randn(T, B, C).astype(np.float32)
    sl = np.array([12, 5, 3, 0, 7], dtype=np.int32)
    labs = [[], [1, 1, 1], [2, 2, 2], [3], [0, 1, 2, 3, 4, 5, 0]]
    return logits, sl, labs


# ---------------------------------------------------------------- the statement
@pytest.mark.parametrize('eps', [0.1, 0.5])
def test_statement_gradient_equals_central_differences_of_its_loss(eps):
    logits, sl, labs = edge_case()
    x = logits.astype(np.float64)
    r = ols.ctc_ls_batch(x, labs, sl, eps)
    assert r['ctc'][2] == 0 and r['kl'][2] == 0 and not r['grad'][:, 2].any()      # infeasible
    assert r['ctc'][3] == 0 and r['kl'][3] == 0 and not r['grad'][:, 3].any()      # seq_len 0
    assert r['kl'][0] > 0 and r['ctc'][0] > 0                                     # the empty label row is smoothed
    for b in range(5):
        assert not r['grad'][int(sl[b]):, b].any()
    h = 1e-6
    fd = np.zeros_like(x)
    for idx in np.ndindex(*x.shape):
        xp, xm = x.copy(), x.copy()
        xp[idx] += h
        xm[idx] -= h
        fd[idx] = (ols.ctc_ls_batch(xp, labs, sl, eps)['total'].sum() - ols.ctc_ls_batch(xm, labs, sl, eps)['total'].sum()) \
            / (2 * h)
    err = np.abs(fd - r['grad']).max()
    print('central differences: max error %.3g' % err)
    assert err < 1e-7
    # the formula of the issue, from the plain occupation: p - (1 - eps) occ - eps / C on the frames of feasible rows
    _, g_plain = octc.ctc_loss_batch(x, labs, sl)
    p = np.exp(octc.log_softmax(x))
    for b in (0, 1, 4):
        n = int(sl[b])
        occ = p[:n, b] - g_plain[:n, b]
        assert np.abs(r['grad'][:n, b] - (p[:n, b] - (1 - eps) * occ - eps / 7)).max() < 1e-14


def test_kl_is_nonnegative_and_zero_for_constant_rows():
    rng = np.random.RandomState(1)
    T, B, C = 9, 4, 11
    x = rng.randn(T, B, C) * 3
    sl = np.array([9, 4, 7, 1])
    labs = [[1], [], [2, 2], [0]]
    kl, g = ols.kl_uniform(x, labs, sl)
    assert (kl > 0).all()
    x[:, 1] = 0.75                                     # constant rows: softmax is uniform
    x[:, 3] = -3.0
    kl, g = ols.kl_uniform(x, labs, sl)
    assert abs(kl[1]) < 1e-12 and abs(kl[3]) < 1e-12 and kl[0] > 0 and kl[2] > 0
    assert np.abs(g[:, 1]).max() < 1e-15
    # each row term against the definition sum_k (1/C) ln((1/C) / p_k)
    p = np.exp(octc.log_softmax(x[:9, 0]))
    assert abs(kl[0] - (np.log(1.0 / C / p) / C).sum()) < 1e-12


def test_stand_in_equals_the_statement_and_checks_its_arguments(monkeypatch):
    ops = cls_ops.install(monkeypatch)
    logits, sl, labs = edge_case()
    flat = torch.tensor(sum(labs, []), dtype=torch.int32)
    off = torch.tensor(np.concatenate([[0], np.cumsum([len(l) for l in labs])]), dtype=torch.int32)
    args = (torch.tensor(logits), flat, off, torch.tensor(sl), 7)
    r = ols.ctc_ls_batch(logits, labs, sl, 0.3)
    loss, kl, grad, img, ninf = ops.ctc_loss_ls(*args, 0.3, grad_scale=0.5, want_image=True)
    assert np.abs(loss.numpy() - r['ctc']).max() < 1e-6 and np.abs(kl.numpy() - r['kl']).max() < 1e-6
    assert np.abs(grad.numpy() - 0.5 * r['grad']).max() < 1e-7
    assert img.shape == (60, 64) and not img[:, 7:].any() and torch.equal(img[:, :7], grad.view(60, 7).to(torch.bfloat16))
    plain, _, _ = ops.ctc_loss(*args)
    assert torch.equal(plain, loss)
    _, kl2, g2, i2, _ = ops.ctc_loss_ls(*args, 0.3, want_grad=False)
    assert g2 is None and i2 is None and torch.equal(kl, kl2)
    assert ops.ctc_ls_counts() == dict(calls=2, lse_done=0, no_grad=1)
    ops.reset_ctc_ls_counts()
    assert ops.ctc_ls_counts() == dict(calls=0, lse_done=0, no_grad=0)
    for bad in (0.0, 1.0, -0.1, 1.5, float('nan')):
        with pytest.raises(ValueError):
            ops.ctc_loss_ls(*args, bad)
    with pytest.raises(ValueError):
        ops.ctc_loss_ls(*args, 0.3, lse_done=True)


def test_ops_front_end_checks_before_any_device_call():
    """The real ops.ctc_loss_ls refuses eps outside (0, 1) and lse_done without a workspace before it touches a handle."""
    from tensorflow_end2end_speech_recognition_amd import ops
    x = torch.zeros(3, 2, 4)
    i = torch.zeros(3, dtype=torch.int32)
    for bad in (0.0, 1.0, -0.5, 2.0, float('nan')):
        with pytest.raises(ValueError):
            ops.ctc_loss_ls(x, i, i, i[:2], 1, bad)
    with pytest.raises(ValueError):
        ops.ctc_loss_ls(x, i, i, i[:2], 1, 0.2, want_grad=False, want_image=True)


# ---------------------------------------------------------------- CTC
def _ctc(enc, D, H, L, C, **kw):
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    return CTC(encoder_type=enc, input_size=D, num_units=H, num_layers=L, num_classes=C, parameter_init=0.1,
               clip_grad_norm=0.05, clip_activation=50, dtype='f32', seed=3, device='cpu', **kw)


def _randomise_biases(model, rng):
    sd = {k: v.numpy().copy() for k, v in model.store.state_dict().items()}
    for k in sd:
        if k.endswith('/bias') or k.endswith('/biases'):
            sd[k] = (rng.randn(*sd[k].shape) * 0.05).astype(np.float32)
    model.store.load_state_dict({k: torch.tensor(v) for k, v in sd.items()})
    return sd


@pytest.mark.parametrize('enc,wd,temp', [('blstm', 0.0, 1), ('lstm', 0.0, 1), ('blstm', 1e-3, 2)])
def test_ctc_model_host_logic_with_label_smoothing(monkeypatch, enc, wd, temp):
    cls_ops.install(monkeypatch)
    rng = np.random.RandomState(5)
    B, T, D, H, L, C = 5, 11, 6, 8, 2, 6
    x, sl, labs, dense = thl._batch(rng, B, T, D, C)
    model = _ctc(enc, D, H, L, C, label_smoothing_prob=EPS, weight_decay=wd)
    assert model.label_smoothing_prob == EPS
    sd = _randomise_biases(model, rng)
    okw = dict(ndir=2 if enc == 'blstm' else 1, cell_clip=50.0, weight_decay=wd, temperature=float(temp))
    with ols.patched(EPS):
        ref = omodel.ctc_model_forward(sd, x, labs, sl, L, **okw)
    plain = omodel.ctc_model_forward(sd, x, labs, sl, L, want_grads=False, **okw)
    assert abs(ref['total_loss'] - plain['total_loss']) > 1e-2            # the term is there
    loss, logits = model.compute_loss(x, dense, sl, keep_prob=1.0, softmax_temperature=temp)
    assert cls_ops.CALLS == dict(calls=1, lse_done=0, no_grad=0)
    assert abs(loss.item() - ref['total_loss']) / abs(ref['total_loss']) < 1e-5
    assert np.abs(logits.numpy() - ref['logits']).max() < 1e-5
    assert np.abs(model.ctc_losses.numpy() - plain['ctc_losses']).max() < 1e-4     # ctc_losses stay the plain ones
    thl._check_grads(model._set_optimizer('sgd', 0.1), loss, model, ref)
    # one momentum step: per-variable clip, then the update
    before = {k: v.numpy().copy() for k, v in model.store.state_dict().items()}
    loss, _ = model.compute_loss(x, dense, sl, keep_prob=1.0, softmax_temperature=temp)
    model.train(loss, 'momentum', 0.1)
    after = model.store.state_dict()
    for name, r in ref['grads'].items():
        want = before[name] - 0.1 * oopt.clip_by_norm(r, 0.05)
        assert np.abs(after[name].numpy() - want).max() < 1e-5, name
    # a dev loss is the plain CTC loss through today's calls
    model.store.load_state_dict({k: torch.tensor(v) for k, v in sd.items()})
    n = cls_ops.CALLS['calls']
    dev, _ = model.compute_loss(x, dense, sl, keep_prob=1.0, softmax_temperature=temp, is_training=False)
    assert cls_ops.CALLS['calls'] == n
    assert abs(dev.item() - plain['total_loss']) / abs(plain['total_loss']) < 1e-5


@pytest.mark.parametrize('enc', ['blstm', 'lstm'])
def test_eps_zero_is_the_model_without_the_keyword(monkeypatch, enc):
    cls_ops.install(monkeypatch)
    rng = np.random.RandomState(6)
    B, T, D, H, L, C = 4, 11, 6, 8, 2, 6
    x, sl, labs, dense = thl._batch(rng, B, T, D, C)
    plain = _ctc(enc, D, H, L, C)
    b, lb = plain.compute_loss(x, dense, sl, keep_prob=1.0)
    gb = {n: g.numpy().copy() for g, n in plain._set_optimizer('sgd', 0.1).compute_gradients(b, model=plain)}
    model = _ctc(enc, D, H, L, C, label_smoothing_prob=0.0)
    a, la = model.compute_loss(x, dense, sl, keep_prob=1.0)
    assert a.numpy().tobytes() == b.numpy().tobytes() and torch.equal(la, lb)
    for g, n in model._set_optimizer('sgd', 0.1).compute_gradients(a, model=model):
        assert g.numpy().tobytes() == gb[n].tobytes(), n
    assert cls_ops.CALLS['calls'] == 0


# ---------------------------------------------------------------- multitask
def _multitask(**kw):
    from tensorflow_end2end_speech_recognition_amd.models.ctc.multitask_ctc import MultitaskCTC
    return MultitaskCTC(encoder_type='multitask_blstm', input_size=6, num_units=8, num_layers_main=3, num_layers_sub=2,
                        num_classes_main=7, num_classes_sub=3, main_task_weight=0.7, parameter_init=0.1,
                        clip_grad_norm=5.0, clip_activation=50, dtype='f32', seed=9, device='cpu', **kw)


def test_multitask_ctc_host_logic_with_label_smoothing(monkeypatch):
    cls_ops.install(monkeypatch)
    rng = np.random.RandomState(17)
    B, T, D, Cm, Cs, w = 4, 10, 6, 7, 3, 0.7
    x, sl, labs_m, dense_m = thl._batch(rng, B, T, D, Cm)
    labs_s = [[int(v) for v in rng.randint(0, Cs, size=max(1, int(sl[b]) // 5))] for b in range(B)]
    dense_s = np.full((B, max(len(l) for l in labs_s)), -1, dtype=np.int64)
    for b, l in enumerate(labs_s):
        dense_s[b, :len(l)] = l
    model = _multitask(label_smoothing_prob=EPS)
    sd = _randomise_biases(model, rng)
    with ols.patched(EPS):
        ref = omodel.multitask_ctc_model_forward(sd, x, labs_m, labs_s, sl, 3, 2, w, ndir=2, cell_clip=50.0)
    plain = omodel.multitask_ctc_model_forward(sd, x, labs_m, labs_s, sl, 3, 2, w, ndir=2, cell_clip=50.0)
    assert abs(ref['total_loss'] - plain['total_loss']) > 1e-2
    loss, lg_m, lg_s = model.compute_loss(x, dense_m, dense_s, sl, keep_prob=1.0)
    assert cls_ops.CALLS['calls'] == 2                                       # both heads
    assert abs(loss.item() - ref['total_loss']) / abs(ref['total_loss']) < 1e-5
    assert np.abs(lg_m.numpy() - ref['logits_main']).max() < 1e-5
    assert np.abs(model.ctc_losses.numpy() - plain['ctc_losses_main']).max() < 1e-4
    assert np.abs(model.ctc_losses_sub.numpy() - plain['ctc_losses_sub']).max() < 1e-4
    thl._check_grads(model._set_optimizer('sgd', 0.1), loss, model, ref)
    dev, _, _ = model.compute_loss(x, dense_m, dense_s, sl, keep_prob=1.0, is_training=False)
    assert cls_ops.CALLS['calls'] == 2
    assert abs(dev.item() - plain['total_loss']) / abs(plain['total_loss']) < 1e-5
    # eps = 0: the model without the keyword, bit for bit
    cls_ops._reset_ctc_ls_counts()
    got = []
    for kw in ({}, dict(label_smoothing_prob=0.0)):
        m = _multitask(**kw)
        l, _, _ = m.compute_loss(x, dense_m, dense_s, sl, keep_prob=1.0)
        got.append((l.numpy().tobytes(), {n: g.numpy().tobytes() for g, n in
                                          m._set_optimizer('sgd', 0.1).compute_gradients(l, model=m)}))
    assert got[0] == got[1] and cls_ops.CALLS['calls'] == 0


# ---------------------------------------------------------------- joint CTC / attention
def _joint(**kw):
    from tensorflow_end2end_speech_recognition_amd.models.attention.joint_ctc_attention import JointCTCAttention
    return thl._mk_att(JointCTCAttention, 'bahdanau_content', 6, 8, 2, 12, 10, 4, 5, lambda_weight=0.5, **kw)


def test_joint_ctc_attention_host_logic_with_ctc_label_smoothing(monkeypatch):
    import _cpu_ops_att_ss
    cls_ops.install(monkeypatch, base=_cpu_ops_att_ss)          # (the attention targets' smoothing has its own stand-in)
    rng = np.random.RandomState(3)
    B, T, D, L, C = 4, 10, 6, 2, 5
    x, sl, labels, lsl, ctc_labels = thl._att_batch(rng, B, T, D, C)
    model = _joint(ctc_label_smoothing_prob=EPS)
    assert model.ctc_label_smoothing_prob == EPS and model.label_smoothing_prob == 0.0
    sd = {k: v.numpy().copy() for k, v in model.store.state_dict().items()}
    ctc_list = [[int(v) for v in row if v >= 0] for row in ctc_labels]
    okw = dict(clip_enc=50.0, clip_dec=50.0, ctc_labels=ctc_list, lambda_weight=0.5)
    with ols.patched(EPS):
        ref = oatt.attention_model_forward(sd, x, labels, sl, lsl, L, 'bahdanau_content', **okw)
    plain = oatt.attention_model_forward(sd, x, labels, sl, lsl, L, 'bahdanau_content', **okw)
    assert abs(ref['total_loss'] - plain['total_loss']) > 1e-2
    loss, logits, ctc_logits, otr, oinf = model.compute_loss(x, labels, ctc_labels, sl, lsl, 1.0, 1.0, 1.0)
    assert cls_ops.CALLS['calls'] == 1
    assert abs(loss.item() - ref['total_loss']) / abs(ref['total_loss']) < 1e-5
    assert np.abs(ctc_logits.numpy() - ref['ctc_logits']).max() < 1e-5
    assert np.abs(model.ctc_losses.numpy() - plain['ctc_losses']).max() < 1e-4
    seen = set()
    for g, name in model._set_optimizer('adam', 1e-3).compute_gradients(loss, model=model):
        r = ref['grads'][name]
        seen.add(name)
        err = np.abs(g.numpy() - r).max()
        assert err < 1e-4 * max(np.abs(r).max(), 1e-3) + 1e-7, (name, err)
    assert seen == set(ref['grads'])
    dev = model.compute_loss(x, labels, ctc_labels, sl, lsl, 1.0, 1.0, 1.0, is_training=False)[0]
    assert cls_ops.CALLS['calls'] == 1
    assert abs(dev.item() - plain['total_loss']) / abs(plain['total_loss']) < 1e-5
    # eps = 0: the model without the keyword, bit for bit; label_smoothing_prob alone never reaches the CTC head
    cls_ops._reset_ctc_ls_counts()
    got = []
    for kw in ({}, dict(ctc_label_smoothing_prob=0.0)):
        m = _joint(**kw)
        l = m.compute_loss(x, labels, ctc_labels, sl, lsl, 1.0, 1.0, 1.0)[0]
        got.append((l.numpy().tobytes(), {n: g.numpy().tobytes() for g, n in
                                          m._set_optimizer('adam', 1e-3).compute_gradients(l, model=m)}))
    assert got[0] == got[1]
    m = _joint(label_smoothing_prob=0.1)
    m.compute_loss(x, labels, ctc_labels, sl, lsl, 1.0, 1.0, 1.0)
    assert cls_ops.CALLS['calls'] == 0


# ---------------------------------------------------------------- keyword contract and recipes
def test_constructor_range_errors(monkeypatch):
    cls_ops.install(monkeypatch)
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError):
            _ctc('blstm', 6, 8, 2, 6, label_smoothing_prob=bad)
        with pytest.raises(ValueError):
            _multitask(label_smoothing_prob=bad)
        with pytest.raises(ValueError):
            _joint(ctc_label_smoothing_prob=bad)
    assert _ctc('lstm', 6, 8, 1, 6, label_smoothing_prob=0.999).label_smoothing_prob == 0.999
    assert _ctc('lstm', 6, 8, 1, 6).label_smoothing_prob == 0.0


def _yml(rel):
    import yaml
    with open(os.path.join(ROOT, 'examples/timit/config', rel)) as f:
        return yaml.safe_load(f)['param']


def test_recipe_run_name_tags(monkeypatch):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    cls_ops.install(monkeypatch)
    from examples.timit.training import train_ctc, train_joint_ctc_attention, train_multitask_ctc
    small = dict(input_size=6, num_units=8, num_layers=1, dtype='f32', device='cpu')
    p = dict(_yml('ctc/blstm_ctc_phone61.yml'), **small)
    plain = train_ctc.build_model(dict(p))
    assert '_ls' not in plain.name and plain.label_smoothing_prob == 0.0
    assert '_ls' not in train_ctc.build_model(dict(p, label_smoothing_prob=None)).name
    assert '_ls' not in train_ctc.build_model(dict(p, label_smoothing_prob=0)).name
    ls = _yml('ctc/blstm_ctc_phone61_ls.yml')
    assert ls['label_smoothing_prob'] == 0.2
    assert {k: v for k, v in ls.items() if k != 'label_smoothing_prob'} == _yml('ctc/blstm_ctc_phone61.yml')
    m = train_ctc.build_model(dict(ls, **small))
    assert m.name == plain.name + '_ls0.2' and m.label_smoothing_prob == 0.2
    mt = _yml('ctc/multitask_blstm_ctc_char_phone61.yml')
    base = train_multitask_ctc.run_name_suffix(mt)
    assert '_ls' not in base and train_multitask_ctc.run_name_suffix(dict(mt, label_smoothing_prob=0.1)) == base + '_ls0.1'
    at = dict(_yml('attention/blstm_attention_phone61.yml'), lambda_weight=0.3)
    base = train_joint_ctc_attention.joint_run_name(at)
    assert base.endswith('_lambda0.3') and '_ctcls' not in base
    assert train_joint_ctc_attention.joint_run_name(dict(at, ctc_label_smoothing_prob=0.2)) == base + '_ctcls0.2'
    # the attention targets' key keeps its own tag and does not add the CTC one
    both = train_joint_ctc_attention.joint_run_name(dict(at, label_smoothing_prob=0.1))
    assert '_ls0.1' in both and '_ctcls' not in both


def test_timit_label_smoothing_recipe_takes_two_steps(monkeypatch, tmp_path):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    cls_ops.install(monkeypatch)
    from examples.timit.training import train_ctc
    corpus = str(tmp_path / 'corpus')
    thl._make_timit_like(corpus, np.random.RandomState(0), n_train=16, n_dev=2, n_test=2, multitask=False)
    cfg = thl._recipe_cfg(ROOT, 'examples/timit/config/ctc/blstm_ctc_phone61_ls.yml', tmp_path, input_size=6, num_units=8,
                          num_layers=1, batch_size=8, num_epoch=1, eval_start_epoch=1, print_step=1, optimizer='adam',
                          learning_rate=0.05, dropout=0.0, weight_decay=0, decay_start_epoch=2, dtype='f32', device='cpu',
                          dataset_root=corpus, sort_stop_epoch=2)
    random.seed(0)
    out = train_ctc.main(cfg, str(tmp_path / 'runs'))
    assert out['save_path'].endswith(os.path.join('ctc', 'phone61', 'blstm_ctc_8_1_adam_lr0.05_ls0.2'))
    assert out['model'].label_smoothing_prob == 0.2
    assert cls_ops.CALLS['calls'] == 2 and cls_ops.CALLS['no_grad'] == 0       # two training steps; dev losses are plain
    assert len(out['ler_dev']) == 1
