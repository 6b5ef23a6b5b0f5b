"""On-device input augmentation (input_noise_std, freq_mask_*, time_mask_*: an extension) on the host: the numpy statement
(tests/_input_aug_oracle.py) against its known answers, the distribution of the mask draws, keyword validation, the
ModelBase hook in CTC / MultitaskCTC / AttentionSeq2Seq / JointCTCAttention on the CPU stand-ins
(tests/_cpu_ops_input_aug.py), _add_noise_to_inputs, the recipes, and the per-rank key under gloo."""
import inspect
import os
import random
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import _cpu_ops_input_aug as ia_ops
import _cpu_ops_weight_noise as wn_ops
import _input_aug_oracle as iao
import test_host_logic as thl
from test_distributed_cpu import _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUG = dict(input_noise_std=0.05, freq_mask_num=2, freq_mask_width=1, time_mask_num=2, time_mask_width=4)
OFF = dict(input_noise_std=0.0, freq_mask_num=0, freq_mask_width=0, time_mask_num=0, time_mask_width=0)


# ---------------------------------------------------------------- the statement
def test_known_answers():
    """Seed 1234, offset 0, n_ch 4, lengths [40, 17, 1], two frequency masks of width <= 3, two time masks of width <= 10
    at ratio 0.5, as (width, start): overlapping masks, a zero-width mask, an utterance too short to be time-masked."""
    lens = np.array([40, 17, 1])
    fd = iao.freq_draws(3, 4, 2, 3, 1234, 0)
    td = iao.time_draws(lens, 2, 10, 0.5, 1234, 0)
    assert fd.tolist() == [[[3, 0], [2, 0]], [[2, 0], [0, 2]], [[3, 1], [2, 0]]]
    assert td.tolist() == [[[1, 22], [10, 22]], [[1, 1], [6, 5]], [[0, 1], [0, 1]]]
    assert iao.time_cap(lens, 10, 0.5).tolist() == [10, 8, 0]
    # and the cover they give
    x = np.random.RandomState(0).randn(3, 40, 12).astype(np.float32)
    x[1, 17:] = np.nan
    x[2, 1:] = np.nan
    y = iao.augment(x, lens, 4, 0.0, (2, 3), (2, 10, 0.5), -7.0, 1234, 0)
    m = y == np.float32(-7.0)
    assert m[0][:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].all() and m[0, 22:32].all() and not m[0, :22, 3::4].any()
    assert m[1, :17][:, [0, 1, 4, 5, 8, 9]].all() and m[1, 1].all() and m[1, 5:11].all() and not m[1, 0, 2:4].any()
    assert m[2, 0].all()                                   # (3,1) and (2,0) together cover all four channels
    keep = ~m
    assert np.array_equal(y.view(np.int32)[keep], x.view(np.int32)[keep])   # padded NaN included
    assert np.isnan(y[1, 17:]).all() and np.isnan(y[2, 1:]).all()


def test_slots_and_offsets_do_not_collide():
    lens = np.full(4, 30)
    a = iao.time_draws(lens, 8, 10, 1.0, 5, 1 << 40)
    assert not np.array_equal(a, iao.time_draws(lens, 8, 10, 1.0, 5, 2 << 40))
    assert not np.array_equal(a, iao.time_draws(lens, 8, 10, 1.0, 6, 1 << 40))
    # slot m of a call with fewer masks is slot m of a call with more, and time slots are not the frequency slots
    assert np.array_equal(a[:, :3], iao.time_draws(lens, 3, 10, 1.0, 5, 1 << 40))
    c = iao._slot_blocks(4, 0, 16, 5, 1 << 40)
    assert len({tuple(r) for r in c.reshape(-1, 4).tolist()}) == 64
    # the noise counters offset + [0, 2^39) and the mask slots offset + 2^39 + [0, 16 B) stay inside one k << 40 window
    assert iao.MASK_BASE + 16 * (1 << 20) < (1 << 40)


def _cells_within(values, n_cells, what):
    n = len(values)
    counts = np.bincount(values, minlength=n_cells)
    assert len(counts) == n_cells, what
    p = 1.0 / n_cells
    dev = np.abs(counts - n * p) / np.sqrt(n * p * (1 - p))
    assert dev.max() < 5, (what, dev.max())
    return dev.max()


def test_draws_are_uniform_on_their_ranges():
    B, n_ch, fcap, T, tcap = 1 << 16, 41, 6, 40, 10
    fd = iao.freq_draws(B, n_ch, 1, fcap, 99, 7 << 40)[:, 0]
    td = iao.time_draws(np.full(B, T), 1, tcap, 0.5, 99, 7 << 40)[:, 0]
    worst = [_cells_within(fd[:, 0], fcap + 1, 'fw'), _cells_within(td[:, 0], tcap + 1, 'tw')]
    for w in range(fcap + 1):
        worst.append(_cells_within(fd[fd[:, 0] == w, 1], n_ch - w + 1, 'fs | fw = %d' % w))
    for w in range(tcap + 1):
        worst.append(_cells_within(td[td[:, 0] == w, 1], T - w + 1, 'ts | tw = %d' % w))
    print('largest deviation of a cell: %.2f standard errors' % max(worst))
    assert (fd[:, 1] + fd[:, 0] <= n_ch).all() and (td[:, 1] + td[:, 0] <= T).all()


def test_stand_in_is_the_statement_and_checks_like_the_entry_point(monkeypatch):
    ops = ia_ops.install(monkeypatch)
    x = torch.from_numpy(np.random.RandomState(1).randn(2, 9, 6).astype(np.float32))
    keep = x.clone()
    sl = torch.tensor([9, 4], dtype=torch.int32)
    y = ops.input_augment(x, sl, 2, noise_std=0.1, freq_masks=(1, 1), time_masks=(2, 3, 1.0), seed=3, offset=1 << 40)
    assert torch.equal(x, keep) and y.data_ptr() != x.data_ptr()
    want = iao.augment(keep.numpy(), [9, 4], 2, 0.1, (1, 1), (2, 3, 1.0), 0.0, 3, 1 << 40)
    assert np.array_equal(y.numpy(), want) and np.array_equal(y.numpy()[1, 4:], keep.numpy()[1, 4:])
    assert ops.input_augment_counts() == dict(calls=1, elements=108, vec_calls=1)
    for bad in (dict(n_ch=4), dict(n_ch=0), dict(freq_masks=(9, 1)), dict(time_masks=(1, -1, 1.0)),
                dict(time_masks=(1, 1, 1.5)), dict(noise_std=-1.0), dict(noise_std=float('nan')),
                dict(mask_value=float('inf'))):
        with pytest.raises(ValueError):
            ops.input_augment(x, sl, **dict(dict(n_ch=2), **bad))
    ops.reset_input_augment_counts()
    assert ops.input_augment_counts() == dict(calls=0, elements=0, vec_calls=0)


# ---------------------------------------------------------------- models
def _ctc(enc='blstm', **kw):
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    kw.setdefault('seed', 3)
    return CTC(encoder_type=enc, input_size=6, num_units=8, num_layers=2, num_classes=6, parameter_init=0.1,
               clip_grad_norm=5.0, clip_activation=50, dtype='f32', device='cpu', **kw)


def _multitask(**kw):
    from tensorflow_end2end_speech_recognition_amd.models.ctc.multitask_ctc import MultitaskCTC
    return MultitaskCTC(encoder_type='multitask_blstm', input_size=6, num_units=8, num_layers_main=3, num_layers_sub=2,
                        num_classes_main=7, num_classes_sub=3, main_task_weight=0.7, parameter_init=0.1,
                        clip_grad_norm=5.0, clip_activation=50, dtype='f32', seed=9, device='cpu', **kw)


def _att(joint, **kw):
    from tensorflow_end2end_speech_recognition_amd.models.attention.attention_seq2seq import AttentionSeq2Seq
    from tensorflow_end2end_speech_recognition_amd.models.attention.joint_ctc_attention import JointCTCAttention
    if joint:
        return thl._mk_att(JointCTCAttention, 'location', 6, 8, 2, 12, 10, 4, 5, lambda_weight=0.5, **kw)
    return thl._mk_att(AttentionSeq2Seq, 'location', 6, 8, 2, 12, 10, 4, 5, **kw)


def _bytes(t):
    return t.detach().numpy().tobytes()


MAKERS = [_ctc, _multitask, lambda **kw: _att(False, **kw), lambda **kw: _att(True, **kw)]


def test_keyword_validation():
    for mk in MAKERS:
        for bad in (dict(freq_mask_num=9), dict(freq_mask_num=-1), dict(time_mask_num=9), dict(time_mask_num=-1),
                    dict(freq_mask_width=2), dict(freq_mask_width=5), dict(freq_mask_width=-1),
                    dict(time_mask_width=-1), dict(time_mask_ratio=1.01), dict(time_mask_ratio=-0.1),
                    dict(time_mask_ratio=float('nan')), dict(input_noise_std=-1e-9), dict(input_noise_std=float('nan')),
                    dict(input_noise_std=float('inf')), dict(input_channels=4), dict(input_channels=0)):
            with pytest.raises(ValueError):
                mk(**bad)                                  # (input_size 6: 2 base channels, so a width of 2 is too wide)
        m = mk(**AUG)
        assert m.input_channels == 2 and m.time_mask_ratio == 1.0 and m.input_noise_std == 0.05
        assert (m.freq_mask_num, m.freq_mask_width, m.time_mask_num, m.time_mask_width) == (2, 1, 2, 4)
        assert mk(input_channels=6, freq_mask_width=5).input_channels == 6
        assert mk(input_channels=3).input_channels == 3
        plain = mk()
        assert plain.input_channels == 2 and not plain._augment_on() and m._augment_on()
        assert not mk(freq_mask_num=2, time_mask_num=2)._augment_on()      # no width: nothing to do
        assert not mk(freq_mask_width=1, time_mask_width=4)._augment_on()  # no count
        assert not mk(time_mask_num=1, time_mask_width=4, time_mask_ratio=0.0)._augment_on()


def test_default_channels_follow_input_size():
    from tensorflow_end2end_speech_recognition_amd.models.model_base import ModelBase
    m = ModelBase()
    m._set_input_augment(123)
    assert m.input_channels == 41
    m._set_input_augment(40)
    assert m.input_channels == 40
    m._set_input_augment(123, freq_mask_width=40)
    with pytest.raises(ValueError):
        m._set_input_augment(123, freq_mask_width=41)


def test_student_ctc_and_rnnlm_do_not_take_the_keywords():
    from tensorflow_end2end_speech_recognition_amd.models.ctc.student_ctc import StudentCTC
    from tensorflow_end2end_speech_recognition_amd.models.lm.base import RNNLM
    for cls in (StudentCTC, RNNLM):
        sig = inspect.signature(cls.__init__)
        assert not {'input_noise_std', 'freq_mask_num', 'time_mask_num', 'input_channels'} & set(sig.parameters)
        assert not any(p.kind == p.VAR_KEYWORD for p in sig.parameters.values())


def _check_hook(a, b, run, seed, x, sl, infer=None):
    """a: the augmenting model, b: its plain twin; run(model, inputs, **kw) -> the tuple compute_loss returns."""
    x_keep = x.copy()
    for k in (1, 2):
        n = ia_ops.CALLS['calls']
        ra = run(a, x)
        assert ia_ops.CALLS['calls'] == n + 1 and a._augment_calls == k
        log = ia_ops.LOG[-1]
        assert (log['seed'], log['offset'], log['n_ch']) == (seed + 11, k << 40, 2)
        assert (log['noise_std'], log['freq_masks'], log['time_masks'], log['mask_value']) == \
            (0.05, (2, 1), (2, 4, 1.0), 0.0)
        assert np.array_equal(log['seq_len'], sl) and log['shape'] == x.shape
        assert np.array_equal(x, x_keep)                   # the caller's array is untouched
        # the step is the plain twin's step on the augmented inputs
        xa = iao.augment(x, sl, 2, 0.05, (2, 1), (2, 4, 1.0), 0.0, seed + 11, k << 40)
        assert not np.array_equal(xa, x)
        rb = run(b, xa)
        assert ia_ops.CALLS['calls'] == n + 1 and b._augment_calls == 0
        ta, tb = [t for t in ra if torch.is_tensor(t)], [t for t in rb if torch.is_tensor(t)]
        assert len(ta) == len(tb) >= 2 and all(_bytes(u) == _bytes(v) for u, v in zip(ta, tb))
        a.train(ra[0], 'sgd', 0.1)
        b.train(rb[0], 'sgd', 0.1)
        assert _bytes(a.store.grad) == _bytes(b.store.grad) and _bytes(a.store.flat) == _bytes(b.store.flat)
        # a dev loss sees the clean inputs and counts nothing
        da, db = run(a, x, is_training=False), run(b, x, is_training=False)
        assert _bytes(da[0]) == _bytes(db[0]) and ia_ops.CALLS['calls'] == n + 1 and a._augment_calls == k
        if infer is not None:
            assert np.array_equal(infer(a), infer(b)) and ia_ops.CALLS['calls'] == n + 1
    # a device tensor handed in is not written either
    xt = torch.from_numpy(x.copy())
    run(a, xt)
    assert np.array_equal(xt.numpy(), x_keep) and a._augment_calls == 3


def test_ctc_hook(monkeypatch):
    ia_ops.install(monkeypatch)
    x, sl, labs, dense = thl._batch(np.random.RandomState(5), 5, 11, 6, 6)
    run = lambda m, xx, **k: m.compute_loss(xx, dense, sl, keep_prob=1.0, **k)           # noqa: E731
    _check_hook(_ctc(seed=4, **AUG), _ctc(seed=4), run, 4, x, sl)


def test_multitask_hook(monkeypatch):
    ia_ops.install(monkeypatch)
    rng = np.random.RandomState(17)
    x, sl, labs_m, dense_m = thl._batch(rng, 4, 10, 6, 7)
    dense_s = rng.randint(0, 3, size=(4, 2)).astype(np.int64)
    run = lambda m, xx, **k: m.compute_loss(xx, dense_m, dense_s, sl, keep_prob=1.0, **k)   # noqa: E731
    _check_hook(_multitask(**AUG), _multitask(), run, 9, x, sl)


@pytest.mark.parametrize('joint', [False, True])
def test_attention_hooks(monkeypatch, joint):
    ia_ops.install(monkeypatch)
    x, sl, labels, lsl, ctc_labels = thl._att_batch(np.random.RandomState(3), 4, 10, 6, 5)

    def run(m, xx, **k):
        args = (xx, labels, ctc_labels, sl, lsl) if joint else (xx, labels, sl, lsl)
        return m.compute_loss(*args, 1.0, 1.0, 1.0, **k)

    a, b = _att(joint, **AUG), _att(joint)
    _check_hook(a, b, run, 5, x, sl, infer=lambda m: m.infer(x, sl))
    # the lazy inference output of a training forward decodes the AUGMENTED inputs
    ra = run(a, x)
    k = a._augment_calls
    ids_infer = a.decode(ra[-2], ra[-1])[1]
    xa = iao.augment(x, sl, 2, 0.05, (2, 1), (2, 4, 1.0), 0.0, 5 + 11, k << 40)
    assert np.array_equal(ids_infer.numpy(), a.infer(xa, sl)) and a._augment_calls == k


def test_all_off_is_the_model_without_the_keywords(monkeypatch):
    ia_ops.install(monkeypatch)
    x, sl, labs, dense = thl._batch(np.random.RandomState(5), 5, 11, 6, 6)
    runs = []
    for kw in ({}, OFF, dict(OFF, time_mask_ratio=0.3, input_channels=3), dict(input_noise_std=None)):
        m = _ctc(**kw)
        trace = []
        for _ in range(2):
            loss, logits = m.compute_loss(x, dense, sl, keep_prob=0.8)
            m.train(loss, 'momentum', 0.05)
            trace.append((_bytes(loss), _bytes(logits), _bytes(m.store.flat)))
        assert m._augment_calls == 0
        runs.append(trace)
    assert all(r == runs[0] for r in runs[1:])
    assert ia_ops.CALLS['calls'] == 0
    xt = torch.from_numpy(x)
    assert m._augment_inputs(xt, torch.from_numpy(sl)) is xt          # the argument itself comes back


def test_counter_is_apart_from_dropout_and_weight_noise(monkeypatch):
    ia_ops.install(monkeypatch, base=wn_ops)
    x, sl, labs, dense = thl._batch(np.random.RandomState(5), 5, 11, 6, 6)
    m = _ctc(weight_noise_std=0.05, **AUG)
    m.compute_loss(x, dense, sl, keep_prob=0.8, is_training=False)
    for k in (1, 2):
        loss, _ = m.compute_loss(x, dense, sl, keep_prob=0.8)
        m.train(loss, 'sgd', 0.1)
        assert (m._augment_calls, m._noise_calls) == (k, k)
    assert [e['offset'] for e in ia_ops.LOG] == [1 << 40, 2 << 40] and [e[2] for e in wn_ops.LOG] == [1 << 40, 2 << 40]
    assert {e['seed'] for e in ia_ops.LOG} == {3 + 11} and {e[1] for e in wn_ops.LOG} == {3 + 7}


def test_add_noise_to_inputs(monkeypatch):
    ia_ops.install(monkeypatch)
    m = _ctc(seed=4)
    x = np.random.RandomState(2).randn(3, 7, 6).astype(np.float32)
    keep = x.copy()
    y = m._add_noise_to_inputs(x)
    assert np.array_equal(x, keep) and m._augment_calls == 1
    assert np.array_equal(y.numpy(), iao.augment(x, [7, 7, 7], 6, 0.075, seed=4 + 11, offset=1 << 40))
    log = ia_ops.LOG[-1]
    assert (log['noise_std'], log['freq_masks'], log['time_masks'][:2]) == (0.075, (0, 0), (0, 0))
    z = (y.numpy().astype(np.float64) - x) / 0.075
    assert abs(z.mean()) < 0.5 and 0.5 < z.std() < 1.5
    # lengths: padded frames stay; every call has its own offset; std = 0 is a copy
    y2 = m._add_noise_to_inputs(torch.from_numpy(x), stddev=0.2, inputs_seq_len=[7, 2, 0])
    assert np.array_equal(y2.numpy(), iao.augment(x, [7, 2, 0], 6, 0.2, seed=4 + 11, offset=2 << 40))
    assert np.array_equal(y2.numpy()[1, 2:], x[1, 2:]) and np.array_equal(y2.numpy()[2], x[2])
    assert np.array_equal(m._add_noise_to_inputs(x, stddev=0.0).numpy(), x)
    for bad in (-0.1, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            m._add_noise_to_inputs(x, stddev=bad)
    with pytest.raises(NotImplementedError):
        m._add_noise_to_gradients([], 0.1)


# ---------------------------------------------------------------- recipes
def _yml(rel):
    import yaml
    with open(os.path.join(ROOT, 'examples/timit/config', rel)) as f:
        return yaml.safe_load(f)['param']


AUG_KEYS = ('input_noise_std', 'freq_mask_num', 'freq_mask_width', 'time_mask_num', 'time_mask_width', 'time_mask_ratio',
            'input_channels')


def test_recipe_run_name_tags(monkeypatch):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    ia_ops.install(monkeypatch)
    from examples.librispeech.training import train_ctc as libri_ctc
    from examples.timit.training import train_attention, train_ctc, train_joint_ctc_attention, train_multitask_ctc
    from examples.timit.training._common import input_augment_kwargs, input_augment_tag
    assert input_augment_tag({}) == '' and input_augment_tag(dict.fromkeys(AUG_KEYS)) == ''
    assert input_augment_tag(dict(freq_mask_num=2, time_mask_num=2, time_mask_ratio=0.2)) == ''     # no width: off
    assert input_augment_tag(dict(input_noise_std=0.075)) == '_in0.075'
    assert input_augment_tag(dict(freq_mask_num=2, freq_mask_width=6)) == '_sa2x6_0x0'
    assert input_augment_tag(dict(time_mask_num=1, time_mask_width=20)) == '_sa0x0_1x20'
    assert input_augment_tag(dict(input_noise_std=0.1, freq_mask_num=2, freq_mask_width=6, time_mask_num=2,
                                  time_mask_width=20, time_mask_ratio=0.2)) == '_in0.1_sa2x6_2x20_r0.2'
    assert input_augment_kwargs({}) == OFF
    sa = _yml('ctc/blstm_ctc_phone61_specaug.yml')
    base = _yml('ctc/blstm_ctc_phone61.yml')
    assert {k: v for k, v in sa.items() if k not in AUG_KEYS} == base and not set(AUG_KEYS) & set(base)
    assert input_augment_kwargs(sa) == dict(input_noise_std=0.0, freq_mask_num=2, freq_mask_width=6, time_mask_num=2,
                                            time_mask_width=20, time_mask_ratio=0.2)
    small = dict(num_units=8, num_layers=1, dtype='f32', device='cpu')
    plain = train_ctc.build_model(dict(base, **small))
    assert '_sa' not in plain.name and '_in' not in plain.name and not plain._augment_on()
    for absent in (None, 0):
        m = train_ctc.build_model(dict(base, **small, **dict.fromkeys(AUG_KEYS[:5], absent)))
        assert m.name == plain.name and not m._augment_on()
    m = train_ctc.build_model(dict(sa, **small))
    assert m.name == plain.name + '_sa2x6_2x20_r0.2' and m._augment_on() and m.input_channels == 41
    assert (m.freq_mask_num, m.freq_mask_width, m.time_mask_num, m.time_mask_width, m.time_mask_ratio) == (2, 6, 2, 20, 0.2)
    mt = _yml('ctc/multitask_blstm_ctc_char_phone61.yml')
    sfx = train_multitask_ctc.run_name_suffix(mt)
    assert train_multitask_ctc.run_name_suffix(dict(mt, input_noise_std=0.075)) == sfx + '_in0.075'
    at = _yml('attention/blstm_attention_phone61.yml')
    asa = _yml('attention/blstm_attention_phone61_specaug.yml')
    assert {k: v for k, v in asa.items() if k not in AUG_KEYS} == at and not set(AUG_KEYS) & set(at)
    name = train_attention.run_name(at)
    assert train_attention.run_name(asa) == name + '_sa2x6_2x20_r0.2'
    kw = train_attention.model_kwargs(dict(asa, num_classes=61))
    assert (kw['freq_mask_num'], kw['freq_mask_width'], kw['time_mask_ratio'], kw['input_noise_std']) == (2, 6, 0.2, 0.0)
    assert train_attention.model_kwargs(dict(at, num_classes=61))['freq_mask_num'] == 0
    assert train_joint_ctc_attention.joint_run_name(asa) == train_joint_ctc_attention.joint_run_name(at).replace(
        '_lambda', '_sa2x6_2x20_r0.2_lambda')
    lp = dict(base, label_type='character', train_data_size='100h', num_proj=0, seed=2, **small)
    lm = libri_ctc.build_model(dict(lp, input_noise_std=0.075, input_channels=123), 'cpu')
    assert lm.input_noise_std == 0.075 and lm.input_channels == 123
    assert lm.name == libri_ctc.build_model(dict(lp), 'cpu').name + '_in0.075'


def test_librispeech_joint_driver_reads_the_keys():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from examples.librispeech.training import train_joint_ctc_attention as libri_joint
    from examples.timit.training import train_attention
    assert libri_joint.model_kwargs is train_attention.model_kwargs and libri_joint.run_name is train_attention.run_name


def test_timit_ctc_specaug_recipe_takes_two_steps(monkeypatch, tmp_path):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    ia_ops.install(monkeypatch)
    from examples.timit.training import train_ctc
    corpus = str(tmp_path / 'corpus')
    thl._make_timit_like(corpus, np.random.RandomState(0), n_train=16, n_dev=2, n_test=2, multitask=False)
    # (6 columns are 2 base channels: the band shrinks with them)
    cfg = thl._recipe_cfg(ROOT, 'examples/timit/config/ctc/blstm_ctc_phone61_specaug.yml', tmp_path, input_size=6,
                          freq_mask_width=1, num_units=8, num_layers=1, batch_size=8, num_epoch=1, eval_start_epoch=1,
                          print_step=1, optimizer='adam', learning_rate=0.05, dropout=0.0, weight_decay=0,
                          decay_start_epoch=2, dtype='f32', device='cpu', dataset_root=corpus, sort_stop_epoch=2)
    random.seed(0)
    out = train_ctc.main(cfg, str(tmp_path / 'runs'))
    assert out['save_path'].endswith(os.path.join('ctc', 'phone61', 'blstm_ctc_8_1_adam_lr0.05_sa2x1_2x20_r0.2'))
    model = out['model']
    assert model._augment_calls == 2
    # two training steps, each with its own draw; the monitoring and evaluation passes drew nothing
    assert [(e['freq_masks'], e['time_masks'], e['offset']) for e in ia_ops.LOG] == \
        [((2, 1), (2, 20, 0.2), 1 << 40), ((2, 1), (2, 20, 0.2), 2 << 40)]
    assert len(out['ler_dev']) == 1


def test_timit_attention_specaug_recipe_takes_two_steps(monkeypatch, tmp_path):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    ia_ops.install(monkeypatch)
    from examples.timit.training import train_attention
    corpus = str(tmp_path / 'corpus')
    thl._make_timit_like(corpus, np.random.RandomState(0), n_train=16, n_dev=2, n_test=2, multitask=False)
    cfg = thl._recipe_cfg(ROOT, 'examples/timit/config/attention/blstm_attention_phone61_specaug.yml', tmp_path,
                          input_size=6, freq_mask_width=1, encoder_num_units=8, encoder_num_layers=1, attention_dim=6,
                          decoder_num_units=8, embedding_dim=4, max_decode_length=10, dropout_encoder=0.0,
                          dropout_decoder=0.1, dropout_embedding=0.1, batch_size=8, num_epoch=1, eval_start_epoch=1,
                          print_step=1, optimizer='adam', learning_rate=0.02, weight_decay=0, decay_start_epoch=2,
                          dtype='f32', device='cpu', dataset_root=corpus, sort_stop_epoch=2)
    random.seed(0)
    out = train_attention.main(cfg, str(tmp_path / 'runs'))
    assert '_sa2x1_2x20_r0.2' in os.path.basename(out['save_path'])
    assert out['model']._augment_calls == 2
    assert [e['offset'] for e in ia_ops.LOG] == [1 << 40, 2 << 40]


# ---------------------------------------------------------------- data parallel (gloo)
def _dp_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    ia_ops.install(None)
    model = _ctc(seed=6, **AUG)
    x, sl, labs, dense = thl._batch(np.random.RandomState(8), 6, 11, 6, 6)
    lo, hi = ((0, 3), (3, 6))[rank]
    for _ in range(2):
        model.compute_loss(x[lo:hi], dense[lo:hi], sl[lo:hi], keep_prob=1.0)
    q.put((rank, model._augment_key(), [(e['seed'], e['offset']) for e in ia_ops.LOG]))
    dist.destroy_process_group()


def test_data_parallel_ranks_draw_under_different_keys():
    world, port = 2, _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    (_, k0, log0), (_, k1, log1) = res
    assert k0 == 6 + 11 and k1 - k0 == 1 << 32
    assert log0 == [(k0, 1 << 40), (k0, 2 << 40)] and log1 == [(k1, 1 << 40), (k1, 2 << 40)]
    assert _ctc(seed=6)._augment_key() == 6 + 11              # no process group: rank 0
