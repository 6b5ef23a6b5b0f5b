"""CPU: StudentCTC (models/ctc/student_ctc.py, reference student_ctc.py) and the four student encoders on the kernel
stand-ins of _cpu_ops_student: construction, variables, loss and gradients against what the reference's own code computes
(tests/golden/student_v1.npz, tests/golden/make_golden_student.py), batch statistics over padded frames, the moving-average
commit, weight decay, checkpoints and the single-device guard."""
import numpy as np
import pytest
import torch

import _cpu_ops_student
import _student_golden as G

ENCODERS = ['student_cnn', 'student_cnn_compact', 'student_cnn_xe', 'student_cnn_compact_xe']


def _model(enc, dtype='f32', **kw):
    from tensorflow_end2end_speech_recognition_amd.models.ctc.student_ctc import StudentCTC
    input_size = 240 if not enc.endswith('_xe') else 1200
    return StudentCTC(enc, input_size, 30, splice=5, num_stack=2, device='cpu', dtype=dtype, **kw)


@pytest.mark.parametrize('enc', ENCODERS)
def test_builds_every_encoder(enc):
    m = _model(enc)
    assert m.name == enc + '_ctc' and m.num_classes == 31
    assert m.encoder.F == 40 and m.encoder.W == 10 and m.encoder.Hp == 14
    full = 'compact' not in enc
    assert m.encoder.output_dim == (2048 if full else 768)
    assert tuple(m.store['CNN2/conv/weight'].shape) == ((3, 4, 128, 256) if full else (3, 4, 64, 128))


def test_unknown_encoder_and_registry():
    from tensorflow_end2end_speech_recognition_amd.models.ctc.student_ctc import StudentCTC
    from tensorflow_end2end_speech_recognition_amd.models.encoders.load_encoder import load
    with pytest.raises(NotImplementedError):
        StudentCTC('student_cnn_ctc', 240, 30, splice=5, num_stack=2, device='cpu')
    with pytest.raises(ValueError):
        load('student_cnn_ctc')
    with pytest.raises(AssertionError):
        StudentCTC('student_cnn', 240, 30, splice=4, num_stack=2, device='cpu')


def test_world_size_guard():
    with pytest.raises(ValueError, match='single device'):
        _model('student_cnn_compact', world_size=2)


@pytest.mark.parametrize('case', sorted(['ctc_student_cnn_T5', 'ctc_student_cnn_compact_T5', 'xe_student_cnn_xe',
                                         'xe_student_cnn_compact_xe']))
def test_variables_match_reference_metadata(case):
    _, meta = G.load()
    mc = meta[case]
    m = _model(mc['encoder_type'])
    got = [[n, list(sh), t] for n, sh, t in m.variables()]
    assert got == mc['vars']


# ---------------------------------------------------------------- against the reference's own code
def fixture_model(case, dtype='f32'):
    _, meta = G.load()
    mc = meta[case]
    m = _model(mc['encoder_type'], dtype=dtype, weight_decay=mc['weight_decay'])
    vals = {n: torch.from_numpy(G.values(mc['vkey'], n, sh)).float() for n, sh, _ in mc['vars']}
    m.store.load_state_dict(vals)
    m.state.load_state_dict(vals)
    return m


def run_case(m, case, is_training=None):
    z, meta = G.load()
    mc = meta[case]
    is_training = mc['is_training'] if is_training is None else is_training
    x = z[case + '|in|inputs']
    if mc['encoder_type'].endswith('_xe'):
        loss, logits = m.compute_xe_loss(x, z[case + '|in|soft_targets'], 1.0, is_training=is_training)
        return loss, logits.double().cpu().numpy(), m.xe_losses.double().cpu().numpy()
    lens = z[case + '|in|inputs_seq_len'].astype(np.int32)
    flat, ll = z[case + '|in|labels_flat'], z[case + '|in|labels_len']
    dense = np.full((len(ll), int(ll.max())), -1, dtype=np.int64)
    o = 0
    for b, n in enumerate(ll):
        dense[b, :n] = flat[o:o + n]
        o += n
    loss, logits = m.compute_ctc_loss(x, dense, lens, 1.0, is_training=is_training)
    lg = logits.double().cpu().numpy()
    valid = np.concatenate([lg[:lens[b], b] for b in range(len(lens))], 0)
    return loss, valid, m.ctc_losses.double().cpu().numpy()


def check_forward(m, case, loss_tol, logit_tol):
    z, _ = G.load()
    loss, logits, losses = run_case(m, case)
    ref = float(z[case + '|out|total_loss'])
    assert abs(loss.item() - ref) <= loss_tol * abs(ref), (loss.item(), ref)
    rl = z[case + '|out|losses']
    assert np.abs(losses - rl).max() <= loss_tol * np.abs(rl).max(), (losses, rl)
    rv = z[case + '|out|logits']
    assert np.linalg.norm(logits - rv) <= logit_tol * np.linalg.norm(rv)


def check_gradients(m, case, grad_tol):
    z, _ = G.load()
    m._backward()
    errs = {n: G.gradient_error(z, case, n, m.store.g(n).double().cpu().numpy()) for n in m.store.names}
    bad = {n: e for n, e in errs.items() if e >= grad_tol}
    assert not bad, bad
    return errs


@pytest.mark.parametrize('case', ['ctc_student_cnn_T5', 'ctc_student_cnn_compact_T5', 'ctc_student_cnn_T7',
                                  'ctc_student_cnn_compact_T7', 'xe_student_cnn_xe', 'xe_student_cnn_compact_xe',
                                  'ctc_wd'])
def test_fp32_model_against_reference_fixture(monkeypatch, case):
    _cpu_ops_student.install(monkeypatch)
    m = fixture_model(case)
    check_forward(m, case, 1e-5, 1e-5)
    errs = check_gradients(m, case, 1e-4)
    assert {'CNN1/batch_norm/gamma', 'CNN1/batch_norm/beta', 'CNN2/batch_norm/gamma'} <= set(errs)
    assert set(m.encoder.conv_path.values()) == {'im2col'}


@pytest.mark.parametrize('enc', ['student_cnn', 'student_cnn_compact'])
def test_padding_enters_the_batch_statistics(monkeypatch, enc):
    """The same utterances padded to T = 5 and T = 7 give different valid-frame logits, each matching its own fixture:
    statistics over the valid frames only (or over a 16-utterance tile) would match neither."""
    _cpu_ops_student.install(monkeypatch)
    z, _ = G.load()
    outs = []
    for T in (5, 7):
        case = 'ctc_%s_T%d' % (enc, T)
        m = fixture_model(case)
        _, logits, _ = run_case(m, case)
        rv = z[case + '|out|logits']
        assert np.linalg.norm(logits - rv) <= 1e-5 * np.linalg.norm(rv)
        outs.append(logits)
    assert np.linalg.norm(outs[0] - outs[1]) > 1e-3 * np.linalg.norm(outs[0])


@pytest.mark.parametrize('case', ['ctc_student_cnn_compact_T5', 'xe_student_cnn_xe'])
def test_moving_averages_commit_once_per_step(monkeypatch, case):
    _cpu_ops_student.install(monkeypatch)
    z, meta = G.load()
    m = fixture_model(case)
    before = {n: v.clone() for n, v in m.state.state_dict().items()}
    run_case(m, case)                                        # a forward alone: nothing moves
    run_case(m, case)
    for n, v in m.state.state_dict().items():
        assert torch.equal(v, before[n]), n
    loss, _, _ = run_case(m, case)
    m.train(loss, 'sgd', 0.0)
    for n, v in m.state.state_dict().items():
        r = z['%s|avg_after|%s' % (case, n)]
        assert np.abs(v.double().cpu().numpy() - r).max() <= 1e-5 * max(1.0, np.abs(r).max()), n
    after = {n: v.clone() for n, v in m.state.state_dict().items()}
    run_case(m, case, is_training=False)                     # evaluation with the averages moves nothing either
    for n, v in m.state.state_dict().items():
        assert torch.equal(v, after[n]), n


def test_eval_mode_uses_the_moving_averages(monkeypatch):
    _cpu_ops_student.install(monkeypatch)
    case = 'ctc_eval'
    m = fixture_model(case)
    check_forward(m, case, 1e-5, 1e-5)
    with pytest.raises(RuntimeError):
        m._backward()


def test_weight_decay_covers_gamma_and_beta_not_biases_or_averages(monkeypatch):
    """ctc_wd matches the reference (checked with the fixture test); here the rule itself: the decay mask holds exactly
    the trainable variables without 'bias' in their names, the averages are not in the flat buffer at all."""
    m = _model('student_cnn_compact', weight_decay=1e-3)
    mask = dict(zip(m.store.names, m.store.decay_mask.tolist()))
    assert mask['CNN1/batch_norm/gamma'] == 1 and mask['CNN2/batch_norm/beta'] == 1
    assert mask['CNN1/conv/bias'] == 0 and mask['fc1/biases'] == 0 and mask['CNN1/conv/weight'] == 1
    assert not any('avg_' in n for n in m.store.names)
    assert m.state.names == ['CNN1/batch_norm/avg_mean', 'CNN1/batch_norm/avg_variance',
                             'CNN2/batch_norm/avg_mean', 'CNN2/batch_norm/avg_variance']


def test_checkpoint_keeps_the_moving_averages(monkeypatch, tmp_path):
    from tensorflow_end2end_speech_recognition_amd.utils.training.checkpoint import Saver
    _cpu_ops_student.install(monkeypatch)
    case = 'ctc_student_cnn_compact_T5'
    m = fixture_model(case)
    loss, _, _ = run_case(m, case)
    m.train(loss, 'adam', 1e-3)
    saver = Saver()
    prefix = saver.save(m, str(tmp_path / 'model.ckpt'), global_step=1)
    m2 = _model('student_cnn_compact')
    saver.restore(m2, prefix)
    for n, v in m.state.state_dict().items():
        assert torch.equal(m2.state[n], v), n
    for n, v in m.store.state_dict().items():
        assert torch.equal(m2.store[n], v), n
    z = dict(np.load(prefix + '.npz'))
    z.pop('CNN2/batch_norm/avg_variance')
    np.savez(str(tmp_path / 'bad.npz'), **z)
    with pytest.raises(ValueError, match='CNN2/batch_norm/avg_variance'):
        saver.restore(_model('student_cnn_compact'), str(tmp_path / 'bad'))


def test_xe_ignores_the_temperature(monkeypatch):
    _cpu_ops_student.install(monkeypatch)
    case = 'xe_student_cnn_compact_xe'
    z, _ = G.load()
    m = fixture_model(case)
    l1, _ = m.compute_xe_loss(z[case + '|in|inputs'], z[case + '|in|soft_targets'], 1.0, softmax_temperature=2)
    assert abs(l1.item() - float(z[case + '|out|total_loss'])) <= 1e-5 * float(z[case + '|out|total_loss'])


def test_bf16_implicit_path_composition(monkeypatch):
    """bf16 model on the stand-ins: CNN2 takes the implicit 3x4 path and matches the reference to bf16 tolerance.  The
    batch-norm backward over 10 images amplifies the bf16 rounding of the stored operands: the lowest layers' gradients
    sit up to ~0.26 relative L2 from the fp64 reference on this case (the fp32 path holds 1e-4)."""
    _cpu_ops_student.install(monkeypatch)
    case = 'ctc_student_cnn_compact_T5'
    m = fixture_model(case, dtype='bf16')
    check_forward(m, case, 2e-2, 5e-2)
    assert m.encoder.conv_path == {'CNN1/conv': 'im2col', 'CNN2/conv': 'implicit'}
    check_gradients(m, case, 0.5)
