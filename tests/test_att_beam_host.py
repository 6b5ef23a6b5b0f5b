"""CPU: attention beam search -- the host statement of models/attention/decoders/beam_search against the fixture the
reference's own functions produced (tests/golden/att_beam_v1.npz), and the model / recipe surface on the CPU stand-ins of
tests/_cpu_ops_att_beam.py."""
import os
import sys

import numpy as np
import pytest
import torch

import _att_beam_golden as G
import _cpu_ops_att_beam

from tensorflow_end2end_speech_recognition_amd.models.attention.decoders.beam_search import util as U
from tensorflow_end2end_speech_recognition_amd.models.attention.decoders.beam_search.beam_search_decoder import (
    BeamSearchDecoder, beam_search_step, cut_at_eos, initial_beam_state)
from tensorflow_end2end_speech_recognition_amd.models.attention.decoders.beam_search.namedtuple import (
    BeamSearchDecoderOutput, BeamSearchDecoderState, BeamSearchStepOutput, FinalBeamDecoderOutput)

META, ARR = G.load()


def test_fixture_covers_what_the_kernels_must_get_right():
    shapes = {(c['W'], c['C2']) for c in META.values() if c['kind'] == 'chain'}
    assert shapes == set(G.SHAPES) and {c['alpha'] for c in META.values()} == set(G.ALPHAS)
    assert set(META) == set(G.cases())
    all_done = 0
    for name, c in META.items():
        assert 1 <= c['steps'] <= 10 and (c['kind'] == 'tie' or c['steps'] >= 6)
        fin = ARR[name + '|out_finished']
        if c['kind'] == 'chain':
            assert c['min_gap'] > G.MARGIN
            all_done += bool(fin[-2].all())
            if c['W'] > 1 and c['all_eos_from'] is None:
                first = np.where(fin.any(0), fin.argmax(0), 99)
                assert len(set(first.tolist())) >= 2, name          # slots finish at different steps
        for k in ('score', 'in_log_probs', 'out_log_probs'):
            assert np.abs(ARR[name + '|' + k]).max() < 64
    assert all_done >= 1
    tie = ARR['tie_W3_C7|score'][0]
    assert tie[0] == tie[1] and ARR['tie_W3_C7|parent'][0].tolist()[:2] == [0, 1]


@pytest.mark.parametrize('name', sorted(G.cases()))
def test_host_statement_reproduces_the_reference(name):
    """beam_search_step / mask_probs / normalize_score / gather_tree_py on torch tensors in fp64, every step fed the
    fixture's own input state: ids, parents, finished and lengths exactly, scores and log_probs to 1e-12."""
    c = META[name]
    W, C2, eos = c['W'], c['C2'], c['C2'] - 1
    a = lambda f: ARR[name + '|' + f]                                                  # noqa: E731
    for s in range(c['steps']):
        x = torch.tensor(G.logits(name, c, s, c['seeds'][s]))
        state = BeamSearchDecoderState(torch.tensor(a('in_log_probs')[s]), torch.tensor(a('in_finished')[s]),
                                       torch.tensor(a('in_lengths')[s]))
        out, nxt = beam_search_step(c['time0'] + s, x, state, W, C2, eos, c['alpha'])
        assert isinstance(out, BeamSearchStepOutput) and isinstance(nxt, BeamSearchDecoderState)
        assert out.predicted_ids.tolist() == a('word')[s].tolist(), (name, s)
        assert out.beam_parent_ids.tolist() == a('parent')[s].tolist(), (name, s)
        assert nxt.finished.tolist() == a('out_finished')[s].tolist()
        assert nxt.lengths.tolist() == a('out_lengths')[s].tolist()
        assert np.abs(out.scores.numpy() - a('score')[s]).max() <= 1e-12
        assert np.abs(nxt.log_probs.numpy() - a('out_log_probs')[s]).max() <= 1e-12
    assert np.array_equal(U.gather_tree_py(a('word'), a('parent')), a('gathered'))


def test_length_penalty_quirk_and_none():
    rng = np.random.RandomState(0)
    lp = torch.tensor(rng.randn(3, 5))
    ln = torch.tensor(rng.randint(0, 9, size=(3, 5)))
    assert torch.equal(U.normalize_score(lp, ln, 1), lp)                 # the reference's quirk: 1 means "off"
    assert torch.equal(U.normalize_score(lp, ln, 1.0), lp)
    assert torch.equal(U.normalize_score(lp, ln, None), U.normalize_score(lp, ln, 0.0))       # deviation: None is 0
    assert torch.equal(U.normalize_score(lp, ln, 0.0), lp)
    want = lp / ((5.0 + ln.double()) ** 0.999 / 6.0 ** 0.999)
    assert torch.allclose(U.normalize_score(lp, ln, 0.999), want, rtol=0, atol=1e-15)
    assert not torch.allclose(U.normalize_score(lp, ln, 0.999), lp, atol=1e-3)                 # ... and only exactly 1
    masked = U.mask_probs(lp, 4, torch.tensor([False, True, False]))
    assert torch.equal(masked[0], lp[0]) and masked[1].tolist() == [U.F32_MIN] * 4 + [0.0]


def test_beam_width_validation(monkeypatch):
    for bad, C2 in ((0, 9), (33, 100), (12, 11), (4, 3)):
        with pytest.raises(ValueError):
            U.check_beam_width(bad, C2)
    assert U.check_beam_width(11, 11) == 11 and U.check_beam_width(32, 40) == 32
    _cpu_ops_att_beam.install(monkeypatch)
    model, x, sl = _model('bahdanau_content', 'zeros', C=5)
    with pytest.raises(ValueError):
        model.infer(x, sl, beam_width=8)                                 # > num_classes + 2 = 7
    with pytest.raises(ValueError):
        model.infer(x, sl, beam_width=33)
    with pytest.raises(ValueError):
        BeamSearchDecoder(None, 8, 7, 6, 0.0, 5)
    assert FinalBeamDecoderOutput._fields == ('predicted_ids', 'beam_search_output')
    assert BeamSearchDecoderOutput._fields == ('logits', 'predicted_ids', 'log_probs', 'scores', 'beam_parent_ids',
                                               'original_outputs')
    assert initial_beam_state(3).lengths.tolist() == [0, 0, 0]


def _model(att, prev, C=9, eos_bias=None, cls=None, seed=5, **kw):
    from tensorflow_end2end_speech_recognition_amd.models.attention.attention_seq2seq import AttentionSeq2Seq
    rng = np.random.RandomState(seed)
    B, T, D, H, U_, A, Em = 4, 11, 6, 8, 12, 10, 4
    model = (cls or AttentionSeq2Seq)(
        input_size=D, encoder_type='blstm', encoder_num_units=H, encoder_num_layers=1, encoder_num_proj=None,
        attention_type=att, attention_dim=A, decoder_type='lstm', decoder_num_units=U_, decoder_num_layers=1,
        embedding_dim=Em, num_classes=C, sos_index=C, eos_index=C + 1, max_decode_length=9, parameter_init=0.5,
        clip_grad_norm=5.0, clip_activation_encoder=50, clip_activation_decoder=50, dtype='f32', seed=seed, device='cpu',
        prev_alpha=prev, **kw)
    if eos_bias is not None:
        sd = {k: v.clone() for k, v in model.store.state_dict().items()}
        sd['attention_decoder/decoder/output_layer/biases'][C + 1] = eos_bias
        model.store.load_state_dict(sd)
    sl = np.array([T, 9, 6, 3], dtype=np.int32)
    x = rng.randn(B, T, D).astype(np.float32) * (np.arange(T)[None, :, None] < sl[:, None, None])
    return model, x, sl


@pytest.mark.parametrize('att,prev,eos_bias', [('bahdanau_content', 'zeros', 0.6), ('location', 'carry', 0.6),
                                               ('hybrid', 'carry', -50.0), ('luong_general', 'zeros', 50.0)])
def test_beam_width_one_is_the_greedy_decode(monkeypatch, att, prev, eos_bias):
    """The anchor: _decode_beam(beam_width=1) goes through tiling, select, reorder and back-trace and must return what
    infer() returns up to and including each row's first <EOS> (both pad with zeros behind it)."""
    _cpu_ops_att_beam.install(monkeypatch)
    model, x, sl = _model(att, prev, eos_bias=eos_bias)
    greedy = model.infer(x, sl)
    beam = model.infer(x, sl, beam_width=1)                               # (takes the greedy path: untouched)
    assert np.array_equal(greedy, beam)
    model.encoder._lens_host = sl
    got = model._decode_beam(torch.tensor(x), torch.tensor(sl), 1)
    eos = model.eos_index
    for b in range(len(sl)):
        assert cut_at_eos(got[b], eos) == cut_at_eos(greedy[b], eos), (b, got[b], greedy[b])
        n = len(cut_at_eos(got[b], eos))
        assert not got[b][n:].any()
    raw = model._beam_raw
    assert raw['ids'].shape == (4, 1, 9) and raw['steps_issued'] >= got.shape[1]
    if eos_bias == 50.0:
        assert got.shape[1] == 1
    if eos_bias == -50.0:
        assert got.shape[1] == 9


@pytest.mark.parametrize('cls', ['attention', 'joint'])
def test_beam_search_never_scores_below_greedy(monkeypatch, cls):
    """infer(beam_width=4): per utterance the best hypothesis' score is >= the greedy hypothesis' score under the same
    statement (alpha = 0: the score is the total log-probability; the greedy path's is read off a width-1 search)."""
    _cpu_ops_att_beam.install(monkeypatch)
    kw = {}
    if cls == 'joint':
        from tensorflow_end2end_speech_recognition_amd.models.attention.joint_ctc_attention import JointCTCAttention
        kw = dict(cls=JointCTCAttention, lambda_weight=0.5)
    model, x, sl = _model('bahdanau_content', 'zeros', eos_bias=0.3, **kw)
    best = model.infer(x, sl, beam_width=4)
    raw4 = model._beam_raw
    assert raw4['ids'].shape == (4, 4, 9) and raw4['beam_width'] == 4
    assert np.array_equal(best, raw4['ids'][:, 0, :best.shape[1]])
    assert (np.diff(raw4['scores'], axis=1) <= 0).all()                   # slots are in score order
    model.encoder._lens_host = sl
    model._decode_beam(torch.tensor(x), torch.tensor(sl), 1)
    raw1 = model._beam_raw
    assert (raw4['scores'][:, 0] >= raw1['scores'][:, 0] - 1e-6).all(), (raw4['scores'][:, 0], raw1['scores'][:, 0])
    assert (raw4['scores'][:, 0] > raw1['scores'][:, 0] + 1e-4).any() or np.array_equal(raw4['ids'][:, 0], raw1['ids'][:, 0])


def test_beam_search_decoder_class_surface(monkeypatch):
    """BeamSearchDecoder drives the statement over a step function: step 0 continues slot 0 alone, the back-traced
    hypotheses are gather_tree_py of the per-step record, and their lengths are the state's."""
    _cpu_ops_att_beam.install(monkeypatch)
    rng = np.random.RandomState(2)
    W, C2, eos, steps = 3, 8, 7, 6
    table = torch.tensor(rng.uniform(-2, 2, size=(steps, C2, C2)))        # logits depend on the step and the last word

    def step_fn(k, word, parent, state):
        last = torch.full((W,), C2 - 2, dtype=torch.long) if word is None else word
        return table[k][last], state

    dec = BeamSearchDecoder(step_fn, W, C2, eos, 0.6, steps)
    final, (_, beam) = dec(None)
    assert final.predicted_ids.shape[1] == W and dec.min_margin > 0
    first = torch.log_softmax(table[0][C2 - 2], -1)                       # step 0: slot 0's W best classes, in order
    assert final.beam_search_output.predicted_ids[0].tolist() == torch.sort(first, descending=True)[1][:W].tolist()
    assert beam.lengths.tolist() == [len([v for v in cut_at_eos(final.predicted_ids[:, w], eos) if v != eos]) for w in range(W)]
    assert np.array_equal(final.predicted_ids, U.gather_tree_py(final.beam_search_output.predicted_ids,
                                                                final.beam_search_output.beam_parent_ids))


def test_timit_eval_attention_with_beam_width(monkeypatch, tmp_path):
    """examples/timit/evaluation/eval_attention.py --beam_width 3 end to end on the synthetic corpus: equals scoring
    the trained model object with do_eval_per(beam_width=3); the default stays the greedy decode."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import test_host_logic as thl
    _cpu_ops_att_beam.install(monkeypatch)
    corpus = str(tmp_path / 'corpus')
    thl._make_timit_like(corpus, np.random.RandomState(0), n_train=8, n_dev=2, n_test=3, multitask=False)
    from examples.timit.training import train_attention as drv
    cfg = thl._recipe_cfg(root, 'examples/timit/config/attention/blstm_attention_phone61.yml', tmp_path,
                          encoder_num_units=8, encoder_num_layers=1, attention_dim=6, decoder_num_units=8,
                          embedding_dim=4, max_decode_length=10, dropout_encoder=0.0, dropout_decoder=0.0,
                          dropout_embedding=0.0, input_size=6, batch_size=8, num_epoch=1, eval_start_epoch=1, print_step=2,
                          optimizer='adam', learning_rate=0.02, weight_decay=0, decay_start_epoch=2, dtype='f32',
                          device='cpu', dataset_root=corpus, sort_stop_epoch=2)
    res = drv.main(cfg, str(tmp_path / 'runs'))
    run, model = res['save_path'], res['model']
    from examples.timit.evaluation import eval_attention
    from examples.timit.metrics.attention import do_eval_per
    from examples.timit.training.train_attention import make_datasets
    from tensorflow_end2end_speech_recognition_amd.utils.training.checkpoint import Saver
    Saver().save(model, os.path.join(run, 'model.ckpt'), global_step=99)
    map_dir = os.path.join(run, 'mapping_files')
    params = dict(label_type='phone61', splice=1, num_stack=1, num_skip=1, batch_size=8, num_epoch=1, sort_stop_epoch=1,
                  dataset_root=corpus)
    test_data = make_datasets(drv.Dataset, params, map_dir)[2]
    ev = dict(is_test=True, eval_batch_size=1, map_dir=map_dir)
    want3 = do_eval_per(None, None, None, model, test_data, 'phone61', beam_width=3, **ev)
    assert model._beam_raw['beam_width'] == 3
    want1 = do_eval_per(None, None, None, model, test_data, 'phone61', **ev)
    got3 = eval_attention.main([run, '--device', 'cpu', '--beam_width', '3'])
    got3p = eval_attention.main([run, '--device', 'cpu', '--beam_width', '3', '--length_penalty_weight', '0.6'])
    got1 = eval_attention.main([run, '--device', 'cpu'])
    assert abs(got3 - want3) < 1e-9 and abs(got1 - want1) < 1e-9 and got3p >= 0
