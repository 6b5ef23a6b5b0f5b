"""CPU (stand-ins): the language model recipes on a generated corpus -- examples/timit/training/train_lm.py and
examples/timit/evaluation/eval_attention.py --lm_path / --lm_weight."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest

import _cpu_ops_lm as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _train_lm(thl, tmp_path, corpus):
    from examples.timit.training import train_lm
    cfg = thl._recipe_cfg(ROOT, 'examples/timit/config/lm/lstm_lm_phone61.yml', tmp_path, input_size=6, embedding_dim=4,
                          num_units=8, num_layers=1, batch_size=8, num_epoch=2, eval_start_epoch=1, print_step=2,
                          learning_rate=0.02, weight_decay=0, dropout=0.1, decay_start_epoch=2, device='cpu',
                          dataset_root=corpus, sort_stop_epoch=2)
    return train_lm.main(cfg, str(tmp_path / 'runs'))


def test_train_lm_writes_the_run_directory(monkeypatch, tmp_path):
    """train_lm.py runs two epochs on the synthetic corpus and leaves the run directory of the other recipes under
    <save>/lm/<label_type>/<name>: config.yml, train.log, loss_ler.csv, a checkpoint with its index, complete.txt; the
    restored model is the trained one bit for bit."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import test_host_logic as thl
    M.install(monkeypatch)
    corpus = str(tmp_path / 'corpus')
    thl._make_timit_like(corpus, np.random.RandomState(0), n_train=16, n_dev=4, n_test=3, multitask=False)
    res = _train_lm(thl, tmp_path, corpus)
    run = res['save_path']
    assert os.path.relpath(run, str(tmp_path / 'runs')).split(os.sep)[:2] == ['lm', 'phone61']
    for name in ('config.yml', 'train.log', 'loss_ler.csv', 'complete.txt', 'checkpoint'):
        assert os.path.isfile(os.path.join(run, name)), name
    assert res['steps'] == 4 and len(res['checkpoints']) >= 1 and len(res['ler_dev']) == 2
    assert all(0.0 < v < 1.0 for v in res['ler_dev'])
    from examples.timit.training.train_lm import restore_lm
    from tensorflow_end2end_speech_recognition_amd.utils.training.checkpoint import Saver
    Saver().save(res['model'], os.path.join(run, 'model.ckpt'), global_step=99)
    back = restore_lm(run, device='cpu')
    assert back.num_classes == 63 and back.sos_index == 61 and back.eos_index == 62
    for n in back.store.names:
        assert np.array_equal(back.store[n].numpy(), res['model'].store[n].numpy()), n


@pytest.mark.parametrize('joint', [False, True])
def test_eval_attention_with_a_language_model(monkeypatch, tmp_path, joint):
    """eval_attention.py --beam_width 3 --lm_path ... --lm_weight 0.3 runs end to end, with and without --joint --ctc_weight
    0.3, and equals scoring the model objects with do_eval_per(lm=, lm_weight=0.3); with --lm_weight 0 it prints what the
    run without --lm_path prints; --lm_weight without --lm_path is refused."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import test_host_logic as thl
    M.install(monkeypatch)
    corpus = str(tmp_path / 'corpus')
    thl._make_timit_like(corpus, np.random.RandomState(0), n_train=8, n_dev=2, n_test=3, multitask=False)
    lm_res = _train_lm(thl, tmp_path, corpus)
    if joint:
        from examples.timit.training import train_joint_ctc_attention as drv
    else:
        from examples.timit.training import train_attention as drv
    cfg = thl._recipe_cfg(ROOT, 'examples/timit/config/attention/blstm_attention_phone61.yml', tmp_path,
                          encoder_num_units=8, encoder_num_layers=1, attention_dim=6, decoder_num_units=8,
                          embedding_dim=4, max_decode_length=10, dropout_encoder=0.0, dropout_decoder=0.0,
                          dropout_embedding=0.0, input_size=6, batch_size=8, num_epoch=1, eval_start_epoch=1, print_step=2,
                          optimizer='adam', learning_rate=0.02, weight_decay=0, decay_start_epoch=2, dtype='f32',
                          device='cpu', dataset_root=corpus, sort_stop_epoch=2)
    res = drv.main(cfg, str(tmp_path / 'runs'))
    run, model, lm_run, lm = res['save_path'], res['model'], lm_res['save_path'], lm_res['model']
    from examples.timit.evaluation import eval_attention
    from examples.timit.metrics.attention import do_eval_per
    from examples.timit.training.train_attention import make_datasets
    from tensorflow_end2end_speech_recognition_amd.utils.training.checkpoint import Saver
    Saver().save(model, os.path.join(run, 'model.ckpt'), global_step=99)
    Saver().save(lm, os.path.join(lm_run, 'model.ckpt'), global_step=99)
    map_dir = os.path.join(run, 'mapping_files')
    params = dict(label_type='phone61', splice=1, num_stack=1, num_skip=1, batch_size=8, num_epoch=1, sort_stop_epoch=1,
                  dataset_root=corpus)
    test_data = make_datasets(drv.Dataset, params, map_dir)[2]
    extra = ['--joint', '--ctc_weight', '0.3'] if joint else []
    kw = dict(ctc_weight=0.3) if joint else {}
    want = do_eval_per(None, None, None, model, test_data, 'phone61', beam_width=3, lm=lm, lm_weight=0.3, is_test=True,
                       eval_batch_size=1, map_dir=map_dir, is_jointctcatt=joint, **kw)
    assert 'lm_score' in model._beam_raw and ('ctc_score' in model._beam_raw) == joint
    base = [run, '--device', 'cpu', '--beam_width', '3'] + extra
    got = eval_attention.main(base + ['--lm_path', lm_run, '--lm_weight', '0.3'])
    assert abs(got - want) < 1e-9

    def printed(argv):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            eval_attention.main(argv)
        return buf.getvalue()
    assert printed(base + ['--lm_path', lm_run, '--lm_weight', '0']) == printed(base)
    with pytest.raises(SystemExit):
        eval_attention.main(base + ['--lm_weight', '0.3'])
