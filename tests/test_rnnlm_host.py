"""CPU (the stand-ins of tests/_cpu_ops.py): RNNLM's loss and gradients against a float64 restatement, training, checkpoints,
perplexity, and the argument checks of infer(lm=, lm_weight=)."""
import numpy as np
import pytest
import torch

import _cpu_ops_lm as M
import _lm_oracle as LO
from test_gpu_lm_fusion import lm_batch


def _model(L, clip, wd, seed=3, H=16):
    from tensorflow_end2end_speech_recognition_amd.models.lm.base import RNNLM
    return RNNLM(num_classes=7, embedding_dim=8, num_units=H, num_layers=L, sos_index=5, eos_index=6, parameter_init=0.3,
                 clip_grad_norm=5.0, clip_activation=clip, weight_decay=wd, seed=seed, device='cpu')


@pytest.mark.parametrize('L,clip,wd', [(1, None, 0.0), (2, 0.6, 1e-3), (2, None, 1e-3), (1, 0.6, 0.0)])
def test_rnnlm_loss_grads_training_and_checkpoint(monkeypatch, tmp_path, L, clip, wd):
    """B = 4, L <= 9 with ragged lengths, 7 classes, Em = 8, H = 16, 1 and 2 layers, with and without cell clip and weight
    decay, against tests/_lm_oracle.rnnlm_reference (float64, from oracle.lstm's cell and layer functions): loss to 1e-4
    relative, logits to 1e-4, every gradient (the embedding's included) to 2e-3 of its largest entry -- the fp32 bars of
    test_ctc_model_loss_grads_and_step (tests/test_gpu_model.py:46, :48, :71).  Ten optimizer steps lower the loss, a
    checkpoint round-trips bit for bit, perplexity == exp(loss) at zero weight decay."""
    from tensorflow_end2end_speech_recognition_amd.utils.training.checkpoint import Saver
    M.install(monkeypatch)
    labels, lens = lm_batch(np.random.RandomState(11 + L))
    model = _model(L, clip, wd)
    names = list(model.store.names)
    assert names[0] == 'rnnlm/embedding/W_embedding' and names[-2:] == ['rnnlm/output/weights', 'rnnlm/output/biases']
    assert names[1:3] == ['rnnlm/lstm_hidden1/lstm_cell/kernel', 'rnnlm/lstm_hidden1/lstm_cell/bias']
    sd = {k: v.cpu().numpy() for k, v in model.store.state_dict().items()}
    ref = LO.rnnlm_reference(sd, labels, lens, L, clip, wd)
    loss, logits = model.compute_loss(labels, lens, keep_prob=1.0)
    assert abs(loss.item() - ref['total_loss']) / abs(ref['total_loss']) < 1e-4
    assert np.abs((logits.numpy() - ref['logits']) * ref['live'][:, :, None]).max() < 1e-4
    opt = model._set_optimizer('adam', 0.01)
    for g, name in opt.compute_gradients(loss, model=model):
        r = ref['grads'][name]
        assert np.abs(g.numpy() - r).max() / max(np.abs(r).max(), 1e-8) < 2e-3, name
    if clip:
        assert (np.abs(LO.lm_params_of(sd, L, clip)['kernels'][0]) > 0).any()
    if wd == 0.0:
        assert model.perplexity(labels, lens) == pytest.approx(float(np.exp(model.sequence_loss.item())), rel=1e-6)
        assert model.perplexity(labels, lens) == pytest.approx(float(np.exp(ref['seq_loss'])), rel=1e-4)
    first = None
    for _ in range(10):
        loss, _ = model.compute_loss(labels, lens, keep_prob=0.9)
        first = loss.item() if first is None else first
        model.train(loss, 'adam', 0.01)
    last, _ = model.compute_loss(labels, lens, keep_prob=1.0, is_training=False)
    assert last.item() < first
    prefix = Saver().save(model, str(tmp_path / 'model.ckpt'), global_step=2)
    fresh = _model(L, clip, wd, seed=99)
    Saver().restore(fresh, prefix)
    for n in names:
        assert torch.equal(fresh.store[n], model.store[n]), n
    lg_a, st_a = model.step(torch.tensor([5, 0, 3], dtype=torch.int32), model.step_state(3))
    lg_b, _ = fresh.step(torch.tensor([5, 0, 3], dtype=torch.int32), fresh.step_state(3))
    assert torch.equal(lg_a, lg_b) and tuple(lg_a.shape) == (3, 7) and tuple(st_a[0].shape) == (L, 3, 16)


def test_step_is_the_sequence_model(monkeypatch):
    """RNNLM.step, fed a sequence word by word, gives the logits compute_loss gives for it."""
    M.install(monkeypatch)
    labels, lens = lm_batch(np.random.RandomState(4))
    model = _model(2, 0.6, 0.0)
    _, logits = model.compute_loss(labels, lens, keep_prob=1.0, is_training=False)
    state = model.step_state(labels.shape[0])
    for k in range(int(lens.max()) - 1):
        lg, state = model.step(torch.tensor(labels[:, k]), state)
        live = (k < lens - 1)
        assert np.abs((lg.numpy() - logits[:, k].numpy())[live]).max() < 1e-4


def test_argument_checks(monkeypatch):
    from tensorflow_end2end_speech_recognition_amd.models.attention.attention_seq2seq import AttentionSeq2Seq
    from tensorflow_end2end_speech_recognition_amd.models.lm.base import RNNLM
    from tensorflow_end2end_speech_recognition_amd.models.lm.char_rnnlm import CharRNNLM
    from tensorflow_end2end_speech_recognition_amd.models.lm.word_rnnlm import WordRNNLM
    M.install(monkeypatch)
    with pytest.raises(ValueError):
        RNNLM(7, 8, 16, 1, 5, 6, dtype='bf16', device='cpu')
    assert CharRNNLM(7, 8, 16, 1, 5, 6, device='cpu').name == 'char_rnnlm'
    assert WordRNNLM(7, 8, 16, 1, 5, 6, device='cpu').name == 'word_rnnlm'
    C = 5
    model = AttentionSeq2Seq(input_size=6, encoder_type='blstm', encoder_num_units=16, encoder_num_layers=1,
                             encoder_num_proj=None, attention_type='bahdanau_content', attention_dim=8, decoder_type='lstm',
                             decoder_num_units=16, decoder_num_layers=1, embedding_dim=4, num_classes=C, sos_index=C,
                             eos_index=C + 1, max_decode_length=6, device='cpu')
    x, sl = np.random.RandomState(0).randn(2, 10, 6).astype(np.float32), np.array([10, 7], np.int32)
    good = RNNLM(C + 2, 8, 16, 1, C, C + 1, device='cpu')
    for bad in (RNNLM(C + 3, 8, 16, 1, C, C + 1, device='cpu'), RNNLM(C + 2, 8, 16, 1, C - 1, C + 1, device='cpu'),
                RNNLM(C + 2, 8, 16, 1, C, C, device='cpu')):
        with pytest.raises(ValueError):
            model.infer(x, sl, beam_width=2, lm=bad, lm_weight=0.3)
    with pytest.raises(ValueError):
        model.infer(x, sl, beam_width=2, lm_weight=0.3)                  # a weight without a model
    with pytest.raises(ValueError):
        model.infer(x, sl, beam_width=2, lm=good, lm_weight=-1.0)
    with pytest.raises(ValueError):
        model.infer(x, sl, beam_width=2, lm=good, lm_weight=0.3, native=False)
    plain = model.infer(x, sl, beam_width=2)
    assert np.array_equal(model.infer(x, sl, beam_width=2, lm=good, lm_weight=0.0), plain)
    fused = model.infer(x, sl, beam_width=2, lm=good, lm_weight=0.3)
    assert fused.shape[0] == 2 and model._beam_raw['lm_score'].shape == (2, 2)
