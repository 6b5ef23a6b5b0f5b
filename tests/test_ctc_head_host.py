"""CPU: host logic around the fused CTC head launches and the frames form of the weight-gradient products.  On CPU
tensors the models must keep to the launches the stand-ins of tests/_cpu_ops.py know (the new ops are reached for device
tensors only); asr_ctc_head_ok is a host function and is checked against the dispatch rule of asr_gemm it mirrors; the
encoder's bookkeeping for a deferred top-layer dropout is checked on the stand-ins."""
import numpy as np
import pytest
import torch

import _cpu_ops


def _lib():
    from tensorflow_end2end_speech_recognition_amd import _lib
    return _lib.load()


def _one_pass(rows, E, C):
    """asr_gemm's generic kernel runs [rows, E] x [E, C] in one pass over E (launch_gemm of csrc/gemm.hip)."""
    t128 = -(-rows // 128) * -(-C // 128)
    t64 = -(-rows // 64) * -(-C // 64)
    return t128 >= 320 or not (t64 < 256 and E >= 1024)


@pytest.mark.parametrize('rows', [1, 16, 208, 1120, 11920, 16320, 16384, 40960, 105600])
@pytest.mark.parametrize('E', [32, 64, 96, 128, 512, 1024, 1088])
@pytest.mark.parametrize('C', [1, 2, 3, 39, 62, 64, 65, 3387])
def test_head_ok_is_the_shape_rule(rows, E, C):
    want = E >= 64 and E % 64 == 0 and E <= 1024 and 2 <= C <= 64 and _one_pass(rows, E, C)
    assert bool(_lib().asr_ctc_head_ok(rows, E, C)) == want


def test_new_ops_are_not_cpu_stand_ins():
    """The stand-ins file knows none of the new front-end functions: model code may call them for device tensors only."""
    for name in ('ctc_head_fwd', 'ctc_loss_ex', 'ctc_head_prep', 'ctc_head_bwd', 'gemm_tn_frames'):
        assert name not in _cpu_ops.STAND_INS


def _cpu_step(monkeypatch, fused, frames):
    from tensorflow_end2end_speech_recognition_amd.models.ctc import ctc as ctc_mod
    from tensorflow_end2end_speech_recognition_amd.models.encoders.core import rnn_util
    ops = _cpu_ops.install(monkeypatch)
    monkeypatch.setattr(ctc_mod, 'HEAD_FUSED', fused)
    monkeypatch.setattr(rnn_util, 'TN_FRAMES', frames)

    def boom(*a, **k):
        raise AssertionError('a device-only launch was reached on CPU tensors')
    for name in ('ctc_head_fwd', 'ctc_loss_ex', 'ctc_head_prep', 'ctc_head_bwd', 'gemm_tn_frames'):
        monkeypatch.setattr(ops, name, boom)
    rng = np.random.RandomState(2)
    B, T, D, C = 3, 9, 12, 5
    x = rng.randn(B, T, D).astype(np.float32)
    sl = np.array([T, 4, 6], dtype=np.int32)
    dense = np.array([[0, 1, 1], [2, -1, -1], [3, 0, -1]], dtype=np.int64)
    m = ctc_mod.CTC('blstm', D, 64, 2, C, clip_grad_norm=5.0, clip_activation=50, dtype='bf16', device='cpu', seed=1)
    loss, logits = m.compute_loss(x, dense, sl, keep_prob=0.8)
    m.train(loss, 'adam', 1e-3)
    assert m.encoder._top_deferred is False and m._head_state is None
    return float(loss), logits.numpy().copy(), {k: v.numpy().copy() for k, v in m.store.state_dict().items()}


def test_cpu_tensors_keep_the_separate_launches(monkeypatch):
    a = _cpu_step(monkeypatch, True, True)
    b = _cpu_step(monkeypatch, False, False)
    assert a[0] == b[0] and np.isfinite(a[0])
    assert np.array_equal(a[1], b[1])
    for k in a[2]:
        assert np.array_equal(a[2][k], b[2][k]), k


def test_encoder_defers_only_a_descriptor_on_one_pipeline(monkeypatch):
    """defer_top_dropout leaves _out_op un-dropped and reports the descriptor; a mask TENSOR is applied as before, and
    backward(top_masked=True) skips the top layer's mask pass exactly once."""
    from tensorflow_end2end_speech_recognition_amd.models.encoders.load_encoder import load
    from tensorflow_end2end_speech_recognition_amd.utils.parameter import ParamStore
    _cpu_ops.install(monkeypatch)
    rng = np.random.RandomState(0)
    B, T, D, H = 2, 7, 12, 64
    x = torch.from_numpy(rng.randn(B, T, D).astype(np.float32))
    sl = torch.tensor([T, 3], dtype=torch.int32)

    def run(defer, masks=None):
        enc = load('blstm')(num_units=H, num_proj=None, num_layers=2, lstm_impl='LSTMBlockCell', use_peephole=True,
                            parameter_init=0.1, clip_activation=50, time_major=True, dtype='f32')
        store = ParamStore(torch.device('cpu'))
        enc.build(store, D, np.random.RandomState(4))
        store.finalize()
        enc.defer_top_dropout = defer
        enc(x, sl, 0.8, True, drop_masks=masks, rng_state=(7, 1 << 40) if masks is None else None)
        return enc
    plain, deferred = run(False), run(True)
    assert plain._top_deferred is False and plain._top_drop is None
    assert deferred._top_deferred is True and deferred._top_drop == plain.layers[-1].ctx['mask']
    assert isinstance(deferred._top_drop, tuple)
    hout = deferred._out_op
    assert torch.equal(hout, plain.layers[-1].ctx['hout'])
    from tensorflow_end2end_speech_recognition_amd import ops
    assert torch.equal(ops.dropout_apply(hout, *deferred._top_drop), plain._out_op)
    # a mask tensor is not a descriptor: applied by the layer, nothing deferred
    Bp = 16
    masks = [torch.ones((T, Bp, 2 * H)) for _ in range(2)]
    with_tensor = run(True, masks)
    assert with_tensor._top_deferred is False
    # the gradients of a masked d_outputs with top_masked equal those of the unmasked one without
    g = torch.from_numpy(rng.randn(T, Bp, 2 * H).astype(np.float32))
    plain.backward(g.clone())
    deferred.backward(ops.dropout_apply(g, *deferred._top_drop), top_masked=True)
    for name in plain.layers[0].store.names:
        assert torch.equal(plain.layers[0].store.g(name), deferred.layers[0].store.g(name)), name
