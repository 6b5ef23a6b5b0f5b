"""GPU: the CTC prefix beam search with LM fusion and an insertion bonus (csrc/ctc_beam_lm.hip) -- the frame kernel alone
against the float64 statement (models/ctc/decoders/charlm_beam_search_decoder.py) with a table LM whose logits rows the
host hands to both sides; the whole native call (asr_ctc_beam_decode_lm) against the statement with the float64
restatement of the RNNLM; bit identity with asr_ctc_beam_decode at lm_weight = insertion_bonus = 0; the bonus alone;
padded batches on a poisoned workspace; CTC.decoder(lm=) on a small BLSTM-CTC model.

The fp32 bound.  The search itself is fp64 on both sides; what is fp32 is the LM (its step, and the running sum of the LM
total).  BOUND = max(1e-4, 4 x E), E = the largest error of a numpy float32 emulation of the LM propagated through the
statement to score and lm_score on the native-call test's own cases: E = 8.8e-6 (scripts/probe_ctc_beam_lm.py --bound;
asserted on the CPU by tests/test_ctc_lm_fusion_host.py::test_bound_of_the_gpu_tests), so BOUND = 1e-4.  Labels are compared
only under seeds whose float64 min_margin is at least MARGIN = 10 x BOUND (asserted first; seeds fixed in
tests/_cpu_ops_ctc_lm.py, found on the CPU).  The frame-kernel test compares fp64 with fp64: neighbouring totals are
either exactly equal or 1e-9 apart (asserted on the CPU and again here)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _cpu_ops_ctc_lm as K
import _lm_oracle as LO
from oracle import decoders as odec

pytestmark = pytest.mark.gpu

S = K.S
I32 = torch.int32
BOUND = 1e-4
MARGIN = 10 * BOUND


def _dev(a, dtype, cuda):
    return torch.tensor(np.asarray(a), dtype=dtype, device=cuda)


def _labels(lab, n):
    lab, n = lab.cpu().numpy(), n.cpu().numpy()
    for b in range(lab.shape[0]):
        assert (lab[b, int(n[b]):] == -1).all() and (lab[b, :int(n[b])] >= 0).all()
    return [lab[b, :int(n[b])].tolist() for b in range(lab.shape[0])]


# ----------------------------------------------------------------------------------------------- 1. the frame kernel
def _close64(got, want):
    if want == -np.inf or got == -np.inf:
        return got == want
    return abs(got - want) <= 1e-9 * max(1.0, abs(want))


def _run_frames(cuda, case, W, alpha, beta):
    """Drives ops.CtcBeamLmFrames frame by frame with the table LM's rows of the slots' prefixes and compares every new
    beam with the statement's."""
    from tensorflow_end2end_speech_recognition_amd import ops
    want = K.frame_statement(case, W, alpha, beta)
    assert min(f['order_gap'] for u in want for f in u) >= K.FRAME_ORDER_GAP
    lm, seq = case['lm'], case['seq_len']
    T, B, C = case['logits'].shape
    fr = ops.CtcBeamLmFrames(_dev(case['logits'], torch.float32, cuda), _dev(seq, I32, cuda), W, alpha, beta)
    prefixes = [[()] * W for _ in range(B)]
    worst = 0.0
    for t in range(T):
        rows = np.stack([lm.row(p) for b in range(B) for p in prefixes[b]])
        parent, word, pb, pnb, lmt, nb = (v.cpu().numpy() for v in fr.frame(t, _dev(rows, torch.float32, cuda)))
        for b in range(B):
            if t >= seq[b]:
                assert parent[b].tolist() == list(range(W)) and (word[b] == -1).all()
                continue
            ref = want[b][t]['beam']
            assert int(nb[b]) == len(ref), (t, b)
            old = prefixes[b]
            new = [old[parent[b, w]] + ((int(word[b, w]),) if word[b, w] >= 0 else ()) for w in range(W)]
            for w, (p, rpb, rpnb, rlm) in enumerate(ref):
                assert new[w] == p, (t, b, w, new[w], p)
                # word is -1 exactly when the prefix was in the old beam
                assert (word[b, w] < 0) == (p in old[:len(want[b][t - 1]['beam']) if t else 1]), (t, b, w)
                assert _close64(pb[b, w], rpb) and _close64(pnb[b, w], rpnb), (t, b, w, pb[b, w], rpb, pnb[b, w], rpnb)
                # an fp32 running sum of len(p) terms, each the fp32 image of a float64 difference
                assert abs(lmt[b, w] - rlm) <= 2.0 ** -23 * (len(p) + 1) * max(1.0, abs(rlm)), (t, b, w, lmt[b, w], rlm)
                if np.isfinite(rpnb):
                    worst = max(worst, abs(pnb[b, w] - rpnb) / max(1.0, abs(rpnb)))
            prefixes[b] = new[:len(ref)] + [()] * (W - len(ref))
    assert ops.check_async_errors(0) == 0
    return worst


@pytest.mark.parametrize('beta', K.FRAME_BETAS)
@pytest.mark.parametrize('alpha', K.FRAME_ALPHAS)
@pytest.mark.parametrize('C,W', K.FRAME_SHAPES)
def test_frame_kernel_against_the_statement(cuda, C, W, alpha, beta):
    """T = 12, B = 3 (12, 1 and 7 frames), table LM: after every frame the kernel's beam -- rebuilt from parent_slot / word
    alone -- is the statement's, prefix for prefix in order, with p_b / p_nb within 1e-9 relative and the fp32 LM totals
    within the rounding of an fp32 running sum."""
    worst = _run_frames(cuda, K.frame_case(C, W), W, alpha, beta)
    print('frame kernel C=%d W=%d alpha=%g beta=%g: largest relative error of p_nb %.3g' % (C, W, alpha, beta, worst))


@pytest.mark.parametrize('C,W', K.FRAME_TIE_SHAPES)
def test_frame_kernel_tie_order(cuda, C, W):
    """Logits quantised to multiples of 0.5, alpha = 1, an integer table LM: equal totals occur (at the trimming boundary
    too: asserted) and the kernel keeps the reference's insertion order among them."""
    case = K.frame_case(C, W, tie=True)
    lp = K.log_probs_btc(case['logits'])
    assert S.charlm_prefix_search(lp[0], C - 1, W, 1.0, 0.0, case['lm'], None, case['lm'].sos)['min_margin'] == 0.0
    _run_frames(cuda, case, W, 1.0, 0.0)


# -------------------------------------------------------------------------------------------- 2. the whole native call
@pytest.mark.parametrize('clip', K.LOOP_CLIPS)
@pytest.mark.parametrize('C,B,W', K.LOOP_CASES)
def test_native_call_against_the_statement(cuda, C, B, W, clip):
    """T = 24 (ragged), LM Em = 8, H = 64, L = 2 over V = C + 1 classes, with and without cell clip, alpha = 0.7,
    beta = 0.3: labels and lengths exact, score and lm_score within BOUND of the statement with the float64 RNNLM.  The
    counters show T frame launches, T LM steps (<= T + 1) and T - 1 commits; R = B W <= 32 rows take the fused
    cell-GEMM path for the layer whose K is a multiple of 64 (layer 1), R = 60 takes asr_gemm_act for both."""
    from tensorflow_end2end_speech_recognition_amd import ops
    seed = K.LOOP_SEEDS[(C, B, W, clip)]
    case = K.loop_case(C, B, W, clip, seed)
    lab, sc, lms, margin = K.loop_statement(case, W, K.LOOP_ALPHA, K.LOOP_BETA)
    assert margin >= MARGIN, margin
    lm = dict(K.M.params_torch(case['lm'], cuda), sos=case['sos'], eos=case['eos'])
    ops.reset_ctc_beam_lm_counts(0)
    ops.reset_att_path_counts(0)
    out, n, score, lm_score = ops.ctc_beam_decode_lm(_dev(case['logits'], torch.float32, cuda), _dev(case['seq_len'], I32, cuda),
                                                     W, lm=lm, lm_weight=K.LOOP_ALPHA, insertion_bonus=K.LOOP_BETA)
    counts = ops.ctc_beam_lm_counts(0)
    paths = {k: v for k, v in ops.att_path_counts(0).items() if v}
    T = K.LOOP_T
    assert counts == dict(frames=T, lm_steps=T, commits=T - 1) and counts['lm_steps'] <= T + 1
    assert paths == (dict(fwd_cell_f32img=T, fwd_cell_gemm=T) if B * W <= 32 else dict(fwd_cell_gemm=2 * T)), paths
    assert _labels(out, n) == lab
    es = float(np.abs(score.cpu().numpy() - sc).max())
    el = float(np.abs(lm_score.cpu().double().numpy() - lms).max())
    print('native call C=%d B=%d W=%d clip=%g: score error %.3g, lm_score error %.3g (margin %.3g)' % (C, B, W, clip, es, el,
                                                                                                      margin))
    assert es <= BOUND and el <= BOUND
    assert ops.check_async_errors(0) == 0


# ---------------------------------------------------------------------------------- 3. identity with the plain search
@pytest.mark.parametrize('kind', K.IDENT_KINDS)
@pytest.mark.parametrize('C,W', K.IDENT_SHAPES)
def test_zero_weights_are_the_existing_decode_bit_for_bit(cuda, C, W, kind):
    """lm_weight = 0, insertion_bonus = 0 with an LM given, and lm = None through the new op: labels, lengths and the
    score BITS of ops.ctc_beam_decode, on flat, peaked, tie-heavy and all-equal posteriors (T = 40, B = 4 ragged).  The frame kernel
    takes the log-softmax, the stay and the extension totals in beam.hip's operation order, so no tolerance is needed."""
    from tensorflow_end2end_speech_recognition_amd import ops
    x = _dev(K.ctc_logits(C + W, K.IDENT_T, len(K.IDENT_SEQ), C, kind), torch.float32, cuda)
    sl = _dev(K.IDENT_SEQ, I32, cuda)
    lm = dict(K.M.params_torch(K.M.lm_params(np.random.RandomState(C), C + 1, 8, 64, 1), cuda), sos=C)
    want = ops.ctc_beam_decode(x, sl, W)
    for kw in (dict(lm=lm, lm_weight=0.0), dict(lm=None)):
        got = ops.ctc_beam_decode_lm(x, sl, W, insertion_bonus=0.0, **kw)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert torch.equal(got[2].view(torch.int64), want[2].view(torch.int64)), (got[2], want[2])
    assert ops.check_async_errors(0) == 0


# ------------------------------------------------------------------------------------------- 4. the insertion bonus
def test_insertion_bonus_alone(cuda):
    """lm = None, beta = +0.5 / -0.5 on a fixed case: the statement's labels exactly and its scores to 1e-9; hypotheses
    get longer with the bonus and shorter with the penalty (in total, and none moves the other way)."""
    from tensorflow_end2end_speech_recognition_amd import ops
    C, B, W, T = 12, 3, 8, 24
    x = K.ctc_logits(11, T, B, C, 'flat')
    case = dict(logits=x, seq_len=K.loop_seq(B), blank=C - 1)
    ops.reset_ctc_beam_lm_counts(0)
    lens = {}
    for beta in (0.5, 0.0, -0.5):
        lab, sc, _, margin = K.loop_statement(case, W, 0.0, beta)
        assert margin >= 1e-9, margin                                            # fp64 against fp64
        out, n, score, lm_score = ops.ctc_beam_decode_lm(_dev(x, torch.float32, cuda), _dev(case['seq_len'], I32, cuda), W,
                                                         insertion_bonus=beta)
        assert _labels(out, n) == lab
        assert np.abs(score.cpu().numpy() - sc).max() <= 1e-9 * max(1.0, np.abs(sc).max())
        assert (lm_score.cpu().numpy() == 0).all()
        lens[beta] = [len(l) for l in lab]
    assert ops.ctc_beam_lm_counts(0) == dict(frames=3 * T, lm_steps=0, commits=0)
    assert all(a >= b >= c for a, b, c in zip(lens[0.5], lens[0.0], lens[-0.5])), lens
    assert sum(lens[0.5]) > sum(lens[0.0]) > sum(lens[-0.5]), lens


# ------------------------------------------------------------------------- 5. a long prefix, padding, poisoned workspace
def test_padded_batch_on_a_poisoned_workspace(cuda):
    """seq_len = (T, 1, 0): every frame of utterance 0 emits (a peaked posterior that never repeats a label: a prefix of T
    labels), utterance 1 has one frame, utterance 2 none (the empty hypothesis, score 0, lm_score 0).  Outputs beyond
    out_len are -1; a workspace that starts as NaN bit patterns gives the same bits."""
    from tensorflow_end2end_speech_recognition_amd import ops
    C, B, W, T, seed = 9, 3, 4, 24, 0
    case = K.loop_case(C, B, W, 1.5, seed)
    x = case['logits'].copy()
    x[:, 0, :] = -4.0
    x[np.arange(T), 0, np.arange(T) % (C - 1)] = 8.0                               # 0 1 2 ... 7 0 1 ...: no repeats, no blank
    case = dict(case, logits=x, seq_len=np.array([T, 1, 0], dtype=np.int32))
    lab, sc, lms, _ = K.loop_statement(case, W, K.LOOP_ALPHA, K.LOOP_BETA)
    assert lab[0] == [t % (C - 1) for t in range(T)] and len(lab[1]) <= 1 and lab[2] == [] and sc[2] == 0.0
    lm = dict(K.M.params_torch(case['lm'], cuda), sos=case['sos'], eos=case['eos'])
    args = (_dev(x, torch.float32, cuda), _dev(case['seq_len'], I32, cuda), W)
    kw = dict(lm=lm, lm_weight=K.LOOP_ALPHA, insertion_bonus=K.LOOP_BETA)
    clean = ops.ctc_beam_decode_lm(*args, **kw)
    dirty = ops.ctc_beam_decode_lm(*args, _poison=True, **kw)
    assert _labels(clean[0], clean[1]) == lab                                     # (_labels: -1 beyond out_len)
    assert np.abs(clean[2].cpu().numpy() - sc).max() <= BOUND and np.abs(clean[3].cpu().double().numpy() - lms).max() <= BOUND
    assert float(clean[2][2]) == 0.0 and float(clean[3][2]) == 0.0
    for a, b in zip(clean, dirty):
        assert torch.equal(a.view(torch.int64 if a.dtype == torch.float64 else torch.int32),
                           b.view(torch.int64 if b.dtype == torch.float64 else torch.int32))
    assert ops.check_async_errors(0) == 0


# ------------------------------------------------------------------------------------------------------ 6. the model
MODEL_SEED = 5           # under it the statement's margin over the model's own logits is >= MARGIN (asserted)


def ctc_lm_models(seed, device):
    """A 1 x 64 BLSTM-CTC model over 9 classes, a 2 x 64 RNNLM over 10, a batch of three ragged utterances."""
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    from tensorflow_end2end_speech_recognition_amd.models.lm.base import RNNLM
    C = 9
    model = CTC('blstm', 12, 64, 1, C - 1, parameter_init=0.5, clip_grad_norm=5.0, clip_activation=50, dtype='f32',
                seed=seed, device=device)
    lm = RNNLM(num_classes=C + 1, embedding_dim=8, num_units=64, num_layers=2, sos_index=C, eos_index=C - 1,
               parameter_init=0.5, clip_activation=50, seed=100 + seed, device=device)
    rng = np.random.RandomState(200 + seed)
    x = (rng.randn(3, 20, 12) * 2.0).astype(np.float32)
    sl = np.array([20, 7, 13], dtype=np.int32)
    for b in range(3):
        x[b, sl[b]:] = 0
    return model, lm, x, sl, C


def model_decode(model, lm, x, sl, beam_width=4, lm_weight=0.3):
    """(logits [T,B,C] of the model, hypotheses of CTC.decoder(lm=, lm_weight=) without the merge_repeated pass)."""
    from tensorflow_end2end_speech_recognition_amd.utils.io.labels.sparsetensor import sparsetensor2list
    _, logits = model.compute_loss(x, np.zeros((len(sl), 1), dtype=np.int64), sl, keep_prob=1.0, is_training=False)
    dec = model.decoder(logits, sl, beam_width, merge_repeated=False, lm=lm, lm_weight=lm_weight)
    return logits, [list(map(int, h)) for h in sparsetensor2list(dec, len(sl))]


def model_statement(logits, lm, sl, C, beam_width=4, lm_weight=0.3):
    params = LO.lm_params_of({k: v.cpu().numpy() for k, v in lm.store.state_dict().items()}, lm.num_layers, lm.clip_activation)
    fn, st = S.rnnlm_callable(params)
    return S.charlm_beam_search_decode(K.log_probs_btc(logits.detach().cpu().numpy()), sl, C - 1, beam_width, lm_weight, 0.0,
                                       fn, st, lm.sos_index)


def test_model_decoder_with_a_language_model(cuda, tmp_path):
    """CTC.decoder(..., lm=RNNLM, lm_weight=0.3) on a 1 x 64 BLSTM-CTC model equals the statement over the model's own
    logits (margin asserted first), and an LM restored from a checkpoint gives the same decode."""
    from tensorflow_end2end_speech_recognition_amd import ops
    from tensorflow_end2end_speech_recognition_amd.models.lm.base import RNNLM
    from tensorflow_end2end_speech_recognition_amd.utils.training.checkpoint import Saver
    model, lm, x, sl, C = ctc_lm_models(MODEL_SEED, cuda)
    ops.reset_ctc_beam_lm_counts(0)
    logits, hyp = model_decode(model, lm, x, sl)
    assert ops.ctc_beam_lm_counts(0)['frames'] == logits.shape[0]
    want, _, _, margin = model_statement(logits, lm, sl, C)
    assert margin >= MARGIN, margin
    assert hyp == want
    assert hyp != odec.beam_search_decode(K.log_probs_btc(logits.detach().cpu().numpy()), sl, C - 1, 4)[0]   # the LM matters
    prefix = Saver().save(lm, str(tmp_path / 'model.ckpt'), global_step=3)
    fresh = RNNLM(num_classes=C + 1, embedding_dim=8, num_units=64, num_layers=2, sos_index=C, eos_index=C - 1,
                  clip_activation=50, seed=77, device=cuda)
    Saver().restore(fresh, prefix)
    assert model_decode(model, fresh, x, sl)[1] == hyp
    assert ops.check_async_errors(0) == 0


def test_fused_ctc_decode_is_reproducible_across_processes(cuda):
    """The model-level decode (beam 4, lm_weight 0.3, insertion bonus 0.2) gives the same label and score bytes in two
    fresh processes."""
    here = os.path.dirname(os.path.abspath(__file__))
    outs = []
    for _ in range(2):
        r = subprocess.run([sys.executable, os.path.join(here, '_ctc_lm_determinism_worker.py')], capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(r.stdout.strip().splitlines()[-1])
    assert outs[0] == outs[1] and len(outs[0]) == 64
