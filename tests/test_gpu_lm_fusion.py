"""GPU: shallow fusion of an RNN language model into the attention beam search (csrc/lm_fusion.hip, csrc/att_beam.hip) -- the LM step, the
fused selection step by step and the LM-state re-ordering against the float64 statement
(models/attention/decoders/beam_search/lm_fusion.py through tests/_cpu_ops_lm.py), the native loop
(asr_att_decoder_beam_lm) against the step-by-step statement, infer(lm=, lm_weight=) against the statement driven by
oracle.attention, the oracle's CTC head and the float64 LM, and RNNLM training against a float64 restatement.

The fp32 bound.  BOUND = max(1e-4, 4 x E) where E is the largest error of a numpy float32 emulation of the candidates and
rank kernels' stated operation order (tests/_cpu_ops_lm.emulate_select32, with _cpu_ops_att_joint.emulate_score32 for the
CTC term) against the float64 statement on the selection test's own shapes and seeds: E = 5.36e-6
(scripts/probe_lm_fusion.py --bound; asserted on the CPU by tests/test_lm_fusion_host.py::test_fp32_bound_of_the_gpu_tests),
the factor 4 is for the device's expf / logf differing from numpy's by a few ulp per call, and 1e-4 is the project's bar
for beam scores.  4 x E = 2.1e-5, so BOUND = 1e-4.  All finite values stay below 64 in magnitude (asserted).  Exact
comparisons of ids are made only under seeds whose float64 selection margin is at least 10 x BOUND (asserted first)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _cpu_ops_att_joint as J
import _cpu_ops_lm as M
import _lm_oracle as LO
from tensorflow_end2end_speech_recognition_amd.models.attention.decoders.beam_search import lm_fusion as LF

pytestmark = pytest.mark.gpu

I32 = torch.int32
BOUND = 1e-4
MARGIN = 10 * BOUND
MU = M.LM_WEIGHT


def _dev(a, dtype, cuda):
    return torch.tensor(np.asarray(a), dtype=dtype, device=cuda)


# ------------------------------------------------------------------------------------------------------- the LM step
@pytest.mark.parametrize('R,Em,L', [(6, 8, 1), (6, 8, 2), (40, 8, 1), (40, 8, 2), (6, 64, 2)])
def test_lm_step_against_the_float64_step(cuda, R, Em, L):
    """ops.lm_step (asr_lm_prep + asr_lm_step) at H = 64, 12 classes, cell clip on, from a random non-zero state: logits and
    the new state within 2e-5 x max(1, |reference|) of lm_fusion.lm_step, the forward bar of the attention kernels against
    float64 (tests/test_gpu_attention.py:187, :360).  The path of every layer is asserted through asr_att_path_counts: R = 6
    rows run product + cell as one launch where the layer's K = Din + H is a multiple of 64 (Em_lm = 8: layer 0 has K = 72
    and falls back, layer 1 has K = 128; Em_lm = 64: both fused), R = 40 rows exceed the fused kernel's 32 and run
    asr_gemm_act + asr_lstm_cell_fwd_ex."""
    from tensorflow_end2end_speech_recognition_amd import ops
    rng = np.random.RandomState(100 * R + Em + L)
    H, C2 = 64, 12
    p = M.lm_params(rng, C2, Em, H, L, clip=1.5)
    words = rng.randint(0, C2, size=R)
    c0, h0 = (rng.randn(L, R, H) * 1.2).astype(np.float32), (rng.randn(L, R, H) * 0.5).astype(np.float32)
    want_lg, (want_c, want_h) = LF.lm_step(p, words, (c0.astype(np.float64), h0.astype(np.float64)))
    assert (np.abs(want_c) == 1.5).any() and (np.abs(want_c) < 1.5).any()                 # the clip is reached, not everywhere
    ops.reset_att_path_counts(0)
    ops.reset_att_lm_counts(0)
    lg, c1, h1 = ops.lm_step(M.params_torch(p, cuda), _dev(words, I32, cuda), _dev(c0, torch.float32, cuda),
                             _dev(h0, torch.float32, cuda))
    counts = {k: v for k, v in ops.att_path_counts(0).items() if v}
    fused = sum(1 for l in range(L) if R <= 32 and ((Em if l == 0 else H) + H) % 64 == 0)
    want_counts = {k: v for k, v in (('fwd_cell_f32img', fused), ('fwd_cell_gemm', L - fused)) if v}
    assert counts == want_counts, (counts, want_counts)
    assert ops.att_lm_counts(0) == dict(lm_step=1, fused_select=0, lm_reorder=0)
    for name, g, w in (('logits', lg, want_lg), ('c', c1, want_c), ('h', h1, want_h)):
        e = float(np.abs(g.cpu().double().numpy() - w).max())
        print('lm_step R=%d Em=%d L=%d %s: error %.3g at |value| <= %.3g' % (R, Em, L, name, e, np.abs(w).max()))
        assert e < 2e-5 * max(1.0, float(np.abs(w).max())), (name, e)
    assert ops.check_async_errors(0) == 0


# ------------------------------------------------------------------------------------------------ the fused selection
@pytest.mark.parametrize('lpw', M.SELECT_LPWS)
@pytest.mark.parametrize('lam', M.SELECT_LAMS)
@pytest.mark.parametrize('W,C2', M.SELECT_CASES)
def test_fused_select_against_the_statement(cuda, W, C2, lam, lpw):
    """ops.att_beam_select_fused at lm_weight 0.3 over a 4-step search of 3 utterances (24, 9 and 3 frames; the joint select
    test's case generator plus LM logits), every step fed the statement's own input state (errors do not accumulate): word
    / parent / finished / lengths (/ last) exactly (the seed's float64 margin is asserted to be >= 10 x BOUND), score /
    log_probs / lm_score (/ ctc_score) within BOUND and below 64 in magnitude.  One launch for the three utterances equals
    one launch per utterance bit for bit; a step with some, but not all, slots finished is present; lm_weight = 0 raises."""
    from tensorflow_end2end_speech_recognition_amd import ops
    case, margin = M.select_case(W, C2, lam, lpw, M.SELECT_SEEDS[(W, C2, lam, lpw)])
    assert margin >= MARGIN, margin
    N, seq, B = case['N'], case['seq_len'], case['B']
    y, sl = _dev(case['y32'], torch.float32, cuda), _dev(seq, I32, cuda)
    assert any(s['out']['finished'].any() and not s['out']['finished'].all() for s in case['steps'])
    worst = 0.0
    ops.reset_att_lm_counts(0)
    for k, s in enumerate(case['steps']):
        o = s['out']
        a = dict(logits=_dev(s['logits'], torch.float32, cuda), lm_logits=_dev(s['lm_logits'], torch.float32, cuda),
                 log_probs=_dev(s['log_probs'], torch.float32, cuda), lm_score=_dev(s['lm_score'], torch.float32, cuda),
                 finished=_dev(s['finished'], I32, cuda), lengths=_dev(s['lengths'], I32, cuda))
        if lam > 0:
            a.update(r=_dev(s['r'], torch.float32, cuda), last=_dev(s['last'], I32, cuda),
                     ctc_score=_dev(s['ctc_score'], torch.float32, cuda))

        def run(rows, ys, sls, count=None, mu=MU):
            ctc = dict(ctc_weight=lam, y=ys, seq_len=sls, r=a['r'][rows].contiguous(), last=a['last'][rows].contiguous(),
                       ctc_score=a['ctc_score'][rows].contiguous()) if lam > 0 else {}
            return ops.att_beam_select_fused(a['logits'][rows].contiguous(), a['lm_logits'][rows].contiguous(), N, mu, lpw,
                                             s['first'], a['log_probs'][rows].contiguous(), a['finished'][rows].contiguous(),
                                             a['lengths'][rows].contiguous(), a['lm_score'][rows].contiguous(), beam_width=W,
                                             unfinished=count, **ctc)
        count = torch.zeros(1, dtype=I32, device=cuda)
        got = run(slice(None), y, sl, count)
        word, parent, score, lp, fin, ln, ls, last, ctc = got
        ints = [('word', word, o['word']), ('parent', parent, o['parent']), ('finished', fin, o['finished']),
                ('lengths', ln, o['lengths'])] + ([('last', last, o['last'])] if lam > 0 else [])
        for name, g, w_ in ints:
            assert g.cpu().reshape(-1).tolist() == np.asarray(w_).astype(np.int64).reshape(-1).tolist(), (name, k)
        assert int(count) == int((~o['finished']).sum())
        floats = [('score', score, o['score']), ('log_probs', lp, o['log_probs']), ('lm_score', ls, o['lm_score'])] + \
            ([('ctc_score', ctc, o['ctc_score'])] if lam > 0 else [])
        for name, g, w_ in floats:
            e, m = J.max_err(g.cpu().numpy().reshape(-1), np.asarray(w_).reshape(-1))
            assert m < 64 and e < BOUND, (name, k, e, m)
            worst = max(worst, e)
        if lam == 0:
            assert last is None and ctc is None
        for b in range(B):
            one = run(slice(b * W, (b + 1) * W), y[:, b:b + 1].contiguous(), sl[b:b + 1].contiguous())
            for t_all, t_one in zip(got, one):
                if t_all is not None:
                    assert torch.equal(t_all.reshape(B, W)[b], t_one.reshape(-1)), (k, b)
    assert ops.att_lm_counts(0)['fused_select'] == len(case['steps']) * (1 + B)
    print('att_beam_select_fused W=%d C2=%d ctc_weight=%g a=%g: largest error %.3g' % (W, C2, lam, lpw, worst))
    with pytest.raises(ValueError):
        run(slice(None), y, sl, mu=0.0)
    assert ops.check_async_errors(0) == 0


# --------------------------------------------------------------------------------------------- the LM-state re-ordering
def test_lm_beam_reorder_is_a_gather(cuda):
    """ops.lm_beam_reorder at L = 2, H = 64, Em_lm = 8, B = 3, W = 5: c / h and the h_prev columns of the cell-input rows are
    index_select by parent (utterance 0: slot 2 chosen three times, slots 1 and 3 by none), layer 0's x columns the embedding
    of the word, bit for bit; the sources are untouched."""
    from tensorflow_end2end_speech_recognition_amd import ops
    rng = np.random.RandomState(5)
    B, W, L, H, Em, C2 = 3, 5, 2, 64, 8, 12
    R = B * W
    parent = rng.randint(0, W, size=(B, W))
    parent[0] = [2, 2, 2, 0, 4]
    word = rng.randint(0, C2, size=(B, W))
    c_src, h_src = _dev(rng.randn(L, R, H), torch.float32, cuda), _dev(rng.randn(L, R, H), torch.float32, cuda)
    emb = _dev(rng.randn(C2, Em), torch.float32, cuda)
    c0, h0 = c_src.clone(), h_src.clone()
    ops.reset_att_lm_counts(0)
    c, h, ins = ops.lm_beam_reorder(_dev(parent, I32, cuda), _dev(word, I32, cuda), c_src, h_src, emb)
    assert ops.att_lm_counts(0) == dict(lm_step=0, fused_select=0, lm_reorder=1)
    rows = torch.tensor((np.arange(B)[:, None] * W + parent).reshape(-1), device=cuda)
    assert torch.equal(c, c_src.index_select(1, rows)) and torch.equal(h, h_src.index_select(1, rows))
    assert torch.equal(ins[0][:, :Em], emb.index_select(0, torch.tensor(word.reshape(-1), device=cuda)))
    assert torch.equal(ins[0][:, Em:], h[0]) and torch.equal(ins[1][:, H:], h[1])
    assert tuple(ins[0].shape) == (R, Em + H) and tuple(ins[1].shape) == (R, 2 * H)
    assert torch.equal(c_src, c0) and torch.equal(h_src, h0)
    assert ops.check_async_errors(0) == 0


# ------------------------------------------------------------------------------------------------ the array-level loop
@pytest.mark.parametrize('W,att,lam', sorted(M.LOOP_SEEDS))
def test_native_fused_loop_against_the_step_by_step_statement(cuda, W, att, lam):
    """ops.att_decoder_beam_lm at lm_weight 0.3, length penalty 0.6, against _cpu_ops_lm._att_decoder_beam_lm (the beam loop
    test's operands -- B = 3, T = 40, U = 64, 12 classes, 12 steps -- with and without carried attention weights, an LM of
    H = 64, L = 2, Em_lm = 8, and for ctc_weight 0.3 CTC posteriors [40,3,11]): the statement's margin is asserted to be
    >= 10 x BOUND first; then word, parent, the back-traced ids and the integer state are exact and score / log_probs /
    lm_score (/ ctc_score) within BOUND.  One utterance has finished early while another searches to the last step;
    check_every = 4 gives what check_every = 0 gives; the counters show per issued step one LM step, one fused selection,
    one LM re-ordering, one attention re-ordering, one state advance iff CTC, and no launch of the plain or the joint
    selection; two runs are bit-identical."""
    import test_gpu_att_beam as tb
    from tensorflow_end2end_speech_recognition_amd import ops
    seed = M.LOOP_SEEDS[(W, att, lam)]
    a, head, eos = tb.beam_loop_arrays(W, False, att, seed)
    y32, _ = J.loop_posteriors(seed)
    y_cpu, sl_cpu = torch.tensor(y32), torch.tensor(J.LOOP_SEQ, dtype=I32)
    lmp = M.loop_lm(seed)
    To = a['To']
    ref = M._att_decoder_beam_lm(tb._clone(a), head['W_av'], head['W_out'], head['b_out'], head['embedding'], eos, W,
                                 M.params_torch(lmp), MU, 0.6, check_every=0, y=y_cpu, seq_len=sl_cpu, ctc_weight=lam)
    assert ref['min_margin'] >= MARGIN, ref['min_margin']
    done_at = tb.done_after(ref, eos)
    assert min(done_at) < To and max(done_at) == To, done_at
    y, sl, lm_dev = y_cpu.to(cuda), sl_cpu.to(cuda), M.params_torch(lmp, cuda)
    ctc = dict(y=y, seq_len=sl, ctc_weight=lam) if lam > 0 else {}

    def run(check_every):
        ga, gh = tb._clone(a, cuda), tb._clone(head, cuda)
        out = ops.att_decoder_beam_lm(ga, gh['W_av'], gh['W_out'], gh['b_out'], gh['embedding'], eos, W, lm_dev, MU, 0.6,
                                      check_every=check_every, **ctc)
        torch.cuda.synchronize()
        return out
    ops.reset_att_joint_counts(0)
    ops.reset_att_beam_counts(0)
    ops.reset_att_lm_counts(0)
    got = run(0)
    assert got['steps_issued'] == To
    assert ops.att_lm_counts(0) == dict(lm_step=To, fused_select=To, lm_reorder=To)
    assert ops.att_beam_counts(0) == dict(select=0, reorder=To, backtrace=1)
    n_ctc = To if lam > 0 else 0
    assert ops.att_joint_counts(0) == dict(score=n_ctc, advance=n_ctc, joint_select=0)
    for k in ('word', 'parent', 'ids', 'hyp_len', 'finished', 'lengths'):
        assert torch.equal(got[k].cpu(), ref[k]), k
    assert torch.equal(got['unfinished'].cpu()[1:], ref['unfinished'][1:])
    floats = ('score', 'final_score', 'log_probs', 'lm_score') + (('ctc_score',) if lam > 0 else ())
    for k in floats:
        e, m = J.max_err(got[k].cpu().numpy(), ref[k].double().numpy())
        print('fused loop W=%d %s ctc_weight=%g %s: error %.3g at |value| <= %.3g' % (W, att, lam, k, e, m))
        assert m < 64 and e < BOUND, (k, e, m)
    again = run(0)
    for k in ('word', 'parent', 'score', 'ids', 'hyp_len', 'finished', 'lengths') + floats:
        assert torch.equal(again[k], got[k]), k
    early = run(4)
    n2 = early['steps_issued']
    assert 1 <= n2 <= To
    for k in ('ids', 'hyp_len', 'finished', 'lengths') + floats[1:]:
        assert torch.equal(early[k], got[k]), k
    for k in ('word', 'parent', 'score'):
        assert torch.equal(early[k][:n2], got[k][:n2]), k
    assert ops.check_async_errors(0) == 0


# ------------------------------------------------------------------------------------------------------- model level
LM_SHAPE = dict(embedding_dim=8, num_units=64, num_layers=2)


def _language_model(C, seed, device):
    """An fp32 RNNLM (H = 64, L = 2) over the model's classes whose output layer is scaled by 20 and embedding by 10, so that
    the LM moves the ranking."""
    from tensorflow_end2end_speech_recognition_amd.models.lm.base import RNNLM
    lm = RNNLM(num_classes=C + 2, sos_index=C, eos_index=C + 1, clip_activation=50, seed=seed + 1, device=device, **LM_SHAPE)
    lsd = {k: v.clone() for k, v in lm.store.state_dict().items()}
    lsd['rnnlm/output/weights'] *= 20.0
    lsd['rnnlm/embedding/W_embedding'] *= 10.0
    lm.store.load_state_dict(lsd)
    return lm, lsd


def attention_model(dtype, seed, device, max_decode_length=12):
    """AttentionSeq2Seq as test_gpu_att_beam._model builds one (H = 64, U = 128, 9 labels, B = 5, T = 70; location attention
    with carried weights) on `device`, its output layer scaled by 40 and the <EOS> bias 0.35 as
    test_model_beam_search_against_the_oracle_statement sets them."""
    from tensorflow_end2end_speech_recognition_amd.models.attention.attention_seq2seq import AttentionSeq2Seq
    rng = np.random.RandomState(seed)
    B, T, D, H, L, U, A, Em, C = 5, 70, 12, 64, 1, 128, 32, 8, 9
    sl = rng.randint(T // 2, T + 1, size=B).astype(np.int32)
    sl[0] = T
    x = (rng.randn(B, T, D) * (np.arange(T)[None, :, None] < sl[:, None, None])).astype(np.float32)
    model = AttentionSeq2Seq(input_size=D, encoder_type='blstm', encoder_num_units=H, encoder_num_layers=L,
                             encoder_num_proj=None, attention_type='location', attention_dim=A, decoder_type='lstm',
                             decoder_num_units=U, decoder_num_layers=1, embedding_dim=Em, num_classes=C, sos_index=C,
                             eos_index=C + 1, max_decode_length=max_decode_length, parameter_init=0.1, clip_grad_norm=5.0,
                             clip_activation_encoder=50, clip_activation_decoder=50, dtype=dtype, seed=seed,
                             sharpening_factor=1.5, prev_alpha='carry', device=device)
    sd = {k: v.clone() for k, v in model.store.state_dict().items()}
    sd['attention_decoder/decoder/output_layer/weights'] *= 40.0
    sd['attention_decoder/decoder/output_layer/biases'][C + 1] = 0.35
    model.store.load_state_dict(sd)
    return model, x, sl, C, sd


def fused_models(dtype, seed, device, joint=True):
    """joint: test_gpu_att_joint.joint_model (a JointCTCAttention; H = 64, U = 128, 9 labels, B = 5, T = 70); otherwise
    attention_model (an AttentionSeq2Seq of the same size) -- and the language model over its classes."""
    import test_gpu_att_joint as tj
    model, x, sl, C, sd = tj.joint_model(dtype, seed, device) if joint else attention_model(dtype, seed, device)
    lm, lsd = _language_model(C, seed, device)
    return model, lm, x, sl, C, sd, lsd


def oracle_fused(sd, lsd, x, sl, C, dtype, lam):
    from oracle import lstm as olstm
    sdn = {k: v.cpu().numpy() for k, v in sd.items()}
    kw = dict(operand_round=olstm.bf16_round_t) if dtype == 'bf16' else {}
    return LO.fused_beam_infer(sdn, LO.lm_params_of(lsd, LM_SHAPE['num_layers'], 50.0), MU, x, sl, 1, 'location', C, C + 1, 12, 4,
                               0.6, ctc_weight=lam, clip_enc=50.0, clip_dec=50.0, sharpening=1.5, prev_alpha='carry', **kw)


# ctc_weight 0: AttentionSeq2Seq.infer(lm=, lm_weight=); ctc_weight 0.3: JointCTCAttention.infer(lm=, lm_weight=, ctc_weight=)
MODEL_CASES = [('f32', 0.0), ('bf16', 0.0), ('f32', 0.3), ('bf16', 0.3)]
# (dtype, ctc_weight) -> seed of models and batch under which the float64 statement's margin is >= 1e-3 for every utterance
# (asserted; found on the CPU, scripts/probe_lm_fusion.py --seeds model)
MODEL_SEEDS = {('f32', 0.0): 1, ('bf16', 0.0): 19, ('f32', 0.3): 3, ('bf16', 0.3): 7}


def find_model_seeds(margin, tries=80):
    found = {}
    for dtype, lam in MODEL_CASES:
        for seed in range(tries):
            _, _, x, sl, C, sd, lsd = fused_models(dtype, seed, 'cpu', joint=lam > 0)
            want = oracle_fused(sd, lsd, x, sl, C, dtype, lam)
            margins = [r['margin'] for r in want]
            print('model', dtype, lam, seed, min(margins), flush=True)
            if min(margins) >= margin:
                found[(dtype, lam)] = seed
                break
    return found


@pytest.mark.parametrize('dtype,lam', MODEL_CASES)
def test_model_fused_decode_against_the_oracle_statement(cuda, dtype, lam):
    """AttentionSeq2Seq.infer(beam_width=4, length_penalty_weight=0.6, lm=, lm_weight=0.3) (ctc_weight 0: a model without a CTC
    head) and JointCTCAttention.infer(..., ctc_weight=0.3), each with fp32 and bf16 operands for the acoustic model and an
    fp32 LM, equal LMFusedBeamSearchDecoder driven by oracle.attention's float64 step functions (with the bf16 model's
    rounding points), the oracle's CTC head and the float64 LM: every hypothesis of every utterance, ids exactly (the margin
    of every utterance is asserted to be >= 10 x BOUND; none is skipped), scores, lm_score and ctc_score to 1e-3 absolute,
    the bar of test_model_joint_decode_against_the_oracle_statement for both dtypes."""
    from tensorflow_end2end_speech_recognition_amd import ops
    from tensorflow_end2end_speech_recognition_amd.models.attention.joint_ctc_attention import JointCTCAttention
    model, lm, x, sl, C, sd, lsd = fused_models(dtype, MODEL_SEEDS[(dtype, lam)], cuda, joint=lam > 0)
    assert isinstance(model, JointCTCAttention) == (lam > 0)
    want = oracle_fused(sd, lsd, x, sl, C, dtype, lam)
    assert all(r['margin'] >= MARGIN for r in want), [r['margin'] for r in want]
    ops.reset_att_lm_counts(0)
    kw = dict(ctc_weight=lam) if lam > 0 else {}
    best = model.infer(x, sl, beam_width=4, length_penalty_weight=0.6, lm=lm, lm_weight=MU, **kw)
    raw = model._beam_raw
    n = raw['steps_issued']
    assert ops.att_lm_counts(0) == dict(lm_step=n, fused_select=n, lm_reorder=n)
    assert raw['ids'].shape == (5, 4, 12) and raw['lm_score'].shape == (5, 4)
    for b, r in enumerate(want):
        for w in range(4):
            k = int(raw['hyp_len'][b, w])
            assert raw['ids'][b, w, :k].tolist() == r['ids'][w], (b, w)
            assert not raw['ids'][b, w, k:].any()
        e = np.abs(raw['scores'][b] - r['scores']).max()
        el = np.abs(raw['lm_score'][b] - r['lm_score']).max()
        print('model fused %s ctc_weight=%g utterance %d: margin %.3g, score error %.3g, lm_score error %.3g'
              % (dtype, lam, b, r['margin'], e, el))
        assert e < 1e-3 and el < 1e-3
        if lam > 0:
            assert np.abs(raw['ctc_score'][b] - r['ctc_score']).max() < 1e-3
        assert best[b, :len(r['ids'][0])].tolist() == r['ids'][0]
    assert ops.check_async_errors(0) == 0


def test_lm_weight_zero_is_the_decode_without_a_language_model(cuda):
    """infer(lm=lm, lm_weight=0.0) is infer() without lm bit for bit -- greedy, beam and joint -- without one call of the
    LM-fusion entries; a language model over other classes, and lm_weight > 0 without one, raise."""
    from tensorflow_end2end_speech_recognition_amd import ops
    from tensorflow_end2end_speech_recognition_amd.models.lm.base import RNNLM
    model, lm, x, sl, C, _, _ = fused_models('f32', 7, cuda)
    ops.reset_att_lm_counts(0)
    for kw in (dict(), dict(beam_width=4, length_penalty_weight=0.6), dict(beam_width=4, length_penalty_weight=0.6, ctc_weight=0.3)):
        plain = model.infer(x, sl, **kw)
        raw_plain = model._beam_raw if kw else None
        zero = model.infer(x, sl, lm=lm, lm_weight=0.0, **kw)
        assert np.array_equal(zero, plain), kw
        if kw:
            assert np.array_equal(model._beam_raw['ids'], raw_plain['ids'])
            assert np.array_equal(model._beam_raw['scores'].view(np.int32), raw_plain['scores'].view(np.int32))
    assert ops.att_lm_counts(0) == dict(lm_step=0, fused_select=0, lm_reorder=0)
    with pytest.raises(ValueError):
        model.infer(x, sl, beam_width=4, lm_weight=0.3)
    other = RNNLM(num_classes=C + 3, sos_index=C, eos_index=C + 1, device=cuda, **LM_SHAPE)
    with pytest.raises(ValueError):
        model.infer(x, sl, beam_width=4, lm=other, lm_weight=0.3)
    assert ops.check_async_errors(0) == 0


# ------------------------------------------------------------------------------------------------- RNNLM on the device
def lm_batch(rng, B=4, Lmax=9, C=5):
    """labels [B,Lmax] (<SOS> = C first, <EOS> = C + 1 last, padded with <EOS>) with ragged lengths, one of them Lmax."""
    lens = rng.randint(3, Lmax + 1, size=B)
    lens[0] = Lmax
    labels = np.full((B, Lmax), C + 1, dtype=np.int32)
    for b, n in enumerate(lens):
        labels[b, 0] = C
        labels[b, 1:n - 1] = rng.randint(0, C, size=n - 2)
    return labels, lens.astype(np.int32)


@pytest.mark.parametrize('L,clip,wd', [(1, None, 0.0), (2, 0.6, 1e-3)])
def test_rnnlm_loss_grads_and_training(cuda, tmp_path, L, clip, wd):
    """RNNLM at B = 4, L <= 9 ragged, 7 classes, Em = 8, H = 64 against the float64 restatement (tests/_lm_oracle.py, from
    oracle.lstm's cell and layer functions): loss to 1e-4 relative, logits to 1e-4 absolute, every gradient -- the embedding
    included -- to 2e-3 of its largest entry, the fp32 bars of test_ctc_model_loss_grads_and_step
    (tests/test_gpu_model.py:46, :48, :71).  Ten optimizer steps lower the loss; perplexity is exp(loss) at zero weight
    decay; a checkpoint saved on the device restores into a fresh model with identical variables and identical logits and
    state over a chain of five steps (the fused infer with the restored LM: test_restored_lm_gives_the_same_fused_infer)."""
    from tensorflow_end2end_speech_recognition_amd.models.lm.base import RNNLM
    from tensorflow_end2end_speech_recognition_amd.utils.training.checkpoint import Saver
    rng = np.random.RandomState(11 + L)
    labels, lens = lm_batch(rng)
    mk = lambda seed: RNNLM(num_classes=7, embedding_dim=8, num_units=64, num_layers=L, sos_index=5, eos_index=6,   # noqa: E731
                            parameter_init=0.3, clip_grad_norm=5.0, clip_activation=clip, weight_decay=wd, seed=seed, device=cuda)
    model = mk(3)
    sd = {k: v.cpu().numpy() for k, v in model.store.state_dict().items()}
    ref = LO.rnnlm_reference(sd, labels, lens, L, clip, wd)
    loss, logits = model.compute_loss(labels, lens, keep_prob=1.0)
    assert abs(loss.item() - ref['total_loss']) / abs(ref['total_loss']) < 1e-4
    live = ref['live'][:, :, None]
    assert np.abs((logits.cpu().numpy() - ref['logits']) * live).max() < 1e-4
    opt = model._set_optimizer('adam', 0.01)
    for g, name in opt.compute_gradients(loss, model=model):
        r = ref['grads'][name]
        rel = np.abs(g.cpu().numpy() - r).max() / max(np.abs(r).max(), 1e-8)
        assert rel < 2e-3, (name, rel)
    if wd == 0.0:
        assert abs(model.perplexity(labels, lens) - np.exp(ref['seq_loss'])) / np.exp(ref['seq_loss']) < 1e-4
    first = None
    for _ in range(10):
        loss, _ = model.compute_loss(labels, lens, keep_prob=1.0)
        first = loss.item() if first is None else first
        model.train(loss, 'adam', 0.01)
    last, _ = model.compute_loss(labels, lens, keep_prob=1.0, is_training=False)
    assert last.item() < first
    prefix = Saver().save(model, str(tmp_path / 'model.ckpt'), global_step=1)
    fresh = mk(99)
    Saver().restore(fresh, prefix)
    for n in model.store.names:
        assert torch.equal(fresh.store[n], model.store[n]), n
    st_a, st_b = model.step_state(4), fresh.step_state(4)
    for k in range(5):                                       # a chain of steps with the carried state
        words = torch.tensor(labels[:, k], dtype=I32)
        (lg_a, st_a), (lg_b, st_b) = model.step(words, st_a), fresh.step(words, st_b)
        assert torch.equal(lg_a, lg_b) and torch.equal(st_a[0], st_b[0]) and torch.equal(st_a[1], st_b[1]), k
    from tensorflow_end2end_speech_recognition_amd import ops
    assert ops.check_async_errors(0) == 0


def test_restored_lm_gives_the_same_fused_infer(cuda, tmp_path):
    """A language model checkpoint saved on the device and restored into a fresh RNNLM gives, fused into the attention
    model's beam search, the output of the original: ids, scores and lm_score bit for bit."""
    from tensorflow_end2end_speech_recognition_amd.models.lm.base import RNNLM
    from tensorflow_end2end_speech_recognition_amd.utils.training.checkpoint import Saver
    model, lm, x, sl, C, _, _ = fused_models('f32', 1, cuda, joint=False)
    prefix = Saver().save(lm, str(tmp_path / 'model.ckpt'), global_step=3)
    fresh = RNNLM(num_classes=C + 2, sos_index=C, eos_index=C + 1, clip_activation=50, seed=77, device=cuda, **LM_SHAPE)
    Saver().restore(fresh, prefix)
    outs = []
    for m in (lm, fresh):
        ids = model.infer(x, sl, beam_width=4, length_penalty_weight=0.6, lm=m, lm_weight=MU)
        outs.append((ids, model._beam_raw['ids'].copy(), model._beam_raw['scores'].copy(), model._beam_raw['lm_score'].copy()))
    for a, b in zip(*outs):
        assert np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


# ------------------------------------------------------------------------------------------------------- determinism
def test_fused_decode_is_reproducible_across_processes(cuda):
    """The fused model-level decode (beam 4, ctc_weight 0.3, lm_weight 0.3) gives the same bytes in two fresh processes."""
    here = os.path.dirname(os.path.abspath(__file__))
    outs = []
    for _ in range(2):
        r = subprocess.run([sys.executable, os.path.join(here, '_lm_determinism_worker.py')], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(r.stdout.strip().splitlines()[-1])
    assert outs[0] == outs[1] and len(outs[0]) == 64
