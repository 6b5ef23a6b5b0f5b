"""GPU: joint CTC / attention beam search (csrc/ctc_prefix.hip, csrc/att_beam.hip) -- the prefix scorer and the state advance against the
float64 statement (models/attention/decoders/beam_search/ctc_prefix_score.py through tests/_cpu_ops_att_joint.py), the
joint selection step by step, the native loop (asr_att_decoder_beam_joint) against the step-by-step statement, and
JointCTCAttention.infer(ctc_weight=...) against the statement driven by oracle.attention and the oracle's CTC head.

The fp32 bound.  BOUND = max(1e-4, 4 x E) where E is the largest error of a numpy float32 emulation of the kernels' stated
operation order (tests/_cpu_ops_att_joint.emulate_score32 / emulate_advance32) against the float64 statement on the
scorer test's own shapes: E = 1.36e-5 (scripts/probe_att_joint.py --bound; asserted on the CPU by
tests/test_att_joint_host.py::test_fp32_bound_of_the_gpu_tests), the factor 4 is for the device's expf / logf differing
from numpy's by a few ulp per call over T chained calls, and 1e-4 is the project's bar for beam scores.  4 x E = 5.4e-5,
so BOUND = 1e-4.  All finite values stay below 64 in magnitude (asserted), where an fp32 ulp is at most 3.8e-6.
Exact comparisons of ids are made only under seeds whose float64 selection margin is at least 10 x BOUND (asserted)."""
import numpy as np
import pytest
import torch

import _cpu_ops_att_joint as J

pytestmark = pytest.mark.gpu

I32 = torch.int32
BOUND = 1e-4
MARGIN = 10 * BOUND


def _dev(a, dtype, cuda):
    return torch.tensor(np.asarray(a), dtype=dtype, device=cuda)


# ------------------------------------------------------------------------------------------- scorer and state advance
@pytest.mark.parametrize('W,Cc', J.PREFIX_CASES)
def test_prefix_score_and_advance_against_the_statement(cuda, W, Cc):
    """ops.ctc_prefix_score and ops.ctc_prefix_advance on tests/_cpu_ops_att_joint.prefix_case: T = 70 (crosses the
    64-frame chunk), B = 6 with seq_len 70, 65, 64, 63, 2, 1, hypotheses of depth 0, 1 and 3 (some no longer fit the 2- and
    1-frame utterances), a finished row, candidates that always hold the hypothesis's own last label, <SOS> and <EOS>.
    Infeasible entries and <SOS> are exactly -inf, nothing is NaN, finite entries are within BOUND (module docstring).
    The state of the selected hypotheses (a parent chosen three times, parents chosen by none) is within BOUND, rows
    copied for <EOS> / a finished parent are bit-identical to their source, and the sources are untouched.  r is handed
    over with NaN behind every utterance's last frame: nothing there may be read."""
    from tensorflow_end2end_speech_recognition_amd import ops
    c = J.prefix_case(W, Cc)
    N, seq = c['N'], c['seq_len']
    y = _dev(c['y32'], torch.float32, cuda)
    sl = _dev(seq, I32, cuda)
    r = _dev(c['r'], torch.float32, cuda)                    # NaN at t >= T_b
    last, fin = _dev(c['last'], I32, cuda), _dev(c['finished'], I32, cuda)
    cand = _dev(c['cand'], I32, cuda)
    ops.reset_att_joint_counts(0)
    psi = ops.ctc_prefix_score(y, sl, r, last, fin, cand, N)
    e, m = J.max_err(psi.cpu().numpy(), c['psi'])
    print('ctc_prefix_score W=%d Cc=%d: largest |psi error| %.3g at |psi| <= %.3g' % (W, Cc, e, m))
    assert m < 64 and e < BOUND, (e, m)
    assert torch.isinf(psi[:, 1]).all()                      # <SOS>
    r0 = r.clone()
    nxt = ops.ctc_prefix_advance(y, sl, r, last, _dev(c['parent'], I32, cuda), _dev(c['word'], I32, cuda), N)
    assert ops.att_joint_counts(0) == dict(score=1, advance=1, joint_select=0)
    e2, m2 = J.max_err(nxt.cpu().numpy(), c['r_next'])
    print('ctc_prefix_advance W=%d Cc=%d: largest |state error| %.3g at |r| <= %.3g' % (W, Cc, e2, m2))
    assert m2 < 64 and e2 < BOUND, (e2, m2)
    assert torch.equal(r.view(I32), r0.view(I32))            # out of place
    got, src, copied = nxt.cpu().numpy(), r.cpu().numpy(), 0
    for b in range(c['B']):
        for w in range(W):
            if c['word'][b, w] == N + 1:
                p = b * W + c['parent'][b, w]
                assert np.array_equal(got[b * W + w, :, :seq[b]].view(np.int32), src[p, :, :seq[b]].view(np.int32)), (b, w)
                copied += 1
    assert copied > 0
    # the empty hypothesis from the device: the blank prefix sum, summed in ascending t
    r_i, last_i, score_i = ops.ctc_prefix_init(y, sl, W)
    want_r, _, _ = J.arrays_of(J.init64(c['y'], seq, W, c['blank']), c['T'])
    e3, _ = J.max_err(r_i.cpu().numpy(), want_r)
    assert e3 < BOUND and (last_i.cpu() == -1).all() and (score_i.cpu() == 0).all()
    with pytest.raises(ValueError):
        ops.ctc_prefix_score(y, sl, r, last, fin, cand, Cc)  # more labels than CTC classes
    with pytest.raises(ValueError):
        ops.ctc_prefix_score(y, sl, r[:, :, :8].contiguous(), last, fin, cand, N)    # the state is not T frames long
    assert ops.check_async_errors(0) == 0


def test_log_softmax_rows(cuda):
    """ops.log_softmax_rows against float64 on rows of 3, 41 and 3388 columns with a spread of 60 (where log(softmax) would
    lose the small posteriors to underflow): within 2e-5 -- |values| < 128 (ulp 7.6e-6), a tree-reduced sum and one
    subtraction."""
    from tensorflow_end2end_speech_recognition_amd import ops
    rng = np.random.RandomState(0)
    for rows, cols in ((5, 3), (70, 41), (9, 3388)):
        x = (rng.randn(rows, cols) * 15).clip(-60, 60).astype(np.float32)
        want = torch.log_softmax(torch.tensor(x, dtype=torch.float64), dim=1).numpy()
        xd = torch.tensor(x, device=cuda)
        got = ops.log_softmax_rows(xd)
        assert np.abs(got.cpu().double().numpy() - want).max() < 2e-5 and np.isfinite(got.cpu().numpy()).all()
        assert torch.equal(ops.log_softmax_rows(xd, out=xd), got)            # in place
    assert ops.check_async_errors(0) == 0


# ------------------------------------------------------------------------------------------------ the joint selection
# (W, C2, ctc_weight, length_penalty_weight) -> seed under which the float64 statement's selection margin is >= 1e-3 at every
# step of tests/_cpu_ops_att_joint.select_case (asserted in the test; found on the CPU, scripts/probe_att_joint.py --seeds)
_SELECT_SEEDS = {(2, 3, 0.3, 0.0): 0, (2, 3, 0.3, 0.6): 0, (2, 3, 0.3, 1.0): 0, (2, 3, 1.0, 0.0): 0, (2, 3, 1.0, 0.6): 0,
                 (2, 3, 1.0, 1.0): 0, (5, 40, 0.3, 0.0): 1, (5, 40, 0.3, 0.6): 0, (5, 40, 0.3, 1.0): 1, (5, 40, 1.0, 0.0): 0,
                 (5, 40, 1.0, 0.6): 0, (5, 40, 1.0, 1.0): 0, (20, 3389, 0.3, 0.0): 0, (20, 3389, 0.3, 0.6): 0,
                 (20, 3389, 0.3, 1.0): 0, (20, 3389, 1.0, 0.0): 8, (20, 3389, 1.0, 0.6): 8, (20, 3389, 1.0, 1.0): 8}


@pytest.mark.parametrize('lpw', [0.0, 0.6, 1.0])
@pytest.mark.parametrize('lam', [0.3, 1.0])
@pytest.mark.parametrize('W,C2', J.SELECT_CASES)
def test_joint_select_against_the_statement(cuda, W, C2, lam, lpw):
    """ops.att_beam_select_joint over a 4-step search of 3 utterances (24, 9 and 3 frames), every step fed the statement's
    own input state (errors do not accumulate): word / parent / finished / lengths / last exactly (the seed's float64
    margin is asserted to be >= 10 x BOUND), score / log_probs / ctc_score within BOUND, and the state advance that
    follows within BOUND of the statement's next state.  One launch for the three utterances equals one launch per
    utterance bit for bit."""
    from tensorflow_end2end_speech_recognition_amd import ops
    case, margin = J.select_case(W, C2, lam, lpw, _SELECT_SEEDS[(W, C2, lam, lpw)])
    assert margin >= MARGIN, margin
    N, seq, T, B = case['N'], case['seq_len'], case['T'], case['B']
    y, sl = _dev(case['y32'], torch.float32, cuda), _dev(seq, I32, cuda)
    assert any(s['out']['finished'].any() and not s['out']['finished'].all() for s in case['steps'])
    worst = 0.0
    for k, s in enumerate(case['steps']):
        o = s['out']
        args = dict(logits=_dev(s['logits'], torch.float32, cuda), r=_dev(s['r'], torch.float32, cuda),
                    last=_dev(s['last'], I32, cuda), ctc_score=_dev(s['ctc_score'], torch.float32, cuda),
                    log_probs=_dev(s['log_probs'], torch.float32, cuda), finished=_dev(s['finished'], I32, cuda),
                    lengths=_dev(s['lengths'], I32, cuda))

        def run(rows, ys, sls, count=None):
            return ops.att_beam_select_joint(args['logits'][rows].contiguous(), ys, sls, args['r'][rows].contiguous(),
                                             args['last'][rows].contiguous(), args['ctc_score'][rows].contiguous(), N, lam, lpw,
                                             s['first'], args['log_probs'][rows].contiguous(), args['finished'][rows].contiguous(),
                                             args['lengths'][rows].contiguous(), count)
        count = torch.zeros(1, dtype=I32, device=cuda)
        word, parent, score, lp, fin, ln, last, ctc = got = run(slice(None), y, sl, count)
        for name, g, w_ in (('word', word, o['word']), ('parent', parent, o['parent']), ('finished', fin, o['finished']),
                            ('lengths', ln, o['lengths']), ('last', last, o['last'])):
            assert g.cpu().reshape(-1).tolist() == np.asarray(w_).astype(np.int64).reshape(-1).tolist(), (name, k)
        assert int(count) == int((~o['finished']).sum())
        for name, g, w_ in (('score', score, o['score']), ('log_probs', lp, o['log_probs']), ('ctc_score', ctc, o['ctc_score'])):
            e, m = J.max_err(g.cpu().numpy().reshape(-1), np.asarray(w_).reshape(-1))
            assert m < 64 and e < BOUND, (name, k, e, m)
            worst = max(worst, e)
        nxt = ops.ctc_prefix_advance(y, sl, args['r'], args['last'], parent, word, N)
        e, m = J.max_err(nxt.cpu().numpy(), J.arrays_of(o['states'], T)[0])
        assert m < 64 and e < BOUND, ('state', k, e, m)
        worst = max(worst, e)
        for b in range(B):
            one = run(slice(b * W, (b + 1) * W), y[:, b:b + 1].contiguous(), sl[b:b + 1].contiguous())
            for t_all, t_one in zip(got, one):
                assert torch.equal(t_all.reshape(B, W)[b], t_one.reshape(-1)), (k, b)
    print('att_beam_select_joint W=%d C2=%d lambda=%g a=%g: largest error %.3g' % (W, C2, lam, lpw, worst))
    with pytest.raises(ValueError):
        ops.att_beam_select_joint(args['logits'], y, sl, args['r'], args['last'], args['ctc_score'], N, 0.0, lpw, False,
                                  args['log_probs'], args['finished'], args['lengths'])
    assert ops.check_async_errors(0) == 0


def test_joint_select_with_an_utterance_without_frames(cuda):
    """seq_len must be >= 1 (the float64 statement and JointCTCAttention.infer raise); the kernels' documented behaviour at
    0 frames, so that a caller's mistake cannot fault: the utterance has the empty hypothesis alone (psi(<EOS>) = 0, every
    label -inf), places no candidate reaches are finished <EOS> slots with score and log_probs -inf, nothing is NaN, the
    state advance writes nothing for it, and the other utterance of the launch is what it is alone, bit for bit."""
    from tensorflow_end2end_speech_recognition_amd import ops
    rng = np.random.RandomState(7)
    B, W, N, T = 2, 3, 5, 5
    y32, _ = J.ctc_posteriors(rng, T, B, N + 1)
    y, sl = _dev(y32, torch.float32, cuda), _dev([T, 0], I32, cuda)
    logits = _dev(rng.randn(B * W, N + 2), torch.float32, cuda)
    r, last, ctc = ops.ctc_prefix_init(y, sl, W)
    zf, zi = torch.zeros(B * W, device=cuda), torch.zeros(B * W, dtype=I32, device=cuda)
    got = ops.att_beam_select_joint(logits, y, sl, r, last, ctc, N, 0.3, 0.6, True, zf, zi, zi)
    word, parent, score, lp, fin, ln, last2, ctc2 = (t.cpu().reshape(B, W) for t in got)
    assert word[1].tolist() == [N + 1] * W and parent[1].tolist() == [0, 1, 2] and fin[1].tolist() == [1] * W
    assert ln[1].tolist() == [0] * W and last2[1].tolist() == [-1] * W and ctc2[1].tolist() == [0.0] * W
    assert np.isfinite(float(score[1, 0])) and np.isfinite(float(lp[1, 0]))
    assert score[1, 1:].tolist() == [float('-inf')] * 2 and lp[1, 1:].tolist() == [float('-inf')] * 2
    assert not any(torch.isnan(t.float()).any() for t in (score, lp, ctc2))
    one = ops.att_beam_select_joint(logits[:W].contiguous(), y[:, :1].contiguous(), sl[:1].contiguous(), r[:W].contiguous(),
                                    last[:W].contiguous(), ctc[:W].contiguous(), N, 0.3, 0.6, True, zf[:W], zi[:W], zi[:W])
    for t_all, t_one in zip(got, one):
        assert torch.equal(t_all.reshape(B, W)[0], t_one.reshape(-1))
    nxt = ops.ctc_prefix_advance(y, sl, r, last, got[1], got[0], N)
    assert not torch.isnan(nxt[:W]).any()
    assert ops.check_async_errors(0) == 0


# ------------------------------------------------------------------------------------------------ the array-level loop
# (W, attention type) -> seed of test_gpu_att_beam.beam_loop_arrays and _cpu_ops_att_joint.loop_posteriors under which the
# float64 statement's selection margin is >= 1e-3, one utterance has all its slots finished early and another searches to
# the last step (all asserted in the test; found on the CPU, scripts/probe_att_joint.py --seeds)
_JOINT_LOOP_SEEDS = {(1, 'bahdanau_content'): 1, (1, 'location'): 0, (4, 'bahdanau_content'): 1, (4, 'location'): 12,
                     (5, 'bahdanau_content'): 9, (5, 'location'): 71}


@pytest.mark.parametrize('W,att', sorted(_JOINT_LOOP_SEEDS))
def test_native_joint_loop_against_the_step_by_step_statement(cuda, W, att):
    """ops.att_decoder_beam_joint at ctc_weight 0.3 against _cpu_ops_att_joint._att_decoder_beam_joint (the beam loop test's
    operands -- B = 3, T = 40, 2H = 128, U = 64, A = 32, Em = 8, 12 classes, 12 steps -- with and without carried attention
    weights, and CTC posteriors [40,3,11]): the statement's margin is asserted to be >= 10 x BOUND first; then word, parent,
    the back-traced ids and the integer state are exact and score / log_probs / ctc_score within BOUND.  One utterance has
    finished early while another searches to the last step; check_every = 4 gives what check_every = 0 gives; the
    counters show one scorer launch, one advance and one joint selection per issued step; two runs are bit-identical."""
    import test_gpu_att_beam as tb
    from tensorflow_end2end_speech_recognition_amd import ops
    seed = _JOINT_LOOP_SEEDS[(W, att)]
    a, head, eos = tb.beam_loop_arrays(W, False, att, seed)
    y32, _ = J.loop_posteriors(seed)
    y_cpu, sl_cpu = torch.tensor(y32), torch.tensor(J.LOOP_SEQ, dtype=I32)
    To = a['To']
    ref = J._att_decoder_beam_joint(tb._clone(a), head['W_av'], head['W_out'], head['b_out'], head['embedding'], eos, W, y_cpu,
                                    sl_cpu, 0.3, 0.6, check_every=0)
    assert ref['min_margin'] >= MARGIN, ref['min_margin']
    done_at = tb.done_after(ref, eos)
    assert min(done_at) < To and max(done_at) == To, done_at
    y, sl = y_cpu.to(cuda), sl_cpu.to(cuda)

    def run(check_every):
        ga, gh = tb._clone(a, cuda), tb._clone(head, cuda)
        out = ops.att_decoder_beam_joint(ga, gh['W_av'], gh['W_out'], gh['b_out'], gh['embedding'], eos, W, y, sl, 0.3, 0.6,
                                         check_every=check_every)
        torch.cuda.synchronize()
        return out
    ops.reset_att_joint_counts(0)
    ops.reset_att_beam_counts(0)
    got = run(0)
    assert got['steps_issued'] == To
    assert ops.att_joint_counts(0) == dict(score=To, advance=To, joint_select=To)
    assert ops.att_beam_counts(0) == dict(select=0, reorder=To, backtrace=1)
    for k in ('word', 'parent', 'ids', 'hyp_len', 'finished', 'lengths'):
        assert torch.equal(got[k].cpu(), ref[k]), k
    assert torch.equal(got['unfinished'].cpu()[1:], ref['unfinished'][1:])
    for k in ('score', 'final_score', 'log_probs', 'ctc_score'):
        e, m = J.max_err(got[k].cpu().numpy(), ref[k].double().numpy())
        print('joint loop W=%d %s %s: error %.3g at |value| <= %.3g' % (W, att, k, e, m))
        assert m < 64 and e < BOUND, (k, e, m)
    again = run(0)
    for k in ('word', 'parent', 'score', 'ids', 'hyp_len', 'final_score', 'log_probs', 'ctc_score', 'finished', 'lengths'):
        assert torch.equal(again[k], got[k]), k
    early = run(4)
    n2 = early['steps_issued']
    assert 1 <= n2 <= To
    for k in ('ids', 'hyp_len', 'final_score', 'log_probs', 'ctc_score', 'finished', 'lengths'):
        assert torch.equal(early[k], got[k]), k
    for k in ('word', 'parent', 'score'):
        assert torch.equal(early[k][:n2], got[k][:n2]), k
    assert ops.check_async_errors(0) == 0


# ------------------------------------------------------------------------------------------------------- model level
def joint_model(dtype, seed, device, max_decode_length=12):
    """JointCTCAttention in the size of test_gpu_att_beam._model (H = 64, U = 128, 9 labels, B = 5, T = 70), location
    attention with carried weights; the output layer scaled by 40 and an <EOS> bias of 0.35 as there."""
    from tensorflow_end2end_speech_recognition_amd.models.attention.joint_ctc_attention import JointCTCAttention
    rng = np.random.RandomState(seed)
    B, T, D, H, L, U, A, Em, C = 5, 70, 12, 64, 1, 128, 32, 8, 9
    sl = rng.randint(T // 2, T + 1, size=B).astype(np.int32)
    sl[0] = T
    x = (rng.randn(B, T, D) * (np.arange(T)[None, :, None] < sl[:, None, None])).astype(np.float32)
    model = JointCTCAttention(input_size=D, encoder_type='blstm', encoder_num_units=H, encoder_num_layers=L,
                              encoder_num_proj=None, attention_type='location', attention_dim=A, decoder_type='lstm',
                              decoder_num_units=U, decoder_num_layers=1, embedding_dim=Em, lambda_weight=0.5, num_classes=C,
                              sos_index=C, eos_index=C + 1, max_decode_length=max_decode_length, parameter_init=0.1,
                              clip_grad_norm=5.0, clip_activation_encoder=50, clip_activation_decoder=50, dtype=dtype, seed=seed,
                              device=device, sharpening_factor=1.5, prev_alpha='carry', honour_ctor_args=True)
    sd = {k: v.clone() for k, v in model.store.state_dict().items()}
    sd['attention_decoder/decoder/output_layer/weights'] *= 40.0
    sd['attention_decoder/decoder/output_layer/biases'][C + 1] = 0.35
    sd['ctc_output/biases'][C] = 5.0                         # a CTC head that prefers the blank, as a trained one does
    model.store.load_state_dict(sd)
    return model, x, sl, C, sd


def oracle_joint(sd, x, sl, C, dtype):
    import _att_joint_oracle as jo
    from oracle import lstm as olstm
    sdn = {k: v.cpu().numpy() for k, v in sd.items()}
    return jo.joint_beam_infer(sdn, x, sl, 1, 'location', C, C + 1, 12, 4, 0.3, 0.6, clip_enc=50.0, clip_dec=50.0,
                               sharpening=1.5, prev_alpha='carry', operand_round=olstm.bf16_round_t if dtype == 'bf16' else None)


# dtype -> seed of model and batch under which the float64 statement's margin is >= 1e-3 for every utterance (asserted)
_MODEL_SEEDS = {'f32': 7, 'bf16': 7}


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_model_joint_decode_against_the_oracle_statement(cuda, dtype):
    """JointCTCAttention.infer(beam_width=4, length_penalty_weight=0.6, ctc_weight=0.3) on a small fp32 model and a
    bf16-operand one equals JointBeamSearchDecoder driven by oracle.attention's float64 step functions and the oracle's CTC
    head (with the bf16 model's rounding points): every hypothesis of every utterance, ids exactly (the margin of every
    utterance is asserted to be >= 10 x BOUND; none is skipped) and scores to 1e-3 absolute, the bar of
    test_model_beam_search_against_the_oracle_statement.  ctc_weight = 0 is infer(beam_width=4) bit for bit, without one
    launch of the joint kernels."""
    from tensorflow_end2end_speech_recognition_amd import ops
    model, x, sl, C, sd = joint_model(dtype, _MODEL_SEEDS[dtype], cuda)
    want = oracle_joint(sd, x, sl, C, dtype)
    assert all(r['margin'] >= MARGIN for r in want), [r['margin'] for r in want]
    ops.reset_att_joint_counts(0)
    best = model.infer(x, sl, beam_width=4, length_penalty_weight=0.6, ctc_weight=0.3)
    raw = model._beam_raw
    n = raw['steps_issued']
    assert ops.att_joint_counts(0) == dict(score=n, advance=n, joint_select=n)
    assert raw['ids'].shape == (5, 4, 12) and raw['ctc_score'].shape == (5, 4)
    for b, r in enumerate(want):
        for w in range(4):
            k = int(raw['hyp_len'][b, w])
            assert raw['ids'][b, w, :k].tolist() == r['ids'][w], (b, w)
            assert not raw['ids'][b, w, k:].any()
        e = np.abs(raw['scores'][b] - r['scores']).max()
        ec = np.abs(raw['ctc_score'][b] - r['ctc_score']).max()
        print('model joint %s utterance %d: margin %.3g, score error %.3g, ctc_score error %.3g' % (dtype, b, r['margin'], e, ec))
        assert e < 1e-3 and ec < 1e-3
        assert best[b, :len(r['ids'][0])].tolist() == r['ids'][0]
    ops.reset_att_joint_counts(0)
    plain = model.infer(x, sl, beam_width=4, length_penalty_weight=0.6)
    raw_plain = model._beam_raw
    zero = model.infer(x, sl, beam_width=4, length_penalty_weight=0.6, ctc_weight=0.0)
    assert ops.att_joint_counts(0) == dict(score=0, advance=0, joint_select=0)
    assert np.array_equal(zero, plain)
    assert np.array_equal(model._beam_raw['ids'], raw_plain['ids'])
    assert np.array_equal(model._beam_raw['scores'].view(np.int32), raw_plain['scores'].view(np.int32))
    assert ops.check_async_errors(0) == 0
