"""GPU: attention beam search -- att_beam_select_kernel against the fixture the reference's own beam_search_step produced,
the reorder and back-trace kernels against their statements, the native loop (asr_att_decoder_beam) against the
step-by-step float64 statement of tests/_cpu_ops_att_beam.py, and AttentionSeq2Seq.infer(beam_width=...) against the host
statement driven by oracle.attention."""
import numpy as np
import pytest
import torch

import _att_beam_golden as G

pytestmark = pytest.mark.gpu

I32 = torch.int32


# ------------------------------------------------------------------------------------------------ the select kernel
@pytest.mark.parametrize('name', sorted(G.cases()))
def test_select_kernel_against_the_reference_fixture(cuda, name):
    """ops.att_beam_select on the fixture's logits, every step fed the fixture's own input state (errors do not
    accumulate).  word / parent / finished / lengths exactly: the generator asserted a margin of 1e-3 between the scores
    that decide them (the tie case: exact ties, lower flat index first).  score / log_probs within 1e-4 absolute: values
    are below 64, where an fp32 ulp is at most 3.8e-6 (7.6e-6 with the rounding of the input state), and the kernel's
    tree-reduced log-softmax, one add and one divide are about ten roundings.  (20, 3388) and (2, 3) are the shape
    extremes, (5, 40) a beam width that is no power of two."""
    from tensorflow_end2end_speech_recognition_amd import ops
    meta, arr = G.load()
    c = meta[name]
    W, C2, eos = c['W'], c['C2'], c['C2'] - 1
    a = lambda f: arr[name + '|' + f]                                                  # noqa: E731
    worst = 0.0
    for s in range(c['steps']):
        x = torch.tensor(G.logits(name, c, s, c['seeds'][s]), dtype=torch.float32, device=cuda)
        lp = torch.tensor(a('in_log_probs')[s], dtype=torch.float32, device=cuda)
        fin = torch.tensor(a('in_finished')[s].astype(np.int32), device=cuda)
        ln = torch.tensor(a('in_lengths')[s].astype(np.int32), device=cuda)
        count = torch.zeros(1, dtype=I32, device=cuda)
        word, parent, score, lp2, fin2, ln2 = ops.att_beam_select(x, W, eos, c['alpha'], c['time0'] + s == 0, lp, fin, ln, count)
        assert word.cpu().view(-1).tolist() == a('word')[s].tolist(), (name, s)
        assert parent.cpu().view(-1).tolist() == a('parent')[s].tolist(), (name, s)
        assert fin2.cpu().tolist() == a('out_finished')[s].astype(int).tolist()
        assert ln2.cpu().tolist() == a('out_lengths')[s].tolist()
        assert int(count) == int((~a('out_finished')[s]).sum())
        e = max(np.abs(score.cpu().double().numpy().reshape(-1) - a('score')[s]).max(),
                np.abs(lp2.cpu().double().numpy() - a('out_log_probs')[s]).max())
        worst = max(worst, float(e))
        assert torch.equal(lp, torch.tensor(a('in_log_probs')[s], dtype=torch.float32, device=cuda))     # inputs untouched
    print('att_beam_select %s: largest |score / log_probs error| %.3g' % (name, worst))
    assert worst < 1e-4, worst
    assert ops.check_async_errors(0) == 0


def test_select_kernel_batches_utterances_and_updates_in_place(cuda):
    """Several utterances per launch (one workgroup each) give what one launch per utterance gives, bit for bit."""
    from tensorflow_end2end_speech_recognition_amd import ops
    rng = np.random.RandomState(3)
    B, W, C2 = 5, 5, 40
    x = torch.tensor(rng.uniform(-4, 4, size=(B * W, C2)), dtype=torch.float32, device=cuda)
    lp = torch.tensor(-rng.rand(B * W) * 5, dtype=torch.float32, device=cuda)
    fin = torch.tensor((rng.rand(B * W) < 0.3).astype(np.int32), device=cuda)
    ln = torch.tensor(rng.randint(0, 6, size=B * W).astype(np.int32), device=cuda)
    whole = ops.att_beam_select(x, W, C2 - 1, 0.6, False, lp, fin, ln)
    for b in range(B):
        r = slice(b * W, (b + 1) * W)
        one = ops.att_beam_select(x[r].contiguous(), W, C2 - 1, 0.6, False, lp[r].contiguous(), fin[r].contiguous(), ln[r].contiguous())
        for t_all, t_one in zip(whole, one):
            assert torch.equal(t_all.reshape(B, W)[b], t_one.reshape(-1))
    with pytest.raises(ValueError):
        ops.att_beam_select(x[:33 * 1], 33, C2 - 1, 0.0, False, lp[:33], fin[:33], ln[:33])
    with pytest.raises(ValueError):
        ops.att_beam_select(x[:, :3].contiguous(), 5, 2, 0.0, False, lp, fin, ln)
    assert ops.check_async_errors(0) == 0


# ------------------------------------------------------------------------------------- reorder and back-trace kernels
@pytest.mark.parametrize('U,E2,Em', [(64, 128, 8), (16, 64, 64), (300, 72, 3)])
@pytest.mark.parametrize('carry', [False, True])
def test_reorder_and_backtrace_kernels(cuda, U, E2, Em, carry):
    """Pure data movement, so exact: against tests/_cpu_ops_att_beam.py on random parents that include a parent chosen by
    several children and one chosen by none; with and without the carried attention weights (T = 70)."""
    import _cpu_ops_att_beam as cpub
    from tensorflow_end2end_speech_recognition_amd import ops
    rng = np.random.RandomState(U + Em)
    B, W, T, C2, To = 3, 5, 70, 12, 9
    R, Din = B * W, Em + E2 + U
    f = lambda *s: torch.tensor(rng.randn(*s), dtype=torch.float32)                    # noqa: E731
    parent = torch.tensor(rng.randint(0, W, size=(B, W)).astype(np.int32))
    parent[0] = torch.tensor([2, 2, 2, 0, 4])                # 2 chosen three times, 1 and 3 by none
    word = torch.tensor(rng.randint(0, C2, size=(B, W)).astype(np.int32))
    src = dict(c=f(R, U), h=f(R, U), din=f(R, Din), alpha=f(R, T) if carry else None, emb=f(C2, Em))
    want = cpub._att_beam_reorder(parent, word, src['c'], src['h'], src['din'], src['alpha'], src['emb'])
    d = {k: (v.to(cuda) if v is not None else None) for k, v in src.items()}
    got = ops.att_beam_reorder(parent.to(cuda), word.to(cuda), d['c'], d['h'], d['din'], d['alpha'], d['emb'])
    for g, w_ in zip(got, want):
        assert (g is None) == (w_ is None)
        if g is not None:
            assert torch.equal(g.cpu(), w_)
    for k in ('c', 'h', 'din'):
        assert torch.equal(d[k].cpu(), src[k])               # out of place: the sources are untouched
    # back-trace: random trees, <EOS> (= C2 - 1) turning up at different depths, also never
    words = torch.tensor(rng.randint(0, C2, size=(To, B, W)).astype(np.int32))
    words[:, 1] = torch.tensor(rng.randint(0, C2 - 1, size=(To, W)).astype(np.int32))       # utterance 1: no <EOS> at all
    parents = torch.tensor(rng.randint(0, W, size=(To, B, W)).astype(np.int32))
    score = f(To, B, W)
    for steps in (1, 4, To):
        wi, wn, ws = cpub._att_beam_backtrace(words, parents, score, steps, C2 - 1)
        gi, gn, gs = ops.att_beam_backtrace(words.to(cuda), parents.to(cuda), score.to(cuda), steps, C2 - 1)
        assert torch.equal(gi.cpu(), wi) and torch.equal(gn.cpu(), wn) and torch.equal(gs.cpu(), ws)
    assert int(wn[1].min()) == To and int(wn.min()) < To
    assert ops.check_async_errors(0) == 0


# ------------------------------------------------------------------------------------------------ the array-level loop
# Seeds under which the float64 statement's selection margin (smallest gap among the top W + 1 candidate scores, over all
# steps and utterances that still search) is above 1e-3 and utterance 0 has all its slots finished after step 3 while
# another utterance searches on to the last step -- both asserted in the test, so neither the exact comparison nor the
# invariance check can pass vacuously.  Found on the CPU (scripts/probe_att_beam.py --seeds).
_BEAM_LOOP_SEEDS = {(1, False, 'bahdanau_content'): 32, (4, False, 'bahdanau_content'): 32, (5, False, 'bahdanau_content'): 32,
                    (1, True, 'bahdanau_content'): 32, (4, True, 'bahdanau_content'): 32, (5, True, 'bahdanau_content'): 32,
                    (4, False, 'location'): 25, (5, True, 'location'): 25}


def beam_loop_arrays(W, cell_bf16, att, seed):
    """Operands of asr_att_decoder_beam on the CPU: B = 3 utterances x W slots, T = 40, 2H = 128, U = 64, A = 32, Em = 8,
    12 classes, 12 steps.  Utterance 0's encoder carries a constant that the attentional vector turns into a large
    <EOS> logit from the step `boost_from` on (through one unit of the attentional vector that its context saturates),
    so all its slots finish early."""
    rng = np.random.RandomState(seed)
    B, T, To, Em, E2, U, A, C2 = 3, 40, 12, 8, 128, 64, 32, 12
    R, Din = B * W, Em + E2 + U
    carry = att == 'location'
    f = lambda *s, sc=1.0: torch.tensor(rng.randn(*s) * sc, dtype=torch.float32)      # noqa: E731
    seq_u = torch.tensor([T, 31, 17], dtype=torch.int32)
    enc_u = f(T, B, E2, sc=0.5) * (torch.arange(T).view(T, 1, 1) < seq_u.view(1, B, 1))
    enc_u[:, 0, 0] = 6.0                                     # utterance 0's mark (its context column 0 is 6 at every step)
    keys_u = None if carry else f(T, B, A, sc=0.5)
    rows = torch.arange(B).repeat_interleave(W)
    W_cell = f(Din, 4 * U, sc=0.08)
    emb = f(C2, Em, sc=0.5)
    c0, h0 = f(B, U, sc=0.3), f(B, U, sc=0.3)
    a = dict(To=To, B=R, T=T, U=U, Em=Em, E2=E2, A=A, att_mode=0, has_query_fc=1, carry_alpha=int(carry),
             taps=201 if carry else 0, enc_dtype=0, forget_bias=1.0, cell_clip=3.0, sharpening=1.5,
             W_cell=W_cell.to(torch.bfloat16).float() if cell_bf16 else W_cell, b_cell=f(4 * U, sc=0.1),
             peep=f(3, U, sc=0.1), W_q=f(U, A, sc=0.1), b_q=f(A, sc=0.1) if carry else None, v=f(A, sc=0.5),
             keys=keys_u[:, rows].contiguous() if keys_u is not None else None, enc=enc_u[:, rows].contiguous(),
             seq_len=seq_u[rows].contiguous(), filt=f(201, 1, 10, sc=0.3) if carry else None,
             wfil=f(10, A, sc=0.3) if carry else None, alpha_zero=torch.zeros(R, T) if carry else None,
             live=torch.ones(R), dec_in=torch.zeros(2, R, Din), av_in=torch.zeros(1, R, U + E2),
             alpha_all=torch.zeros(1, R, T), gates_all=torch.zeros(1, R, 4 * U), craw_all=torch.zeros(1, R, U),
             c_all=torch.zeros(2, R, U), h_all=torch.zeros(2, R, U), qz_all=torch.zeros(1, R, A))
    if cell_bf16:
        a['cell_bf16'] = True
    a['c_all'][0] = c0[rows]
    a['h_all'][0] = h0[rows]
    a['dec_in'][0, :, :Em] = emb[C2 - 2]                     # <SOS>
    a['dec_in'][0, :, Em + E2:] = h0[rows]
    head = dict(W_av=f(U + E2, U, sc=0.15), W_out=f(U, C2, sc=0.6), b_out=f(C2, sc=0.3), embedding=emb)
    head['W_av'][:, 0] = 0.0
    head['W_av'][U, 0] = 0.5                                 # attentional unit 0 = tanh(0.5 * context column 0): ~1 for utterance 0
    head['W_out'][0, :] = 0.0
    head['W_out'][0, C2 - 1] = 3.0                           # ... and <EOS> reads it
    head['b_out'][C2 - 1] = 0.5
    return a, head, C2 - 1


def done_after(ref, eos):
    """Per utterance, the step after which all its slots are finished (To if some slot never finishes)."""
    To, B, W = ref['word'].shape
    out = []
    for b in range(B):
        n = [int(v) for v in ref['hyp_len'][b]]
        all_eos = all(int(ref['ids'][b, w, n[w] - 1]) == eos for w in range(W))
        out.append(max(n) - 1 if all_eos else To)
    return out


def _clone(d, dev=None):
    return {k: ((v.clone().to(dev) if dev is not None else v.clone()) if torch.is_tensor(v) else v) for k, v in d.items()}


_LOOP_CASES = [(1, False, 'bahdanau_content'), (4, False, 'bahdanau_content'), (5, False, 'bahdanau_content'),
               (1, True, 'bahdanau_content'), (4, True, 'bahdanau_content'), (5, True, 'bahdanau_content'),
               (4, False, 'location'), (5, True, 'location')]


@pytest.mark.parametrize('W,cell_bf16,att', _LOOP_CASES)
def test_native_beam_loop_against_the_step_by_step_statement(cuda, W, cell_bf16, att):
    """ops.att_decoder_beam against _cpu_ops_att_beam._att_decoder_beam (the greedy loop's step, then select and reorder,
    in float64), in the pattern of test_native_inference_loop_at_the_fused_cell_widths: the statement's selection margin
    is asserted to be above 1e-3 first; then word, parent and the back-traced ids are exact and the scores within that
    test's forward bound (2e-5 of the largest entry).  Two device runs, check_every = 0 (all 12 steps) and 4 (early
    exit allowed), give identical outputs; utterance 0, whose slots have all finished after step 3, keeps its
    hypotheses to step 12."""
    import _cpu_ops_att_beam as cpub
    from tensorflow_end2end_speech_recognition_amd import ops
    seed = _BEAM_LOOP_SEEDS[(W, cell_bf16, att)]
    a, head, eos = beam_loop_arrays(W, cell_bf16, att, seed)
    To, B = a['To'], 3
    ref = cpub._att_decoder_beam(_clone(a), head['W_av'], head['W_out'], head['b_out'], head['embedding'], eos, W, 0.6,
                                 check_every=0)
    assert ref['min_margin'] > 1e-3, ref['min_margin']
    done_at = done_after(ref, eos)
    assert done_at[0] == 3 and max(done_at) == To, done_at
    assert ref['steps_issued'] == To
    ga, gh = _clone(a, cuda), _clone(head, cuda)
    ops.reset_att_beam_counts(0)
    got = ops.att_decoder_beam(ga, gh['W_av'], gh['W_out'], gh['b_out'], gh['embedding'], eos, W, 0.6, check_every=0)
    torch.cuda.synchronize()
    assert got['steps_issued'] == To
    assert ops.att_beam_counts(0) == dict(select=To, reorder=To, backtrace=1)
    for k in ('word', 'parent', 'ids', 'hyp_len', 'finished', 'lengths'):
        assert torch.equal(got[k].cpu(), ref[k]), k
    assert torch.equal(got['unfinished'].cpu()[1:], ref['unfinished'][1:])
    rel = lambda x, y: float(np.abs(x.cpu().double().numpy() - y.double().numpy()).max() / max(np.abs(y.double().numpy()).max(), 1e-2))
    for k in ('score', 'final_score', 'log_probs'):
        err = rel(got[k], ref[k])
        print('beam loop W=%d %s %s %s %.3g' % (W, 'bf16' if cell_bf16 else 'f32', att, k, err))
        assert err < 2e-5, (k, err)
    # utterance 0 after step 3: every later step repeats its slots in place, and its hypotheses are those of step 3
    w_np, p_np = got['word'].cpu().numpy(), got['parent'].cpu().numpy()
    assert (w_np[4:, 0] == eos).all() and (p_np[4:, 0] == np.arange(W)[None]).all()
    early = cpub._att_beam_backtrace(ref['word'], ref['parent'], ref['score'], 4, eos)
    assert torch.equal(early[0][0], got['ids'].cpu()[0]) and torch.equal(early[1][0], got['hyp_len'].cpu()[0])
    # surplus steps change nothing: a run that may stop early returns the same hypotheses
    ga2, gh2 = _clone(a, cuda), _clone(head, cuda)
    got2 = ops.att_decoder_beam(ga2, gh2['W_av'], gh2['W_out'], gh2['b_out'], gh2['embedding'], eos, W, 0.6, check_every=4)
    torch.cuda.synchronize()
    n2 = got2['steps_issued']
    assert 1 <= n2 <= To
    for k in ('ids', 'hyp_len', 'final_score', 'log_probs', 'finished', 'lengths'):
        assert torch.equal(got2[k], got[k]), k
    for k in ('word', 'parent', 'score'):
        assert torch.equal(got2[k][:n2], got[k][:n2]), k
    assert ops.check_async_errors(0) == 0


# ------------------------------------------------------------------------------------------------------- model level
def _model(att, prev, dtype, cuda, seed=5, max_decode_length=40):
    from tensorflow_end2end_speech_recognition_amd.models.attention.attention_seq2seq import AttentionSeq2Seq
    rng = np.random.RandomState(seed)
    B, T, D, H, L, U, A, Em, C = 5, 70, 12, 64, 1, 128, 32, 8, 9
    sl = rng.randint(T // 2, T + 1, size=B).astype(np.int32)
    sl[0] = T
    x = (rng.randn(B, T, D) * (np.arange(T)[None, :, None] < sl[:, None, None])).astype(np.float32)
    model = AttentionSeq2Seq(input_size=D, encoder_type='blstm', encoder_num_units=H, encoder_num_layers=L,
                             encoder_num_proj=None, attention_type=att, attention_dim=A, decoder_type='lstm',
                             decoder_num_units=U, decoder_num_layers=1, embedding_dim=Em, num_classes=C, sos_index=C,
                             eos_index=C + 1, max_decode_length=max_decode_length, parameter_init=0.1, clip_grad_norm=5.0,
                             clip_activation_encoder=50, clip_activation_decoder=50, dtype=dtype, seed=seed,
                             sharpening_factor=1.5, prev_alpha=prev)
    return model, x, sl, C


def _set_eos_bias(model, C, bias, out_scale=1.0):
    sd = {k: v.clone() for k, v in model.store.state_dict().items()}
    sd['attention_decoder/decoder/output_layer/weights'] *= out_scale
    sd['attention_decoder/decoder/output_layer/biases'][C + 1] = bias
    model.store.load_state_dict(sd)
    return sd


@pytest.mark.parametrize('att,prev,dtype', [('location', 'carry', 'f32'), ('hybrid', 'zeros', 'bf16'),
                                            ('bahdanau_content', 'zeros', 'f32')])
def test_beam_width_one_is_the_native_greedy_decode(cuda, att, prev, dtype):
    """_decode_beam(beam_width=1) -- tiling, select, reorder, back-trace -- returns infer()'s ids up to and including
    each row's first <EOS>, on the model of test_native_greedy_inference_loop (H = 64, U = 128, 9 classes) at its three
    <EOS> biases: nobody finishes (40 steps), rows finish at different steps, everybody finishes at once."""
    from tensorflow_end2end_speech_recognition_amd import ops
    from tensorflow_end2end_speech_recognition_amd.models.attention.decoders.beam_search.beam_search_decoder import cut_at_eos
    model, x, sl, C = _model(att, prev, dtype, cuda)
    lens = []
    for bias in (-50.0, 0.35, 50.0):
        _set_eos_bias(model, C, bias)
        greedy = model.infer(x, sl)
        assert np.array_equal(model.infer(x, sl, beam_width=1), greedy)
        ops.reset_att_beam_counts(0)
        beam = model._decode_beam(ops.to_device(x, torch.float32, model.device), ops.to_device(sl, torch.int32, model.device), 1)
        raw = model._beam_raw
        assert ops.att_beam_counts(0) == dict(select=raw['steps_issued'], reorder=raw['steps_issued'], backtrace=1)
        assert beam.shape == greedy.shape, (bias, beam.shape, greedy.shape)
        for b in range(len(sl)):
            assert cut_at_eos(beam[b], C + 1) == cut_at_eos(greedy[b], C + 1), (bias, b)
            assert not beam[b][len(cut_at_eos(beam[b], C + 1)):].any()
        lens.append(beam.shape[1])
    assert lens[0] == 40 and lens[2] == 1 and 1 <= lens[1] <= 40
    assert ops.check_async_errors(0) == 0


# (attention type, previous weights, seed of model and batch): seeds under which the float64 statement's margin is above
# 1e-3 for EVERY utterance, so none is skipped (found on the CPU; asserted in the test).  The output layer's weights are
# scaled by 40: at parameter_init = 0.1 the logits of an untrained model are so flat that four hypotheses over a dozen
# steps always meet a near-tie somewhere.
@pytest.mark.parametrize('att,prev,seed', [('location', 'carry', 15), ('bahdanau_content', 'zeros', 10)])
def test_model_beam_search_against_the_oracle_statement(cuda, att, prev, seed):
    """infer(beam_width=4, length_penalty_weight=0.6) on an fp32 model (H = 64, U = 128, 9 classes, at most 12 steps)
    equals BeamSearchDecoder driven by oracle.attention's float64 step functions: every hypothesis of every utterance
    (ids exactly; scores to 1e-3 absolute -- fp32 logits of magnitude ~10 summed over up to 12 steps), wherever that
    statement's margin is above 1e-3 -- at most one utterance in five may be skipped for margin, and under these seeds
    none is (asserted).  Hypotheses end at different steps within an utterance and across the batch."""
    import _att_beam_oracle as bo
    from tensorflow_end2end_speech_recognition_amd import ops
    model, x, sl, C = _model(att, prev, 'f32', cuda, seed=seed, max_decode_length=12)
    sd = _set_eos_bias(model, C, 0.35, out_scale=40.0)
    sdn = {k: v.cpu().numpy() for k, v in sd.items()}
    want = bo.beam_infer(sdn, x, sl, 1, att, C, C + 1, 12, 4, 0.6, clip_enc=50.0, clip_dec=50.0, sharpening=1.5,
                         prev_alpha=prev)
    skipped = [b for b, r in enumerate(want) if not r['margin'] > 1e-3]
    assert len(skipped) == 0, [r['margin'] for r in want]
    ops.reset_att_beam_counts(0)
    best = model.infer(x, sl, beam_width=4, length_penalty_weight=0.6)
    raw = model._beam_raw
    assert ops.att_beam_counts(0) == dict(select=raw['steps_issued'], reorder=raw['steps_issued'], backtrace=1)
    assert raw['ids'].shape == (5, 4, 12)
    assert len({len(i) for r in want for i in r['ids']}) >= 3
    for b, r in enumerate(want):
        for w in range(4):
            n = int(raw['hyp_len'][b, w])
            assert raw['ids'][b, w, :n].tolist() == r['ids'][w], (b, w)
            assert not raw['ids'][b, w, n:].any()
        print('model beam %s utterance %d: margin %.3g, score error %.3g' % (att, b, r['margin'],
                                                                             np.abs(raw['scores'][b] - r['scores']).max()))
        assert np.abs(raw['scores'][b] - r['scores']).max() < 1e-3
        assert best[b, :len(r['ids'][0])].tolist() == r['ids'][0]
    assert ops.check_async_errors(0) == 0
