#!/usr/bin/env python
"""Probes for the joint CTC / attention beam search (models/attention/decoders/beam_search/ctc_prefix_score.py,
csrc/ctc_prefix.hip for the prefix scorer, csrc/att_beam.hip for the selection).

    python scripts/probe_att_joint.py --seeds     CPU: the seeds the tests assert -- a case whose best hypothesis differs
                                                  between ctc_weight 0.5 and attention alone, and seeds of the selection
                                                  and loop tests whose float64 margin is >= 1e-3
    python scripts/probe_att_joint.py --bound     CPU: largest error of the numpy float32 emulation of the kernels' operation
                                                  order against the float64 statement, on the GPU tests' shapes
    python scripts/probe_att_joint.py --time      GPU: us per decode step of the beam search at cfg D's widths (5 x 512 BLSTM,
                                                  T = 400, B = 32, W = 10), attention alone and ctc_weight 0.3 alternating in one
                                                  process, device events, five repeats of >= 1 s each
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

MARGIN = 1e-3            # 10 x the tests' 1e-4 bound


def find_seeds():
    import _cpu_ops_att_joint as J
    import test_gpu_att_beam as tb
    for seed in range(50):
        a, j, margin = J.best_hypotheses(seed)
        if a != j and margin > MARGIN:
            print('non-vacuous: seed %d attention-only %s joint %s margin %.3g' % (seed, a, j, margin))
            break
    found = {}
    for W, C2 in J.SELECT_CASES:
        for lam in (0.3, 1.0):
            for lpw in (0.0, 0.6, 1.0):
                for seed in range(200):
                    _, margin = J.select_case(W, C2, lam, lpw, seed)
                    if margin >= MARGIN:
                        found[(W, C2, lam, lpw)] = seed
                        break
                print('select', (W, C2, lam, lpw), found.get((W, C2, lam, lpw)), flush=True)
    print('_SELECT_SEEDS =', found)
    loop = {}
    for W in (1, 4, 5):
        for att in ('bahdanau_content', 'location'):
            for seed in range(100):
                a, head, eos = tb.beam_loop_arrays(W, False, att, seed)
                y32, _ = J.loop_posteriors(seed)
                ref = J._att_decoder_beam_joint(a, head['W_av'], head['W_out'], head['b_out'], head['embedding'], eos, W,
                                                torch.tensor(y32), torch.tensor(J.LOOP_SEQ, dtype=torch.int32), 0.3, 0.6,
                                                check_every=0)
                done = tb.done_after(ref, eos)
                if ref['min_margin'] >= MARGIN and min(done) < a['To'] - 4 and max(done) == a['To']:
                    loop[(W, att)] = seed
                    print('loop', (W, att), seed, ref['min_margin'], done, flush=True)
                    break
    print('_JOINT_LOOP_SEEDS =', loop)
    print('_MODEL_SEEDS =', find_model_seeds())


def find_model_seeds():
    """Seeds of test_gpu_att_joint.joint_model under which every utterance's float64 margin is >= 1e-3 (the parameters are
    drawn on the host, so the CPU sees the model the device test builds)."""
    import test_gpu_att_joint as tj
    found = {}
    for dtype in ('f32', 'bf16'):
        for seed in range(60):
            _, x, sl, C, sd = tj.joint_model(dtype, seed, 'cpu')
            want = tj.oracle_joint(sd, x, sl, C, dtype)
            margins = [r['margin'] for r in want]
            lens = {len(i) for r in want for i in r['ids']}
            print('model', dtype, seed, min(margins), sorted(lens), flush=True)
            if min(margins) >= MARGIN and len(lens) >= 3:
                found[dtype] = seed
                break
    return found


def bound():
    import _cpu_ops_att_joint as J
    worst = 0.0
    for W, Cc in J.PREFIX_CASES:
        c = J.prefix_case(W, Cc)
        r32 = c['r'].astype(np.float32)
        psi = J.emulate_score32(c['y32'], r32, c['last'], c['finished'], c['cand'], c['seq_len'], c['N'], W)
        e1, m1 = J.max_err(psi, c['psi'])
        nxt = J.emulate_advance32(c['y32'], r32, c['last'], c['parent'], c['word'], c['seq_len'], c['N'], c['blank'])
        e2, m2 = J.max_err(nxt, c['r_next'])
        print('W=%d Cc=%d: psi error %.3g (|psi| <= %.3g), state error %.3g (|r| <= %.3g)' % (W, Cc, e1, m1, e2, m2))
        worst = max(worst, e1, e2)
    print('largest emulated error %.3g; 4 x = %.3g; bound = %.3g' % (worst, 4 * worst, max(1e-4, 4 * worst)))


def time_decode(out_path, once=False):
    from tensorflow_end2end_speech_recognition_amd import ops
    from tensorflow_end2end_speech_recognition_amd.models.attention.joint_ctc_attention import JointCTCAttention
    B, T, D, H, L, U, A, Em, C, W = 32, 400, 240, 512, 5, 512, 128, 64, 28, 10
    rng = np.random.RandomState(3)
    seq_len = rng.randint(T // 2, T + 1, size=B).astype(np.int32)
    seq_len[0] = T
    x = (rng.randn(B, T, D) * (np.arange(T)[None, :, None] < seq_len[:, None, None])).astype(np.float32)

    def model_for(To):
        m = JointCTCAttention(input_size=D, encoder_type='blstm', encoder_num_units=H, encoder_num_layers=L,
                              encoder_num_proj=None, attention_type='location', attention_dim=A, decoder_type='lstm',
                              decoder_num_units=U, decoder_num_layers=1, embedding_dim=Em, lambda_weight=0.5, num_classes=C,
                              sos_index=C, eos_index=C + 1, max_decode_length=To, parameter_init=0.1, clip_grad_norm=5.0,
                              clip_activation_encoder=50, clip_activation_decoder=50, dtype='bf16', seed=5, device='cuda:0')
        sd = {k: v.clone() for k, v in m.store.state_dict().items()}
        sd['attention_decoder/decoder/output_layer/biases'][C + 1] = -50.0       # nobody finishes: every step is issued
        m.store.load_state_dict(sd)
        return m

    if once:             # for a kernel trace (rocprofv3 --kernel-trace --stats -- python scripts/probe_att_joint.py --once)
        m = model_for(20)
        for _ in range(3):
            m.infer(x, seq_len, beam_width=W, ctc_weight=0.3)
        torch.cuda.synchronize()
        print(json.dumps(dict(steps_issued=m._beam_raw['steps_issued'], joint_counts=ops.att_joint_counts(0))))
        return
    models = {To: model_for(To) for To in (20, 60)}
    xd = ops.to_device(x, torch.float32, models[20].device)

    def run(To, lam):
        m = models[To]
        m.infer(xd, seq_len, beam_width=W, ctc_weight=lam)                       # warm-up
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n, total = 0, 0.0
        while total < 1000.0:
            e0.record()
            m.infer(xd, seq_len, beam_width=W, ctc_weight=lam)
            e1.record()
            torch.cuda.synchronize()
            total += e0.elapsed_time(e1)
            n += 1
        assert m._beam_raw['steps_issued'] == To
        return total / n

    rec = dict(config='5x512 BLSTM, location attention, U=512, A=128, T=400, B=32, W=10, bf16 operands', repeats=[])
    for rep in range(5):
        r = {}
        for name, lam in (('attention_only', 0.0), ('joint_0.3', 0.3)):
            t20, t60 = run(20, lam), run(60, lam)
            r[name] = dict(ms_20_steps=t20, ms_60_steps=t60, us_per_step=(t60 - t20) / 40.0 * 1e3)
        r['ratio'] = r['joint_0.3']['us_per_step'] / r['attention_only']['us_per_step']
        rec['repeats'].append(r)
        print(json.dumps(r), flush=True)
    rec['median_ratio'] = float(np.median([r['ratio'] for r in rec['repeats']]))
    rec['joint_counts_last_call'] = ops.att_joint_counts(0)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, 'w') as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(dict(median_ratio=rec['median_ratio'])))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--seeds', action='store_true')
    ap.add_argument('--bound', action='store_true')
    ap.add_argument('--time', action='store_true')
    ap.add_argument('--once', action='store_true', help='GPU: three joint decodes of 20 steps at the --time shape, for a kernel trace')
    ap.add_argument('--out', default=None, help='--time: write the record to this JSON file')
    args = ap.parse_args(argv)
    if args.seeds:
        find_seeds()
    if args.bound:
        bound()
    if args.time:
        time_decode(args.out)
    if args.once:
        time_decode(None, once=True)


if __name__ == '__main__':
    main()
