#!/usr/bin/env python
"""Probes for shallow LM fusion in the attention beam search (models/attention/decoders/beam_search/lm_fusion.py,
csrc/lm_fusion.hip for the language model, csrc/att_beam.hip for the selection).

    python scripts/probe_lm_fusion.py             GPU: infer() at cfg D's widths (scripts/probe_att_beam.py: 5 x 512 BLSTM,
                                                  T = 400, B = 32) at W in {1, 5, 10, 20}: without a language model, and with
                                                  a 2 x 512 and a 1 x 256 LSTM LM at ctc_weight 0 and 0.3 -- device events,
                                                  a warm-up, medians of five repeats; tokens/s and us per decoder step
                                                  (--no-lm: only the rows without a language model; W = 1 without LM and
                                                  CTC is the greedy loop)
    python scripts/probe_lm_fusion.py --seeds     CPU: seeds of the selection, loop and model tests whose float64 margin is
                                                  >= 1e-3 (10 x the tests' bound)
    python scripts/probe_lm_fusion.py --bound     CPU: largest error of the numpy float32 emulation of the selection kernels'
                                                  operation order against the float64 statement, on the GPU tests' shapes
    python scripts/probe_lm_fusion.py --once      GPU: three fused decodes of 20 steps at W = 10, for a kernel trace
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


def find_seeds(which):
    import _cpu_ops_lm as M
    import test_gpu_att_beam as tb
    import _cpu_ops_att_joint as J
    if 'select' in which:
        found = {}
        for W, C2 in M.SELECT_CASES:
            for lam in M.SELECT_LAMS:
                for lpw in M.SELECT_LPWS:
                    for seed in range(200):
                        case, margin = M.select_case(W, C2, lam, lpw, seed)
                        some = any(s['out']['finished'].any() and not s['out']['finished'].all() for s in case['steps'])
                        if margin >= MARGIN and some:
                            found[(W, C2, lam, lpw)] = seed
                            break
                    print('select', (W, C2, lam, lpw), found.get((W, C2, lam, lpw)), flush=True)
        print('SELECT_SEEDS =', found)
    if 'loop' in which:
        loop = {}
        for W in (1, 4, 5):
            for att in ('bahdanau_content', 'location'):
                for lam in (0.0, 0.3):
                    for seed in range(200):
                        a, head, eos = tb.beam_loop_arrays(W, False, att, seed)
                        y32, _ = J.loop_posteriors(seed)
                        ref = M._att_decoder_beam_lm(a, head['W_av'], head['W_out'], head['b_out'], head['embedding'], eos, W,
                                                     M.params_torch(M.loop_lm(seed)), M.LM_WEIGHT, 0.6, check_every=0,
                                                     y=torch.tensor(y32), seq_len=torch.tensor(J.LOOP_SEQ, dtype=torch.int32),
                                                     ctc_weight=lam)
                        done = tb.done_after(ref, eos)
                        if ref['min_margin'] >= MARGIN and min(done) < a['To'] - 4 and max(done) == a['To']:
                            loop[(W, att, lam)] = seed
                            print('loop', (W, att, lam), seed, ref['min_margin'], done, flush=True)
                            break
        print('LOOP_SEEDS =', loop)
    if 'model' in which:
        import test_gpu_lm_fusion as tl
        print('MODEL_SEEDS =', tl.find_model_seeds(MARGIN))


def bound():
    import _cpu_ops_lm as M
    worst = 0.0
    for (W, C2, lam, lpw), seed in sorted(M.SELECT_SEEDS.items()):
        case, _ = M.select_case(W, C2, lam, lpw, seed)
        e = M.emulation_error(case, W, lam, M.LM_WEIGHT, lpw)
        print('W=%d C2=%d ctc_weight=%g lpw=%g: emulation error %.3g' % (W, C2, lam, lpw, e), flush=True)
        worst = max(worst, e)
    print('largest emulated error %.3g; 4 x = %.3g; bound = %.3g' % (worst, 4 * worst, max(1e-4, 4 * worst)))


def _cfg_d(To, device='cuda:0'):
    from tensorflow_end2end_speech_recognition_amd.models.attention.joint_ctc_attention import JointCTCAttention
    B, T, D, H, L, U, A, Em, C = 32, 400, 240, 512, 5, 512, 128, 64, 28
    rng = np.random.RandomState(3)
    seq_len = rng.randint(T // 2, T + 1, size=B).astype(np.int32)
    seq_len[0] = T
    x = (rng.randn(B, T, D) * (np.arange(T)[None, :, None] < seq_len[:, None, None])).astype(np.float32)
    m = JointCTCAttention(input_size=D, encoder_type='blstm', encoder_num_units=H, encoder_num_layers=L,
                          encoder_num_proj=None, attention_type='location', attention_dim=A, decoder_type='lstm',
                          decoder_num_units=U, decoder_num_layers=1, embedding_dim=Em, lambda_weight=0.5, num_classes=C,
                          sos_index=C, eos_index=C + 1, max_decode_length=To, parameter_init=0.1, clip_grad_norm=5.0,
                          clip_activation_encoder=50, clip_activation_decoder=50, dtype='bf16', seed=5, device=device)
    sd = {k: v.clone() for k, v in m.store.state_dict().items()}
    sd['attention_decoder/decoder/output_layer/biases'][C + 1] = -50.0       # nobody finishes: every step is issued
    m.store.load_state_dict(sd)
    return m, x, seq_len, C


def _lm(C, layers, units, device='cuda:0'):
    from tensorflow_end2end_speech_recognition_amd.models.lm.base import RNNLM
    lm = RNNLM(num_classes=C + 2, embedding_dim=64, num_units=units, num_layers=layers, sos_index=C, eos_index=C + 1,
               seed=11, device=device)
    sd = {k: v.clone() for k, v in lm.store.state_dict().items()}
    sd['rnnlm/output/biases'][C + 1] = -50.0
    lm.store.load_state_dict(sd)
    return lm


def time_decode(out_path, once=False, no_lm=False):
    from tensorflow_end2end_speech_recognition_amd import ops
    if once:
        m, x, sl, C = _cfg_d(20)
        lm = _lm(C, 2, 512)
        for _ in range(3):
            m.infer(x, sl, beam_width=10, ctc_weight=0.3, lm=lm, lm_weight=0.3)
        torch.cuda.synchronize()
        print(json.dumps(dict(steps_issued=m._beam_raw['steps_issued'], lm_counts=ops.att_lm_counts(0))))
        return
    models = {To: _cfg_d(To) for To in (20, 60)}
    _, x, sl, C = models[20]
    xd = ops.to_device(x, torch.float32, models[20][0].device)
    lms = {'none': None} if no_lm else {'none': None, 'lm_2x512': _lm(C, 2, 512), 'lm_1x256': _lm(C, 1, 256)}
    B = x.shape[0]

    def run(To, W, lm, lam):
        m = models[To][0]
        kw = dict(beam_width=W, ctc_weight=lam)
        if lm is not None:
            kw.update(lm=lm, lm_weight=0.3)
        m.infer(xd, sl, **kw)                                                    # warm-up
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = []
        for _ in range(5):
            e0.record()
            m.infer(xd, sl, **kw)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        return float(np.median(times))

    rec = dict(config='5x512 BLSTM, location attention, U=512, A=128, T=400, B=32, bf16 operands; LM fp32, lm_weight 0.3',
               rows=[])
    for W in (1, 5, 10, 20):
        for name, lm in lms.items():
            for lam in (0.0, 0.3):
                t20, t60 = run(20, W, lm, lam), run(60, W, lm, lam)
                us = (t60 - t20) / 40.0 * 1e3
                r = dict(W=W, lm=name, ctc_weight=lam, ms_20_steps=t20, ms_60_steps=t60, us_per_step=us,
                         tokens_per_s=B * 60 / (t60 * 1e-3))
                rec['rows'].append(r)
                print(json.dumps(r), flush=True)
    if not no_lm:
        rec['lm_counts_last_call'] = ops.att_lm_counts(0)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, 'w') as f:
            json.dump(rec, f, indent=1)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--seeds', nargs='?', const='select,loop,model', default=None,
                    help='CPU: find seeds (optionally a comma list of select, loop, model)')
    ap.add_argument('--bound', action='store_true')
    ap.add_argument('--once', action='store_true', help='GPU: three fused decodes of 20 steps, for a kernel trace')
    ap.add_argument('--no-lm', action='store_true', help='timing mode: only the rows without a language model (this runs on '
                    'the commit before the language model as well: the untouched path must not have moved)')
    ap.add_argument('--out', default=None, help='timing mode: write the record to this JSON file')
    args = ap.parse_args(argv)
    if args.seeds:
        find_seeds(args.seeds.split(','))
    if args.bound:
        bound()
    if args.once:
        time_decode(None, once=True)
    if not (args.seeds or args.bound or args.once):
        time_decode(args.out, no_lm=args.no_lm)


if __name__ == '__main__':
    main()
