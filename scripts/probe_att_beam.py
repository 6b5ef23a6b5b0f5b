#!/usr/bin/env python
"""Attention beam search (asr_att_decoder_beam) at the cfg D shape of bench.py: wall time of the beam loop at width 1
against the greedy loop (asr_att_decoder_infer) on the same batch, and tokens/s at width 20 (BEAM_WIDTH).  Nothing is
asserted on the numbers.

    python scripts/probe_att_beam.py            # needs the GPU
    python scripts/probe_att_beam.py --seeds    # CPU: the seeds of tests/test_gpu_att_beam.py's loop cases (the first
                                                # under which the float64 statement's selection margin is above 1e-3,
                                                # utterance 0 has finished after step 3 and another searches to the end)
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch


def find_seeds():
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import _cpu_ops_att_beam as cpub
    import test_gpu_att_beam as t
    found = {}
    for W, cell_bf16, att in t._LOOP_CASES:
        for seed in range(400):
            a, head, eos = t.beam_loop_arrays(W, cell_bf16, att, seed)
            ref = cpub._att_decoder_beam(a, head['W_av'], head['W_out'], head['b_out'], head['embedding'], eos, W, 0.6,
                                         check_every=0)
            if not ref['min_margin'] > 1e-3:
                continue
            done_at = t.done_after(ref, eos)
            if done_at[0] == 3 and max(done_at) == a['To']:
                found[(W, cell_bf16, att)] = seed
                print((W, cell_bf16, att), seed, 'margin %.3g' % ref['min_margin'], done_at, flush=True)
                break
        else:
            print((W, cell_bf16, att), 'no seed')
    print('_BEAM_LOOP_SEEDS =', found)


def main():
    from bench import device_features
    from tensorflow_end2end_speech_recognition_amd.models.attention.joint_ctc_attention import JointCTCAttention
    dev = torch.device('cuda:0')
    seed, D, C, att, tlo, thi, ldiv = 3, 240, 28, 'location', 100, 1600, 4
    B, H, L, U, A, Em = 32, 512, 5, 512, 128, 64
    rng = np.random.RandomState(seed)
    seq_len = rng.randint(tlo, thi + 1, size=B).astype(np.int32)
    Lmax = int(np.maximum(1, seq_len // ldiv).max()) + 2
    xd = device_features(seed, seq_len, D, dev)
    model = JointCTCAttention(input_size=D, encoder_type='blstm', encoder_num_units=H, encoder_num_layers=L,
                              encoder_num_proj=None, attention_type=att, attention_dim=A, decoder_type='lstm',
                              decoder_num_units=U, decoder_num_layers=1, embedding_dim=Em, lambda_weight=0.5,
                              num_classes=C, sos_index=C, eos_index=C + 1, max_decode_length=Lmax, parameter_init=0.1,
                              clip_grad_norm=5.0, clip_activation_encoder=50, clip_activation_decoder=50, dtype='bf16',
                              seed=5, device=str(dev))
    wide = int(os.environ.get('BEAM_WIDTH', '20'))
    isl = torch.tensor(seq_len, device=dev)
    for name, fn in (('greedy loop', lambda: model.infer(xd, seq_len)),
                     ('beam loop W=1', lambda: model._decode_beam(xd, isl, 1)),
                     ('beam loop W=%d' % wide, lambda: model.infer(xd, seq_len, beam_width=wide, length_penalty_weight=0.6))):
        try:
            fn()
        except Exception as e:                               # (e.g. the handle's scratch is too small for B * W rows)
            print('cfg D %s: %s' % (name, e), flush=True)
            continue
        torch.cuda.synchronize()
        best = None
        for it in range(3):
            t0 = time.perf_counter()
            ids = fn()
            t = time.perf_counter() - t0
            best = t if best is None else min(best, t)
        raw = model._infer_raw if name == 'greedy loop' else model._beam_raw
        print('cfg D %s: %.1f ms per call (encoder included), %d steps issued, ids %s -> %.0f tokens/s' % (
            name, best * 1e3, int(raw['steps_issued']), tuple(ids.shape), B * ids.shape[1] / best), flush=True)


if __name__ == '__main__':
    find_seeds() if '--seeds' in sys.argv else main()
