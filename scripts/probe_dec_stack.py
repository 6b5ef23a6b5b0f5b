#!/usr/bin/env python
"""Probe for the multi-layer LSTM decoder of the attention models (decoder_num_layers > 1; csrc/dec_stack.hip).

    python scripts/probe_dec_stack.py [--out profiles/dec_stack_probe.json]

From one process, with device events, a warm-up and medians of seven repeats that alternate the variants (the convention of
scripts/probe_gru_decoder.py), on bench.py's cfg D shard (5 x 512 BLSTM joint CTC-attention, location, bf16, B = 32,
400 decoder steps, dropout 0.2, adam), models with decoder_num_layers = 1, 2 and 3:
  * one training step (compute_loss + train);
  * the decoder's forward loop alone (ops.att_decoder_fwd on the step's own loop dict) and its backward loop alone
    (ops.att_decoder_bwd), per decoder step, beside the estimate from the launch structure: one more launch per upper layer
    on each chain, at the chain's own time per launch (forward 34.9 us over 4 launches, backward 47.5 us over 4);
  * the one-launch backward of a lower layer against its generic form (two products + the cell launch) in the backward loop
    of the same loop dict (ASR_DEC_STACK_FUSED=0 is the A/B switch);
  * greedy infer() of max_decode_length steps (an untrained model never emits <EOS>: every row decodes every step), as
    tokens per second, the encoder included;
  * per loop, which kernels a step ran (the path counters).
The one-layer variant runs the entry points the commit before ran, call for call (tests/test_gpu_att_stack.py holds it
bit-identical and counts no stack call in it), so it stands for that commit here.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts.probe_gru_decoder import REPEATS, alternate          # noqa: E402

# launches on a decoder step's serial chain at cfg D and their measured time (profiles/gru_decoder_probe.json, LSTM decoder)
FWD_CHAIN = dict(us=34.9, launches=4)       # cell (product + cell), query FC, fused attention step (2)
BWD_CHAIN = dict(us=47.5, launches=4)       # d-alpha + softmax, energy backward, query-FC + cell backward, d_in product


def cfgd(dev, layers):
    import bench
    from tensorflow_end2end_speech_recognition_amd.models.attention.joint_ctc_attention import JointCTCAttention
    seed, D, C, B, H, L, U, A, Em = 3, 240, 28, 32, 512, 5, 512, 128, 64
    rng = np.random.RandomState(seed)
    seq_len = rng.randint(100, 1601, size=B).astype(np.int32)
    lens = np.maximum(1, seq_len // 4)
    Lmax = int(lens.max()) + 2
    labels = np.full((B, Lmax), C + 1, dtype=np.int64)
    ctc = np.full((B, int(lens.max())), -1, dtype=np.int64)
    for b in range(B):
        y = rng.randint(0, C, size=lens[b])
        labels[b, 0] = C
        labels[b, 1:1 + lens[b]] = y
        ctc[b, :lens[b]] = y
    xd = bench.device_features(seed, seq_len, D, torch.device(dev))
    model = JointCTCAttention(input_size=D, encoder_type='blstm', encoder_num_units=H, encoder_num_layers=L,
                              encoder_num_proj=None, attention_type='location', attention_dim=A, decoder_type='lstm',
                              decoder_num_units=U, decoder_num_layers=layers, embedding_dim=Em, lambda_weight=0.5,
                              num_classes=C, sos_index=C, eos_index=C + 1, max_decode_length=Lmax - 1, parameter_init=0.1,
                              clip_grad_norm=5.0, clip_activation_encoder=50, clip_activation_decoder=50, dtype='bf16', seed=5,
                              device=dev)
    return model, (xd, labels, ctc, seq_len, lens + 2), Lmax - 1


def main(argv=None):
    from tensorflow_end2end_speech_recognition_amd import ops
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=None, help='write the record to this JSON file')
    args = ap.parse_args(argv)
    dev = 'cuda:0'
    rec = dict(device=torch.cuda.get_device_name(0), repeats=REPEATS,
               method='device events around each call, medians of %d repeats alternating the variants' % REPEATS)
    models, batch, To = {}, None, None
    for n in (1, 2, 3):
        models['L%d' % n], batch, To = cfgd(dev, n)
    rec['workload'] = ('cfg D shard: 5x512 BLSTM joint CTC-attention (location, A=128, U=512, E=64, C=28, lambda 0.5), bf16, '
                       'B=32, %d decoder steps, dropout 0.2, adam; decoder_num_layers 1 / 2 / 3' % To)

    # ---- the training step
    def make_step(m):
        def step():
            loss, *_ = m.compute_loss(*batch, 0.8, 0.8, 0.8)
            m.train(loss, 'adam', 1e-3)
        return step
    med, raw = alternate({k: make_step(m) for k, m in models.items()}, warmup=3)
    rec['train_step'] = dict(ms_per_step=med, over_L1={k: v / med['L1'] for k, v in med.items()}, ms_all=raw)
    print(json.dumps({k: rec['train_step'][k] for k in ('ms_per_step', 'over_L1')}), flush=True)

    # ---- the loops alone, on the loop dict of a step of each model
    loops = {}
    for k, m in models.items():
        loss, *_ = m.compute_loss(*batch, 0.8, 0.8, 0.8)
        loops[k] = m._tape['loop']
        m._set_optimizer('sgd', 0.0).compute_gradients(loss, model=m)     # fills the loop dict's backward fields
    torch.cuda.synchronize()
    counts = {}
    for k, a in loops.items():
        ops.reset_att_path_counts(0)
        ops.reset_att_stack_counts(0)
        ops.att_decoder_fwd(a)
        ops.att_decoder_bwd(a)
        counts[k] = dict(att={n: v for n, v in ops.att_path_counts(0).items() if v}, stack=dict(ops.att_stack_counts(0)))
    torch.cuda.synchronize()
    fwd, fraw = alternate({k: (lambda a=a: ops.att_decoder_fwd(a)) for k, a in loops.items()})
    bwd, braw = alternate({k: (lambda a=a: ops.att_decoder_bwd(a)) for k, a in loops.items()})
    est = lambda chain, n: chain['us'] + (n - 1) * chain['us'] / chain['launches']                  # noqa: E731
    rec['decoder_loops'] = dict(
        steps=To, fwd_us_per_step={k: v / To * 1e3 for k, v in fwd.items()},
        bwd_us_per_step={k: v / To * 1e3 for k, v in bwd.items()},
        estimate_from_launch_structure=dict(
            note='one more launch per upper layer on each chain, at the chain\'s own time per launch (%.1f us / %d launches '
                 'forward, %.1f us / %d backward at L = 1)' % (FWD_CHAIN['us'], FWD_CHAIN['launches'], BWD_CHAIN['us'],
                                                               BWD_CHAIN['launches']),
            fwd_us_per_step={'L%d' % n: est(FWD_CHAIN, n) for n in (1, 2, 3)},
            bwd_us_per_step={'L%d' % n: est(BWD_CHAIN, n) for n in (1, 2, 3)}),
        fwd_ms_all=fraw, bwd_ms_all=braw, path_counts=counts)
    print(json.dumps({k: rec['decoder_loops'][k] for k in ('fwd_us_per_step', 'bwd_us_per_step')}), flush=True)

    # ---- the one-launch backward of a lower layer against its generic form (same loop dicts)
    forms = {}
    for k in ('L2', 'L3'):
        a = loops[k]

        def form(fused, a=a):
            def run():
                a['stack']['fused'] = fused
                ops.att_decoder_bwd(a)
            return run
        two, traw = alternate({'fused': form(True), 'generic': form(False)})
        a['stack']['fused'] = True
        forms[k] = dict(bwd_us_per_step={n: v / To * 1e3 for n, v in two.items()}, fused_over_generic=two['fused'] / two['generic'],
                        bwd_ms_all=traw)
    rec['lower_layer_backward_forms'] = forms
    print(json.dumps({k: v['bwd_us_per_step'] for k, v in forms.items()}), flush=True)

    # ---- greedy decoding
    x, sl = batch[0], batch[3]
    steps = {}

    def make_infer(k, m):
        def run():
            steps[k] = int(m.infer(x, sl).shape[1])
        return run
    inf, iraw = alternate({k: make_infer(k, m) for k, m in models.items()})
    B = len(sl)
    rec['greedy_infer'] = dict(steps_decoded=steps, ms={k: v for k, v in inf.items()},
                               tokens_per_s={k: B * steps[k] / (v * 1e-3) for k, v in inf.items()}, ms_all=iraw)
    print(json.dumps({k: rec['greedy_infer'][k] for k in ('steps_decoded', 'ms', 'tokens_per_s')}), flush=True)
    assert ops.check_async_errors(0) == 0
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(rec, f, indent=1)


if __name__ == '__main__':
    main()
