#!/usr/bin/env python
"""Probe for the GRU decoder of the attention models (decoder_type='gru'; csrc/gru_decoder.hip).

    python scripts/probe_gru_decoder.py [--out profiles/gru_decoder_probe.json]

From one process, with device events, a warm-up and medians of seven repeats that alternate the variants (the convention of
scripts/probe_sched_sampling.py), on bench.py's cfg D shard (5 x 512 BLSTM joint CTC-attention, location, bf16, B = 32,
400 decoder steps, dropout 0.2, adam), an LSTM-decoder model against a GRU-decoder model:
  * one training step (compute_loss + train);
  * the decoder's forward loop alone (ops.att_decoder_fwd on the step's own loop dict) and its backward loop alone
    (ops.att_decoder_bwd), per decoder step;
  * greedy infer() of max_decode_length steps (an untrained model never emits <EOS>: every row decodes every step), as
    tokens per second, the encoder included;
  * per loop, which kernels a step ran (the path counters) and the launches of its cell part.
The LSTM variant runs the entry points the commit before the GRU decoder ran, call for call (tests/test_gpu_att_gru.py
holds the LSTM decoder bit-identical and counts no GRU call in it), so it stands for that commit here.
The GRU cell's two forms are also timed against each other in the forward loop (ASR_DEC_GRU_GEMM=0 is the A/B switch).
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

REPEATS = 7


def alternate(calls, repeats=REPEATS, warmup=2):
    """{name: median ms} of the callables, run alternately `repeats` times after `warmup` rounds."""
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in calls}
    for _ in range(repeats):
        for k, fn in calls.items():
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    return {k: float(np.median(v)) for k, v in times.items()}, {k: [round(t, 4) for t in v] for k, v in times.items()}


def cfgd(dev, decoder_type):
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
                              encoder_num_proj=None, attention_type='location', attention_dim=A, decoder_type=decoder_type,
                              decoder_num_units=U, decoder_num_layers=1, embedding_dim=Em, lambda_weight=0.5, num_classes=C,
                              sos_index=C, eos_index=C + 1, max_decode_length=Lmax - 1, parameter_init=0.1,
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
    for dt in ('lstm', 'gru'):
        models[dt], batch, To = cfgd(dev, dt)
    rec['workload'] = ('cfg D shard: 5x512 BLSTM joint CTC-attention (location, A=128, U=512, E=64, C=28, lambda 0.5), bf16, '
                       'B=32, %d decoder steps, dropout 0.2, adam' % To)

    # ---- the training step
    def make_step(m):
        def step():
            loss, *_ = m.compute_loss(*batch, 0.8, 0.8, 0.8)
            m.train(loss, 'adam', 1e-3)
        return step
    med, raw = alternate({k: make_step(m) for k, m in models.items()}, warmup=3)
    rec['train_step'] = dict(ms_per_step=med, gru_over_lstm=med['gru'] / med['lstm'], ms_all=raw)
    print(json.dumps({k: rec['train_step'][k] for k in ('ms_per_step', 'gru_over_lstm')}), flush=True)

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
        ops.reset_att_gru_counts(0)
        ops.att_decoder_fwd(a)
        f = {n: v for n, v in ops.att_path_counts(0).items() if v}
        g = dict(ops.att_gru_counts(0))
        ops.reset_att_path_counts(0)
        ops.reset_att_gru_counts(0)
        ops.att_decoder_bwd(a)
        counts[k] = dict(fwd=f, fwd_gru=g, bwd={n: v for n, v in ops.att_path_counts(0).items() if v},
                         bwd_gru=dict(ops.att_gru_counts(0)))
    torch.cuda.synchronize()
    fwd, fraw = alternate({k: (lambda a=a: ops.att_decoder_fwd(a)) for k, a in loops.items()})
    bwd, braw = alternate({k: (lambda a=a: ops.att_decoder_bwd(a)) for k, a in loops.items()})
    rec['decoder_loops'] = dict(
        steps=To, fwd_us_per_step={k: v / To * 1e3 for k, v in fwd.items()},
        bwd_us_per_step={k: v / To * 1e3 for k, v in bwd.items()}, fwd_gru_over_lstm=fwd['gru'] / fwd['lstm'],
        bwd_gru_over_lstm=bwd['gru'] / bwd['lstm'], fwd_ms_all=fraw, bwd_ms_all=braw, path_counts=counts,
        cell_launches_per_step=dict(
            lstm=dict(fwd=1, bwd=2, note='forward: product + cell in one launch on the bf16 image; backward: the cell '
                      'backward rides in the query-FC backward launch (fused_q) and the dpre W^T product is one launch -- the '
                      'counters above say whether a step took these forms'),
            gru=dict(fwd=2, fwd_general=4, bwd=4, bwd_query_fc=1, note='forward: phase A + phase B; backward: two elementwise '
                     'kernels and two products, behind the separate query-FC backward product of the unfused branch')))
    print(json.dumps({k: rec['decoder_loops'][k] for k in ('fwd_us_per_step', 'bwd_us_per_step', 'fwd_gru_over_lstm',
                                                           'bwd_gru_over_lstm')}), flush=True)
    # the GRU cell's two forms against each other (same loop dict)
    a = loops['gru']

    def form(fused):
        def run():
            a['gru']['fused'] = fused
            ops.att_decoder_fwd(a)
        return run
    two, traw = alternate({'two_launch': form(True), 'four_launch': form(False)})
    a['gru']['fused'] = True
    rec['gru_cell_forms'] = dict(fwd_us_per_step={k: v / To * 1e3 for k, v in two.items()}, fwd_ms_all=traw)
    print(json.dumps(rec['gru_cell_forms']['fwd_us_per_step']), flush=True)

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
