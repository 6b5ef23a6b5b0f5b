#!/usr/bin/env python
"""Headline benchmark: acoustic frames/sec of BLSTM-CTC training on MI355X.

    python bench.py --gpus N --steps K --warmup W

Workload (BASELINE.json configs[1], SURVEY.md section 8d cfg B): TIMIT-61-shaped synthetic batch,
5x256 BLSTM-CTC, bf16 MFMA operands / fp32 state, B=16 utterances per GPU, D=120 (40 log-mel
x {static, delta, delta-delta}), C=62, seq_len ~ U{100..778}, L = clip(len//8, 5, 75);
recipe hyper-parameters of the repo's own config (blstm_ctc_100h_char.yml): rmsprop 1e-3,
clip_grad_norm 5, clip_activation 50, dropout 0.2.
A step = forward + CTC loss + backward + per-variable clip + (all-reduce) + optimizer update.

A plain run does what the headline needs and no more: it sets up, warms up, times the K steps and prints the result
line.  Its figures all come from the timed steps themselves: value / ms_per_step, step_ms, the serial kernels' event
times and the recurrence roofline derived from them (and, at N > 1, per_rank / comm).
  --dump-outputs DIR     after the timed steps, what the LAST timed step computed (loss, per-utterance CTC losses,
                         logits with the frames past each utterance's length zeroed, every updated parameter) as
                         DIR/<name>.npy in float32, <= 64 MB in all (a fixed seeded sample of each array beyond that);
                         the same arguments give the same inputs in every run, so two builds compare output for output;
  --full                 everything below that takes work or runs of its own (h2d_inclusive, parity, cpu_baseline, the
                         other configurations, other_padding at N > 1) and the complete result object written to the
                         files of FULL_RESULT_PATHS; the --no-* and --aux options select within it.
The LAST stdout line rank 0 prints is the compact form of the result (compact_line: numbers only, <= 6 000 bytes, the
driver keeps 8 000).  The full object holds
  value / ms_per_step    K steps bracketed by barrier + synchronize, inputs resident in HBM (the contract's number);
  step_ms                per-step durations from HIP events on the launch stream: median / min / max; the host's time
                         to ENQUEUE a step (host_issue_mean) and, apart from it, the time the host spent waiting for
                         the device (it runs at most three steps ahead: ops.ErrorWatch);
  h2d_inclusive          the same K steps with the batch uploaded from pinned host memory every step
                         (double-buffered on a copy stream, SURVEY 8d's step definition) -- reported, never `value`;
  parity                 CTC-loss match and greedy-label match against the CPU oracle on the same batch cut to its
                         first --cpu-tmax frames (computed outside the timed region, before training starts);
  roofline               dominant kernel, HIP-event duration measured live in the timed region;
  cpu_baseline           oracle/fast_cpu.py port of the TF1 CPU path on a bounded sample, thread sweep, best reported;
and, at N = 1, the other BASELINE configurations timed with the same harness (a few steps each):
  headline_f32           the headline shard itself with fp32 operands (20 steps): throughput and oracle parity at the
                         precision the north_star's 1e-4 / identical-labels statement is made at;
  cfgA                   configs[0] (TIMIT-39, 2x128, fp32): the configuration the 1e-4 fp32 loss tolerance is about;
  cfgC                   configs[2] VGG-BLSTM 4x512 CTC, B = 64;
  cfgD                   configs[3] 5x512 BLSTM joint CTC-attention (location), the per-GPU shard B = 32;
  cfgE                   configs[4] hybrid-attention encoder-decoder + CTC head at the kanji vocabulary, B = 32;
  decode                 greedy and prefix-beam CTC decode (TIMIT-61 width 20, kanji width 100) in utterances/s, the
                         oracle's restatement of the reference's numpy decoders timed beside them on one core;
  bgru                   the reference's GRU encoder family: bgru 2x256 CTC (fp32) on the headline batch;
  blstmp                 the reference's projected cells (lstm_impl='LSTMCell', num_proj): blstm 5x256 proj 128 CTC (operand dtype of the headline)
                         on the headline batch;
  input_width_D39, batch_scaling   the headline model at the other input width / at B = 32 .. 128 per GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: 8 TB/s spec
MFMA_BF16_PEAK_TF = 2500.0   # dense bf16
MFMA_F32_PEAK_TF = 157.3


_T0 = time.perf_counter()


def log(msg):
    """Progress on stderr with the seconds since start (stdout carries only the JSON line)."""
    sys.stderr.write('[bench %7.1f s] %s\n' % (time.perf_counter() - _T0, msg))
    sys.stderr.flush()


# ------------------------------------------------------------------------------------------------ synthetic batches
def make_batch(seed, B, D, C, tmin, tmax, label_div=8, label_lo=5, label_hi=75):
    rng = np.random.RandomState(seed)
    seq_len = rng.randint(tmin, tmax + 1, size=B).astype(np.int32)
    T = int(seq_len.max())
    x = rng.randn(B, T, D).astype(np.float32)
    labels = []
    for b in range(B):
        x[b, seq_len[b]:] = 0
        L = int(np.clip(seq_len[b] // label_div, label_lo, label_hi))
        labels.append(rng.randint(0, C - 1, size=L).tolist())
    return x, seq_len, labels, dense_labels(labels)


def dense_labels(labels):
    dense = np.full((len(labels), max(len(l) for l in labels)), -1, dtype=np.int64)
    for b, l in enumerate(labels):
        dense[b, :len(l)] = l
    return dense


def device_features(seed, seq_len, D, dev, T=None):
    """[B, T, D] ~ N(0,1) fp32, zero past seq_len, generated ON the device (the cfg C batch is 550 MB: numpy takes
    seconds for it).  Only for workloads whose timed loop keeps the batch resident."""
    g = torch.Generator(device=dev)
    g.manual_seed(int(seed))
    T = int(seq_len.max()) if T is None else int(T)
    x = torch.randn((len(seq_len), T, D), generator=g, device=dev, dtype=torch.float32)
    keep = torch.arange(T, device=dev).view(1, T, 1) < torch.as_tensor(seq_len, device=dev).view(-1, 1, 1)
    return x * keep


def truncate_batch(x, seq_len, labels, tcut, label_div=8):
    """The same utterances cut to their first tcut frames, labels cut to stay feasible (bounded CPU sample)."""
    sl = np.minimum(seq_len, tcut).astype(np.int32)
    xc = x[:, :int(sl.max())].copy()
    for b in range(len(sl)):
        xc[b, sl[b]:] = 0
    labs = [list(l[:max(1, int(n) // label_div)]) for l, n in zip(labels, sl)]
    return xc, sl, labs, dense_labels(labs)


# ------------------------------------------------------------------------------------------------ timing harness
def _conv_work(a, k):
    """flops of one 3x3 convolution call: x [n, H, W, Cin] against a weight image [Cout, 9 Cin] (ops.conv3x3_fwd*)."""
    n, H, W, Cin = a[0].shape
    return 2.0 * n * H * W * 9 * Cin * a[1].shape[0]


def _conv_bwd_weight_work(a, k):
    n, H, W, Cin = a[0].shape            # x [n, H, W, Cin], dY [n, H, W, Cout]
    return 2.0 * n * H * W * 9 * Cin * a[1].shape[3]


def _gemm_work(a, k):
    """(group, flops) of one ops.gemm call; the group names the operand layout (reduction-major = weight gradients)."""
    A, B = a[0], a[1]
    tA = bool(a[2]) if len(a) > 2 else bool(k.get('transA', False))
    tB = bool(a[3]) if len(a) > 3 else bool(k.get('transB', False))
    M, K = (A.shape[1], A.shape[0]) if tA else (A.shape[0], A.shape[1])
    N = B.shape[0] if tB else B.shape[1]
    return ('gemm_tn' if tA else ('gemm_nt' if tB else 'gemm_nn')), 2.0 * M * N * K


# per timed op: callable(args, kwargs) -> work units of THAT call (flops), or (record name, work units)
CALL_WORK = {'conv3x3_fwd': _conv_work, 'conv3x3_fwd_drop': _conv_work, 'conv3x3_bwd_data_relu': _conv_work,
             'conv3x3_bwd_weight': _conv_bwd_weight_work, 'conv3x3_bwd_weight_bias': _conv_bwd_weight_work,
             'gemm': _gemm_work}


class KernelTimer(object):
    """HIP-event brackets (torch.cuda.Event on the current stream == the launch stream of ops.*, inside ops.side_lane
    that lane's stream).  Every record keeps the work of ITS call (CALL_WORK), so a step that runs a kernel several times
    on parts of the batch (the VGG forward in runs of images) is credited call by call."""

    def __init__(self, ops, names):
        self.ops, self.names = ops, names
        self.records = {}
        self.enabled = False
        self._orig = {}

    def install(self):
        for n in self.names:
            orig = getattr(self.ops, n)
            self._orig[n] = orig
            work = CALL_WORK.get(n)

            def wrapped(*a, _n=n, _o=orig, _w=work, **k):
                if not self.enabled:
                    return _o(*a, **k)
                key, units = _n, 0.0
                if _w is not None:
                    w = _w(a, k)
                    key, units = w if isinstance(w, tuple) else (_n, w)
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                r = _o(*a, **k)
                e1.record()
                self.records.setdefault(key, []).append((e0, e1, units))
                return r
            setattr(self.ops, n, wrapped)

    def uninstall(self):
        for n, o in self._orig.items():
            setattr(self.ops, n, o)

    def summary(self):
        out = {}
        for n, evs in self.records.items():
            if evs:
                ms = [a.elapsed_time(b) for a, b, _ in evs]
                out[n] = dict(calls=len(ms), total_ms=float(np.sum(ms)), avg_us=float(np.mean(ms) * 1e3))
                work = float(sum(u for _, _, u in evs))
                if work:
                    out[n]['work'] = work
        return out


def fence(world):
    import torch.distributed as dist
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()


def time_steps(step, steps, warmup, world, dev_index, timed_ops=('lstm_fwd', 'lstm_bwd', 'ctc_loss')):
    """W untimed + K timed calls of step() between barrier + synchronize; per-step HIP events; host issue time with
    the ErrorWatch's wait for the device (the host may run three steps ahead, no more) accounted separately."""
    from tensorflow_end2end_speech_recognition_amd import ops
    # only the serial kernels are bracketed: an event pair around each of the ~40 small GEMMs of a step costs
    # milliseconds of queue serialisation and would distort the number being measured
    timer = KernelTimer(ops, list(timed_ops))
    timer.install()
    try:
        for _ in range(warmup):
            loss = step()
        fence(world)
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
        waited0 = ops.watch_waited_seconds(dev_index)
        host = 0.0
        timer.enabled = True
        t0 = time.perf_counter()
        marks[0].record()
        for i in range(steps):
            h0 = time.perf_counter()
            loss = step()
            marks[i + 1].record()
            host += time.perf_counter() - h0
        fence(world)
        elapsed = time.perf_counter() - t0
        timer.enabled = False
    finally:
        timer.uninstall()
    waited = ops.watch_waited_seconds(dev_index) - waited0
    per_step = np.array([marks[i].elapsed_time(marks[i + 1]) for i in range(steps)])
    return dict(elapsed=elapsed, final_loss=float(loss.item()), kernels=timer.summary(),
                handoff_flags=ops.check_async_errors(dev_index),   # sticky error word of the multi-CU recurrence kernels
                step_ms=dict(median=float(np.median(per_step)), min=float(per_step.min()), max=float(per_step.max()),
                             slow_steps=[[int(i), round(float(per_step[i]), 3)] for i in np.flatnonzero(per_step > 1.15 * np.median(per_step))[:10]],
                             host_issue_mean=(host - waited) / steps * 1e3, host_wait_for_device_mean=waited / steps * 1e3,
                             note='HIP events between steps on the launch stream; host_issue = Python + C time to enqueue '
                                  'one step; host_wait_for_device = time the issue loop spent blocked because it was '
                                  'three steps ahead of the GPU (the step is device-bound while this is > 0)'))


# ------------------------------------------------------------------------------------------------ parity / CPU legs
def parity_vs_oracle(model, x, seq_len, labels, L, dtype, tcut):
    """Device loss / greedy labels against the CPU oracle on the batch cut to its first tcut frames.  For the bf16
    operand path the oracle is evaluated on the bf16-rounded operands (inputs, kernels, emitted h), so what is compared
    is the arithmetic, not the precision choice; for fp32 it is the plain fp64 oracle (tolerance 1e-4, north_star)."""
    from oracle import decoders as odec
    from oracle import lstm as olstm
    from oracle import model as omodel
    from tensorflow_end2end_speech_recognition_amd.utils.io.labels.sparsetensor import sparsetensor2list
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    xc, sl, labs, dn = truncate_batch(x, seq_len, labels, tcut)
    t0 = time.perf_counter()
    sd = {k: v.cpu().numpy() for k, v in model.store.state_dict().items()}
    ref = omodel.ctc_model_forward(sd, xc, labs, sl, L, cell_clip=50.0, want_grads=False,
                                   operand_round=olstm.bf16_round_t if dtype == 'bf16' else None)
    loss, logits = model.compute_loss(xc, dn, sl, keep_prob=1.0, is_training=False)
    B = len(sl)
    C = logits.shape[2]
    hyp = [list(h) for h in sparsetensor2list(model.decoder(logits, sl, beam_width=1), B)]
    ref_hyp = odec.greedy_decode(np.transpose(ref['logits'], (1, 0, 2)), sl, C - 1)
    per_utt = np.abs(model.ctc_losses.cpu().numpy() - ref['ctc_losses']) / np.abs(ref['ctc_losses'])
    return dict(loss_device=float(loss.item()), loss_oracle=float(ref['total_loss']),
                loss_rel_err_vs_oracle=abs(float(loss.item()) - ref['total_loss']) / abs(ref['total_loss']),
                per_utterance_loss_rel_err_max=float(per_utt.max()),
                greedy_label_mismatch=int(sum(h != r for h, r in zip(hyp, ref_hyp))),
                greedy_labels_compared=int(sum(len(r) for r in ref_hyp)), utterances=B,
                oracle='oracle.model fp64' + (' on bf16-rounded operands' if dtype == 'bf16' else ''),
                sample='first %d frames of every utterance of the timed batch (%d valid frames), dropout off'
                       % (tcut, int(sl.sum())), seconds=time.perf_counter() - t0)


def cpu_baseline_blstm_ctc(args, wl, model, x, seq_len, labels):
    """oracle/fast_cpu.py (torch-CPU fp32 restatement of the TF1 CPU step) on the timed batch cut to its first
    --cpu-tmax frames.  Thread sweep over the box's host cores on a short probe (the batch cut to 32 frames, one step
    each: the per-step loop of small matrix products does not scale with threads, and 256 threads on a 256-core host
    take minutes per step on the full sample), then the full sample at the probe's best thread count."""
    from oracle import fast_cpu
    sd = {k: v.cpu().numpy() for k, v in model.store.state_dict().items()}
    ncpu = os.cpu_count() or 1
    # (never all cores: on the 256-core GPU box a 256-thread run of even the 32-frame probe did not finish in 6 minutes,
    # and 64 threads are already 5x slower than 16 -- the per-step loop is latency-bound on the CPU as well)
    sweep = sorted(set(min(int(t), ncpu, 64) for t in args.cpu_threads.split(',') if t))
    xp, slp, labp, _ = truncate_batch(x, seq_len, labels, 32)
    probes = []
    for nt in sweep:
        cm = fast_cpu.CpuBLSTMCTC(sd, wl['layers'], cell_clip=50.0, clip_grad_norm=5.0, threads=nt, optimizer='rmsprop')
        t = fast_cpu.time_train_steps(cm, xp, labp, slp, steps=1, warmup=1)
        probes.append(dict(threads=nt, frames_per_s=int(slp.sum()) / t, seconds_per_step=t))
        log('cpu probe %d threads: %.2f s/step' % (nt, t))
    best_nt = max(probes, key=lambda r: r['frames_per_s'])['threads']
    xc, sl, labs, _ = truncate_batch(x, seq_len, labels, args.cpu_tmax)
    cframes = int(sl.sum())
    cm = fast_cpu.CpuBLSTMCTC(sd, wl['layers'], cell_clip=50.0, clip_grad_norm=5.0, threads=best_nt, optimizer='rmsprop')
    t = fast_cpu.time_train_steps(cm, xc, labs, sl, steps=args.cpu_steps, warmup=1)
    return dict(value=cframes / t, unit='frames/s', cores=best_nt, kind='port', host_cores=ncpu,
                thread_sweep_probe=probes, seconds_per_step=t,
                sample='%d timed training step(s) after 1 warm-up step of the same %d-utterance batch cut to its first '
                       '%d frames (%d valid frames), rmsprop, torch-CPU fp32 restatement of the TF1 path '
                       '(oracle/fast_cpu.py) at %d threads -- the best of a sweep over %s threads of the %d-core host '
                       'on a 32-frame probe of the same batch (more threads are slower: 64 threads 5x, all cores do not finish; a 512-frame cut takes 33 s per step at '
                       '16 threads -- 176 frames/s -- against 1.5 s for this 256-frame one, so the shorter cut favours the CPU)'
                       % (args.cpu_steps, wl['batch'], args.cpu_tmax, cframes, best_nt, [r['threads'] for r in probes], ncpu))


def cpu_baseline_oracle_call(fn, frames, what, threads):
    """One forward + backward of the oracle's model function (fp32, autograd) on a bounded sample."""
    torch.set_num_threads(threads)
    fn()                                   # warm-up (thread pool, allocator)
    t0 = time.perf_counter()
    fn()
    t = time.perf_counter() - t0
    return dict(value=frames / t, unit='frames/s', cores=threads, kind='port', host_cores=os.cpu_count() or 1,
                seconds_per_step=t, sample=what)


# ------------------------------------------------------------------------------------------------ rooflines
def recurrence_roofline(H, frames_dirs, T, dtype, ks, traffic=None, traffic_source=None, tiles=1, steps=None):
    """Roofline entry of the dominant recurrence kernel.  Algorithmic HBM bytes per launch:
      fwd: read x W_x + b 16H, write gates s*4H + c 4H + h s*H     per valid frame per direction
      bwd: read gates s*4H + c 4H + dh 4H, write dgates s*4H       per valid frame per direction
    + W_h once per direction; `frames_dirs` = valid frames x directions of one launch."""
    dom = max(('lstm_fwd', 'lstm_bwd'), key=lambda n: ks.get(n, {}).get('total_ms', 0))
    if dom not in ks:
        return None
    s_act = 2 if dtype == 'bf16' else 4
    per_frame = {'lstm_fwd': 20 * H + 5 * s_act * H, 'lstm_bwd': 8 * H + 8 * s_act * H}[dom]
    flops_frame = 2 * 4 * H * H   # recurrent h W_h (fwd) / dG W_h^T (bwd), per frame per direction
    bytes_launch = frames_dirs * per_frame + 2 * 4 * H * H * s_act
    dur = ks[dom]['avg_us'] * 1e-6
    ach = bytes_launch / dur / 1e9
    peak_tf = MFMA_BF16_PEAK_TF if dtype == 'bf16' else MFMA_F32_PEAK_TF
    return dict(kernel=dom, bound='hbm', achieved=ach, peak=HBM_PEAK_GBS, unit='GB/s', frac=ach / HBM_PEAK_GBS,
                traffic=traffic, traffic_source=traffic_source, avg_launch_us=ks[dom]['avg_us'],
                us_per_recurrence_step=ks[dom]['avg_us'] / T, algorithmic_bytes_per_launch=bytes_launch,
                ms_per_step=(ks[dom]['total_ms'] / steps) if steps else None,
                mfma_tflops=frames_dirs * flops_frame / dur / 1e12,
                mfma_frac=frames_dirs * flops_frame / dur / 1e12 / peak_tf, utterance_tiles_per_direction=tiles,
                note='serial recurrence over T frames, one 16-utterance MFMA tile per cluster: bound by the per-step '
                     'chain (LDS operand reads, gate math issue, one cross-CU L2 hop), not by HBM or MFMA throughput '
                     '(DESIGN.md section 4); traffic = HBM bytes per launch from a separate rocprofv3 --pmc pass '
                     '(profiles/pmc_hbm_traffic.json), null if no pass matches this workload')


def conv_roofline(F, W, frames, steps, ks):
    """MFMA entry of cfg C's image-resident forward convolutions (conv3x3_img_kernel<64,64>, <64,128>, <128,128>;
    ops.conv3x3_fwd / conv3x3_fwd_drop).  achieved = the flops of the timed calls / their HIP-event time, CALL BY CALL
    (`work` of KernelTimer: 2 * images * pixels * 9 * Cin * Cout of the images that call processed): the VGG forward goes
    through in ASR_VGG_FWD_CHUNKS runs of images (vgg_blstm.py), so a step makes several calls per kernel on part of the
    batch each -- counting calls as steps doubled this figure in round 5.  `steps` = the timed steps of the loop; the
    summed work must equal steps x valid frames x the per-frame figure (2 * pixels * 9 * Cin * Cout with F x W pixels
    before and ceil(F/2) x ceil(W/2) after the first pool, models/encoders/core/vgg_blstm.py:113-151).  Calls of two runs
    overlap on two lanes: summing their event times can only UNDERSTATE the rate."""
    ka, kb = ks.get('conv3x3_fwd'), ks.get('conv3x3_fwd_drop')
    if not ka or not kb or not steps:
        return None
    p1, p2 = F * W, ((F + 1) // 2) * ((W + 1) // 2)
    flops_frame = 2.0 * 9 * (p1 * 64 * 64 + p2 * 64 * 128 + p2 * 128 * 128)
    assert ka['calls'] % steps == 0 and kb['calls'] % steps == 0 and ka['calls'] == 2 * kb['calls'], \
        (ka['calls'], kb['calls'], steps)
    work = ka.get('work', 0.0) + kb.get('work', 0.0)
    expect = flops_frame * frames * steps
    assert abs(work - expect) <= 1e-6 * expect, ('timed convolution calls do not add up to the batch', work, expect)
    total_ms = ka['total_ms'] + kb['total_ms']
    ach = work / (total_ms * 1e-3) / 1e12
    return dict(kernel='conv3x3_img_fwd', bound='mfma', achieved=ach,
                peak=MFMA_BF16_PEAK_TF, unit='TFLOP/s', frac=ach / MFMA_BF16_PEAK_TF, traffic=None,
                avg_launch_us=total_ms * 1e3 / (ka['calls'] + kb['calls']), calls_per_step=(ka['calls'] + kb['calls']) // steps,
                ms_per_step=total_ms / steps, algorithmic_flops_per_frame=flops_frame,
                note='flops of the timed calls (2 * images * pixels * 9 * Cin * Cout each) / their summed HIP-event time: '
                     'the three image-resident forward convolutions (ReLU + bias, one of them + dropout, in the epilogue)')


def mfma_group_roofline(name, k, steps):
    """MFMA entry of one group of timed matrix calls (ops.gemm by operand layout, convolution gradients): the flops of
    the calls / their summed HIP-event time on the lanes they ran on."""
    if not k or not k.get('work'):
        return None
    ach = k['work'] / (k['total_ms'] * 1e-3) / 1e12
    return dict(kernel=name, bound='mfma', achieved=ach, peak=MFMA_BF16_PEAK_TF, unit='TFLOP/s', frac=ach / MFMA_BF16_PEAK_TF,
                traffic=None, avg_launch_us=k['avg_us'], calls_per_step=k['calls'] / float(steps), ms_per_step=k['total_ms'] / steps)


def dominant_roofline(entries):
    """Of {name: roofline entry with ms_per_step}, the one whose calls took the most event time per step."""
    live = {n: e for n, e in entries.items() if e and e.get('ms_per_step')}
    return max(live.values(), key=lambda e: e['ms_per_step']) if live else None


def ops_flags(dev_index):
    from tensorflow_end2end_speech_recognition_amd import ops
    return ops.check_async_errors(dev_index)


def load_traffic_table():
    tpath = os.path.join(ROOT, 'profiles', 'pmc_hbm_traffic.json')
    return json.load(open(tpath)) if os.path.exists(tpath) else None


# ------------------------------------------------------------------------------------------------ --dump-outputs
DUMP_LIMIT = 63 << 20     # bytes of array data in all: with the .npy headers the directory stays under 64 MB


def dump_outputs(out_dir, model, last, seq_len, limit=DUMP_LIMIT):
    """What the last timed step handed back to its caller, as float32 out_dir/<name>.npy: loss (0-dim), ctc_losses [B],
    logits [T, B, C] (time-major; frames past each utterance's length set to 0, nothing defines them) and every
    parameter after the step's update (param.<variable name with '/' -> '.'>).  Beyond `limit` bytes in all, every
    array keeps the same fraction of its entries, flattened, at indices drawn with a fixed seed (in index order).
    Returns {file name: bytes of array data}."""
    arrays = {'loss': last['loss'], 'ctc_losses': model.ctc_losses, 'logits': last['logits']}
    for n, v in model.store.state_dict().items():
        arrays['param.' + n.replace('/', '.')] = v
    arrays = {k: v.detach().float().cpu().contiguous().numpy() for k, v in arrays.items()}
    lg = arrays['logits']
    lg[np.arange(lg.shape[0])[:, None] >= np.asarray(seq_len)[None, :]] = 0.0
    frac = min(1.0, float(limit) / sum(a.nbytes for a in arrays.values()))
    os.makedirs(out_dir, exist_ok=True)
    written = {}
    for name, a in arrays.items():
        if frac < 1.0 and a.size > 1:
            idx = np.sort(np.random.RandomState(0).choice(a.size, max(1, int(a.size * frac)), replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(out_dir, name + '.npy'), a)
        written[name + '.npy'] = a.nbytes
    return written


# ------------------------------------------------------------------------------------------------ BLSTM-CTC workloads
def run_blstm_ctc(args, wl, dev, world, rank, dev_index, steps, warmup, want_parity, want_h2d, want_cpu, dump_dir=None):
    """Times one BLSTM-CTC workload description `wl` on this rank; returns the result dict (rank 0 aggregates).
    dump_dir: write what the last timed step computed there (dump_outputs), before any further leg trains the model."""
    import torch.distributed as dist
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    from tensorflow_end2end_speech_recognition_amd.utils.training import multi_gpu

    H, L, C = wl['units'], wl['layers'], wl['classes'] + 1
    # every rank gets its own shard of the global batch (weak scaling: B per GPU fixed)
    x, seq_len, labels, dense = make_batch(wl['seed'] + rank, wl['batch'], wl['input_size'], C, wl['tmin'], wl['tmax'])
    if world > 1 and wl.get('global_tmax', True):
        # the reference pads the GLOBAL batch to its longest utterance and then splits it (utils/dataset/ctc.py:137-139,
        # :171-182): every tower runs Tmax(global) recurrence steps, so do the ranks here
        tg = torch.tensor([x.shape[1]], device=dev, dtype=torch.int64)
        dist.all_reduce(tg, op=dist.ReduceOp.MAX)
        if int(tg.item()) > x.shape[1]:
            x = np.concatenate([x, np.zeros((x.shape[0], int(tg.item()) - x.shape[1], x.shape[2]), np.float32)], 1)
    model = CTC('blstm', wl['input_size'], H, L, wl['classes'], parameter_init=0.1, clip_grad_norm=5.0,
                clip_activation=50, dtype=wl['dtype'], device=str(dev), seed=0)
    multi_gpu.broadcast_parameters(model.store)
    frames = int(seq_len.sum())
    res = dict(frames=frames, T=int(x.shape[1]))
    if want_parity and rank == 0:
        res['parity'] = parity_vs_oracle(model, x, seq_len, labels, L, wl['dtype'], args.cpu_tmax)
        log('parity leg done in %.1f s' % res['parity']['seconds'])
    xd = torch.tensor(x, device=dev)
    sld = torch.tensor(seq_len, device=dev)
    opt = model._set_optimizer('rmsprop', 1e-3)
    cur = [xd]
    last = {}                # what the latest step handed back to its caller (dump_dir only)
    comm_events = []
    if world > 1:     # duration of the collectives on the communication stream (HIP events on that stream)
        orig_ar = multi_gpu._allreduce_mean_

        def timed_ar(t):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = orig_ar(t)
            e1.record()
            comm_events.append((e0, e1, t.numel() * 4))
            return r
        multi_gpu._allreduce_mean_ = timed_ar

    def step():
        loss, logits = model.compute_loss(cur[0], dense, sld, keep_prob=wl['keep_prob'])
        # gradients -> per-variable clip on the tower (BEFORE averaging) -> mean over towers: per group of encoder
        # layers on a communication stream under the BPTT of the layers below when N > 1 (multi_gpu.BucketedAverager)
        multi_gpu.clip_and_average(model, opt, loss)
        opt.apply_gradients(None)
        if dump_dir:
            last['loss'], last['logits'] = loss, logits
        return loss

    log('%dx%d %s B=%d: timing %d steps' % (L, H, wl['dtype'], wl['batch'], steps))
    res.update(time_steps(step, steps, warmup, world, dev_index))
    log('   %.3f ms/step' % (res['elapsed'] / steps * 1e3))
    if dump_dir:
        res['dumped'] = dump_outputs(dump_dir, model, last, seq_len)
        log('outputs of the last timed step: %d arrays, %.1f MB in %s' % (len(res['dumped']), sum(res['dumped'].values()) / 1e6, dump_dir))
    if world > 1:
        multi_gpu._allreduce_mean_ = orig_ar
        n_timed = len(comm_events) * steps // (steps + warmup)     # the warm-up steps' collectives come first
        ev = comm_events[-n_timed:] if n_timed else []
        ms = [a.elapsed_time(b) for a, b, _ in ev]
        avg = multi_gpu.averager_for(model)
        res['comm'] = dict(allreduce_calls_per_step=len(ev) / max(steps, 1), allreduce_ms_per_step=float(np.sum(ms)) / max(steps, 1),
                           bytes_per_step=float(sum(n for _, _, n in ev)) / max(steps, 1),
                           bucket_min_mb=getattr(avg, 'bucket_min_bytes', 0) / float(1 << 20),
                           buckets=[dict(layers=list(b.get('layers', ())), mbytes=(b['end'] - b['start']) * 4 / 1e6)
                                    for b in avg.buckets] + [dict(rest=True, mbytes=(b['end'] - b['start']) * 4 / 1e6)
                                                             for b in avg.rest],
                           note='HIP events on the communication stream around each clip + all-reduce(mean) of a '
                                'gradient bucket; these run beside the BPTT kernels of the layers below')
    if want_h2d:
        # the same K steps with the batch coming from pinned host memory each step: upload of step i+1 on a copy
        # stream under the compute of step i (what a prefetching input pipeline does); all K uploads in the bracket
        xp = torch.from_numpy(x).pin_memory()
        bufs = [torch.empty_like(xd), torch.empty_like(xd)]
        copy_stream = torch.cuda.Stream(device=dev)
        ready = [None, None]
        done = [None, None]

        def upload(i):
            with torch.cuda.stream(copy_stream):
                if done[i % 2] is not None:
                    copy_stream.wait_event(done[i % 2])        # the step that last read this buffer has finished
                bufs[i % 2].copy_(xp, non_blocking=True)
                e = torch.cuda.Event()
                e.record(copy_stream)
                ready[i % 2] = e
        fence(world)
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
        t0 = time.perf_counter()
        upload(0)
        marks[0].record()
        for i in range(steps):
            if i + 1 < steps:
                upload(i + 1)
            torch.cuda.current_stream().wait_event(ready[i % 2])
            cur[0] = bufs[i % 2]
            step()
            e = torch.cuda.Event()
            e.record()
            done[i % 2] = e
            marks[i + 1].record()
        fence(world)
        res['elapsed_h2d'] = time.perf_counter() - t0
        res['h2d_median_ms'] = float(np.median([marks[i].elapsed_time(marks[i + 1]) for i in range(steps)]))
        cur[0] = xd
    if want_cpu and rank == 0:
        res['cpu_baseline'] = cpu_baseline_blstm_ctc(args, wl, model, x, seq_len, labels)
        log('cpu baseline done: %.0f frames/s at %d threads' % (res['cpu_baseline']['value'], res['cpu_baseline']['cores']))
    del model, opt
    return res


def blstm_ctc_entry(args, wl, res, steps, desc):
    """The JSON object of an auxiliary BLSTM-CTC workload (N = 1)."""
    ks = res['kernels']
    tt = load_traffic_table()
    key = '%dx%d_%s_B%d_T%d' % (wl['layers'], wl['units'], wl['dtype'], wl['batch'], wl['tmax'])
    traffic = src = None
    dom = max(('lstm_fwd', 'lstm_bwd'), key=lambda n: ks.get(n, {}).get('total_ms', 0))
    if tt and key in tt.get('workloads', {}):
        traffic, src = tt['workloads'][key].get(dom), tt.get('source')
    return dict(workload=desc, value=res['frames'] * steps / res['elapsed'], unit='frames/s', dtype=wl['dtype'],
                steps=steps, ms_per_step=res['elapsed'] / steps * 1e3, step_ms=res['step_ms'],
                final_loss=res['final_loss'], cluster_handoff_flags=res['handoff_flags'], parity=res.get('parity'),
                kernels=ks, roofline=recurrence_roofline(wl['units'], res['frames'] * 2, res['T'], wl['dtype'], ks,
                                                         traffic, src, tiles=(wl['batch'] + 15) // 16),
                cpu_baseline=res.get('cpu_baseline'))


# ------------------------------------------------------------------------------------------------ cfg C
def run_cfgC(args, dev, dev_index):
    """BASELINE configs[2] (SURVEY 8d cfg C, seed 2): LibriSpeech-100h-character-shaped batch, B = 64, F = 40 mel x
    {static, d, dd}, splice 11 -> D = 1320, seq_len ~ U{150..1650}, L = len // 7 over 28 characters, VGG front-end +
    4x512 BLSTM + 29-class CTC, bf16 operands, dropout 0.2, rmsprop 1e-3."""
    from oracle import lstm as olstm
    from oracle import model as omodel
    from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
    B, F, W, H, L, C = 64, 40, 11, 512, 4, 28
    rng = np.random.RandomState(2)
    seq_len = rng.randint(150, 1651, size=B).astype(np.int32)
    labels = [rng.randint(0, C, size=max(1, int(n) // 7)).tolist() for n in seq_len]
    dense = dense_labels(labels)
    xd = device_features(2, seq_len, F * W * 3, dev)
    sld = torch.tensor(seq_len, device=dev)
    model = CTC('vgg_blstm', 3 * F, H, L, C, splice=W, parameter_init=0.1, clip_grad_norm=5.0, clip_activation=50,
                dtype='bf16', device=str(dev), seed=0)

    def step():
        loss, _ = model.compute_loss(xd, dense, sld, keep_prob=0.8)
        model.train(loss, 'rmsprop', 1e-3)
        return loss
    steps = args.aux_steps
    res = time_steps(step, steps, args.aux_warmup, 1, dev_index,
                     timed_ops=('lstm_fwd', 'lstm_bwd', 'ctc_loss', 'conv3x3_fwd', 'conv3x3_fwd_drop',
                                'conv3x3_bwd_data_relu', 'conv3x3_bwd_weight_bias', 'gemm'))
    frames = int(seq_len.sum())
    T = int(seq_len.max())
    ks = res['kernels']
    # one roofline entry per group of timed calls; `roofline` is the group that took the most event time per step
    # (the entry named the best matrix kernel, not the dominant one), the others sit beside it
    groups = dict(recurrence=recurrence_roofline(H, frames * 2, T, 'bf16', ks, tiles=B // 16, steps=steps),
                  conv_fwd=conv_roofline(F, W, frames, steps, ks),
                  conv_bwd_data=mfma_group_roofline('conv3x3_bwd_data_relu', ks.get('conv3x3_bwd_data_relu'), steps),
                  conv_bwd_weight=mfma_group_roofline('conv3x3_bwd_weight_bias', ks.get('conv3x3_bwd_weight_bias'), steps),
                  gemm_tn=mfma_group_roofline('gemm_tn_bf16 (weight gradients, side lanes)', ks.get('gemm_tn'), steps),
                  gemm_nt=mfma_group_roofline('gemm_nt_bf16 (projections, dx)', ks.get('gemm_nt'), steps),
                  gemm_nn=mfma_group_roofline('gemm_nn', ks.get('gemm_nn'), steps))
    out = dict(workload='LibriSpeech-100h char shaped: VGG (40x11x3 frame images) + 4x512 BLSTM + CTC(29), B=64, '
                        'D=1320, seq_len~U{150..1650}, bf16 operands, dropout 0.2, rmsprop, train step',
               value=frames * steps / res['elapsed'], unit='frames/s', dtype='bf16', steps=steps,
               frames_per_step=frames, ms_per_step=res['elapsed'] / steps * 1e3, step_ms=res['step_ms'],
               final_loss=res['final_loss'], cluster_handoff_flags=res['handoff_flags'], kernels=ks,
               algorithmic_flops_per_frame=399.3e6,
               mfma_frac_whole_step=399.3e6 * frames * steps / res['elapsed'] / 1e12 / MFMA_BF16_PEAK_TF,
               roofline=dominant_roofline(groups), roofline_groups=groups,
               roofline_conv=groups['conv_fwd'], roofline_recurrence=groups['recurrence'],
               parity_tests='model-level parity at these widths: tests/test_gpu_configs.py::test_cfgC_vgg_blstm_4x512_bf16_ragged_two_tiles')
    if not args.no_parity:
        # bounded parity leg: the first 4 utterances cut to 48 frames, dropout off, against the fp64 oracle evaluated at
        # the device path's rounding points
        nb, tc = 4, 48
        t0 = time.perf_counter()
        sd = {k: v.cpu().numpy() for k, v in model.store.state_dict().items()}
        xc = xd[:nb, :tc].cpu().numpy()
        slc = np.minimum(seq_len[:nb], tc).astype(np.int32)
        labs = [l[:max(1, tc // 7)] for l in labels[:nb]]
        ref = omodel.ctc_model_forward(sd, xc, labs, slc, L, ndir=2, cell_clip=50.0, vgg=(F, W), want_grads=False,
                                       operand_round=olstm.bf16_round_t)
        loss_c, _ = model.compute_loss(xc, dense_labels(labs), slc, keep_prob=1.0, is_training=False)
        per = np.abs(model.ctc_losses.cpu().numpy()[:nb] - ref['ctc_losses']) / np.abs(ref['ctc_losses'])
        out['parity'] = dict(loss_device=float(loss_c.item()), loss_oracle=float(ref['total_loss']),
                             loss_rel_err_vs_oracle=abs(float(loss_c.item()) - ref['total_loss']) / abs(ref['total_loss']),
                             per_utterance_loss_rel_err_max=float(per.max()), utterances=nb,
                             oracle='oracle.model fp64 on bf16-rounded operands',
                             sample='first %d utterances cut to %d frames, dropout off' % (nb, tc),
                             seconds=time.perf_counter() - t0)
    if not args.no_cpu_baseline:
        # bounded CPU sample: the first 4 utterances cut to 48 frames through the oracle's VGG + BLSTM + CTC model
        # (fp32 autograd forward + backward; no optimizer step -- favours the CPU)
        nb, tc = 4, 48
        sd = {k: v.cpu().numpy() for k, v in model.store.state_dict().items()}
        xc = xd[:nb, :tc].cpu().numpy()
        slc = np.minimum(seq_len[:nb], tc)
        labs = [l[:max(1, tc // 7)] for l in labels[:nb]]
        th = min(16, os.cpu_count() or 1)
        out['cpu_baseline'] = cpu_baseline_oracle_call(
            lambda: omodel.ctc_model_forward(sd, xc, labs, slc, L, ndir=2, cell_clip=50.0, vgg=(F, W), dtype=torch.float32),
            int(slc.sum()), 'forward + backward (no update) of oracle.model.ctc_model_forward(vgg=(40, 11)) in fp32 on the '
            'first %d utterances cut to %d frames (%d frames), %d threads' % (nb, tc, int(slc.sum()), th), th)
    del model
    return out


# ------------------------------------------------------------------------------------------------ cfg D / E
def run_attention_cfg(args, dev, dev_index, which):
    """BASELINE configs[3] (cfg D, seed 3: 5x512 BLSTM encoder on D = 240, LOCATION attention A = 128, LSTM decoder
    U = 512, embedding 64, 28 characters, lambda = 0.5, per-GPU shard B = 32, seq_len ~ U{100..1600}, L = len // 4 + 2)
    and configs[4] (cfg E, seed 4: D = 246, HYBRID attention, 3 386 kanji -> 3 388-class softmax + 3 387-class CTC head,
    seq_len ~ U{100..1000}, L = len // 6 + 2).  bf16 encoder operands, dropout 0.2 everywhere, adam 1e-3."""
    from oracle import attention as oatt
    from tensorflow_end2end_speech_recognition_amd import ops
    from tensorflow_end2end_speech_recognition_amd.models.attention.joint_ctc_attention import JointCTCAttention
    if which == 'D':
        seed, D, C, att, tlo, thi, ldiv = 3, 240, 28, 'location', 100, 1600, 4
    else:
        seed, D, C, att, tlo, thi, ldiv = 4, 246, 3386, 'hybrid', 100, 1000, 6
    B, H, L, U, A, Em = 32, 512, 5, 512, 128, 64
    rng = np.random.RandomState(seed)
    seq_len = rng.randint(tlo, thi + 1, size=B).astype(np.int32)
    lens = np.maximum(1, seq_len // ldiv)
    Lmax = int(lens.max()) + 2
    labels = np.full((B, Lmax), C + 1, dtype=np.int64)
    ctc = np.full((B, int(lens.max())), -1, dtype=np.int64)
    for b in range(B):
        y = rng.randint(0, C, size=lens[b])
        labels[b, 0] = C
        labels[b, 1:1 + lens[b]] = y
        ctc[b, :lens[b]] = y
    xd = device_features(seed, seq_len, D, dev)
    model = JointCTCAttention(input_size=D, encoder_type='blstm', encoder_num_units=H, encoder_num_layers=L,
                              encoder_num_proj=None, attention_type=att, attention_dim=A, decoder_type='lstm',
                              decoder_num_units=U, decoder_num_layers=1, embedding_dim=Em, lambda_weight=0.5,
                              num_classes=C, sos_index=C, eos_index=C + 1, max_decode_length=Lmax, parameter_init=0.1,
                              clip_grad_norm=5.0, clip_activation_encoder=50, clip_activation_decoder=50, dtype='bf16',
                              seed=5, device=str(dev))

    # greedy attention inference (attention_seq2seq.py:462-509) through the native loop: encoder + up to
    # max_decode_length decoder steps with the output head, argmax and embedding feedback on the device, one read-back
    try:
        model.infer(xd, seq_len)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reps = 2
        for _ in range(reps):
            ids = model.infer(xd, seq_len)
        tinf = (time.perf_counter() - t0) / reps
        infer_rec = dict(tokens_per_s=B * ids.shape[1] / tinf, ms_per_call=tinf * 1e3, decoded_steps=int(ids.shape[1]),
                         steps_issued=int(model._infer_raw['steps_issued']), batch=B,
                         note='encoder forward + native greedy decoder loop (asr_att_decoder_infer) on the training batch with '
                              'the FRESHLY INITIALISED weights, i.e. before the timed training steps (rows then rarely emit EOS: '
                              'max_decode_length steps; round 5 ran this leg after training, where the cfg E model had learnt to '
                              'stop after 9 tokens and the figure was the encoder time over 288 tokens)')
    except Exception as e:
        infer_rec = dict(error=repr(e)[:300])
    def step():
        loss, *_ = model.compute_loss(xd, labels, ctc, seq_len, lens + 2, 0.8, 0.8, 0.8)
        model.train(loss, 'adam', 1e-3)
        return loss
    steps = args.aux_steps
    res = time_steps(step, steps, args.aux_warmup, 1, dev_index,
                     timed_ops=('lstm_fwd', 'lstm_bwd', 'ctc_loss', 'att_decoder_fwd', 'att_decoder_bwd'))
    frames = int(seq_len.sum())
    T = int(seq_len.max())
    desc = ('LibriSpeech-960h shaped per-GPU shard: 5x512 BLSTM + joint CTC-attention (location, A=128, U=512, E=64, '
            'C=28, lambda 0.5), B=32, D=240, seq_len~U{100..1600}, %d decoder steps' % (Lmax - 1)) if which == 'D' else \
           ('CSJ-kanji shaped per-GPU shard: 5x512 BLSTM + hybrid attention decoder (3388 classes) + CTC head (3387), '
            'B=32, D=246, seq_len~U{100..1000}, %d decoder steps' % (Lmax - 1))
    out = dict(workload=desc + ', bf16 encoder operands, dropout 0.2, adam, train step', value=frames * steps / res['elapsed'],
               unit='frames/s', dtype='bf16', steps=steps, frames_per_step=frames, decoder_steps=Lmax - 1,
               ms_per_step=res['elapsed'] / steps * 1e3, step_ms=res['step_ms'], final_loss=res['final_loss'],
               cluster_handoff_flags=res['handoff_flags'], kernels=res['kernels'],
               roofline=recurrence_roofline(H, frames * 2, T, 'bf16', res['kernels'], tiles=B // 16),
               greedy_infer=infer_rec,
               parity_tests='model-level parity at these widths: tests/test_gpu_configs.py::test_cfg%s_*' % which)
    if not args.no_parity:
        # bounded parity leg: 4 utterances cut to 64 frames / 10 labels, dropout off, against the fp64 oracle evaluated at
        # the device path's rounding points (teacher-forced joint loss)
        from oracle import lstm as olstm
        nb, tc, lc = 4, 64, 10
        t0 = time.perf_counter()
        sd = {k: v.cpu().numpy() for k, v in model.store.state_dict().items()}
        xc = xd[:nb, :tc].cpu().numpy()
        slc = np.minimum(seq_len[:nb], tc).astype(np.int32)
        lab_c = np.full((nb, lc + 2), C + 1, dtype=np.int64)
        lab_c[:, 0] = C
        lab_c[:, 1:1 + lc] = labels[:nb, 1:1 + lc]
        ctc_d = np.asarray(lab_c[:, 1:1 + lc])
        ref = oatt.attention_model_forward(sd, xc, lab_c, slc, np.full(nb, lc + 2), L, att, clip_enc=50.0, clip_dec=50.0,
                                           ctc_labels=[[int(v) for v in r] for r in ctc_d], lambda_weight=0.5,
                                           operand_round=olstm.bf16_round_t)
        loss_c, *_ = model.compute_loss(xc, lab_c, ctc_d, slc, np.full(nb, lc + 2), 1.0, 1.0, 1.0, is_training=False)
        out['parity'] = dict(loss_device=float(loss_c.item()), loss_oracle=float(ref['total_loss']),
                             loss_rel_err_vs_oracle=abs(float(loss_c.item()) - ref['total_loss']) / abs(ref['total_loss']),
                             utterances=nb, oracle='oracle.attention fp64 at the device path\'s rounding points',
                             sample='first %d utterances cut to %d frames / %d labels, dropout off' % (nb, tc, lc),
                             seconds=time.perf_counter() - t0)
        # the fp32 leg: the SAME parameters in a model with fp32 operands end to end against the PLAIN fp64 oracle (no
        # rounding points) -- north_star's statement (loss within 1e-4 relative in fp32) at this configuration's widths
        t0 = time.perf_counter()
        m32 = JointCTCAttention(input_size=D, encoder_type='blstm', encoder_num_units=H, encoder_num_layers=L,
                                encoder_num_proj=None, attention_type=att, attention_dim=A, decoder_type='lstm',
                                decoder_num_units=U, decoder_num_layers=1, embedding_dim=Em, lambda_weight=0.5,
                                num_classes=C, sos_index=C, eos_index=C + 1, max_decode_length=Lmax, parameter_init=0.1,
                                clip_grad_norm=5.0, clip_activation_encoder=50, clip_activation_decoder=50, dtype='f32',
                                seed=5, device=str(dev))
        m32.store.load_state_dict({k: torch.tensor(v) for k, v in sd.items()})
        ref32 = oatt.attention_model_forward(sd, xc, lab_c, slc, np.full(nb, lc + 2), L, att, clip_enc=50.0, clip_dec=50.0,
                                             ctc_labels=[[int(v) for v in r] for r in ctc_d], lambda_weight=0.5)
        loss32, *_ = m32.compute_loss(xc, lab_c, ctc_d, slc, np.full(nb, lc + 2), 1.0, 1.0, 1.0, is_training=False)
        out['parity_fp32'] = dict(loss_device=float(loss32.item()), loss_oracle=float(ref32['total_loss']),
                                  loss_rel_err_vs_oracle=abs(float(loss32.item()) - ref32['total_loss']) / abs(ref32['total_loss']),
                                  utterances=nb, oracle='oracle.attention fp64, no rounding points',
                                  sample='fp32-operand model with the same parameters on the same cut',
                                  seconds=time.perf_counter() - t0)
        del m32
    if not args.no_cpu_baseline:
        nb, tc, lc = 4, 64, 10
        sd = {k: v.cpu().numpy() for k, v in model.store.state_dict().items()}
        xc = xd[:nb, :tc].cpu().numpy()
        slc = np.minimum(seq_len[:nb], tc)
        lab_c = np.full((nb, lc + 2), C + 1, dtype=np.int64)
        lab_c[:, 0] = C
        lab_c[:, 1:1 + lc] = labels[:nb, 1:1 + lc]
        ctc_c = [[int(v) for v in lab_c[b, 1:1 + lc]] for b in range(nb)]
        th = min(16, os.cpu_count() or 1)
        out['cpu_baseline'] = cpu_baseline_oracle_call(
            lambda: oatt.attention_model_forward(sd, xc, lab_c, slc, np.full(nb, lc + 2), L, att, clip_enc=50.0,
                                                 clip_dec=50.0, ctc_labels=ctc_c, lambda_weight=0.5, dtype=torch.float32),
            int(slc.sum()), 'forward + backward (no update) of oracle.attention.attention_model_forward in fp32 on the first '
            '%d utterances cut to %d frames / %d labels (%d frames), %d threads' % (nb, tc, lc, int(slc.sum()), th), th)
    del model
    return out


# ------------------------------------------------------------------------------------------------ decode
def run_decode(args, dev):
    """CTC decode throughput (models/ctc/decoders/*.py, ctc.py:325-352): asr_ctc_greedy_decode and asr_ctc_beam_decode on
    softmax-peaked random logits, next to the oracle's restatement of the reference's numpy GreedyDecoder /
    BeamSearchDecoder (pure Python, one core; pinned bit-exact to the reference's own outputs by
    tests/golden/decoders_*.{npz,json}) on a bounded cut of the same posteriors."""
    from oracle import decoders as odec
    from tensorflow_end2end_speech_recognition_amd import ops
    out = {}
    rng = np.random.RandomState(5)
    # two posterior shapes per vocabulary: 'flat' = N(0, 9) logits (no class is ever negligible: the worst case for the
    # prefix search's class pruning and far flatter than a trained model emits) and 'peaked' = what a trained CTC model
    # emits (blank wins ~60 % of the frames by a wide margin, one label most of the others, N(0, 1) noise underneath)
    for name, T, B, C, W, tcut_cpu, bcut_cpu, shape in (('timit61_beam20', 778, 16, 62, 20, 60, 1, 'flat'),
                                                         ('timit61_beam20_peaked', 778, 16, 62, 20, 120, 1, 'peaked'),
                                                         ('kanji3387_beam100', 1000, 8, 3387, 100, 20, 1, 'flat'),
                                                         ('kanji3387_beam100_peaked', 1000, 8, 3387, 100, 20, 1, 'peaked')):
        if shape == 'flat':
            lg = rng.randn(T, B, C).astype(np.float32) * 3
        else:
            lg = rng.randn(T, B, C).astype(np.float32)
            win = np.where(rng.rand(T, B) < 0.6, C - 1, rng.randint(0, C - 1, size=(T, B)))
            np.put_along_axis(lg, win[:, :, None], 12.0 + rng.rand(T, B, 1).astype(np.float32), axis=2)
        logits = torch.tensor(lg, device=dev)
        sl = torch.full((B,), T, dtype=torch.int32, device=dev)
        ent = {}
        for kind in ('greedy', 'beam'):
            fn = (lambda: ops.ctc_greedy_decode(logits, sl)) if kind == 'greedy' else \
                 (lambda: ops.ctc_beam_decode(logits, sl, beam_width=W))
            fn()
            torch.cuda.synchronize()
            reps = 3 if kind == 'beam' else 20
            t0 = time.perf_counter()
            for _ in range(reps):
                r = fn()
            torch.cuda.synchronize()
            t = (time.perf_counter() - t0) / reps
            ent[kind] = dict(utterances_per_s=B / t, frames_per_s=B * T / t, ms_per_call=t * 1e3, batch=B, frames=T,
                             classes=C, posteriors=shape, **({'beam_width': W} if kind == 'beam' else {}))
            if kind == 'greedy':     # one pass over the logits: HBM roofline (wall time of the two launches incl. launch gaps)
                gbs = B * T * C * 4 / t / 1e9
                ent[kind]['roofline'] = dict(bound='hbm', achieved=gbs, peak=HBM_PEAK_GBS, unit='GB/s', frac=gbs / HBM_PEAK_GBS,
                                             algorithmic_bytes=B * T * C * 4, traffic=None)
            # CPU: the oracle decoder on log-softmax of the first tcut frames of the first utterance(s), one core
            lp = torch.log_softmax(logits[:tcut_cpu, :bcut_cpu].transpose(0, 1).double().cpu(), 2).numpy()
            slc = np.full(bcut_cpu, tcut_cpu)
            t0 = time.perf_counter()
            if kind == 'greedy':
                for _ in range(50):
                    ref = odec.greedy_decode(lp, slc, C - 1)
                tc = (time.perf_counter() - t0) / 50
            else:
                ref, _ = odec.beam_search_decode(lp, slc, C - 1, beam_width=W)
                tc = time.perf_counter() - t0
            ent[kind]['cpu_baseline'] = dict(value=bcut_cpu * tcut_cpu / tc, unit='frames/s', cores=1, kind='port',
                                             sample='oracle.decoders.%s on %d utterance(s) x %d frames, C=%d%s'
                                                    % ('greedy_decode' if kind == 'greedy' else 'beam_search_decode',
                                                       bcut_cpu, tcut_cpu, C, '' if kind == 'greedy' else ', width %d' % W))
            # the device result on that cut must be the oracle's (bit-exact labels)
            lg_cut = logits[:tcut_cpu, :bcut_cpu].contiguous()
            slcut = torch.full((bcut_cpu,), tcut_cpu, dtype=torch.int32, device=dev)
            if kind == 'greedy':
                lab, n = ops.ctc_greedy_decode(lg_cut, slcut)
            else:
                lab, n, _ = ops.ctc_beam_decode(lg_cut, slcut, beam_width=W)
            lab, n = lab.cpu().numpy(), n.cpu().numpy()
            ent[kind]['labels_identical_to_oracle_on_cpu_sample'] = bool(
                all(list(lab[b, :int(n[b])]) == list(ref[b]) for b in range(bcut_cpu)))
        out[name] = ent
    out['note'] = ('HIP decoders on whole batches resident in HBM (one wave per (frame, utterance) row for greedy, one '
                   'workgroup per utterance for the prefix beam search); cpu_baseline = oracle/decoders.py, the '
                   'restatement of the reference numpy decoders (models/ctc/decoders/*.py) that tests/golden pins '
                   'bit-exactly to the reference\'s own outputs (the reference itself is not on the GPU box), single '
                   'core, bounded cut; flat = N(0, 9) logits, peaked = trained-model-like posteriors')
    return out



# ------------------------------------------------------------------------------------------------ the result line
COMPACT_LIMIT = 6000      # bytes; the driver keeps the last 8 000 bytes of stdout (a 20.7 KB line was cut)
FULL_RESULT_PATHS = ('bench_full.json', os.path.join('gpurun_out', 'bench_full.json'))


def _sig(v, n=5):
    """Numbers to n significant digits, recursively (the line is a record, not a checkpoint)."""
    if isinstance(v, bool) or v is None or isinstance(v, (int, str)):
        return v
    if isinstance(v, float):
        return float('%.*g' % (n, v)) if np.isfinite(v) else None
    if isinstance(v, dict):
        return {k: _sig(x, n) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_sig(x, n) for x in v]
    return _sig(float(v), n) if isinstance(v, (np.floating, np.integer)) else v


def _numbers_only(d, keys=None):
    return {k: v for k, v in (d or {}).items() if not isinstance(v, str) and (keys is None or k in keys)}


def _compact_roofline(r, full=True):
    if not r:
        return None
    if not full:
        return dict(kernel=r.get('kernel'), frac=r.get('frac'), bound=r.get('bound'), achieved=r.get('achieved'),
                    unit=r.get('unit'))
    out = {k: r.get(k) for k in ('kernel', 'bound', 'achieved', 'peak', 'unit', 'frac', 'traffic')}
    src = r.get('traffic_source') or ''
    out['traffic_file'] = src.split(':')[0] if src else None          # a path, no prose
    for k in ('avg_launch_us', 'us_per_recurrence_step', 'algorithmic_bytes_per_launch', 'mfma_frac'):
        if k in r:
            out[k] = r[k]
    return out


def _compact_cpu(c, full=True):
    if not c:
        return None
    out = dict(value=c.get('value'), cores=c.get('cores'))
    if full:
        out.update(unit=c.get('unit'), kind=c.get('kind'), host_cores=c.get('host_cores'),
                   seconds_per_step=c.get('seconds_per_step'), sample=(c.get('sample') or '')[:160])
    return out


def _compact_aux(e):
    """Per auxiliary configuration only the handful of numbers VERDICT r03 item 1 lists."""
    if not isinstance(e, dict) or 'value' not in e:
        return e if not isinstance(e, dict) else {k: (v[:120] if isinstance(v, str) else v) for k, v in e.items()}
    sm = e.get('step_ms') or {}
    out = dict(value=e['value'], ms_per_step=e.get('ms_per_step'), dtype=e.get('dtype'),
               roofline=_compact_roofline(e.get('roofline'), full=False),
               cpu_baseline=_compact_cpu(e.get('cpu_baseline'), full=False),
               host_issue_mean=sm.get('host_issue_mean'), host_wait_for_device_mean=sm.get('host_wait_for_device_mean'))
    for k in ('mfma_frac_whole_step', 'decoder_steps', 'cluster_handoff_flags'):
        if k in e:
            out[k] = e[k]
    if isinstance(e.get('roofline_groups'), dict):       # [fraction of the bound's peak, ms of event time per step] per group
        out['groups'] = {n: [g.get('frac'), g.get('ms_per_step')] for n, g in e['roofline_groups'].items() if g}
    if isinstance(e.get('greedy_infer'), dict):
        out['greedy_infer_tokens_per_s'] = e['greedy_infer'].get('tokens_per_s')
    if isinstance(e.get('parity'), dict):
        out['parity'] = _numbers_only(e['parity'], ('loss_rel_err_vs_oracle', 'per_utterance_loss_rel_err_max',
                                                    'greedy_label_mismatch', 'greedy_labels_compared'))
    if isinstance(e.get('parity_fp32'), dict):
        out['parity_fp32_loss_rel'] = e['parity_fp32'].get('loss_rel_err_vs_oracle')
    ks = e.get('kernels') or {}
    out['kernel_us'] = {k: v.get('avg_us') for k, v in ks.items()}
    return out


def _compact_decode(d):
    out = {}
    for name, ent in (d or {}).items():
        if not isinstance(ent, dict):
            continue
        if 'error' in ent or 'skipped' in ent:
            out[name] = {k: (v[:120] if isinstance(v, str) else v) for k, v in ent.items()}
            continue
        o = {}
        for kind, r in ent.items():
            if not isinstance(r, dict):
                continue
            c = r.get('cpu_baseline') or {}
            o[kind] = dict(utt_per_s=r.get('utterances_per_s') if 'utterances_per_s' in r else r.get('tokens_per_s'),
                           ms_per_call=r.get('ms_per_call'), cpu_frames_per_s=c.get('value'), cpu_kind=c.get('kind'),
                           gpu_frames_per_s=r.get('frames_per_s'),
                           identical=r.get('labels_identical_to_oracle_on_cpu_sample'))
            if r.get('roofline'):
                o[kind]['hbm_frac'] = r['roofline'].get('frac')
        out[name] = o
    return out


def compact_line(out, limit=COMPACT_LIMIT):
    """The ONE line the driver parses: every contract key, numbers only, a file path where the full object has prose.
    Sheds optional detail in a fixed order until it fits `limit` bytes (tests/test_host_logic.py pins that it does)."""
    top = ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
           'vs_baseline', 'dtype', 'data')
    c = {k: out.get(k) for k in top}
    cfg = dict(out.get('config') or {})
    c['config'] = cfg
    c['step_ms'] = _numbers_only(out.get('step_ms'))
    h = out.get('h2d_inclusive') or {}
    c['h2d_inclusive'] = _numbers_only(h, ('value', 'ms_per_step', 'median_ms'))
    c['final_loss'] = out.get('final_loss')
    c['cluster_handoff_flags'] = out.get('cluster_handoff_flags')
    p = out.get('parity')
    c['parity'] = dict(_numbers_only(p), oracle=p.get('oracle')) if isinstance(p, dict) else p
    c['kernels'] = {k: dict(calls=v.get('calls'), avg_us=v.get('avg_us')) for k, v in (out.get('kernels') or {}).items()}
    c['roofline'] = _compact_roofline(out.get('roofline'))
    c['cpu_baseline'] = _compact_cpu(out.get('cpu_baseline'))
    for k in ('headline_f32', 'cfgA', 'cfgC', 'cfgD', 'cfgE', 'input_width_D39'):
        if out.get(k) is not None:
            c[k] = _compact_aux(out[k])
    if out.get('decode') is not None:
        c['decode'] = _compact_decode(out['decode']) if 'error' not in out['decode'] and 'skipped' not in out['decode'] \
            else _compact_aux(out['decode'])
    for key in ('bgru', 'blstmp'):
        if isinstance(out.get(key), dict):
            g = out[key]
            c[key] = {k: g.get(k) for k in ('value', 'ms_per_step', 'cluster_handoff_flags')} if 'value' in g else _compact_aux(g)
    bs = out.get('batch_scaling')
    if isinstance(bs, dict):
        c['batch_scaling'] = [[r.get('batch'), r.get('value'), r.get('ms_per_step')] for r in bs.get('rows', [])] \
            if 'rows' in bs else _compact_aux(bs)
    if out.get('per_rank') is not None:
        pr = out['per_rank']
        c['per_rank'] = dict(step_median_ms=pr.get('step_median_ms'), elapsed_s=pr.get('elapsed_s'), frames=pr.get('frames'),
                             comm_ms=pr.get('comm_stream_allreduce_ms_per_step'))
        cm = out.get('comm') or {}
        c['comm'] = _numbers_only(cm, ('allreduce_calls_per_step', 'allreduce_ms_per_step', 'bytes_per_step', 'bucket_min_mb',
                                       'ranks', 'rccl_ranks'))
        c['comm']['backend'] = cm.get('backend')
        op = out.get('other_padding')
        if op:
            c['other_padding'] = dict(padded_to=op.get('padded_to'), value=op.get('value'), ms_per_step=op.get('ms_per_step'),
                                      per_rank_step_median_ms=op.get('per_rank_step_median_ms'))
    c['full'] = out.get('full')
    c = _sig(c)
    line = json.dumps(c, separators=(',', ':'))
    # shed optional detail, least important first, until the line fits
    for drop in (('batch_scaling',), ('input_width_D39',), ('headline_f32', 'kernel_us'), ('headline_f32', 'cpu_baseline'),
                 ('cfgA', 'kernel_us'), ('cfgE', 'kernel_us'), ('cfgC', 'kernel_us'), ('cfgD', 'kernel_us'), ('blstmp',), ('bgru',),
                 ('decode',), ('per_rank',), ('h2d_inclusive',), ('other_padding',),
                 ('cfgC', 'groups'), ('headline_f32',), ('cfgE',), ('cfgD',), ('cfgC',), ('cfgA',), ('comm',)):
        if len(line) <= limit:
            break
        if len(drop) == 1:
            if drop[0] in c:
                c[drop[0]] = 'see full'
        elif isinstance(c.get(drop[0]), dict):
            c[drop[0]].pop(drop[1], None)
        line = json.dumps(c, separators=(',', ':'))
    return line


def write_full(out):
    """The complete object (prose notes, thread sweeps, per-kernel tables) goes to bench_full.json at the repo root and,
    when that scratch directory exists, to gpurun_out/ so it comes back from a GPU box."""
    written = []
    for rel in FULL_RESULT_PATHS:
        path = os.path.join(ROOT, rel)
        if os.path.isdir(os.path.dirname(path)):
            try:
                with open(path, 'w') as f:
                    json.dump(out, f, indent=1)
                written.append(rel)
            except OSError:
                pass
    return written[0] if written else None


# ------------------------------------------------------------------------------------------------ launching N ranks
def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(('127.0.0.1', 0))
        return sk.getsockname()[1]


def self_launch(n, argv):
    """`python bench.py --gpus N ...` outside a launcher: run `python -m torch.distributed.run --nnodes=1
    --nproc-per-node N --master-addr 127.0.0.1 --master-port <free> bench.py <the same arguments>` (the driver's own
    command for N > 1), pass the ranks' stderr through, and print the LAST stdout line that parses as a JSON object --
    rank 0's result -- as this process's single stdout line.  Returns the job's exit status (1 if no line came)."""
    import subprocess
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    env.setdefault('OMP_NUM_THREADS', str(max(1, (os.cpu_count() or 1) // n)))
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n),
           '--master-addr', '127.0.0.1', '--master-port', str(_free_port()), os.path.abspath(__file__)] + list(argv)
    log('self-launch: ' + ' '.join(cmd))
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, env=env)
    out = p.communicate()[0].decode('utf-8', 'replace')
    line = None
    for ln in out.splitlines():
        ln = ln.strip()
        if ln.startswith('{') and ln.endswith('}'):
            try:
                json.loads(ln)
                line = ln
            except ValueError:
                pass
    if line is not None:
        sys.stdout.write(line + '\n')
        sys.stdout.flush()
    else:
        sys.stderr.write('bench.py: the %d-rank job printed no result line (exit status %d)\n' % (n, p.returncode))
    return p.returncode if (p.returncode or line is not None) else 1


def dry_run_launch(args, world, rank, result_fd):
    """The launch path without a GPU: process group on gloo, one all-gather of a per-rank record, the contract's line
    from rank 0 with value null and dry_run true.  Nothing is measured and nothing is claimed."""
    import torch.distributed as dist
    if world > 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group('gloo', rank=rank, world_size=world)
        mine = torch.tensor([float(rank), float(os.getpid())], dtype=torch.float64)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        ranks = sorted(int(t[0].item()) for t in allr)
        dist.barrier()
    else:
        ranks = [0]
    if rank == 0:
        assert ranks == list(range(world)), ranks
        out = dict(metric='acoustic frames/sec (train), TIMIT-shaped BLSTM-CTC', value=None, unit='frames/s', n_gpus=world,
                   steps=args.steps, warmup=args.warmup, ms_per_step=None, higher_is_better=True, scaling='weak',
                   vs_baseline=None, dtype=args.dtype, data='synthetic', dry_run=True, ranks_seen=ranks,
                   config=dict(workload='launch check only: no kernels ran', global_batch=args.batch * world,
                               parallelism='dp%d' % world))
        os.write(result_fd, (json.dumps(out, separators=(',', ':')) + '\n').encode())
    if world > 1:
        dist.destroy_process_group()
    os.close(result_fd)
    return 0


# ------------------------------------------------------------------------------------------------ main
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--dtype', default='bf16')
    ap.add_argument('--units', type=int, default=256)
    ap.add_argument('--layers', type=int, default=5)
    ap.add_argument('--batch', type=int, default=16, help='utterances per GPU')
    ap.add_argument('--classes', type=int, default=61)
    ap.add_argument('--input-size', type=int, default=120)
    ap.add_argument('--tmin', type=int, default=100)
    ap.add_argument('--tmax', type=int, default=778)
    ap.add_argument('--keep-prob', type=float, default=0.8)
    ap.add_argument('--no-global-tmax', action='store_true',
                    help='N > 1: every rank pads to its own longest utterance instead of the global one')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-parity', action='store_true')
    ap.add_argument('--no-cfgA', action='store_true')
    ap.add_argument('--no-aux', action='store_true', help='skip cfgC / cfgD / cfgE / decode / input width / batch scaling')
    ap.add_argument('--aux', default='f32,cfgC,cfgD,cfgE,decode,gru,lstmp,D39,batch', help='which auxiliary entries to run (N = 1)')
    ap.add_argument('--aux-steps', type=int, default=5)
    ap.add_argument('--aux-warmup', type=int, default=2)
    ap.add_argument('--cpu-steps', type=int, default=2)
    ap.add_argument('--cpu-threads', default='8,16,32', help='thread counts of the CPU baseline sweep (capped at 64)')
    ap.add_argument('--time-budget', type=float, default=420.0,
                    help='seconds after which the remaining auxiliary entries are skipped (recorded as such)')
    ap.add_argument('--dry-run-launch', action='store_true',
                    help='rendezvous + one gloo all-gather per rank and a line marked dry_run, NO kernels: checks the '
                         'launch path of --gpus N on a box without GPUs (tests/test_distributed_cpu.py)')
    ap.add_argument('--own-tmax-steps', type=int, default=10,
                    help='N > 1: timed steps of the second leg with every rank padded to its OWN longest utterance '
                         '(0 = skip); the headline pads to the global Tmax as the reference does')
    ap.add_argument('--cpu-tmax', type=int, default=256,
                    help='CPU legs (baseline, oracle parity): the same batch truncated to its first N frames')
    ap.add_argument('--full', action='store_true',
                    help='also the legs beyond the headline (h2d-inclusive timing, oracle parity, CPU baseline, cfgA, '
                         'the auxiliary entries, at N > 1 the other padding rule) and the complete result object in '
                         'bench_full.json; a plain run only times the headline')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='write what the last timed step computed (loss, per-utterance losses, logits, updated '
                         'parameters) as DIR/<name>.npy, float32, <= 64 MB in all')
    args = ap.parse_args()

    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    if args.gpus > 1 and 'RANK' not in os.environ and 'WORLD_SIZE' not in os.environ:
        # `python bench.py --gpus N` without a launcher: start the N ranks ourselves (one process per GPU under
        # torch.distributed.run, rendezvous on 127.0.0.1) and hand on rank 0's line and the job's exit status
        sys.exit(self_launch(args.gpus, sys.argv[1:]))
    if world != args.gpus:
        sys.exit('bench.py --gpus %d inside a job of WORLD_SIZE %d: the two must agree' % (args.gpus, world))

    # stdout carries exactly ONE line, the JSON result: libraries that print banners to file descriptor 1 (RCCL's
    # version block, gloo's rank messages) are sent to stderr for the duration of the run
    sys.stdout.flush()
    result_fd = os.dup(1)
    os.dup2(2, 1)
    if not args.dry_run_launch and os.environ.get('ASR_BENCH_BACKEND') == 'gloo' and not torch.cuda.is_available():
        log('no GPU visible and ASR_BENCH_BACKEND=gloo: launch check only (the line says dry_run, value null)')
        args.dry_run_launch = True
    if args.dry_run_launch:
        return dry_run_launch(args, world, rank, result_fd)
    # dry-run knobs for a box with fewer GPUs than ranks (scripts/r02_dp_dryrun.sh): ASR_BENCH_DEVICE pins every rank to
    # one device, ASR_BENCH_BACKEND=gloo replaces RCCL (which refuses two ranks on one GPU).  Never set by the driver.
    dev_index = int(os.environ.get('ASR_BENCH_DEVICE', local_rank))
    backend = os.environ.get('ASR_BENCH_BACKEND', 'nccl')
    torch.cuda.set_device(dev_index)
    dev = torch.device('cuda', dev_index)
    import torch.distributed as dist
    from tensorflow_end2end_speech_recognition_amd.utils.training import multi_gpu
    if world > 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        if backend == 'nccl':
            dist.init_process_group('nccl', rank=rank, world_size=world, device_id=dev)
            multi_gpu.warm_up_collectives(dev)      # RCCL rings + the C ABI's communicator: before step 1, not inside it
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    wl = dict(units=args.units, layers=args.layers, classes=args.classes, dtype=args.dtype, batch=args.batch,
              input_size=args.input_size, tmin=args.tmin, tmax=args.tmax, keep_prob=args.keep_prob, seed=1,
              global_tmax=not args.no_global_tmax)
    res = run_blstm_ctc(args, wl, dev, world, rank, dev_index, args.steps, args.warmup,
                        want_parity=args.full and not args.no_parity, want_h2d=args.full,
                        want_cpu=(args.full and world == 1 and not args.no_cpu_baseline),
                        dump_dir=args.dump_outputs if rank == 0 else None)
    # aggregate: slowest rank's time, all ranks' frames; per-rank medians so a straggler is visible
    stats = torch.tensor([res['elapsed'], res.get('elapsed_h2d', 0.0), float(res['frames']), res['step_ms']['median'],
                          float(res['T']), res.get('comm', {}).get('allreduce_ms_per_step', 0.0)],
                         device=dev, dtype=torch.float64)
    if world > 1:
        allst = [torch.zeros_like(stats) for _ in range(world)]
        dist.all_gather(allst, stats)
        allst = torch.stack(allst).cpu().numpy()
    else:
        allst = stats.cpu().numpy()[None]
    elapsed, elapsed_h2d, total_frames = float(allst[:, 0].max()), float(allst[:, 1].max()), float(allst[:, 2].sum())
    value = total_frames * args.steps / elapsed
    other_padding = None
    if args.full and world > 1 and args.own_tmax_steps > 0:
        # the same shards under the OTHER padding rule (default leg: the reference's global Tmax; this leg: every rank
        # padded to its own longest utterance -- ranks then finish their recurrences at different times and the slowest
        # one sets the step), a short run, reported beside the headline
        wo = dict(wl, global_tmax=not wl['global_tmax'])
        ro = run_blstm_ctc(args, wo, dev, world, rank, dev_index, args.own_tmax_steps, min(args.warmup, 3),
                           want_parity=False, want_h2d=False, want_cpu=False)
        so = torch.tensor([ro['elapsed'], float(ro['frames']), ro['step_ms']['median'], float(ro['T'])], device=dev,
                          dtype=torch.float64)
        allo = [torch.zeros_like(so) for _ in range(world)]
        dist.all_gather(allo, so)
        allo = torch.stack(allo).cpu().numpy()
        other_padding = dict(padded_to='global Tmax %d on every rank' % int(allo[:, 3].max()) if wo['global_tmax']
                             else 'own Tmax per rank', steps=args.own_tmax_steps,
                             value=float(allo[:, 1].sum()) * args.own_tmax_steps / float(allo[:, 0].max()),
                             ms_per_step=float(allo[:, 0].max()) / args.own_tmax_steps * 1e3,
                             per_rank_step_median_ms=[float(v) for v in allo[:, 2]], per_rank_T=[int(v) for v in allo[:, 3]])
        del ro

    if rank == 0:
        ks = res['kernels']
        H, L, C = wl['units'], wl['layers'], wl['classes'] + 1
        tt = load_traffic_table()
        key = '%dx%d_%s_B%d_T%d' % (L, H, wl['dtype'], wl['batch'], wl['tmax'])
        dom = max(('lstm_fwd', 'lstm_bwd'), key=lambda n: ks.get(n, {}).get('total_ms', 0))
        traffic = src = None
        if tt and key in tt.get('workloads', {}):
            traffic, src = tt['workloads'][key].get(dom), tt.get('source')
        out = dict(metric='acoustic frames/sec (train), TIMIT-shaped BLSTM-CTC', value=value, unit='frames/s',
                   n_gpus=world, steps=args.steps, warmup=args.warmup,
                   ms_per_step=elapsed / args.steps * 1e3, higher_is_better=True, scaling='weak',
                   vs_baseline=None, dtype=args.dtype, data='synthetic',
                   config=dict(workload='TIMIT 61-phone %dx%d BLSTM-CTC, B=%d/GPU, D=%d, C=%d, '
                                        'seq_len~U{%d..%d}, dropout %.1f, rmsprop, train step'
                                        % (L, H, args.batch, args.input_size, C, args.tmin, args.tmax,
                                           1 - args.keep_prob),
                               global_batch=args.batch * world, frames_per_step=total_frames,
                               parallelism='dp%d' % world,
                               padded_to=('global Tmax %d on every rank' % int(allst[:, 4].max())) if (world > 1 and wl['global_tmax'])
                               else 'own Tmax per rank'),
                   step_ms=res['step_ms'],
                   h2d_inclusive=dict(value=total_frames * args.steps / elapsed_h2d, unit='frames/s',
                                      ms_per_step=elapsed_h2d / args.steps * 1e3, median_ms=res['h2d_median_ms'],
                                      note='batch uploaded from pinned host memory every step, double-buffered on a '
                                           'copy stream (SURVEY 8d step definition); reported next to `value`, which '
                                           'has the inputs resident as the bench contract asks') if args.full else None,
                   final_loss=res['final_loss'], cluster_handoff_flags=res['handoff_flags'],
                   parity=res.get('parity'), kernels=ks,
                   roofline=recurrence_roofline(H, res['frames'] * 2, res['T'], wl['dtype'], ks, traffic, src,
                                                tiles=(wl['batch'] + 15) // 16),
                   cpu_baseline=res.get('cpu_baseline'), cfgA=None)
        if world > 1:
            out['per_rank'] = dict(step_median_ms=[float(v) for v in allst[:, 3]], frames=[float(v) for v in allst[:, 2]],
                                   elapsed_s=[float(v) for v in allst[:, 0]],
                                   comm_stream_allreduce_ms_per_step=[float(v) for v in allst[:, 5]])
            out['comm'] = res.get('comm')
            if out['comm'] is not None:
                native = multi_gpu.native_comm(dev) is not None
                out['comm'].update(ranks=dist.get_world_size(), backend=dist.get_backend(),
                                   collective='asr_allreduce_mean: RCCL through the C ABI' if native else
                                   'torch.distributed all_reduce (%s)' % dist.get_backend(), rccl_ranks=world if native else 0)
            out['other_padding'] = other_padding
        del res
        torch.cuda.empty_cache()
        log('headline done: %.0f frames/s' % value)
        if args.full and world == 1 and not args.no_cfgA:
            # BASELINE configs[0]: TIMIT-39, 2x128 BLSTM-CTC, fp32 (exact fp32 MFMA path), B=16, dropout 0.5
            wa = dict(units=128, layers=2, classes=39, dtype='f32', batch=16, input_size=120, tmin=100, tmax=778,
                      keep_prob=0.5, seed=0)
            ra = run_blstm_ctc(args, wa, dev, 1, 0, dev_index, args.steps, args.warmup, want_parity=not args.no_parity,
                               want_h2d=False, want_cpu=not args.no_cpu_baseline)
            out['cfgA'] = blstm_ctc_entry(args, wa, ra, args.steps,
                                          'TIMIT 39-phone 2x128 BLSTM-CTC fp32, B=16, D=120, C=40, seq_len~U{100..778}, '
                                          'dropout 0.5, rmsprop, train step')
            del ra
        aux = set() if (not args.full or world > 1 or args.no_aux) else set(a for a in args.aux.split(',') if a)
        def over_budget(name):
            if time.perf_counter() - _T0 > args.time_budget:
                out[name] = dict(skipped='time budget of %.0f s used up' % args.time_budget)
                log('%s skipped: time budget' % name)
                return True
            return False
        if 'f32' in aux and wl['dtype'] != 'f32' and not over_budget('headline_f32'):
            # the headline workload itself in fp32 operands (the three-term recurrence kernels at H = 256): the north_star's
            # parity statement -- loss <= 1e-4 of the oracle, label indices identical -- is an fp32 statement, the headline
            # `value` is bf16; this is what the same shard costs at the precision the statement is made at
            log('headline workload in fp32 ...')
            wf = dict(wl, dtype='f32')
            try:
                rf = run_blstm_ctc(args, wf, dev, 1, 0, dev_index, 20, 5, want_parity=not args.no_parity, want_h2d=False,
                                   want_cpu=False)
                out['headline_f32'] = blstm_ctc_entry(args, wf, rf, 20, 'the headline shard (5x%d BLSTM-CTC, B=%d) with fp32 '
                                                      'operands' % (wl['units'], wl['batch']))
                del rf
            except Exception as e:
                out['headline_f32'] = dict(error=repr(e)[:400])
            torch.cuda.empty_cache()
        for name, fn in (('cfgC', lambda: run_cfgC(args, dev, dev_index)),
                         ('cfgD', lambda: run_attention_cfg(args, dev, dev_index, 'D')),
                         ('cfgE', lambda: run_attention_cfg(args, dev, dev_index, 'E')),
                         ('decode', lambda: run_decode(args, dev))):
            if name in aux and not over_budget(name):
                log('%s ...' % name)
                try:
                    out[name] = fn()
                except Exception as e:      # an auxiliary entry must not cost the headline line
                    out[name] = dict(error=repr(e)[:400])
                torch.cuda.empty_cache()
        if 'D39' in aux and not over_budget('input_width_D39'):
            log('D39 ...')
            # SURVEY 8d names a "D = 40" variant; the class surface rejects it as the reference does (input_size % 3,
            # models/ctc/ctc.py:79: features come as static + delta + delta-delta): 39 = 13 x 3 is the nearest valid width
            wd = dict(wl, input_size=39)
            rd = run_blstm_ctc(args, wd, dev, 1, 0, dev_index, 20, 5, want_parity=False, want_h2d=False, want_cpu=False)
            out['input_width_D39'] = blstm_ctc_entry(args, wd, rd, 20, 'headline model on D=39 (13x3) features: input_size '
                                                     '40 is rejected by the class surface as by the reference (ctc.py:79)')
            del rd
        if 'gru' in aux and not over_budget('bgru'):
            # the reference's other recurrent encoder family (models/encoders/core/gru.py) on the headline shard: bgru 2 x 256
            # CTC, fp32 (the GRU kernels are fp32), the same batch -- on the GRU clusters of round 6
            log('bgru ...')
            try:
                from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
                xb, slb, _, denseb = make_batch(wl['seed'], wl['batch'], wl['input_size'], wl['classes'] + 1, wl['tmin'], wl['tmax'])
                xg_, sg_ = torch.tensor(xb, device=dev), torch.tensor(slb, device=dev)
                mg = CTC('bgru', wl['input_size'], 256, 2, wl['classes'], clip_grad_norm=5.0, seed=0, device=str(dev))
                for _ in range(3):
                    lg_, _ = mg.compute_loss(xg_, denseb, sg_, keep_prob=wl['keep_prob'])
                    mg.train(lg_, 'rmsprop', 1e-3)
                torch.cuda.synchronize()
                tg0 = time.perf_counter()
                for _ in range(10):
                    lg_, _ = mg.compute_loss(xg_, denseb, sg_, keep_prob=wl['keep_prob'])
                    mg.train(lg_, 'rmsprop', 1e-3)
                torch.cuda.synchronize()
                tg = (time.perf_counter() - tg0) / 10
                out['bgru'] = dict(workload='bgru 2x256 CTC fp32 on the headline batch (B=%d, T<=%d), train step' % (wl['batch'], wl['tmax']),
                                   value=float(slb.sum()) / tg, unit='frames/s', ms_per_step=tg * 1e3, dtype='f32', steps=10,
                                   final_loss=float(lg_.item()), cluster_handoff_flags=ops_flags(dev_index))
                del mg, xg_, sg_
            except Exception as e:
                out['bgru'] = dict(error=repr(e)[:400])
            torch.cuda.empty_cache()
        if 'lstmp' in aux and not over_budget('blstmp'):
            # lstm_impl='LSTMCell' with num_proj (the reference's projected cells, blstm.py:187-230) on the headline shard:
            # blstm 5 x 256, projection 128, fp32 -- the whole-sequence recurrence kernels on W_p W_h (round 6)
            log('blstmp ...')
            try:
                from tensorflow_end2end_speech_recognition_amd.models.ctc.ctc import CTC
                xb, slb, _, denseb = make_batch(wl['seed'], wl['batch'], wl['input_size'], wl['classes'] + 1, wl['tmin'], wl['tmax'])
                xp_, sp_ = torch.tensor(xb, device=dev), torch.tensor(slb, device=dev)
                mp_ = CTC('blstm', wl['input_size'], 256, 5, wl['classes'], lstm_impl='LSTMCell', num_proj=128, clip_grad_norm=5.0,
                          clip_activation=50.0, seed=0, dtype=wl['dtype'], device=str(dev))
                for _ in range(3):
                    lp_, _ = mp_.compute_loss(xp_, denseb, sp_, keep_prob=wl['keep_prob'])
                    mp_.train(lp_, 'rmsprop', 1e-3)
                torch.cuda.synchronize()
                tp0 = time.perf_counter()
                for _ in range(10):
                    lp_, _ = mp_.compute_loss(xp_, denseb, sp_, keep_prob=wl['keep_prob'])
                    mp_.train(lp_, 'rmsprop', 1e-3)
                torch.cuda.synchronize()
                tp = (time.perf_counter() - tp0) / 10
                out['blstmp'] = dict(workload='blstm 5x256 LSTMCell num_proj 128 CTC (%s operands) on the headline batch (B=%d, T<=%d), train step'
                                     % (wl['dtype'], wl['batch'], wl['tmax']), value=float(slb.sum()) / tp, unit='frames/s', ms_per_step=tp * 1e3,
                                     dtype=wl['dtype'], steps=10, final_loss=float(lp_.item()), cluster_handoff_flags=ops_flags(dev_index))
                del mp_, xp_, sp_
            except Exception as e:
                out['blstmp'] = dict(error=repr(e)[:400])
            torch.cuda.empty_cache()
        if 'batch' in aux and not over_budget('batch_scaling'):
            log('batch scaling ...')
            # what the design delivers per GPU at the recipes' own batch sizes: one 16-utterance tile per cluster,
            # so B = 32 .. 128 puts 2 .. 8 clusters per direction side by side (16 .. 64 of the 256 CUs)
            rows = []
            for Bn in (32, 64, 128):
                wb = dict(wl, batch=Bn)
                rb = run_blstm_ctc(args, wb, dev, 1, 0, dev_index, 10, 3, want_parity=False, want_h2d=False, want_cpu=False)
                rows.append(dict(batch=Bn, value=rb['frames'] * 10 / rb['elapsed'], unit='frames/s',
                                 ms_per_step=rb['elapsed'] / 10 * 1e3, lstm_fwd_us=rb['kernels'].get('lstm_fwd', {}).get('avg_us'),
                                 lstm_bwd_us=rb['kernels'].get('lstm_bwd', {}).get('avg_us'),
                                 cluster_handoff_flags=rb['handoff_flags']))
                del rb
                torch.cuda.empty_cache()
            out['batch_scaling'] = dict(workload='headline model (5x256 bf16, D=120, C=62, T<=778) at larger per-GPU batches', rows=rows)
        sys.stdout.flush()
        out['full'] = write_full(out) if args.full else None
        os.write(result_fd, (compact_line(out) + '\n').encode())
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    os.close(result_fd)


if __name__ == '__main__':
    main()
