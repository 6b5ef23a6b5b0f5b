"""The launch-counter table: one row per native counter family of include/asr_hip.h, one row per public view of ops.

Data only (no torch, no ctypes).  _lib binds asr_<family> / asr_reset_<family> from FAMILIES; ops builds its *_counts /
reset_*_counts functions from VIEWS; tests/test_counters_host.py holds the key counts to the header's enums and
parameter names.  A family is an array of unsigned long long on the handle; its keys name the words in native order
(for a sized family, the order of its enum in asr_hip.h), so a key goes where its enumerator goes.
"""
import collections

# getter / reset: the exported names; sized: the getter is (h, out, n) and zero-fills past its words, else (h, out<N>)
Family = collections.namedtuple('Family', 'getter reset sized keys')
# name: the ops function; keys = FAMILIES[family].keys[offset:offset + len(keys)]; reset: the ops function that zeroes the
# family, or None for a view that shares another view's reset
View = collections.namedtuple('View', 'name family offset keys reset doc')

_GEMM_PATH_KEYS = ('rows_128', 'rows_256', 'rows_full')
_TN_PATH_KEYS = ('tn_frames', 'tn_frames_generic')
_HEAD_BWD_KEYS = ('head_bwd_lean', 'head_bwd_full')
# the kernel a full product ended in, and the second passes of gemm(mul=...) / gemm(drop=...)
_GEMM_KERNEL_KEYS = ('skinny_nn16', 'skinny_nn32', 'skinny_nt16', 'skinny_nt32', 'nt128', 'nt256', 'tn_lean', 'generic128',
                     'generic64', 'generic64_splitk', 'mul_pass', 'drop_pass')

# family -> (sized, keys); the family's name is its export without the asr_ prefix
_FAMILY_ROWS = (
    ('recurrence_path_counts', False,
     ('lstm_cluster', 'lstm_single_cu', 'lstm_split_calls', 'gru_cluster', 'gru_single_cu', 'gru_split_calls')),
    ('gru_kernel_counts', False,
     ('fwd_cluster', 'fwd_persistent', 'fwd_per_step', 'bwd_cluster', 'bwd_persistent', 'bwd_per_step')),
    # the ASR_LSTM_* enum
    ('lstm_kernel_counts', True,
     ('fwd_bf16_cu16', 'fwd_bf16_hs32', 'fwd_bf16_hs64', 'fwd_f32_split', 'fwd_f32_hs32', 'fwd_f32_hs64',
      'fwd_single_bf16', 'fwd_single_f32',
      'bwd_bf16_hs32', 'bwd_bf16_hs64', 'bwd_f32_split', 'bwd_f32_hs32', 'bwd_f32_hs64',
      'bwd_single_bf16', 'bwd_single_f32')),
    # the ASR_ATT_* enum
    ('att_path_counts', True,
     ('fwd_step_fused', 'fwd_step_4launch', 'fwd_cell_bf16', 'fwd_cell_f32img', 'fwd_cell_gemm',
      'bwd_step_fused_q', 'bwd_step_unfused', 'bwd_cell_bf16', 'bwd_cell_gemm', 'bwd_softmax_folded',
      'bwd_softmax_separate',
      'energy_fwd_16', 'energy_fwd_32', 'energy_fwd_64', 'energy_fwd_64x2', 'energy_fwd_general',
      'energy_bwd_16', 'energy_bwd_32', 'energy_bwd_64', 'energy_bwd_64x2', 'energy_bwd_general',
      'loc_fwd_16', 'loc_fwd_32', 'loc_fwd_64', 'loc_fwd_general',
      'loc_bwd_16', 'loc_bwd_32', 'loc_bwd_64', 'loc_bwd_general',
      'fused_fwd_16', 'fused_fwd_32', 'fused_fwd_64', 'fused_fwd_64x2')),
    # the ASR_CONVP_* enum
    ('conv_path_counts', True,
     ('img', 'tiled', 'pair_64_64', 'pair_64_128', 'pair_128_128', 'pair_128_64', 'pair_other',
      'maxv_2', 'maxv_4', 'maxv_8', 'maxv_14', 'maxv_16', 'act_0', 'act_1', 'act_2', 'act_3', 'act_4',
      'nbuf_1', 'nbuf_2', 'stream', 'w8', 'tiled_bn128', 'tiled_bn64',
      'wgrad_img_64_small', 'wgrad_img_64_large', 'wgrad_img_128', 'split', 'bias_in_kernel',
      'reduce_vec', 'reduce_scalar', 'wgrad_tr_128', 'wgrad_tr_64', 'wgrad_colpix')),
    # the ASR_GEMMP_* enum: four public views, one behind the other
    ('gemm_path_counts', True, _GEMM_PATH_KEYS + _TN_PATH_KEYS + _HEAD_BWD_KEYS + _GEMM_KERNEL_KEYS),
    ('ctc_head_counts', False, ('head_fwd', 'loss_ex', 'loss')),
    ('ctc_ls_counts', False, ('calls', 'lse_done', 'no_grad')),
    ('att_beam_counts', False, ('select', 'reorder', 'backtrace')),
    ('att_joint_counts', False, ('score', 'advance', 'joint_select')),
    ('att_gru_counts', False, ('fwd_fused', 'fwd_general', 'bwd')),
    ('att_stack_counts', False, ('fwd_image', 'fwd_two_launch', 'bwd_fused', 'bwd_generic')),
    ('att_lm_counts', False, ('lm_step', 'fused_select', 'lm_reorder')),
    ('ctc_beam_lm_counts', False, ('frames', 'lm_steps', 'commits')),
    ('weight_noise_counts', False, ('calls', 'elements', 'vec_calls')),
    ('input_augment_counts', False, ('calls', 'elements', 'vec_calls')),
)

FAMILIES = collections.OrderedDict(
    (name, Family('asr_' + name, 'asr_reset_' + name, sized, keys)) for name, sized, keys in _FAMILY_ROWS)

# (public name, family, the view's keys or None for the whole family, reset name or None, docstring); the views of a
# family follow one another in native order
_VIEW_ROWS = (
    ('recurrence_path_counts', 'recurrence_path_counts', None, 'reset_recurrence_path_counts',
     """Which path the recurrence calls on `device` took since the last reset, summed over its handles: cluster launches
    (one per tile group), single-CU calls, and calls that were split into more than one tile group, for LSTM and GRU.
    Host counters: no device work, no synchronisation."""),
    ('gru_kernel_counts', 'gru_kernel_counts', None, 'reset_gru_kernel_counts',
     """The form each gru_fwd / gru_bwd call on `device` ended in since the last reset_gru_kernel_counts, summed over its
    handles (asr_gru_kernel_counts): clusters, the persistent single-CU kernel, or the launch-per-step kernels.  Host
    counters: no device work, no synchronisation."""),
    ('lstm_kernel_counts', 'lstm_kernel_counts', None, 'reset_lstm_kernel_counts',
     """The form each lstm_fwd / lstm_bwd call on `device` ended in since the last reset_lstm_kernel_counts, summed over its
    handles (asr_lstm_kernel_counts): the bf16 clusters of 16 / 32 / 64 units per CU, the fp32 three-term split, the exact
    fp32 clusters of 32 / 64 units per CU, or the single-CU kernels, forward and backward.  One count per call, however
    many tile groups it ran as.  Host counters: no device work, no synchronisation."""),
    ('att_path_counts', 'att_path_counts', None, 'reset_att_path_counts',
     """Which kernels the attention decoder calls on `device` launched since the last reset, summed over its handles
    (asr_att_path_counts): decoder-loop steps by path (forward step, forward cell, backward step, backward cell product,
    softmax backward) and energy / location / fused-step launches by lane shape.  Host counters: no device work, no
    synchronisation."""),
    ('conv_path_counts', 'conv_path_counts', None, 'reset_conv_path_counts',
     """Which kernel instantiations the conv3x3_* calls on `device` launched since the last reset, summed over its handles
    (asr_conv_path_counts): forward / data-gradient launches by form (img / tiled), channel pair of the product, and for
    the image-resident kernel MAXV, compile-time ACT, LDS buffers, stream / w8; weight-gradient calls by form, split,
    bias_in_kernel and reduce kernel.  Host counters: no device work, no synchronisation."""),
    ('gemm_path_counts', 'gemm_path_counts', _GEMM_PATH_KEYS, 'reset_gemm_path_counts',
     """What the listed-row products (gemm(..., rows=...)) on `device` ran since the last reset, summed over its handles
    (asr_gemm_path_counts): listed-row launches of the 128 x 128 and of the 256 x 256 NT kernel, and calls that ignored
    their list and ran the full product.  Host counters: no device work, no synchronisation."""),
    ('tn_frames_path_counts', 'gemm_path_counts', _TN_PATH_KEYS, None,
     """What the gemm_tn_frames calls on `device` ran since the last reset_gemm_path_counts: calls on the lean TN kernel
    and calls on the generic kernel (shape outside the lean TN path); neither loads the rows of padded frames."""),
    ('ctc_head_bwd_counts', 'gemm_path_counts', _HEAD_BWD_KEYS, None,
     """What the ctc_head_bwd calls on `device` ran since the last reset_gemm_path_counts: calls on the lean NT kernels
    (on the listed rows where a list was given) and calls that ran the full generic product."""),
    ('gemm_kernel_counts', 'gemm_path_counts', _GEMM_KERNEL_KEYS, None,
     """The kernel each full product on `device` ended in since the last reset_gemm_path_counts (gemm() without rows, and
    the listed-row / tn-frames / head-bwd calls that fell to the full product): the four skinny fp32 forms, the lean NT
    kernels by tile size, the lean TN kernel, the generic kernel by tile size and split-K; and the calls whose multiplier
    (mul_pass) or dropout (drop_pass) ran as a second pass instead of in an epilogue."""),
    ('ctc_head_counts', 'ctc_head_counts', None, 'reset_ctc_head_counts',
     """CTC head calls on `device` since the last reset (asr_ctc_head_counts): fused forward launches (ctc_head_fwd),
    ctc_loss_ex calls, and calls of the plain ctc_loss.  Host counters: no device work, no synchronisation."""),
    ('ctc_ls_counts', 'ctc_ls_counts', None, 'reset_ctc_ls_counts',
     """ctc_loss_ls calls on `device` since the last reset (asr_ctc_ls_counts): all, those that continued from
    ctc_head_fwd's workspace, those without a gradient.  Host counters: no device work, no synchronisation."""),
    ('att_beam_counts', 'att_beam_counts', None, 'reset_att_beam_counts',
     """Launches of the beam search kernels on `device` since the last reset, summed over its handles
    (asr_att_beam_counts).  Host counters: no device work, no synchronisation."""),
    ('att_joint_counts', 'att_joint_counts', None, 'reset_att_joint_counts',
     """Launches of the joint-search entry points on `device` since the last reset, summed over its handles
    (asr_att_joint_counts).  Host counters: no device work, no synchronisation."""),
    ('att_gru_counts', 'att_gru_counts', None, 'reset_att_gru_counts',
     """GRU decoder steps on `device` since the last reset, summed over its handles (asr_att_gru_counts): two-launch forward
    steps, four-launch forward steps, backward steps.  Host counters: no device work, no synchronisation."""),
    ('att_stack_counts', 'att_stack_counts', None, 'reset_att_stack_counts',
     """Upper-layer steps of decoder stacks on `device` since the last reset, summed over its handles
    (asr_att_stack_counts): forward on the image (one launch), forward as product + cell, backward fused, backward generic.
    Host counters: no device work, no synchronisation."""),
    ('att_lm_counts', 'att_lm_counts', None, 'reset_att_lm_counts',
     """Calls of the LM-fusion entry points on `device` since the last reset, summed over its handles (asr_att_lm_counts).
    Host counters: no device work, no synchronisation."""),
    ('ctc_beam_lm_counts', 'ctc_beam_lm_counts', None, 'reset_ctc_beam_lm_counts',
     """Launches of the LM-fused CTC prefix search on `device` since the last reset, summed over its handles
    (asr_ctc_beam_lm_counts): frame kernels, LM steps, commits.  Host counters: no device work, no synchronisation."""),
    ('weight_noise_counts', 'weight_noise_counts', None, 'reset_weight_noise_counts',
     """weight_noise_perturb calls on `device` since the last reset (asr_weight_noise_counts): calls, elements, calls that
    ran the 16-byte kernel.  Host counters: no device work, no synchronisation."""),
    ('input_augment_counts', 'input_augment_counts', None, 'reset_input_augment_counts',
     """input_augment calls on `device` since the last reset (asr_input_augment_counts): calls, elements, calls that ran
    the 16-byte kernel.  Host counters: no device work, no synchronisation."""),
)


def _views():
    """VIEWS, each view's offset the running total of the keys of its family's views in front of it."""
    out, used = collections.OrderedDict(), {}
    for name, family, keys, reset, doc in _VIEW_ROWS:
        keys = FAMILIES[family].keys if keys is None else keys
        out[name] = View(name, family, used.get(family, 0), keys, reset, doc)
        used[family] = out[name].offset + len(keys)
    return out


VIEWS = _views()
