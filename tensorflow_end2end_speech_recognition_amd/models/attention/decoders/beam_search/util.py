"""The pieces of a beam search step on torch tensors (models/attention/decoders/beam_search/util.py of the reference):
the host statement of what att_beam_select_kernel / att_beam_backtrace_kernel compute, in whatever floating dtype the
caller's tensors have (the tests run it in fp64)."""
import numpy as np
import torch

MAX_BEAM_WIDTH = 32          # the kernels keep one candidate list per wave lane group; asr_att_beam_select refuses more
F32_MIN = float(np.finfo(np.float32).min)


def check_beam_width(beam_width, vocab_size):
    """1 <= beam_width <= 32, and no wider than the vocabulary: step 0 selects among ONE slot's vocab_size candidates
    (beam_search_decoder.py:287-290), where the reference's top_k would be asked for more entries than there are."""
    w = int(beam_width)
    if w < 1 or w > MAX_BEAM_WIDTH:
        raise ValueError('beam_width must be in 1 .. %d, got %d' % (MAX_BEAM_WIDTH, w))
    if w > int(vocab_size):
        raise ValueError('beam_width %d exceeds the %d classes (num_classes + 2) step 0 selects among' % (w, vocab_size))
    return w


def gather_tree_py(values, parents):
    """util.py:14-26.  values / parents [steps, W] (numpy): row `level` of the result holds, per final slot, the value on
    the path that ends in that slot."""
    values, parents = np.asarray(values), np.asarray(parents)
    steps, W = values.shape
    res = np.zeros_like(values)
    res[-1] = values[-1]
    for w in range(W):
        p = parents[-1][w]
        for level in range(steps - 2, -1, -1):
            res[level, w] = values[level][p]
            p = parents[level][p]
    return res


def mask_probs(probs, eos_token, finished):
    """util.py:37-68.  probs [W, C2] log-probabilities, finished [W] bool: a finished slot's row becomes 0 at <EOS> and
    float32.min elsewhere (all its mass on <EOS>), the others stay."""
    row = torch.full((probs.shape[1],), F32_MIN, dtype=probs.dtype, device=probs.device)
    row[int(eos_token)] = 0.0
    return torch.where(finished.bool().unsqueeze(1), row.unsqueeze(0), probs)


def length_penalty(lengths, length_penalty_weight, dtype):
    """((5 + len) ^ a) / (6 ^ a), https://arxiv.org/abs/1609.08144 (util.py:84-86)."""
    a = float(length_penalty_weight)
    return (5.0 + lengths.to(dtype)) ** a / (6.0 ** a)


def normalize_score(log_probs, sequence_lengths, length_penalty_weight):
    """util.py:71-95.  QUIRK, reproduced: a weight of exactly 1 returns the log-probabilities UN-normalised (the
    reference tests `length_penalty_weight == 1` where it means "disabled", util.py:90-91).  DEVIATION: None is read as
    0.0 (no penalty); the reference raises on None before it reaches its own None test."""
    a = 0.0 if length_penalty_weight is None else float(length_penalty_weight)
    if a == 1.0:
        return log_probs
    return log_probs / length_penalty(sequence_lengths, a, log_probs.dtype)


def choose_top_k(scores_flat, beam_width):
    """tf.nn.top_k (util.py:98-109): the beam_width largest, equal scores in ascending index order."""
    s, i = torch.sort(scores_flat, descending=True, stable=True)
    return s[:beam_width], i[:beam_width]
