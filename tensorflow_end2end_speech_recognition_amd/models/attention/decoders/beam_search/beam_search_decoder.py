"""Beam search over the attention decoder, host statement (models/attention/decoders/beam_search/beam_search_decoder.py of
the reference).  beam_search_step is one selection on torch tensors -- what att_beam_select_kernel computes per
utterance -- and BeamSearchDecoder drives it over any step function: the class-surface form of
AttentionSeq2Seq._decode_beam (whose native form is one call, ops.att_decoder_beam) and the oracle of its tests."""
import numpy as np
import torch

from .namedtuple import (BeamSearchDecoderOutput, BeamSearchDecoderState, BeamSearchStepOutput,
                         FinalBeamDecoderOutput)
from .util import check_beam_width, choose_top_k, gather_tree_py, mask_probs, normalize_score


def initial_beam_state(beam_width, dtype=torch.float64, device=None):
    """beam_search_decoder.py:165-169."""
    return BeamSearchDecoderState(log_probs=torch.zeros(beam_width, dtype=dtype, device=device),
                                  finished=torch.zeros(beam_width, dtype=torch.bool, device=device),
                                  lengths=torch.zeros(beam_width, dtype=torch.int64, device=device))


def beam_search_step(time, logits, beam_state, beam_width, vocab_size, eos_index, length_penalty_weight,
                     choose_successors_fn=choose_top_k, want_totals=False):
    """beam_search_decoder.py:234-332 for ONE utterance.  logits [W, C2]; returns (BeamSearchStepOutput,
    BeamSearchDecoderState).  want_totals: also the [W, C2] scores (tests measure selection margins on them)."""
    W, C2, eos = int(beam_width), int(vocab_size), int(eos_index)
    was_finished = beam_state.finished.bool()
    probs = mask_probs(torch.log_softmax(logits, dim=-1), eos, was_finished)
    total = beam_state.log_probs.to(probs.dtype).unsqueeze(1) + probs
    # a continuation is one longer unless it is <EOS> or its slot had finished
    grows = torch.ones(C2, dtype=torch.int64, device=logits.device)
    grows[eos] = 0
    cand_len = beam_state.lengths.long().unsqueeze(1) + (~was_finished).long().unsqueeze(1) * grows.unsqueeze(0)
    scores = normalize_score(total, cand_len, length_penalty_weight)
    # at the first step every slot holds the same hypothesis: only slot 0 continues
    flat = scores.reshape(-1) if int(time) > 0 else scores[0]
    next_scores, idx = choose_successors_fn(flat, W)
    word = idx % C2
    parent = idx // C2
    next_finished = was_finished[parent] | (word == eos)
    next_len = beam_state.lengths.long()[parent] + ((word != eos) & ~next_finished).long()
    out = BeamSearchStepOutput(scores=next_scores, predicted_ids=word, beam_parent_ids=parent)
    state = BeamSearchDecoderState(log_probs=total.reshape(-1)[idx], finished=next_finished, lengths=next_len)
    return (out, state, scores) if want_totals else (out, state)


class BeamSearchDecoder(object):
    """step_fn(time, predicted_ids, beam_parent_ids, decoder_state) -> (logits [W, C2], decoder_state) is the wrapped
    decoder for one utterance tiled to W rows: at time 0 both id arguments are None (<SOS>, the tiled initial state);
    later it gathers whatever it carries by beam_parent_ids and feeds the embedding of predicted_ids
    (beam_search_decoder.py:173-231)."""

    def __init__(self, step_fn, beam_width, vocab_size, eos_index, length_penalty_weight, max_decode_length,
                 choose_successors_fn=choose_top_k):
        self.step_fn = step_fn
        self.beam_width = check_beam_width(beam_width, vocab_size)
        self.vocab_size, self.eos_index = int(vocab_size), int(eos_index)
        self.length_penalty_weight = length_penalty_weight
        self.max_decode_length = int(max_decode_length)
        self.choose_successors_fn = choose_successors_fn

    def __call__(self, decoder_state, dtype=torch.float64):
        beam = initial_beam_state(self.beam_width, dtype)
        words, parents, scores, log_probs = [], [], [], []
        word = parent = None
        self.min_margin = float('inf')           # smallest gap between the W-th and the (W+1)-th candidate score seen
        for k in range(self.max_decode_length):
            logits, decoder_state = self.step_fn(k, word, parent, decoder_state)
            out, beam, all_scores = beam_search_step(k, logits.to(dtype), beam, self.beam_width, self.vocab_size,
                                                     self.eos_index, self.length_penalty_weight,
                                                     self.choose_successors_fn, want_totals=True)
            flat = torch.sort(all_scores.reshape(-1) if k > 0 else all_scores[0], descending=True, stable=True)[0]
            top = flat[:self.beam_width + 1]
            if len(top) > 1:
                self.min_margin = min(self.min_margin, float((top[:-1] - top[1:]).min()))
            word, parent = out.predicted_ids, out.beam_parent_ids
            words.append(word)
            parents.append(parent)
            scores.append(out.scores)
            log_probs.append(beam.log_probs)
            if bool(beam.finished.all()):
                break
        return self.finalize(words, parents, scores, log_probs), (decoder_state, beam)

    def finalize(self, words, parents, scores, log_probs):
        """beam_search_decoder.py:125-150: predicted_ids [steps, W] = gather_tree over (word, parent)."""
        w, p = torch.stack(words).cpu().numpy(), torch.stack(parents).cpu().numpy()
        step_out = BeamSearchDecoderOutput(logits=None, predicted_ids=w, log_probs=torch.stack(log_probs),
                                           scores=torch.stack(scores), beam_parent_ids=p, original_outputs=None)
        return FinalBeamDecoderOutput(predicted_ids=gather_tree_py(w, p), beam_search_output=step_out)


def cut_at_eos(ids, eos_index):
    """One back-traced hypothesis (1-D) up to and including its first <EOS>."""
    ids = [int(v) for v in np.asarray(ids).reshape(-1)]
    return ids[:ids.index(int(eos_index)) + 1] if int(eos_index) in ids else ids
