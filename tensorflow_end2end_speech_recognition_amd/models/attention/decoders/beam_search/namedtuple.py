"""The records the beam search passes around (models/attention/decoders/beam_search/namedtuple.py of the reference: same
names, same field order)."""
from collections import namedtuple

# what the search returns: predicted_ids = the back-traced hypotheses, beam_search_output = the per-step record below
FinalBeamDecoderOutput = namedtuple('FinalBeamDecoderOutput', ['predicted_ids', 'beam_search_output'])

# one step (or, stacked over time, the whole search) as the decoder interface reports it
BeamSearchDecoderOutput = namedtuple('BeamSearchDecoderOutput', ['logits', 'predicted_ids', 'log_probs', 'scores',
                                                                 'beam_parent_ids', 'original_outputs'])

# what a step carries to the next: per slot, the total log probability, the finished flag and the hypothesis length
BeamSearchDecoderState = namedtuple('BeamSearchDecoderState', ['log_probs', 'finished', 'lengths'])

# what a step selects: per slot, the score, the word and the slot of the previous step it continues
BeamSearchStepOutput = namedtuple('BeamSearchStepOutput', ['scores', 'predicted_ids', 'beam_parent_ids'])
