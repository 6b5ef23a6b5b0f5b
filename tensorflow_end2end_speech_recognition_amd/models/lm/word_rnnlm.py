"""Word-level RNN language model (models/lm/word_rnnlm.py of the reference, a stub there that raises
NotImplementedError).  EXTENSION: the definition is RNNLM's (base.py); this class only names the unit.  It fuses with a
word-level attention model; a word-level LM for a character model is out of scope (lm_fusion.py)."""
from .base import RNNLM


class WordRNNLM(RNNLM):
    """RNNLM over word classes."""

    def __init__(self, *args, **kwargs):
        kwargs.setdefault('name', 'word_rnnlm')
        super(WordRNNLM, self).__init__(*args, **kwargs)
