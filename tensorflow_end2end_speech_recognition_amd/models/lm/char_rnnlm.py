"""Character-level RNN language model (models/lm/char_rnnlm.py of the reference, a stub there that raises
NotImplementedError).  EXTENSION: the definition is RNNLM's (base.py); this class only names the unit."""
from .base import RNNLM


class CharRNNLM(RNNLM):
    """RNNLM over character (or phone) classes: the unit of the attention model it is fused with."""

    def __init__(self, *args, **kwargs):
        kwargs.setdefault('name', 'char_rnnlm')
        super(CharRNNLM, self).__init__(*args, **kwargs)
