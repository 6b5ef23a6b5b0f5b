"""Select & load encoder -- mirror of models/encoders/load_encoder.py:26-57.

The registry is the reference's plugin point: an encoder is a class with
__call__(inputs, inputs_seq_len, keep_prob, is_training) -> (outputs, final_state).
Keys of the reference not built here (vgg_wang, pyramid_blstm, student_*) raise the same
ValueError as an unknown key.  pyramid_blstm stays unknown: what the reference's unfinished pyramidal_blstm.py set out
to do is the `blstm` encoder with subsample_type='concat' (the subsample_list / subsample_type keywords of the models,
core/subsample.py), which needs no key of its own."""
from .core.blstm import BLSTMEncoder
from .core.lstm import LSTMEncoder
from .core.vgg_blstm import VGGBLSTMEncoder, VGGLSTMEncoder
from .core.multitask_blstm import MultitaskBLSTMEncoder
from .core.multitask_lstm import MultitaskLSTMEncoder
from .core.gru import GRUEncoder, BGRUEncoder
from .core.cldnn_wang import CLDNNEncoder
from .core.cnn_zhang import CNNEncoder

ENCODERS = {
    "blstm": BLSTMEncoder,
    "lstm": LSTMEncoder,
    "vgg_blstm": VGGBLSTMEncoder,
    "vgg_lstm": VGGLSTMEncoder,
    "multitask_blstm": MultitaskBLSTMEncoder,     # the same kernels recombined
    "multitask_lstm": MultitaskLSTMEncoder,
    "bgru": BGRUEncoder,
    "gru": GRUEncoder,
    "cldnn_wang": CLDNNEncoder,
    "cnn_zhang": CNNEncoder,
}


def register(encoder_type, cls):
    ENCODERS[encoder_type] = cls


def load(encoder_type):
    if encoder_type not in ENCODERS.keys():
        raise ValueError(
            "encoder_type should be one of [%s], you provided %s." %
            (", ".join(ENCODERS), encoder_type))
    return ENCODERS[encoder_type]
