"""TEST INFRASTRUCTURE: one LM-fused joint decode of a small fixed configuration in a FRESH process, printed as one SHA-256
digest (the style of tests/_determinism_worker.py).

    python tests/_lm_determinism_worker.py     ->  a last line of 64 hex digits

tests/test_gpu_lm_fusion.py starts two of these and demands identical digests: the same seeded models and batch must give
the same hypotheses, lengths, scores, lm_score and ctc_score BITS in every process."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    import torch
    import test_gpu_lm_fusion as tl
    from tensorflow_end2end_speech_recognition_amd import ops
    model, lm, x, sl, _, _, _ = tl.fused_models('f32', 7, torch.device('cuda:0'))
    model.infer(x, sl, beam_width=4, length_penalty_weight=0.6, ctc_weight=0.3, lm=lm, lm_weight=0.3)
    raw = model._beam_raw
    h = hashlib.sha256()
    for k in ('ids', 'hyp_len', 'scores', 'lm_score', 'ctc_score'):
        h.update(np.ascontiguousarray(raw[k]).tobytes())
    ops.check_async_errors()
    print(h.hexdigest())


if __name__ == '__main__':
    for p in (os.path.dirname(HERE), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    main()
