"""TEST INFRASTRUCTURE: one LM-fused CTC prefix beam search of a small fixed configuration in a FRESH process, printed as one
SHA-256 digest (the style of tests/_lm_determinism_worker.py).

    python tests/_ctc_lm_determinism_worker.py     ->  a last line of 64 hex digits

tests/test_gpu_ctc_lm_fusion.py starts two of these and demands identical digests: the same seeded models and batch must
give the same labels, lengths, score and lm_score BITS in every process."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    import torch
    import test_gpu_ctc_lm_fusion as tc
    from tensorflow_end2end_speech_recognition_amd import ops
    from tensorflow_end2end_speech_recognition_amd.models.ctc.decoders.charlm_beam_search_decoder import lm_weights_of
    dev = torch.device('cuda:0')
    model, lm, x, sl, _ = tc.ctc_lm_models(tc.MODEL_SEED, dev)
    _, logits = model.compute_loss(x, np.zeros((len(sl), 1), dtype=np.int64), sl, keep_prob=1.0, is_training=False)
    out = ops.ctc_beam_decode_lm(logits.contiguous(), torch.as_tensor(sl, dtype=torch.int32, device=dev), 4,
                                 lm=lm_weights_of(lm), lm_weight=0.3, insertion_bonus=0.2)
    h = hashlib.sha256()
    for t in out:
        h.update(np.ascontiguousarray(t.cpu().numpy()).tobytes())
    ops.check_async_errors()
    print(h.hexdigest())


if __name__ == '__main__':
    for p in (os.path.dirname(HERE), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    main()
