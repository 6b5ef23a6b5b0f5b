"""TEST INFRASTRUCTURE (child process of tests/test_gpu_gemm_variants.py::test_switched_nt_kernels_in_a_fresh_process):

    python tests/_gemm_variant_worker.py     ->  one line 'GEMM ' + JSON {"counts": {...}, "digests": {...}}

ASR_GEMM_NT_BIG is read once per process into a static constant, so the 256 x 256 NT kernel at small shapes (= 2) and the
128 x 128 kernel at shapes the default gives to the large tiles (= 0) can only be reached by a process that starts with
the switch set.  This one reads the same switch from its environment, runs the NT shapes of tests/_gemm_variants.py
(WORKER_SHAPES, every form of WORKER_FORMS, fp32 and bf16 results) on integer data against the exact fp64 reference, one
shape on gaussian data, and asserts the kernel counters of every call against the dispatch rule under that switch."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch                                                                            # noqa: E402

from _gemm_variants import (Case, Tally, WORKER_FORMS, WORKER_GAUSSIAN, WORKER_SHAPES,  # noqa: E402
                            check_product, nt_big_switch)


def main():
    from tensorflow_end2end_speech_recognition_amd import ops
    big = nt_big_switch(os.environ)
    tally = Tally()
    digests = {}
    for s in WORKER_SHAPES:
        check_product(tally, Case('bf16', 0, 1, *s), WORKER_FORMS, big=big, results=digests)
    check_product(tally, Case('bf16', 0, 1, *WORKER_GAUSSIAN), WORKER_FORMS, regime='gaussian', big=big)
    torch.cuda.synchronize()
    assert ops.check_async_errors(0) == 0
    print('GEMM ' + json.dumps(dict(counts=tally.total, digests=digests), sort_keys=True))


if __name__ == '__main__':
    main()
