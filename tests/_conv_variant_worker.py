"""TEST INFRASTRUCTURE (child process of tests/test_gpu_conv3x3_variants.py::test_switched_kernels_in_a_fresh_process):

    python tests/_conv_variant_worker.py     ->  one line 'CONV ' + JSON {"counts": {...}, "digests": {...}}

The eight ASR_CONV_* switches are read once per process into static constants, so a kernel behind a switch can only be
reached by a process that starts with the switch set.  This one reads the same switches from its environment, runs the
fixed list of layer shapes of tests/_conv_variants.py (WORKER_FORWARD, WORKER_WGRAD) against the fp64 references with the
bounds stated there, and asserts the path counters of every launch against the dispatch rule under those switches."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch                                                                            # noqa: E402

from _conv_variants import (Tally, WORKER_FORWARD, WORKER_WGRAD, check_forward_family,  # noqa: E402
                            check_weight_gradient, switches)


def main():
    from tensorflow_end2end_speech_recognition_amd import ops
    sw = switches()
    tally = Tally()
    digests = {}
    for c in WORKER_FORWARD:
        digests['fwd %d %d %d %d %d' % c] = check_forward_family(tally, *c, sw=sw)
    for c in WORKER_WGRAD:
        digests['wgrad %d %d %d %d %d' % c] = check_weight_gradient(tally, *c, sw=sw)
    torch.cuda.synchronize()
    assert ops.check_async_errors(0) == 0
    print('CONV ' + json.dumps(dict(counts=tally.total, digests=digests), sort_keys=True))


if __name__ == '__main__':
    main()
