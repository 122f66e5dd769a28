"""Record tests/golden/pooled_asss_bits.npz on a GPU: what the library selected
by AMH_LIB_PATH (default: the tree's own build) computes for the cases of
tests/pooled_asss_bits.py.  Run it with the build whose bits are to be kept --
before a refactor of the pooled ASSS kernels, the parent commit's libamh.so:

  AMH_LIB_PATH=/path/to/parent/libamh.so python tests/golden/make_pooled_asss_bits.py [OUT]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "adaptive-mcmc_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import pooled_asss_bits as bits  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else bits.PATH
    out = {}
    for case in bits.CASES:
        for name, v in bits.run(*case).items():
            out[f"{bits.case_id(*case)}/{name}"] = v
    np.savez_compressed(out_path, **out)
    print(f"{out_path}: {len(out)} arrays, {os.path.getsize(out_path)} bytes")


if __name__ == "__main__":
    main()
