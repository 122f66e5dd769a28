"""The recorded bits of fused pooled ASSS (tests/golden/pooled_asss_bits.npz).

TEST INFRASTRUCTURE ONLY (never imported by the product package).

The fused kernel (amh_pooled_asss_stats_k) is otherwise pinned to a float64
reference within tolerances and byte-equal to its external twin, which shares
its pieces; the fixture holds what one build of the library computed, so that a
later build is compared with it byte for byte.  run() is the one statement of
what is recorded: tests/golden/make_pooled_asss_bits.py saves it,
tests/test_gpu_pooled_asss.py compares with it.

Cases (kind, d, C, K): S^1 and a 1 x 1 factor; fewer chains than one chunk;
33 chunks with a ragged tail and a K-block; odd d with padded LDS rows; the
full wave and the kernel's EXACT instance; one case per model instantiation.
"""
from __future__ import annotations

import os

import numpy as np

CASES = [("gaussian", 1, 65, 1), ("gaussian", 2, 40, 1), ("gaussian", 7, 517, 4), ("gaussian", 33, 300, 1),
         ("gaussian", 64, 300, 2), ("eight_schools", None, 70, 1), ("kidiq", None, 70, 1), ("diamonds", None, 70, 1),
         ("diamonds_ss", None, 70, 1), ("poisson", 8, 70, 1)]
SEED = 7
NUM_WARMUP = 4
BLOCKS = 3
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pooled_asss_bits.npz")


def case_id(kind, d, C, K):
    return f"{kind}_{d or 0}_{C}_{K}"


def run(kind, d, C, K):
    """BLOCKS blocks of PooledASSS from init with PRNGKey(SEED), num_warmup =
    NUM_WARMUP and z0 uniform(-2, 2) from default_rng(SEED) -> {name: array}:
    per block b the sums, the shared leaves and pe; z after the last block."""
    import torch
    from helpers import make_case, shared_to_host
    from kernels_amd import PooledASSS, PRNGKey
    kw, mk, om = make_case(kind, d)
    z0 = np.random.default_rng(SEED).uniform(-2, 2, size=(C, om.d)).astype(np.float32)
    k = PooledASSS(num_chains=C, sync_every=K, **kw)
    st = k.init(PRNGKey(SEED), NUM_WARMUP, torch.as_tensor(z0), (), mk)
    out = {}
    for b in range(BLOCKS):
        st = k.sample(st)
        torch.cuda.synchronize()
        out[f"b{b}_sums"] = k._sums.cpu().numpy().copy()
        out[f"b{b}_pe"] = st.potential_energy.cpu().numpy().copy()
        for name, v in shared_to_host(st).items():
            out[f"b{b}_{name}"] = v
    out["z"] = st.z.cpu().numpy().copy()
    return out
