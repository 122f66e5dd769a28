"""Pooled ASSS against the kernels it sits beside, in one run:
python3 tools/pooled_asss_run.py [reps] [window_s]

Shapes: the d = 64 Gaussian at C = 65,536 with sync_every 1 and 16, and eight
schools at C = 262,144.  At each shape PooledASSS, per-chain ASSS.sample_ and
PooledARWMH (d = 64 Gaussian: its MFMA form; d = 63 Gaussian and eight
schools: the lane-per-row form PooledASSS shares) are timed in turn, `reps`
times round robin, each window sized to about `window_s` seconds of steps and
ended by a device synchronise.  Prints chain-steps/s and ms per block (median,
min - max over the repetitions) and one JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "adaptive-mcmc_amd"))
import torch  # noqa: E402

import posteriors as P  # noqa: E402
from kernels_amd import ASSS, PooledARWMH, PooledASSS, PRNGKey  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
WINDOW = float(sys.argv[2]) if len(sys.argv) > 2 else 0.5


def make(cls, shape, C, K):
    kw = dict(num_chains=C) if cls is ASSS else dict(num_chains=C, sync_every=K)
    if shape == "eight_schools":
        k = cls(model=P.eight_schools, **kw)
        return k, k.init(PRNGKey(0), 0, None, (), dict(P.EIGHT_SCHOOLS_DATA))
    d = int(shape[1:])
    k = cls(potential_fn=P.correlated_gaussian(d), **kw)
    return k, k.init(PRNGKey(0), 0, (torch.rand(C, d, device="cuda") * 4 - 2).contiguous(), (), {})


def window(k, st, steps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    k.sample_(st, steps)
    torch.cuda.synchronize()
    return time.perf_counter() - t


def main():
    rows = [("d64", 65536, 1), ("d64", 65536, 16), ("d63", 65536, 1), ("eight_schools", 262144, 1)]
    out = []
    for shape, C, K in rows:
        legs = []
        for name, cls in (("PooledASSS", PooledASSS), ("ASSS per chain", ASSS), ("PooledARWMH", PooledARWMH)):
            k, st = make(cls, shape, C, K)
            k.sample_(st, 20 * K)  # past the first blocks, whose factor is still the identity
            el = window(k, st, 4 * K)
            steps = max(K, int(WINDOW / (el / (4 * K))) // K * K)
            legs.append((name, k, st, steps, []))
        for _ in range(REPS):
            for name, k, st, steps, ts in legs:
                ts.append(window(k, st, steps) / steps)
        for name, k, st, steps, ts in legs:
            ts.sort()
            med = ts[len(ts) // 2]
            rec = dict(shape=shape, C=C, K=K, sampler=name, steps=steps, ms_per_block=med * K * 1e3,
                       chain_steps_per_s=C / med, lo=C / ts[-1], hi=C / ts[0])
            out.append(rec)
            print(f"{shape:14s} C={C:6d} K={K:2d} {name:15s}: {rec['chain_steps_per_s']:.4g} chain-steps/s "
                  f"({rec['lo']:.4g} - {rec['hi']:.4g}), {rec['ms_per_block']:.4f} ms/block, {steps} steps/window")
        del legs
        torch.cuda.empty_cache()
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), reps=REPS, rows=out)))


if __name__ == "__main__":
    main()
