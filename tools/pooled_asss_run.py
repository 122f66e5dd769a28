"""Pooled ASSS against the kernels it sits beside, in one run:
python3 tools/pooled_asss_run.py [reps] [window_s]

Shapes: the d = 64 Gaussian at C = 65,536 with sync_every 1 and 16, and eight
schools at C = 262,144.  At each shape PooledASSS, per-chain ASSS.sample_ and
PooledARWMH (d = 64 Gaussian: its MFMA form; d = 63 Gaussian and eight
schools: the lane-per-row form PooledASSS shares) are timed in turn, `reps`
times round robin, each window sized to about `window_s` seconds of steps and
ended by a device synchronise.  Prints chain-steps/s and ms per block (median,
min - max over the repetitions) and one JSON line.

python3 tools/pooled_asss_run.py external [N]
The cost of cutting the transition around a caller's potential: the d = 64
Gaussian at C = 65,536, K = 1, one rank, PooledASSS(host_shrink=True) with the
library's own Gaussian potential (amh_potential) behind the callable against
the fused PooledASSS of the same build from the same start and key (the two
runs are byte-identical).  After 20 transitions, three windows of N single
transitions each (HIP events): seconds per transition (median, min - max), the
mean and maximum shrink rounds per transition, and the ratio.

python3 tools/pooled_asss_run.py legs [N]
The legs an A/B of two builds compares (select the build with AMH_LIB_PATH):
the fused PooledASSS step at d = 64, C = 65,536, K = 1 and at eight schools,
C = 262,144; the per-chain ASSS(host_shrink=True) step at d = 64, C = 512
around the library's potential; the lane-per-row PooledARWMH step at d = 63,
C = 65,536 and at eight schools, C = 262,144; and, around the library's
potential behind a callable at C = 65,536, the PooledARWMH step at d = 63
(pooled_ext_stats_kernel) and the PooledASSS(host_shrink=True) step at d = 64
(pooled_asss_ext_finish_kernel); one JSON line with us per transition of each."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "adaptive-mcmc_amd"))
import torch  # noqa: E402

import posteriors as P  # noqa: E402
from kernels_amd import ASSS, PooledARWMH, PooledASSS, PRNGKey  # noqa: E402

MODE = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] in ("external", "legs") else "shapes"
ARGS = sys.argv[2:] if MODE != "shapes" else sys.argv[1:]
REPS = int(ARGS[0]) if MODE == "shapes" and len(ARGS) > 0 else 5
WINDOW = float(ARGS[1]) if MODE == "shapes" and len(ARGS) > 1 else 0.5
N = int(ARGS[0]) if MODE != "shapes" and len(ARGS) > 0 else 100


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


def timed(step, n):
    """us per call of `step` over one window of n calls (HIP events)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def library_potential(d):
    """The library's Gaussian potential as a plain callable."""
    kg = ASSS(potential_fn=P.correlated_gaussian(d), num_chains=8)
    kg.init(PRNGKey(1), 0, torch.zeros(8, d), (), {})
    return lambda z: kg.potential(z)


def external():
    d, C = 64, 65536
    z0 = (torch.rand(C, d, device="cuda") * 4 - 2).contiguous()
    kf = PooledASSS(potential_fn=P.correlated_gaussian(d), num_chains=C)
    sf = kf.init(PRNGKey(0), 0, z0, (), {})
    ke = PooledASSS(potential_fn=library_potential(d), num_chains=C, host_shrink=True)
    se = ke.init(PRNGKey(0), 0, z0, (), {})
    kf.sample_(sf, 20)
    ke.sample_(se, 20)
    rounds = []

    def ext_step():
        ke.sample_(se, 1)
        rounds.append(ke.shrink_rounds)

    te, tf = [], []
    for _ in range(3):
        te.append(timed(ext_step, N))
        tf.append(timed(lambda: kf.sample_(sf, 1), N))
    torch.cuda.synchronize()
    same = bool(torch.equal(se.z, sf.z)) and bool(torch.equal(se.adapt_state.scale, sf.adapt_state.scale))
    te.sort()
    tf.sort()
    r = torch.tensor(rounds, dtype=torch.float64)
    rec = dict(mode="external", d=d, C=C, K=1, n=N, external_s=te[1] * 1e-6, external_lo_s=te[0] * 1e-6,
               external_hi_s=te[2] * 1e-6, fused_s=tf[1] * 1e-6, fused_lo_s=tf[0] * 1e-6, fused_hi_s=tf[2] * 1e-6,
               ratio=te[1] / tf[1], rounds_mean=float(r.mean()), rounds_max=int(r.max()), same_bytes=same)
    print(f"d={d} C={C} K=1: external {rec['external_s']:.3e} s per transition ({te[0] * 1e-6:.3e} - "
          f"{te[2] * 1e-6:.3e}), rounds mean {rec['rounds_mean']:.2f} max {rec['rounds_max']}; fused "
          f"{rec['fused_s']:.3e} s ({tf[0] * 1e-6:.3e} - {tf[2] * 1e-6:.3e}); ratio {rec['ratio']:.1f}; "
          f"states byte-equal: {same}")
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), **rec)))


def legs():
    d = 64
    out = {}

    def leg(name, k, st, warm, n):
        k.sample_(st, warm)
        out[name] = sorted(timed(lambda: k.sample_(st, 1), n) for _ in range(3))[1]

    def start(C, dim):
        return (torch.rand(C, dim, device="cuda") * 4 - 2).contiguous()

    kf = PooledASSS(potential_fn=P.correlated_gaussian(d), num_chains=65536)
    leg("pooled_asss_fused_us", kf, kf.init(PRNGKey(0), 0, start(65536, d), (), {}), 20, 4 * N)
    ka = ASSS(potential_fn=library_potential(d), num_chains=512, host_shrink=True)
    leg("asss_host_shrink_us", ka, ka.init(PRNGKey(0), 0, start(512, d), (), {}), 100, N)
    for name, cls in (("pooled_asss_es_us", PooledASSS), ("pooled_arwmh_es_us", PooledARWMH)):
        k, st = make(cls, "eight_schools", 262144, 1)
        leg(name, k, st, 20, 4 * N)
    k, st = make(PooledARWMH, "d63", 65536, 1)
    leg("pooled_arwmh_d63_us", k, st, 20, 4 * N)
    ke = PooledARWMH(potential_fn=library_potential(63), num_chains=65536)
    leg("pooled_arwmh_ext_d63_us", ke, ke.init(PRNGKey(0), 0, start(65536, 63), (), {}), 20, N)
    kh = PooledASSS(potential_fn=library_potential(d), num_chains=65536, host_shrink=True)
    leg("pooled_asss_ext_us", kh, kh.init(PRNGKey(0), 0, start(65536, d), (), {}), 20, N)
    print(json.dumps(dict(mode="legs", lib=os.environ.get("AMH_LIB_PATH", "release"), n=N, **out)))


if __name__ == "__main__":
    dict(shapes=main, external=external, legs=legs)[MODE]()
