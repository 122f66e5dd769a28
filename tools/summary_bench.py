"""Streaming summaries (csrc/amh_summary.hip, infer_amd.StreamingSummary):
  update   seconds per StreamingSummary.update of one block x [B, C, k] and the
           achieved bytes / s with bytes = 4 B C k + 80 C k (the block read once,
           the five float64 accumulators read and written), next to a torch copy
           of the same block timed in the same process (4 B C k read + 4 B C k
           written).  Once for spread draws (normals, 8 std range) and once for
           draws that all fall into one bin per column: the LDS-atomic worst case
  mcmc     MCMC on the correlated Gaussian, stored draws against
           summary_only=True: wall seconds of run() and
           torch.cuda.max_memory_allocated
Device seconds are the median of `--reps` runs after two untimed ones, by
device events.  DESIGN.md §7.1 holds the table.
Usage (GPU box): python3 tools/summary_bench.py [--out profiles/summary_bench.jsonl]
                 [--chains 65536] [--cols 64] [--draws 64] [--nbins 512] [--reps 10]
                 [--samples 1000] [--warmup 200] [--skip-mcmc]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "adaptive-mcmc_amd"))
import torch  # noqa: E402

import posteriors as P  # noqa: E402
from infer_amd import MCMC, StreamingSummary  # noqa: E402
from kernels_amd import ARWMH, PRNGKey  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "summary_bench.jsonl"))
ap.add_argument("--chains", type=int, default=65536)
ap.add_argument("--cols", type=int, default=64)
ap.add_argument("--draws", type=int, default=64)
ap.add_argument("--nbins", type=int, default=512)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--samples", type=int, default=1000)
ap.add_argument("--warmup", type=int, default=200)
ap.add_argument("--skip-mcmc", action="store_true")
args = ap.parse_args()

dev = torch.device("cuda", 0)
rows = []


def emit(rec):
    rows.append(rec)
    print(json.dumps(rec), flush=True)


def device_seconds(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3)
    return statistics.median(out), min(out), max(out)


B, C, k = args.draws, args.chains, args.cols
block_bytes = 4 * B * C * k
x = torch.empty(B, C, k, dtype=torch.float32, device=dev)
dst = torch.empty_like(x)
sec, lo, hi = device_seconds(lambda: dst.copy_(x), args.reps)
emit(dict(kind="copy", B=B, C=C, k=k, seconds=sec, seconds_min=lo, seconds_max=hi, bytes=2 * block_bytes,
          bytes_per_s=2 * block_bytes / sec))
del dst
for name in ("spread", "one_bin"):
    if name == "spread":
        x.normal_()
    else:
        x.fill_(0.25)
    s = StreamingSummary(C, k, batch=8, nbins=args.nbins, device=dev).set_range([0.0] * k, [8.0] * k)
    sec, lo, hi = device_seconds(lambda: s.update(x), args.reps)
    nbytes = block_bytes + 80 * C * k
    emit(dict(kind="update", draws=name, B=B, C=C, k=k, nbins=args.nbins, seconds=sec, seconds_min=lo,
              seconds_max=hi, bytes=nbytes, bytes_per_s=nbytes / sec, elements_per_s=B * C * k / sec,
              occupied_bins_col0=int((s.hist[0] > 0).sum())))
    del s
del x
torch.cuda.empty_cache()

if not args.skip_mcmc:
    d = 64
    g = P.correlated_gaussian(d)
    z0 = torch.zeros(C, d)
    for mode in ("stored", "summary_only"):
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        m = MCMC(ARWMH(potential_fn=g, num_chains=C, device=dev), num_warmup=args.warmup, num_samples=args.samples)
        torch.cuda.synchronize()
        t = time.perf_counter()
        m.run(PRNGKey(0), init_params=z0, summary_only=(mode == "summary_only"))
        torch.cuda.synchronize()
        run_s = time.perf_counter() - t
        t = time.perf_counter()
        if mode == "summary_only":
            st = m.streaming_summary.summary()
            mean0, n_eff0 = float(st["mean"][0]), float(st["n_eff"][0])
        else:
            z = m.get_samples(group_by_chain=True)
            mean0, n_eff0 = float(z[..., 0].double().mean()), None
            del z
        torch.cuda.synchronize()
        emit(dict(kind="mcmc", mode=mode, chains=C, d=d, warmup=args.warmup, samples=args.samples, run_seconds=run_s,
                  result_seconds=time.perf_counter() - t, max_memory_allocated=torch.cuda.max_memory_allocated(dev),
                  mean0=mean0, n_eff0=n_eff0))
        del m

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    for rec in rows:
        f.write(json.dumps(rec) + "\n")
print(f"wrote {args.out}")
