"""wasserstein_dist11_p: method="auction" (device, csrc/amh_assign.hip) against
method="hungarian" (host scipy) on the grid of the reference's
compare_wasserstein.py, n in {30, 100, 300, 1000, 3000, 10000} x d in
{5, 10, 25}, on the stored diamonds draws (tests/golden/diamonds_example_*.npz,
last n rows and last d columns), and the rounds / seconds of
linear_assignment at theta in {2, 4, 8, 16} (DESIGN.md §8 holds the tables).
Device seconds: the best of `--reps` runs after one untimed run, each ended by
a synchronize; host seconds: one run.
Usage (GPU box): python3 tools/assign_bench.py [--out profiles/assign_grid.jsonl]
                 [--min-n 30] [--max-n 10000] [--hungarian-max-n 10000] [--reps 3] [--no-theta]
The host path at n = 10000 on these draws runs for many minutes per cell;
--hungarian-max-n 3000 leaves it out (the record then holds null for it)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "adaptive-mcmc_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch  # noqa: E402

import extract_diamonds_pkl as X  # noqa: E402
from utils_amd import evaluation as E  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assign_grid.jsonl"))
ap.add_argument("--min-n", type=int, default=30)
ap.add_argument("--max-n", type=int, default=10000)
ap.add_argument("--no-theta", action="store_true", help="skip the theta sweep")
ap.add_argument("--hungarian-max-n", type=int, default=10000)
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()

references, samples, _ = X.load_fixture()
rows = []


def emit(rec):
    rows.append(rec)
    print(json.dumps(rec), flush=True)


def cost_matrix(n, d):
    x, y = E._dev(references[-n:, -d:]), E._dev(samples[-n:, -d:])
    return x, y, E._dist2(x, y).clamp_(min=0.0).sqrt_()


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    best, out = float("inf"), None
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    return best, out


# theta sweep: the solver alone on a ready cost matrix
for n, d in [(1000, 25), (3000, 5), (3000, 25), (10000, 25)]:
    if args.no_theta or not args.min_n <= n <= args.max_n:
        continue
    _, _, C = cost_matrix(n, d)
    for theta in (2, 4, 8, 16):
        sec, r = timed(lambda: E.linear_assignment(C, theta=theta), args.reps)
        emit(dict(kind="theta", n=n, d=d, theta=theta, rounds=r["rounds"], phases=r["phases"], seconds=sec,
                  cost=r["cost"], converged=r["converged"]))

# the grid: both methods end to end (cost matrix included), default theta
for n in (30, 100, 300, 1000, 3000, 10000):
    if not args.min_n <= n <= args.max_n:
        continue
    for d in (5, 10, 25):
        x, y, C = cost_matrix(n, d)
        r = E.linear_assignment(C)
        sec, val = timed(lambda: E.wasserstein_dist11_p(x, y, method="auction"), args.reps)
        rec = dict(kind="grid", n=n, d=d, theta=E.ASSIGN_THETA, rounds=r["rounds"], phases=r["phases"],
                   quantum=r["quantum"], auction_seconds=sec, auction=val, hungarian_seconds=None, hungarian=None)
        if n <= args.hungarian_max_n:
            xh, yh = references[-n:, -d:], samples[-n:, -d:]
            t = time.perf_counter()
            rec["hungarian"] = E.wasserstein_dist11_p(xh, yh)
            rec["hungarian_seconds"] = time.perf_counter() - t
        emit(rec)

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    for rec in rows:
        f.write(json.dumps(rec) + "\n")
print(f"wrote {args.out}")
