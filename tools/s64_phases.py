"""Where a wave of the headline launch (arwmh_step64_kernel, d = 64, 65,536
chains) spends its loop: per-wave totals of the four phases of one iteration
on the constant 100 MHz clock, from the diagnostic build (make -C
adaptive-mcmc_amd/csrc stamps):
  (a) the vmcnt(0) wait for the chain's DMA at the top of the loop,
  (b) hand-over start -> first factor store issued,
  (c) -> last DMA of the next chain issued (and the next ticket drawn),
  (d) compute, and its parts in the ARWMH transition: noise, proposal,
      potential, accept + schedule (with gamma), sweep 1 + coefficients, sweep 2
      (every stamp is a scalar-memory round trip: the parts carry their own
      cost and (d) is longer than in the release build).
Prints, per launch, the mean per iteration and the share of the loop of each
phase, and the spread over waves.  Usage (GPU box): python3 tools/s64_phases.py
(AMH_LIB_PATH selects another stamps build)."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("AMH_LIB_PATH", os.path.join(ROOT, "adaptive-mcmc_amd", "lib", "diag", "libamh_stamps.so"))
sys.path.insert(0, os.path.join(ROOT, "adaptive-mcmc_amd"))

import torch  # noqa: E402

import posteriors as P  # noqa: E402
from kernels_amd import ARWMH, PRNGKey  # noqa: E402
from kernels_amd import _lib  # noqa: E402

dev = torch.device("cuda", 0)
C, d = 65536, 64
k = ARWMH(potential_fn=P.correlated_gaussian(d), num_chains=C, device=dev)
st = k.init(PRNGKey(0), 0, (torch.rand(C, d, device=dev) * 4 - 2).contiguous(), (), {})
for _ in range(300):
    k.sample_(st, 1)
torch.cuda.synchronize()
W, S = 1 << 16, 16
L = _lib.lib()
L.amh_diag_s64_stamps.argtypes = [ctypes.c_void_p, ctypes.c_int64]
print(f"library {os.environ['AMH_LIB_PATH']}")
NAMES = ["(a) wait", "(b) ->1st store", "(c) ->last DMA", "(d) compute"]
SUB = ["noise", "proposal", "potential", "accept + gamma", "sweep 1 + coef", "sweep 2"]
for rep in range(3):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    k.sample_(st, 1)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    buf = np.zeros(W * S, np.uint64)
    assert L.amh_diag_s64_stamps(buf.ctypes.data, buf.nbytes) == 0
    s = buf.reshape(W, S)
    ph = s[s[:, 1] > 0]  # one record per wave (amh_step64.hip): start, end, items, block, phases (a) .. (d)
    if len(ph) == 0:
        sys.exit("no phase records: not a stamps build of this kernel")
    items = ph[:, 2].astype(np.float64)
    tot = ph[:, 4:8].astype(np.float64) * 10e-3  # us per wave
    loop = tot.sum(axis=1)
    print(f"launch {ms * 1e3:.1f} us (events); waves {len(ph)}; items/wave {items.mean():.2f}; "
          f"loop time per wave {loop.mean():.1f} us (min {loop.min():.1f} max {loop.max():.1f})")
    for i, n in enumerate(NAMES):
        per = tot[:, i] / np.maximum(items, 1)
        q = np.quantile(per, [0.1, 0.5, 0.9])
        print(f"  {n:16s} {tot[:, i].mean():7.1f} us per wave = {100 * tot[:, i].sum() / loop.sum():5.1f} % of the loop; "
              f"per iteration mean {per.mean():6.2f} us, 10/50/90 % of waves {q[0]:.2f} / {q[1]:.2f} / {q[2]:.2f}")
    sub = ph[:, 8:14].astype(np.float64) * 10e-3
    for i, n in enumerate(SUB):
        per = sub[:, i] / np.maximum(items, 1)
        q = np.quantile(per, [0.1, 0.5, 0.9])
        print(f"    (d) {n:14s} {100 * sub[:, i].sum() / max(tot[:, 3].sum(), 1e-9):5.1f} % of (d); "
              f"per iteration mean {per.mean():6.2f} us, 10/50/90 % of waves {q[0]:.2f} / {q[1]:.2f} / {q[2]:.2f}")
