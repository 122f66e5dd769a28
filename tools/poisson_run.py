"""Poisson regression (AMH_MODEL_POISSON) at the diamonds shape, N = 5000,
K = 24, C = 262,144 chains, synthetic data with offsets: ms per transition of
ARWMH.sample_ over 20 calls after a 0.3 s warm-up (as tools/logistic_run.py),
the MFMA potential kernel alone by events, and the same posterior through the
external path with a torch restatement of U.
Usage (GPU box): python3 tools/poisson_run.py          all of the above
                 python3 tools/poisson_run.py trace    10 model transitions only
                 (under rocprofv3 --kernel-trace --stats -- for the kernels' own times)"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "adaptive-mcmc_amd"))
import torch  # noqa: E402

import posteriors as P  # noqa: E402
from kernels_amd import ARWMH, PRNGKey  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "all"
N, K, C = 5000, 24, 262144
dev = torch.device("cuda", 0)
data = P.synthetic_poisson(N, K, 9)
e = P.poisson_regression(data["X"], data["y"], data["offset"])
d = K + 1
g = torch.Generator(device=dev)
g.manual_seed(7)
# starts in U(-0.25, 0.25)^d: eta stays within a few units, as in a run that has converged
z0 = (torch.rand(C, d, device=dev, generator=g) * 0.5 - 0.25).contiguous()


def rate(k, st, steps, label):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.3:
        k.sample_(st, 1)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        k.sample_(st, 1)
    torch.cuda.synchronize()
    el = time.perf_counter() - t
    print(f"{label}: {el / steps * 1e3:.4f} ms per transition, {C * steps / el:.4g} chain-steps/s "
          f"(accept {float(st.mean_accept_prob.mean()):.3f})", flush=True)


km = ARWMH(model=e, num_chains=C, device=dev)
st = km.init(PRNGKey(0), 0, z0, (), {})
if mode == "trace":
    for _ in range(10):
        km.sample_(st, 1)
    torch.cuda.synchronize()
    sys.exit(0)
rate(km, st, 20, "poisson model, sample_(st, 1) x 20")
t = time.perf_counter()
km.sample_(st, 20)
torch.cuda.synchronize()
print(f"poisson model, sample_(st, 20): {(time.perf_counter() - t) / 20 * 1e3:.4f} ms per transition", flush=True)
# the MFMA potential alone, by events
ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for _ in range(3):
    km.potential(st.z)
ev0.record()
for _ in range(20):
    km.potential(st.z)
ev1.record()
torch.cuda.synchronize()
ms = ev0.elapsed_time(ev1) / 20
print(f"amh_potential (MFMA kernel) by events: {ms:.4f} ms per call = {N * C / ms / 1e6:.4g} G row-chain elements/s",
      flush=True)

# the only way the parent commit runs this model: a torch restatement through the external path
X = torch.as_tensor(e.X, device=dev)
y = torch.as_tensor(e.y, device=dev)
o = torch.as_tensor(e.offset, device=dev)
iI2, ib2, c0 = (float(v) for v in e.consts)
Xt = X.t().contiguous()
Xy = X.t() @ y
yo = float((y.double() * o.double()).sum())


def U(z):
    eta = torch.addmm((z[:, :1] + o), z[:, 1:], Xt)   # [C, N]
    # sum_n exp(eta) - y.eta, the second term through X'y (no second [C, N] pass)
    s = torch.exp_(eta).sum(-1) - (z[:, 0] * y.sum() + z[:, 1:] @ Xy + yo)
    return s + 0.5 * ib2 * (z[:, 1:] ** 2).sum(-1) + 0.5 * iI2 * z[:, 0] ** 2 + c0


kt = ARWMH(potential_fn=U, num_chains=C, device=dev)
st2 = kt.init(PRNGKey(0), 0, z0, (), {})
u_m = km.potential(z0)
u_t = U(z0)
print("torch U vs model U at the starts: max rel diff", float(((u_m - u_t).abs() / u_m.abs()).max()), flush=True)
rate(kt, st2, 10, "torch callable (external path), sample_(st, 1) x 10")
