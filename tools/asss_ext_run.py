"""ASSS with the caller's potential (host_shrink=True): shrink rounds and time
per transition, beside the ARWMH external path at the same shape.  Two shapes:
the 3-D Gaussian written in torch at C = 4096, and the library's Gaussian
potential (amh_potential) as the callable at d = 64, C = 512.  Per shape: 100
warm-up transitions, then N single transitions timed as one window (HIP
events) with shrink_rounds read after each; the mean and maximum of the rounds
and us per transition.  Usage: python3 tools/asss_ext_run.py [N]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "adaptive-mcmc_amd"))
import torch  # noqa: E402

import posteriors as P  # noqa: E402
from kernels_amd import ARWMH, ASSS, PRNGKey  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 300


def timed(step, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def shape(name, U, C, d):
    z0 = (torch.rand(C, d, device="cuda") * 4 - 2).contiguous()
    ks = ASSS(potential_fn=U, num_chains=C, host_shrink=True)
    st = ks.init(PRNGKey(0), 0, z0, (), {})
    ks.sample_(st, 100)
    rounds = []

    def step():
        ks.sample_(st, 1)
        rounds.append(ks.shrink_rounds)

    reps = [timed(step, N) for _ in range(3)]
    r = torch.tensor(rounds, dtype=torch.float64)
    kw = ARWMH(potential_fn=U, num_chains=C)
    sw = kw.init(PRNGKey(0), 0, z0, (), {})
    kw.sample_(sw, 100)
    wreps = [timed(lambda: kw.sample_(sw, 1), N) for _ in range(3)]
    print(f"{name} C={C} d={d}: ASSS host_shrink rounds mean {r.mean():.2f} max {int(r.max())}, "
          f"us per transition {sorted(reps)[1]:.1f} (min {min(reps):.1f} max {max(reps):.1f}); "
          f"ARWMH external us per transition {sorted(wreps)[1]:.1f} (min {min(wreps):.1f} max {max(wreps):.1f})",
          flush=True)


S = torch.tensor([[1.0, 0.5, 0.0], [0.5, 2.0, -0.3], [0.0, -0.3, 0.5]], dtype=torch.float64)
Pm = torch.linalg.inv(S).to(torch.float32).cuda()
m = torch.tensor([1.0, -2.0, 0.5], device="cuda")


def U3(z):
    x = z - m
    return 0.5 * ((x @ Pm) * x).sum(-1)


shape("torch 3-D Gaussian", U3, 4096, 3)
kg = ARWMH(potential_fn=P.correlated_gaussian(64), num_chains=8)
kg.init(PRNGKey(1), 0, torch.zeros(8, 64), (), {})
shape("library Gaussian", lambda z: kg.potential(z), 512, 64)
