"""The fused ASSS legs, for comparing two builds of libamh.so (AMH_LIB_PATH
selects the library; run the builds alternately on one box): ms per launch of
  asss64     ASSS.sample at the d = 64 Gaussian, 65,536 chains (one transition)
  fused_es   ASSS.sample_(st, 20) at eight schools, 262,144 chains
  fused_g32  ASSS.sample_(st, 20) at the d = 32 Gaussian, 65,536 chains
each as the median, minimum and maximum of 5 windows of 20 launches after a
warm-up of 20 launches (HIP events).  Usage: python3 tools/asss_ab.py [LABEL]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "adaptive-mcmc_amd"))
import torch  # noqa: E402

import posteriors as P  # noqa: E402
from kernels_amd import ASSS, PRNGKey  # noqa: E402

label = sys.argv[1] if len(sys.argv) > 1 else "release"


def windows(launch, n=20, reps=5):
    for _ in range(n):
        launch()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            launch()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / n)
    return sorted(out)


def leg(name, k, st, n_steps):
    box = [st]

    def launch():
        if n_steps == 1:
            box[0] = k.sample(box[0])
        else:
            k.sample_(box[0], n_steps)

    w = windows(launch)
    print(f"{label} {name}: {w[len(w) // 2]:.4f} ms per launch (min {w[0]:.4f} max {w[-1]:.4f})", flush=True)


C = 65536
k = ASSS(potential_fn=P.correlated_gaussian(64), num_chains=C)
leg("asss64", k, k.init(PRNGKey(0), 0, (torch.rand(C, 64, device="cuda") * 4 - 2).contiguous(), (), {}), 1)
k = ASSS(model=P.eight_schools, num_chains=262144)
leg("fused_es", k, k.init(PRNGKey(0), 0, None, (), dict(P.EIGHT_SCHOOLS_DATA)), 20)
k = ASSS(potential_fn=P.correlated_gaussian(32), num_chains=C)
leg("fused_g32", k, k.init(PRNGKey(0), 0, (torch.rand(C, 32, device="cuda") * 4 - 2).contiguous(), (), {}), 20)
