"""ASSS sample() per launch (out of place, one transition per call) at the
d = 64 Gaussian, 65,536 chains: ms per launch over 100 launches after 50
warm-up launches (HIP events).  Usage: python3 tools/asss_run.py [C] [d] [pnx]
(pnx: times sample_Pnx(n=8) over C chains, C / 64 points of 64 samples each,
with chain 0's adapt state after 20 transitions, instead: the frozen kernel)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "adaptive-mcmc_amd"))
import torch  # noqa: E402

import posteriors as P  # noqa: E402
from kernels_amd import ASSS, PRNGKey  # noqa: E402

C = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
d = int(sys.argv[2]) if len(sys.argv) > 2 else 64
k = ASSS(potential_fn=P.correlated_gaussian(d), num_chains=C)
st = k.init(PRNGKey(0), 0, (torch.rand(C, d, device="cuda") * 4 - 2).contiguous(), (), {})
pnx = len(sys.argv) > 3 and sys.argv[3] == "pnx"
if pnx:
    for _ in range(20):
        st = k.sample(st)
    frozen = (st.adapt_state.loc[0].clone(), st.adapt_state.scale[0].clone())
    x = st.z[:C // 64].clone()


def call():
    global st
    if pnx:
        k.sample_Pnx(PRNGKey(1), x, frozen, n=8, n_samples=64)
    else:
        st = k.sample(st)


for _ in range(50):
    call()
torch.cuda.synchronize()
a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
a.record()
for _ in range(100):
    call()
b.record()
torch.cuda.synchronize()
ms = a.elapsed_time(b) / 100
lib = os.path.basename(os.path.dirname(os.environ.get("AMH_LIB_PATH", "release/x")))
if pnx:
    print(f"asss {lib} pnx C={C} d={d}: {ms:.4f} ms per sample_Pnx(n=8), {8 * C / ms * 1e3:.4g} chain-steps/s", flush=True)
    sys.exit(0)
print(f"asss {lib} C={C} d={d}: {ms:.4f} ms per sample(), {C / ms * 1e3:.4g} chain-steps/s", flush=True)
