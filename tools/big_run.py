"""ARWMH sample() per launch at large d (regime A: per-chain adaptation; the
step pass chains the next proposal), correlated Gaussian with kappa = 1e4 as
BASELINE configs[3]: ms per launch over 100 launches after 50 warm-up
launches (HIP events).  Usage: python3 tools/big_run.py [C] [d] [nochain|pnx]
(nochain: every sample() runs the propose pass instead of taking the step
pass's next proposal; pnx: times sample_Pnx(n=8) over C chains, C / 64 points
of 64 samples each, with chain 0's adapt state after 20 transitions, instead:
big_pnx_kernel)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "adaptive-mcmc_amd"))
import torch  # noqa: E402

import posteriors as P  # noqa: E402
from kernels_amd import ARWMH, PRNGKey  # noqa: E402

C = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
d = int(sys.argv[2]) if len(sys.argv) > 2 else 256
k = ARWMH(potential_fn=P.correlated_gaussian(d, log10_kappa=4.0), num_chains=C)
k.chain_proposals = not (len(sys.argv) > 3 and sys.argv[3] == "nochain")
st = k.init(PRNGKey(0), 0, (torch.rand(C, d, device="cuda") * 4 - 2).contiguous(), (), {})
pnx = len(sys.argv) > 3 and sys.argv[3] == "pnx"
if pnx:
    for _ in range(20):
        st = k.sample(st, (), {})
    ad = st.adapt_state
    frozen = (ad.loc[0].clone(), ad.scale[0].clone(), ad.log_step_size[0].clone())
    x = st.z[:C // 64].clone()


def call():
    global st
    if pnx:
        k.sample_Pnx(PRNGKey(1), x, frozen, n=8, n_samples=64)
    else:
        st = k.sample(st, (), {})


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
    print(f"arwmh {lib} pnx C={C} d={d}: {ms:.4f} ms per sample_Pnx(n=8), {8 * C / ms * 1e3:.4g} chain-steps/s", flush=True)
    sys.exit(0)
print(f"arwmh {lib}{'' if k.chain_proposals else ' nochain'} C={C} d={d}: {ms:.4f} ms per sample(), {C / ms * 1e3:.4g} chain-steps/s", flush=True)
