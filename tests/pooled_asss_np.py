"""Float64 restatement of one pooled ASSS block (include/amh.h "pooled ASSS").

TEST INFRASTRUCTURE ONLY (never imported by the product package).

A block is built from the literal asss_np.sample per chain-step with the
shared (loc, scale) as its adapt state: only x', pe' and the shrinkage's
round count are taken from it (its per-chain adaptation is discarded).  The
sums and the layout helpers are oracle/pooled_np.py's; the update is the
pooled one without a step size:

    n = block count, gamma = n^-a
    mu'  = mu + gamma S_d / N
    Sig' = (1 - gamma) Sig + gamma S_dd / N,  L' = chol(Sig') or keep (L, Sig)
    macc' = macc + (S_a / N - macc) / n,  lam copied through
    as_change = ||mu' - mu||_2 + ||L' - L||_F,  i' = i + K
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import arwmh_np
import asss_np as lit
import pooled_np as pnp

# the GPU cases of tests/test_gpu_pooled_asss.py: (kind, d, C, K)
CASES = [("gaussian", 7, 517, 1), ("gaussian", 7, 517, 4), ("eight_schools", None, 70, 1),
         ("gaussian", 33, 300, 1), ("gaussian", 64, 300, 2), ("gaussian", 1, 65, 1), ("gaussian", 2, 40, 1)]
SEED = 7


def potential(kind, om):
    """The float64 potential of one point (tests/test_oracle.py lit_potential)."""
    from test_oracle import lit_potential
    return lit_potential(kind, om)


def step(U, it, x, keys, mu, L, eps=1e-6, dtype=np.float64):
    """One frozen transition of every chain at stream position `it`:
    asss_np.sample with the shared (mu, L [d, d]) -> (x' [C, d], pe' [C],
    n_iter [C]) in `dtype`."""
    x = np.asarray(x)
    C, d = x.shape
    xo, po, ni = np.empty((C, d), dtype), np.empty(C, dtype), np.empty(C, np.int64)
    adapt = lit.ASSSAdaptState(np.asarray(mu, dtype), np.asarray(L, dtype))
    for c in range(C):
        v, ut, th0, uks = lit.draws(keys[c], int(it), d)
        new, n = lit.sample(lit.ASSSState(int(it), x[c], None, adapt, 0.0, None), U, v, ut, th0, uks, eps=eps,
                            dtype=dtype)
        xo[c], po[c], ni[c] = new.z, new.potential_energy, n
    return xo, po, ni


def moved(n_iter):
    """a of the sums: 0 where the shrinkage reached its cap (theta = 0)."""
    return (np.asarray(n_iter) < lit.MAX_ITERATIONS).astype(np.float64)


def block(U, i, z, keys, mu, L, K=1, eps=1e-6):
    """K frozen transitions of every chain and the block's float64 sums."""
    d = np.asarray(z).shape[1]
    Lm = pnp.unpack(L, d) if np.asarray(L).ndim == 1 else np.asarray(L, np.float64)
    zs, S_a, pe = [np.asarray(z, np.float64)], 0.0, None
    for t in range(K):
        x, pe, ni = step(U, int(i) + t, zs[-1], keys, mu, Lm, eps)
        zs.append(x)
        S_a += float(moved(ni).sum())
    zs = np.stack(zs)
    S_d, S_dd, _, _ = pnp.sums_of(zs[1:], mu)
    return SimpleNamespace(zs=zs, pe=pe, sums=pnp.pack_sums(S_d, S_dd, S_a, float(K * zs.shape[1])))


def update(sums, shared, K=1, num_warmup=0, lr_decay=2 / 3, gamma=None):
    """The shared-state update from a sums vector, in float64 (`shared` in the
    layout of orc.pooled_init_shared, not modified)."""
    d = np.asarray(shared["mu"]).shape[0]
    i = int(np.asarray(shared["i"]).reshape(-1)[0])
    S_d, S_dd, S_a, N = pnp.split_sums(sums, d)
    n = pnp.block_n(i, K, int(num_warmup))
    g = float(arwmh_np.lr_gamma(n, float(np.float32(lr_decay)))) if gamma is None else float(gamma)
    mu0 = np.asarray(shared["mu"], np.float64)
    macc0 = float(np.asarray(shared["macc"]).reshape(-1)[0])
    L0, cov0 = pnp.unpack(shared["L"], d), pnp.unpack_sym(shared["cov"], d)
    mu = mu0 + g * S_d / N
    cov = (1.0 - g) * cov0 + g * S_dd / N
    try:
        with np.errstate(all="ignore"):
            L = np.linalg.cholesky(cov)
        ok = bool(np.all(np.isfinite(L)))
    except np.linalg.LinAlgError:
        ok = False
    ratio = 0.0
    if ok:
        piv = np.diagonal(L) ** 2
        ratio = float(piv.min() / piv.max())
    else:
        L = L0
    abar = S_a / N
    macc = macc0 + (abar - macc0) / n
    asc = float(np.linalg.norm(mu - mu0) + np.linalg.norm(L - L0, "fro"))
    return SimpleNamespace(n=n, gamma=g, mu=mu, cov=cov if ok else cov0, cov_new=cov, L=L, refactored=ok,
                           pivot_ratio=ratio, macc=macc, asc=asc, i=i + K,
                           terms=dict(mu=np.abs(mu0) + g * np.abs(S_d / N),
                                      macc=abs(macc0) + (abs(abar) + abs(macc0)) / n))


def as_change_bound(mu1, mu0, L1, L0, ref, d):
    """|as_change - ref| <= u (|| |L'| + |L| ||_F + || |mu'| + |mu| ||_2) +
    gamma_{P+2} ref, u = 2^-24, ref the float64 value of the float32 leaves.
    Each entry fl(L'_rk - L_rk) is one rounded difference, off by at most u
    |L'_rk - L_rk| <= u (|L'_rk| + |L_rk|), so the norm moves by at most u
    || |L'| + |L| ||_F (triangle inequality); likewise the d differences of mu.
    The float32 sum of the P = d (d + 1) / 2 squares and its root add gamma_{P+1}
    relative to the factor's norm (the d squares of mu fewer), and the final
    add of the two norms one more rounding: gamma_{P+2} ref covers both."""
    P = d * (d + 1) // 2
    m = float(np.linalg.norm(np.ravel(np.abs(L1) + np.abs(L0))) + np.linalg.norm(np.abs(mu1) + np.abs(mu0)))
    return pnp.U32 * m + float(pnp.gam(P + 2)) * ref


def lane_sum_bound(A, d, C, K):
    """bounds.S_d / S_dd of oracle/pooled_np.py with the lane-per-row form's
    own float32 chain at every d <= 64 (pooled ASSS keeps that form at d = 64,
    where the ARWMH bound describes the MFMA kernel): a wave's cpw K
    chain-steps and the 4-level tree, then the double adds over the chunks of
    16 cpw chains in groups of 16 and the groups."""
    cpw = min(16, max(1, -(-C // 4096)))
    chunks = -(-C // (16 * cpw))
    return (pnp.gam(cpw * K + 4 + 3) + pnp.gam(16 + -(-chunks // 16), pnp.U64)) * A


def warm_case(kind, d, C, K):
    """-> (om, U, keys, z0 float32, shared): the warm start of a GPU case
    (helpers.pooled_warm_start) with its float64 potential and chain keys."""
    from helpers import make_case, pooled_warm_start
    from kernels_amd import PRNGKey
    _, _, om = make_case(kind, d)
    z0, sh = pooled_warm_start(kind, d, C, SEED, K)
    keys = arwmh_np.chain_keys(PRNGKey(SEED), 0, C)
    return om, potential(kind, om), keys, z0, sh
