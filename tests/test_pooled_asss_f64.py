"""The pooled ASSS recurrence (include/amh.h "pooled ASSS") on the float64
restatement tests/pooled_asss_np.py alone, no GPU: it reduces to the
reference's recurrence with one chain, keeps the factor when Sigma' has no
Cholesky factor, and the GPU cases of tests/test_gpu_pooled_asss.py start where
a float32 evaluation follows the float64 slice path."""
import numpy as np
import pytest

import arwmh_np
import asss_np as lit
import pooled_asss_np as pa
import pooled_np as pnp


def _shared(d, L, mu, i):
    cov = L @ L.T
    return dict(i=np.array([i], np.int32), macc=np.array([0.5], np.float32), mu=mu, L=pnp.pack(L),
                lam=np.zeros(1, np.float32), asc=np.zeros(1, np.float32), cov=pnp.pack(cov))


@pytest.mark.parametrize("d,i", [(1, 1), (3, 1), (8, 4), (16, 30)])
def test_one_chain_is_the_reference_recurrence(d, i):
    """N = 1: chol((1 - gamma) L L^T + gamma delta delta^T) is
    cholesky_update(sqrt(1 - gamma) L, delta, gamma), asss.py:254, and mu', as_change
    are asss.py:252, 259-260."""
    rng = np.random.default_rng(d)
    A = rng.normal(size=(d, d))
    L = np.linalg.cholesky(A @ A.T + d * np.eye(d))
    mu, x = rng.normal(size=d), rng.normal(size=d) * 2
    delta = x - mu
    sums = pnp.pack_sums(delta, np.outer(delta, delta), 1.0, 1.0)
    up = pa.update(sums, _shared(d, L, mu, i))
    g = float(arwmh_np.lr_gamma(i + 1, float(np.float32(2 / 3))))
    assert up.gamma == g and up.refactored
    ref = arwmh_np.cholesky_update(np.sqrt(1.0 - g) * L, delta, g)
    np.testing.assert_allclose(up.L, ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max())
    np.testing.assert_allclose(up.mu, mu + g * delta, rtol=1e-15)
    assert up.asc == pytest.approx(np.linalg.norm(g * delta) + np.linalg.norm(ref - L, "fro"), rel=1e-12)
    assert up.i == i + 1 and up.macc == pytest.approx(0.5 + 0.5 / (i + 1))


def test_rank_deficient_first_block_keeps_the_factor():
    """gamma_1 = 1 with C < d chains: Sigma' = S_dd / N has rank C, so the
    factor and cov are kept and mu moves by the mean delta."""
    d, C = 16, 8
    rng = np.random.default_rng(0)
    delta = rng.normal(size=(C, d))
    sums = pnp.pack_sums(delta.sum(0), delta.T @ delta, float(C), float(C))
    sh = _shared(d, np.eye(d), np.zeros(d), 0)
    up = pa.update(sums, sh)
    assert up.gamma == 1.0 and not up.refactored
    assert np.array_equal(up.L, np.eye(d)) and np.array_equal(up.cov, np.eye(d))
    np.testing.assert_allclose(up.mu, delta.mean(0), rtol=1e-15)
    assert up.asc == pytest.approx(np.linalg.norm(delta.mean(0)))


def test_capped_shrinkage_does_not_count_as_moved():
    assert pa.moved(np.array([0, 3, lit.MAX_ITERATIONS - 1, lit.MAX_ITERATIONS])).tolist() == [1.0, 1.0, 1.0, 0.0]


@pytest.mark.parametrize("kind,d,C,K", pa.CASES)
def test_gpu_cases_follow_one_slice_path(kind, d, C, K, orc):
    """The condition the GPU comparison relies on, on the reference alone: from
    the warm start of each GPU case, the float32 evaluation of the literal and
    the float64 one take the same number of shrinkage rounds for all but at
    most max(1, C K // 50) chains, and no chain reaches the 50-round cap.  Each
    step starts both from the float64 trajectory rounded to float32, as the
    GPU comparison is teacher-forced on float32 states."""
    om, U, keys, z0, sh = pa.warm_case(kind, d, C, K)
    dd = om.d
    L = pnp.unpack(sh["L"], dd)
    x = np.asarray(z0, np.float32)
    differ = np.zeros(C, bool)
    for t in range(K):
        it = int(sh["i"][0]) + t
        x64, _, n64 = pa.step(U, it, x.astype(np.float64), keys, sh["mu"], L)
        _, _, n32 = pa.step(U, it, x, keys, sh["mu"], L, dtype=np.float32)
        assert n64.max() < lit.MAX_ITERATIONS and n32.max() < lit.MAX_ITERATIONS
        differ |= n64 != n32
        x = x64.astype(np.float32)
    print(f"{kind} d={dd}: {int(differ.sum())} of {C} chains on another slice path")
    assert differ.sum() <= max(1, C * K // 50)
