"""The pooled mode against a float64 restatement at many chains, on the CPU.

oracle/pooled_np.py restates a pooled block from its formulas (no chunks,
waves or accumulation orders).  Here the C oracle (orc_pooled_*), which the
GPU suite compares the kernels with bit for bit, is held to it from a warm
start in the typical set, where a fair share of the proposals is accepted at
every d; tests/test_gpu_pooled_f64.py holds the kernels themselves to it over
the same matrix.  Every tolerance is a documented bound of pooled_np.bounds,
and the last test perturbs the reference in six ways that a shared
misreading of kernel and mirror could take, each of which the bounds must
reject."""
import numpy as np
import pytest

from helpers import (OraclePooled, make_case, pooled_f64_blocks, pooled_ref_model, pooled_reference_shares,
                     pooled_warm_start)

# (kind, d, C, K, W): the matrix of tests/test_gpu_pooled_f64.py.  W = 21 with
# i = 20 at the start makes the second block the warmup reset (gamma = 1).
MATRIX = [("gaussian", 7, 517, 1, 0), ("gaussian", 7, 517, 4, 0), ("eight_schools", None, 70, 1, 0),
          ("gaussian", 64, 300, 1, 0), ("gaussian", 64, 300, 4, 0), ("gaussian", 64, 300, 1, 21),
          ("gaussian", 96, 257, 1, 0), ("gaussian", 128, 300, 1, 0), ("gaussian", 128, 300, 3, 0),
          ("gaussian", 256, 257, 1, 0), ("gaussian", 40, 300, 1, 0)]
SHARE = (0.10, 0.50)


def setup_case(kind, d, C, K, W, seed=7):
    """-> (om, model, keys, z0, shared) after asserting, on the float64
    reference alone, that every block of the run accepts a share of its
    proposals within SHARE."""
    import arwmh_np as lit
    from kernels_amd import PRNGKey
    _, _, om = make_case(kind, d)
    model = pooled_ref_model(kind, om)
    z0, sh = pooled_warm_start(kind, d, C, seed, K)
    keys = lit.chain_keys(PRNGKey(seed), 0, C)
    shares = pooled_reference_shares(model, keys, z0, sh, K, W, 3)
    print("reference accepted share per block:", " ".join(f"{s:.3f}" for s in shares))
    assert all(SHARE[0] <= s <= SHARE[1] for s in shares), shares
    return om, model, keys, z0, sh


@pytest.mark.parametrize("kind,d,C,K,W", MATRIX)
def test_oracle_against_float64(kind, d, C, K, W, orc):
    """Three blocks of the oracle from the warm start: per-chain state, sums
    (teacher-forced on the z it wrote) and the update (teacher-forced on its
    own sums) within the bounds of pooled_np.bounds."""
    om, model, keys, z0, sh = setup_case(kind, d, C, K, W)
    impl = OraclePooled(orc, kind, d, C, K, W, 7, z0, sh)
    assert np.array_equal(impl.keys, keys)
    pooled_f64_blocks(impl, model, keys, K, W)


# ------------------------------------------------- the checker checks itself --
def _reference_block(model, keys, z0, sh, K, W, d):
    """One block of the reference in the checker's input form: the float64
    outputs rounded to the formats an implementation holds."""
    import pooled_np as pnp
    s = pnp.stats(model.U, int(sh["i"][0]), z0, None, keys, sh["mu"], sh["L"], float(sh["lam"][0]), K=K)
    zs = s.zs.astype(np.float32)
    # the sums of the rounded history, so the unperturbed reference sits at error 0
    S_d, S_dd, _, _ = pnp.sums_of(zs[1:], sh["mu"])
    sums = pnp.pack_sums(S_d, S_dd, s.S_a, s.N)
    return s, zs, s.pe.astype(np.float32), sums


def _after(sums, sh, K, W, n=None):
    """The reference's update with gamma rounded to float32 (as every
    implementation holds it), the result rounded to the leaves' formats."""
    import arwmh_np as lit
    import pooled_np as pnp
    n = pnp.block_n(int(sh["i"][0]), K, W) if n is None else n
    g = float(np.float32(lit.lr_gamma(n, float(np.float32(2 / 3)))))
    up = pnp.update(sums, sh, K=K, num_warmup=W, gamma=g, n=n)
    return dict(i=np.array([up.i], np.int32), macc=np.array([up.macc], np.float32), mu=up.mu.astype(np.float32),
                L=pnp.pack(up.L).astype(np.float32), lam=np.array([up.lam], np.float32),
                asc=np.array([up.asc], np.float32), cov=pnp.pack(up.cov))


@pytest.mark.parametrize("d,C,K", [(64, 300, 1), (64, 300, 4), (128, 300, 3)])
def test_checker_rejects_shared_misreadings(d, C, K):
    """The reference's own block passes its checker; each of six misreadings
    applied to the reference's outputs is rejected, on the quantity it
    corrupts.  A tolerance that let one through would be too wide."""
    import pooled_np as pnp
    W = 0
    om, model, keys, z0, sh = setup_case("gaussian", d, C, K, W)
    s, zs, pe, sums = _reference_block(model, keys, z0, sh, K, W, d)
    P = pnp.packed_size(d)

    def check(sums_, after=None):
        return pnp.check_block(model, keys, sh, zs, pe, sums_, _after(sums_, sh, K, W) if after is None else after,
                               K=K, num_warmup=W)

    clean = check(sums)
    print("clean:", clean)
    assert not pnp.worst(clean) and clean["skipped"] <= max(2, C / 100)
    mu = np.asarray(sh["mu"], np.float64)
    # (a) the last chain dropped from the sums
    S_d, S_dd, _, _ = pnp.sums_of(zs[1:, :-1], mu)
    r = check(pnp.pack_sums(S_d, S_dd, s.S_a - s.alpha[:, -1].sum(), s.N))
    # (S_a's bound carries the float32 potential's worst case, about 1 % of S_a
    # at d = 64: one chain's alpha can hide in it, the outer products cannot)
    assert r["S_dd"] > 1 and r["S_d"] > 1, r
    # (b) N off by one, either way
    for dn in (-1, 1):
        bad = sums.copy()
        bad[-1] += dn
        assert check(bad)["N"] > 1
    # (c) delta against the updated mean
    mu1 = pnp.update(sums, sh, K=K, num_warmup=W).mu
    S_d, S_dd, _, _ = pnp.sums_of(zs[1:], mu1)
    r = check(pnp.pack_sums(S_d, S_dd, s.S_a, s.N))
    assert r["S_dd"] > 1 and r["S_d"] > 1, r
    # (d) S_a from the accept decisions
    bad = sums.copy()
    bad[d + P] = float(s.accept.sum())
    r = check(bad)
    print(f"(d) |sum accept - sum alpha| / bound = {r['S_a']:.3g}")
    # The S_a bound is the worst case of the float32 potential, linear in the
    # chain-steps: 0.3 % of N at d = 64, but 1.8 % of N at d = 128 (|c0| = 118
    # and 1/2 |y|^T |P| |y| = 2270 against U - c0 = 64).  Decisions and alpha
    # differ by a binomial spread sqrt(sum alpha (1 - alpha)) = 0.35 sqrt(N),
    # which at d = 128, N = 900 (10) is inside that bound (16; measured ratio
    # 0.48): there S_a is pinned to 1.8 % only and this misreading is not
    # separable by it.  Up to d = 64 it is, and must be rejected.
    if d <= 64:
        assert r["S_a"] > 1
    # (e) gamma counted per step in a K-block
    if K > 1:
        i0 = int(sh["i"][0])
        r = check(sums, after=_after(sums, sh, K, W, n=i0 + 1))
        assert r["mu"] > 1 and r["cov"] > 1 and r["lam"] > 1, r
    # (f) two packed S_dd entries swapped across the 32-column tile boundary
    bad = sums.copy()
    row = d - 1
    a = d + sum(d - j for j in range(31)) + (row - 31)  # (row, 31)
    b = d + sum(d - j for j in range(32)) + (row - 32)  # (row, 32)
    bad[a], bad[b] = bad[b], bad[a]
    assert check(bad)["S_dd"] > 1


def test_update_matches_the_d6_formula_check(orc):
    """pooled_np.update against the oracle where tests/test_pooled.py pins the
    oracle to the formula (d = 6, K = 4, W = 8): the two references agree."""
    import pooled_np as pnp
    from kernels_amd import PRNGKey
    K, W, C = 4, 8, 50
    _, _, om = make_case("gaussian", 6)
    st = orc.init(om, PRNGKey(1), C)
    z, pe, keys = st.z, st.potential_energy, st.rng_key
    sh = orc.pooled_init_shared(6)
    for _ in range(4):
        z, pe, sums = orc.pooled_stats(om, int(sh["i"][0]), z, pe, keys, sh["mu"], sh["L"], float(sh["lam"][0]),
                                       k_steps=K)
        before = {k: v.copy() for k, v in sh.items()}
        orc.pooled_update(om, sums, sh, num_warmup=W, k_steps=K)
        g = float(orc.lr_gamma([pnp.block_n(int(before["i"][0]), K, W)], 2 / 3)[0])
        up = pnp.update(sums, before, K=K, num_warmup=W, gamma=g)
        np.testing.assert_allclose(sh["cov"], pnp.pack(up.cov), rtol=pnp.COV_RTOL)
        assert up.i == int(sh["i"][0])
