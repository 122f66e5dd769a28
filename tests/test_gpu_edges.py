"""GPU parity at non-finite and extreme states: the HIP transition kernels
against the C oracle where the select-based kernels and the branchy C mirror
could drift apart (fmaxf / min NaN ordering, inf - inf, 0 * inf, group votes
against per-chain ifs, casts of out-of-range floats).  Scenarios and the
NaN-aware comparison are in tests/helpers.py; tests/test_edges.py shows on the
CPU that the scenarios reach the edges and that the oracle is right there.

Read before the first run (amh_kernels.hip, amh_step64.hip, amh_split.hip, amh_big.hip,
amh_asss.h, amh_pooled.hip, amh_big_pooled.hip, amh_device.h, amh_math.h): no
memory index, trip count or launch dimension derives from a float state value
-- lookup_gamma indexes by the integer step number, the ASSS shrink loops end
at kAsssMaxIter whatever the potentials are, amh_expf clamps before its (int),
amh_logf takes its exponent from the bit pattern, the ASSS angle is built from
uniforms alone (|theta| < 2 pi, so amh_sincosf's quadrant cast is in range),
and every other cast or loop bound comes from thread indices, d, C or N."""
import numpy as np
import pytest
import torch

from helpers import (ASSS_FIELDS, EDGE_MATRIX, HOSTILE_WARMUP, assert_bitequal_nan, assert_state_bitequal_nan,
                     edge_init, edge_points, hostile_adapt, log_scale_coords, make_case, make_edge_case)

pytestmark = pytest.mark.gpu

C = 160
ASSS_MATRIX = [("gaussian", 1), ("gaussian", 5), ("gaussian", 64), ("gaussian", 100), ("gaussian", 256),
               ("eight_schools", None), ("kidiq", None), ("diamonds", None), ("mixture", 3),
               ("logistic", 8), ("logistic", 32), ("poisson", 9), ("poisson", 32)]


def _start(cls, kind, d, orc, start, num_warmup, seed=0):
    """Product kernel + state and the oracle's, from the same flat start."""
    from kernels_amd import PRNGKey
    kw, mk, om, ost, z0 = edge_init(kind, d, C, orc, seed=seed, start=start)
    k = cls(num_chains=C, **kw)
    st = k.init(PRNGKey(seed), num_warmup, torch.from_numpy(z0.copy()), (), mk)
    torch.cuda.synchronize()
    return k, st, om, ost, z0


def _stuck_stay(st, ost, z0, stuck):
    """Chains whose initial potential is NaN or -inf never accept: still at their start."""
    if stuck.any():
        assert_bitequal_nan(ost.z[stuck], z0[stuck], "oracle: stuck chains left their start")
        assert_bitequal_nan(st.z.cpu().numpy()[stuck], z0[stuck], "gpu: stuck chains left their start")


# ------------------------------------------------------------- potential ----
@pytest.mark.parametrize("kind,d", EDGE_MATRIX)
def test_potential_edges(kind, d, gpu, orc):
    from kernels_amd import ARWMH, PRNGKey
    kw, mk, om = make_edge_case(kind, d)
    k = ARWMH(num_chains=8, **kw)
    k.init(PRNGKey(0), 0, torch.zeros(8, om.d), (), mk)
    zt, z = edge_points(om.d, 11, log_scale_coords(kind.replace("_n77", ""), om.d))
    pe = k.potential(zt.to(gpu))
    assert_bitequal_nan(pe, orc.potential(om, z), f"{kind} d={om.d} potential at edge points")


# ----------------------------------------------------------------- ARWMH ----
@pytest.mark.parametrize("kind,d", EDGE_MATRIX)
def test_arwmh_wild_starts(kind, d, gpu, orc):
    """Starts N(0, 1) * 10^k, k in [-3, 20]: init, 40 single steps compared
    after each, accept_count, then one fused run with thinned z / pe.  Chains
    whose initial potential is NaN carry NaN mean_accept_prob / log_step_size
    for ever; with NaN or -inf they stay at their start on both sides (a +inf
    start accepts the first finite proposal, as arwmh.py:173-178 does)."""
    from kernels_amd import ARWMH
    k, st, om, ost, z0 = _start(ARWMH, kind, d, orc, "wild", 5)
    assert_state_bitequal_nan(st, ost, f"{kind} wild init")
    # exp(pe0 - pe') is NaN or 0 for every proposal: never accepted (a +inf start accepts any finite proposal)
    stuck = np.isnan(ost.potential_energy) | np.isneginf(ost.potential_energy)
    acc = np.zeros(C, np.int32)
    for t in range(40):
        st = k.sample(st, (), {})
        orc.step(om, ost, 1, num_warmup=5, accept_count=acc)
        torch.cuda.synchronize()
        assert_state_bitequal_nan(st, ost, f"{kind} wild step {t}")
    st, cz, cp = k.run(st, 20, thinning=2, collect_z=True, collect_pe=True)
    ocz = orc.step(om, ost, 20, num_warmup=5, accept_count=acc, collect_z=True)[1::2]
    torch.cuda.synchronize()
    assert_state_bitequal_nan(st, ost, f"{kind} wild run")
    assert_bitequal_nan(cz, ocz, f"{kind} wild collected z")
    ocp = orc.potential(om, ocz.reshape(-1, om.d)).reshape(ocz.shape[:2])
    assert_bitequal_nan(cp, ocp, f"{kind} wild collected pe")
    np.testing.assert_array_equal(k.accept_count.cpu().numpy(), acc)
    assert not acc[stuck].any()
    _stuck_stay(st, ost, z0, stuck)


@pytest.mark.parametrize("kind,d", EDGE_MATRIX)
def test_arwmh_hostile_adapt(kind, d, gpu, orc):
    """5 benign steps, hostile_adapt on both sides, then single steps compared
    after each and one fused run with collection (12 + 8 steps; 6 + 4 at
    d > 64): the keep-L vote, inf passing it, e^lambda at both clamps, the
    warmup reset from hostile values."""
    from kernels_amd import ARWMH
    W = HOSTILE_WARMUP
    k, st, om, ost, _ = _start(ARWMH, kind, d, orc, "uniform", W)
    n1, n2 = (6, 4) if om.d > 64 else (12, 8)
    acc = np.zeros(C, np.int32)
    k.sample_(st, 5)
    orc.step(om, ost, 5, num_warmup=W, accept_count=acc)
    assert_state_bitequal_nan(st, ost, f"{kind} benign steps")
    hostile_adapt(st)
    hostile_adapt(ost)
    assert_state_bitequal_nan(st, ost, f"{kind} after hostile_adapt")
    for t in range(n1):
        st = k.sample(st, (), {})
        orc.step(om, ost, 1, num_warmup=W, accept_count=acc)
        torch.cuda.synchronize()
        assert_state_bitequal_nan(st, ost, f"{kind} hostile step {t}")
    st, cz, cp = k.run(st, n2, thinning=1, collect_z=True, collect_pe=True)
    ocz = orc.step(om, ost, n2, num_warmup=W, accept_count=acc, collect_z=True)
    torch.cuda.synchronize()
    assert_state_bitequal_nan(st, ost, f"{kind} hostile run")
    assert_bitequal_nan(cz, ocz, f"{kind} hostile collected z")
    # every collected row: a chain's pe is the potential of the z it holds
    ocp = orc.potential(om, ocz.reshape(-1, om.d)).reshape(ocz.shape[:2])
    assert_bitequal_nan(ocp[-1], ost.potential_energy, f"{kind} oracle: carried pe is the potential of z")
    assert_bitequal_nan(cp, ocp, f"{kind} hostile collected pe")
    np.testing.assert_array_equal(k.accept_count.cpu().numpy(), acc)


# ------------------------------------------------------------------ ASSS ----
@pytest.mark.parametrize("kind,d", ASSS_MATRIX)
def test_asss_wild_starts(kind, d, gpu, orc):
    """ASSS.sample x 25, ASSS.run (thinned z / pe) and ASSS.sample_ from the
    wild starts."""
    from kernels_amd import ASSS
    k, st, om, ost, z0 = _start(ASSS, kind, d, orc, "wild", 5)
    assert_state_bitequal_nan(st, ost, f"{kind} wild init", ASSS_FIELDS)
    for t in range(25):
        st = k.sample(st, (), {})
        orc.asss_step(om, ost, 1, num_warmup=5)
        torch.cuda.synchronize()
        assert_state_bitequal_nan(st, ost, f"{kind} asss wild step {t}", ASSS_FIELDS)
    st, cz, cp = k.run(st, 6, thinning=2, collect_z=True, collect_pe=True)
    ocz, ocp = orc.asss_step(om, ost, 6, num_warmup=5, collect_z=True, collect_pe=True)
    torch.cuda.synchronize()
    assert_state_bitequal_nan(st, ost, f"{kind} asss wild run", ASSS_FIELDS)
    assert_bitequal_nan(cz, ocz[1::2], f"{kind} asss wild collected z")
    assert_bitequal_nan(cp, ocp[1::2], f"{kind} asss wild collected pe")
    k.sample_(st, 3)
    orc.asss_step(om, ost, 3, num_warmup=5)
    torch.cuda.synchronize()
    assert_state_bitequal_nan(st, ost, f"{kind} asss wild in place", ASSS_FIELDS)


@pytest.mark.parametrize("kind,d", ASSS_MATRIX)
def test_asss_hostile_adapt(kind, d, gpu, orc):
    """hostile_adapt without the step-size leaf, 12 single ASSS steps, a fused
    run with collection and in-place steps: the degen / capped fallbacks, z
    leaving the finite range under a 1e19-scale factor, the keep-L vote."""
    from kernels_amd import ASSS
    W = HOSTILE_WARMUP
    k, st, om, ost, _ = _start(ASSS, kind, d, orc, "uniform", W)
    k.sample_(st, 5)
    orc.asss_step(om, ost, 5, num_warmup=W)
    assert_state_bitequal_nan(st, ost, f"{kind} asss benign steps", ASSS_FIELDS)
    hostile_adapt(st, step_size=False)
    hostile_adapt(ost, step_size=False)
    for t in range(12):
        st = k.sample(st, (), {})
        orc.asss_step(om, ost, 1, num_warmup=W)
        torch.cuda.synchronize()
        assert_state_bitequal_nan(st, ost, f"{kind} asss hostile step {t}", ASSS_FIELDS)
    st, cz, cp = k.run(st, 4, thinning=2, collect_z=True, collect_pe=True)
    ocz, ocp = orc.asss_step(om, ost, 4, num_warmup=W, collect_z=True, collect_pe=True)
    torch.cuda.synchronize()
    assert_state_bitequal_nan(st, ost, f"{kind} asss hostile run", ASSS_FIELDS)
    assert_bitequal_nan(cz, ocz[1::2], f"{kind} asss hostile collected z")
    assert_bitequal_nan(cp, ocp[1::2], f"{kind} asss hostile collected pe")
    k.sample_(st, 2)
    orc.asss_step(om, ost, 2, num_warmup=W)
    torch.cuda.synchronize()
    assert_state_bitequal_nan(st, ost, f"{kind} asss hostile in place", ASSS_FIELDS)


# -------------------------------------------------------- frozen kernels ----
def _theta_chains():
    """Eight hostile_adapt chains, one per step-size value (c % 8 = j) and one
    per factor scale; the odd ones from the upper half (loc at 1e19)."""
    return [9 * j if j % 2 == 0 else 80 + 9 * j for j in range(8)]


@pytest.mark.parametrize("d", [16, 128])
@pytest.mark.parametrize("algo", ["arwmh", "asss"])
def test_frozen_kernels_hostile_theta(algo, d, gpu, orc):
    """sample_Pnx with theta from hostile_adapt chains, three start points
    (one at 1e19), n = 4, n_samples = 16."""
    from kernels_amd import ARWMH, ASSS, PRNGKey
    cls = ASSS if algo == "asss" else ARWMH
    k, st, om, ost, _ = _start(cls, "gaussian", d, orc, "uniform", HOSTILE_WARMUP)
    k.sample_(st, 5)
    hostile_adapt(st, step_size=algo == "arwmh")
    torch.cuda.synchronize()
    x = np.random.default_rng(5).normal(size=(3, d)).astype(np.float32)
    x[2] = np.float32(1e19)
    a = st.adapt_state
    for c in _theta_chains():
        loc, scale = a.loc[c].clone(), a.scale[c].clone()
        if algo == "asss":
            out = k.sample_Pnx(PRNGKey(9), x, (loc, scale), n=4, n_samples=16)
            ref = orc.asss_sample_pnx(om, PRNGKey(9), x, loc.cpu().numpy(), scale.cpu().numpy(), 4, 16)
        else:
            lam = a.log_step_size[c].clone()
            out = k.sample_Pnx(PRNGKey(9), x, (loc, scale, lam), n=4, n_samples=16)
            ref = orc.sample_pnx(om, PRNGKey(9), x, loc.cpu().numpy(), scale.cpu().numpy(), float(lam.cpu()), 4, 16)
        assert out.shape == (3, 16, d)
        assert_bitequal_nan(out, ref, f"{algo} d={d} sample_Pnx, theta of chain {c}")


# ---------------------------------------------------------------- pooled ----
OUTLIERS = (5, 64, 65, 130, 255, 299)


def _pooled_hostile_z0(Cn, d, case):
    """"nan-sums": six chains at +-1e19 in every coordinate (their potential
    is NaN), one z[0] = inf, one z[3] = nan.  "outlier-1": the six chains at
    +-1e19 in coordinate 0 only (potential ~1e38, every sum finite, a factor
    of scale 1e18).  "outlier-2": in coordinates 3 and 40 (potential +inf, so
    only S_a is NaN; the finite S_dd is numerically singular in those two
    coordinates and the first refactorisation fails amh_pivot_ok)."""
    z0 = np.random.default_rng(3).uniform(-2, 2, size=(Cn, d)).astype(np.float32)
    coords = {"nan-sums": slice(None), "outlier-1": [0], "outlier-2": [3, 40]}[case]
    for j, c in enumerate(OUTLIERS):
        z0[c, coords] = np.float32(1e19 if j % 2 == 0 else -1e19)
    if case == "nan-sums":
        z0[17, 0] = np.inf
        z0[201, 3] = np.nan
    return z0


def _pooled_compare(k, st, z, pe, sums, sh, what):
    assert_bitequal_nan(k._sums, sums, f"{what}: sums")
    got = dict(z=st.z, pe=st.potential_energy, mu=st.adapt_state.loc, L=st.adapt_state.scale,
               lam=st.adapt_state.log_step_size, macc=st.mean_accept_prob, asc=st.as_change, cov=st.cov, i=st.i)
    want = dict(z=z, pe=pe, mu=sh["mu"], L=sh["L"], lam=sh["lam"], macc=sh["macc"], asc=sh["asc"], cov=sh["cov"],
                i=sh["i"])
    for f in got:
        assert_bitequal_nan(got[f], np.asarray(want[f]), f"{what}: {f}")


@pytest.mark.parametrize("case", ["nan-sums", "outlier-1", "outlier-2"])
@pytest.mark.parametrize("d", [64, 128])
def test_pooled_hostile_chains(d, case, gpu, orc):
    """PooledARWMH with six hostile chains (_pooled_hostile_z0): 4 steps at
    sync_every = 1 and one block of 4 against the oracle's pooled mirror --
    sums, shared state, chain state.  The outlier cases keep S_d and S_dd
    finite, so the refactorisation's amh_pivot_ok keep-factor path (outlier-2)
    and a 1e18-scale factor (outlier-1) are compared apart from the NaN-sums
    path."""
    from kernels_amd import PooledARWMH, PRNGKey
    Cn = 300
    kw, mk, om = make_case("gaussian", d)
    z0 = _pooled_hostile_z0(Cn, d, case)
    for K, blocks in ((1, 4), (4, 1)):
        k = PooledARWMH(num_chains=Cn, sync_every=K, **kw)
        st = k.init(PRNGKey(2), 0, torch.from_numpy(z0.copy()), (), mk)
        ost = orc.init(om, PRNGKey(2), Cn, init_z=z0)
        z, pe, keys = ost.z, ost.potential_energy, ost.rng_key
        assert_bitequal_nan(st.potential_energy, pe, "pooled init pe")
        sh = orc.pooled_init_shared(om.d)
        for t in range(blocks):
            st = k.sample(st)
            z, pe, sums = orc.pooled_stats(om, int(sh["i"][0]), z, pe, keys, sh["mu"], sh["L"], float(sh["lam"][0]),
                                           k_steps=K)
            torch.cuda.synchronize()
            refactorised = orc.pooled_update(om, sums, sh, k_steps=K)
            if K == 1 and t == 0 and case != "nan-sums":  # reach: finite S_dd, pivot test fails only in outlier-2
                assert np.isfinite(sums[:-2]).all() and refactorised == (case == "outlier-1")
            _pooled_compare(k, st, z, pe, sums, sh, f"pooled d={d} K={K} block {t + 1}")
