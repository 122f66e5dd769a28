"""The GLM kernels (AMH_MODEL_LOGISTIC, AMH_MODEL_POISSON) and the diamonds
MFMA kernel at its tile edges against the C oracle's mirror (pot_glm,
pot_diamonds in oracle/amh_oracle.c), uint32 for uint32: NaN positions and the
signs of inf and of zero are compared (helpers.assert_bitequal_nan; only a
NaN's payload is not, x86 and gfx950 make different default NaNs).  The
transitions of the registry kinds "logistic" / "poisson" are in the matrices
of tests/test_gpu_parity.py, test_gpu_asss.py and test_gpu_edges.py; here are
the potential over the shape grid, the pooled sampler and diamonds' shapes."""
import ctypes
import re
import os

import numpy as np
import pytest
import torch

from helpers import (POOLED_LEAVES, assert_bitequal_nan, assert_state_bitequal, assert_state_bitequal_nan, edge_points,
                     make_case, pooled_leaves)

pytestmark = pytest.mark.gpu

KS = (1, 2, 8, 9, 16, 17, 24, 25, 31)  # both sides of every GV boundary (8, 16, 24), both parities
NS = (1, 31, 32, 33, 64, 77, 300)      # below, at, past one 32-row tile; two full tiles; ragged last tiles
CS = (1, 37, 130, 257)                 # one chain; a half-empty B tile; a wave's second tile partly filled
#                                        (128 + 2); one chain past a full 256-chain block


def _entry(family, N, K, offset=True):
    """The data of the two GLM test files: logistic with rows 0 and 1 scaled
    by +-40 (the softplus saturates in both directions), Poisson with those
    rows, y = 0 in row 0 and y = 1000 in the last row, with or without
    offsets.  -> (entry, orc.Model on the entry's own packed float32 data)"""
    import orc
    if family == "logistic":
        from test_gpu_logistic import _entry as make
        e = make(N, K, seed=N, saturate=True)
    else:
        from test_gpu_poisson import _entry as make
        e = make(N, K, seed=N, offset=offset, extreme=True)
    arr, (n, k) = e.pack_fn(None)
    return e, orc.Model(orc.LOGISTIC if family == "logistic" else orc.POISSON, K + 1, arr, n_data=n, k_data=k)


def _points(family, d, seed):
    """uniform(-2, 2) starts, helpers.edge_points, and the saturating and
    cancelling rows of the family's own test file."""
    if family == "logistic":
        from test_gpu_logistic import _edge_points as own
    else:
        from test_gpu_poisson import _edge_points as own
    u = np.random.default_rng(seed).uniform(-2, 2, size=(max(CS), d)).astype(np.float32)
    return np.concatenate([u, edge_points(d, seed)[1], own(d)]).astype(np.float32)


def _classes(a):
    return np.array([np.isnan(a).sum(), np.isposinf(a).sum(), np.isneginf(a).sum(), np.isfinite(a).sum()])


# ------------------------------------------------ 1. potential = the mirror --
@pytest.mark.parametrize("family,offset", [("logistic", True), ("poisson", True), ("poisson", False)])
@pytest.mark.parametrize("K", KS)
def test_potential_equals_mirror(family, offset, K, gpu, orc):
    """amh_potential and amh_init's potential_energy (the MFMA kernel,
    glm_pot_mfma_kernel<Fam, GV>, over glm_pack_kernel's tile copy) against
    orc.potential / orc.init at every N of NS.  The kernel's chain count is
    the number of points of a call: every C of CS (rows taken from the pool at
    a C-dependent offset, so each count sees starts and edge rows) and the
    whole pool once.  Across the grid NaN, +inf and finite values are all
    compared, and the counts are printed: per N the pool holds at least 17
    rows with a NaN coordinate and 257 starts, and b'b overflows at the rows
    of 3e38 (Poisson's rows scaled by +-40 overflow amh_expf at about half
    of the starts as well)."""
    from kernels_amd import ARWMH, PRNGKey
    d = K + 1
    seen = np.zeros(4, np.int64)
    for N in NS:
        e, om = _entry(family, N, K, offset)
        pool = _points(family, d, 100 * K + N)
        want = orc.potential(om, pool)
        for C in CS:
            z = np.roll(pool, -(C * 7 + N), axis=0)[:C].copy()
            k = ARWMH(model=e, num_chains=C)
            st = k.init(PRNGKey(N), 0, torch.as_tensor(z), (), {})
            what = f"{family} K={K} N={N} C={C}"
            assert_state_bitequal_nan(st, orc.init(om, PRNGKey(N), C, init_z=z), what + " init")
            assert_bitequal_nan(k.potential(torch.as_tensor(z, device=gpu)), orc.potential(om, z), what + " potential")
        got = k.potential(torch.as_tensor(pool, device=gpu))
        assert_bitequal_nan(got, want, f"{family} K={K} N={N} pool")
        seen += _classes(want)
    print(f"{family} offset={offset} K={K}: compared NaN {seen[0]}, +inf {seen[1]}, -inf {seen[2]}, finite {seen[3]}")
    assert seen[0] >= 100 and seen[1] >= 5 and seen[3] >= 1000, seen


# --------------------------------------------- 2. ARWMH sample_Pnx, d = 17 --
@pytest.mark.parametrize("kind", ["logistic", "poisson"])
def test_sample_pnx_equals_mirror(kind, gpu, orc):
    """The fused frozen kernel (GlmM in the chain's lane group) against
    orc.sample_pnx, with the adapted state of a short run as the frozen theta."""
    from kernels_amd import ARWMH, PRNGKey
    kw, mk, om = make_case(kind, 17)
    k = ARWMH(num_chains=8, **kw)
    st = k.init(PRNGKey(1), 0, None, (), mk)
    st = k.sample_(st, 30)
    ad = st.adapt_state
    x = np.random.default_rng(3).normal(size=(4, 17)).astype(np.float32) * 0.1
    out = k.sample_Pnx(PRNGKey(7), x, (ad.loc[2], ad.scale[2], ad.log_step_size[2]), n=6, n_samples=33)
    ref = orc.sample_pnx(om, PRNGKey(7), x, ad.loc[2].cpu().numpy(), ad.scale[2].cpu().numpy(),
                         float(ad.log_step_size[2].cpu()), 6, 33)
    assert out.shape == (4, 33, 17)
    assert_bitequal_nan(out, ref, f"{kind} sample_Pnx")
    assert np.mean(np.any(ref != x[:, None, :], axis=-1)) > 0.2  # accepted moves are compared, not only rejections


# ------------------------------------------------------------- 3. pooled ----
def _pooled_pair(kind, d, C, K, orc, seed=2):
    from kernels_amd import PooledARWMH, PRNGKey
    kw, mk, om = make_case(kind, d)
    k = PooledARWMH(num_chains=C, sync_every=K, **kw)
    z0 = np.random.default_rng(seed).uniform(-0.5, 0.5, size=(C, om.d)).astype(np.float32)
    st = k.init(PRNGKey(seed), 0, torch.as_tensor(z0), (), mk)
    ost = orc.init(om, PRNGKey(seed), C, init_z=z0)
    assert_bitequal_nan(st.rng_key, ost.rng_key, "keys")
    assert_bitequal_nan(st.potential_energy, ost.potential_energy, "pe0")
    return k, st, om, ost


@pytest.mark.parametrize("kind", ["logistic", "poisson"])
@pytest.mark.parametrize("d,C,K", [(7, 517, 1), (32, 300, 1), (7, 517, 4), (32, 300, 4)])
def test_pooled_equals_mirror(kind, d, C, K, gpu, orc):
    """PooledARWMH(model) against orc.pooled_stats + orc.pooled_update, three
    blocks, every leaf and the sums (517 chains: 33 chunks of 16, the last one
    ragged).  At sync_every = 4 the product adds the completely reduced sums of
    K single-step launches in step order (PooledARWMH._step_order_block), so
    the reference is K oracle calls at positions i + t with the shared state
    frozen, summed in that order, then orc.pooled_update(k_steps = K)."""
    k, st, om, ost = _pooled_pair(kind, d, C, K, orc)
    z, pe, keys = ost.z, ost.potential_energy, ost.rng_key
    sh = orc.pooled_init_shared(om.d)
    moved = 0
    for b in range(3):
        st = k.sample(st)
        sums = None
        for t in range(K):
            zn, pe, s = orc.pooled_stats(om, int(sh["i"][0]) + t, z, pe, keys, sh["mu"], sh["L"], float(sh["lam"][0]))
            moved += int(np.any(zn != z, axis=1).sum())
            z = zn
            sums = s if sums is None else sums + s
        orc.pooled_update(om, sums, sh, k_steps=K)
        torch.cuda.synchronize()
        what = f"{kind} d={d} C={C} K={K} block {b + 1}"
        assert_bitequal_nan(k._sums, sums, what + ": sums")
        assert_bitequal_nan(st.z, z, what + ": z")
        assert_bitequal_nan(st.potential_energy, pe, what + ": pe")
        got = pooled_leaves(st)
        for f in POOLED_LEAVES:
            assert_bitequal_nan(got[f], sh[f], what + ": " + f)
    assert 0.05 <= moved / (3 * K * C) <= 0.6, moved  # accepted and rejected chain-steps were both compared


@pytest.mark.parametrize("kind,d,C", [("logistic", 7, 517), ("poisson", 32, 300)])
def test_pooled_stats_k_entry_equals_mirror(kind, d, C, gpu, orc):
    """amh_pooled_stats_k itself at k_steps = 4, which PooledARWMH never calls
    for these models: per chain z and pe, and the sums with the in-chunk
    association of every other registry model (one float32 accumulator per wave
    over a chain's 4 steps), against orc.pooled_stats(k_steps = 4)."""
    from kernels_amd import _lib
    k, st, om, ost = _pooled_pair(kind, d, C, 1, orc)
    sh = orc.pooled_init_shared(om.d)
    z, pe, keys = ost.z, ost.potential_energy, ost.rng_key
    for _ in range(2):  # off the identity factor first
        st = k.sample(st)
        z, pe, sums = orc.pooled_stats(om, int(sh["i"][0]), z, pe, keys, sh["mu"], sh["L"], float(sh["lam"][0]))
        orc.pooled_update(om, sums, sh)
    dev = st.z.device
    zo, po = torch.empty_like(st.z), torch.empty_like(st.potential_energy)
    out = torch.zeros(om.d + om.d * (om.d + 1) // 2 + 2, dtype=torch.float64, device=dev)
    c = k._c(st)
    with torch.cuda.device(dev.index):
        _lib.check(_lib.lib().amh_pooled_stats_k(k._handle.h, C, ctypes.byref(c), 4, _lib.ptr(zo), _lib.ptr(po),
                                                 _lib.ptr(out), _lib.stream_ptr(dev.index)), k._handle.h)
    torch.cuda.synchronize()
    z4, pe4, s4 = orc.pooled_stats(om, int(sh["i"][0]), z, pe, keys, sh["mu"], sh["L"], float(sh["lam"][0]), k_steps=4)
    assert_bitequal_nan(zo, z4, f"{kind} k_steps=4: z")
    assert_bitequal_nan(po, pe4, f"{kind} k_steps=4: pe")
    assert_bitequal_nan(out, s4, f"{kind} k_steps=4: sums")
    assert s4[-1] == 4 * C and np.any(z4 != z)


# ------------------------------------- 4. diamonds' MFMA kernel, tile edges --
def _dia_mfma_kc():
    """kDiaMfmaKc of csrc/amh_internal.h: the Kc at which amh_bind_model makes
    the tile copy (amh_split.hip pack_cols) and run_potential_lane takes
    diamonds_pot_mfma_kernel."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "adaptive-mcmc_amd", "csrc", "amh_internal.h")) as f:
        return int(re.search(r"constexpr int kDiaMfmaKc = (\d+);", f.read()).group(1))


def _diamonds(N, orc):
    import posteriors as P
    mk = P.synthetic_diamonds(N=N, K=25, seed=N)
    arr, (n, K) = P.diamonds.pack_fn(mk)
    # the MFMA path is the one these shapes take (the lane kernel has test_split_path_generic_k)
    assert K - 1 == _dia_mfma_kc() and n >= 1
    return P, mk, orc.Model(orc.DIAMONDS, K + 1, arr, n_data=n, k_data=K)


@pytest.mark.parametrize("N", [1, 31, 32, 33, 64])
def test_diamonds_mfma_tile_edges(N, gpu, orc):
    """diamonds_pot_mfma_kernel over the shared tile copy (glm_pack_kernel, one
    side vector) at one ragged tile (N < 32: the prefetch of tile m + 1 reads
    tile m again), exactly one and two full tiles, and one row past a tile;
    one chain, one chain past a B tile, one past a 256-chain block."""
    from kernels_amd import ARWMH, PRNGKey
    P, mk, om = _diamonds(N, orc)
    for C in (1, 33, 257):
        k = ARWMH(model=P.diamonds, num_chains=C)
        st = k.init(PRNGKey(N), 0, None, (), mk)
        assert_state_bitequal(st, orc.init(om, PRNGKey(N), C), f"diamonds N={N} C={C} init")
        z = np.random.default_rng(C).normal(size=(C, om.d)).astype(np.float32)
        assert_bitequal_nan(k.potential(torch.as_tensor(z, device=gpu)), orc.potential(om, z),
                            f"diamonds N={N} C={C} potential")


def test_diamonds_mfma_steps_off_tile(gpu, orc):
    """Five single steps of the split transition at N = 33, C = 66."""
    from kernels_amd import ARWMH, PRNGKey
    P, mk, om = _diamonds(33, orc)
    k = ARWMH(model=P.diamonds, num_chains=66)
    st = k.init(PRNGKey(4), 2, None, (), mk)
    ost = orc.init(om, PRNGKey(4), 66)
    for t in range(5):
        st = k.sample(st, (), {})
        orc.step(om, ost, 1, num_warmup=2)
        torch.cuda.synchronize()
        assert_state_bitequal(st, ost, f"diamonds N=33 step {t}")
