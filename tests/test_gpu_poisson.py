"""AMH_MODEL_POISSON on the GPU (include/amh.h): the MFMA potential against
the lane-group one bit for bit and against float64 within a forward error
bound, the fused transitions (ARWMH, ASSS, pooled ARWMH, pooled ASSS) against
the external paths fed the library's own potential (which
tests/test_gpu_external.py, test_gpu_asss_external.py,
test_gpu_pooled_external.py and test_gpu_pooled_asss_external.py pin to the
oracle), the posterior it samples, the driver and the binding's limits."""
import contextlib
import ctypes
import io
import math

import numpy as np
import pytest
import torch

from helpers import ASSS_FIELDS, FIELDS, assert_bitequal_nan, assert_state_bitequal_nan

pytestmark = pytest.mark.gpu

NS = (1, 31, 32, 33, 77, 300)  # below, at, just past one 32-row tile; ragged last tiles
CS = (1, 37, 130)              # partial and full blocks of the potential kernel
KS = (1, 8, 9, 17, 31)         # GV = 1 (K = 1, and full at K = 8), 2, 3, 4; both parities


def _entry(N, K, seed=0, offset=True, extreme=False):
    """Synthetic data; extreme: y = 0 in row 0 and y = 1000 in the last row,
    and rows 0 and 1 scaled by +40 and -40, so that eta is large of both signs
    there (amh_expf overflows in one, underflows in the other) for any
    coefficients that are not small."""
    import posteriors as P
    d = P.synthetic_poisson(N, K, seed)
    if extreme:
        d["y"][0] = 0.0
        d["y"][N - 1] = 1000.0
        d["X"][0] *= 40.0
        if N > 1:
            d["X"][1] *= -40.0
    return P.poisson_regression(d["X"], d["y"], d["offset"] if offset else None)


def _starts(C, d, seed, width=2.0):
    return np.random.default_rng(seed).uniform(-width, width, size=(C, d)).astype(np.float32)


def _same_class_or_bits(a, b, what):
    """uint32 equality; a non-finite entry only has to be non-finite (NaN or
    inf, payloads not compared) on both sides.  -> the finite count."""
    a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
    fa, fb = np.isfinite(a), np.isfinite(b)
    assert np.array_equal(fa, fb), (what, a[fa != fb], b[fa != fb])
    bad = np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)) & fa)
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} differ; first {bad[:5]}: {a[bad[:5]]} vs {b[bad[:5]]}"
    return int(fa.sum())


# ------------------------------------------- 1. MFMA kernel = group kernel --
@pytest.mark.parametrize("offset", [True, False])
@pytest.mark.parametrize("K", KS)
def test_mfma_potential_equals_group_potential(K, offset, gpu):
    """amh_potential (and amh_init's pe0) run the MFMA kernel; the fused slice
    transition evaluates PoissonM in the chain's lane group and stores U of
    the point it stores (amh_asss.h asss_outcome: pen = U0 or ux, the energy of
    xnew, NaN -> +inf).  So after ASSS.sample the stored energies must be the
    MFMA kernel's of the stored points."""
    from kernels_amd import ASSS, PRNGKey
    d = K + 1
    moved = finite = nonfinite = 0
    for N in NS:
        e = _entry(N, K, seed=N, offset=offset, extreme=True)
        for C in CS:
            z0 = _starts(C, d, 7 * N + C)
            if C > 3:
                z0[1] *= 30.0           # large coefficients: exp overflows or underflows in many rows
                z0[2, d - 1] = np.nan   # a NaN coordinate
            k = ASSS(model=e, num_chains=C)
            st = k.init(PRNGKey(N), 0, torch.as_tensor(z0), (), {})
            f = _same_class_or_bits(st.potential_energy, k.potential(st.z), f"K={K} N={N} C={C} init")
            finite, nonfinite = finite + f, nonfinite + C - f
            for t in range(2):
                st = k.sample(st, (), {})
                _same_class_or_bits(st.potential_energy, k.potential(st.z), f"K={K} N={N} C={C} step {t}")
            moved += int((st.z.cpu() != torch.as_tensor(z0)).any(-1).sum())
    assert moved > 100  # the compared points are the transitions' own, not only the starts
    assert finite > 100 and nonfinite > 5, (finite, nonfinite)  # both classes were compared


# ------------------------------------------------------- 2. float64 anchor --
def _edge_points(d):
    """Zero, tiny, overflowing, underflowing and cancelling points."""
    rows = [np.zeros(d), np.full(d, 1e-30), np.full(d, -1e-30)]
    for s in (3.0, -3.0, 100.0, -100.0):
        r = np.zeros(d)
        r[1:] = s
        rows.append(r)
    r = np.full(d, 50.0) * (-1.0) ** np.arange(d)
    r[0] = 2.0
    rows.append(r)
    r = np.zeros(d)
    r[0], r[d - 1] = -2.0, 1e4
    rows.append(r)
    r = np.zeros(d)
    r[0] = -30.0  # every e^eta tiny: U is y |eta| and the constants
    rows.append(r)
    return np.asarray(rows, np.float32)


@pytest.mark.parametrize("K", KS)
def test_potential_float64_anchor(K, gpu):
    """|U_gpu - U_f64| <= c u (sum_n row_n + (N/32 + 6) sum_n (e^eta_n + |y_n eta_n|) + 6 (prior terms + |c0|)),
    row_n = (e^eta_n + y_n)(K + 2)(s_n + |I| + |o_n|) + 4 e^eta_n + 2 |y_n eta_n|, s_n = sum_k |X_nk b_k|,
    u = 2^-24, evaluated per point in float64, with c = 2.

    Where the terms and c come from, to first order in u (1 ulp <= 2 u
    relative).  eta: the K fmaf of m_n round by at most K u s_n, the addition
    I + m_n by u (|I| + s_n) and + o_n by u (|I| + s_n + |o_n|): |d eta| <=
    u (K + 2)(s_n + |I| + |o_n|), and |dt / d eta| = |e^eta - y| <= e^eta + y.
    amh_expf is within 1.5 ulp (tests/test_rng_math.py test_expf): 3 u e^eta;
    the product y eta rounds by u |y eta| and the difference by u |t| <=
    u (e^eta + |y eta|): together 4 u e^eta + 2 u |y eta|.  That is row_n.  A
    residue's partial sum has at most N/32 + 1 additions and the butterfly 5
    more, each at most u times the sum of the |t|: (N/32 + 6) sum (e^eta +
    |y eta|).  B: a square (u), 5 butterfly additions of non-negative terms
    (5 u) and the product with ib2 (u), 7 u of its prior term; (0.5 (I I)) iI2:
    2 u; the last three additions each round by u times a partial total, at
    most 3 u (sum |t| + prior terms + |c0|).  First-order total: sum row_n +
    (N/32 + 9) sum |t| + 10 prior terms + 3 |c0|.  The bracket of the issue
    has (N/32 + 6) sum (e^eta + |y eta|) and 6 (prior terms + |c0|); twice the
    bracket covers the total, because 3 sum |t| <= (N/32 + 6) sum (e^eta +
    |y eta|) and 10 P + 3 |c0| <= 12 (P + |c0|): c = 2.  What is left of the
    second bracket, at least (N/32 + 3) sum |t| + sum row_n, pays for the terms
    of second order: (1 + u)^n - 1 - n u over n <= 50 roundings (3e-6
    relative) and e^{d eta} - 1 - d eta, at most d eta itself while d eta <=
    1.25, which the test asserts for every compared point (the largest is
    1.5e-2, at the point with one coefficient of 1e4).  "prior terms" are |B ib2 / 2| +
    |I^2 iI2 / 2|.  Every point with U_64 < 1e30 is compared; past it the GPU
    value may be non-finite only where U_64 > 1e37 (DESIGN.md §9's rule; no
    input here is non-finite).  The measured maximum ratio to the bound with
    c = 1 is in DESIGN.md §9."""
    import posteriors as P
    from kernels_amd import ARWMH, PRNGKey
    d = K + 1
    c, u = 2.0, 2.0 ** -24
    worst, compared, skipped = 0.0, 0, 0
    for N in NS:
        e = _entry(N, K, seed=N)
        X = torch.as_tensor(e.X, dtype=torch.float64)
        y = torch.as_tensor(e.y, dtype=torch.float64)
        o = torch.as_tensor(e.offset, dtype=torch.float64)
        iI2, ib2, c0 = (float(v) for v in e.consts)
        for C in CS:
            z = np.concatenate([_starts(C, d, 11 * N + C), _edge_points(d)])
            k = ARWMH(model=e, num_chains=z.shape[0])
            k.init(PRNGKey(0), 0, torch.as_tensor(z), (), {})
            got = k.potential(torch.as_tensor(z).cuda()).cpu().double()
            z64 = torch.as_tensor(z, dtype=torch.float64)
            ref = P.poisson_potential_f64(z64, e)
            icpt, b = z64[:, 0], z64[:, 1:]
            eta = icpt[:, None] + b @ X.T + o
            ee, ye = torch.exp(eta), (y * eta).abs()
            s = (X.abs()[None] * b.abs()[:, None, :]).sum(-1)  # [points, N]
            deta = (K + 2) * (s + icpt.abs()[:, None] + o.abs())
            row = (ee + y) * deta + 4 * ee + 2 * ye
            prior = 0.5 * (b * b).sum(-1) * ib2 + 0.5 * icpt * icpt * iI2
            bracket = row.sum(-1) + (N / 32 + 6) * (ee + ye).sum(-1) + 6 * (prior + abs(c0))
            use = ref < 1e30  # (an infinite U_64 is not below it)
            allowed = ~(ref <= 1e37)
            assert bool((torch.isfinite(got) | allowed).all()), (K, N, C, got[~torch.isfinite(got) & ~allowed])
            assert bool(torch.isfinite(got[use]).all())
            assert float((u * deta[use]).max()) <= 1.25
            ratio = (got[use] - ref[use]).abs() / (u * bracket[use])
            worst = max(worst, float(ratio.max()))
            compared, skipped = compared + int(use.sum()), skipped + int((~use).sum())
            assert float(ratio.max()) <= c, (K, N, C, int(ratio.argmax()), float(ratio.max()))
    print(f"K={K}: max |dU| / (2^-24 bracket) = {worst:.3f} over {compared} points ({skipped} past 1e30)")
    assert compared > 10 * skipped


# ---------------------------------- 3. ARWMH = the external path, same U --
def _leaf_states(a, b, what, fields=FIELDS):
    assert_state_bitequal_nan(a, b, what, fields=fields)


@pytest.mark.parametrize("d", [17, 26, 32])
def test_arwmh_equals_external_bitexact(d, gpu):
    from kernels_amd import ARWMH, PRNGKey
    C, K = 77, d - 1
    e = _entry(150, K, seed=d)
    z0 = torch.as_tensor(_starts(C, d, 0, 0.5))
    kg = ARWMH(model=e, num_chains=C)
    ke = ARWMH(potential_fn=lambda z: kg.potential(z), num_chains=C)
    sg = kg.init(PRNGKey(0), 4, z0, (), {})
    se = ke.init(PRNGKey(0), 4, z0, (), {})
    _leaf_states(sg, se, f"d={d} init")
    for t in range(8):  # crosses gamma_1 = 1 (keep L) and the warm-up reset at W + 1
        sg = kg.sample(sg, (), {})
        se = ke.sample(se, (), {})
        _leaf_states(sg, se, f"d={d} step {t}")
    assert 0.0 < float(sg.mean_accept_prob.mean()) < 1.0
    kg.sample_(sg, 5)
    for _ in range(5):  # five external single steps
        se = ke.sample(se, (), {})
    _leaf_states(sg, se, f"d={d} in place")
    sg2, cz, cp = kg.run(sg, 6, thinning=3, collect_z=True, collect_pe=True)
    zs, ps = [], []
    for _ in range(6):
        se = ke.sample(se, (), {})
        zs.append(se.z.clone())
        ps.append(se.potential_energy.clone())
    _leaf_states(sg2, se, f"d={d} run")
    assert_bitequal_nan(cz, torch.stack(zs)[2::3], "collected z")
    assert_bitequal_nan(cp, torch.stack(ps)[2::3], "collected pe")


@pytest.mark.parametrize("d", [17, 32])
def test_asss_equals_host_shrink_bitexact(d, gpu):
    from kernels_amd import ASSS, PRNGKey
    C, K = 37, d - 1
    e = _entry(150, K, seed=d)
    z0 = torch.as_tensor(_starts(C, d, 0, 0.5))
    kg = ASSS(model=e, num_chains=C)
    ke = ASSS(potential_fn=lambda z: kg.potential(z), num_chains=C, host_shrink=True)
    sg = kg.init(PRNGKey(0), 4, z0, (), {})
    se = ke.init(PRNGKey(0), 4, z0, (), {})
    _leaf_states(sg, se, f"d={d} init", ASSS_FIELDS)
    for t in range(8):
        sg = kg.sample(sg, (), {})
        se = ke.sample(se, (), {})
        _leaf_states(sg, se, f"d={d} step {t}", ASSS_FIELDS)
    assert bool((sg.z != z0.cuda()).any())
    # sample_Pnx with the frozen adapt state of chain 2
    ad = sg.adapt_state
    loc, scale = ad.loc[2].clone(), ad.scale[2].clone()
    x = np.random.default_rng(3).normal(size=(4, d)).astype(np.float32) * 0.3
    out = kg.sample_Pnx(PRNGKey(7), x, (loc, scale), n=4, n_samples=33)
    ref = ke.sample_Pnx(PRNGKey(7), x, (loc, scale), n=4, n_samples=33)
    assert out.shape == (4, 33, d)
    assert_bitequal_nan(out, ref, "sample_Pnx")
    assert float((out.cpu() != torch.as_tensor(x)[:, None, :]).any(-1).float().mean()) > 0.2


def test_arwmh_sample_pnx_equals_external(gpu):
    """The fused frozen kernel against amh_pnx_propose / amh_pnx_accept
    (ARWMH._sample_pnx_external) around the same U."""
    from kernels_amd import ARWMH, PRNGKey
    d, C = 17, 8
    e = _entry(150, d - 1, seed=5)
    z0 = torch.as_tensor(_starts(C, d, 0, 0.5))
    kg = ARWMH(model=e, num_chains=C)
    st = kg.init(PRNGKey(1), 0, z0, (), {})
    st = kg.sample_(st, 30)
    ad = st.adapt_state
    ke = ARWMH(potential_fn=lambda z: kg.potential(z), num_chains=C)
    ke.init(PRNGKey(1), 0, z0, (), {})
    x = np.random.default_rng(3).normal(size=(4, d)).astype(np.float32) * 0.1
    frozen = (ad.loc[2], ad.scale[2], ad.log_step_size[2])
    out = kg.sample_Pnx(PRNGKey(7), x, frozen, n=6, n_samples=33)
    ref = ke.sample_Pnx(PRNGKey(7), x, frozen, n=6, n_samples=33)
    assert out.shape == (4, 33, d)
    assert_bitequal_nan(out, ref, "sample_Pnx")
    assert float((out.cpu() != torch.as_tensor(x)[:, None, :]).any(-1).float().mean()) > 0.2


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("d,C,K", [(7, 517, 1), (7, 517, 4), (32, 300, 1), (32, 300, 4)])
def test_pooled_model_equals_callable(d, C, K, exact, gpu):
    """PooledARWMH(model) against PooledARWMH(callable) around the same U, as
    tests/test_gpu_logistic.py (517 chains: 33 chunks of 16 with a ragged last
    one); three blocks of sync_every = K steps, every leaf and the sums; at
    K = 4 through PooledARWMH._step_order_block.  exact: the fixed-point sums."""
    from kernels_amd import PooledARWMH, PRNGKey
    e = _entry(150, d - 1, seed=d)
    z0 = torch.as_tensor(_starts(C, d, 2, 0.5))
    kg = PooledARWMH(model=e, num_chains=C, sync_every=K, exact_sums=exact)
    kp = PooledARWMH(model=e, num_chains=C)  # a second binding, for its potential only
    kp.init(PRNGKey(2), 0, z0, (), {})
    ke = PooledARWMH(potential_fn=lambda z: kp.potential(z), num_chains=C, sync_every=K, exact_sums=exact)
    sg = kg.init(PRNGKey(2), 0, z0, (), {})
    se = ke.init(PRNGKey(2), 0, z0, (), {})
    for b in range(3):
        sg = kg.sample(sg)
        se = ke.sample(se)
        torch.cuda.synchronize()
        assert int(sg.i[0]) == (b + 1) * K
        assert torch.equal(kg._sums, ke._sums)
        for name, a, r in zip(("i", "z", "pe", "macc", "asc", "cov", "mu", "L", "lam"),
                              (sg.i, sg.z, sg.potential_energy, sg.mean_accept_prob, sg.as_change, sg.cov)
                              + tuple(sg.adapt_state),
                              (se.i, se.z, se.potential_energy, se.mean_accept_prob, se.as_change, se.cov)
                              + tuple(se.adapt_state)):
            assert_bitequal_nan(a, r, f"d={d} C={C} K={K} block {b + 1}: {name}")
    assert 0.0 < float(sg.mean_accept_prob[0]) < 1.0
    if K > 1:  # in place: in and out states alias
        sg2 = kg.init(PRNGKey(2), 0, z0, (), {})
        kg.sample_(sg2, 3 * K)
        torch.cuda.synchronize()
        assert_bitequal_nan(sg2.z, se.z, "in place z")
        assert_bitequal_nan(sg2.cov, se.cov, "in place cov")


# ------------- 4. PooledASSS(model) = PooledASSS(callable, host_shrink=True) --
def _pleaves(s):
    a = s.adapt_state
    return dict(i=s.i, z=s.z, potential_energy=s.potential_energy, mean_accept_prob=s.mean_accept_prob, loc=a.loc,
                scale=a.scale, log_step_size=a.log_step_size, as_change=s.as_change, cov=s.cov)


SHARED = ("i", "mean_accept_prob", "loc", "scale", "log_step_size", "as_change", "cov")


def _bytes(t):
    return t.detach().cpu().numpy().tobytes()


def _assert_same(a, b, what, names=None):
    torch.cuda.synchronize()
    la, lb = _pleaves(a), _pleaves(b)
    for n in names or la:
        assert _bytes(la[n]) == _bytes(lb[n]), f"{what}: {n} differs"


def _c_state(st, i=None, z=None, pe=None):
    from kernels_amd import _lib
    a = st.adapt_state
    return _lib.AmhPooledState((st.i if i is None else i).data_ptr(), (st.z if z is None else z).data_ptr(),
                               (st.potential_energy if pe is None else pe).data_ptr(), st.rng_key.data_ptr(),
                               st.mean_accept_prob.data_ptr(), a.loc.data_ptr(), a.scale.data_ptr(),
                               a.log_step_size.data_ptr(), st.as_change.data_ptr(), st.cov.data_ptr())


def _pooled_asss_pair(d, C, K=1, num_warmup=0, seed=0):
    """-> (the model's sampler, its state, the host-shrink sampler around the
    model sampler's own potential, its state): same key, same start."""
    from kernels_amd import PooledASSS, PRNGKey
    e = _entry(150, d - 1, seed=d)
    z0 = torch.as_tensor(_starts(C, d, seed, 0.5))
    kr = PooledASSS(model=e, num_chains=C, sync_every=K)
    sr = kr.init(PRNGKey(seed), num_warmup, z0, (), {})
    ke = PooledASSS(potential_fn=lambda z: kr.potential(z), num_chains=C, sync_every=K, host_shrink=True)
    se = ke.init(PRNGKey(seed), num_warmup, z0, (), {})
    return kr, sr, ke, se


@pytest.mark.parametrize("d,C", [(7, 517), (32, 300)])
def test_pooled_asss_single_transitions(d, C, gpu):
    """K = 1, num_warmup = 4, 8 blocks alternating sample and sample_(1)
    (crosses gamma_1 = 1 and the warm-up reset): every leaf and the sums are
    the host-shrink sampler's bytes after every block (the standard of
    tests/test_gpu_pooled_asss_external.py)."""
    kr, sr, ke, se = _pooled_asss_pair(d, C, num_warmup=4)
    _assert_same(se, sr, f"d={d} init")
    rounds = []
    for b in range(8):
        if b % 2 == 0:
            sr, se = kr.sample(sr), ke.sample(se)
        else:
            kr.sample_(sr, 1)
            ke.sample_(se, 1)
        _assert_same(se, sr, f"d={d} C={C} block {b + 1}")
        assert _bytes(ke._sums) == _bytes(kr._sums), f"d={d} C={C} block {b + 1}: sums differ"
        rounds.append(ke.shrink_rounds)
    print("shrink rounds", rounds)
    assert int(sr.i[0]) == 8
    assert max(rounds) >= 3, rounds  # the multi-round path was taken
    assert 0.0 < float(sr.mean_accept_prob[0]) <= 1.0


def _model_single_steps(kr, st, K):
    """The block's K frozen transitions of `st` as K single-step
    amh_pooled_asss_stats_k launches on the model's handle at i + t ->
    (z, pe after the block, the float64 sum of the K sums in step order)."""
    from kernels_amd import _lib
    dev = st.z.device
    z, pe, total = st.z, st.potential_energy, None
    s = torch.zeros(kr._sums.shape[0], dtype=torch.float64, device=dev)
    for t in range(K):
        it = st.i + t
        zo, po = torch.empty_like(z), torch.empty_like(pe)
        _lib.check(_lib.lib().amh_pooled_asss_stats_k(kr._handle.h, z.shape[0], ctypes.byref(_c_state(st, it, z, pe)),
                                                      1, _lib.ptr(zo), _lib.ptr(po), _lib.ptr(s),
                                                      _lib.stream_ptr(dev.index)), kr._handle.h)
        torch.cuda.synchronize()
        total = s.cpu().numpy().copy() if t == 0 else total + s.cpu().numpy()
        z, pe = zo, po
    return z, pe, total


@pytest.mark.parametrize("d,C", [(7, 517), (32, 300)])
def test_pooled_asss_blocks(d, C, gpu):
    """K = 2, two blocks (the standard of test_blocks there): z / pe are the
    model sampler's fused K-block's bytes from the same state and those of K
    single-step launches; the host-shrink block's sums are the float64 sum, in
    step order, of the K single-step sums of the model's handle; the shared
    leaves are amh_pooled_asss_update_k's from those sums."""
    from kernels_amd import _lib
    K = 2
    kr, _, ke, se = _pooled_asss_pair(d, C, K=K)
    for b in range(2):
        fused = kr.sample(se)  # the fused K-block from the host-shrink sampler's state
        z1, pe1, total = _model_single_steps(kr, se, K)
        out = ke.sample(se)
        torch.cuda.synchronize()
        assert _bytes(out.z) == _bytes(fused.z) == _bytes(z1), f"block {b + 1}: z"
        assert _bytes(out.potential_energy) == _bytes(fused.potential_energy) == _bytes(pe1), f"block {b + 1}: pe"
        assert ke._sums.cpu().numpy().tobytes() == total.tobytes(), f"block {b + 1}: sums"
        assert total[-1] == float(K * C)
        ref = kr._new_like(se)
        sums = torch.as_tensor(total).to(gpu)
        _lib.check(_lib.lib().amh_pooled_asss_update_k(kr._handle.h, _lib.ptr(sums), ctypes.byref(_c_state(se)),
                                                       ctypes.byref(_c_state(ref)), K, _lib.stream_ptr(gpu.index)),
                   kr._handle.h)
        _assert_same(out, ref, f"block {b + 1} update", names=SHARED)
        assert int(out.i[0]) == (b + 1) * K
        se = out


# ------------------------------------------------ 5. samples the posterior --
@pytest.fixture(scope="module")
def posterior_2d():
    """K = 1, N = 40, with offsets: mean and covariance of exp(-U) by the
    float64 quadrature that tests/test_poisson.py::test_posterior_quadrature_grid
    checks on the CPU (spacing at most a tenth of the smaller posterior sd)."""
    from test_poisson import posterior_2d_quadrature, posterior_entry
    e = posterior_entry()
    mean, cov, spacing, _ = posterior_2d_quadrature(e)
    assert spacing.max() <= np.sqrt(np.diag(cov)).min() / 10
    return e, mean, cov


@pytest.mark.parametrize("sampler", ["ARWMH", "ASSS"])
def test_samples_posterior(sampler, posterior_2d, gpu):
    """4,096 independent chains with the schedule of the logistic model's test
    (300 warm-up, 300 more, 2,000 steps thinned by 10): the mean of the kept
    draws has a standard error of at most sd / 64 (were the 200 draws of a
    chain fully correlated), a covariance entry at most sqrt(2) sd_i sd_j / 64
    (normal fourth moments); 6 such errors each."""
    import kernels_amd
    e, mean, cov = posterior_2d
    C = 4096
    k = getattr(kernels_amd, sampler)(model=e, num_chains=C)
    st = k.init(kernels_amd.PRNGKey(3), 300, None, (), {})
    st = k.sample_(st, 300)
    st, cz, _ = k.run(st, 2000, thinning=10)
    assert cz.shape == (200, C, 2)
    z = cz.reshape(-1, 2).double().cpu().numpy()
    sd = np.sqrt(np.diag(cov))
    m = z.mean(0)
    cv = np.cov(z.T)
    print(sampler, "mean", m, "ref", mean, "cov", cv.reshape(-1), "ref", cov.reshape(-1))
    assert np.all(np.abs(m - mean) <= 6 * sd / 64), (m, mean, sd)
    assert np.all(np.abs(cv - cov) <= 6 * math.sqrt(2) * np.outer(sd, sd) / 64), (cv, cov)


# ------------------------------------------------- 6. driver and limits --
def test_mcmc_driver(gpu):
    from infer_amd import MCMC
    from kernels_amd import ARWMH, PRNGKey
    K, C = 5, 64
    e = _entry(77, K, seed=1)
    m = MCMC(ARWMH(model=e, num_chains=C), num_warmup=100, num_samples=50)
    m.run(PRNGKey(0))
    s = m.get_samples()
    assert set(s) == {"Intercept", "b"}
    assert s["Intercept"].shape == (C * 50,) and s["b"].shape == (C * 50, K)
    g = m.get_samples(group_by_chain=True)
    assert g["Intercept"].shape == (C, 50) and g["b"].shape == (C, 50, K)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        m.print_summary()
    assert "Intercept" in buf.getvalue() and "b[4]" in buf.getvalue()


def test_bind_limits_and_rebinding(gpu):
    import posteriors as P
    from kernels_amd import ARWMH, PRNGKey, _lib
    dev = torch.device("cuda", torch.cuda.current_device())
    e1, e2 = _entry(33, 4, seed=1), _entry(77, 4, seed=2)
    data, ip = e1.pack({}, dev)
    h = _lib.Handle(5, 0, 2 / 3, 0.234, 1e-6, dev.index)
    with pytest.raises(_lib.AmhError, match=r"N\*K \+ 2\*N \+ 3"):
        h.bind_model(_lib.AMH_MODEL_POISSON, data[:-1].contiguous(), ip)
    with pytest.raises(_lib.AmhError, match="poisson needs iparams"):
        h.bind_model(_lib.AMH_MODEL_POISSON, data, ip[:1])
    with pytest.raises(_lib.AmhError, match="poisson needs N >= 1"):
        h.bind_model(_lib.AMH_MODEL_POISSON, data, (0, 4))
    with pytest.raises(_lib.AmhError, match="model dimension 4 != config dim 5"):
        h.bind_model(_lib.AMH_MODEL_POISSON, torch.zeros(33 * 3 + 2 * 33 + 3, device=dev), (33, 3))
    h32 = _lib.Handle(33, 0, 2 / 3, 0.234, 1e-6, dev.index)
    with pytest.raises(_lib.AmhError, match="poisson needs 1 <= K <= 31"):
        h32.bind_model(_lib.AMH_MODEL_POISSON, torch.zeros(2 * 32 + 2 * 2 + 3, device=dev), (2, 32))
    h32.close()
    # a second data set on the same handle: the tile copy is replaced
    z = torch.as_tensor(_starts(50, 5, 0, 0.5)).to(dev)
    pe = torch.empty(50, dtype=torch.float32, device=dev)

    def potential():
        _lib.check(_lib.lib().amh_potential(h.h, _lib.ptr(z), _lib.ptr(pe), 50, _lib.stream_ptr(dev.index)), h.h)
        return pe.clone()

    h.bind_model(_lib.AMH_MODEL_POISSON, data, ip)
    u1 = potential()
    data2, ip2 = e2.pack({}, dev)
    h.bind_model(_lib.AMH_MODEL_POISSON, data2, ip2)
    u2 = potential()
    h.bind_model(_lib.AMH_MODEL_POISSON, data, ip)
    u1b = potential()
    h.close()
    for u, e in ((u1, e1), (u2, e2)):
        ref = P.poisson_potential_f64(z.double(), e)
        assert torch.allclose(u.double(), ref, rtol=1e-5, atol=0)
    assert not torch.equal(u1, u2) and torch.equal(u1, u1b)
    k = ARWMH(model=e2, num_chains=50)
    k.init(PRNGKey(0), 0, z, (), {})
    assert torch.equal(k.potential(z), u2)
