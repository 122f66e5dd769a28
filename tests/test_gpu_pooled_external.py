"""PooledARWMH with the caller's potential (AMH_MODEL_EXTERNAL:
amh_pooled_propose, U in torch, amh_pooled_stats_external) on the GPU.

The bit-exact tests use a potential the test can write in torch and the
oracle reproduces bit for bit: the Gaussian with m = 0, c0 = 0 and a
precision that is zero except P[0][0] = 2 and P[d-1][d-1] = 0.5.  Every
summation order of the oracle then adds exact zeros and performs one rounded
add, so U(z) = 0.5 * (z_0 * (2 z_0) + z_{d-1} * (0.5 z_{d-1})) in float32 --
written as separate torch operations, which nothing can contract -- is the
oracle's potential in the lane-per-row form (d < 64) and in the MFMA form
(d >= 64) alike.  The registry twin is the same Gaussian with
logdet_2pi_cov = 0 (P is singular for d > 2, so posteriors.gaussian(), which
derives c0 from the determinant, does not build it)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _precision(d):
    Pm = np.zeros((d, d), np.float64)
    Pm[0, 0] = 2.0
    Pm[d - 1, d - 1] = 0.5
    return Pm


def _orc_model(orc, d):
    data = np.concatenate([np.zeros(d), _precision(d).reshape(-1), [0.0]]).astype(np.float32)
    return orc.Model(orc.GAUSSIAN, d, data)


def _registry_twin(d):
    import posteriors as P
    return P.Gaussian(np.zeros(d), _precision(d), 0.0)


def _torch_U(d):
    def U(z):
        a = z[:, 0] * (2.0 * z[:, 0])
        b = z[:, d - 1] * (0.5 * z[:, d - 1])
        s = a + b
        return 0.5 * s
    return U


def _z0(C, d, seed):
    return np.random.default_rng(seed).uniform(-2, 2, size=(C, d)).astype(np.float32)


def _assert_state(st, z, pe, sh, what):
    got = dict(z=st.z, pe=st.potential_energy, mu=st.adapt_state.loc, L=st.adapt_state.scale,
               lam=st.adapt_state.log_step_size, macc=st.mean_accept_prob, asc=st.as_change, cov=st.cov, i=st.i)
    want = dict(z=z, pe=pe, mu=sh["mu"], L=sh["L"], lam=sh["lam"], macc=sh["macc"], asc=sh["asc"], cov=sh["cov"],
                i=sh["i"])
    for f in got:
        a = got[f].cpu().numpy()
        b = np.asarray(want[f])
        assert a.shape == b.shape, (what, f, a.shape, b.shape)
        assert a.tobytes() == b.astype(a.dtype).tobytes(), f"{what}: {f} differs"


def _oracle_block(orc, om, z, pe, keys, sh, K):
    """A block of K external rounds: K single-step oracle calls at positions
    i + t, z / pe chained, the sums added in float64 in step order."""
    tot = None
    for t in range(K):
        z, pe, s = orc.pooled_stats(om, int(sh["i"][0]) + t, z, pe, keys, sh["mu"], sh["L"], float(sh["lam"][0]),
                                    k_steps=1)
        tot = s.copy() if tot is None else tot + s
    return z, pe, tot


def _start(orc, d, C, seed, K=1, **kw):
    from kernels_amd import PooledARWMH, PRNGKey
    om = _orc_model(orc, d)
    k = PooledARWMH(potential_fn=_torch_U(d), num_chains=C, sync_every=K, **kw)
    z0 = _z0(C, d, seed)
    st = k.init(PRNGKey(seed), 0, torch.as_tensor(z0), (), {})
    ost = orc.init(om, PRNGKey(seed), C, init_z=z0)
    assert np.array_equal(st.rng_key.cpu().numpy().view(np.uint32), ost.rng_key)
    assert np.array_equal(st.potential_energy.cpu().numpy().view(np.uint32), ost.potential_energy.view(np.uint32))
    return k, st, om, ost.z, ost.potential_energy, ost.rng_key, orc.pooled_init_shared(d)


# (7, 517): cpw 1, 33 chunks = both reduce levels with a ragged tail; (40, 4097): cpw 2;
# (64, 2181): 18 chunks of the MFMA form = more than one reduce group
@pytest.mark.parametrize("d,C", [(7, 517), (40, 4097), (63, 300), (64, 300), (64, 2181), (96, 300), (128, 333),
                                 (256, 257)])
def test_pooled_external_bitexact(d, C, gpu, orc):
    """K = 1: per-chain state, the sums and the shared state bit for bit
    against the oracle over 5 steps (crosses gamma_1 = 1)."""
    k, st, om, z, pe, keys, sh = _start(orc, d, C, seed=0)
    accepted = 0
    for t in range(5):
        st = k.sample(st)
        zn, pe, sums = orc.pooled_stats(om, int(sh["i"][0]), z, pe, keys, sh["mu"], sh["L"], float(sh["lam"][0]))
        accepted += int(np.any(zn != z, axis=1).sum())
        z = zn
        torch.cuda.synchronize()
        np.testing.assert_array_equal(k._sums.cpu().numpy().view(np.uint64), sums.view(np.uint64),
                                      err_msg=f"sums step {t + 1}")
        orc.pooled_update(om, sums, sh)
        _assert_state(st, z, pe, sh, f"d={d} C={C} step {t + 1}")
    assert 0 < accepted < 5 * C  # both branches of the accept ran


def test_pooled_external_warm_bitexact(gpu, orc):
    """d = 128 from a warm shared state in the typical set of this potential
    (coordinates 0 and d - 1 at their target scales with the matching factor,
    lambda = log(2.38 / sqrt(2)) for its two informative coordinates): every
    step moves 10 % to 50 % of the chains, and the sums, the shared state and
    the chain state agree with the oracle byte for byte over 3 steps."""
    from helpers import apply_shared
    from kernels_amd import PooledARWMH, PRNGKey
    d, C = 128, 300
    om, sh = _orc_model(orc, d), orc.pooled_init_shared(d)
    k = PooledARWMH(potential_fn=_torch_U(d), num_chains=C)
    var = np.ones(d)
    var[0], var[d - 1] = 0.5, 2.0
    z0 = _z0(C, d, 7)
    z0[:, 0] = (np.random.default_rng(70).normal(size=C) * np.sqrt(var[0])).astype(np.float32)
    z0[:, d - 1] = (np.random.default_rng(71).normal(size=C) * np.sqrt(var[d - 1])).astype(np.float32)
    diag = np.cumsum([0] + [d - j for j in range(d - 1)])  # packed offsets of the diagonal
    sh["i"][:] = 20
    sh["macc"][:] = 0.2
    sh["mu"][:] = 0.05
    sh["lam"][:] = np.log(2.38 / np.sqrt(2.0))
    sh["L"][diag] = np.sqrt(var).astype(np.float32)
    sh["cov"][diag] = var
    st = apply_shared(k.init(PRNGKey(7), 0, torch.as_tensor(z0), (), {}), sh)
    ost = orc.init(om, PRNGKey(7), C, init_z=z0)
    z, pe, keys = ost.z, ost.potential_energy, ost.rng_key
    assert np.array_equal(st.potential_energy.cpu().numpy().view(np.uint32), pe.view(np.uint32))
    for t in range(3):
        st = k.sample(st)
        zn, pe, sums = orc.pooled_stats(om, int(sh["i"][0]), z, pe, keys, sh["mu"], sh["L"], float(sh["lam"][0]))
        share = float(np.any(zn != z, axis=1).mean())
        assert 0.10 <= share <= 0.50, f"moved share {share:.3f} at step {t + 1}"
        z = zn
        torch.cuda.synchronize()
        np.testing.assert_array_equal(k._sums.cpu().numpy().view(np.uint64), sums.view(np.uint64),
                                      err_msg=f"sums step {t + 1}")
        orc.pooled_update(om, sums, sh)
        _assert_state(st, z, pe, sh, f"warm d={d} step {t + 1}")


@pytest.mark.parametrize("d,C,K", [(7, 517, 3), (64, 300, 4), (128, 333, 3)])
def test_pooled_external_blocks(d, C, K, gpu, orc):
    """sync_every = K: a block is K rounds propose -> U -> accept, each
    round's sums reduced completely and added in step order -- K single-step
    oracle calls.  Above d = 64 that is also the oracle's own block order."""
    k, st, om, z, pe, keys, sh = _start(orc, d, C, seed=1, K=K)
    k2, st2, *_ = _start(orc, d, C, seed=1, K=K)
    for b in range(2):
        st = k.sample(st)
        if d == 128:
            zk, pk, sk = orc.pooled_stats(om, int(sh["i"][0]), z, pe, keys, sh["mu"], sh["L"], float(sh["lam"][0]),
                                          k_steps=K)
        z, pe, sums = _oracle_block(orc, om, z, pe, keys, sh, K)
        if d == 128:
            assert zk.tobytes() == z.tobytes() and pk.tobytes() == pe.tobytes()
            np.testing.assert_array_equal(sk.view(np.uint64), sums.view(np.uint64))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(k._sums.cpu().numpy().view(np.uint64), sums.view(np.uint64),
                                      err_msg=f"sums block {b + 1}")
        orc.pooled_update(om, sums, sh, k_steps=K)
        _assert_state(st, z, pe, sh, f"d={d} K={K} block {b + 1}")
    k2.sample_(st2, 2 * K)  # in place: in and out states alias
    torch.cuda.synchronize()
    _assert_state(st2, z, pe, sh, f"d={d} K={K} in place")
    with pytest.raises(ValueError):
        k2.sample_(st2, K + 1)


@pytest.mark.parametrize("d,C,overlap", [(40, 300, False), (128, 300, False), (40, 300, True)])
def test_pooled_external_equals_registry(d, C, overlap, gpu):
    """The same key and start through the external path and through the
    registry Gaussian's fused kernels: equal states after 6 steps."""
    from kernels_amd import PooledARWMH, PRNGKey
    z0 = torch.as_tensor(_z0(C, d, 2))
    ke = PooledARWMH(potential_fn=_torch_U(d), num_chains=C, overlap=overlap)
    kr = PooledARWMH(potential_fn=_registry_twin(d), num_chains=C, overlap=overlap)
    se = ke.init(PRNGKey(2), 0, z0, (), {})
    sr = kr.init(PRNGKey(2), 0, z0, (), {})
    for _ in range(6):
        se = ke.sample(se)
        sr = kr.sample(sr)
    torch.cuda.synchronize()
    assert int(se.i[0]) == 6
    assert torch.equal(ke._sums, kr._sums)
    for a, b in zip((se.i, se.z, se.potential_energy, se.mean_accept_prob, se.as_change, se.cov) + tuple(se.adapt_state),
                    (sr.i, sr.z, sr.potential_energy, sr.mean_accept_prob, sr.as_change, sr.cov) + tuple(sr.adapt_state)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("d,C", [(40, 300), (96, 130)])
def test_pooled_external_run_thinned(d, C, gpu, orc):
    """run() with thinning 3 collects the oracle's draws of steps 3 and 6."""
    k, st, om, z, pe, keys, sh = _start(orc, d, C, seed=3)
    out, cz, cp = k.run(st, 6, thinning=3, collect_z=True, collect_pe=True)
    zs, ps = [], []
    for _ in range(6):
        z, pe, sums = orc.pooled_stats(om, int(sh["i"][0]), z, pe, keys, sh["mu"], sh["L"], float(sh["lam"][0]))
        orc.pooled_update(om, sums, sh)
        zs.append(z.copy())
        ps.append(pe.copy())
    torch.cuda.synchronize()
    assert cz.shape == (2, C, d) and cp.shape == (2, C)
    np.testing.assert_array_equal(cz.cpu().numpy().view(np.uint32), np.stack(zs)[2::3].view(np.uint32))
    np.testing.assert_array_equal(cp.cpu().numpy().view(np.uint32), np.stack(ps)[2::3].view(np.uint32))
    _assert_state(out, z, pe, sh, f"d={d} run")
    assert int(st.i[0]) == 0  # run() leaves its input alone


def test_pooled_external_nan_rejects(gpu):
    """A proposal where U is NaN is rejected (NaN -> +inf, arwmh.py:171) and
    leaves the pooled sums, hence the shared state, finite."""
    from kernels_amd import PooledARWMH, PRNGKey
    U = lambda z: torch.where(z[:, 0] > 0, torch.nan, 0.5 * (z * z).sum(-1))  # noqa: E731
    k = PooledARWMH(potential_fn=U, num_chains=256)
    s = k.init(PRNGKey(2), 0, -torch.ones(256, 2), (), {})
    k.sample_(s, 100)
    torch.cuda.synchronize()
    assert int(s.i[0]) == 100
    assert bool((s.z[:, 0] <= 0).all())
    assert bool(torch.isfinite(s.potential_energy).all())
    assert bool(torch.isfinite(s.adapt_state.scale).all())


def test_pooled_external_samples_target(gpu):
    """U written in torch (the correlated 3-D Gaussian of
    test_torch_potential_samples_target): after 800 pooled steps the final
    state's 16,384 chains have the target's moments within five standard
    errors of that many independent draws (mean: sqrt(S_ii / C); variance of a
    Gaussian: S_ii sqrt(2 / C))."""
    from kernels_amd import PooledARWMH, PRNGKey
    S = torch.tensor([[1.0, 0.5, 0.0], [0.5, 2.0, -0.3], [0.0, -0.3, 0.5]], dtype=torch.float64)
    Pm = torch.linalg.inv(S).to(torch.float32).cuda()
    m = torch.tensor([1.0, -2.0, 0.5], device="cuda")

    def U(z):
        x = z - m
        return 0.5 * ((x @ Pm) * x).sum(-1)

    C = 16384
    k = PooledARWMH(potential_fn=U, num_chains=C)
    st = k.init(PRNGKey(3), 0, torch.rand(C, 3) * 4 - 2, (), {})
    k.sample_(st, 800)
    torch.cuda.synchronize()
    z = st.z.double().cpu()
    sii = torch.diagonal(S)
    mean_err = (z.mean(0) - m.double().cpu()).abs()
    var_err = (z.var(0, unbiased=True) - sii).abs()
    print("mean error / standard error", (mean_err / torch.sqrt(sii / C)).tolist())
    print("variance error / standard error", (var_err / (sii * (2.0 / C) ** 0.5)).tolist())
    assert bool((mean_err <= 5 * torch.sqrt(sii / C)).all())
    assert bool((var_err <= 5 * sii * (2.0 / C) ** 0.5).all())
    np.testing.assert_allclose(st.potential_energy.cpu().numpy(), U(st.z).cpu().numpy(), rtol=1e-6)


def test_pooled_external_limits(gpu):
    """d off the pooled dimensions raises the pooled ValueError; the split
    entries need an external handle; the fused entries still refuse one; a
    potential returning the wrong number of values raises as in ARWMH."""
    from kernels_amd import PooledARWMH, PRNGKey, _lib
    from kernels_amd._lib import AmhError
    U = lambda z: 0.5 * (z * z).sum(-1)  # noqa: E731
    with pytest.raises(ValueError, match="pooled mode"):
        PooledARWMH(potential_fn=U, num_chains=64).init(PRNGKey(0), 0, torch.zeros(64, 100), (), {})
    with pytest.raises(ValueError, match="one each"):
        PooledARWMH(potential_fn=lambda z: z.sum(), num_chains=8).init(PRNGKey(0), 0, torch.zeros(8, 4), (), {})
    L = _lib.lib()

    def entries(k, st):
        dev = st.z.device
        C, d = st.z.shape
        c = k._c(st)
        zp = torch.empty(C, d, device=dev)
        sums = torch.zeros(d + d * (d + 1) // 2 + 2, dtype=torch.float64, device=dev)
        s = _lib.stream_ptr(dev.index)
        h = k._handle.h
        return (lambda: L.amh_pooled_propose(h, C, ctypes.byref(c), 0, _lib.ptr(zp), s),
                lambda: L.amh_pooled_stats_external(h, C, ctypes.byref(c), 0, _lib.ptr(zp),
                                                    _lib.ptr(st.potential_energy), _lib.ptr(st.z),
                                                    _lib.ptr(st.potential_energy), _lib.ptr(sums), 0, s),
                lambda: L.amh_pooled_stats_k(h, C, ctypes.byref(c), 1, _lib.ptr(st.z), _lib.ptr(st.potential_energy),
                                             _lib.ptr(sums), s))

    kr = PooledARWMH(potential_fn=_registry_twin(8), num_chains=32)
    propose, stats_ext, _ = entries(kr, kr.init(PRNGKey(0), 0, torch.zeros(32, 8), (), {}))
    for call, name in ((propose, "amh_pooled_propose"), (stats_ext, "amh_pooled_stats_external")):
        assert call() == -1  # AMH_EINVAL
        with pytest.raises(AmhError, match=name + ": needs AMH_MODEL_EXTERNAL"):
            _lib.check(-1, kr._handle.h)
    ke = PooledARWMH(potential_fn=U, num_chains=32)
    _, _, stats_k = entries(ke, ke.init(PRNGKey(0), 0, torch.zeros(32, 8), (), {}))
    rc = stats_k()
    assert rc == -1
    with pytest.raises(AmhError, match="device potential"):
        _lib.check(rc, ke._handle.h)
    torch.cuda.synchronize()
