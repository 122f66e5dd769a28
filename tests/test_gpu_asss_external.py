"""ASSS with the caller's potential (ASSS(host_shrink=True): amh_asss_ext_begin,
the caller's U, amh_asss_ext_shrink per round, amh_asss_ext_finish;
asss.py:105-131's arbitrary potential_fn) on the GPU.  With U = the library's
own potential of a registry model (amh_potential, bit-identical to the
oracle's) every transition must equal orc_asss_step bit for bit at every
lane-group width -- single launches, in-place runs and thinned collection --
and sample_Pnx must equal orc_asss_sample_pnx.  The shrinkage cap and the
"energy of the accepting round" rule are checked exactly with a stateful
callable; a potential written in torch samples its target."""
import ctypes
import math

import numpy as np
import pytest
import torch

from helpers import ASSS_FIELDS, assert_state_bitequal_nan, make_case

pytestmark = pytest.mark.gpu


def _registry(kind, d, seed=0):
    """A registry kernel bound to the model (for its potential), the oracle
    model and 8 start points."""
    from kernels_amd import ASSS, PRNGKey
    kw, mk, om = make_case(kind, d)
    z8 = np.random.default_rng(seed).uniform(-2, 2, size=(8, om.d)).astype(np.float32)
    kg = ASSS(num_chains=8, **kw)
    st = kg.init(PRNGKey(1), 0, torch.as_tensor(z8), (), mk)
    return kg, st, om


@pytest.mark.parametrize("kind,d,C", [("gaussian", 1, 130), ("gaussian", 3, 37), ("gaussian", 5, 77),
                                      ("gaussian", 17, 65), ("gaussian", 33, 9), ("gaussian", 64, 7),
                                      ("mixture", 1, 130), ("mixture", 3, 37), ("eight_schools", 10, 21)])
def test_host_shrink_matches_oracle_bitexact(kind, d, C, gpu, orc):
    from kernels_amd import ASSS, PRNGKey
    kg, _, om = _registry(kind, d)
    d = om.d
    z0 = np.random.default_rng(0).uniform(-2, 2, size=(C, d)).astype(np.float32)
    ke = ASSS(potential_fn=lambda z: kg.potential(z), num_chains=C, host_shrink=True)
    st = ke.init(PRNGKey(0), 4, torch.as_tensor(z0), (), {})
    ost = orc.init(om, PRNGKey(0), C, init_z=z0)
    torch.cuda.synchronize()
    assert_state_bitequal_nan(st, ost, f"{kind} d={d} init", fields=ASSS_FIELDS)
    rounds = []
    for t in range(8):  # crosses gamma_1 = 1 (keep L) and the warm-up reset at W + 1
        st = ke.sample(st, (), {})
        rounds.append(ke.shrink_rounds)
        orc.asss_step(om, ost, 1, num_warmup=4)
        torch.cuda.synchronize()
        assert_state_bitequal_nan(st, ost, f"{kind} d={d} step {t}", fields=ASSS_FIELDS)
    # every external transition is its own launch sequence (the state goes
    # through memory, L = U diag(dl) stored and re-read), so the oracle runs one
    # step per call: its fused n-step call keeps U between steps
    ke.sample_(st, 5)
    rounds.append(ke.shrink_rounds)
    for _ in range(5):
        orc.asss_step(om, ost, 1, num_warmup=4)
    torch.cuda.synchronize()
    assert_state_bitequal_nan(st, ost, f"{kind} d={d} in place", fields=ASSS_FIELDS)
    st2, cz, cp = ke.run(st, 6, thinning=3, collect_z=True, collect_pe=True)
    rounds.append(ke.shrink_rounds)
    ozs, ops = [], []
    for _ in range(6):
        orc.asss_step(om, ost, 1, num_warmup=4)
        ozs.append(ost.z.copy())
        ops.append(ost.potential_energy.copy())
    torch.cuda.synchronize()
    assert_state_bitequal_nan(st2, ost, f"{kind} d={d} run", fields=ASSS_FIELDS)
    np.testing.assert_array_equal(cz.cpu().numpy().view(np.uint32), np.stack(ozs)[2::3].view(np.uint32))
    np.testing.assert_array_equal(cp.cpu().numpy().view(np.uint32), np.stack(ops)[2::3].view(np.uint32))
    print("shrink rounds", rounds)
    assert all(1 <= r <= 51 for r in rounds)
    assert max(rounds) >= 3, rounds  # the multi-round path was taken


@pytest.mark.parametrize("kind,d", [("mixture", 1), ("gaussian", 5), ("gaussian", 24)])
def test_host_shrink_sample_pnx_bitexact(kind, d, gpu, orc):
    """sample_Pnx around the caller's U (no init() on the external kernel, as
    the reference's notebook uses it) against orc_asss_sample_pnx."""
    from kernels_amd import ASSS, PRNGKey
    kg, st, om = _registry(kind, d)
    kg.sample_(st, 30)
    ad = st.adapt_state
    loc, scale = ad.loc[2].clone(), ad.scale[2].clone()
    ke = ASSS(potential_fn=lambda z: kg.potential(z), host_shrink=True)
    x = np.random.default_rng(3).normal(size=(4, d)).astype(np.float32)
    out = ke.sample_Pnx(PRNGKey(7), x, (loc, scale), n=4, n_samples=33)
    ref = orc.asss_sample_pnx(om, PRNGKey(7), x, loc.cpu().numpy(), scale.cpu().numpy(), 4, 33)
    assert out.shape == (4, 33, d)
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    assert np.mean(np.any(ref != x[:, None, :], axis=-1)) > 0.2


def test_cap_and_accepting_round_rule(gpu):
    """Every re-evaluation of the candidates returns +inf: a chain whose first
    candidate is on the slice stops in round 0 and keeps that candidate with
    the energy round 0 returned for it (later values for its row are ignored);
    every other chain runs into the cap and keeps x(theta = 0) with U0."""
    from kernels_amd import ASSS, PRNGKey
    C, d = 256, 5
    kw, mk, _ = make_case("gaussian", d)
    z0 = torch.as_tensor(np.random.default_rng(0).uniform(-2, 2, size=(C, d)).astype(np.float32))
    kg = ASSS(num_chains=C, **kw)
    st = kg.init(PRNGKey(0), 0, z0, (), mk)
    kg.sample_(st, 20)
    rec = {}

    def U(z):
        if z.shape[0] == 2 * C:
            u = kg.potential(z)
            rec["z"], rec["u"] = z.clone(), u.clone()
            return u
        return torch.full((z.shape[0],), math.inf, device=z.device)

    ke = ASSS(potential_fn=U, num_chains=C, host_shrink=True)
    ke.init(PRNGKey(0), 0, z0, (), {})
    out = ke.sample(st, (), {})
    torch.cuda.synchronize()
    assert ke.shrink_rounds == 51
    bits = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    z, pe = bits(out.z), bits(out.potential_energy)
    x0, x1 = bits(rec["z"][:C]), bits(rec["z"][C:])
    u0, u1 = bits(rec["u"][:C]), bits(rec["u"][C:])
    kept = np.all(z == x0, axis=1)
    moved = np.all(z == x1, axis=1) & ~kept
    assert np.all(kept | moved)
    assert kept.any() and moved.any(), (kept.sum(), moved.sum())
    np.testing.assert_array_equal(pe[kept], u0[kept])
    np.testing.assert_array_equal(pe[moved], u1[moved])
    np.testing.assert_array_equal(out.i.cpu().numpy(), st.i.cpu().numpy() + 1)


def test_torch_potential_samples_target(gpu):
    """U written in torch (the correlated 3-D Gaussian of the ARWMH external
    test): the chains' moments are the target's, and the stored energies are
    U of the stored points."""
    from kernels_amd import ASSS, PRNGKey
    S = torch.tensor([[1.0, 0.5, 0.0], [0.5, 2.0, -0.3], [0.0, -0.3, 0.5]], dtype=torch.float64)
    Pm = torch.linalg.inv(S).to(torch.float32).cuda()
    m = torch.tensor([1.0, -2.0, 0.5], device="cuda")

    def U(z):
        x = z - m
        return 0.5 * ((x @ Pm) * x).sum(-1)

    C = 4096
    k = ASSS(potential_fn=U, num_chains=C, host_shrink=True)
    st = k.init(PRNGKey(3), 0, torch.rand(C, 3) * 4 - 2, (), {})
    k.sample_(st, 300)
    st, cz, _ = k.run(st, 200, thinning=10, collect_z=True)
    z = cz.reshape(-1, 3).double().cpu()
    print("mean error", (z.mean(0) - m.cpu().double()).abs().max().item(),
          "covariance error", (torch.cov(z.T) - S).abs().max().item())
    np.testing.assert_allclose(z.mean(0).numpy(), m.cpu().numpy(), atol=0.05)
    np.testing.assert_allclose(torch.cov(z.T).numpy(), S.numpy(), atol=0.08)
    np.testing.assert_allclose(st.potential_energy.cpu().numpy(), U(st.z).cpu().numpy(), rtol=1e-6, atol=1e-6)


def test_nan_half_space(gpu):
    """U = NaN for z_0 > 0: NaN is +inf on the slice test (asss.py:72-76), so
    no chain is ever stored inside the NaN half (it would hold +inf)."""
    from kernels_amd import ASSS, PRNGKey
    k = ASSS(potential_fn=lambda z: torch.where(z[:, 0] > 0, torch.nan, 0.5 * (z * z).sum(-1)), num_chains=256,
             host_shrink=True)
    s = k.init(PRNGKey(2), 0, -torch.ones(256, 2), (), {})
    k.sample_(s, 100)
    assert bool(torch.isfinite(s.potential_energy).all())


def test_limits_and_driver(gpu):
    import posteriors as P
    from infer_amd import MCMC
    from kernels_amd import ASSS, PRNGKey, _lib
    from kernels_amd._lib import AmhError
    U = lambda z: 0.5 * (z * z).sum(-1)  # noqa: E731
    with pytest.raises(ValueError, match="host_shrink"):
        ASSS(potential_fn=P.correlated_gaussian(4), host_shrink=True)
    with pytest.raises(ValueError, match="host_shrink"):
        ASSS(model=P.eight_schools, host_shrink=True)
    with pytest.raises(ValueError, match="d <= 64"):
        ASSS(potential_fn=U, num_chains=8, host_shrink=True).init(PRNGKey(0), 0, torch.zeros(8, 96), (), {})
    with pytest.raises(AmhError, match="device potential"):
        a = ASSS(potential_fn=U, num_chains=64)
        a.sample(a.init(PRNGKey(0), 0, torch.zeros(64, 4), (), {}))
    # the C entries: a registry-bound handle, a round past the last
    C, d = 16, 4
    kg = ASSS(potential_fn=P.correlated_gaussian(d), num_chains=C)
    st = kg.init(PRNGKey(0), 0, torch.zeros(C, d), (), {})
    n = ctypes.c_int64(0)
    L = _lib.lib()
    _lib.check(L.amh_asss_ext_work_size(d, ctypes.byref(n)))
    dev = st.z.device
    cand = torch.zeros(2, C, d, device=dev)
    work = torch.zeros(C, n.value, device=dev)
    pe = torch.zeros(2, C, device=dev)
    active = torch.zeros(_lib.AMH_ASSS_EXT_ROUNDS, dtype=torch.int32, device=dev)
    s = _lib.stream_ptr(dev.index)
    with pytest.raises(AmhError, match="needs AMH_MODEL_EXTERNAL"):
        _lib.check(L.amh_asss_ext_begin(kg._handle.h, C, kg._c_state(st), _lib.ptr(cand), _lib.ptr(work),
                                        _lib.ptr(active), s), kg._handle.h)
    ke = ASSS(potential_fn=U, num_chains=C, host_shrink=True)
    ke.init(PRNGKey(0), 0, torch.zeros(C, d), (), {})
    rc = L.amh_asss_ext_shrink(ke._handle.h, C, _lib.ptr(pe), 51, _lib.ptr(cand), _lib.ptr(work), _lib.ptr(active), s)
    assert rc == -1  # AMH_EINVAL
    assert b"round" in L.amh_last_error(ke._handle.h)
    m = MCMC(ASSS(potential_fn=U, host_shrink=True, num_chains=64), num_warmup=20, num_samples=20, thinning=2)
    m.run(PRNGKey(0), init_params=torch.rand(64, d) * 4 - 2)
    z = m.get_samples(group_by_chain=True)
    z = z if torch.is_tensor(z) else torch.as_tensor(np.asarray(z))
    assert tuple(z.transpose(0, 1).shape) == (10, 64, d)
    assert bool(torch.isfinite(z).all())
