"""Pooled ASSS with the caller's potential (PooledASSS(host_shrink=True):
amh_pooled_asss_ext_begin, the caller's U, amh_asss_ext_shrink per round,
amh_pooled_asss_ext_finish, amh_pooled_asss_ext_update) on the GPU.  The
checker is the registry PooledASSS with the same key and start, and the
potential handed to the external sampler is the library's own (amh_potential
of a registry twin bound to the same model), so a transition must be the fused
kernel's byte for byte: z, pe, the sums and the update at K = 1; z / pe and the
step-order sum of single-step sums for a block.  The shrinkage cap and the
"energy of the accepting round" rule are checked exactly with a stateful
callable; a potential written in torch samples its target; run, checkpoints,
two ranks, sample_Pnx, the limits and the MCMC driver work on top."""
import ctypes
import math

import numpy as np
import pytest
import torch

from helpers import make_case

pytestmark = pytest.mark.gpu


def _leaves(s):
    a = s.adapt_state
    return dict(i=s.i, z=s.z, potential_energy=s.potential_energy, mean_accept_prob=s.mean_accept_prob, loc=a.loc,
                scale=a.scale, log_step_size=a.log_step_size, as_change=s.as_change, cov=s.cov)


SHARED = ("i", "mean_accept_prob", "loc", "scale", "log_step_size", "as_change", "cov")


def _bytes(t):
    return t.detach().cpu().numpy().tobytes()


def _assert_same(a, b, what, names=None):
    torch.cuda.synchronize()
    la, lb = _leaves(a), _leaves(b)
    for n in names or la:
        assert _bytes(la[n]) == _bytes(lb[n]), f"{what}: {n} differs"


def _c_state(st, i=None, z=None, pe=None):
    from kernels_amd import _lib
    a = st.adapt_state
    return _lib.AmhPooledState((st.i if i is None else i).data_ptr(), (st.z if z is None else z).data_ptr(),
                               (st.potential_energy if pe is None else pe).data_ptr(), st.rng_key.data_ptr(),
                               st.mean_accept_prob.data_ptr(), a.loc.data_ptr(), a.scale.data_ptr(),
                               a.log_step_size.data_ptr(), st.as_change.data_ptr(), st.cov.data_ptr())


def _pair(kind, d, C, K=1, num_warmup=0, seed=0, **opts):
    """-> (registry sampler, its state, external sampler around the registry
    sampler's own potential, its state): same key, same start."""
    from kernels_amd import PooledASSS, PRNGKey
    kw, mk, om = make_case(kind, d)
    z0 = torch.as_tensor(np.random.default_rng(seed).uniform(-2, 2, size=(C, om.d)).astype(np.float32))
    kr = PooledASSS(num_chains=C, sync_every=K, **kw)
    sr = kr.init(PRNGKey(seed), num_warmup, z0, (), mk)
    ke = PooledASSS(potential_fn=lambda z: kr.potential(z), num_chains=C, sync_every=K, host_shrink=True, **opts)
    se = ke.init(PRNGKey(seed), num_warmup, z0, (), {})
    return kr, sr, ke, se


@pytest.mark.parametrize("kind,d,C", [("gaussian", 1, 65), ("gaussian", 2, 5), ("gaussian", 7, 517),
                                      ("gaussian", 7, 4097), ("gaussian", 33, 300), ("gaussian", 64, 300),
                                      ("eight_schools", 10, 70)])
def test_single_transitions_equal_the_registry_sampler(kind, d, C, gpu):
    """K = 1, num_warmup = 4, 8 blocks alternating sample and sample_(1)
    (crosses gamma_1 = 1 and the warm-up reset): every leaf and the sums are
    the registry sampler's bytes after every block.  d = 1: S^1, a 1 x 1
    factor; (2, 5): fewer chains than one chunk, a rank-deficient first block
    keeps the factor; (7, 517): 33 chunks, ragged last one; (7, 4097):
    pooled_cpw = 2; d = 33: odd d, padded LDS rows; d = 64: the full wave and
    the d = 64 instance; eight schools: a non-Gaussian potential."""
    kr, sr, ke, se = _pair(kind, d, C, num_warmup=4)
    _assert_same(se, sr, f"{kind} d={d} init")
    rounds = []
    for b in range(8):
        if b % 2 == 0:
            sr, se = kr.sample(sr), ke.sample(se)
        else:
            kr.sample_(sr, 1)
            ke.sample_(se, 1)
        _assert_same(se, sr, f"{kind} d={d} C={C} block {b + 1}")
        assert _bytes(ke._sums) == _bytes(kr._sums), f"{kind} d={d} C={C} block {b + 1}: sums differ"
        rounds.append(ke.shrink_rounds)
        assert 1 <= ke.shrink_rounds <= 51
    print("shrink rounds", rounds)
    assert int(se.i[0]) == 8
    assert max(rounds) >= 3, rounds  # the multi-round path was taken


def _registry_single_steps(kr, st, K):
    """The block's K frozen transitions of `st` as K single-step
    amh_pooled_asss_stats_k launches on the registry handle at i + t ->
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


@pytest.mark.parametrize("d,C,K", [(7, 517, 4), (64, 300, 2)])
def test_blocks(d, C, K, gpu):
    """Two blocks of K transitions.  z / pe are the registry sampler's bytes
    from the same state (a chain's path does not read the sums); the block's
    sums are the float64 sum, in step order, of the K single-step sums of the
    registry handle; the shared leaves are amh_pooled_asss_update_k's from
    those sums."""
    from kernels_amd import _lib
    kr, _, ke, se = _pair("gaussian", d, C, K=K)
    for b in range(2):
        fused = kr.sample(se)  # the fused K-block from the external sampler's state
        z1, pe1, total = _registry_single_steps(kr, se, K)
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


def test_cap_and_accepting_round_rule(gpu):
    """Every re-evaluation of the candidates returns +inf: a chain whose first
    candidate is on the slice stops in round 0 and keeps that candidate with
    the energy round 0 returned for it; every other chain runs into the cap
    and keeps x(theta = 0) with U0.  The sums count the chains and the moves."""
    from kernels_amd import PooledASSS, PRNGKey
    C, d = 256, 5
    kw, mk, _ = make_case("gaussian", d)
    z0 = torch.as_tensor(np.random.default_rng(0).uniform(-2, 2, size=(C, d)).astype(np.float32))
    kg = PooledASSS(num_chains=C, **kw)
    st = kg.init(PRNGKey(0), 0, z0, (), mk)
    kg.sample_(st, 20)  # a warm shared state
    rec = {}

    def U(z):
        if z.shape[0] == 2 * C:
            u = kg.potential(z)
            rec["z"], rec["u"] = z.clone(), u.clone()
            return u
        return torch.full((z.shape[0],), math.inf, device=z.device)

    ke = PooledASSS(potential_fn=U, num_chains=C, host_shrink=True)
    ke.init(PRNGKey(0), 0, z0, (), {})
    out = ke.sample(st)
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
    sums = ke._sums.cpu().numpy()
    assert sums[-1] == float(C) and sums[-2] == float(moved.sum()), (sums[-2:], moved.sum())
    assert int(out.i[0]) == int(st.i[0]) + 1


# the correlated 3-D Gaussian of the per-chain external tests, written with
# elementwise operations only, so that U of a row does not depend on the batch
_S3 = np.array([[1.0, 0.5, 0.0], [0.5, 2.0, -0.3], [0.0, -0.3, 0.5]])
_P3 = np.linalg.inv(_S3).astype(np.float32)
_M3 = (1.0, -2.0, 0.5)


def _U3(z):
    x = [z[:, j] - _M3[j] for j in range(3)]
    u = torch.zeros_like(z[:, 0])
    for j in range(3):
        for k in range(3):
            u = u + float(_P3[j, k]) * (x[j] * x[k])
    return 0.5 * u


def test_torch_potential_samples_target(gpu):
    """C = 2048 chains, 300 steps: across chains every coordinate's mean is
    within 5 standard errors and its variance within 5 Sigma_jj sqrt(2 / C)
    of the target's; as_change falls; the stored energies are U of the stored
    points."""
    from kernels_amd import PooledASSS, PRNGKey
    C = 2048
    k = PooledASSS(potential_fn=_U3, num_chains=C, host_shrink=True)
    st = k.init(PRNGKey(3), 0, torch.as_tensor(np.random.default_rng(1).uniform(-2, 2, size=(C, 3)).astype(np.float32)),
                (), {})
    k.sample_(st, 20)
    asc20 = float(st.as_change[0])
    k.sample_(st, 280)
    torch.cuda.synchronize()
    for leaf in (st.z, st.potential_energy, st.adapt_state.loc, st.adapt_state.scale, st.cov, st.as_change):
        assert bool(torch.isfinite(leaf).all())
    x = st.z.cpu().numpy().astype(np.float64)
    var, mean = np.diagonal(_S3), np.array(_M3)
    print("mean error / se", np.abs(x.mean(0) - mean) / np.sqrt(var / C), "variance ratio", x.var(0, ddof=1) / var)
    assert np.all(np.abs(x.mean(0) - mean) <= 5 * np.sqrt(var / C))
    assert np.all(np.abs(x.var(0, ddof=1) - var) <= 5 * var * np.sqrt(2 / C))
    assert float(st.as_change[0]) < asc20
    np.testing.assert_allclose(st.potential_energy.cpu().numpy(), _U3(st.z).cpu().numpy(), rtol=1e-6)


def test_nan_half_space(gpu):
    """U = NaN for z_0 > 0: NaN is +inf on the slice test (asss.py:72-76), so
    no chain is ever stored inside the NaN half, and the shared state stays
    finite."""
    from kernels_amd import PooledASSS, PRNGKey
    k = PooledASSS(potential_fn=lambda z: torch.where(z[:, 0] > 0, torch.nan, 0.5 * (z * z).sum(-1)), num_chains=256,
                   host_shrink=True)
    s = k.init(PRNGKey(2), 0, -torch.ones(256, 2), (), {})
    k.sample_(s, 100)
    torch.cuda.synchronize()
    assert int(s.i[0]) == 100
    for name, leaf in _leaves(s).items():
        assert bool(torch.isfinite(leaf).all()), name


def _ext_pair(d, C, K, seed=1, **opts):
    """Two identical external samplers around the library's Gaussian potential."""
    import posteriors as P
    from kernels_amd import ARWMH, PooledASSS, PRNGKey
    kg = ARWMH(potential_fn=P.correlated_gaussian(d), num_chains=1)
    kg.init(PRNGKey(0), 0, torch.zeros(1, d), (), {})
    z0 = torch.as_tensor(np.random.default_rng(seed).uniform(-2, 2, size=(C, d)).astype(np.float32))
    out = []
    for _ in range(2):
        k = PooledASSS(potential_fn=lambda z: kg.potential(z), num_chains=C, sync_every=K, host_shrink=True, **opts)
        out.append((k, k.init(PRNGKey(seed), 0, z0, (), {})))
    return out


def test_run_matches_sample(gpu):
    """PooledASSS.run (collect at block ends) equals sample_ block by block."""
    (a, sa), (b, sb) = _ext_pair(16, 500, 2)
    out, cz, cp = a.run(sa, 13 * 2, thinning=4, collect_z=True, collect_pe=True)
    assert cz.shape == (6, 500, 16) and cp.shape == (6, 500)
    for t in range(6):
        b.sample_(sb, 4)
        assert torch.equal(cz[t], sb.z) and torch.equal(cp[t], sb.potential_energy)
    b.sample_(sb, 2)
    _assert_same(out, sb, "run")
    assert int(out.i[0]) == 26 and int(sa.i[0]) == 0  # run() leaves its input alone


@pytest.mark.parametrize("overlap", [False, True])
def test_checkpoint_resumes_byte_for_byte(overlap, gpu, tmp_path):
    from kernels_amd import load_state, save_state
    (a, sa), (b, sb) = _ext_pair(16, 400, 2, overlap=overlap)
    a.sample_(sa, 12)
    b.sample_(sb, 6)
    path = save_state(str(tmp_path / "ck"), sb, kernel=b)
    (c, sc), _ = _ext_pair(16, 400, 2, overlap=overlap)
    sc = load_state(path, device=gpu, kernel=c)
    c.sample_(sc, 6)
    _assert_same(sa, sc, f"resume overlap={overlap}")


def _U_rank(z):
    """A tridiagonal Gaussian potential from elementwise operations and a
    column-by-column sum: a row's U does not depend on the batch it is in, so
    a shard evaluates what the whole run evaluates."""
    t = 0.5 * z * z
    t[:, 1:] += 0.3 * z[:, 1:] * z[:, :-1]
    u = t[:, 0].clone()
    for j in range(1, z.shape[1]):
        u = u + t[:, j]
    return u


def _rank_worker(rank, world, port, C, d, out_path, align):
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)  # the ranks share the box's one GPU
    from kernels_amd import PooledASSS, PRNGKey
    from kernels_amd.distributed import shard_range
    off, cnt = shard_range(C, rank, world, align=align)
    z0 = torch.as_tensor(np.random.default_rng(0).uniform(-2, 2, size=(C, d)).astype(np.float32))
    k = PooledASSS(potential_fn=_U_rank, num_chains=cnt, chain_offset=off, device=torch.device("cuda", 0),
                   host_shrink=True)
    st = k.init(PRNGKey(2), 0, z0[off:off + cnt].cuda(), (), {})
    k.sample_(st, 1)
    np.savez(f"{out_path}.{rank}.npz", z=st.z.cpu().numpy(), pe=st.potential_energy.cpu().numpy(),
             L=st.adapt_state.scale.cpu().numpy(), mu=st.adapt_state.loc.cpu().numpy(), i=st.i.cpu().numpy())
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_one_block(gpu, tmp_path):
    """d = 32, C = 2001, one block on two ranks with chunk-aligned shards: every
    chain's z / pe is the one-rank external run's byte for byte, and loc /
    scale agree to one float32 ulp (only the double association of the sums
    across ranks differs)."""
    import socket
    import torch.multiprocessing as mp
    from kernels_amd import PooledASSS, PRNGKey, pooled_chunk
    C, d = 2001, 32
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "g")
    mp.start_processes(_rank_worker, args=(2, port, C, d, out, pooled_chunk(d, C)), nprocs=2, join=True,
                       start_method="spawn")
    parts = [np.load(f"{out}.{rank}.npz") for rank in range(2)]
    assert parts[1]["L"].tobytes() == parts[0]["L"].tobytes() and parts[1]["mu"].tobytes() == parts[0]["mu"].tobytes()
    z0 = torch.as_tensor(np.random.default_rng(0).uniform(-2, 2, size=(C, d)).astype(np.float32))
    k = PooledASSS(potential_fn=_U_rank, num_chains=C, host_shrink=True)
    st = k.init(PRNGKey(2), 0, z0.to(gpu), (), {})
    k.sample_(st, 1)
    torch.cuda.synchronize()
    z, pe = np.concatenate([p["z"] for p in parts]), np.concatenate([p["pe"] for p in parts])
    assert int(parts[0]["i"][0]) == 1 and z.shape == (C, d)
    assert z.tobytes() == st.z.cpu().numpy().tobytes()
    assert pe.tobytes() == st.potential_energy.cpu().numpy().tobytes()
    for got, ref in ((parts[0]["mu"], st.adapt_state.loc.cpu().numpy()),
                     (parts[0]["L"], st.adapt_state.scale.cpu().numpy())):
        assert np.all(np.abs(got - ref) <= np.spacing(np.abs(ref)))


def test_sample_pnx_is_asss_sample_pnx(gpu):
    """sample_Pnx of PooledASSS(host_shrink=True) with no init() is
    ASSS(host_shrink=True).sample_Pnx for the same callable."""
    from kernels_amd import ASSS, PooledASSS, PRNGKey
    d = 5
    kw, mk, _ = make_case("gaussian", d)
    kg = ASSS(num_chains=8, **kw)
    st = kg.init(PRNGKey(1), 0, torch.as_tensor(np.random.default_rng(0).uniform(-2, 2, size=(8, d))
                                                .astype(np.float32)), (), mk)
    kg.sample_(st, 30)
    loc, scale = st.adapt_state.loc[2].clone(), st.adapt_state.scale[2].clone()
    U = lambda z: kg.potential(z)  # noqa: E731
    x = np.random.default_rng(3).normal(size=(4, d)).astype(np.float32)
    got = PooledASSS(potential_fn=U, host_shrink=True).sample_Pnx(PRNGKey(7), x, (loc, scale), n=4, n_samples=33)
    ref = ASSS(potential_fn=U, host_shrink=True).sample_Pnx(PRNGKey(7), x, (loc, scale), n=4, n_samples=33)
    torch.cuda.synchronize()
    assert got.shape == (4, 33, d) and _bytes(got) == _bytes(ref)
    assert np.mean(np.any(ref.cpu().numpy() != x[:, None, :], axis=-1)) > 0.2


def test_limits_and_driver(gpu):
    import posteriors as P
    from infer_amd import MCMC
    from kernels_amd import ARWMH, PooledASSS, PRNGKey, _lib
    U = lambda z: 0.5 * (z * z).sum(-1)  # noqa: E731
    with pytest.raises(ValueError, match="host_shrink"):
        PooledASSS(potential_fn=P.correlated_gaussian(4), host_shrink=True)
    with pytest.raises(ValueError, match="host_shrink"):
        PooledASSS(model=P.eight_schools, host_shrink=True)
    with pytest.raises(ValueError):
        PooledASSS(potential_fn=U)
    with pytest.raises(ValueError, match="exact_sums"):
        PooledASSS(potential_fn=U, host_shrink=True, exact_sums=True)
    with pytest.raises(ValueError, match="d <= 64"):
        PooledASSS(potential_fn=U, num_chains=8, host_shrink=True).init(PRNGKey(0), 0, torch.zeros(8, 96), (), {})
    with pytest.raises(ValueError, match="init_params"):
        PooledASSS(potential_fn=U, num_chains=8, host_shrink=True).init(PRNGKey(0), 0, None, (), {})
    # the C entries: a registry-bound handle, then an external handle at d = 65
    C, d = 32, 8
    kr = PooledASSS(potential_fn=P.correlated_gaussian(d), num_chains=C)
    st = kr.init(PRNGKey(0), 0, torch.zeros(C, d), (), {})
    L = _lib.lib()
    n = ctypes.c_int64(0)
    _lib.check(L.amh_asss_ext_work_size(d, ctypes.byref(n)))
    cand = torch.zeros(2, C, d, device=gpu)
    work = torch.zeros(C, n.value, device=gpu)
    active = torch.zeros(_lib.AMH_ASSS_EXT_ROUNDS, dtype=torch.int32, device=gpu)
    sums = torch.zeros(kr._sums.shape[0], dtype=torch.float64, device=gpu)
    cs, s = _c_state(st), _lib.stream_ptr(gpu.index)
    big = ARWMH(potential_fn=U, num_chains=C)
    big.init(PRNGKey(0), 0, torch.zeros(C, 65), (), {})
    for h, msg in ((kr._handle.h, "needs AMH_MODEL_EXTERNAL"), (big._handle.h, "dim")):
        calls = (lambda: L.amh_pooled_asss_ext_begin(h, C, ctypes.byref(cs), 0, _lib.ptr(cand), _lib.ptr(work),
                                                     _lib.ptr(active), s),
                 lambda: L.amh_pooled_asss_ext_finish(h, C, ctypes.byref(cs), _lib.ptr(cand), _lib.ptr(work),
                                                      _lib.ptr(st.z), _lib.ptr(st.potential_energy), _lib.ptr(sums),
                                                      0, s),
                 lambda: L.amh_pooled_asss_ext_update(h, _lib.ptr(sums), ctypes.byref(cs), ctypes.byref(cs), 1, s))
        for call in calls:
            assert call() == -1  # AMH_EINVAL
            assert msg in L.amh_last_error(h).decode(), L.amh_last_error(h)
    ke = PooledASSS(potential_fn=U, num_chains=C, host_shrink=True)
    se = ke.init(PRNGKey(0), 0, torch.zeros(C, d), (), {})
    rc = L.amh_pooled_asss_ext_begin(ke._handle.h, C, ctypes.byref(_c_state(se)), -1, _lib.ptr(cand), _lib.ptr(work),
                                     _lib.ptr(active), s)
    assert rc == -1 and b"amh_pooled_asss_ext_begin" in L.amh_last_error(ke._handle.h)
    m = MCMC(PooledASSS(potential_fn=U, host_shrink=True, num_chains=64), num_warmup=20, num_samples=20, thinning=2)
    m.run(PRNGKey(0), init_params=torch.rand(64, d) * 4 - 2)
    z = m.get_samples(group_by_chain=True)
    z = z if torch.is_tensor(z) else torch.as_tensor(np.asarray(z))
    assert tuple(z.transpose(0, 1).shape) == (10, 64, d)
    assert bool(torch.isfinite(z).all())
