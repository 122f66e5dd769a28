"""Pooled ASSS (kernels_amd.PooledASSS; amh_pooled_asss_*) on the GPU: every
chain-step, the sums and the update against the float64 restatement
tests/pooled_asss_np.py, the byte equalities between its entry points, the
kept factor, the target's moments, two ranks, and the limits.
tests/test_pooled_asss_f64.py checks, on the reference alone, that the cases
below start where a float32 evaluation follows the float64 slice path."""
import ctypes

import numpy as np
import pytest
import torch

import pooled_asss_bits as bits
import pooled_asss_np as pa
import pooled_np as pnp
from helpers import apply_shared, make_case, shared_to_host

pytestmark = pytest.mark.gpu

SEED = pa.SEED


def _c_state(st, i=None, z=None, pe=None):
    from kernels_amd import _lib
    a = st.adapt_state
    return _lib.AmhPooledState((st.i if i is None else i).data_ptr(), (st.z if z is None else z).data_ptr(),
                               (st.potential_energy if pe is None else pe).data_ptr(), st.rng_key.data_ptr(),
                               st.mean_accept_prob.data_ptr(), a.loc.data_ptr(), a.scale.data_ptr(),
                               a.log_step_size.data_ptr(), st.as_change.data_ptr(), st.cov.data_ptr())


def _single_steps(k, st, K):
    """The block's K frozen transitions as K single-step
    amh_pooled_asss_stats_k launches at i + t -> (z after each, pe after each)."""
    from kernels_amd import _lib
    dev = st.z.device
    z, pe, zs, pes = st.z, st.potential_energy, [], []
    sums = torch.zeros(k._sums.shape[0], dtype=torch.float64, device=dev)
    for t in range(K):
        it = st.i + t
        zo, po = torch.empty_like(z), torch.empty_like(pe)
        rc = _lib.lib().amh_pooled_asss_stats_k(k._handle.h, z.shape[0], ctypes.byref(_c_state(st, it, z, pe)), 1,
                                                _lib.ptr(zo), _lib.ptr(po), _lib.ptr(sums),
                                                _lib.stream_ptr(dev.index))
        _lib.check(rc, k._handle.h)
        torch.cuda.synchronize()
        z, pe = zo, po
        zs.append(zo.cpu().numpy())
        pes.append(po.cpu().numpy())
    return zs, pes


def _check_update(before, after, sums, d, K):
    """The update teacher-forced on the kernel's sums and a float32 gamma."""
    assert int(after["i"][0]) == int(before["i"][0]) + K
    assert after["lam"].tobytes() == before["lam"].tobytes()  # log_step_size: copied through
    L0, Lk = pnp.unpack(before["L"], d), pnp.unpack(after["L"], d)
    mu0, muk = before["mu"].astype(np.float64), after["mu"].astype(np.float64)
    kept = after["L"].tobytes() == before["L"].tobytes() and after["cov"].tobytes() == before["cov"].tobytes()
    asc_ref = float(np.linalg.norm(muk - mu0) + np.linalg.norm(Lk - L0, "fro"))
    best = None
    for g in pnp.gamma_candidates(pnp.block_n(int(before["i"][0]), K, 0)):
        up = pa.update(sums, before, K=K, gamma=g)
        q = dict(mu=float(np.max(np.abs(muk - up.mu) / pnp.bounds.scalar(up.terms["mu"]))),
                 macc=abs(float(after["macc"][0]) - up.macc) / pnp.bounds.scalar(up.terms["macc"]))
        if kept:
            q["keep"] = float(np.inf) if up.refactored and up.pivot_ratio >= pnp.PIVOT_RATIO else 0.0
        else:
            covk = pnp.unpack_sym(after["cov"], d)
            q["cov"] = float(np.max(np.abs(covk - up.cov_new) / (pnp.COV_RTOL * np.abs(up.cov_new))))
            q["factor"] = float(np.max(np.abs(Lk @ Lk.T - up.cov_new) / pnp.bounds.factor(Lk, up.cov_new, d)))
            if not np.all(np.diagonal(Lk) > 0):
                q["factor"] = float(np.inf)
        q["asc"] = abs(float(after["asc"][0]) - asc_ref) / pa.as_change_bound(muk, mu0, Lk, L0, asc_ref, d)
        if best is None or max(q.values()) < max(best.values()):
            best = q
    print("update: " + " ".join(f"{k}={v:.3g}" for k, v in best.items()))
    assert all(v <= 1.0 for v in best.values()), best


@pytest.mark.parametrize("kind,d,C,K", pa.CASES)
def test_pooled_asss_against_float64(kind, d, C, K, gpu):
    """Three blocks from a warm start in the typical set.  d = 7: 33 chunks
    with a ragged last one, and a K-block; eight schools: a non-Gaussian
    potential; d = 33: odd d, padded LDS rows; d = 64: the full wave; d = 1:
    S^1 and a 1 x 1 factor; d = 2: the smallest multi-coordinate d.

    Per chain-step the tolerances are those tests/test_asss.py holds the
    float32 oracle to against the same literal (z rtol 1e-4 / atol 1e-5, pe
    rtol 1e-4 / atol 1e-4), the reference teacher-forced on the kernel's z of
    the step before; a chain on another slice path (endpoint far, as there) is
    skipped.  The sums are bounded against the float64 sums of the kernel's z
    history, the update against the float64 update of the kernel's sums."""
    from kernels_amd import PooledASSS, PRNGKey
    kw, mk, _ = make_case(kind, d)
    om, U, keys, z0, sh = pa.warm_case(kind, d, C, K)
    d = om.d
    k = PooledASSS(num_chains=C, sync_every=K, **kw)
    st = apply_shared(k.init(PRNGKey(SEED), 0, torch.as_tensor(z0), (), mk), sh)
    assert np.array_equal(st.rng_key.cpu().numpy().view(np.uint32), keys)
    for b in range(3):
        before = shared_to_host(st)
        z_in = st.z.cpu().numpy()
        hz, hpe = _single_steps(k, st, K)
        st = k.sample(st)
        torch.cuda.synchronize()
        z, pe, sums = st.z.cpu().numpy(), st.potential_energy.cpu().numpy(), k._sums.cpu().numpy()
        # a chain's path does not depend on the sums: K single steps are the block, byte for byte
        assert hz[-1].tobytes() == z.tobytes() and hpe[-1].tobytes() == pe.tobytes(), f"block {b + 1}"
        zs = np.stack([z_in] + hz)
        # ---- per chain-step
        L0, mu32 = pnp.unpack(before["L"], d), before["mu"]
        skipped = np.zeros(C, bool)
        S_a = 0.0
        for t in range(K):
            xr, per, ni = pa.step(U, int(before["i"][0]) + t, zs[t].astype(np.float64), keys, mu32, L0)
            S_a += float(pa.moved(ni).sum())
            far = ~np.all(np.isclose(zs[t + 1], xr, rtol=1e-3, atol=1e-3), axis=1)
            skipped |= far
            ok = ~far
            np.testing.assert_allclose(zs[t + 1][ok], xr[ok], rtol=1e-4, atol=1e-5)
            np.testing.assert_allclose(hpe[t][ok], per[ok], rtol=1e-4, atol=1e-4)
        print(f"block {b + 1}: {int(skipped.sum())} of {C} chains on another slice path")
        assert skipped.sum() <= max(1, C * K // 50)
        # ---- sums against the kernel's z history
        S_d, S_dd, Sa, N = pnp.split_sums(sums, d)
        R_d, R_dd, A_d, A_dd = pnp.sums_of(zs[1:], mu32)
        assert N == float(K * C) and Sa == S_a
        e_d = float(np.max(np.abs(S_d - R_d) / pa.lane_sum_bound(A_d, d, C, K)))
        e_dd = float(np.max(np.abs(S_dd - R_dd) / pa.lane_sum_bound(A_dd, d, C, K)))
        print(f"block {b + 1}: S_d={e_d:.3g} S_dd={e_dd:.3g} of their bounds")
        assert e_d <= 1.0 and e_dd <= 1.0
        if d < 64:  # the lane form's bound is pooled_np's own below d = 64
            assert np.array_equal(pa.lane_sum_bound(A_dd, d, C, K), pnp.bounds.S_dd(A_dd, d, C, K))
        # ---- update from the kernel's own sums
        _check_update(before, shared_to_host(st), sums, d, K)


@pytest.fixture(scope="module")
def recorded_bits():
    return np.load(bits.PATH)


@pytest.mark.parametrize("kind,d,C,K", bits.CASES)
def test_fused_blocks_equal_the_recorded_bits(kind, d, C, K, gpu, recorded_bits):
    """Three blocks from init (PRNGKey(7), num_warmup = 4) against
    tests/golden/pooled_asss_bits.npz, byte for byte: per block the sums, the
    shared leaves and pe, and z after the last block.  The fixture was recorded
    (tests/golden/make_pooled_asss_bits.py) with the build before the fused
    transition and its external twin came to share the slice walk and the
    chunk scaffold, which their mutual byte equality no longer sees into."""
    got = bits.run(kind, d, C, K)
    prefix = bits.case_id(kind, d, C, K) + "/"
    names = [n[len(prefix):] for n in recorded_bits.files if n.startswith(prefix)]
    assert sorted(names) == sorted(got) and len(names) == 1 + bits.BLOCKS * 9
    for name in names:
        ref = recorded_bits[prefix + name]
        assert got[name].dtype == ref.dtype and got[name].shape == ref.shape, name
        assert got[name].tobytes() == ref.tobytes(), name


def _gauss_pair(d, C, K, gpu, seed=1, **opts):
    import posteriors as P
    from kernels_amd import PooledASSS, PRNGKey
    g = P.correlated_gaussian(d)
    z0 = torch.as_tensor(np.random.default_rng(seed).uniform(-2, 2, size=(C, d)).astype(np.float32)).to(gpu)
    out = []
    for _ in range(2):
        k = PooledASSS(potential_fn=g, num_chains=C, sync_every=K, **opts)
        out.append((k, k.init(PRNGKey(seed), 0, z0, (), {})))
    return out


def _same(a, b):
    torch.cuda.synchronize()
    for x, y in ((a.i, b.i), (a.z, b.z), (a.potential_energy, b.potential_energy),
                 (a.mean_accept_prob, b.mean_accept_prob), (a.as_change, b.as_change), (a.cov, b.cov)) + \
            tuple(zip(a.adapt_state, b.adapt_state)):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


@pytest.mark.parametrize("d,C,K", [(16, 999, 1), (16, 999, 4), (64, 300, 2)])
def test_sample_inplace_and_step_entry_agree(d, C, K, gpu):
    """Out-of-place sample (stats -> update per block), in-place sample_
    (amh_pooled_asss_step_k) and the stats -> update loop through the C
    entries give the same bytes; two identical runs are equal."""
    from kernels_amd import _lib
    (a, sa), (b, sb) = _gauss_pair(d, C, K, gpu)
    (c, sc), (e, se) = _gauss_pair(d, C, K, gpu)
    for _ in range(5):
        sa = a.sample(sa)
    b.sample_(sb, 5 * K)
    _same(sa, sb)
    e.sample_(se, 5 * K)
    _same(sb, se)
    cs, dev = _c_state(sc), sc.z.device.index
    for _ in range(5):
        _lib.check(_lib.lib().amh_pooled_asss_stats_k(c._handle.h, C, ctypes.byref(cs), K, _lib.ptr(sc.z),
                                                      _lib.ptr(sc.potential_energy), _lib.ptr(c._bufs[0]),
                                                      _lib.stream_ptr(dev)), c._handle.h)
        _lib.check(_lib.lib().amh_pooled_asss_update_k(c._handle.h, _lib.ptr(c._bufs[0]), ctypes.byref(cs),
                                                       ctypes.byref(cs), K, _lib.stream_ptr(dev)), c._handle.h)
    _same(sb, sc)
    assert int(sb.i[0]) == 5 * K and np.all(np.isfinite(sb.z.cpu().numpy()))


def test_run_matches_sample(gpu):
    """PooledASSS.run (collect at block ends) equals sample_ block by block."""
    (a, sa), (b, sb) = _gauss_pair(16, 500, 2, gpu)
    out, cz, cp = a.run(sa, 13 * 2, thinning=4, collect_z=True, collect_pe=True)
    assert cz.shape == (6, 500, 16) and cp.shape == (6, 500)
    for t in range(6):
        b.sample_(sb, 4)
        assert torch.equal(cz[t], sb.z) and torch.equal(cp[t], sb.potential_energy)
    b.sample_(sb, 2)
    _same(out, sb)
    assert int(out.i[0]) == 26 and int(sa.i[0]) == 0  # run() leaves its input alone


def test_sample_pnx_is_asss_sample_pnx(gpu):
    """A frozen shared state is exactly ASSS.sample_Pnx's argument."""
    import posteriors as P
    from kernels_amd import ASSS, PRNGKey
    (a, sa), _ = _gauss_pair(16, 300, 1, gpu)
    a.sample_(sa, 30)
    x = torch.as_tensor(np.random.default_rng(3).normal(size=(5, 16)).astype(np.float32))
    got = a.sample_Pnx(PRNGKey(4), x, sa.adapt_state, n=3, n_samples=40)
    ref_k = ASSS(potential_fn=P.correlated_gaussian(16))
    ref = ref_k.sample_Pnx(PRNGKey(4), x, (sa.adapt_state.loc, sa.adapt_state.scale), n=3, n_samples=40)
    torch.cuda.synchronize()
    assert got.shape == (5, 40, 16) and got.cpu().numpy().tobytes() == ref.cpu().numpy().tobytes()
    assert "Potential Energy" in a.get_diagnostics_str(sa)


@pytest.mark.parametrize("overlap", [False, True])
def test_checkpoint_resumes_byte_for_byte(overlap, gpu, tmp_path):
    from kernels_amd import load_state, save_state
    (a, sa), (b, sb) = _gauss_pair(16, 400, 2, gpu, overlap=overlap)
    a.sample_(sa, 12)
    b.sample_(sb, 6)
    path = save_state(str(tmp_path / "ck"), sb, kernel=b)
    (c, sc), _ = _gauss_pair(16, 400, 2, gpu, overlap=overlap)
    sc = load_state(path, device=gpu, kernel=c)
    c.sample_(sc, 6)
    _same(sa, sc)


def test_first_block_keeps_a_rank_deficient_factor(gpu):
    """d = 16, C = 8, first block: gamma = 1 and Sigma' = S_dd / N has rank 8,
    so scale and cov are kept, loc moves, as_change = ||mu' - mu||."""
    (a, sa), _ = _gauss_pair(16, 8, 1, gpu)
    L0, cov0 = sa.adapt_state.scale.cpu().numpy().copy(), sa.cov.cpu().numpy().copy()
    mu0 = sa.adapt_state.loc.cpu().numpy().copy()
    out = a.sample(sa)
    torch.cuda.synchronize()
    assert out.adapt_state.scale.cpu().numpy().tobytes() == L0.tobytes()
    assert out.cov.cpu().numpy().tobytes() == cov0.tobytes()
    mu1 = out.adapt_state.loc.cpu().numpy()
    assert np.all(mu1 != mu0)
    np.testing.assert_allclose(mu1, out.z.cpu().numpy().astype(np.float64).mean(0), rtol=1e-6, atol=1e-7)
    ref = float(np.linalg.norm(mu1.astype(np.float64) - mu0))
    assert abs(float(out.as_change[0]) - ref) <= pa.as_change_bound(mu1, mu0, 0 * L0, 0 * L0, ref, 16)
    assert int(out.i[0]) == 1


def test_samples_the_correlated_gaussian(gpu):
    """correlated_gaussian(16), 2048 chains, 300 steps: across chains every
    coordinate's mean is within 5 standard errors and its variance within
    5 Sigma_jj sqrt(2 / C) of the target's; as_change falls."""
    import posteriors as P
    C, d = 2048, 16
    (a, sa), _ = _gauss_pair(d, C, 1, gpu)
    g = P.correlated_gaussian(d)
    ref = pnp.gaussian_model(g.pack("cpu")[0].numpy(), d)
    cov, mean = np.linalg.inv(ref.P), ref.m
    a.sample_(sa, 20)
    asc20 = float(sa.as_change[0])
    a.sample_(sa, 280)
    torch.cuda.synchronize()
    x = sa.z.cpu().numpy().astype(np.float64)
    for leaf in (sa.z, sa.potential_energy, sa.adapt_state.loc, sa.adapt_state.scale, sa.cov, sa.as_change):
        assert bool(torch.isfinite(leaf).all())
    var = np.diagonal(cov)
    assert np.all(np.abs(x.mean(0) - mean) <= 5 * np.sqrt(var / C)), np.abs(x.mean(0) - mean) / np.sqrt(var / C)
    assert np.all(np.abs(x.var(0, ddof=1) - var) <= 5 * var * np.sqrt(2 / C)), x.var(0, ddof=1) / var
    assert float(sa.as_change[0]) < asc20
    assert 0.99 <= float(sa.mean_accept_prob[0]) <= 1.0  # the share of chain-steps that moved


def test_eight_schools_posterior_through_mcmc(gpu):
    """Eight schools through infer_amd.MCMC against notebook cell 29, with the
    tolerances of test_asss_eight_schools_posterior."""
    import posteriors as P
    from infer_amd import MCMC
    from kernels_amd import PooledASSS, PRNGKey
    mk = dict(P.EIGHT_SCHOOLS_DATA)
    k = PooledASSS(model=P.eight_schools, num_chains=4096)
    m = MCMC(k, num_warmup=2000, num_samples=2000, thinning=20)
    m.run(PRNGKey(0), **mk)
    s = m.get_samples()
    assert s["mu"].shape == (4096 * 100,)
    assert float(s["mu"].mean()) == pytest.approx(4.46, abs=0.1)
    assert float(s["mu"].std()) == pytest.approx(3.30, abs=0.1)
    assert float(s["tau"].mean()) == pytest.approx(3.54, abs=0.12)
    assert float(s["tau"].std()) == pytest.approx(3.20, abs=0.12)
    assert "Iteration: 4000" in k.get_diagnostics_str(m.last_state)


def _rank_worker(rank, world, port, C, steps, out_path, d, K, overlap, align):
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)  # the ranks share the box's one GPU
    import posteriors as P
    from kernels_amd import PooledASSS, PRNGKey
    from kernels_amd.distributed import shard_range
    g = P.correlated_gaussian(d)
    off, cnt = shard_range(C, rank, world, align=align)
    z0 = torch.as_tensor(np.random.default_rng(0).uniform(-2, 2, size=(C, d)).astype(np.float32))
    k = PooledASSS(potential_fn=g, num_chains=cnt, chain_offset=off, device=torch.device("cuda", 0),
                   sync_every=K, overlap=overlap)
    st = k.init(PRNGKey(2), 0, z0[off:off + cnt].cuda(), (), {})
    k.sample_(st, steps)
    np.savez(f"{out_path}.{rank}.npz", z=st.z.cpu().numpy(), pe=st.potential_energy.cpu().numpy(),
             L=st.adapt_state.scale.cpu().numpy(), mu=st.adapt_state.loc.cpu().numpy(), i=st.i.cpu().numpy())
    dist.barrier()
    dist.destroy_process_group()


def _two_ranks(C, steps, K, overlap, gpu, tmp_path, d=32, align=1):
    """-> (the two-rank run: z / pe of all chains in global order and rank
    0's shared leaves, the one-rank run's state)."""
    import socket
    import torch.multiprocessing as mp
    import posteriors as P
    from kernels_amd import PooledASSS, PRNGKey
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "g")
    mp.start_processes(_rank_worker, args=(2, port, C, steps, out, d, K, overlap, align), nprocs=2, join=True,
                       start_method="spawn")
    parts = [np.load(f"{out}.{rank}.npz") for rank in range(2)]
    r = dict(z=np.concatenate([p["z"] for p in parts]), pe=np.concatenate([p["pe"] for p in parts]),
             L=parts[0]["L"], mu=parts[0]["mu"], i=parts[0]["i"])
    assert parts[1]["L"].tobytes() == r["L"].tobytes() and parts[1]["mu"].tobytes() == r["mu"].tobytes()
    z0 = torch.as_tensor(np.random.default_rng(0).uniform(-2, 2, size=(C, d)).astype(np.float32))
    k = PooledASSS(potential_fn=P.correlated_gaussian(d), num_chains=C, sync_every=K, overlap=overlap)
    st = k.init(PRNGKey(2), 0, z0.to(gpu), (), {})
    k.sample_(st, steps)
    torch.cuda.synchronize()
    assert int(r["i"][0]) == steps and r["z"].shape == (C, d)
    return r, st


def test_two_ranks_one_block(gpu, tmp_path):
    """After one block every chain's z / pe is the one-rank run's byte for
    byte (a chain's transition does not read the sums), and loc / scale agree
    to one float32 ulp: only the double association of the sums differs.
    That premise needs both runs to cut the same chunks, whose float32
    partials are then the same bits, so the shards start at multiples of the
    chunk (shard_range(..., align=pooled_chunk(d, C)), as exact_sums asks
    of PooledARWMH); from an unaligned offset the float32 partials differ too
    and loc was seen up to 8 ulp apart."""
    from kernels_amd import pooled_chunk
    r, st = _two_ranks(2001, 1, 1, False, gpu, tmp_path, align=pooled_chunk(32, 2001))
    assert r["z"].tobytes() == st.z.cpu().numpy().tobytes()
    assert r["pe"].tobytes() == st.potential_energy.cpu().numpy().tobytes()
    for got, ref in ((r["mu"], st.adapt_state.loc.cpu().numpy()), (r["L"], st.adapt_state.scale.cpu().numpy())):
        assert np.all(np.abs(got - ref) <= np.spacing(np.abs(ref)))


@pytest.mark.parametrize("K,overlap", [(1, False), (4, True)])
def test_two_ranks_twelve_steps(K, overlap, gpu, tmp_path):
    """The criteria of test_pooled_two_ranks after 12 steps."""
    C = 2001
    r, st = _two_ranks(C, 12, K, overlap, gpu, tmp_path)
    np.testing.assert_allclose(r["L"], st.adapt_state.scale.cpu().numpy(), rtol=1e-4, atol=1e-5)
    zd = np.abs(r["z"] - st.z.cpu().numpy()).max(axis=1) > 1e-4 * (1 + np.abs(r["z"]).max(axis=1))
    assert zd.sum() <= max(2, C // 1000), zd.sum()


def test_limits(gpu):
    """d > 64, a torch callable, exact_sums and step counts off the block
    size raise ValueError; the C entries return AMH_EINVAL for an external
    model and for d = 65."""
    import posteriors as P
    from kernels_amd import ARWMH, PooledASSS, PRNGKey, _lib
    with pytest.raises(ValueError):
        PooledASSS(potential_fn=lambda z: (z * z).sum(1))
    with pytest.raises(ValueError):
        PooledASSS(potential_fn=P.correlated_gaussian(8), exact_sums=True)
    big = PooledASSS(potential_fn=P.correlated_gaussian(96), num_chains=4)
    with pytest.raises(ValueError):
        big.init(PRNGKey(0), 0, torch.zeros(4, 96), (), {})
    (a, sa), _ = _gauss_pair(8, 32, 4, gpu)
    with pytest.raises(ValueError):
        a.sample_(sa, 6)
    with pytest.raises(ValueError):
        a.run(sa, 8, thinning=2)
    # the C entries, on handles the per-chain samplers bound
    L = _lib.lib()
    sums = torch.zeros(8 + 36 + 2, dtype=torch.float64, device=gpu)
    cs = _c_state(sa)
    st = _lib.stream_ptr(gpu.index)
    for kern, z0 in ((ARWMH(potential_fn=lambda z: (z * z).sum(1), num_chains=32), torch.zeros(32, 8)),
                     (ARWMH(potential_fn=P.correlated_gaussian(65), num_chains=32), torch.zeros(32, 65))):
        kern.init(PRNGKey(0), 0, z0.to(gpu), (), {})
        h = kern._handle.h
        calls = (lambda: L.amh_pooled_asss_stats_k(h, 32, ctypes.byref(cs), 4, _lib.ptr(sa.z),
                                                   _lib.ptr(sa.potential_energy), _lib.ptr(sums), st),
                 lambda: L.amh_pooled_asss_update_k(h, _lib.ptr(sums), ctypes.byref(cs), ctypes.byref(cs), 4, st),
                 lambda: L.amh_pooled_asss_step_k(h, 32, ctypes.byref(cs), ctypes.byref(cs), 4, 4, _lib.ptr(sums),
                                                  st))
        for call in calls:
            assert call() == -1  # AMH_EINVAL
            msg = L.amh_last_error(h).decode()
            assert ("not external" in msg) if z0.shape[1] == 8 else ("dim must be <= 64" in msg), msg
