"""PooledARWMH(exact_sums=True) on the GPU: a run over `world` ranks whose
shards are chunk-aligned is byte-identical to one process holding all chains
(include/amh.h "exact sums").

The ranks share the one GPU and exchange over gloo (as
test_gpu_pooled.py::_gpu_worker does).  One group of `world` processes is
spawned per world size and runs every case in turn, so the process start-up is
paid twice for the whole file; the one-rank run of each case is computed in
the test process."""
import os
import socket
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

JOIN_LIMIT = 240.0  # seconds a spawned group may take for all its cases

# name -> (d, C, steps, K, overlap, external, worlds); the shapes are the smallest that reach each path:
CASES = {
    # the lane-per-row form: 10 chunks of 16 chains, a ragged last one
    "d32": (32, 16 * 9 + 5, 12, 1, False, False, (2, 3)),
    # ... where a rank's own count (4,096: one chain per wave) and the global one (two) cut different chunks
    "d32_cpw": (32, 8192, 4, 1, False, False, (2,)),
    # pooled_fused64_kernel: 128-chain chunks of two sub-chunks, a ragged tail chunk
    "d64": (64, 128 * 5 + 37, 12, 1, False, False, (2, 3)),
    "d64_k4": (64, 128 * 5 + 37, 16, 4, False, False, (2, 3)),
    "d64_overlap": (64, 128 * 5 + 37, 12, 1, True, False, (2, 3)),
    "d64_k4_overlap": (64, 128 * 5 + 37, 16, 4, True, False, (2, 3)),
    # the large-d fused kernel (K launch sequences accumulate into the words)
    "d128": (128, 128 * 3 + 50, 6, 1, False, False, (2,)),
    "d128_k3": (128, 128 * 3 + 50, 6, 3, False, False, (2,)),
    # a torch callable (amh_pooled_propose / amh_pooled_stats_external_exact rounds)
    "ext64": (64, 128 * 3 + 11, 8, 1, False, True, (2,)),
    "ext64_k4": (64, 128 * 3 + 11, 8, 4, False, True, (2,)),
}
LEAVES = ("z", "potential_energy", "scale", "loc", "log_step_size", "cov", "mean_accept_prob", "as_change", "i")


def _torch_U(d):
    """An elementwise potential (no reduction whose order could depend on the batch shape)."""
    def U(z):
        a = z[:, 0] * (2.0 * z[:, 0])
        b = z[:, d - 1] * (0.5 * z[:, d - 1])
        c = z[:, 1] * z[:, 2]
        return 0.5 * ((a + b) + c * c)
    return U


def _run_case(name, rank, world, device):
    """The case on this rank's chunk-aligned shard (world = 1: all chains);
    returns the state leaves as numpy arrays, and the pending sums with overlap."""
    import posteriors as P
    from kernels_amd import PooledARWMH, PRNGKey, pooled_chunk
    from kernels_amd.distributed import shard_range
    d, C, steps, K, overlap, external, _ = CASES[name]
    off, cnt = shard_range(C, rank, world, align=pooled_chunk(d, C))
    z0 = torch.as_tensor(np.random.default_rng(0).uniform(-2, 2, size=(C, d)).astype(np.float32))
    pot = _torch_U(d) if external else P.correlated_gaussian(d)
    k = PooledARWMH(potential_fn=pot, num_chains=cnt, chain_offset=off, device=device, sync_every=K, overlap=overlap,
                    exact_sums=True)
    st = k.init(PRNGKey(2), 0, z0[off:off + cnt].to(device), (), {})
    k.sample_(st, steps)
    torch.cuda.synchronize()
    a = st.adapt_state
    out = dict(z=st.z, potential_energy=st.potential_energy, scale=a.scale, loc=a.loc, log_step_size=a.log_step_size,
               cov=st.cov, mean_accept_prob=st.mean_accept_prob, as_change=st.as_change, i=st.i)
    out = {f: t.cpu().numpy() for f, t in out.items()}
    if overlap:
        out["pending"] = k.pending_sums()
    return out


def _worker(rank, world, port, names, out_dir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)  # the ranks share the box's one GPU
    for name in names:
        np.savez(os.path.join(out_dir, f"{name}_w{world}_r{rank}.npz"),
                 **_run_case(name, rank, world, torch.device("cuda", 0)))
    dist.barrier()
    dist.destroy_process_group()


def _spawn(world, names, out_dir):
    """One group of `world` ranks for all of `names`, under a join limit of its
    own; a rank that dies fails (ProcessContext.join raises and ends the
    others), and nothing is tried again."""
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.start_processes(_worker, args=(world, port, names, out_dir), nprocs=world, join=False,
                             start_method="spawn")
    deadline = time.monotonic() + JOIN_LIMIT
    try:
        while not ctx.join(timeout=max(0.1, deadline - time.monotonic())):
            if time.monotonic() >= deadline:
                pytest.fail(f"the {world}-rank group did not finish within {JOIN_LIMIT:.0f} s")
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()


@pytest.fixture(scope="module")
def rank_runs(gpu, tmp_path_factory):
    """{world: directory of <case>_w<world>_r<rank>.npz}; each group is spawned once."""
    out = {}
    for world in (2, 3):
        d = str(tmp_path_factory.mktemp(f"world{world}"))
        _spawn(world, [n for n, c in CASES.items() if world in c[6]], d)
        out[world] = d
    return out


@pytest.fixture(scope="module")
def one_rank(gpu):
    """The one-process run of each case, computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _run_case(name, 0, 1, gpu)
        return cache[name]
    return get


@pytest.mark.parametrize("name,world", [(n, w) for n, c in CASES.items() for w in c[6]])
def test_ranks_equal_one_process_by_bytes(name, world, rank_runs, one_rank):
    want = one_rank(name)
    runs = [np.load(os.path.join(rank_runs[world], f"{name}_w{world}_r{r}.npz")) for r in range(world)]
    assert int(want["i"][0]) == CASES[name][2]
    for f in LEAVES + (("pending",) if CASES[name][4] else ()):
        if f in ("z", "potential_energy"):  # per chain: the shards in rank order
            got = np.concatenate([r[f] for r in runs], axis=0)
            assert got.shape == want[f].shape and got.tobytes() == want[f].tobytes(), f"{name}: {f} differs"
        else:  # shared: every rank holds the one-process bytes
            for k, r in enumerate(runs):
                assert r[f].shape == want[f].shape and r[f].tobytes() == want[f].tobytes(), \
                    f"{name}: {f} of rank {k} differs"
    assert np.isfinite(want["scale"]).all() and np.abs(want["z"] - want["z"][0]).max() > 0


def test_exact_equals_default_up_to_association(gpu):
    """One rank, d = 64: the exact sums differ from the default double sums
    as two association orders do, so the two runs agree within the allowance
    test_gpu_pooled.py::test_pooled_two_ranks gives a different association: L
    at rtol 1e-4 / atol 1e-5 and at most max(2, C // 1000) chains differing."""
    import posteriors as P
    from kernels_amd import PooledARWMH, PRNGKey
    d, C, steps = 64, 3001, 12
    g = P.correlated_gaussian(d)
    z0 = torch.as_tensor(np.random.default_rng(0).uniform(-2, 2, size=(C, d)).astype(np.float32)).to(gpu)
    res = []
    for exact in (False, True):
        k = PooledARWMH(potential_fn=g, num_chains=C, exact_sums=exact)
        st = k.init(PRNGKey(2), 0, z0.clone(), (), {})
        k.sample_(st, steps)
        torch.cuda.synchronize()
        res.append((st.adapt_state.scale.cpu().numpy(), st.z.cpu().numpy(), k._sums.cpu().numpy()))
    (L0, zd, s0), (L1, ze, s1) = res
    print("max |L_exact - L_default| =", np.abs(L1 - L0).max(), " last sums max rel diff =",
          np.abs(s1 - s0).max() / np.abs(s0).max())
    np.testing.assert_allclose(L1, L0, rtol=1e-4, atol=1e-5)
    diff = np.abs(ze - zd).max(axis=1) > 1e-4 * (1 + np.abs(zd).max(axis=1))
    print("chains differing:", int(diff.sum()))
    assert diff.sum() <= max(2, C // 1000), diff.sum()


def test_misaligned_offset_is_refused(gpu):
    import posteriors as P
    from kernels_amd import PooledARWMH, PRNGKey, pooled_chunk
    g = P.correlated_gaussian(64)
    z0 = torch.zeros(100, 64, device=gpu)
    assert pooled_chunk(64, 100) == 128
    k = PooledARWMH(potential_fn=g, num_chains=100, chain_offset=64, exact_sums=True)
    with pytest.raises(ValueError, match="chunk of 128"):
        k.init(PRNGKey(0), 0, z0, (), {})
    # the same shard is fine without exact sums, and an aligned one with them
    PooledARWMH(potential_fn=g, num_chains=100, chain_offset=64).init(PRNGKey(0), 0, z0, (), {})
    PooledARWMH(potential_fn=g, num_chains=100, chain_offset=256, exact_sums=True).init(PRNGKey(0), 0, z0, (), {})


def test_exact_sums_is_a_pooled_option(gpu):
    import posteriors as P
    from kernels_amd import ARWMH
    with pytest.raises(TypeError):
        ARWMH(potential_fn=P.correlated_gaussian(8), num_chains=4, exact_sums=True)
