"""Steady-state parity at the BASELINE sizes.

The persistent step kernels hand chains over inside a wave: launch_step64
gives a wave more than one chain only when C > 4,096 (256 blocks x 16 waves),
the generic step kernel when C exceeds CPW x (its co-resident waves), ASSS
when the chain groups exceed 8,192 blocks x 4 waves.  Every test here runs at
a size where each wave owns several chains (the hand-over: store of chain
k-1, the swap through LDS, the flush, the ticket draws) and compares the
WHOLE chain range with the C oracle, bit for bit, through:

  * single sample() launches across the W + 1 warmup reset,
  * a fused run() with thinned collection of z,
  * an in-place sample_() of several steps,
  * the accept counters.

Ragged sizes (4,097 and 65,537 at d = 64) leave one block with one more chain
than the rest.  Reference semantics: python/kernels/arwmh.py:140-207 (ARWMH),
python/kernels/asss.py:197-251 (ASSS).

Every launcher in csrc/ with a capped grid (the chunk-scheduled pooled
kernels, the summary and the assignment kernels aside), and the bit-exact test
in which a wave of it takes a second item (helpers.BIG_CAP = 16,384 chains,
helpers.GROUP_CAP = 32,768 items of CPW chains):

  amh_big.hip wave_grid
    big_init_kernel, big_propose_kernel,
    big_step_kernel<true / false>        test_big_arwmh_second_chain_bitexact
    asss_big_step_kernel                 test_big_asss_second_chain_bitexact
    (three chains per wave)              test_big_third_chain_bitexact
    big_pnx_kernel, asss_big_pnx_kernel  test_gpu_steady_pnx.test_big_pnx_second_chain_bitexact
  amh_kernels.hip grid_for
    arwmh_init_kernel                    test_generic_step_steady_state_bitexact (init compared)
    potential_kernel                     test_potential_second_item_bitexact
    sample_pnx_kernel                    test_gpu_steady_pnx.test_group_pnx_second_item_bitexact, ..third_item..
    pnx_ext_kernel                       test_gpu_steady_pnx.test_external_arwmh_pnx_second_item_bitexact
  amh_asss.hip
    asss_step_kernel                     test_asss_steady_state_bitexact
    asss_pnx_kernel                      test_gpu_steady_pnx.test_group_pnx_second_item_bitexact, ..third_item..
  amh_asss_ext.hip launch_ext
    asss_ext_begin / shrink / finish     test_external_asss_second_item_bitexact
    begin<frozen>, pnx_finish            test_gpu_steady_pnx.test_external_asss_pnx_second_item_bitexact
  amh_split.hip run_propose
    propose_kernel<64>, <32>             test_external_arwmh_second_item_bitexact
    propose_kernel<32, kDiamondsD>       test_gpu_configs.test_diamonds_config_size
  launch_step / launch_step64 (persistent grids): the three tests below."""
import numpy as np
import pytest
import torch

from helpers import (BIG_CAP, GROUP_CAP, assert_chains_bitequal, assert_state_bitequal, items_per_wave, make_case,
                     state_rows)

pytestmark = pytest.mark.gpu


def _init(kind, C, orc, d=None, num_warmup=0, seed=0, cls="ARWMH"):
    import kernels_amd
    kw, mk, om = make_case(kind, d)
    k = getattr(kernels_amd, cls)(num_chains=C, **kw)
    key = kernels_amd.PRNGKey(seed)
    if "potential_fn" in kw:
        z0 = np.random.default_rng(seed + C).uniform(-2, 2, size=(C, om.d)).astype(np.float32)
        st = k.init(key, num_warmup, torch.as_tensor(z0), (), mk)
        ost = orc.init(om, key, C, init_z=z0)
    else:
        st = k.init(key, num_warmup, None, (), mk)
        ost = orc.init(om, key, C)
    torch.cuda.synchronize()
    return k, st, mk, om, ost


def _arwmh_sequence(kind, d, C, W, gpu, orc, n_single=5):
    k, st, mk, om, ost = _init(kind, C, orc, d=d, num_warmup=W)
    assert_state_bitequal(st, ost, f"{kind} C={C} init")
    acc = np.zeros(C, np.int32)
    for t in range(n_single):  # i = 1..n_single: gamma_1 = 1 keep-L, the reset at W + 1
        st = k.sample(st, (), mk)
        orc.step(om, ost, 1, num_warmup=W, accept_count=acc)
        if t in (0, W, n_single - 1):
            torch.cuda.synchronize()
            assert_state_bitequal(st, ost, f"{kind} C={C} sample {t + 1}")
    st, cz, _ = k.run(st, 7, thinning=3, collect_z=True)
    ocz = orc.step(om, ost, 7, num_warmup=W, accept_count=acc, collect_z=True)
    torch.cuda.synchronize()
    assert_state_bitequal(st, ost, f"{kind} C={C} run(7, thinning=3)")
    assert cz.shape == (2, C, om.d)
    np.testing.assert_array_equal(cz.cpu().numpy().view(np.uint32), ocz[2::3].view(np.uint32))
    del cz, ocz
    k.sample_(st, 6)
    orc.step(om, ost, 6, num_warmup=W, accept_count=acc)
    torch.cuda.synchronize()
    assert_state_bitequal(st, ost, f"{kind} C={C} sample_(6)")
    np.testing.assert_array_equal(k.accept_count.cpu().numpy(), acc)
    assert int(st.i.min()) == int(st.i.max()) == n_single + 13


@pytest.mark.parametrize("C", [65536, 4097, 65537])
def test_step64_steady_state_bitexact(C, gpu, orc):
    """arwmh_step64_kernel<16> (the headline kernel) at configs[1]'s size and
    at ragged sizes either side of one chain per wave: every chain, every field."""
    _arwmh_sequence("gaussian", 64, C, 3, gpu, orc)


@pytest.mark.parametrize("kind,C", [("eight_schools", 262144), ("diamonds_ss", 262144), ("kidiq", 131072),
                                    ("gaussian32", 100003)])
def test_generic_step_steady_state_bitexact(kind, C, gpu, orc):
    """arwmh_step_kernel<DMAX, M> with several chain groups per wave:
    eight schools (G = 16, 4 chains per wave), the diamonds sufficient-
    statistics model at configs[2]'s 262,144 chains (compile-time d = 26),
    kidiq (G = 4) and a ragged d = 32 Gaussian."""
    d = None
    if kind == "gaussian32":
        kind, d = "gaussian", 32
    _arwmh_sequence(kind, d, C, 2, gpu, orc, n_single=4)


@pytest.mark.parametrize("kind,d,C", [("gaussian", 64, 65536), ("eight_schools", None, 262144)])
def test_asss_steady_state_bitexact(kind, d, C, gpu, orc):
    """ASSS (amh_asss.hip) with two or more chain groups per wave (grid-stride
    past 8,192 blocks): single launches, a fused run with collection, in place."""
    from test_gpu_asss import assert_bitequal
    k, st, mk, om, ost = _init(kind, C, orc, d=d, num_warmup=2, cls="ASSS")
    for t in range(3):
        st = k.sample(st, (), mk)
        orc.asss_step(om, ost, 1, num_warmup=2)
    torch.cuda.synchronize()
    assert_bitequal(st, ost, f"asss {kind} C={C} sample x3")
    st, cz, cp = k.run(st, 4, thinning=2, collect_z=True, collect_pe=True)
    ocz, ocp = orc.asss_step(om, ost, 4, num_warmup=2, collect_z=True, collect_pe=True)
    torch.cuda.synchronize()
    assert_bitequal(st, ost, f"asss {kind} C={C} run(4)")
    np.testing.assert_array_equal(cz.cpu().numpy().view(np.uint32), ocz[1::2].view(np.uint32))
    np.testing.assert_array_equal(cp.cpu().numpy().view(np.uint32), ocp[1::2].view(np.uint32))
    k.sample_(st, 3)
    orc.asss_step(om, ost, 3, num_warmup=2)
    torch.cuda.synchronize()
    assert_bitequal(st, ost, f"asss {kind} C={C} in place")


# ------------------------------------------- large d: amh_big.hip, wave_grid --
# d -> what the streaming instantiation of that d is made of (DMA piece, row
# slots per lane, 8-column blocks of the factor; an odd block count leaves the
# last block consumed in the LDS buffer the next chain's first DMA lands in)
BIG_DIMS = [72,   # dwordx4, 2 slots, 9 blocks (odd)
            97,   # dword (ragged, odd d), 2 slots, 13 blocks (odd)
            128,  # dwordx4, 2 slots, 16 blocks (even)
            150,  # dword, 3 slots, 19 blocks (odd)
            160,  # dwordx4, 3 slots, 20 blocks (even)
            200,  # dwordx4, 4 slots, 25 blocks (odd)
            250]  # dword, 4 slots, 32 blocks (even)
BIG_C = BIG_CAP + 70       # blocks 0..16 take a second chain in all four waves, block 17 in two of its four
BIG_C3 = 2 * BIG_CAP + 3   # every wave takes two chains, three waves of block 0 a third
BIG_LAM = -2.0             # log step size at which some, not all, chains accept from the uniform start


def _big_slices(d, C):
    """Chain ranges compared with the oracle.  Up to d = 128 every chain; above
    it first-pass chains of waves that go on (0..69), of waves that stop (70..95,
    the middle, 16,336..16,383) and every second-pass chain (16,384..C)."""
    if d <= 128:
        return [(0, C)]
    assert C == BIG_C
    return [(0, 96), (BIG_CAP // 2 - 24, BIG_CAP // 2 + 24), (BIG_CAP - 48, C)]


def _big_start(cls, d, C, W, orc, lam=None):
    """A large-d Gaussian kernel of C chains and one oracle state per compared
    chain range (chain keys depend only on the run key and the global chain
    id: chain_offset, and the range's rows of the start points)."""
    import kernels_amd
    kw, mk, om = make_case("gaussian", d)
    k = getattr(kernels_amd, cls)(num_chains=C, **kw)
    key = kernels_amd.PRNGKey(0)
    z0 = np.random.default_rng(C).uniform(-2, 2, size=(C, d)).astype(np.float32)
    st = k.init(key, W, torch.as_tensor(z0), (), mk)
    sl = _big_slices(d, C)
    osts = [orc.init(om, key, hi - lo, chain_offset=lo, init_z=z0[lo:hi]) for lo, hi in sl]
    if lam is not None:
        st.adapt_state.log_step_size.fill_(lam)
        for o in osts:
            o.log_step_size[:] = lam
    torch.cuda.synchronize()
    return k, st, om, sl, osts


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return a.view(np.uint32)


def _big_arwmh_sequence(d, C, orc):
    from test_gpu_configs import _properties
    assert C > BIG_CAP, "amh_big.hip wave_grid: no wave takes a second chain"
    W = 2
    k, st, om, sl, osts = _big_start("ARWMH", d, C, W, orc, lam=BIG_LAM)
    accs = [np.zeros(hi - lo, np.int32) for lo, hi in sl]

    def check(s, what):
        torch.cuda.synchronize()
        for (lo, hi), o in zip(sl, osts):
            assert_state_bitequal(state_rows(s, lo, hi), o, f"d={d} C={C} chains [{lo}, {hi}) {what}")

    check(st, "init")
    for t in range(1, 5):  # gamma = 1 keeps L at steps 1 and W + 1; the proposal is chained across calls
        st = k.sample(st, (), {})
        for (lo, hi), o, acc in zip(sl, osts, accs):
            before, a1 = o.scale.copy(), np.zeros(hi - lo, np.int32)
            orc.step(om, o, 1, num_warmup=W, accept_count=a1)
            acc += a1
            kept = np.array_equal(before.view(np.uint32), o.scale.view(np.uint32))
            assert kept == (t in (1, W + 1)), f"d={d} step {t}: factor kept = {kept}"
            late = a1[max(BIG_CAP - lo, 0):] if hi > BIG_CAP else a1
            assert 0 < int(late.sum()) < late.size, f"d={d} step {t} chains [{lo}, {hi}): {int(late.sum())} accept"
        if t in (1, W + 1, 4):
            check(st, f"sample {t}")
    st, cz, cp = k.run(st, 5, thinning=2, collect_z=True, collect_pe=True)  # big_step_kernel<NEXT>, collecting
    torch.cuda.synchronize()
    assert cz.shape == (2, C, d) and cp.shape == (2, C)
    for (lo, hi), o, acc in zip(sl, osts, accs):
        zs, ps = [], []
        for _ in range(5):
            orc.step(om, o, 1, num_warmup=W, accept_count=acc)
            zs.append(o.z.copy())
            ps.append(o.potential_energy.copy())
        np.testing.assert_array_equal(_bits(cz[:, lo:hi]), np.stack(zs)[1::2].view(np.uint32))
        np.testing.assert_array_equal(_bits(cp[:, lo:hi]), np.stack(ps)[1::2].view(np.uint32))
    del cz, cp
    check(st, "run(5, thinning=2)")
    k.sample_(st, 4)
    for o, acc in zip(osts, accs):
        orc.step(om, o, 4, num_warmup=W, accept_count=acc)
    check(st, "sample_(4)")
    k.chain_proposals = False  # no kept proposal: a fresh big_propose_kernel pass, then big_step_kernel<false>
    st = k.sample(st, (), {})
    for o, acc in zip(osts, accs):
        orc.step(om, o, 1, num_warmup=W, accept_count=acc)
    check(st, "sample() without a chained proposal")
    for (lo, hi), acc in zip(sl, accs):
        np.testing.assert_array_equal(k.accept_count[lo:hi].cpu().numpy(), acc)
    assert int(st.i.min()) == int(st.i.max()) == 14
    if len(sl) > 1:
        _properties(st, d)


def _asss_properties(st, d):
    """test_gpu_configs._properties for an ASSS state (no acceptance leaf)."""
    from kernels_amd import unpack_scale
    C = st.z.shape[0]
    assert torch.isfinite(st.z).all() and torch.isfinite(st.potential_energy).all()
    assert torch.isfinite(st.adapt_state.scale).all() and torch.isfinite(st.as_change).all()
    idx = torch.arange(d, device=st.z.device)
    assert (st.adapt_state.scale[:, idx * d - idx * (idx - 1) // 2] > 0).all(), "every factor keeps a positive diagonal"
    sub = unpack_scale(st.adapt_state.scale[:: max(1, C // 64)], d)
    assert torch.equal(torch.triu(sub, 1), torch.zeros_like(sub)), "upper triangle stays zero"


def _big_asss_sequence(d, C, orc):
    from test_gpu_asss import assert_bitequal
    assert C > BIG_CAP, "amh_big.hip wave_grid: no wave takes a second chain"
    W = 2
    k, st, om, sl, osts = _big_start("ASSS", d, C, W, orc)

    def check(s, what):
        torch.cuda.synchronize()
        for (lo, hi), o in zip(sl, osts):
            assert_bitequal(state_rows(s, lo, hi), o, f"asss d={d} C={C} chains [{lo}, {hi}) {what}")

    check(st, "init")
    for t in range(3):
        st = k.sample(st, (), {})
        for o in osts:
            z = o.z.copy()
            orc.asss_step(om, o, 1, num_warmup=W)
            assert np.all(np.any(z != o.z, axis=1)), f"asss d={d} step {t + 1}: a chain did not move"
    check(st, "sample x3")
    st, cz, cp = k.run(st, 4, thinning=2, collect_z=True, collect_pe=True)
    torch.cuda.synchronize()
    assert cz.shape == (2, C, d) and cp.shape == (2, C)
    for (lo, hi), o in zip(sl, osts):
        ocz, ocp = orc.asss_step(om, o, 4, num_warmup=W, collect_z=True, collect_pe=True)
        np.testing.assert_array_equal(_bits(cz[:, lo:hi]), ocz[1::2].view(np.uint32))
        np.testing.assert_array_equal(_bits(cp[:, lo:hi]), ocp[1::2].view(np.uint32))
    del cz, cp
    check(st, "run(4, thinning=2)")
    k.sample_(st, 3)
    for o in osts:
        orc.asss_step(om, o, 3, num_warmup=W)
    check(st, "sample_(3)")
    assert int(st.i.min()) == int(st.i.max()) == 10
    if len(sl) > 1:
        _asss_properties(st, d)


@pytest.mark.parametrize("d", BIG_DIMS)
def test_big_arwmh_second_chain_bitexact(d, gpu, orc):
    """big_propose_kernel and big_step_kernel<NEXT> (amh_big.hip, wave_grid:
    4,096 blocks x 4 waves = 16,384 chains per pass) at C = 16,454: blocks 0..16
    take a second chain in all four waves, block 17 in two of four.  Init, four
    sample() calls (keep-L at steps 1 and W + 1, proposals chained across
    calls), a fused run(5) with both collections thinned by 2, sample_(4) in
    place, one sample() with chain_proposals off (a fresh propose pass and
    big_step_kernel<false>) and accept_count; every chain up to d = 128, above it the slices of
    _big_slices plus the properties of the full state."""
    assert items_per_wave(BIG_C, BIG_CAP) == 2 and 0 < (BIG_C - BIG_CAP) % 4
    _big_arwmh_sequence(d, BIG_C, orc)


@pytest.mark.parametrize("d", BIG_DIMS)
def test_big_asss_second_chain_bitexact(d, gpu, orc):
    """asss_big_step_kernel (amh_big.hip, wave_grid: 16,384 chains per pass) at
    C = 16,454, where the shrink loop and the accept branch stay wave-uniform
    only because a wave holds one chain at a time: the sequence of
    test_asss_steady_state_bitexact, chains compared as in the ARWMH test."""
    assert items_per_wave(BIG_C, BIG_CAP) == 2 and 0 < (BIG_C - BIG_CAP) % 4
    _big_asss_sequence(d, BIG_C, orc)


@pytest.mark.parametrize("cls", ["ARWMH", "ASSS"])
def test_big_third_chain_bitexact(cls, gpu, orc):
    """amh_big.hip's step kernels at d = 72 and C = 32,771 = 2 x 16,384 + 3
    (wave_grid): every wave takes two chains and three waves of block 0 a
    third; every chain, every field."""
    assert items_per_wave(BIG_C3, BIG_CAP) == 3 and items_per_wave(BIG_C3 - 3, BIG_CAP) == 2
    (_big_arwmh_sequence if cls == "ARWMH" else _big_asss_sequence)(72, BIG_C3, orc)


# ------------------------------------------------- external potential (C) ----
@pytest.mark.parametrize("d,C,cpw", [(48, GROUP_CAP + 73, 1),          # propose_kernel<64>, one chain per wave
                                     (24, 2 * GROUP_CAP + 71, 2)])     # propose_kernel<32>, CPW = 2, clamped tail
def test_external_arwmh_second_item_bitexact(d, C, cpw, gpu, orc):
    """ARWMH with the caller's U (amh_split.hip run_propose: propose_kernel<64>
    above d = 32, propose_kernel<32> with two chains per wave below; 8,192
    blocks x 4 waves = 32,768 items per pass; U is the registry kernel's
    potential_kernel under grid_for's cap) past one item per wave: init, three
    sample(), sample_(3), run(4, thinning=2) with both collections,
    accept_count.  The oracle runs one step per call (tests/test_gpu_external.py)."""
    from test_gpu_external import _pair
    assert cpw == (1 if d > 32 else 2)  # run_propose's own choice, not dispatch_dim's
    assert C in (32841, 65607) and C % cpw == 1 % cpw
    assert items_per_wave(C, GROUP_CAP, cpw) == 2
    W = 4
    ke, st, om, ost = _pair(d, C, gpu, orc, W=W)
    assert_state_bitequal(st, ost, f"external d={d} C={C} init")
    acc = np.zeros(C, np.int32)
    for t in range(3):
        st = ke.sample(st, (), {})
        a1 = np.zeros(C, np.int32)
        orc.step(om, ost, 1, num_warmup=W, accept_count=a1)
        acc += a1
        late = a1[GROUP_CAP * cpw:]
        assert 0 < int(late.sum()) < late.size, f"step {t + 1}: {int(late.sum())} of {late.size} late chains accept"
    torch.cuda.synchronize()
    assert_state_bitequal(st, ost, f"external d={d} C={C} sample x3")
    ke.sample_(st, 3)
    for _ in range(3):
        orc.step(om, ost, 1, num_warmup=W, accept_count=acc)
    torch.cuda.synchronize()
    assert_state_bitequal(st, ost, f"external d={d} C={C} sample_(3)")
    st, cz, cp = ke.run(st, 4, thinning=2, collect_z=True, collect_pe=True)
    zs, ps = [], []
    for _ in range(4):
        orc.step(om, ost, 1, num_warmup=W, accept_count=acc)
        zs.append(ost.z.copy())
        ps.append(ost.potential_energy.copy())
    torch.cuda.synchronize()
    assert_state_bitequal(st, ost, f"external d={d} C={C} run(4, thinning=2)")
    np.testing.assert_array_equal(_bits(cz), np.stack(zs)[1::2].view(np.uint32))
    np.testing.assert_array_equal(_bits(cp), np.stack(ps)[1::2].view(np.uint32))
    np.testing.assert_array_equal(ke.accept_count.cpu().numpy(), acc)


@pytest.mark.parametrize("d,C", [(33, GROUP_CAP + 73), (5, 8 * GROUP_CAP + 9)])
def test_external_asss_second_item_bitexact(d, C, gpu, orc):
    """ASSS(host_shrink=True) (amh_asss_ext.hip launch_ext: asss_ext_begin,
    asss_ext_shrink per round and asss_ext_finish at the lane-group width of d,
    32,768 items per pass) past one item per wave: d = 33 with one chain per
    wave, d = 5 with eight and a tail group of one chain.  Three sample() and
    sample_(2); the multi-round shrink path is taken."""
    from kernels_amd import ASSS, PRNGKey
    from test_gpu_asss import assert_bitequal
    from test_gpu_asss_external import _registry
    cpw = 64 // orc.group_width(d)  # ExtF in amh_asss_ext.hip: Geo<D>::CPW at dispatch_dim's D
    assert C in (32841, 262153) and C % cpw == 1 % cpw
    assert items_per_wave(C, GROUP_CAP, cpw) == 2
    W = 2
    kg, _, om = _registry("gaussian", d)
    z0 = np.random.default_rng(C).uniform(-2, 2, size=(C, d)).astype(np.float32)
    ke = ASSS(potential_fn=lambda z: kg.potential(z), num_chains=C, host_shrink=True)
    st = ke.init(PRNGKey(0), W, torch.as_tensor(z0), (), {})
    ost = orc.init(om, PRNGKey(0), C, init_z=z0)
    torch.cuda.synchronize()
    assert_bitequal(st, ost, f"host shrink d={d} C={C} init")
    rounds = []
    for t in range(3):
        st = ke.sample(st, (), {})
        rounds.append(ke.shrink_rounds)
        z = ost.z.copy()
        orc.asss_step(om, ost, 1, num_warmup=W)
        assert np.all(np.any(z != ost.z, axis=1)), f"step {t + 1}: a chain did not move"
    torch.cuda.synchronize()
    assert_bitequal(st, ost, f"host shrink d={d} C={C} sample x3")
    ke.sample_(st, 2)
    rounds.append(ke.shrink_rounds)
    for _ in range(2):
        orc.asss_step(om, ost, 1, num_warmup=W)
    torch.cuda.synchronize()
    assert_bitequal(st, ost, f"host shrink d={d} C={C} sample_(2)")
    assert max(rounds) >= 3, rounds


# ------------------------------------------------------ potential_kernel (D) --
@pytest.mark.parametrize("kind,d,n", [("gaussian", 40, GROUP_CAP + 73), ("eight_schools", None, 4 * GROUP_CAP + 25)])
def test_potential_second_item_bitexact(kind, d, n, gpu, orc):
    """potential_kernel (amh_kernels.hip launch_pot, grid_for: 32,768 items per
    pass) past one item per wave: the Gaussian at G = 64 and eight schools at
    G = 16 (four points per wave, a tail group of one point)."""
    k, st, mk, om, ost = _init(kind, 8, orc, d=d)
    cpw = 64 // orc.group_width(om.d)
    assert n in (32841, 131097) and n % cpw == 1 % cpw
    assert items_per_wave(n, GROUP_CAP, cpw) == 2
    z = np.random.default_rng(n).normal(size=(n, om.d)).astype(np.float32)
    pe = k.potential(torch.as_tensor(z, device=gpu))
    assert_chains_bitequal(pe, orc.potential(om, z), GROUP_CAP, cpw, f"{kind} potential n={n}")
