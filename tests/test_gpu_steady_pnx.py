"""sample_Pnx where a wave takes a second and a third item (the sibling of
tests/test_gpu_steady.py for the frozen kernels).

Every launcher of a frozen kernel caps its grid and lets a wave walk the items
w, w + cap, ...: amh_big.hip's wave_grid at 4,096 blocks x 4 waves (16,384
chains, one per wave), amh_kernels.hip's grid_for and its copies in
amh_asss.hip and amh_asss_ext.hip at 8,192 blocks x 4 waves (32,768 items of
CPW = 64 / G chains).  What such a loop carries from one item to the next --
the LDS double buffer of the streamed factor, the frozen U / dl / mu passed by
reference into the slice transition, the split key, the start point
pt = c / n_samples, pe and the chain_ok clamp of a tail group -- is reached
only past the cap, so every case here runs at cap + r items (ragged:
some blocks, and some waves of one block, go on) or at 2 cap + r, and compares
the whole output with the C oracle bit for bit.  Each test asserts that its
size crosses the cap it names.  The moved fractions are the oracle's own."""
import numpy as np
import pytest
import torch

from helpers import BIG_CAP, GROUP_CAP, assert_chains_bitequal, items_per_wave, make_case, make_edge_case

pytestmark = pytest.mark.gpu

KEY = 7


def _theta(cls, kind, d, steps, chain, npts, C0=16):
    """A frozen theta = the adapt state of one chain after a short run of the
    sampler itself (tests/test_gpu_steady.py's _init, on helpers.make_edge_case),
    and npts of that run's points as start points."""
    import kernels_amd
    kw, mk, om = make_edge_case(kind, d)
    k = getattr(kernels_amd, cls)(num_chains=C0, **kw)
    z0 = None
    if "potential_fn" in kw:
        z0 = torch.as_tensor(np.random.default_rng(C0).uniform(-2, 2, size=(C0, om.d)).astype(np.float32))
    st = k.init(kernels_amd.PRNGKey(0), 0, z0, (), mk)
    k.sample_(st, steps)
    theta = tuple(t[chain].clone() for t in st.adapt_state)  # (loc, scale) and ARWMH's log_step_size
    x = st.z[:npts].clone()
    torch.cuda.synchronize()
    return k, om, theta, x


def _oracle_pnx(orc, om, cls, x, theta, n, ns):
    from kernels_amd import PRNGKey
    th = [t.cpu().numpy() for t in theta]
    if cls == "ASSS":
        return orc.asss_sample_pnx(om, PRNGKey(KEY), x, th[0], th[1], n, ns)
    return orc.sample_pnx(om, PRNGKey(KEY), x, th[0], th[1], float(th[2]), n, ns)


def _compare(out, ref, x, cls, cap, cpw, what):
    """The whole output bit for bit; before it, from the oracle alone: enough
    chains moved, among all of them and among those of the later passes."""
    npts, ns, d = ref.shape
    C = npts * ns
    assert tuple(out.shape) == (npts, ns, d)
    moved = np.any(ref != x[:, None, :], axis=-1).reshape(C)
    late = moved[cap * cpw:]
    assert late.size > 0
    if cls == "ASSS":
        assert moved.all(), f"{what}: {C - int(moved.sum())} chains did not move"
    else:
        assert moved.mean() > 0.2, (what, moved.mean())  # accepted moves are compared, not only rejections
        assert 0 < int(late.sum()) < late.size, f"{what}: {int(late.sum())} of {late.size} late chains moved"
    assert_chains_bitequal(out.reshape(C, d), ref.reshape(C, d), cap, cpw, what)


def _case(cls, kind, d, npts, ns, n, orc, cap, steps, chain, passes=2):
    k, om, theta, x = _theta(cls, kind, d, steps, chain, npts)
    C = npts * ns
    cpw = 1 if cap == BIG_CAP else 64 // orc.group_width(om.d)  # amh_big.hip: one chain per wave
    assert items_per_wave(C, cap, cpw) == passes, "no wave takes a later item: the cap moved"
    assert cpw == 1 or C % cpw != 0, "the last group is no clamped tail"
    first_late = (cap * cpw) // ns  # the point of the first chain past the cap
    assert first_late == npts - 1 if passes == 2 else first_late >= 1, "the later passes start at the first point"
    from kernels_amd import PRNGKey
    out = k.sample_Pnx(PRNGKey(KEY), x, theta, n=n, n_samples=ns)
    xh = x.cpu().numpy()
    ref = _oracle_pnx(orc, om, cls, xh, theta, n, ns)
    _compare(out, ref, xh, cls, cap, cpw, f"{cls} {kind} d={om.d} sample_Pnx {npts} x {ns}")


# ------------------------------------------------ A. large d (amh_big.hip) ----
@pytest.mark.parametrize("d", [97, 128, 150, 200])
@pytest.mark.parametrize("cls", ["ARWMH", "ASSS"])
def test_big_pnx_second_chain_bitexact(cls, d, gpu, orc):
    """big_pnx_kernel / asss_big_pnx_kernel (amh_big.hip, wave_grid: 16,384
    chains per pass) at 3 x 5,485 = 16,455 chains, n = 2: the second pass lies
    inside the last point, so pt = c / n_samples, the split key and pe are
    reloaded past the cap, the factor's LDS double buffer is handed from one
    chain to the next (13 and 19 column blocks are odd), and the slice
    kernel's hoisted dl / inv serve a second chain.  theta: chain 5 of a
    12-step run of 16 chains."""
    assert 3 * 5485 == BIG_CAP + 71
    _case(cls, "gaussian", d, 3, 5485, 2, orc, BIG_CAP, steps=12, chain=5)


# ------------------------------------------ B. d <= 64 (grid_for's 32,768) ----
GROUP_CASES = [("gaussian", 40, 3, 10947),       # G = 64, 32,841 chains
               ("gaussian", 64, 3, 10947),       # G = 64, the EXACT instantiation
               ("eight_schools", None, 3, 43699),  # G = 16, 131,097 chains
               ("logistic_n77", 8, 3, 87383),    # G = 8, 262,149 chains; model data (N = 77 rows) staged once in LDS
               ("mixture", 3, 5, 104859)]        # G = 4, 524,295 chains


@pytest.mark.parametrize("kind,d,npts,ns", GROUP_CASES)
@pytest.mark.parametrize("cls", ["ARWMH", "ASSS"])
def test_group_pnx_second_item_bitexact(cls, kind, d, npts, ns, gpu, orc):
    """sample_pnx_kernel (amh_kernels.hip launch_pnx, grid_for) and
    asss_pnx_kernel (amh_asss.hip, the same cap: 8,192 blocks x 4 waves = 32,768
    items of CPW chains) at 32,768 + r items with a tail group of fewer than
    CPW chains, n = 3: the registers' factor and the staged model data serve a
    second item; key, start point, pe and the tail clamp are recomputed; the
    slice transition's U, dl and mu, passed by reference, start a second item."""
    _case(cls, kind, d, npts, ns, 3, orc, GROUP_CAP, steps=50, chain=3)


@pytest.mark.parametrize("cls", ["ARWMH", "ASSS"])
def test_group_pnx_third_item_bitexact(cls, gpu, orc):
    """The mixture at d = 3 (G = 4, 16 chains per item) and 17 x 61,681 =
    1,048,577 chains = 2 x 32,768 x 16 + 1 (grid_for's cap, amh_kernels.hip and
    amh_asss.hip): every wave takes two items, wave 0 a third that holds one
    chain."""
    assert 17 * 61681 == 2 * GROUP_CAP * 16 + 1
    _case(cls, "mixture", 3, 17, 61681, 3, orc, GROUP_CAP, steps=50, chain=3, passes=3)


# --------------------------------------------------- C. external potential ----
def test_external_arwmh_pnx_second_item_bitexact(gpu, orc):
    """pnx_ext_kernel<64, false / true> (amh_kernels.hip run_pnx_ext: d > 32
    runs G = 64, one chain per wave, under grid_for's cap of 32,768 items) with
    U = the registry kernel's potential, d = 40, 3 x 10,947 = 32,841 chains,
    n = 3 (tests/test_gpu_external.py's set-up)."""
    from kernels_amd import ARWMH, PRNGKey
    d, npts, ns, n = 40, 3, 10947, 3
    cpw = 1 if d > 32 else 2  # run_pnx_ext's own choice
    assert items_per_wave(npts * ns, GROUP_CAP, cpw) == 2, "no wave takes a second item: the cap moved"
    kw, mk, om = make_case("gaussian", d)
    kg = ARWMH(num_chains=8, **kw)
    z0 = np.random.default_rng(0).uniform(-2, 2, size=(8, d)).astype(np.float32)
    st = kg.init(PRNGKey(1), 0, torch.as_tensor(z0), (), mk)
    st = kg.sample_(st, 30)
    theta = tuple(t[2].clone() for t in st.adapt_state)
    ke = ARWMH(potential_fn=lambda z: kg.potential(z), num_chains=8)
    ke.init(PRNGKey(1), 0, torch.as_tensor(z0), (), {})
    x = np.random.default_rng(3).normal(size=(npts, d)).astype(np.float32)
    out = ke.sample_Pnx(PRNGKey(KEY), x, theta, n=n, n_samples=ns)
    ref = _oracle_pnx(orc, om, "ARWMH", x, theta, n, ns)
    _compare(out, ref, x, "ARWMH", GROUP_CAP, cpw, f"external ARWMH d={d} sample_Pnx")


def test_external_asss_pnx_second_item_bitexact(gpu, orc):
    """asss_ext_begin_kernel<32, true>, asss_ext_shrink_kernel<32> and
    asss_ext_pnx_finish_kernel<32> (amh_asss_ext.hip launch_ext: 32,768 items
    per pass at the lane-group width of d, two chains per item at d = 24) with
    U = the registry kernel's potential, 3 x 21,869 = 65,607 chains, n = 3
    (tests/test_gpu_asss_external.py's set-up)."""
    from kernels_amd import ASSS, PRNGKey
    from test_gpu_asss_external import _registry
    d, npts, ns, n = 24, 3, 21869, 3
    cpw = 64 // orc.group_width(d)  # ExtF in amh_asss_ext.hip: Geo<D>::CPW at dispatch_dim's D
    assert cpw == 2 and (npts * ns) % cpw == 1
    assert items_per_wave(npts * ns, GROUP_CAP, cpw) == 2, "no wave takes a second item: the cap moved"
    kg, st, om = _registry("gaussian", d)
    kg.sample_(st, 30)
    theta = tuple(t[2].clone() for t in st.adapt_state)
    ke = ASSS(potential_fn=lambda z: kg.potential(z), host_shrink=True)
    x = np.random.default_rng(3).normal(size=(npts, d)).astype(np.float32)
    out = ke.sample_Pnx(PRNGKey(KEY), x, theta, n=n, n_samples=ns)
    ref = _oracle_pnx(orc, om, "ASSS", x, theta, n, ns)
    assert ke.shrink_rounds >= 3, ke.shrink_rounds
    _compare(out, ref, x, "ASSS", GROUP_CAP, cpw, f"external ASSS d={d} sample_Pnx")
