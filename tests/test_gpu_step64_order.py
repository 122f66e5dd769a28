"""The d = 64 step kernel's alternating chain order (arwmh_step64_kernel, ARWMH
and ASSS; amh_capi.hip step64_order).

A launch whose input is what the handle's previous d = 64 launch wrote walks
every block's chain range in the opposite order, so that its first reads hit
what that launch wrote last.  Chains are independent, so the order may not
change one bit: every test here compares whole states with the C oracle, and
reads the order each launch took through amh_step_order, since a broken
pointer comparison would otherwise only lose the speed-up, silently.

Sizes: one chain per wave ends at C = 4,096 (256 blocks x 16 waves).  At
12,325 = 256 * 48 + 37 the blocks own 48 or 49 chains, so every wave takes 3-4
items and the block ranges are ragged; 1, 15, 17 and 4,097 are the edges of
the ticket-to-chain mapping (one block of one wave; one block short of, and
two blocks around, 16 waves; exactly one wave with two items)."""
import copy

import numpy as np
import pytest
import torch

from helpers import assert_state_bitequal, make_case

pytestmark = pytest.mark.gpu

C_RAGGED = 12325


def _start(C, orc, W, cls="ARWMH", seed=0):
    """A kernel object, its initial state and the oracle's twin."""
    import kernels_amd
    kw, mk, om = make_case("gaussian", 64)
    k = getattr(kernels_amd, cls)(num_chains=C, **kw)
    key = kernels_amd.PRNGKey(seed)
    z0 = np.random.default_rng(seed + C).uniform(-2, 2, size=(C, 64)).astype(np.float32)
    st = k.init(key, W, torch.as_tensor(z0), (), mk)
    ost = orc.init(om, key, C, init_z=z0)
    torch.cuda.synchronize()
    return k, st, om, ost


def _clone(st):
    """A deep copy of a product state (namedtuple of tensors, one level of nesting)."""
    return type(st)(*[x.clone() if torch.is_tensor(x) else type(x)(*[t.clone() for t in x]) for x in st])


def _leaves(st):
    for x in st:
        if torch.is_tensor(x):
            yield x
        else:
            yield from x


def _assert_same(a, b, what):
    for n, (x, y) in enumerate(zip(_leaves(a), _leaves(b))):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"{what}: leaf {n} differs"


def _order(k):
    return k._handle.step_order()


def _direction_independence(cls, n_launch, orc, check, ostep):
    W = 1  # launches 1 (ascending) and 2 (descending) both take gamma = 1: keep L, the verbatim copy
    k, st_a, om, ost = _start(C_RAGGED, orc, W, cls=cls)
    st_b = _clone(st_a)
    assert _order(k) == -1
    orders_a, orders_b = [], []
    for t in range(n_launch):
        k.sample_(st_a, 1)
        orders_a.append(_order(k))
        fresh, _, _, _ = _start(C_RAGGED, orc, W, cls=cls)  # a fresh handle: always ascending
        assert _order(fresh) == -1
        fresh.sample_(st_b, 1)
        orders_b.append(_order(fresh))
        torch.cuda.synchronize()
        del fresh
        ostep(om, ost, 1, num_warmup=W)
        check(st_a, ost, f"{cls} alternating, launch {t + 1}")
        check(st_b, ost, f"{cls} ascending, launch {t + 1}")
        _assert_same(st_a, st_b, f"{cls} launch {t + 1}")
    assert orders_a == [t % 2 for t in range(n_launch)]
    assert orders_b == [0] * n_launch


def test_direction_independence_arwmh(gpu, orc):
    """Six in-place launches on one kernel object (orders 0, 1, 0, 1, 0, 1) against
    the same six each through a fresh kernel object (always 0) and the oracle."""
    _direction_independence("ARWMH", 6, orc, assert_state_bitequal, orc.step)


def test_direction_independence_asss(gpu, orc):
    """The ASSS instantiation: four launches, against orc.asss_step."""
    from test_gpu_asss import assert_bitequal
    _direction_independence("ASSS", 4, orc, assert_bitequal, orc.asss_step)


def test_out_of_place_chaining(gpu, orc):
    """sample() returns a new state each time: the launch that reads what the
    last one wrote still alternates, and equals the in-place sequence; a launch
    on an unrelated state in between resets the order to ascending."""
    W = 3
    k, st, om, ost = _start(C_RAGGED, orc, W)
    k2, st2, _, _ = _start(C_RAGGED, orc, W)
    other = _clone(st)
    orders, orders2 = [], []
    ost_first = None
    for t in range(4):
        st = k.sample(st, (), {})
        orders.append(_order(k))
        k2.sample_(st2, 1)
        orders2.append(_order(k2))
        orc.step(om, ost, 1, num_warmup=W)
        if t == 0:
            ost_first = copy.deepcopy(ost)
    torch.cuda.synchronize()
    assert orders == [0, 1, 0, 1] and orders2 == [0, 1, 0, 1]
    assert_state_bitequal(st, ost, "four sample() launches")
    assert_state_bitequal(st2, ost, "four sample_() launches")
    st = k.sample(st, (), {})
    assert _order(k) == 0
    other = k.sample(other, (), {})  # not what the last launch wrote: ascending (alternation would say 1)
    assert _order(k) == 0
    st = k.sample(st, (), {})        # nor is this, any more
    assert _order(k) == 0
    st = k.sample(st, (), {})
    assert _order(k) == 1
    for _ in range(3):  # single launches: a fused call keeps U in registers between steps (other bits)
        orc.step(om, ost, 1, num_warmup=W)
    torch.cuda.synchronize()
    assert_state_bitequal(st, ost, "seven sample() launches around an unrelated one")
    assert_state_bitequal(other, ost_first, "the unrelated state's launch")


def test_collection_in_a_descending_launch(gpu, orc):
    """run() with thinned collection of z and pe right after a sample_(): the
    launch is descending, and every slot and the accept counters match."""
    W = 3
    k, st, om, ost = _start(C_RAGGED, orc, W)
    acc = np.zeros(C_RAGGED, np.int32)
    k.sample_(st, 1)
    assert _order(k) == 0
    st, cz, cp = k.run(st, 4, thinning=2, collect_z=True, collect_pe=True)
    assert _order(k) == 1
    torch.cuda.synchronize()
    orc.step(om, ost, 1, num_warmup=W, accept_count=acc)
    assert cz.shape == (2, C_RAGGED, 64) and cp.shape == (2, C_RAGGED)
    # the oracle collects z only: slot 0's pe from a fused two-step call (the
    # first half of the fused four: the same arithmetic up to there), slot 1's
    # from the final state
    half = copy.deepcopy(ost)
    orc.step(om, half, 2, num_warmup=W)
    ocz = orc.step(om, ost, 4, num_warmup=W, accept_count=acc, collect_z=True)
    np.testing.assert_array_equal(ocz[1].view(np.uint32), half.z.view(np.uint32))
    np.testing.assert_array_equal(cz.cpu().numpy().view(np.uint32), ocz[1::2].view(np.uint32))
    for slot, o in enumerate((half, ost)):
        np.testing.assert_array_equal(cp[slot].cpu().numpy().view(np.uint32), o.potential_energy.view(np.uint32))
    assert_state_bitequal(st, ost, "run(4, thinning=2) descending")
    np.testing.assert_array_equal(k.accept_count.cpu().numpy(), acc)


@pytest.mark.parametrize("C", [1, 15, 17, 4097])
def test_mapping_edges(C, gpu, orc):
    """Four alternating single-step launches at the edges of the mapping; W = 2
    mixes kept (gamma = 1) and updated factors over the four."""
    W = 2
    k, st, om, ost = _start(C, orc, W)
    acc = np.zeros(C, np.int32)
    for t in range(4):
        k.sample_(st, 1)
        assert _order(k) == t % 2
        orc.step(om, ost, 1, num_warmup=W, accept_count=acc)
        torch.cuda.synchronize()
        assert_state_bitequal(st, ost, f"C={C} launch {t + 1}")
    np.testing.assert_array_equal(k.accept_count.cpu().numpy(), acc)
