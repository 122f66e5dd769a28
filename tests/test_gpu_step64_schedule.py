"""The d = 64 step kernel's cache policy by position (arwmh_step64_kernel,
csrc/amh_s64_sched.h): a drawn chain carries its class (hot / mid / tail)
above its index, and the class picks which instantiation of the DMA prefetch
and of the factor flush moves it.

No class may change a bit or lose a chain, so every comparison is whole-state
bit equality with the C oracle, and again with the same launches made through a
fresh handle each (always ascending, never chained: no hot part), as
tests/test_gpu_step64_order.py does.  W = 2 throughout: launches 1 and 3 keep
the factor (gamma = 1: the verbatim copy), 2 and 4 update it (the flush).

Sizes.  The launch has min(256, ceil(C / 16)) blocks and a block of n chains
has h = floor(3 n / 8) hot and h tail chains.
* 12,325 = 256 * 48 + 37: blocks own 48 or 49 chains (h = 18), ragged ranges,
  every wave draws 3-4 chains of more than one class.
* 2, 3, 4: one block whose hot count goes 0 -> 1 -> 1 (every chain mid at 2;
  hot, mid and tail one chain each at 3).
* 767, 768, 769: the two C nearest 256 * ceil(8 / 3) and that C itself -- 48 or
  49 blocks of 15-16 chains here, h = 5 or 6 by block.
* 1, 15, 17, 255, 257, 4,097: the edges of the counter-to-chain mapping (one
  block of one wave; one block short of, and two blocks around, 16 waves; 256
  blocks, one with 17 chains).
* 5,504 = 256 * 21 + 128: half the blocks own 21 chains (h = 7), half 22
  (h = 8).  Blocks with hot counts 0 and 1 in one launch cannot occur: a
  launch of more than one block gives every block at least 8 chains, so the
  nearest mix of two hot counts is tested instead."""
import copy

import numpy as np
import pytest
import torch

from helpers import assert_state_bitequal, make_case
from test_gpu_step64_order import _assert_same, _clone, _order, _start

pytestmark = pytest.mark.gpu

C_RAGGED = 12325
W = 2


def _fresh_kernel(C, cls="ARWMH"):
    """A kernel object with a handle that has launched nothing: its next launch is ascending, unchained."""
    import kernels_amd
    kw, mk, _ = make_case("gaussian", 64)
    k = getattr(kernels_amd, cls)(num_chains=C, **kw)
    k.init(kernels_amd.PRNGKey(1), W, torch.zeros(C, 64), (), mk)
    assert _order(k) == -1
    return k


def _launches(C, n_launch, orc, out_of_place=(), cls="ARWMH", check=assert_state_bitequal, ostep=None):
    """n_launch single-step launches on one kernel object (orders 0, 1, 0, ...),
    those in `out_of_place` through sample(); each against the oracle and
    against the same launch through a fresh handle."""
    ostep = ostep or orc.step
    k, st_a, om, ost = _start(C, orc, W, cls=cls)
    st_b = _clone(st_a)
    for t in range(n_launch):
        if t in out_of_place:
            st_a = k.sample(st_a, (), {})  # a new state: an unvisited chain would be uninitialised memory
        else:
            k.sample_(st_a, 1)
        assert _order(k) == t % 2
        fresh = _fresh_kernel(C, cls)
        fresh.sample_(st_b, 1)
        assert _order(fresh) == 0
        torch.cuda.synchronize()
        del fresh
        ostep(om, ost, 1, num_warmup=W)
        check(st_a, ost, f"{cls} C={C} chained, launch {t + 1}")
        check(st_b, ost, f"{cls} C={C} fresh handles, launch {t + 1}")
        _assert_same(st_a, st_b, f"{cls} C={C} launch {t + 1}")


def test_ragged_in_and_out_of_place(gpu, orc):
    """Six launches at C = 12,325, the third and the sixth out of place."""
    _launches(C_RAGGED, 6, orc, out_of_place=(2, 5))


@pytest.mark.parametrize("C", [1, 2, 3, 4, 15, 17, 255, 257, 767, 768, 769, 4097, 5504])
def test_split_edges(C, gpu, orc):
    """Four alternating launches at the edges of the hot / mid / tail split."""
    _launches(C, 4, orc)


def test_collection_in_a_chained_launch(gpu, orc):
    """run() with thinned collection of z and pe right after a sample_(): the
    launch is descending and chained, and every slot and the accept counters
    match."""
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
    # first half of the fused four), slot 1's from the final state
    half = copy.deepcopy(ost)
    orc.step(om, half, 2, num_warmup=W)
    ocz = orc.step(om, ost, 4, num_warmup=W, accept_count=acc, collect_z=True)
    np.testing.assert_array_equal(ocz[1].view(np.uint32), half.z.view(np.uint32))
    np.testing.assert_array_equal(cz.cpu().numpy().view(np.uint32), ocz[1::2].view(np.uint32))
    for slot, o in enumerate((half, ost)):
        np.testing.assert_array_equal(cp[slot].cpu().numpy().view(np.uint32), o.potential_energy.view(np.uint32))
    assert_state_bitequal(st, ost, "run(4, thinning=2) descending, chained")
    np.testing.assert_array_equal(k.accept_count.cpu().numpy(), acc)


def test_asss_four_launches(gpu, orc):
    """The ASSS instantiation draws through the same counter and classes."""
    from test_gpu_asss import assert_bitequal
    _launches(C_RAGGED, 4, orc, cls="ASSS", check=assert_bitequal, ostep=orc.asss_step)
