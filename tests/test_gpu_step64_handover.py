"""The d = 64 step kernel's pipelined hand-over (arwmh_step64_kernel, ARWMH and
ASSS): while the swap walks the columns, each finished 1-KB piece of the
outgoing chain's factor is stored and the same piece of the chain after next
is DMA'd into its place.

What can go wrong is an overlap inside one wave: the store of chain k - 1, the
registers of chain k and the refill for chain k + 1 share one LDS buffer, so a
refill that lands early, or a piece stored before its last column was written,
shows up as wrong words of `scale` near a piece boundary.  That needs a wave
that takes at least three chains in a row, i.e. C > 2 * 4,096 (256 blocks x 16
waves): 12,325 = 256 * 48 + 37 gives every wave 3-4 items with ragged block
ranges.  Every comparison is bit for bit against the C oracle on whole states.

num_warmup = 2 makes launches 1 and 3 keep L (gamma = 1: the verbatim copy,
the hand-over in today's order) and launches 2, 4, 5, ... update it (the
pipelined hand-over)."""
import copy

import numpy as np
import pytest
import torch

from helpers import _leaf, assert_state_bitequal
from test_gpu_step64_order import C_RAGGED, _order, _start

pytestmark = pytest.mark.gpu

W = 2


def _alternating(cls, n_launch, orc, check, ostep):
    k, st, om, ost = _start(C_RAGGED, orc, W, cls=cls)
    for t in range(n_launch):
        k.sample_(st, 1)
        assert _order(k) == t % 2
        ostep(om, ost, 1, num_warmup=W)
        torch.cuda.synchronize()
        check(st, ost, f"{cls} launch {t + 1}")


def test_alternating_in_place_arwmh(gpu, orc):
    """Six alternating in-place launches, the state checked after every one."""
    _alternating("ARWMH", 6, orc, assert_state_bitequal, orc.step)


def test_alternating_in_place_asss(gpu, orc):
    """The ASSS instantiation: four launches against orc.asss_step."""
    from test_gpu_asss import assert_bitequal
    _alternating("ASSS", 4, orc, assert_bitequal, orc.asss_step)


def _zero_first_pivot(state, every=5):
    """L_00 = 0 for every fifth chain, on a product state (in place, through the
    host) or an orc.State: sqrt(1 - gamma) L_00 = 0 fails the update's pivot
    test, so the update is reverted in every later step and the factor is
    copied verbatim, with every value finite on both sides."""
    scale = _leaf(state, "scale")
    if hasattr(state, "adapt_state"):
        a = scale.detach().cpu().numpy().copy()
        a[::every, 0] = 0.0
        scale.copy_(torch.from_numpy(a))
    else:
        scale[::every, 0] = 0.0


def test_kept_and_updated_factors_interleaved(gpu, orc):
    """Every fifth chain's update reverted among updated neighbours: pipelined
    -> verbatim -> pipelined hand-overs between consecutive items of a wave."""
    k, st, om, ost = _start(C_RAGGED, orc, W)
    k.sample_(st, 3)
    orc.step(om, ost, 3, num_warmup=W)
    torch.cuda.synchronize()
    assert_state_bitequal(st, ost, "three fused steps in")
    _zero_first_pivot(st)
    _zero_first_pivot(ost)
    before = ost.scale.copy()
    for t in range(4):
        k.sample_(st, 1)
        assert _order(k) == (t + 1) % 2
        orc.step(om, ost, 1, num_warmup=W)
        torch.cuda.synchronize()
        assert_state_bitequal(st, ost, f"interleaved launch {t + 1}")
    # the scenario is what it claims: those factors were kept, the others changed
    changed = (ost.scale.view(np.uint32) != before.view(np.uint32)).any(axis=1)
    assert not changed[::5].any()
    assert changed[np.arange(C_RAGGED) % 5 != 0].all()


def test_out_of_place_chaining(gpu, orc):
    """Four sample() launches (input and output buffers differ)."""
    k, st, om, ost = _start(C_RAGGED, orc, W)
    for t in range(4):
        st = k.sample(st, (), {})
        assert _order(k) == t % 2
        orc.step(om, ost, 1, num_warmup=W)
        torch.cuda.synchronize()
        assert_state_bitequal(st, ost, f"sample() launch {t + 1}")


def test_fused_run_with_collection(gpu, orc):
    """run(4, thinning=2) collecting z and pe right after a sample_(): four
    transitions per chain between two hand-overs, in a descending launch."""
    k, st, om, ost = _start(C_RAGGED, orc, W)
    acc = np.zeros(C_RAGGED, np.int32)
    k.sample_(st, 1)
    st, cz, cp = k.run(st, 4, thinning=2, collect_z=True, collect_pe=True)
    assert _order(k) == 1
    torch.cuda.synchronize()
    orc.step(om, ost, 1, num_warmup=W, accept_count=acc)
    half = copy.deepcopy(ost)
    orc.step(om, half, 2, num_warmup=W)
    ocz = orc.step(om, ost, 4, num_warmup=W, accept_count=acc, collect_z=True)
    np.testing.assert_array_equal(cz.cpu().numpy().view(np.uint32), ocz[1::2].view(np.uint32))
    for slot, o in enumerate((half, ost)):
        np.testing.assert_array_equal(cp[slot].cpu().numpy().view(np.uint32), o.potential_energy.view(np.uint32))
    assert_state_bitequal(st, ost, "run(4, thinning=2)")
    np.testing.assert_array_equal(k.accept_count.cpu().numpy(), acc)


@pytest.mark.parametrize("C", [1, 17, 4097, 8193])
def test_item_count_edges(C, gpu, orc):
    """No next item; a second item for one wave only; a third item for exactly
    one wave.  Two launches: the first keeps L, the second updates it."""
    k, st, om, ost = _start(C, orc, W)
    for t in range(2):
        k.sample_(st, 1)
        orc.step(om, ost, 1, num_warmup=W)
        torch.cuda.synchronize()
        assert_state_bitequal(st, ost, f"C={C} launch {t + 1}")
