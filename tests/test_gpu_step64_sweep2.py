"""Sweep 2 of the d = 64 step kernel's rank-one update (arwmh_step64_kernel,
its three instances: single-step ARWMH, fused ARWMH, ASSS).  The four
coefficients of a column (w*_j, c_j and the two as_change factors) go through
the wave's scratch a quarter of the columns at a time into every row of 16
lanes (s64_rows_quarter) and reach the FMAs as DPP row broadcasts of lane
j mod 16 (s64_sweep2_group): a wrong quarter, lane or mask shows up as wrong
words of `scale` in the columns of that quarter and in as_change.

Every comparison is bit for bit against the C oracle on whole states, scale and
as_change included (states that hold NaN: identical NaN positions, every other
word identical), with the helpers of the swap and the compute tests: a factor
whose 2,080 packed entries all differ and num_warmup = 2, so that of the
single-step launches the first and the third take gamma = 1 (keep L, the
factor is copied verbatim) and the second and the fourth update it.

Shapes: C = 1, 17 and 4,097, as in test_gpu_step64_compute."""
import copy

import numpy as np
import pytest
import torch

from helpers import ASSS_FIELDS, _leaf, assert_state_bitequal, assert_state_bitequal_nan
from test_gpu_step64_compute import SHAPES, W, _start_distinct
from test_gpu_step64_order import _assert_same, _order, _start
from test_gpu_step64_swap import _col

pytestmark = pytest.mark.gpu

SINGLE, FUSED = 4, 3


def _edit(state, fn):
    """fn(z, loc, scale, potential_energy) on host copies of a product or an
    oracle state, written back."""
    leaves = [_leaf(state, f) for f in ("z", "loc", "scale", "potential_energy")]
    host = [a.detach().cpu().numpy().copy() if torch.is_tensor(a) else a for a in leaves]
    fn(*host)
    for a, h in zip(leaves, host):
        if torch.is_tensor(a):
            a.copy_(torch.from_numpy(h))
    if torch.is_tensor(leaves[0]):
        torch.cuda.synchronize()


@pytest.mark.parametrize("C", SHAPES)
def test_arwmh_single_then_fused(C, gpu, orc):
    """Four single-step launches (the single-step instance; the second and the
    fourth update L), then a fused launch of three steps (the fused instance,
    three updates with U kept in registers)."""
    k, st, om, ost = _start_distinct(C, orc)
    for t in range(SINGLE):
        before = ost.scale.copy()
        k.sample_(st, 1)
        orc.step(om, ost, 1, num_warmup=W)
        torch.cuda.synchronize()
        assert_state_bitequal(st, ost, f"C={C} launch {t + 1}")
        changed = (ost.scale.view(np.uint32) != before.view(np.uint32)).any(axis=1)
        assert changed.all() if t % 2 == 1 else not changed.any()
    k.sample_(st, FUSED)
    orc.step(om, ost, FUSED, num_warmup=W)
    torch.cuda.synchronize()
    assert_state_bitequal(st, ost, f"C={C} fused launch of {FUSED}")
    assert int(ost.i[0]) == SINGLE + FUSED


def test_asss_single_then_fused(gpu, orc):
    """The same launches for the ASSS instance."""
    from test_gpu_asss import assert_bitequal
    C = 17
    k, st, om, ost = _start_distinct(C, orc, cls="ASSS")
    for t, n in enumerate([1] * SINGLE + [FUSED]):
        k.sample_(st, n)
        orc.asss_step(om, ost, n, num_warmup=W)
        torch.cuda.synchronize()
        assert_bitequal(st, ost, f"ASSS launch {t + 1} ({n} steps)")
    assert_state_bitequal_nan(st, ost, "ASSS final", ASSS_FIELDS)


# chain -> the column whose diagonal entry is spoilt: in a block's range of
# eight or nine chains, first and second items of a wave, each between chains
# that update
BAD = {1: 0, 4: 31, 10: 62, 13: 63}


@pytest.mark.parametrize("value", [0.0, np.inf, np.nan], ids=["zero", "inf", "nan"])
def test_kept_factor_beside_updated_chains(value, gpu, orc):
    """Chains whose diagonal holds 0, inf or NaN in column 0, 31, 62 or 63 fail
    the pivot test in every step (sweep 2 is skipped, the factor is kept),
    their neighbours update: five single-step launches and a fused one, every
    state compared, so that what a skipped sweep 2 leaves in the wave's
    registers (the unit and zero pattern of U) is pinned by the chain after
    it, in both chain orders."""
    C = 17
    k, st, om, ost = _start_distinct(C, orc)

    def spoil(z, loc, scale, pe):
        for c, j in BAD.items():
            scale[c, _col(j)] = np.float32(value)
    _edit(st, spoil)
    _edit(ost, spoil)
    first = ost.scale.copy()
    bad = np.array(sorted(BAD))
    good = np.setdiff1d(np.arange(C), bad)
    for t, n in enumerate([1, 1, 1, 1, 1, FUSED]):
        before = ost.scale.copy()
        k.sample_(st, n)
        orc.step(om, ost, n, num_warmup=W)
        torch.cuda.synchronize()
        assert_state_bitequal_nan(st, ost, f"diagonal {value}, launch {t + 1}")
        changed = (ost.scale.view(np.uint32) != before.view(np.uint32)).any(axis=1)
        assert not changed[bad].any()
        assert changed[good].all() if t in (1, 3, 4, 5) else not changed[good].any()
    np.testing.assert_array_equal(ost.scale[bad].view(np.uint32), first[bad].view(np.uint32))
    assert np.isfinite(ost.scale[good]).all() and np.isfinite(ost.z[good]).all()


# chain -> what delta = z - loc holds at coordinates 0, 31 and 63 of a rejected step
EXTREME = {2: "+0", 5: "-0", 8: "denormal", 11: "1e18", 14: "all"}
COORDS = [0, 31, 63]


def _extreme_delta(z, loc, scale, pe):
    for c, kind in EXTREME.items():
        pe[c] = np.float32(-1e30)  # exp(pe - pe') = 0: the proposal is rejected, delta = z - loc
        if kind == "+0":
            z[c, COORDS] = loc[c, COORDS]
        elif kind == "-0":
            z[c, COORDS], loc[c, COORDS] = np.float32(-0.0), np.float32(0.0)
        elif kind == "denormal":
            z[c, COORDS], loc[c, COORDS] = np.float32(1e-45), np.float32(0.0)
        elif kind == "1e18":
            z[c, COORDS], loc[c, COORDS] = np.float32(1e18), np.float32(0.0)
        else:
            loc[c, :4] = np.float32(0.0)
            z[c, :4] = np.array([0.0, -0.0, 1e-45, -1e18], np.float32)
            z[c, 60:], loc[c, 60:] = np.array([1e18, -1e-45, -0.0, 1e18], np.float32), np.float32(0.0)


def test_coefficient_extremes(gpu, orc):
    """delta with +-0, denormal and 1e18 components in an updating step that
    directly follows an n = 1 step (gamma = 1), and the step after it: the
    coefficients w*_j, c_j and the as_change factors reach sweep 2 as they
    are, and none of these chains reverts."""
    C = 17
    k, st, om, ost = _start_distinct(C, orc)
    for t in range(3):  # i = 0, 1, 2: the third is the n = 1 step after the warm-up
        k.sample_(st, 1)
        orc.step(om, ost, 1, num_warmup=W)
        torch.cuda.synchronize()
        assert_state_bitequal(st, ost, f"launch {t + 1}")
    assert int(ost.i[0]) == W + 1
    _edit(st, _extreme_delta)
    _edit(ost, _extreme_delta)
    delta = ost.z - ost.loc
    assert delta[2, 31] == 0.0 and not np.signbit(delta[2, 31]) and np.signbit(delta[5, 31]) and delta[5, 31] == 0.0
    assert 0.0 < delta[8, 63] < 1e-38 and delta[11, 0] == np.float32(1e18) and delta[14, 3] == np.float32(-1e18)
    chains = np.array(sorted(EXTREME))
    for t in range(2):  # n = 2, 3: both update
        before = copy.deepcopy(ost)
        k.sample_(st, 1)
        orc.step(om, ost, 1, num_warmup=W)
        torch.cuda.synchronize()
        assert_state_bitequal(st, ost, f"extreme delta, launch {t + 1}")
        # the scenario is what it claims: rejected, updated, finite
        np.testing.assert_array_equal(ost.z[chains].view(np.uint32), before.z[chains].view(np.uint32))
        assert (ost.scale.view(np.uint32) != before.scale.view(np.uint32)).any(axis=1).all()
        assert np.isfinite(ost.scale).all() and np.isfinite(ost.as_change).all()
    k.sample_(st, FUSED)
    orc.step(om, ost, FUSED, num_warmup=W)
    torch.cuda.synchronize()
    assert_state_bitequal(st, ost, "extreme delta, fused launch")


@pytest.mark.parametrize("C", [17, 4097])
def test_two_handles_in_opposite_directions(C, gpu, orc):
    """The same launches on two handles: from the second launch on, one walks
    its chains descending where the other walks them ascending.  Equal states,
    both equal to the oracle's."""
    k_a, st_a, om, ost = _start_distinct(C, orc)
    k_b, st_b, _, _ = _start_distinct(C, orc)
    k_0, _, _, _ = _start(C, orc, W)
    orders_a, orders_b = [], []
    for t, n in enumerate([1] * SINGLE + [FUSED]):
        k_a.sample_(st_a, n)
        orders_a.append(_order(k_a))
        h = k_0 if t == 0 else k_b  # st_b's first launch goes through a third handle: k_b starts a launch late
        h.sample_(st_b, n)
        orders_b.append(_order(h))
        orc.step(om, ost, n, num_warmup=W)
        torch.cuda.synchronize()
        assert_state_bitequal(st_a, ost, f"C={C} handle a, launch {t + 1}")
        assert_state_bitequal(st_b, ost, f"C={C} handle b, launch {t + 1}")
        _assert_same(st_a, st_b, f"C={C} launch {t + 1}")
    assert orders_a == [0, 1, 0, 1, 0]
    assert orders_b == [0, 0, 1, 0, 1]
