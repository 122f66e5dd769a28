"""Row broadcasts of the d = 64 step kernel (arwmh_step64_kernel, its three
instances: single-step ARWMH, fused ARWMH, ASSS).  In a single-step ARWMH
launch a per-lane vector is copied into every row of 16 lanes by permlane
swaps (s64_rows) and column j's FMA takes lane j mod 16 of quarter j / 16 as a
DPP row_newbcast operand: the proposal's vector (s64_matvec_rows), the
potential's (s64_gauss_pot_rows) and sweep 2's four coefficient vectors
(s64_sweep2<true>); the fused and the ASSS instance take theirs through the
wave's scratch.  A wrong quarter, row or lane picks another coordinate's
value, so the cases put a value into one coordinate at the edges of the
quarters and compare everything, in single-step and in fused launches.

Every comparison is bit for bit against the C oracle on whole states (states
that hold NaN: identical NaN positions, every other word identical), with the
helpers of the sweep-2 tests: a factor whose 2,080 packed entries all differ
and num_warmup = 2, so that of the single-step launches the first and the
third take gamma = 1 (keep L) and the second and the fourth update it.

Shapes: C = 1, 17 and 4,097 (a wave takes a second item), as in
test_gpu_step64_compute; the cases that place values use the smallest C that
holds their chains."""
import copy

import numpy as np
import pytest
import torch

from helpers import ASSS_FIELDS, assert_state_bitequal, assert_state_bitequal_nan
from test_gpu_step64_compute import SHAPES, W, _start_distinct
from test_gpu_step64_order import _assert_same, _order, _start
from test_gpu_step64_swap import DIAG, _col
from test_gpu_step64_sweep2 import FUSED, SINGLE, _edit

pytestmark = pytest.mark.gpu

LAUNCHES = [1] * SINGLE + [FUSED]


def _changed(after, before):
    return (after.view(np.uint32) != before.view(np.uint32)).any(axis=1)


@pytest.mark.parametrize("C", SHAPES)
def test_arwmh_three_instances(C, gpu, orc):
    """Four single-step launches (the single-step instance; the second and the
    fourth update L), then a fused launch of three steps (the fused instance),
    on two handles that walk their chains in opposite directions."""
    k_a, st_a, om, ost = _start_distinct(C, orc)
    k_b, st_b, _, _ = _start_distinct(C, orc)
    k_0, _, _, _ = _start(C, orc, W)
    orders_a, orders_b = [], []
    for t, n in enumerate(LAUNCHES):
        before = ost.scale.copy()
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
        changed = _changed(ost.scale, before)
        assert changed.all() if t in (1, 3, 4) else not changed.any()
    assert orders_a == [0, 1, 0, 1, 0] and orders_b == [0, 0, 1, 0, 1]
    assert int(ost.i[0]) == SINGLE + FUSED and np.isfinite(ost.scale).all()


def test_asss_instance(gpu, orc):
    """The same launches for the ASSS instance (S z, S v, every potential and
    sweep 2 through the scratch, sweep 1 shared with ARWMH)."""
    from test_gpu_asss import assert_bitequal
    C = 17
    k, st, om, ost = _start_distinct(C, orc, cls="ASSS")
    first = ost.scale.copy()
    for t, n in enumerate(LAUNCHES):
        k.sample_(st, n)
        orc.asss_step(om, ost, n, num_warmup=W)
        torch.cuda.synchronize()
        assert_bitequal(st, ost, f"ASSS launch {t + 1} ({n} steps)")
    assert_state_bitequal_nan(st, ost, "ASSS final", ASSS_FIELDS)
    assert _changed(ost.scale, first).all() and np.isfinite(ost.scale).all()


# the first and the last lane of every row of 16: the edges of the quarters
EDGES = [0, 15, 16, 31, 32, 47, 48, 63]
C_ONE = 1 + 2 * len(EDGES)


def _one_coordinate(z, loc, scale, pe):
    """Chain 1 + i: the factor's diagonal is zero but for L_jj, j = EDGES[i], so
    the proposal's vector eta = diag(L) xi is nonzero in coordinate j alone
    (and every update is reverted on the zero pivots); chain 9 + i keeps its
    factor.  In both z - loc is nonzero in coordinate j alone."""
    for i, j in enumerate(EDGES):
        a, b = 1 + i, 1 + len(EDGES) + i
        keep = scale[a, _col(j)]
        scale[a, DIAG] = np.float32(0.0)
        scale[a, _col(j)] = keep
        for c, v in ((a, 1.5), (b, -0.75)):
            z[c] = loc[c]
            z[c, j] = loc[c, j] + np.float32(v)


def test_one_coordinate(gpu, orc):
    """The proposal's vector and z - loc nonzero in exactly one coordinate, at
    the edges of the quarters: a wrong row, quarter or lane index reads a zero
    (or another chain's nothing) and changes z, potential_energy and the accept
    decision of that chain."""
    C = C_ONE
    k, st, om, ost = _start_distinct(C, orc)
    _edit(st, _one_coordinate)
    _edit(ost, _one_coordinate)
    one_hot = np.arange(1, 1 + len(EDGES))
    rest = np.setdiff1d(np.arange(C), one_hot)
    for i, j in enumerate(EDGES):
        for c in (1 + i, 1 + len(EDGES) + i):
            assert np.flatnonzero(ost.z[c] - ost.loc[c]).tolist() == [j]
        assert np.flatnonzero(ost.scale[1 + i, DIAG]).tolist() == [j]
    first, z0 = ost.scale.copy(), ost.z.copy()
    for t, n in enumerate(LAUNCHES):
        before = ost.scale.copy()
        k.sample_(st, n)
        orc.step(om, ost, n, num_warmup=W)
        torch.cuda.synchronize()
        assert_state_bitequal(st, ost, f"one coordinate, launch {t + 1}")
        changed = _changed(ost.scale, before)
        assert not changed[one_hot].any()
        assert changed[rest].all() if t in (1, 3, 4) else not changed[rest].any()
    np.testing.assert_array_equal(ost.scale[one_hot].view(np.uint32), first[one_hot].view(np.uint32))
    for f in ("z", "loc", "scale", "potential_energy", "as_change"):
        assert np.isfinite(getattr(ost, f)).all(), f
    # the proposals were not all rejected: the accept decision is part of what is compared
    assert _changed(ost.z, z0)[one_hot].any() and _changed(ost.z, z0)[rest].any()


# what delta = z - loc holds in one coordinate of a rejected step
VALUES = {"inf": np.inf, "nan": np.nan, "1e38": 1e38, "-0": -0.0}
BLOCK_EDGES = [15, 16, 31, 32, 47, 48]
COLUMNS = BLOCK_EDGES + [0, 62, 63]
# chain 1 + 4 p + v: value v in column COLUMNS[p] alone; the last four chains: value v at all six block edges
C_MASK = 1 + 4 * len(COLUMNS) + 4


def _mask_chain(p, v):
    return 1 + 4 * p + v


def _sweep1_delta(z, loc, scale, pe):
    pe[1:] = np.float32(-1e30)  # exp(pe - pe') = 0: the proposal is rejected, delta = z - loc
    for v, val in enumerate(VALUES.values()):
        for p, j in enumerate(COLUMNS):
            z[_mask_chain(p, v), j], loc[_mask_chain(p, v), j] = np.float32(val), np.float32(0.0)
        c = _mask_chain(len(COLUMNS), v)
        z[c, BLOCK_EDGES], loc[c, BLOCK_EDGES] = np.float32(val), np.float32(0.0)


def test_sweep1_blocks_and_masks(gpu, orc):
    """A rejected step whose delta holds inf, NaN, 1e38 or -0 in one column (the
    block edges, 0, 62, 63) or at all six block edges, and the step after it:
    sweep 1 carries w_j to the lanes above column j and to no other, so the
    non-finite values sit where the oracle has them and nowhere else."""
    C = C_MASK
    k, st, om, ost = _start_distinct(C, orc)
    for t in range(3):  # i = 0, 1, 2: the third is the n = 1 step after the warm-up
        k.sample_(st, 1)
        orc.step(om, ost, 1, num_warmup=W)
        torch.cuda.synchronize()
        assert_state_bitequal(st, ost, f"launch {t + 1}")
    assert int(ost.i[0]) == W + 1
    _edit(st, _sweep1_delta)
    _edit(ost, _sweep1_delta)
    delta = ost.z - ost.loc
    names = list(VALUES)
    for p, j in enumerate(COLUMNS):
        assert np.isposinf(delta[_mask_chain(p, names.index("inf")), j])
        assert np.isnan(delta[_mask_chain(p, names.index("nan")), j])
        assert delta[_mask_chain(p, names.index("1e38")), j] == np.float32(1e38)
        m0 = delta[_mask_chain(p, names.index("-0")), j]
        assert m0 == 0.0 and np.signbit(m0)
    edited = np.arange(1, C)
    bad = np.array([_mask_chain(p, v) for p in range(len(COLUMNS) + 1) for v in (0, 1)])  # inf, NaN
    zero = np.array([_mask_chain(p, names.index("-0")) for p in range(len(COLUMNS) + 1)])
    for t in range(2):  # n = 2, 3: both update where delta allows it
        before = copy.deepcopy(ost)
        k.sample_(st, 1)
        orc.step(om, ost, 1, num_warmup=W)
        torch.cuda.synchronize()
        assert_state_bitequal_nan(st, ost, f"sweep 1 masks, launch {t + 1}")
        changed = _changed(ost.scale, before.scale)
        if t == 0:  # the scenario is what it claims: rejected; inf and NaN keep the factor; -0 and chain 0 update, finite
            same = ost.z[edited].view(np.uint32) == before.z[edited].view(np.uint32)
            assert (same | np.isnan(ost.z[edited])).all()
        assert not changed[bad].any() and np.isfinite(ost.scale[bad]).all()
        assert changed[zero].all() and changed[0]
        for f in ("z", "loc", "scale", "as_change"):
            assert np.isfinite(getattr(ost, f)[zero]).all() and np.isfinite(getattr(ost, f)[0]).all(), f
    # a non-finite delta_j stays in coordinate j of loc: the other coordinates never saw it
    for p, j in enumerate(COLUMNS):
        for v in (0, 1):
            c = _mask_chain(p, v)
            assert np.flatnonzero(~np.isfinite(ost.loc[c])).tolist() == [j]
    k.sample_(st, FUSED)
    orc.step(om, ost, FUSED, num_warmup=W)
    torch.cuda.synchronize()
    assert_state_bitequal_nan(st, ost, "sweep 1 masks, fused launch")
