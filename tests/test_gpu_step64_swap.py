"""The d = 64 step kernel's in-place swap written as group statements
(arwmh_step64_kernel, ARWMH and ASSS: s64_group_read / s64_group_write /
s64_group_norm, one exec shift per masked operation and one restore per
statement).

Column j of the incoming factor is read on lanes r > j, column j of the
outgoing L' is written on lanes r >= j at the same addresses, and U_rj is
normalised on lanes r > j.  A wrong mask or offset in one column shows up as
wrong words of `scale` at or above that column's diagonal and, from the next
launch on, as a broken unit pattern of U.  A factor whose 2,080 packed entries
all differ (the initial one is a multiple of the identity) makes every such
word visible from the first launch.  Every comparison is bit for bit against
the C oracle on whole states.

num_warmup = 2: launches 1 and 3 keep L (gamma = 1: the columns are only read
and normalised, the factor is copied verbatim), launches 2 and 4 update it
(reads, L' writes and normalisation).  C = 12,325 = 256 * 48 + 37 gives every
wave 3-4 items with ragged block ranges."""
import copy

import numpy as np
import pytest
import torch

from helpers import _leaf, assert_state_bitequal
from test_gpu_step64_order import C_RAGGED, _clone, _order, _start

pytestmark = pytest.mark.gpu

W = 2
D = 64
P = D * (D + 1) // 2


def _col(j):
    """offset of column j (rows j .. 63) in the packed factor"""
    return j * D - j * (j - 1) // 2


DIAG = np.array([_col(j) for j in range(D)])


def _distinct_factor(C, seed=7):
    """[C, 2080] packed lower factors, positive diagonal: per chain the 64
    diagonals are a permutation of 64 values in [0.5, 1.5], the 2,016 strictly
    lower entries a signed permutation of 2,016 values in [1e-3, 2e-3)."""
    rng = np.random.default_rng(seed + C)
    L = np.empty((C, P), np.float32)
    lower = np.setdiff1d(np.arange(P), DIAG)
    pool = (1e-3 * (1.0 + np.arange(lower.size) / lower.size)).astype(np.float32)
    sign = np.where(np.arange(lower.size) % 2 == 0, 1.0, -1.0).astype(np.float32)
    L[:, lower] = rng.permuted(np.broadcast_to(pool * sign, (C, lower.size)), axis=1)
    dpool = (0.5 + np.arange(D) / (D - 1.0)).astype(np.float32)
    L[:, DIAG] = rng.permuted(np.broadcast_to(dpool, (C, D)), axis=1)
    assert all(np.unique(np.abs(row)).size == P for row in L[:: max(1, C // 7)])
    return L


def _set_scale(state, L):
    scale = _leaf(state, "scale")
    if torch.is_tensor(scale):
        scale.copy_(torch.from_numpy(L))
    else:
        scale[...] = L


def _start_distinct(C, orc, cls="ARWMH"):
    k, st, om, ost = _start(C, orc, W, cls=cls)
    L = _distinct_factor(C)
    _set_scale(st, L)
    _set_scale(ost, L)
    torch.cuda.synchronize()
    return k, st, om, ost


def test_distinct_entries_arwmh(gpu, orc):
    """Four in-place launches from a factor of 2,080 different entries, the
    state checked after every one."""
    k, st, om, ost = _start_distinct(C_RAGGED, orc)
    for t in range(4):
        k.sample_(st, 1)
        assert _order(k) == t % 2
        orc.step(om, ost, 1, num_warmup=W)
        torch.cuda.synchronize()
        assert_state_bitequal(st, ost, f"distinct entries, launch {t + 1}")


def test_distinct_entries_asss(gpu, orc):
    """The ASSS instantiation: two launches against orc.asss_step."""
    from test_gpu_asss import assert_bitequal
    k, st, om, ost = _start_distinct(C_RAGGED, orc, cls="ASSS")
    for t in range(2):
        k.sample_(st, 1)
        orc.asss_step(om, ost, 1, num_warmup=W)
        torch.cuda.synchronize()
        assert_bitequal(st, ost, f"ASSS distinct entries, launch {t + 1}")


@pytest.fixture(scope="module")
def three_steps_in(gpu, orc):
    """One kernel object and the product and oracle states after three fused
    steps (computed once; every case works on copies)."""
    k, st, om, ost = _start(C_RAGGED, orc, W)
    k.sample_(st, 3)
    orc.step(om, ost, 3, num_warmup=W)
    torch.cuda.synchronize()
    assert_state_bitequal(st, ost, "three fused steps in")
    return k, st, om, ost


def _zero_pivot(state, j, every=5):
    """L_jj = 0 for every fifth chain (test_gpu_step64_handover._zero_first_pivot
    for any column): sqrt(1 - gamma) L_jj = 0 fails the update's pivot test, so
    the update is reverted in every later step and the factor is kept, with
    every value finite on both sides."""
    scale = _leaf(state, "scale")
    if torch.is_tensor(scale):
        a = scale.detach().cpu().numpy().copy()
        a[::every, _col(j)] = 0.0
        scale.copy_(torch.from_numpy(a))
    else:
        scale[::every, _col(j)] = 0.0


@pytest.mark.parametrize("j", [1, 3, 4, 31, 32, 59, 60, 62, 63])
def test_kept_factor_at_group_boundaries(j, three_steps_in, orc):
    """Every fifth chain's update reverted by a zero pivot in the first, the
    last or a middle column of a swap group: 1 / l_j = 0 on the incoming side,
    a zero column of L' on the outgoing one, kept and updated factors
    alternating between consecutive items of a wave."""
    k, st0, om, ost0 = three_steps_in
    st, ost = _clone(st0), copy.deepcopy(ost0)
    _zero_pivot(st, j)
    _zero_pivot(ost, j)
    before = ost.scale.copy()
    for t in range(3):
        k.sample_(st, 1)
        orc.step(om, ost, 1, num_warmup=W)
        torch.cuda.synchronize()
        assert_state_bitequal(st, ost, f"L_{j},{j} = 0, launch {t + 1}")
    # the scenario is what it claims: those factors were kept, the others changed
    changed = (ost.scale.view(np.uint32) != before.view(np.uint32)).any(axis=1)
    assert not changed[::5].any()
    assert changed[np.arange(C_RAGGED) % 5 != 0].all()


@pytest.mark.parametrize("C", [1, 17, 4097, 8193])
def test_item_count_edges(C, gpu, orc):
    """No next item; a second item for one wave only; a third item for exactly
    one wave.  Two launches from the distinct-entries state: the first keeps L,
    the second updates it."""
    k, st, om, ost = _start_distinct(C, orc)
    for t in range(2):
        k.sample_(st, 1)
        orc.step(om, ost, 1, num_warmup=W)
        torch.cuda.synchronize()
        assert_state_bitequal(st, ost, f"C={C} launch {t + 1}")
