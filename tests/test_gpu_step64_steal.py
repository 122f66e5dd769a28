"""Stealable block tails of the single-step d = 64 launch (arwmh_step64_kernel,
its single-step ARWMH instance; csrc/amh_s64_sched.h).  The last T chains of a
block's draw order come from the block's head word in device memory, and a
block that has run out of work draws from other blocks' heads.  Which block
computes a chain changes no bit; a wrong split, a stale head word or a wrong
victim range loses a chain or runs it twice.  So every case compares whole
states bit for bit against the C oracle after each of six consecutive
single-step launches on one handle (both directions, chained launches, the
launch tag advancing, every block re-arming its head), and checks that every
chain's step counter advanced by exactly one per launch.

Shapes: C = 1, 17, 255, 257 and 4,097: blocks of 1, 16 and 17 chains (a wave
takes a second item) and ragged last blocks.  T = 0 (no tail), 1, the default
and 65,535 (every chain of every block is stealable, so a block that starts
early steals).  No case requires that a steal happens: the count of stolen
chains is only bounded.  The oracle's trajectory is computed once per C."""
import copy

import numpy as np
import pytest
import torch

from helpers import assert_state_bitequal
from test_gpu_step64_compute import W, _start_distinct

pytestmark = pytest.mark.gpu

LAUNCHES = 6
CS = [1, 17, 255, 257, 4097]
STEALS = [0, 1, None, 65535]  # None: the handle's default

_REF = {}


def _reference(C, orc):
    """The oracle's states after 0 ... LAUNCHES single steps from _start_distinct(C), computed once."""
    if C not in _REF:
        _, _, om, ost = _start_distinct(C, orc)
        snaps = [copy.deepcopy(ost)]
        for _ in range(LAUNCHES):
            orc.step(om, ost, 1, num_warmup=W)
            snaps.append(copy.deepcopy(ost))
        _REF[C] = snaps
    return _REF[C]


def _check(st, ref, C, t, what):
    torch.cuda.synchronize()
    assert_state_bitequal(st, ref[t], f"{what}, launch {t}")
    i = st.i.cpu().numpy()
    assert i.shape == (C,) and (i == int(ref[0].i[0]) + t).all(), f"{what}, launch {t}: a chain was dropped or run twice"


def _stolen_ok(k, C, steal):
    n = k._handle.stolen()
    assert (n == 0) if steal == 0 else (0 <= n <= C), (n, C, steal)


@pytest.mark.parametrize("steal", STEALS)
@pytest.mark.parametrize("C", CS)
def test_six_launches(C, steal, gpu, orc):
    ref = _reference(C, orc)
    k, st, _, _ = _start_distinct(C, orc)
    if steal is not None:
        k._handle.set_steal(steal)
    _check(st, ref, C, 0, f"C={C} T={steal}")
    for t in range(1, LAUNCHES + 1):
        k.sample_(st, 1)
        _check(st, ref, C, t, f"C={C} T={steal}")
        _stolen_ok(k, C, steal)
    assert np.isfinite(ref[-1].scale).all()
    # of the six launches, the first and the third keep the factor (gamma = 1), the others update it
    same = [np.array_equal(ref[t].scale.view(np.uint32), ref[t - 1].scale.view(np.uint32))
            for t in range(1, LAUNCHES + 1)]
    assert same == [True, False, True, False, False, False]


def test_two_handles_alternate_on_one_stream(gpu, orc):
    """Two handles, each with its own head words and tags, take turns on one state."""
    C = 257
    ref = _reference(C, orc)
    k_a, st, _, _ = _start_distinct(C, orc)
    k_b, _, _, _ = _start_distinct(C, orc)
    for k in (k_a, k_b):
        k._handle.set_steal(65535)
    for t in range(1, LAUNCHES + 1):
        k = (k_a, k_b)[t % 2]
        k.sample_(st, 1)
        _check(st, ref, C, t, "two handles")
        _stolen_ok(k, C, 65535)


def test_steal_changed_between_launches(gpu, orc):
    """A launch's tail length is its own: heads left by a launch with another T are exhausted."""
    C = 4097
    ref = _reference(C, orc)
    k, st, _, _ = _start_distinct(C, orc)
    for t, steal in enumerate([0, 65535, 1, 16, 0, 65535], start=1):
        k._handle.set_steal(steal)
        k.sample_(st, 1)
        _check(st, ref, C, t, f"T={steal}")
        _stolen_ok(k, C, steal)


def test_set_steal_range(gpu, orc):
    from kernels_amd._lib import AmhError
    k, _, _, _ = _start_distinct(1, orc)
    for bad in (-1, 65536):
        with pytest.raises(AmhError):
            k._handle.set_steal(bad)
    assert k._handle.stolen() == 0  # no launch yet


def test_fused_instance_unchanged(gpu, orc):
    """sample_(st, 5) runs the fused instance, which has no tail, between single-step launches that do."""
    C = 257
    k, st, om, ost = _start_distinct(C, orc)
    k._handle.set_steal(65535)
    for t, n in enumerate([1, 5, 1, 5]):
        k.sample_(st, n)
        orc.step(om, ost, n, num_warmup=W)
        torch.cuda.synchronize()
        assert_state_bitequal(st, ost, f"fused, launch {t + 1} ({n} steps)")
    assert (st.i.cpu().numpy() == int(ost.i[0])).all() and int(ost.i[0]) == 12


def test_asss_instance_unchanged(gpu, orc):
    from test_gpu_asss import assert_bitequal
    C = 257
    k, st, om, ost = _start_distinct(C, orc, cls="ASSS")
    k._handle.set_steal(65535)
    for t, n in enumerate([1, 1, 3]):
        k.sample_(st, n)
        orc.asss_step(om, ost, n, num_warmup=W)
        torch.cuda.synchronize()
        assert_bitequal(st, ost, f"ASSS launch {t + 1} ({n} steps)")
    assert k._handle.stolen() == 0
