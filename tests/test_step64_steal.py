"""The stealable block tails of the single-step d = 64 launch
(csrc/amh_s64_sched.h), read through the host-only entry
amh_step64_steal_schedule: no GPU.

A block's draw order is that of amh_step64_schedule, split in two: the first
n - T draws (the own part) come from the block's LDS counter, the last T =
min(n, steal) from the block's head word in device memory, where other blocks
may draw too.  A wrong split loses a chain or runs it twice, so the own part
and the tail must partition 0 ... n - 1 in the unsplit order.  A tail chain has
class "tail" whenever the tail fits into the tail class (T <= floor(3 n / 8)),
and the class bits of the unsplit schedule otherwise.  The victims a block
visits once its own head is exhausted lie inside the grid, are at most
AMH_S64_STEAL_TRIES, and never name the block itself."""
import ctypes

import numpy as np
import pytest

from test_step64_schedule import TAIL, _library, hot_count

NS = [1, 2, 3, 15, 16, 17, 256]
TRIES = 4  # include/amh.h AMH_S64_STEAL_TRIES
STEAL_MAX = 1 << 15

I32P = ctypes.POINTER(ctypes.c_int32)


def _p(a):
    return a.ctypes.data_as(I32P)


def _steal_schedule(L, n, desc, steal, block=0, grid=1):
    idx, cls = np.full(n + 1, -7, np.int32), np.full(n + 1, -7, np.int32)  # one guard entry past the end
    vic = np.full(TRIES + 1, -7, np.int32)
    n_own, n_vic = ctypes.c_int32(-7), ctypes.c_int32(-7)
    rc = L.amh_step64_steal_schedule(n, desc, steal, block, grid, ctypes.byref(n_own), _p(idx), _p(cls), _p(vic),
                                     ctypes.byref(n_vic))
    assert rc == 0, (n, desc, steal, block, grid)
    assert idx[n] == -7 and cls[n] == -7 and 0 <= n_vic.value <= TRIES and vic[n_vic.value] == -7
    return n_own.value, idx[:n].copy(), cls[:n].copy(), vic[:n_vic.value].copy()


def _schedule(L, n, desc):
    idx, cls = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    assert L.amh_step64_schedule(n, desc, _p(idx), _p(cls)) == 0
    return idx[:n], cls[:n]


@pytest.mark.parametrize("n", NS)
def test_own_part_and_tail_partition_the_draw_order(n):
    L = _library()
    for desc in (0, 1):
        ref_idx, ref_cls = _schedule(L, n, desc)
        for steal in (0, 1, 16, n, n + 5):
            T = min(n, steal)
            n_own, idx, cls, _ = _steal_schedule(L, n, desc, steal)
            what = (n, desc, steal)
            assert n_own == n - T, what
            # own part, then tail: the unsplit order, so a partition of 0 ... n - 1
            assert np.array_equal(idx, ref_idx), what
            assert np.array_equal(np.sort(np.concatenate([idx[:n_own], idx[n_own:]])), np.arange(n)), what
            assert set(idx[:n_own].tolist()).isdisjoint(idx[n_own:].tolist()), what
            # classes: those of the unsplit schedule; a tail that fits the tail class is all "tail"
            assert np.array_equal(cls, ref_cls), what
            if T <= hot_count(n):
                assert np.all(cls[n_own:] == TAIL), what


def test_tail_length_is_capped():
    """The head word's count has 16 bits: the tail never exceeds 2^15 chains."""
    L = _library()
    n = STEAL_MAX + 100
    for desc in (0, 1):
        n_own, idx, _, _ = _steal_schedule(L, n, desc, 65535)
        assert n_own == 100
        assert np.array_equal(idx, np.arange(n)[::-1] if desc else np.arange(n))


def test_default_tail_lies_in_the_tail_class():
    """At the headline shape (256 chains per block) the default tail is all class "tail"."""
    L = _library()
    for desc in (0, 1):
        n_own, _, cls, _ = _steal_schedule(L, 256, desc, 16)
        assert n_own == 240 and np.all(cls[n_own:] == TAIL)


@pytest.mark.parametrize("grid", [1, 2, 3, 7, 8, 9, 16, 17, 24, 32, 33, 256, 257, 1024])
def test_victims(grid):
    L = _library()
    for block in range(grid):
        _, _, _, vic = _steal_schedule(L, 1, 0, 1, block, grid)
        assert np.all((0 <= vic) & (vic < grid)), (block, grid)
        assert block not in vic.tolist(), (block, grid)
        assert len(set(vic.tolist())) == len(vic), (block, grid)
        # b + 8, b + 16, ... mod the grid, until the sequence would come back to b
        want = []
        for k in range(1, TRIES + 1):
            v = (block + 8 * k) % grid
            if v == block:
                break
            want.append(v)
        assert vic.tolist() == want, (block, grid)
    if grid == 256:
        assert len(vic) == TRIES and all(v % 8 == block % 8 for v in vic)


def test_bad_arguments_are_refused():
    L = _library()
    one = ctypes.c_int32(0)
    buf = np.zeros(8, np.int32)
    ok = (ctypes.byref(one), _p(buf), _p(buf), _p(buf), ctypes.byref(one))
    assert L.amh_step64_steal_schedule(1, 0, 1, 0, 1, *ok) == 0
    assert L.amh_step64_steal_schedule(-1, 0, 1, 0, 1, *ok) == -1
    assert L.amh_step64_steal_schedule(1, 0, -1, 0, 1, *ok) == -1
    assert L.amh_step64_steal_schedule(1, 0, 1, 1, 1, *ok) == -1  # block outside the grid
    assert L.amh_step64_steal_schedule(1, 0, 1, 0, 0, *ok) == -1
    assert L.amh_step64_steal_schedule(1, 0, 1, 0, 1, None, _p(buf), _p(buf), _p(buf), ctypes.byref(one)) == -1
    assert b"amh_step64_steal_schedule" in L.amh_last_error(None)
    assert L.amh_step64_set_steal(None, 0) == -1
    assert L.amh_step64_stolen(None, None, None) == -1
