"""The d = 64 step kernel's block-local schedule (csrc/amh_s64_sched.h), read
through the host-only entry amh_step64_schedule: no GPU.

For a block of n chains and a direction the schedule is the sequence of
(local index, class) the block's counter hands out.  Class bit 0 is "hot" (the
chain is among the first draws of a launch chained to an oppositely ordered
one: that launch drew it last), bit 1 "tail" (among the last draws: the next
launch draws it first).  Both parts hold h = floor(3 n / 8) chains -- rounded
down, so h = 0 for n < 3 (every chain "mid") and h <= n / 2 always: no chain is
both.  The kernel picks the cache policy of a chain's factor traffic by the
class, so a wrong class only costs speed -- silently, which is why it is pinned
here; a wrong index would lose or repeat a chain."""
import ctypes
import os

import numpy as np
import pytest

N_MAX = 600
HOT, TAIL = 1, 2


def _library():
    from kernels_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def schedules():
    """{(n, descending): (index[n], cls[n])} for n = 0 ... N_MAX, computed once."""
    L = _library()
    out = {}
    for n in range(N_MAX + 1):
        for desc in (0, 1):
            idx = np.full(n + 1, -7, np.int32)  # one guard entry past the end
            cls = np.full(n + 1, -7, np.int32)
            rc = L.amh_step64_schedule(n, desc, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                       cls.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
            assert rc == 0, (n, desc)
            assert idx[n] == -7 and cls[n] == -7, (n, desc)  # n entries written, no more
            out[n, desc] = (idx[:n].copy(), cls[:n].copy())
    return out


def hot_count(n):
    return 3 * n // 8


def test_sequence_is_a_permutation(schedules):
    for (n, desc), (idx, _) in schedules.items():
        assert np.array_equal(np.sort(idx), np.arange(n)), (n, desc)


def test_direction(schedules):
    """Ascending draws 0, 1, 2, ...; descending draws n - 1, n - 2, ..."""
    for n in range(N_MAX + 1):
        assert np.array_equal(schedules[n, 0][0], np.arange(n)), n
        assert np.array_equal(schedules[n, 1][0], np.arange(n)[::-1]), n


def test_hot_and_tail_sizes(schedules):
    sizes = set()
    for (n, desc), (idx, cls) in schedules.items():
        h = hot_count(n)
        sizes.add(h)
        assert set(np.unique(cls)) <= {0, HOT, TAIL}, (n, desc)  # never both, nothing else
        assert int(np.sum(cls == HOT)) == h, (n, desc)
        assert int(np.sum(cls == TAIL)) == h, (n, desc)
        # hot chains are the first h draws, the tail the last h
        assert np.all(cls[:h] == HOT) and np.all(cls[n - h:] == TAIL), (n, desc)
    assert 0 in sizes and 1 in sizes and 3 * N_MAX // 8 in sizes  # the edges were exercised
    assert hot_count(2) == 0 and hot_count(3) == 1  # 0 allowed at the small end, first 1 at n = 3


def test_hot_set_is_what_the_other_direction_visits_last(schedules):
    for n in range(N_MAX + 1):
        h = hot_count(n)
        for desc in (0, 1):
            idx, cls = schedules[n, desc]
            other_idx, other_cls = schedules[n, 1 - desc]
            hot = set(idx[cls == HOT].tolist())
            last = set(other_idx[n - h:].tolist())
            assert hot == last, (n, desc)
            # ... and that is the other direction's tail
            assert hot == set(other_idx[other_cls == TAIL].tolist()), (n, desc)


def test_bad_arguments_are_refused():
    L = _library()
    assert L.amh_step64_schedule(-1, 0, None, None) == -1
    assert L.amh_step64_schedule(3, 0, None, None) == -1
    assert b"amh_step64_schedule" in L.amh_last_error(None)
    assert L.amh_step64_schedule(0, 0, None, None) == 0
