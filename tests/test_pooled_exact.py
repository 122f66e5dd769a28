"""The fixed-point format of the pooled mode's exact sums (include/amh.h
"exact sums", csrc/amh_exact.h) through its two host entries, which compile
the functions the kernels use, against Python integers and fractions; and
distributed.shard_range(align=).  No GPU."""
import ctypes
import itertools
import math
from fractions import Fraction

import numpy as np
import pytest

BITS, LIMBS, FRAC, WORDS = 40, 4, 80, 5  # AMH_EXACT_* of include/amh.h


@pytest.fixture(scope="module")
def L():
    import os
    from kernels_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def quantise(L, rows, acc=None):
    """amh_pooled_exact_quantise of float32 rows [n][V]; acc: added to a copy of it."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n, V = rows.shape
    out = np.zeros((V, WORDS), dtype=np.int64) if acc is None else acc.copy()
    rc = L.amh_pooled_exact_quantise(rows.ctypes.data_as(ctypes.c_void_p), n, V, out.ctypes.data_as(ctypes.c_void_p),
                                     0 if acc is None else 1)
    assert rc == 0
    return out


def to_double(L, acc):
    acc = np.ascontiguousarray(acc, dtype=np.int64)
    out = np.empty(acc.shape[0], dtype=np.float64)
    assert L.amh_pooled_exact_to_double(acc.ctypes.data_as(ctypes.c_void_p), acc.shape[0],
                                        out.ctypes.data_as(ctypes.c_void_p)) == 0
    return out


def limb_value(words) -> int:
    """The integer sum_j limb_j 2^(BITS j) of one component (in units of 2^-FRAC)."""
    return sum(int(words[j]) << (BITS * j) for j in range(LIMBS))


def image(p) -> int:
    """trunc(p 2^FRAC) of a finite float32 inside the range."""
    return int(Fraction(float(p)) * (1 << FRAC))  # int() cuts toward zero


def ulp_distance(x: float, exact: Fraction) -> Fraction:
    """|x - exact| in units of the spacing of doubles at `exact`."""
    if exact == 0:
        return Fraction(0) if x == 0.0 else Fraction(10)
    return abs(Fraction(x) - exact) / Fraction(math.ulp(float(exact)))


def random_partials(rng, n, V, lo_exp, hi_exp):
    """float32 values m 2^e with a random 24-bit m, e spread over [lo_exp,
    hi_exp), mixed signs, and zeros (of both signs) and denormals mixed in."""
    m = rng.integers(1 << 23, 1 << 24, size=(n, V)).astype(np.float64)
    e = rng.integers(lo_exp, hi_exp, size=(n, V))
    x = np.ldexp(m, e - 23) * rng.choice([-1.0, 1.0], size=(n, V))
    x = x.astype(np.float32)
    kind = rng.integers(0, 12, size=(n, V))
    x[kind == 0] = 0.0
    x[kind == 1] = -0.0
    den = (rng.integers(1, 1 << 23, size=(n, V)).astype(np.uint32)
           | (rng.integers(0, 2, size=(n, V)).astype(np.uint32) << 31)).view(np.float32)
    x[kind == 2] = den[kind == 2]
    assert np.isfinite(x).all() and (np.abs(x.astype(np.float64)) < 2.0 ** 80).all()
    return x


@pytest.fixture(scope="module")
def partials():
    # exponents from far below the grid (2^-80) up to the top of the range (2^80)
    return random_partials(np.random.default_rng(7), 37, 53, -110, 80)


def test_limbs_are_the_sum_of_the_truncated_partials(L, partials):
    acc = quantise(L, partials)
    assert (acc[:, LIMBS] == 0).all()
    for v in range(partials.shape[1]):
        assert limb_value(acc[v]) == sum(image(p) for p in partials[:, v]), v


def test_limb_totals_do_not_depend_on_the_partition(L, partials):
    whole = quantise(L, partials)
    n = partials.shape[0]
    rng = np.random.default_rng(8)
    for cuts in [(1,), (n // 2,), (n - 1,), (5, 6), (3, 20), (12, 30)]:
        blocks = np.split(partials, cuts)
        for order in itertools.permutations(range(len(blocks))):
            acc = None
            for b in order:
                acc = quantise(L, blocks[b], acc)
            assert np.array_equal(acc, whole), (cuts, order)
    for _ in range(3):
        assert np.array_equal(quantise(L, partials[rng.permutation(n)]), whole)


def test_to_double_is_within_one_ulp_of_the_exact_sum(L, partials):
    acc = quantise(L, partials)
    got = to_double(L, acc)
    for v in range(partials.shape[1]):
        exact = Fraction(sum(image(p) for p in partials[:, v]), 1 << FRAC)
        assert ulp_distance(got[v], exact) <= 1, (v, got[v], float(exact))
        assert got[v] == float(exact)  # in fact correctly rounded (int / int division rounds to nearest even)


def test_on_grid_inputs_sum_exactly(L):
    rng = np.random.default_rng(9)
    x = random_partials(rng, 29, 41, -57, 80)  # lowest set bit >= 2^(-57 - 23) = 2^-80
    x[np.abs(x) < 2.0 ** -57] = 0.0            # (the denormals are off the grid)
    acc = quantise(L, x)
    got = to_double(L, acc)
    for v in range(x.shape[1]):
        exact = sum(Fraction(float(p)) for p in x[:, v])
        assert Fraction(limb_value(acc[v]), 1 << FRAC) == exact
        assert got[v] == float(exact)
    # a narrow range, where the exact sum is itself a double
    y = (rng.integers(-(1 << 20), 1 << 20, size=(64, 17)) * 2.0 ** -12).astype(np.float32)
    assert np.array_equal(to_double(L, quantise(L, y)), y.astype(np.float64).sum(axis=0))


def test_to_double_rounds_ties_to_even_and_carries_signed_limbs(L):
    def words(value):  # un-normalised limbs of an integer: everything in limb 0 .. 3 by plain division
        w, sign, value = [0] * WORDS, -1 if value < 0 else 1, abs(value)
        for j in range(LIMBS):
            w[j] = sign * (value & ((1 << BITS) - 1))
            value >>= BITS
        assert value == 0
        return w
    cases = [(1 << 100) + (1 << 47), (1 << 100) + (1 << 47) + 1, (1 << 100) + 3 * (1 << 47), -((1 << 100) + (1 << 47)),
             1, -1, (1 << 159) - 1, -(1 << 159) + 12345, (1 << 53) + 1, (1 << 93) + (1 << 40), 0]
    acc = np.array([words(c) for c in cases], dtype=np.int64)
    # limbs of mixed sign and far above their payload (the headroom): same values
    acc2 = acc.copy()
    acc2[:, 1] += 1 << 60
    acc2[:, 2] -= 1 << 20
    acc2[:, 0] -= 5
    extra = (1 << 60 << BITS) - (1 << 20 << (2 * BITS)) - 5
    got, got2 = to_double(L, acc), to_double(L, acc2)
    for c, g, g2 in zip(cases, got, got2):
        assert g == Fraction(c, 1 << FRAC).__float__(), c
        assert g2 == float(Fraction(c + extra, 1 << FRAC)), c
    assert math.copysign(1.0, got[-1]) == 1.0  # an empty total is +0


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan, 2.0 ** 80, -3.0e38])
def test_partial_out_of_range_poisons_its_component_only(L, partials, bad):
    x = partials.copy()
    clean = to_double(L, quantise(L, x))
    x[11, 7] = bad
    n = x.shape[0]
    for cuts in [(), (11,), (12,), (4, 30)]:
        blocks = np.split(x, cuts)
        for order in itertools.permutations(range(len(blocks))):
            acc = None
            for b in order:
                acc = quantise(L, blocks[b], acc)
            got = to_double(L, acc)
            assert not np.isfinite(got[7]), (cuts, order)
            keep = np.arange(x.shape[1]) != 7
            assert np.array_equal(got[keep], clean[keep])
            assert np.array_equal(acc, quantise(L, x))
    # ... and stays non-finite when a partial of the other sign joins it
    y = np.array([[bad], [-bad]], dtype=np.float32)
    assert not np.isfinite(to_double(L, quantise(L, y))[0])


def test_sizes_and_chunk(L):
    from kernels_amd import pooled_chunk
    from kernels_amd.pooled import exact_size, sums_size
    for d in (1, 7, 32, 64, 128, 256):
        assert exact_size(d) == WORDS * sums_size(d)
    assert pooled_chunk(32, 16 * 9 + 5) == 16 and pooled_chunk(32, 8192) == 32 and pooled_chunk(32, 4096) == 16
    assert pooled_chunk(63, 10 ** 9) == 256
    assert pooled_chunk(64, 128 * 5 + 37) == 128 and pooled_chunk(128, 5) == 128 and pooled_chunk(256, 10 ** 6) == 128
    assert pooled_chunk(64, 3 * 4096) % 128 == 0 and pooled_chunk(64, 3 * 4096) % 48 == 0
    from kernels_amd._lib import AmhError
    with pytest.raises(AmhError):
        pooled_chunk(100, 64)


def _old_shard_range(num_chains, rank, world):
    base, extra = divmod(num_chains, world)
    return rank * base + min(rank, extra), base + (1 if rank < extra else 0)


def test_shard_range_align():
    from kernels_amd.distributed import shard_range
    for C, world in itertools.product([0, 1, 2, 7, 64, 100, 149, 677, 8192], [1, 2, 3, 8]):
        for r in range(world):
            assert shard_range(C, r, world) == _old_shard_range(C, r, world)
            assert shard_range(C, r, world, align=1) == _old_shard_range(C, r, world)
    for C, world, a in [(149, 2, 16), (149, 3, 16), (677, 2, 128), (677, 3, 128), (8192, 2, 32), (434, 2, 128),
                        (395, 2, 128), (128, 1, 128), (129, 2, 128), (1000, 8, 16), (256, 2, 128)]:
        shards = [shard_range(C, r, world, align=a) for r in range(world)]
        pos = 0
        for off, cnt in shards:
            assert off == pos and off % a == 0 and cnt > 0
            pos += cnt
        assert pos == C
        assert all(cnt % a == 0 for _, cnt in shards[:-1])  # the ragged tail is the last rank's
        n_chunks = -(-C // a)
        assert [-(-cnt // a) for _, cnt in shards] == [_old_shard_range(n_chunks, r, world)[1] for r in range(world)]
    for C, world, a in [(128, 2, 128), (300, 4, 128), (0, 1, 16), (16, 2, 16)]:
        with pytest.raises(ValueError):
            shard_range(C, world - 1, world, align=a)
    with pytest.raises(ValueError):
        shard_range(100, 0, 2, align=0)
