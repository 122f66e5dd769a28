"""Input sets for the elementwise checks of include/amh_math.h
(tests/test_rng_math.py: the host compile against float64; tests/test_gpu_math.py:
the device compile against the host compile).  Seeded, deterministic, built once
per process and returned read-only.

Exclusions, each with its reason:
  * amh_sincosf is compared only on finite |x| <= 2^30: beyond that the header's
    `(int)kf` is out of int range (undefined in C, so the two compiles may
    differ) and its callers stay below 2 pi.
  * amh_erfinvf only on (-1, 1), its domain (amh_normal_from_bits clamps to it).
  * amh_rsqrt_nr only where amh_pivot_ok holds: its callers accept no other pivot.
  * NaN payloads are not part of the spec: a NaN must meet a NaN, nothing more.
"""
import functools

import numpy as np

NBHD = 64  # neighbourhoods reach this many ulp to either side
FLT_MAX = np.float32(3.4028234663852886e38)
STUDENT3_C = float(np.float32(-3.30347394261755545))
# lp_student3's (loc, scale, c) in the diamonds models: the intercept's prior, sigma's prior
STUDENT3_TRIPLES = ((8.0, 10.0, STUDENT3_C), (0.0, 10.0, STUDENT3_C))
LR_DECAYS = (float(np.float32(2 / 3)), 0.5, float(np.float32(0.51)), float(np.float32(0.99)), 1.0)
POISSON_Y = (0.0, 1.0, 7.0, 1000.0)
LOGISTIC_Y = (0.0, 1.0)


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def bits32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _ordered(x):
    """float32 -> int64 that counts representable values through zero."""
    b = bits32(x).astype(np.int64)
    return np.where(b < 0x80000000, b, -(b & 0x7FFFFFFF))


def _unordered(i):
    i = np.asarray(i, np.int64)
    return f32(np.where(i >= 0, i, (-i) | 0x80000000).astype(np.uint32))


def around(centres, k=NBHD):
    """Every float32 within k ulp of each centre (the centres are rounded to
    float32 first), stopping at +-inf; sorted ascending, no duplicates."""
    c = _ordered(np.atleast_1d(np.asarray(centres, np.float64)).astype(np.float32))
    i = (c[:, None] + np.arange(-k, k + 1, dtype=np.int64)[None, :]).ravel()
    i = np.unique(np.clip(i, -0x7F800000, 0x7F800000))
    return _unordered(i)


SPECIALS = (0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001)
_EDGE_MANTISSAS = (0, 1, 2, 0x3FFFFF, 0x400000, 0x400001, 0x7FFFFE, 0x7FFFFF)
LATTICE_RANDOM = 1024
LATTICE_SIZE = 255 * 2 * (len(_EDGE_MANTISSAS) + LATTICE_RANDOM) + len(SPECIALS)


@functools.lru_cache(maxsize=None)
def lattice32():
    """Both signs x biased exponents 0..254 (the subnormal band is exponent 0) x
    (8 edge mantissas + 1024 random ones), then +-0, +-inf and three NaNs."""
    rng = np.random.default_rng(20240532)
    man = np.empty((2, 255, len(_EDGE_MANTISSAS) + LATTICE_RANDOM), np.uint32)
    man[:, :, :len(_EDGE_MANTISSAS)] = np.array(_EDGE_MANTISSAS, np.uint32)
    man[:, :, len(_EDGE_MANTISSAS):] = rng.integers(0, 1 << 23, size=(2, 255, LATTICE_RANDOM), dtype=np.uint32)
    sign = (np.arange(2, dtype=np.uint32) << 31)[:, None, None]
    expo = (np.arange(255, dtype=np.uint32) << 23)[None, :, None]
    b = np.concatenate([(sign | expo | man).ravel(), np.array(SPECIALS, np.uint32)])
    assert b.size == LATTICE_SIZE
    return _frozen(f32(b))


def _cat(*parts):
    return _frozen(np.concatenate([np.asarray(p, np.float32).ravel() for p in parts]))


# ------------------------------------------------------ per-function sets --
@functools.lru_cache(maxsize=None)
def logf_cases():
    # the subnormal switch, m = sqrt(1/2) (mantissa 0x3504F3) at ten exponents, 1.0
    half_sqrt = f32((np.array([1, 2, 25, 64, 101, 126, 127, 128, 200, 254], np.uint32) << 23) | 0x3504F3)
    return _cat(lattice32(), around([1.17549435e-38, 1.0]), around(half_sqrt))


def expf_subnormal_edge():
    """Sorted neighbourhood of the x below which amh_expf's result is subnormal."""
    return around([-87.3365])


@functools.lru_cache(maxsize=None)
def expf_cases():
    ties = (np.arange(-151, 129, dtype=np.float64) + 0.5) * np.log(2.0)  # rintf ties of x log2(e)
    return _cat(lattice32(), around([88.7228317, -103.972084, 0.0]), expf_subnormal_edge(), around(ties))


@functools.lru_cache(maxsize=None)
def log1pf_cases():
    # u = 1 + x rounds to 1 below 2^-24 (2^-25 on the negative side); the pole; the overflow of u
    e = [2.0 ** -24, -2.0 ** -24, 2.0 ** -25, -2.0 ** -25, -1.0, float(FLT_MAX)]
    return _cat(lattice32(), around(e))


LOG1P_SQ_SWITCH = np.float32(1.8e19)


def log1p_sq_edges():
    e = [1.8e19, -1.8e19, 1.8446743e19, -1.8446743e19]  # the switch, sqrt(FLT_MAX)
    return around(e)


@functools.lru_cache(maxsize=None)
def log1p_sq_cases():
    return _cat(lattice32(), log1p_sq_edges())


SINCOS_MAX = np.float32(2.0 ** 30)


def sincos_edges():
    return around(np.arange(-16, 17, dtype=np.float64) * (np.pi / 4))  # odd k: the rintf ties


@functools.lru_cache(maxsize=None)
def sincos_cases():
    x = lattice32()
    x = x[np.isfinite(x) & (np.abs(x) <= SINCOS_MAX)]
    return _cat(x, sincos_edges())


@functools.lru_cache(maxsize=None)
def erfinv_cases():
    x = lattice32()
    x = x[np.abs(x) < 1.0]  # drops the NaNs too
    u5 = np.sqrt(-np.expm1(-5.0))  # w = -log((1 - u)(1 + u)) crosses 5 here
    return _cat(x, around([u5, -u5]))


@functools.lru_cache(maxsize=None)
def pivot_cases():
    """The lattice members amh_pivot_ok accepts: normal, finite, positive."""
    x = lattice32()
    return _frozen(x[(x >= np.float32(1.17549435e-38)) & np.isfinite(x)])


NORMAL_BITS_SIZE = (1 << 23) + (1 << 16)


@functools.lru_cache(maxsize=None)
def normal_bits_cases():
    """Only b >> 9 enters: every m << 9, then 2^16 of them with the low nine bits set."""
    m = np.arange(1 << 23, dtype=np.uint32) << 9
    pick = np.random.default_rng(9).choice(1 << 23, size=1 << 16, replace=False).astype(np.uint32)
    return _frozen(np.concatenate([m, (pick << 9) | 0x1FF]))


@functools.lru_cache(maxsize=None)
def eta_cases():
    return _cat(lattice32(), np.linspace(-120.0, 120.0, (1 << 16) + 1).astype(np.float32))


def with_y(eta, ys):
    """(eta, y) pairs: every eta with every y."""
    e = np.tile(eta, len(ys))
    y = np.repeat(np.asarray(ys, np.float32), eta.size)
    return _frozen(e), _frozen(y)


@functools.lru_cache(maxsize=None)
def gamma_n_cases():
    rng = np.random.default_rng(31)
    return _frozen(np.concatenate([
        np.arange(1, (1 << 21) + 1, dtype=np.int32),
        rng.integers(1, (1 << 31) - 1, size=4096, dtype=np.int64).astype(np.int32),
        np.array([(1 << 31) - 1], np.int32)]))


GAMMA_N_SIZE = (1 << 21) + 4096 + 1


def log_d_cases():
    return _frozen(gamma_n_cases().astype(np.float64))


def exp_d_cases(log_d_of_n):
    """a log_d(n), formed as amh_lr_gamma forms it, for every decay rate, then
    2^20 uniform points of (-700, 700)."""
    parts = [np.float64(np.float32(a)) * log_d_of_n for a in LR_DECAYS]
    parts.append(np.random.default_rng(32).uniform(-700.0, 700.0, 1 << 20))
    return _frozen(np.concatenate(parts))


EXP_D_SIZE = len(LR_DECAYS) * GAMMA_N_SIZE + (1 << 20)
