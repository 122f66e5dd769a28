"""Inputs shared by tests/test_assign.py and tests/test_gpu_assign.py: float32
cost matrices, and the mirror's and scipy's answers computed once each."""
import functools

import numpy as np

import assign_np

CLOUD_CPU = (1, 2, 3, 63, 64, 65, 257)
# 255 / 256 / 257 straddle a workgroup; 1030 gives several elements per lane and a ragged 16-byte tail
CLOUD_GPU = CLOUD_CPU + (255, 256, 1030)
SPECIAL = ("grid", "self", "self_perm", "zeros", "outlier")


def _dist(x, y):
    from scipy.spatial import distance_matrix
    return np.ascontiguousarray(distance_matrix(x, y).astype(np.float32))


@functools.lru_cache(maxsize=None)
def cost(name):
    """The float32 cost matrix of case `name` (an int: normal clouds, d = 5)."""
    if isinstance(name, int):
        rng = np.random.default_rng(1000 + name)
        x = rng.normal(size=(name, 5)).astype(np.float32)
        y = (rng.normal(size=(name, 5)) + 0.7).astype(np.float32)
        return _dist(x, y)
    rng = np.random.default_rng(7)
    if name == "grid":  # 200 points on a 3 x 3 integer grid: massive ties
        return _dist(rng.integers(0, 3, size=(200, 2)).astype(np.float32),
                     rng.integers(0, 3, size=(200, 2)).astype(np.float32))
    if name == "self":
        x = rng.normal(size=(130, 4)).astype(np.float32)
        return _dist(x, x.copy())
    if name == "self_perm":
        x = rng.normal(size=(130, 4)).astype(np.float32)
        return _dist(x, x[rng.permutation(130)])
    if name == "zeros":
        return np.zeros((70, 70), np.float32)
    if name == "outlier":  # one point scaled by 10^6
        x = rng.normal(size=(100, 3)).astype(np.float32)
        y = rng.normal(size=(100, 3)).astype(np.float32)
        y[7] *= 1e6
        return _dist(x, y)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def mirror(name, theta):
    return assign_np.solve(cost(name), theta=theta)


@functools.lru_cache(maxsize=None)
def hungarian_mean(name):
    from scipy.optimize import linear_sum_assignment
    c = cost(name).astype(np.float64)
    r, k = linear_sum_assignment(c)
    return float(c[r, k].mean())


def check_bound(name, perm, quantum):
    """perm is a permutation with -s <= mean c(perm) - mean c(Hungarian) <= 2 quantum + s,
    s = n 2^-52 cmax (float64 summation slack)."""
    c = cost(name).astype(np.float64)
    n = c.shape[0]
    perm = np.asarray(perm)
    assert sorted(perm.tolist()) == list(range(n))
    got = float(c[np.arange(n), perm].mean())
    s = n * 2.0 ** -52 * float(c.max())
    diff = got - hungarian_mean(name)
    print(f"{name}: n = {n} mean - optimum = {diff:.3e}, 2 quantum = {2 * quantum:.3e}, s = {s:.3e}")
    assert -s <= diff <= 2 * quantum + s
    return got
