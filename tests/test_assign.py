"""The linear-assignment bit spec without a GPU: its numpy mirror
(tests/assign_np.py) against scipy's Hungarian algorithm on the same float32
costs, and the argument checks of wasserstein_dist11_p that come before any
device work."""
import numpy as np
import pytest

import assign_cases as AC
import assign_np


@pytest.mark.parametrize("name", AC.CLOUD_CPU + AC.SPECIAL)
@pytest.mark.parametrize("theta", [2, assign_np.DEFAULT_THETA])
def test_mirror_within_two_quanta_of_hungarian(name, theta):
    r = AC.mirror(name, theta)
    assert r["converged"]
    qmax = int(assign_np.quantise(AC.cost(name))[0].max())
    quantum = 2.0 ** r["e"] if qmax else 0.0
    got = AC.check_bound(name, r["perm"], quantum)
    if name in ("self", "self_perm", "zeros"):
        assert got == 0.0


def test_quantum():
    """e is the smallest integer with cmax 2^-e <= 2^30; the scaling is exact."""
    for cmax, e in [(1.0, -30), (1.5, -29), (2.0, -29), (2.0 ** 30, 0), (2.0 ** 30 + 128, 1), (3e38, 98), (1e-40, -162)]:
        q, got = assign_np.quantise(np.array([[cmax]], np.float32))
        assert got == e, cmax
        assert 2 ** 29 < q[0, 0] <= 2 ** 30
    assert assign_np.quantise(np.zeros((2, 2), np.float32))[1] == 0
    for bad in (np.nan, np.inf, -1.0):
        with pytest.raises(ValueError):
            assign_np.quantise(np.array([[bad]], np.float32))


def test_round_cap():
    r = assign_np.solve(AC.cost(257), max_rounds=3)
    assert not r["converged"] and r["rounds"] == 3 and r["phases"] == 1


def test_theta_default_matches_package():
    from utils_amd import evaluation as E
    assert E.ASSIGN_THETA == assign_np.DEFAULT_THETA


def test_method_checks_need_no_device():
    from utils_amd import evaluation as E
    assert "linear_assignment" in E.__all__
    x = np.zeros((5, 2), np.float32)
    with pytest.raises(ValueError, match="method"):
        E.wasserstein_dist11_p(x, x, method="bogus")
    with pytest.raises(ValueError, match="equally many"):
        E.wasserstein_dist11_p(x, np.zeros((6, 2), np.float32), method="auction")
