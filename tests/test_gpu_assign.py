"""linear_assignment / wasserstein_dist11_p(method="auction") on the GPU
(csrc/amh_assign.hip): bit for bit against the numpy mirror of the spec
(tests/assign_np.py), within two quanta of scipy's Hungarian optimum, the
same from run to run, and refusing what the spec refuses."""
import numpy as np
import pytest
import torch

import assign_cases as AC
import assign_np

pytestmark = pytest.mark.gpu

CASES = AC.CLOUD_GPU + AC.SPECIAL


def _solve(gpu, name, theta=None, **kw):
    from utils_amd import evaluation as E
    return E.linear_assignment(torch.as_tensor(AC.cost(name)).to(gpu), theta=theta, **kw)


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("theta", [2, None])
def test_bit_equal_to_mirror_and_bound(name, theta, gpu):
    got = _solve(gpu, name, theta)
    ref = AC.mirror(name, assign_np.DEFAULT_THETA if theta is None else theta)
    assert got["converged"] and ref["converged"]
    assert (got["rounds"], got["phases"], got["e"]) == (ref["rounds"], ref["phases"], ref["e"])
    assert got["perm"].dtype == torch.int64 and got["perm"].is_cuda
    np.testing.assert_array_equal(got["perm"].cpu().numpy(), ref["perm"])
    np.testing.assert_array_equal(got["price"].cpu().numpy(), ref["price"])
    qmax = int(assign_np.quantise(AC.cost(name))[0].max())
    assert got["quantum"] == (2.0 ** ref["e"] if qmax else 0.0)
    # the 2 quantum bound against scipy, the quantum read from the result
    mean = AC.check_bound(name, got["perm"].cpu().numpy(), got["quantum"])
    n = AC.cost(name).shape[0]
    assert got["cost"] == pytest.approx(mean, rel=n * 2.0 ** -52, abs=0.0)
    if name in ("self", "self_perm", "zeros"):
        assert got["cost"] == 0.0


def test_unaligned_rows(gpu):
    """A cost matrix that starts 4 bytes past a 16-byte boundary: every row has a ragged head."""
    from utils_amd import evaluation as E
    c = AC.cost(65)
    buf = torch.zeros(65 * 65 + 1, dtype=torch.float32, device=gpu)
    view = buf[1:].view(65, 65)
    view.copy_(torch.as_tensor(c))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    got, ref = E.linear_assignment(view), AC.mirror(65, assign_np.DEFAULT_THETA)
    np.testing.assert_array_equal(got["perm"].cpu().numpy(), ref["perm"])
    np.testing.assert_array_equal(got["price"].cpu().numpy(), ref["price"])
    assert got["rounds"] == ref["rounds"]


def test_run_to_run_determinism(gpu):
    a, b = _solve(gpu, 1030), _solve(gpu, 1030)
    assert torch.equal(a["perm"], b["perm"]) and torch.equal(a["price"], b["price"])
    assert a["rounds"] == b["rounds"] and a["cost"] == b["cost"]


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -1.0])
def test_refuses_bad_costs(bad, gpu):
    from utils_amd import evaluation as E
    c = torch.as_tensor(AC.cost(65)).to(gpu).clone()
    c[64, 64] = bad
    with pytest.raises(ValueError):
        E.linear_assignment(c)


def test_refuses_bad_shapes_and_cpu_tensors(gpu):
    from kernels_amd import _lib
    from utils_amd import evaluation as E
    with pytest.raises(ValueError):
        E.linear_assignment(torch.zeros(3, 4, device=gpu))
    with pytest.raises(ValueError):
        E.linear_assignment(torch.zeros(3, device=gpu))
    with pytest.raises(_lib.AmhError):
        E.linear_assignment(torch.zeros(3, 3))
    # the C entries refuse n outside 1 .. 65536 and null pointers with a message
    L = _lib.lib()
    import ctypes
    nbytes = ctypes.c_int64()
    assert L.amh_assign_work_size(0, ctypes.byref(nbytes)) == -1
    assert L.amh_assign_work_size(65537, ctypes.byref(nbytes)) == -1
    assert L.amh_assign_begin(None, 4, None, None) == -1
    assert b"amh_assign_begin" in L.amh_last_error(None)


def test_round_cap(gpu, monkeypatch):
    """max_rounds = 3 at n = 257: the budget runs out, nothing hangs."""
    from utils_amd import evaluation as E
    got = _solve(gpu, 257, max_rounds=3)
    ref = assign_np.solve(AC.cost(257), max_rounds=3)
    assert got["converged"] is False and got["rounds"] == 3 and got["phases"] == 1
    np.testing.assert_array_equal(got["perm"].cpu().numpy(), ref["perm"])
    np.testing.assert_array_equal(got["price"].cpu().numpy(), ref["price"])
    rng = np.random.default_rng(3)
    x = rng.normal(size=(257, 5)).astype(np.float32)
    monkeypatch.setattr(E, "ASSIGN_MAX_ROUNDS", 3)
    with pytest.raises(RuntimeError):
        E.wasserstein_dist11_p(x, x + 1.0, method="auction")


def test_agrees_with_host_path(gpu):
    """The n = 200, d = 4 pair of test_sinkhorn_unbiased_and_exact_limit:
    method="auction" is within 2 quantum + s of method="hungarian"."""
    from utils_amd import evaluation as E
    rng = np.random.default_rng(11)
    x = rng.normal(size=(200, 4)).astype(np.float32)
    y = (rng.normal(size=(200, 4)) + 0.7).astype(np.float32)
    host = E.wasserstein_dist11_p(x, y, ord=2.0)
    dev = E.wasserstein_dist11_p(x, y, ord=2.0, method="auction")
    cost = E._dist2(E._dev(x), E._dev(y)).clamp_(min=0.0).sqrt_()
    res = E.linear_assignment(cost)
    s = 200 * 2.0 ** -52 * float(cost.max())
    print(f"auction - hungarian = {dev - host:.3e}, float32 costs along perm - hungarian = {res['cost'] - host:.3e}, "
          f"2 quantum = {2 * res['quantum']:.3e}, s = {s:.3e}")
    assert -s <= dev - host <= 2 * res["quantum"] + s
