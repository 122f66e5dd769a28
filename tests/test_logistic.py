"""posteriors.logistic_regression (include/amh.h AMH_MODEL_LOGISTIC): the
registry entry's layout, constants and argument checks, and the float64
restatement of its potential against closed forms.  No GPU."""
import math

import numpy as np
import pytest
import torch


def _entry(N=7, K=3, seed=0, **kw):
    import posteriors as P
    d = P.synthetic_logistic(N, K, seed)
    return P.logistic_regression(d["X"], d["y"], **kw), d


def test_registry_entry_layout():
    import posteriors as P
    from kernels_amd import _lib
    assert _lib.AMH_MODEL_LOGISTIC == 8
    e, d = _entry(N=7, K=3, prior_scale=1.5, intercept_scale=4.0)
    assert e.model_id == _lib.AMH_MODEL_LOGISTIC
    assert e.dim({}) == 4 and e.dim() == 4
    assert [(s.name, s.size, s.transform) for s in e.sites({})] == [("Intercept", 1, "identity"),
                                                                    ("b", 3, "identity")]
    data, ip = e.pack({}, "cpu")
    assert ip == (7, 3)
    assert data.dtype == torch.float32 and data.shape == (7 * 3 + 7 + 3,)
    a = data.numpy()
    np.testing.assert_array_equal(a[:21], d["X"].reshape(-1))  # X row-major
    np.testing.assert_array_equal(a[21:28], d["y"])
    assert set(np.unique(a[21:28])) <= {0.0, 1.0}
    # iI2, ib2, c0: float64 on the host, rounded once
    c0 = math.log(4.0 * math.sqrt(2 * math.pi)) + 3 * math.log(1.5 * math.sqrt(2 * math.pi))
    want = np.array([1.0 / 16.0, 1.0 / 2.25, c0], np.float64).astype(np.float32)
    np.testing.assert_array_equal(a[28:].view(np.uint32), want.view(np.uint32))
    # defaults: prior_scale 2.5, intercept_scale 10
    e2 = P.logistic_regression(d["X"], d["y"])
    np.testing.assert_array_equal(e2.consts[:2], np.array([0.01, 0.16], np.float64).astype(np.float32))


@pytest.mark.parametrize("K", [1, 5])
def test_unravel_postprocess_shapes(K):
    e, _ = _entry(N=4, K=K)
    z = torch.arange(6 * 2 * (K + 1), dtype=torch.float32).reshape(6, 2, K + 1)
    for out in (e.unravel(z, {}), e.postprocess(z, {})):
        assert list(out) == ["Intercept", "b"]
        assert out["Intercept"].shape == (6, 2) and out["b"].shape == (6, 2, K)
        assert torch.equal(out["Intercept"], z[..., 0]) and torch.equal(out["b"], z[..., 1:])


def test_argument_checks():
    import posteriors as P
    X = np.zeros((5, 2), np.float32)
    y = np.array([0, 1, 0, 1, 1], np.float32)
    P.logistic_regression(X, y)
    P.logistic_regression(np.zeros((5, 31)), y)
    bad = [
        (dict(X=np.zeros(5), y=y), "2-D"),
        (dict(X=np.zeros((5, 2, 1)), y=y), "2-D"),
        (dict(X=np.zeros((5, 32)), y=y), "K = 32"),
        (dict(X=np.zeros((5, 0)), y=y), "K = 0"),
        (dict(X=np.zeros((0, 2)), y=np.zeros(0)), "row"),
        (dict(X=np.array([[np.inf, 0]] * 5), y=y), "finite"),
        (dict(X=np.array([[np.nan, 0]] * 5), y=y), "finite"),
        (dict(X=np.full((5, 2), 1e39), y=y), "finite"),  # overflows float32
        (dict(X=X, y=y[:4]), "entries"),
        (dict(X=X, y=np.array([0, 1, 2, 0, 1])), "0 or 1"),
        (dict(X=X, y=np.array([0, 1, 0.5, 0, 1])), "0 or 1"),
        (dict(X=X, y=np.array([0, 1, np.nan, 0, 1])), "0 or 1"),
        (dict(X=X, y=y, prior_scale=0.0), "prior_scale"),
        (dict(X=X, y=y, prior_scale=-1.0), "prior_scale"),
        (dict(X=X, y=y, intercept_scale=0.0), "intercept_scale"),
        (dict(X=X, y=y, intercept_scale=float("nan")), "intercept_scale"),
    ]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            P.logistic_regression(**kw)


def test_pooled_asss_refuses_the_model():
    """The pooled slice kernels are instantiated per model and have none for
    this one: the class says so."""
    from kernels_amd import PooledASSS
    e, _ = _entry()
    with pytest.raises(ValueError, match="logistic_regression"):
        PooledASSS(model=e, num_chains=4)


def test_synthetic_logistic():
    import posteriors as P
    d = P.synthetic_logistic(50, 4, seed=3)
    assert d["X"].shape == (50, 4) and d["X"].dtype == np.float32
    assert d["y"].shape == (50,) and set(np.unique(d["y"])) == {0.0, 1.0}
    d2 = P.synthetic_logistic(50, 4, seed=3)
    assert d["X"].tobytes() == d2["X"].tobytes() and d["y"].tobytes() == d2["y"].tobytes()


def test_f64_potential_closed_forms():
    import posteriors as P
    # z = 0: every row gives log 2, the priors give c0
    e, _ = _entry(N=23, K=5)
    u = P.logistic_potential_f64(torch.zeros(3, 6), e)
    assert u.dtype == torch.float64 and u.shape == (3,)
    np.testing.assert_allclose(u.numpy(), 23 * math.log(2.0) + float(e.consts[2]), rtol=1e-15)
    # one row, K = 1, by hand: X = 0.5, y = 1, I = 0.25, b = -1.5
    e1 = P.logistic_regression(np.array([[0.5]]), np.array([1.0]), prior_scale=2.0, intercept_scale=4.0)
    eta = 0.25 + 0.5 * -1.5
    want = (math.log1p(math.exp(eta)) - eta) + 0.5 * 1.5 ** 2 * float(e1.consts[1]) \
        + 0.5 * 0.25 ** 2 * float(e1.consts[0]) + float(e1.consts[2])
    got = float(P.logistic_potential_f64(np.array([0.25, -1.5]), e1))
    assert got == pytest.approx(want, rel=1e-15)
    assert float(e1.consts[0]) == 1 / 16 and float(e1.consts[1]) == 0.25
    # saturated rows stay finite in float64
    big = P.logistic_potential_f64(np.array([0.0, 4000.0]), e1)
    assert math.isfinite(float(big))


def test_f64_potential_gradient():
    """Central differences of logistic_potential_f64 against X'(sigma(eta) - y)
    plus the prior terms."""
    import posteriors as P
    e, d = _entry(N=31, K=4, seed=5)
    X, y = d["X"].astype(np.float64), d["y"].astype(np.float64)
    iI2, ib2 = float(e.consts[0]), float(e.consts[1])
    z = np.random.default_rng(1).uniform(-2, 2, size=(6, 5))
    r = 1.0 / (1.0 + np.exp(-(z[:, :1] + z[:, 1:] @ X.T))) - y  # [6, N]
    grad = np.concatenate([r.sum(-1, keepdims=True) + z[:, :1] * iI2, r @ X + z[:, 1:] * ib2], axis=1)
    h = 1e-5
    for j in range(5):
        dz = np.zeros(5)
        dz[j] = h
        fd = (P.logistic_potential_f64(z + dz, e) - P.logistic_potential_f64(z - dz, e)).numpy() / (2 * h)
        # central differences: O(h^2 U''') truncation + O(eps U / h) rounding, both below 1e-8 * scale here
        np.testing.assert_allclose(fd, grad[:, j], rtol=1e-7, atol=1e-7)
