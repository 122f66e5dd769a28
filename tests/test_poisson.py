"""posteriors.poisson_regression (include/amh.h AMH_MODEL_POISSON): the
registry entry's layout, constants and argument checks, and the float64
restatement of its potential against closed forms.  No GPU."""
import math

import numpy as np
import pytest
import torch


def _entry(N=7, K=3, seed=0, offset=True, **kw):
    import posteriors as P
    d = P.synthetic_poisson(N, K, seed)
    return P.poisson_regression(d["X"], d["y"], d["offset"] if offset else None, **kw), d


def test_registry_entry_layout():
    import posteriors as P
    from kernels_amd import _lib
    assert _lib.AMH_MODEL_POISSON == 9
    e, d = _entry(N=7, K=3, prior_scale=1.5, intercept_scale=4.0)
    assert e.model_id == _lib.AMH_MODEL_POISSON
    assert e.dim({}) == 4 and e.dim() == 4
    assert [(s.name, s.size, s.transform) for s in e.sites({})] == [("Intercept", 1, "identity"),
                                                                    ("b", 3, "identity")]
    data, ip = e.pack({}, "cpu")
    assert ip == (7, 3)
    assert data.dtype == torch.float32 and data.shape == (7 * 3 + 2 * 7 + 3,)
    a = data.numpy()
    np.testing.assert_array_equal(a[:21], d["X"].reshape(-1))  # X row-major
    np.testing.assert_array_equal(a[21:28], d["y"])
    np.testing.assert_array_equal(a[28:35].view(np.uint32), d["offset"].view(np.uint32))
    assert d["y"].max() >= 2  # counts, so that lgamma(y + 1) is not all 0
    # iI2, ib2, c0 (with sum_n lgamma(y_n + 1)): float64 on the host, rounded once
    c0 = math.log(4.0 * math.sqrt(2 * math.pi)) + 3 * math.log(1.5 * math.sqrt(2 * math.pi)) \
        + math.fsum(math.lgamma(float(v) + 1.0) for v in d["y"])
    want = np.array([1.0 / 16.0, 1.0 / 2.25, c0], np.float64).astype(np.float32)
    np.testing.assert_array_equal(a[35:].view(np.uint32), want.view(np.uint32))
    # no offset: all +0 (the sign bit too)
    e0 = P.poisson_regression(d["X"], d["y"])
    a0 = e0.pack({}, "cpu")[0].numpy()
    assert np.all(a0[28:35].view(np.uint32) == 0)
    # defaults: prior_scale 2.5, intercept_scale 10
    np.testing.assert_array_equal(e0.consts[:2], np.array([0.01, 0.16], np.float64).astype(np.float32))
    # y by hand: lgamma(1) + lgamma(2) + lgamma(4) + lgamma(11) = log 6 + log 10!
    e1 = P.poisson_regression(np.zeros((4, 1)), [0, 1, 3, 10], prior_scale=1.0, intercept_scale=1.0)
    want1 = np.float32(2 * math.log(math.sqrt(2 * math.pi)) + math.log(6.0) + math.log(3628800.0))
    assert abs(float(e1.consts[2]) - float(want1)) <= float(np.spacing(want1))


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
    y = np.array([0, 1, 0, 7, 2.0 ** 24], np.float32)
    o = np.linspace(-1, 1, 5)
    P.poisson_regression(X, y)
    P.poisson_regression(X, y, o)
    P.poisson_regression(np.zeros((5, 31)), y, offset=o)
    bad = [
        (dict(X=np.zeros(5), y=y), "2-D"),
        (dict(X=np.zeros((5, 2, 1)), y=y), "2-D"),
        (dict(X=np.zeros((5, 32)), y=y), "K = 32"),
        (dict(X=np.zeros((5, 0)), y=y), "K = 0"),
        (dict(X=np.zeros((0, 2)), y=np.zeros(0)), "row"),
        (dict(X=np.array([[np.inf, 0]] * 5), y=y), "X must be finite"),
        (dict(X=np.array([[np.nan, 0]] * 5), y=y), "X must be finite"),
        (dict(X=np.full((5, 2), 1e39), y=y), "X must be finite"),  # overflows float32
        (dict(X=X, y=y, offset=np.array([0, 0, np.inf, 0, 0])), "offset must be finite"),
        (dict(X=X, y=y, offset=np.array([0, 0, np.nan, 0, 0])), "offset must be finite"),
        (dict(X=X, y=y, offset=np.array([0, 0, 1e39, 0, 0])), "offset must be finite"),
        (dict(X=X, y=y, offset=o[:4]), "offset has 4 entries"),
        (dict(X=X, y=y[:4]), "y has 4 entries"),
        (dict(X=X, y=np.array([0, 1, -1, 0, 1])), "every y"),
        (dict(X=X, y=np.array([0, 1, 0.5, 0, 1])), "every y"),
        (dict(X=X, y=np.array([0, 1, np.nan, 0, 1])), "every y"),
        (dict(X=X, y=np.array([0, 1, np.inf, 0, 1])), "every y"),
        (dict(X=X, y=np.array([0, 1, 2.0 ** 24 + 2, 0, 1])), "every y"),
        (dict(X=X, y=y, prior_scale=0.0), "prior_scale"),
        (dict(X=X, y=y, prior_scale=-1.0), "prior_scale"),
        (dict(X=X, y=y, prior_scale=float("inf")), "prior_scale"),
        (dict(X=X, y=y, intercept_scale=0.0), "intercept_scale"),
        (dict(X=X, y=y, intercept_scale=float("nan")), "intercept_scale"),
    ]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            P.poisson_regression(**kw)


def test_synthetic_poisson():
    import posteriors as P
    d = P.synthetic_poisson(500, 4, seed=3)
    assert d["X"].shape == (500, 4) and d["X"].dtype == np.float32
    assert d["y"].shape == (500,) and d["y"].dtype == np.float32
    assert d["offset"].shape == (500,) and d["offset"].dtype == np.float32
    assert np.all(d["y"] >= 0) and np.all(d["y"] == np.floor(d["y"])) and d["y"].max() > 1
    assert np.all(np.abs(d["offset"]) <= 1.0) and d["offset"].min() < -0.5 and d["offset"].max() > 0.5
    d2 = P.synthetic_poisson(500, 4, seed=3)
    for k in ("X", "y", "offset"):
        assert d[k].tobytes() == d2[k].tobytes()
    assert P.synthetic_poisson(500, 4, seed=4)["y"].tobytes() != d["y"].tobytes()
    # eta stays within a few units at the generating coefficients' scale, at small and large K
    for K in (1, 31):
        dk = P.synthetic_poisson(2000, K, seed=1)
        assert dk["y"].max() < 200  # e^5.3
    P.poisson_regression(d["X"], d["y"], d["offset"])


def test_f64_potential_closed_forms():
    import posteriors as P
    # z = 0: eta_n = o_n, so row n gives e^{o_n} - y_n o_n, the priors give c0
    e, d = _entry(N=23, K=5)
    u = P.poisson_potential_f64(torch.zeros(3, 6), e)
    assert u.dtype == torch.float64 and u.shape == (3,)
    o64, y64 = d["offset"].astype(np.float64), d["y"].astype(np.float64)
    want = float((np.exp(o64) - y64 * o64).sum()) + float(e.consts[2])
    np.testing.assert_allclose(u.numpy(), want, rtol=1e-14)
    # ... which is sum_n e^{o_n} + c0 where y o vanishes: all counts 0 (c0 then has no lgamma share)
    ez = P.poisson_regression(d["X"], np.zeros(23), d["offset"])
    np.testing.assert_allclose(P.poisson_potential_f64(np.zeros(6), ez).numpy(),
                               float(np.exp(o64).sum()) + float(ez.consts[2]), rtol=1e-14)
    # without an offset: N + c0
    e0, _ = _entry(N=23, K=5, offset=False)
    np.testing.assert_allclose(P.poisson_potential_f64(np.zeros(6), e0).numpy(), 23 + float(e0.consts[2]), rtol=1e-15)
    # one row, K = 1, by hand: X = 0.5, y = 3, o = 0.25, I = 0.25, b = -1.5
    e1 = P.poisson_regression(np.array([[0.5]]), np.array([3.0]), np.array([0.25]), prior_scale=2.0,
                              intercept_scale=4.0)
    eta = 0.25 + 0.5 * -1.5 + 0.25
    want = (math.exp(eta) - 3.0 * eta) + 0.5 * 1.5 ** 2 * float(e1.consts[1]) \
        + 0.5 * 0.25 ** 2 * float(e1.consts[0]) + float(e1.consts[2])
    got = float(P.poisson_potential_f64(np.array([0.25, -1.5]), e1))
    assert got == pytest.approx(want, rel=1e-15)
    assert float(e1.consts[0]) == 1 / 16 and float(e1.consts[1]) == 0.25
    c0 = math.log(4.0 * math.sqrt(2 * math.pi)) + math.log(2.0 * math.sqrt(2 * math.pi)) + math.log(6.0)
    assert float(e1.consts[2]) == float(np.float32(c0))


def test_f64_potential_gradient():
    """Central differences of poisson_potential_f64 against X'(e^eta - y) plus
    the prior terms."""
    import posteriors as P
    e, d = _entry(N=31, K=4, seed=5)
    X, y, o = (d[k].astype(np.float64) for k in ("X", "y", "offset"))
    iI2, ib2 = float(e.consts[0]), float(e.consts[1])
    z = np.random.default_rng(1).uniform(-1, 1, size=(6, 5))
    r = np.exp(z[:, :1] + z[:, 1:] @ X.T + o) - y  # [6, N]
    grad = np.concatenate([r.sum(-1, keepdims=True) + z[:, :1] * iI2, r @ X + z[:, 1:] * ib2], axis=1)
    h = 1e-5
    for j in range(5):
        dz = np.zeros(5)
        dz[j] = h
        fd = (P.poisson_potential_f64(z + dz, e) - P.poisson_potential_f64(z - dz, e)).numpy() / (2 * h)
        # central differences: O(h^2 U''') truncation + O(eps U / h) rounding; U and its derivatives are at
        # most a few thousand here (31 rows, |eta| < 8), so both stay below 1e-6 absolute
        np.testing.assert_allclose(fd, grad[:, j], rtol=1e-7, atol=1e-6)


def posterior_2d_quadrature(e):
    """Mean and covariance of exp(-U) of a K = 1 entry by float64 quadrature in
    two passes: a 401 x 401 grid over [-8, 8]^2 locates the posterior (mean m1,
    sds s1), then a 401 x 401 grid over m1 +- 8 s1 (spacing s1 / 25) gives the
    moments.  -> (mean [2], cov [2, 2], spacing [2], the largest weight on the
    fine grid's boundary relative to the largest weight)."""
    import posteriors as P

    def moments(g0, g1):
        zz = torch.stack(torch.meshgrid(g0, g1, indexing="ij"), -1).reshape(-1, 2)
        u = P.poisson_potential_f64(zz, e)
        w = torch.exp(-(u - u.min()))
        edge = w.reshape(len(g0), len(g1))
        edge = max(float(edge[0].max()), float(edge[-1].max()), float(edge[:, 0].max()), float(edge[:, -1].max()))
        w = w / w.sum()
        mean = (w[:, None] * zz).sum(0)
        dz = zz - mean
        cov = (w[:, None, None] * dz[:, :, None] * dz[:, None, :]).sum(0)
        return mean, cov, edge

    g = torch.linspace(-8.0, 8.0, 401, dtype=torch.float64)
    m1, c1, _ = moments(g, g)
    s1 = torch.sqrt(torch.diagonal(c1))
    gs = [torch.linspace(float(m1[j] - 8 * s1[j]), float(m1[j] + 8 * s1[j]), 401, dtype=torch.float64) for j in (0, 1)]
    mean, cov, edge = moments(*gs)
    spacing = np.array([float(gs[j][1] - gs[j][0]) for j in (0, 1)])
    return mean.numpy(), cov.numpy(), spacing, edge


def posterior_entry():
    """The K = 1, N = 40 data set with offsets of the posterior tests
    (tests/test_gpu_poisson.py::test_samples_posterior)."""
    import posteriors as P
    d = P.synthetic_poisson(40, 1, 40)
    return P.poisson_regression(d["X"], d["y"], d["offset"])


def test_posterior_quadrature_grid():
    """The reference moments of the GPU posterior test: the fine grid's spacing
    is at most a tenth of the smaller posterior sd, the grid holds the mass
    (boundary weights below 1e-9 of the peak) and the moments are plausible."""
    e = posterior_entry()
    mean, cov, spacing, edge = posterior_2d_quadrature(e)
    sd = np.sqrt(np.diag(cov))
    print("posterior mean", mean, "sd", sd, "spacing", spacing, "edge", edge)
    assert spacing.max() <= sd.min() / 10
    assert edge < 1e-9  # 8 sds out; the GPU test's budget is 6 / 64 of an sd
    assert np.all(sd > 0.02) and np.all(sd < 2.0) and abs(cov[0, 1]) < sd[0] * sd[1]
    # the posterior sits near the generating intercept 0.5 (flat priors, 40 rows)
    assert abs(mean[0] - 0.5) < 5 * sd[0] + 0.5
