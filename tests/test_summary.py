"""Streaming summaries without a GPU: the numpy mirror of the spec
(tests/summary_np.py) against the stored-draws estimators and closed forms,
and the argument checks of StreamingSummary / MCMC that need no device."""
import math

import numpy as np
import pytest
import torch

import summary_np as SN


def _stream(x, batch, nbins=512, span=8.0, blocks=None):
    """x [C, N, k] float32 stored draws -> mirror state fed in draw order."""
    C, N, k = x.shape
    x64 = x.reshape(-1, k).astype(np.float64)
    cal = SN.calibration(x64.mean(axis=0), span * x64.std(axis=0), nbins)
    st = SN.State(C, k, batch, nbins, cal)
    xt = np.ascontiguousarray(x.transpose(1, 0, 2))  # [N, C, k]
    at = 0
    for B in (blocks or [N]):
        SN.update(st, xt[at:at + B])
        at += B
    assert at == N
    return st


def _draws(C, N, k, seed):
    rng = np.random.default_rng(seed)
    loc = rng.uniform(-50, 50, k)
    scale = 10.0 ** rng.uniform(-2, 2, k)
    chain = rng.normal(size=(C, 1, k)) * 0.3  # chains disagree a little: r_hat > 1
    return ((rng.normal(size=(C, N, k)) + chain) * scale + loc).astype(np.float32)


@pytest.mark.parametrize("C,N,k", [(1, 50, 2), (2, 7, 3), (37, 129, 5), (1024, 64, 1), (16, 4096, 2)])
def test_r_hat_mean_std_equal_stored_draws(C, N, k):
    """float64 sums, sequential over N <= 4096 then C <= 1024 terms: each
    quantity is within about (N + C) 2^-53 of the stored-draws value on
    centred data, three orders inside 1e-9."""
    from infer_amd import diagnostics as D
    x = _draws(C, N, k, seed=C + N)
    out = SN.finalise(_stream(x, batch=max(1, math.isqrt(N))))
    np.testing.assert_allclose(out["r_hat"], D.gelman_rubin(x), rtol=1e-9, atol=0)
    x64 = x.astype(np.float64)
    np.testing.assert_allclose(out["mean"], x64.mean(axis=(0, 1)), rtol=1e-9, atol=0)
    np.testing.assert_allclose(out["std"], x64.std(axis=(0, 1)), rtol=1e-9, atol=0)
    assert out["n_draws"] == N


@pytest.mark.parametrize("nbins", [64, 512, 2048])
def test_quantile_within_a_bin_of_the_order_statistic(nbins):
    """The order statistic sort(x)[ceil(p n) - 1] lies in the located bin, and
    the float32 bin coordinate is off by less than 1e-3 bins."""
    x = _draws(33, 257, 4, seed=nbins)
    st = _stream(x, batch=16, nbins=nbins)
    probs = (0.0, 0.001, 0.05, 0.25, 0.5, 0.75, 0.95, 0.999, 1.0)
    q = SN.finalise(st, probs)["quantiles"]
    w = 1.0 / st.calib[2].astype(np.float64)
    flat = np.sort(x.reshape(-1, 4).astype(np.float64), axis=0)
    n = flat.shape[0]
    for i, p in enumerate(probs):
        order = flat[max(1, math.ceil(p * n)) - 1]
        assert np.all(np.abs(q[i] - order) <= 1.001 * w), (p, q[i], order, w)


def test_quantile_tails_and_nan_bin():
    """Mass outside the range gives -inf / +inf; NaNs leave the count n."""
    cal = SN.calibration([0.0], [4.0], 64)
    st = SN.State(2, 1, 1, 64, cal)
    x = np.array([[-5.0, 0.0], [5.0, np.nan], [1.0, 2.0]], np.float32).reshape(3, 2, 1)
    SN.update(st, x)
    out = SN.finalise(st, (0.0, 0.5, 1.0))
    assert (out["below"][0], out["above"][0], out["nan"][0]) == (1, 1, 1)
    assert out["quantiles"][0, 0] == -np.inf and out["quantiles"][2, 0] == np.inf
    assert 1.0 <= out["quantiles"][1, 0] <= 1.125  # r = 3 of n = 5: -5, 0, [1], 2, 5; bin width 1/8
    assert np.isnan(out["mean"][0]) and np.isnan(out["std"][0])


def test_bin_edges():
    cal = SN.calibration([0.0, 0.0], [4.0, 4.0], 64)  # lo = -4, w = 1/8: exact
    lo = np.float32(-4.0)
    x = np.array([lo, np.nextafter(lo, np.float32(-np.inf)), 4.0, 3.5,
                  np.inf, -np.inf, np.nan, -0.0], np.float32)
    b = SN.bins(np.stack([x, x], axis=-1), cal, 64)[:, 0]
    assert b.tolist() == [1, 0, 65, 61, 65, 0, 66, 33]


@pytest.mark.parametrize("phi,b,lo,hi", [(0.5, 64, 0.9, 1.1), (0.8, 50, 0.9, 1.1)])
def test_batch_means_n_eff_of_ar1(phi, b, lo, hi):
    """AR(1), C = 256, N = 4096: n_eff within 10 % of C N / tau_b, with
    tau_b = tau - 2 phi (1 - phi^b) / (b (1 - phi)^2) the batch-means
    expectation at batch length b and tau = (1 + phi) / (1 - phi)."""
    C, N = 256, 4096
    rng = np.random.default_rng(7)
    e = rng.normal(size=(C, N)) * math.sqrt(1 - phi * phi)
    x = np.empty((C, N))
    x[:, 0] = rng.normal(size=C)
    for t in range(1, N):
        x[:, t] = phi * x[:, t - 1] + e[:, t]
    out = SN.finalise(_stream(x[..., None].astype(np.float32), batch=b))
    tau = (1 + phi) / (1 - phi)
    tau_b = tau - 2 * phi * (1 - phi ** b) / (b * (1 - phi) ** 2)
    ratio = out["n_eff"][0] / (C * N / tau_b)
    print(f"phi {phi} b {b}: n_eff / (C N / tau_b) = {ratio:.4f}, n_eff / (C N / tau) = {ratio * tau / tau_b:.4f}, "
          f"n_eff_between / (C N / tau) = {out['n_eff_between'][0] / (C * N / tau):.3f}")
    assert lo <= ratio <= hi


def test_blocking_does_not_change_the_state():
    x = _draws(5, 23, 3, seed=1)
    a = _stream(x, batch=4)
    b = _stream(x, batch=4, blocks=[2, 1, 4, 9, 7])
    assert a.acc.tobytes() == b.acc.tobytes() and a.hist.tobytes() == b.hist.tobytes()
    assert SN.finalise(a)["n_eff"].shape == (3,)
    assert np.isnan(SN.finalise(_stream(x[:, :7], batch=4))["n_eff"]).all()  # one complete batch


# ------------------------------------------------------------ argument checks --
def test_constructor_refuses_bad_arguments():
    from infer_amd import StreamingSummary
    for kw in [dict(num_chains=0, num_cols=1, batch=1), dict(num_chains=1, num_cols=0, batch=1),
               dict(num_chains=1, num_cols=1025, batch=1), dict(num_chains=1, num_cols=1, batch=0),
               dict(num_chains=1, num_cols=1, batch=1, nbins=100), dict(num_chains=1, num_cols=1, batch=1, nbins=32),
               dict(num_chains=1, num_cols=1, batch=1, nbins=4096)]:
        with pytest.raises(ValueError):
            StreamingSummary(device="cpu", **kw)


def test_update_and_calibration_refuse_bad_input_without_a_launch():
    from infer_amd import StreamingSummary
    s = StreamingSummary(4, 3, batch=2, device="cpu")
    good = torch.zeros(2, 4, 3)
    with pytest.raises(ValueError, match="not calibrated"):
        s.update(good)
    with pytest.raises(ValueError, match="column 1"):
        s.calibrate(torch.tensor([[0.0, 1.0, 2.0], [1.0, 1.0, 3.0]]))  # column 1 is constant
    with pytest.raises(ValueError, match="column 2"):
        s.calibrate(torch.tensor([[0.0, 1.0, float("inf")], [1.0, 2.0, 3.0]]))
    with pytest.raises(ValueError, match="column 0"):
        s.set_range([0.0, 0.0, 0.0], [0.0, 1.0, 1.0])
    with pytest.raises(ValueError):
        s.set_range([0.0, 0.0], [1.0, 1.0])
    s.set_range([0.0, 1.0, 2.0], [1.0, 2.0, 4.0])
    np.testing.assert_array_equal(s.calib.numpy(), SN.calibration([0.0, 1.0, 2.0], [1.0, 2.0, 4.0], 512))
    for bad in (torch.zeros(2, 4, 3, dtype=torch.float64), torch.zeros(2, 3, 3), torch.zeros(2, 4, 3, 1),
                torch.zeros(0, 4, 3), torch.zeros(2, 4, 6)[:, :, ::2], np.zeros((2, 4, 3), np.float32)):
        with pytest.raises(ValueError):
            s.update(bad)
    from kernels_amd._lib import AmhError
    with pytest.raises(AmhError):  # a host tensor: no CPU fallback
        s.update(good)
    assert s.n_draws == 0 and not s.acc.any() and not s.hist.any()
    with pytest.raises(RuntimeError):
        s.summary()


def test_state_dict_shape_checks():
    from infer_amd import StreamingSummary
    a = StreamingSummary(4, 3, batch=2, device="cpu").set_range([0.0] * 3, [1.0] * 3)
    sd = a.state_dict()
    b = StreamingSummary(4, 3, batch=2, device="cpu").load_state_dict(sd)
    assert torch.equal(a.calib, b.calib) and b.n_draws == 0
    with pytest.raises(ValueError):
        StreamingSummary(4, 3, batch=3, device="cpu").load_state_dict(sd)
    with pytest.raises(ValueError):
        StreamingSummary(5, 3, batch=2, device="cpu").load_state_dict(sd)


def test_mcmc_summary_arguments():
    from infer_amd import MCMC
    m = MCMC(object(), num_warmup=1, num_samples=4)
    with pytest.raises(ValueError, match="summary_only"):
        m.run(None, summary_batch=2)
    with pytest.raises(ValueError, match="summary_only"):
        m.run(None, summary_block=2)
    with pytest.raises(ValueError, match="extra_fields"):
        m.run(None, summary_only=True, extra_fields=("potential_energy",))
    with pytest.raises(ValueError):
        m.run(None, summary_only=True, summary_batch=0)
    with pytest.raises(ValueError):
        m.run(None, summary_only=True, summary_block=0)


@pytest.mark.parametrize("C,N,k,b", [(1, 9, 2, 2), (7, 40, 3, 6), (3, 1, 2, 1), (5, 3, 1, 4)])
def test_summary_finalisation_equals_the_mirror(C, N, k, b):
    """StreamingSummary.summary() on a state loaded from the mirror (host
    tensors: the finalisation is torch float64, no kernel)."""
    from infer_amd import StreamingSummary
    x = _draws(C, N, k, seed=N)
    x[0, 0, 0] = 1e9
    st = _stream(x, batch=b, nbins=128, span=1.0)  # a 1 std range: draws in the under and over bins
    s = StreamingSummary(C, k, batch=b, nbins=128, device="cpu")
    s.load_state_dict({"num_chains": C, "num_cols": k, "batch": b, "nbins": 128, "n_draws": st.n,
                       "acc": torch.as_tensor(st.acc), "hist": torch.as_tensor(st.hist),
                       "calib": torch.as_tensor(st.calib)})
    probs = (0.0, 0.05, 0.5, 0.95, 1.0)
    got, ref = s.summary(probs), SN.finalise(st, probs)
    assert set(got) == set(ref)
    for name in ref:
        np.testing.assert_allclose(got[name], ref[name], rtol=1e-9, atol=0, equal_nan=True, err_msg=name)
    assert got["above"][0] >= 1 and got["quantiles"][-1, 0] == np.inf
