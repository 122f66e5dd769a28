"""Streaming summaries on the GPU (csrc/amh_summary.hip through
infer_amd.StreamingSummary and MCMC(summary_only=True)): accumulators and
histogram byte for byte against the numpy mirror of the spec
(tests/summary_np.py), independent of blocking and of the run, the edge
values in their bins, and the finalisation against the mirror's and against
the stored-draws estimators."""
import math

import numpy as np
import pytest
import torch

import summary_np as SN

pytestmark = pytest.mark.gpu

# C, k, B, b, nbins: one element; k < tile with ragged chains; k just past the
# 32-column tile at the 16-column tile of 2048 bins; k = two full tiles, more
# than one chain group per pass; k = 65 (a one-column last tile); k = 256
SHAPES = [(1, 1, 1, 1, 64), (63, 10, 5, 3, 512), (65, 33, 4, 3, 2048), (257, 64, 7, 4, 512), (130, 65, 3, 2, 128),
          (64, 256, 2, 5, 256)]


def _block(C, k, B, seed=0):
    rng = np.random.default_rng([seed, C, k, B])
    loc = rng.uniform(-20, 20, k)
    scale = 10.0 ** rng.uniform(-1, 1, k)
    return (rng.normal(size=(B, C, k)) * scale + loc).astype(np.float32), loc, scale


def _pair(gpu, C, k, b, nbins, loc, scale, span=3.0):
    """(device summary, mirror state) with the same calibration; span 3 puts
    some draws into the under and over bins."""
    from infer_amd import StreamingSummary
    s = StreamingSummary(C, k, batch=b, nbins=nbins, device=gpu).set_range(loc, span * scale)
    cal = SN.calibration(loc, span * scale, nbins)
    np.testing.assert_array_equal(s.calib.cpu().numpy(), cal)
    return s, SN.State(C, k, b, nbins, cal)


def _same_bytes(s, st):
    assert s.acc.cpu().numpy().tobytes() == st.acc.tobytes()
    assert s.hist.cpu().numpy().tobytes() == st.hist.tobytes()
    assert s.n_draws == st.n


@pytest.mark.parametrize("C,k,B,b,nbins", SHAPES)
def test_bytes_equal_the_mirror(C, k, B, b, nbins, gpu):
    x, loc, scale = _block(C, k, B)
    s, st = _pair(gpu, C, k, b, nbins, loc, scale)
    xd = torch.as_tensor(x).to(gpu)
    for _ in range(2):  # the second block starts mid-batch when b does not divide B
        s.update(xd)
        SN.update(st, x)
    _same_bytes(s, st)
    assert int(s.hist.sum()) == 2 * B * C * k
    if C * B >= 100:
        assert int(s.hist[:, 0].sum()) > 0 and int(s.hist[:, nbins + 1].sum()) > 0


@pytest.mark.parametrize("C,k,b,nbins", [(63, 10, 3, 512), (257, 64, 4, 512)])
def test_blocking_and_rerun_do_not_change_a_byte(C, k, b, nbins, gpu):
    x, loc, scale = _block(C, k, 7, seed=1)
    xd = torch.as_tensor(x).to(gpu)
    whole, st = _pair(gpu, C, k, b, nbins, loc, scale)
    whole.update(xd)
    SN.update(st, x)
    _same_bytes(whole, st)
    again, _ = _pair(gpu, C, k, b, nbins, loc, scale)
    again.update(xd)
    parts, _ = _pair(gpu, C, k, b, nbins, loc, scale)
    parts.update(xd[:2]).update(xd[2]).update(xd[3:])  # 2 + 1 + 4; [C, k] is one draw
    for other in (again, parts):
        assert torch.equal(other.acc.view(torch.int64), whole.acc.view(torch.int64))
        assert torch.equal(other.hist, whole.hist)
        assert other.n_draws == 7


def test_edge_values(gpu):
    """One chain per case, one draw each (then a finite one): lo, the float
    below lo, lo + nbins w, +inf, -inf, NaN, and -0.0."""
    from infer_amd import StreamingSummary
    nbins = 64
    lo = np.float32(-4.0)  # center 0, hw 4: lo and w = 1/8 are exact, lo + nbins w = 4
    vals = np.array([lo, np.nextafter(lo, np.float32(-np.inf)), 4.0, np.inf, -np.inf, np.nan, -0.0], np.float32)
    want = [1, 0, nbins + 1, nbins + 1, 0, nbins + 2, 33]
    C = len(vals)
    x = np.stack([vals[:, None], np.ones((C, 1), np.float32)])  # [2, C, 1]
    s = StreamingSummary(C, 1, batch=1, nbins=nbins, device=gpu).set_range([0.0], [4.0])
    s.update(torch.as_tensor(x[:1]).to(gpu))
    hist = s.hist.cpu().numpy()[0]
    ref = np.bincount(want, minlength=nbins + 3)
    np.testing.assert_array_equal(hist, ref)
    s.update(torch.as_tensor(x[1:]).to(gpu))
    st = SN.update(SN.State(C, 1, 1, nbins, SN.calibration([0.0], [4.0], nbins)), x)
    np.testing.assert_array_equal(s.hist.cpu().numpy(), st.hist)
    acc = s.acc.cpu().numpy()
    # NaN payloads are not part of the spec: NaN where the mirror has NaN, equal bytes elsewhere
    np.testing.assert_array_equal(np.isnan(acc), np.isnan(st.acc))
    fin = ~np.isnan(acc)
    assert acc[fin].tobytes() == st.acc[fin].tobytes()
    S1, S2, bs, S1b, Q = acc[:, :, 0]
    assert S1[3] == np.inf and S2[3] == np.inf and S1b[3] == np.inf and Q[3] == np.inf
    assert S1[4] == -np.inf and S2[4] == np.inf and Q[4] == np.inf
    assert np.isnan(acc[:, 5, 0][[0, 1, 3, 4]]).all() and bs[5] == 0.0
    assert S1[0] == -3.0 and S2[0] == 17.0 and Q[0] == 17.0  # -4 and 1, untouched by the other rows
    out = s.summary()
    assert out["nan"][0] == 1 and out["below"][0] == 2 and out["above"][0] == 2
    assert np.isnan(out["mean"][0])


def test_block_view_off_a_16_byte_boundary(gpu):
    C, k, B, b, nbins = 65, 33, 4, 3, 512
    x, loc, scale = _block(C, k, B, seed=2)
    s, st = _pair(gpu, C, k, b, nbins, loc, scale)
    buf = torch.zeros(B * C * k + 1, dtype=torch.float32, device=gpu)
    view = buf[1:].view(B, C, k)
    view.copy_(torch.as_tensor(x))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    s.update(view)
    SN.update(st, x)
    _same_bytes(s, st)


def test_summary_against_mirror_and_stored_draws(gpu):
    from infer_amd import StreamingSummary
    from infer_amd import diagnostics as D
    C, k, N, b = 48, 5, 96, 8
    rng = np.random.default_rng(5)
    x, loc, scale = _block(C, k, N, seed=3)
    x += (rng.normal(size=(1, C, k)) * 0.3 * scale).astype(np.float32)  # chains disagree a little
    xd = torch.as_tensor(x).to(gpu)
    s = StreamingSummary(C, k, batch=b, device=gpu).calibrate(xd)
    st = SN.State(C, k, b, 512, s.calib.cpu().numpy())
    x64 = x.reshape(-1, k).astype(np.float64)
    np.testing.assert_allclose(st.calib.astype(np.float64),
                               SN.calibration(x64.mean(axis=0), 8.0 * x64.std(axis=0), 512), rtol=1e-6)
    for at in range(0, N, 40):
        s.update(xd[at:at + 40])
        SN.update(st, x[at:at + 40])
    _same_bytes(s, st)
    probs = (0.0, 0.05, 0.5, 0.95, 1.0)
    got, ref = s.summary(probs), SN.finalise(st, probs)
    assert set(got) == set(ref)
    for name in ref:
        np.testing.assert_allclose(got[name], ref[name], rtol=1e-9, atol=0, err_msg=name)
    stored = x.transpose(1, 0, 2)  # [C, N, k]
    np.testing.assert_allclose(got["r_hat"], D.gelman_rubin(stored), rtol=1e-9, atol=0)
    np.testing.assert_allclose(got["mean"], x64.mean(axis=0), rtol=1e-9, atol=0)
    np.testing.assert_allclose(got["std"], x64.std(axis=0), rtol=1e-9, atol=0)
    w = 1.0 / st.calib[2].astype(np.float64)
    flat = np.sort(x64, axis=0)
    for i, p in enumerate(probs):
        order = flat[max(1, math.ceil(p * flat.shape[0])) - 1]
        assert np.all(np.abs(got["quantiles"][i] - order) <= 1.001 * w), (p, got["quantiles"][i], order)
    assert np.all(got["n_eff"] > 0) and np.all(got["n_eff_between"] > 0)


def test_state_dict_round_trip_mid_stream(gpu):
    from infer_amd import StreamingSummary
    C, k, b, nbins = 63, 10, 3, 512
    x, loc, scale = _block(C, k, 7, seed=4)
    xd = torch.as_tensor(x).to(gpu)
    whole, _ = _pair(gpu, C, k, b, nbins, loc, scale)
    whole.update(xd)
    first, _ = _pair(gpu, C, k, b, nbins, loc, scale)
    first.update(xd[:4])  # stops inside the second batch
    sd = first.state_dict()
    assert all(not v.is_cuda for v in sd.values() if isinstance(v, torch.Tensor))
    resumed = StreamingSummary(C, k, batch=b, nbins=nbins, device=gpu).load_state_dict(sd)
    first.update(xd[4:5])  # the saved state is a copy: the source moving on does not touch it
    resumed.update(xd[4:])
    assert torch.equal(resumed.acc.view(torch.int64), whole.acc.view(torch.int64))
    assert torch.equal(resumed.hist, whole.hist) and resumed.n_draws == 7


def test_update_refuses_bad_blocks_on_the_device(gpu):
    x, loc, scale = _block(4, 3, 2)
    s, _ = _pair(gpu, 4, 3, 2, 64, loc, scale)
    xd = torch.as_tensor(x).to(gpu)
    for bad in (xd.double(), xd[:, :3], xd.transpose(0, 1), xd.cpu(), torch.zeros(2, 4, 6, device=gpu)[:, :, ::2]):
        with pytest.raises(ValueError):
            s.update(bad)
    assert s.n_draws == 0 and not s.acc.any() and not s.hist.any()


def test_mcmc_summary_only_eight_schools(gpu):
    """64 chains, 200 warmup, 256 samples, block 64: the accumulators equal
    the mirror fed the same blocks from a manual kernel.run loop under the
    same key; no draws are kept; one table row per constrained site."""
    import posteriors as P
    from infer_amd import MCMC
    from kernels_amd import ARWMH, PRNGKey
    C = 64
    data = dict(P.EIGHT_SCHOOLS_DATA)
    m = MCMC(ARWMH(model=P.eight_schools, num_chains=C, device=gpu), num_warmup=200, num_samples=256)
    m.run(PRNGKey(11), summary_only=True, summary_block=64, **data)
    s = m.streaming_summary
    assert s is not None and s.n_draws == 256 and s.num_cols == 18 and s.batch == 16  # mu, tau, theta_base, theta
    with pytest.raises(RuntimeError, match="no draws were kept"):
        m.get_samples()

    k = ARWMH(model=P.eight_schools, num_chains=C, device=gpu)
    state = k.init(PRNGKey(11), 200, None, (), data)
    k.sample_(state, 200)
    fn = k.postprocess_fn((), data)
    st = None
    for _ in range(4):
        state, cz, _ = k.run(state, 64, 1, collect_z=True, collect_pe=False)
        sites = fn(cz)
        assert list(sites) == ["mu", "tau", "theta_base", "theta"]
        x = torch.cat([v.reshape(64, C, -1) for v in sites.values()], dim=2).cpu().numpy()
        if st is None:
            x64 = x.reshape(-1, 18).astype(np.float64)
            # the calibration is the device's float64 reduction: the same numbers to rounding
            np.testing.assert_allclose(s.calib.cpu().numpy(),
                                       SN.calibration(x64.mean(axis=0), 8.0 * x64.std(axis=0), 512), rtol=1e-6)
            st = SN.State(C, 18, 16, 512, s.calib.cpu().numpy())
        SN.update(st, x)
    _same_bytes(s, st)
    assert torch.equal(m.last_state.z, state.z)

    txt = m.summary_str()
    rows = [ln for ln in txt.split("\n") if ln.strip()]
    assert rows[0] == "                   mean       std    median      5.0%     95.0%     n_eff     r_hat"
    assert [r.split()[0] for r in rows[1:11]] == ["mu", "tau"] + [f"theta_base[{i}]" for i in range(8)]
    assert len(rows) == 12 and "equal-tailed" in rows[11] and "not split" in rows[11] and "batch means" in rows[11]
    ref = SN.finalise(st, (0.05, 0.5, 0.95))
    mu = rows[1].split()
    assert mu[1] == f"{ref['mean'][0]:.2f}" and mu[3] == f"{ref['quantiles'][1, 0]:.2f}"
    assert len([ln for ln in m.summary_str(exclude_deterministic=False).split("\n") if ln.strip()]) == 20


def test_mcmc_summary_only_flat_potential_default_block(gpu):
    """A potential_fn kernel (no sites: the columns are z) with thinning and
    the default block and batch."""
    import posteriors as P
    from infer_amd import MCMC
    from kernels_amd import ARWMH, PRNGKey
    C, d = 96, 16
    g = P.correlated_gaussian(d)
    z0 = torch.zeros(C, d)
    m = MCMC(ARWMH(potential_fn=g, num_chains=C, device=gpu), num_warmup=100, num_samples=50, thinning=3)
    m.run(PRNGKey(2), init_params=z0, summary_only=True)
    s = m.streaming_summary
    assert (s.n_draws, s.num_cols, s.batch) == (16, d, 4)
    m2 = MCMC(ARWMH(potential_fn=g, num_chains=C, device=gpu), num_warmup=100, num_samples=50, thinning=3)
    m2.run(PRNGKey(2), init_params=z0)  # 16 draws fit one default block: the same single fused launch
    z = m2.get_samples(group_by_chain=True).cpu().numpy()  # [C, 16, d]
    st = SN.State(C, d, 4, 512, s.calib.cpu().numpy())
    SN.update(st, np.ascontiguousarray(z.transpose(1, 0, 2)))
    _same_bytes(s, st)
    rows = [ln for ln in m.summary_str().split("\n") if ln.strip()]
    assert len(rows) == 1 + d + 1 and rows[1].split()[0] == "Param:0[0]"


def test_block_past_two_to_the_31_elements(gpu):
    """64-bit indexing: a block of 2^31 + 2^22 elements (8.6 GB) whose last
    draw alone is random; every other draw is 0.25, so the expected state has
    a closed form (sums of 0.25 are exact in float64)."""
    from infer_amd import StreamingSummary
    C, k, B, nbins = 1 << 16, 64, 513, 64
    assert (B - 1) * C * k == 1 << 31
    x = torch.full((B, C, k), 0.25, dtype=torch.float32, device=gpu)
    last = np.random.default_rng(9).normal(size=(C, k)).astype(np.float32)
    x[B - 1].copy_(torch.as_tensor(last))
    s = StreamingSummary(C, k, batch=B, nbins=nbins, device=gpu).set_range([0.0] * k, [4.0] * k)
    s.update(x)
    del x
    l64 = last.astype(np.float64)
    S1 = (B - 1) * 0.25 + l64
    S2 = (B - 1) * 0.0625 + l64 * l64
    acc = s.acc.cpu().numpy()
    for got, want in zip(acc, (S1, S2, np.zeros_like(S1), S1, S1 * S1)):
        assert got.tobytes() == want.tobytes()
    cal = SN.calibration([0.0] * k, [4.0] * k, nbins)
    hist = np.zeros((k, nbins + 3), np.int64)
    hist[:, int(SN.bins(np.full((1, k), 0.25, np.float32), cal, nbins)[0, 0])] = (B - 1) * C
    b = SN.bins(last, cal, nbins)
    for j in range(k):
        hist[j] += np.bincount(b[:, j], minlength=nbins + 3)
    np.testing.assert_array_equal(s.hist.cpu().numpy(), hist)
