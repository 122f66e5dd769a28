"""The noise stream and elementary functions of include/amh_math.h, pinned
independently: Random123 known-answer vectors for Philox4x32-10, numpy/scipy
float64 references for log/exp/log1p/erfinv and the learning-rate schedule."""
import numpy as np
import pytest
from scipy import stats
from scipy.special import erfinv

import arwmh_np as lit

# Random123 kat_vectors, philox4x32 R=10
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def ulp_err(y, ref):
    sp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return np.abs(y.astype(np.float64) - ref) / sp


def test_philox_kat_c(orc):
    ctr = np.array([k[0] for k in KAT], np.uint32)
    key = np.array([k[1] for k in KAT], np.uint32)
    out = orc.philox(ctr, key)
    np.testing.assert_array_equal(out, np.array([k[2] for k in KAT], np.uint32))


def test_philox_kat_numpy_and_product():
    from kernels_amd import random as krandom
    for ctr, key, exp in KAT:
        o = lit.philox4x32_10(*[np.uint32(c) for c in ctr], np.uint32(key[0]), np.uint32(key[1]))
        assert tuple(int(v) for v in o) == exp
        a, b = krandom._philox(*[np.uint32(c) for c in ctr], key[0], key[1])
        assert (int(a), int(b)) == exp[:2]


def test_philox_c_equals_numpy(orc):
    rng = np.random.default_rng(0)
    ctr = rng.integers(0, 2 ** 32, size=(5000, 4), dtype=np.uint64).astype(np.uint32)
    key = rng.integers(0, 2 ** 32, size=(5000, 2), dtype=np.uint64).astype(np.uint32)
    c = orc.philox(ctr, key)
    n = np.stack(lit.philox4x32_10(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], key[:, 0], key[:, 1]), axis=1)
    np.testing.assert_array_equal(c, n)


def test_logf(orc):
    x = np.exp(np.random.default_rng(0).uniform(-87, 88, 300000)).astype(np.float32)
    assert ulp_err(orc.elementwise("logf", x), np.log(x.astype(np.float64))).max() <= 1.0
    sp = np.array([0.0, -0.0, -1.0, np.inf, np.nan, 1.0, 1e-45], np.float32)
    y = orc.elementwise("logf", sp)
    assert y[0] == -np.inf and y[1] == -np.inf and np.isnan(y[2]) and y[3] == np.inf and np.isnan(y[4])
    assert y[5] == 0.0 and abs(y[6] - np.log(np.float64(np.float32(1e-45)))) < 1e-3


def test_expf(orc):
    x = np.random.default_rng(1).uniform(-87, 88.7, 300000).astype(np.float32)
    assert ulp_err(orc.elementwise("expf", x), np.exp(x.astype(np.float64))).max() <= 1.5
    sp = np.array([np.inf, -np.inf, np.nan, 0.0, 100.0, -120.0], np.float32)
    y = orc.elementwise("expf", sp)
    assert y[0] == np.inf and y[1] == 0 and np.isnan(y[2]) and y[3] == 1.0 and y[4] == np.inf and y[5] == 0


def test_log1pf(orc):
    x = np.random.default_rng(2).uniform(-0.999, 1e4, 300000).astype(np.float32)
    assert ulp_err(orc.elementwise("log1pf", x), np.log1p(x.astype(np.float64))).max() <= 3.0


def test_erfinv(orc):
    x = np.random.default_rng(3).uniform(-0.9999999, 0.9999999, 300000).astype(np.float32)
    y = orc.elementwise("erfinvf", x)
    r = erfinv(x.astype(np.float64))
    assert np.max(np.abs(y - r) / np.maximum(np.abs(r), 1e-30)) < 1e-6


def test_normal_stream(orc):
    b = np.random.default_rng(5).integers(0, 2 ** 32, 2_000_000, dtype=np.uint64).astype(np.uint32)
    z = orc.normal_from_bits(b)
    zr = lit.normal_from_bits(b)  # float64 erfinv of the same uniforms
    assert np.max(np.abs(z - zr)) < 2e-6 * 5
    assert abs(z.mean()) < 3e-3 and abs(z.std() - 1) < 3e-3
    assert stats.kstest(z[:200000].astype(np.float64), "norm").pvalue > 1e-3
    u = lit.unif01_from_bits(b)
    assert u.min() >= 0.0 and u.max() < 1.0


@pytest.mark.parametrize("a", [2 / 3, 0.5, 1.0])
def test_lr_gamma(orc, a):
    n = np.arange(1, 2_000_001, dtype=np.int32)
    g = orc.lr_gamma(n, a)
    assert g[0] == 1.0  # gamma_1 = 1 exactly: the keep-L quirk at n = 1 depends on it
    ref = 1.0 / n.astype(np.float64) ** np.float64(np.float32(a))
    assert ulp_err(g, ref).max() <= 1.5


# ---------------------------------------------------------------------------
# The rest of the header, host compile against float64 (input sets:
# tests/math_cases.py).  Every test prints its measured maximum beside the bound.
import math_cases as mc  # noqa: E402


def _report(what, got, bound):
    print(f"{what}: measured {got:.4g}, bound {bound:.4g}")


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("name,div,bound", [("log1p_sqf", 1.0, 4.0), ("log1p_sq3f", 3.0, 5.0)])
def test_log1p_sq_below_the_switch(orc, name, div, bound):
    """|t| <= 1.8e19: the bits of amh_log1pf of the float32 argument (the
    header's claim), and within test_log1pf's 3 ulp plus one ulp per float32
    rounding of that argument (t * t; the division by 3) of float64 log1p."""
    t = mc.log1p_sq_cases()
    t = t[np.abs(t) <= mc.LOG1P_SQ_SWITCH]  # NaN and inf drop out
    assert t.size > 390_000
    arg = t * t if div == 1.0 else (t * t) / np.float32(3.0)
    assert arg.dtype == np.float32
    y = orc.elementwise(name, t)
    assert _bits_equal(y, orc.elementwise("log1pf", arg))
    t64 = t.astype(np.float64)
    err = ulp_err(y, np.log1p(t64 * t64 / div)).max()
    _report(f"{name} |t| <= 1.8e19, ulp", err, bound)
    assert err <= bound


@pytest.mark.parametrize("name,div", [("log1p_sqf", 1.0), ("log1p_sq3f", 3.0)])
def test_log1p_sq_above_the_switch(orc, name, div):
    """Past 1.8e19: 2 log|t| (- log 3) within 2 ulp of float64 log1p (amh_logf's
    1 ulp doubled exactly, plus sq3's fmaf rounding), finite for every finite t,
    and no step of more than 2 ulp across the switch."""
    t = mc.log1p_sq_cases()
    fin = t[np.isfinite(t)]
    assert np.isfinite(orc.elementwise(name, fin)).all()
    t = fin[np.abs(fin) > mc.LOG1P_SQ_SWITCH]
    assert t.size > 60_000
    t64 = t.astype(np.float64)
    err = ulp_err(orc.elementwise(name, t), np.log1p(t64 * t64 / div)).max()
    _report(f"{name} |t| > 1.8e19, ulp", err, 2.0)
    assert err <= 2.0
    a = mc.LOG1P_SQ_SWITCH  # the last value of the plain form; the next one takes 2 log|t|
    pair = np.array([a, np.nextafter(a, np.float32(np.inf)), -a, np.nextafter(-a, np.float32(-np.inf))], np.float32)
    y = orc.elementwise(name, pair).astype(np.float64)
    step = max(abs(y[1] - y[0]), abs(y[3] - y[2])) / np.spacing(np.float32(y[0]))
    _report(f"{name} step across the switch, ulp", step, 2.0)
    assert step <= 2.0


@pytest.mark.parametrize("span", [2 * np.pi, 1e5])
def test_sincosf(orc, span):
    """|s - sin x|, |c - cos x| <= 2^-22 (two float32 roundings at 1.0) and
    |s^2 + c^2 - 1| <= 2^-21 on |x| <= 2 pi (the ASSS range) and on |x| <= 1e5;
    a wrong coefficient, reduction constant or quadrant gives 1e-5 or more."""
    x = np.random.default_rng(int(span)).uniform(-span, span, 2_000_000).astype(np.float32)
    x = np.concatenate([x, mc.sincos_edges()])
    x = x[np.abs(x) <= np.float32(span)] if span < 10 else x
    assert x.size >= 2_000_000
    s, c = orc.elementwise("sincosf", x)
    x64, s64, c64 = x.astype(np.float64), s.astype(np.float64), c.astype(np.float64)
    es, ec = np.abs(s64 - np.sin(x64)).max(), np.abs(c64 - np.cos(x64)).max()
    en = np.abs(s64 * s64 + c64 * c64 - 1.0).max()
    _report(f"sincosf |x| <= {span:.6g}: |s - sin|", es, 2.0 ** -22)
    _report(f"sincosf |x| <= {span:.6g}: |c - cos|", ec, 2.0 ** -22)
    _report(f"sincosf |x| <= {span:.6g}: |s^2 + c^2 - 1|", en, 2.0 ** -21)
    assert es <= 2.0 ** -22 and ec <= 2.0 ** -22
    assert en <= 2.0 ** -21


def test_rsqrt_nr(orc):
    """Relative error <= 4 x 2^-23 of float64 1 / sqrt(x) on every lattice value
    amh_pivot_ok accepts (three Newton steps leave 3e-11; the rest is the five
    roundings of the last step), and L_kk = x * y within 4 ulp of sqrt(x)."""
    x = mc.pivot_cases()
    assert x.size == 254 * 1032  # positive, biased exponents 1..254
    ok = orc.elementwise("pivot_ok", mc.lattice32())
    lat = mc.lattice32()
    assert np.array_equal(ok != 0, (lat >= np.float32(1.17549435e-38)) & np.isfinite(lat))
    y = orc.elementwise("rsqrt_nr", x)
    x64 = x.astype(np.float64)
    rel = (np.abs(y.astype(np.float64) * np.sqrt(x64) - 1.0)).max()
    _report("rsqrt_nr relative error", rel, 4 * 2.0 ** -23)
    assert rel <= 4 * 2.0 ** -23
    lkk = ulp_err(x * y, np.sqrt(x64)).max()
    _report("x * rsqrt_nr(x) against sqrt(x), ulp", lkk, 4.0)
    assert lkk <= 4.0


def test_expf_subnormal_results(orc):
    """x in [-103.97, -87.34], where the result is subnormal: one rounding of a
    subnormal, |error| <= 2^-149; and non-decreasing across the edge of the band."""
    x = np.random.default_rng(11).uniform(-103.97, -87.34, 1_000_000).astype(np.float32)
    e = mc.expf_cases()
    x = np.concatenate([x, e[(e >= np.float32(-103.97)) & (e <= np.float32(-87.34))]])
    assert x.size > 1_000_000
    y = orc.elementwise("expf", x)
    assert (y < np.float32(1.17549435e-38)).mean() > 0.99 and (y > 0).any()
    err = np.abs(y.astype(np.float64) - np.exp(x.astype(np.float64))).max() / 2.0 ** -149
    _report("expf subnormal results, |error| / 2^-149", err, 1.0)
    assert err <= 1.0
    edge = mc.expf_subnormal_edge()
    assert edge.size == 2 * mc.NBHD + 1 and (np.diff(edge) > 0).all()
    ye = orc.elementwise("expf", edge)
    assert ye[0] < np.float32(1.17549435e-38) < ye[-1]  # the set straddles the edge
    drop = float(-np.diff(ye.astype(np.float64)).min())
    _report("expf largest decrease over the sorted edge set", max(drop, 0.0), 0.0)
    assert drop <= 0.0


def test_logf_subnormal_inputs(orc):
    b = np.random.default_rng(12).integers(1, 1 << 23, 1_000_000, dtype=np.uint32)
    x = mc.f32(b)
    assert (x > 0).all() and (x < np.float32(1.17549435e-38)).all()
    err = ulp_err(orc.elementwise("logf", x), np.log(x.astype(np.float64))).max()
    _report("logf on subnormal inputs, ulp", err, 1.0)
    assert err <= 1.0


def _same(what, got, ref, n_expected):
    """NaN in the same places, every other value bit for bit."""
    assert got.size == ref.size == n_expected, (what, got.size, ref.size, n_expected)
    u = np.uint64 if got.dtype.itemsize == 8 else np.uint32
    nan_g, nan_r = np.isnan(got), np.isnan(ref)
    bad = (nan_g != nan_r) | (~nan_r & (got.view(u) != ref.view(u)))
    print(f"{what}: {got.size} points, {int(bad.sum())} differ")
    assert not bad.any(), (what, int(bad.sum()), np.flatnonzero(bad)[:16])


def test_three_compiles_agree(orc):
    """hipcc's host clang compile of the header (it fills the gamma table in
    amh_create) against the oracle's gcc compile, bit for bit, on the lr_gamma,
    log_d, exp_d, expf and logf sets.  Needs the probe library, not a device."""
    import math_probe
    n = mc.gamma_n_cases()
    for a in mc.LR_DECAYS:
        g = math_probe.host("lr_gamma", n, a)
        assert g[0] == 1.0
        _same(f"lr_gamma a = {a:.6g}", g, orc.lr_gamma(n, a), mc.GAMMA_N_SIZE)
    ld = orc.elementwise("log_d", mc.log_d_cases())
    _same("log_d", math_probe.host("log_d", mc.log_d_cases()), ld, mc.GAMMA_N_SIZE)
    xe = mc.exp_d_cases(ld)
    _same("exp_d", math_probe.host("exp_d", xe), orc.elementwise("exp_d", xe), mc.EXP_D_SIZE)
    for name, x in (("expf", mc.expf_cases()), ("logf", mc.logf_cases())):
        _same(name, math_probe.host(name, x), orc.elementwise(name, x), x.size)
