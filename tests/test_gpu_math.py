"""The device compile of include/amh_math.h (and of the row terms of
amh_device.h) against the host compile, bit for bit, function by function:
elementwise probe kernels (csrc/amh_probe.hip) against the C oracle on the
structured input sets of tests/math_cases.py -- every exponent with edge and
random mantissas, the subnormal band, +-0, +-inf, NaNs, and +-64 ulp around
every constant at which a function branches or rounds to an integer.

The rule, the same for every function: NaN in the same positions (payloads
are not part of the spec), every other output identical bits, the sign of zero
included.  Each test asserts the number of points it compared."""
import numpy as np
import pytest

import math_cases as mc
import math_probe

pytestmark = pytest.mark.gpu


def same_bits(name, dev_out, host_out, n_expected, inputs=None):
    """Asserts the rule; prints the point count, and on failure the function,
    the count and the first 16 (input bits, device bits, host bits)."""
    assert dev_out.shape == host_out.shape and dev_out.dtype == host_out.dtype, name
    assert dev_out.size == n_expected, f"{name}: compared {dev_out.size} points, expected {n_expected}"
    u = {4: np.uint32, 8: np.uint64}[dev_out.dtype.itemsize]
    db, hb = np.ascontiguousarray(dev_out).view(u), np.ascontiguousarray(host_out).view(u)
    if dev_out.dtype.kind == "f":
        nan_d, nan_h = np.isnan(dev_out), np.isnan(host_out)
        bad = (nan_d != nan_h) | (~nan_h & (db != hb))
    else:
        bad = db != hb
    nbad = int(bad.sum())
    print(f"{name}: {dev_out.size} points compared, {nbad} differ")
    if nbad:
        idx = np.flatnonzero(bad)[:16]
        ins = [] if inputs is None else [np.ascontiguousarray(a) for a in inputs]
        rows = []
        for i in idx:
            xin = " ".join(f"{int(a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])[i]):#x}" for a in ins)
            rows.append(f"  in {xin}  device {int(db[i]):#x}  host {int(hb[i]):#x}")
        pytest.fail(f"{name}: {nbad} of {dev_out.size} outputs differ between the device and the host compile\n"
                    + "\n".join(rows))


F2F_SETS = {
    "logf": mc.logf_cases, "expf": mc.expf_cases, "log1pf": mc.log1pf_cases, "log1p_sqf": mc.log1p_sq_cases,
    "log1p_sq3f": mc.log1p_sq_cases, "erfinvf": mc.erfinv_cases, "rsqrt_nr": mc.pivot_cases,
}


@pytest.mark.parametrize("name", sorted(F2F_SETS))
def test_float_functions(name, gpu, orc):
    x = F2F_SETS[name]()
    full = name not in ("erfinvf", "rsqrt_nr")  # those two have a stated domain (math_cases.py)
    assert x.size >= (mc.LATTICE_SIZE if full else 254 * 1032)
    same_bits(name, math_probe.device(gpu, name, x), orc.elementwise(name, x), x.size, [x])


def test_sincosf(gpu, orc):
    x = mc.sincos_cases()
    assert x.size >= 2 * 157 * 1032 and np.abs(x).max() == mc.SINCOS_MAX  # exponents 0..156 and 2^30 itself
    s, c = orc.elementwise("sincosf", x)
    same_bits("sincosf.sin", math_probe.device(gpu, "sin", x), s, x.size, [x])
    same_bits("sincosf.cos", math_probe.device(gpu, "cos", x), c, x.size, [x])


@pytest.mark.parametrize("name", ["pivot_ok", "isfinite", "isnan"])
def test_predicates(name, gpu, orc):
    x = mc.lattice32()
    host = orc.elementwise(name, x)
    ref = {"pivot_ok": (x >= np.float32(1.17549435e-38)) & np.isfinite(x), "isfinite": np.isfinite(x),
           "isnan": np.isnan(x)}[name]
    assert np.array_equal(host != 0, ref) and 0 < int(ref.sum()) < x.size
    same_bits(name, math_probe.device(gpu, name, x), host, mc.LATTICE_SIZE, [x])


def test_unif01(gpu, orc):
    """Only b >> 9 enters: the exhaustive set of the normals serves."""
    b = mc.normal_bits_cases()
    host = orc.elementwise("unif01", b)
    assert host.min() == 0.0 and host.max() == np.float32(1.0 - 2.0 ** -23)
    same_bits("unif01_from_bits", math_probe.device(gpu, "unif01", b), host, mc.NORMAL_BITS_SIZE, [b])


def test_normal_from_bits_exhaustive(gpu, orc):
    """Every one of the 2^23 distinct draws, and the batched form of the pooled
    d > 64 kernel (amh_normal_head + amh_erfinv_tail) against the same values."""
    b = mc.normal_bits_cases()
    host = orc.normal_from_bits(b)
    assert np.isfinite(host).all()
    same_bits("normal_from_bits", math_probe.device(gpu, "normal_from_bits", b), host, mc.NORMAL_BITS_SIZE, [b])
    same_bits("normal_split", math_probe.device(gpu, "normal_split", b), host, mc.NORMAL_BITS_SIZE, [b])


@pytest.mark.parametrize("name,ys", [("logistic_term", mc.LOGISTIC_Y), ("poisson_term", mc.POISSON_Y)])
def test_glm_row_terms(name, ys, gpu, orc):
    eta, y = mc.with_y(mc.eta_cases(), ys)
    n = len(ys) * (mc.LATTICE_SIZE + (1 << 16) + 1)
    same_bits(name, math_probe.device(gpu, name, eta, y), orc.elementwise(name, eta, y), n, [eta, y])


@pytest.mark.parametrize("which", [0, 1])
def test_lp_student3(which, gpu, orc):
    """x from the lattice reaches the 1.8e19 switch of amh_log1p_sq3f through
    (x - loc) / scale."""
    x = mc.lattice32()
    name = ("lp_student3_intercept", "lp_student3_sigma")[which]
    host = orc.elementwise("lp_student3", x, *mc.STUDENT3_TRIPLES[which])
    same_bits(name, math_probe.device(gpu, name, x), host, mc.LATTICE_SIZE, [x])


@pytest.mark.parametrize("a", mc.LR_DECAYS)
def test_lr_gamma(a, gpu, orc):
    n = mc.gamma_n_cases()
    got = math_probe.device(gpu, "lr_gamma", n, a=a)
    assert n[0] == 1 and got[0] == np.float32(1.0)  # gamma_1 = 1 exactly
    same_bits(f"lr_gamma a = {a:.6g}", got, orc.lr_gamma(n, a), mc.GAMMA_N_SIZE, [n])


def test_log_d_exp_d(gpu, orc):
    x = mc.log_d_cases()
    host = orc.elementwise("log_d", x)
    same_bits("log_d", math_probe.device(gpu, "log_d", x), host, mc.GAMMA_N_SIZE, [x])
    xe = mc.exp_d_cases(host)
    same_bits("exp_d", math_probe.device(gpu, "exp_d", xe), orc.elementwise("exp_d", xe), mc.EXP_D_SIZE, [xe])
