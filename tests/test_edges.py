"""The edge scenarios of tests/test_gpu_edges.py on the CPU: they reach the
edges (reach conditions, asserted on the C oracle alone so a later edit cannot
turn the scenarios benign), and the oracle is right there (float64 anchors:
a wrong oracle matched by a kernel that is wrong the same way is the hole the
bit-exact design cannot see).  Plus the stand-alone sanitizer run of the
oracle's steps from hostile states (oracle/edge_ubsan.c)."""
import os
import subprocess

import numpy as np
import pytest

import arwmh_np as lit
import asss_np as alit
from helpers import (EDGE_MATRIX, HOSTILE_WARMUP, edge_init, edge_points, hostile_adapt, log_scale_coords, make_edge_case)
from test_oracle import lit_potential, unpack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 160


def _base(kind):
    return kind.replace("_n77", "")


# ------------------------------------------------------- reach conditions ----
@pytest.mark.parametrize("kind,d", EDGE_MATRIX)
def test_edge_points_reach(kind, d, orc):
    """Every model sees at least one NaN, one +inf and >= 60 % finite potentials."""
    _, _, om = make_edge_case(kind, d)
    _, z = edge_points(om.d, 11, log_scale_coords(_base(kind), om.d))
    pe = orc.potential(om, z)
    assert np.isnan(pe).any() and np.isposinf(pe).any()
    assert np.isfinite(pe).mean() >= 0.6, np.isfinite(pe).mean()
    for c in log_scale_coords(_base(kind), om.d):  # every value reaches the log-scale coordinate
        col = z[:, c]
        for v in (87.0, 88.8, 89.0, -104.0, 1e19, np.inf):
            assert (col == np.float32(v)).any(), (c, v)
        assert np.isnan(col).any()


@pytest.mark.parametrize("kind", ["eight_schools", "kidiq"])
def test_wild_starts_reach(kind, orc):
    """The log-scale models have chains whose initial potential is non-finite."""
    _, _, om, ost, _ = edge_init(kind, None, C, orc, start="wild")
    assert (~np.isfinite(ost.potential_energy)).sum() >= 1


@pytest.mark.parametrize("algo", ["arwmh", "asss"])
@pytest.mark.parametrize("kind,d", EDGE_MATRIX)
def test_hostile_adapt_reach(kind, d, algo, orc):
    """hostile_adapt over 12 single steps: the factor is bit-unchanged in
    10-90 % of chain-steps, a chain ends with a non-finite factor entry, and
    at least 25 % of the chains moved.  (With num_warmup = 0 the d = 1 models
    kept the factor in only 9.8 % of chain-steps; HOSTILE_WARMUP = 8 widens the
    scenario by the warmup reset, one gamma = 1 step from hostile values.)"""
    _, _, om, ost, _ = edge_init(kind, d, C, orc)
    step = (lambda n: orc.asss_step(om, ost, n, num_warmup=HOSTILE_WARMUP)) if algo == "asss" else \
        (lambda n: orc.step(om, ost, n, num_warmup=HOSTILE_WARMUP))
    step(5)
    hostile_adapt(ost, step_size=algo == "arwmh")
    z0 = ost.z.copy()
    kept = 0
    for _ in range(12):
        L0 = ost.scale.copy()
        step(1)
        kept += int((L0.view(np.uint32) == ost.scale.view(np.uint32)).all(1).sum())
    frac = kept / (12 * C)
    assert 0.1 <= frac <= 0.9, frac
    assert (~np.isfinite(ost.scale)).any()
    assert (ost.z.view(np.uint32) != z0.view(np.uint32)).any(1).mean() >= 0.25


# ------------------------------------------------------- potential anchor ----
# measured max |U_oracle - U_float64| / max(|U_float64|, 1) on the anchor rows
# (edge_points(d, 11)); the test asserts 4x these
MEASURED_POTENTIAL_REL = {
    ("gaussian", 1): 5.9e-8, ("gaussian", 5): 1.7e-7, ("gaussian", 33): 2.3e-7, ("gaussian", 64): 2.5e-7,
    ("gaussian", 72): 3.7e-7, ("gaussian", 100): 7.9e-7, ("gaussian", 128): 5.5e-7, ("gaussian", 256): 1.1e-6,
    ("eight_schools", None): 1.7e-7, ("kidiq", None): 3.2e-7, ("diamonds", None): 2.7e-7,
    ("diamonds_n77", None): 2.1e-7, ("diamonds_ss", None): 2.8e-7, ("mixture", 1): 6.2e-8, ("mixture", 3): 1.2e-7,
    ("logistic", 8): 1.6e-7, ("logistic", 32): 1.6e-7, ("logistic_n77", 8): 1.9e-7, ("logistic_n77", 32): 1.4e-7,
    # Poisson: e^eta carries eta's absolute error as a relative one, and the anchor rows reach |eta| ~ 60
    # (a coefficient of +-200 on columns of scale 1/16): (K + 2) |eta| 2^-24 is 4e-5 at K = 8
    ("poisson", 9): 3.5e-6, ("poisson", 32): 7.9e-6, ("poisson_n77", 9): 2.0e-6, ("poisson_n77", 32): 7.8e-6,
}


def _poisson_eta_out_of_range(om, z):
    """Rows of z at which some eta_n = I + X_n b + o_n, evaluated in float64 on
    the float32 data, lies past log(FLT_MAX) = 88.72, where amh_expf returns
    +inf (then U is +inf, or inf - inf = NaN once y_n eta_n overflows too), or
    at which |y_n eta_n| itself is past float32's range (eta_n very negative)."""
    N, K = om.n_data, om.k_data
    raw = np.asarray(om.data, np.float64)
    X, y, o = raw[:N * K].reshape(N, K), raw[N * K:N * K + N], raw[N * K + N:N * K + 2 * N]
    z = z.astype(np.float64)
    with np.errstate(all="ignore"):
        eta = z[:, :1] + z[:, 1:] @ X.T + o
        return ~(eta.max(1) <= 88.72) | ~(np.abs(y * eta).max(1) <= 3.4e38)


@pytest.mark.parametrize("kind,d", EDGE_MATRIX)
def test_potential_anchor(kind, d, orc):
    """orc.potential against the float64 literal potentials (oracle/arwmh_np.py)
    at the edge_points rows whose float64 value is finite and below 1e30 and
    whose log-scale coordinates stay within +-88.  The bound is 4x the largest
    relative error measured per model (relative to max(|U|, 1): several
    potentials cross zero), MEASURED_POTENTIAL_REL above: 6e-8 (d = 1) to
    1.1e-6 (Gaussian d = 256), i.e. a few float32 roundings of the largest
    term -- far below a wrong or missing term.

    Conversely the oracle is non-finite only where the input is non-finite, a
    log-scale coordinate exceeds 88 in magnitude, or the float64 value exceeds
    1e37.  (Before amh_log1p_sqf this failed for kidiq and diamonds at
    log sigma = 87: the half-Cauchy / Student-t prior squared sigma / s in
    float32, +inf from sigma ~ 4e19 on, where U is about N log sigma.)
    Poisson exponentiates every row's eta, not a coordinate: there the oracle
    may also be non-finite where a float64 eta_n is past amh_expf's range
    (_poisson_eta_out_of_range).  On these rows the clause adds nothing to the
    1e37 rule (e^88.72 alone is 3.4e38), which the test asserts."""
    _, _, om = make_edge_case(kind, d)
    lc = log_scale_coords(_base(kind), om.d)
    _, z = edge_points(om.d, 11, lc)
    pe = orc.potential(om, z)
    U = lit_potential(_base(kind), om)
    with np.errstate(all="ignore"):
        ul = np.array([float(U(r.astype(np.float64))) for r in z])
    infin = np.isfinite(z).all(1)
    logbig = np.zeros(len(z), bool)
    for c in lc:
        logbig |= np.abs(z[:, c]) > 88
    with np.errstate(invalid="ignore"):
        use = np.isfinite(ul) & (np.abs(ul) < 1e30) & ~logbig & infin
        allowed = ~infin | logbig | ~(np.abs(ul) <= 1e37)
    if _base(kind) == "poisson":
        eta_out = _poisson_eta_out_of_range(om, z) & infin
        assert not (eta_out & ~allowed).any()
        allowed |= eta_out
    assert use.sum() >= 0.5 * len(z)
    fin = np.isfinite(pe)
    finding = ~fin & ~allowed
    assert not finding.any(), (z[finding], pe[finding], ul[finding])
    assert fin[use].all()
    rel = np.abs(pe[use].astype(np.float64) - ul[use]) / np.maximum(np.abs(ul[use]), 1.0)
    print(f"{kind} {d}: {use.sum()} anchor rows, max rel {rel.max():.3e}")
    assert rel.max() <= 4 * MEASURED_POTENTIAL_REL[(kind, d)], rel.max()


# ------------------------------------------------------------ step anchor ----
def _cls(a):
    """0 finite, 1 +inf, 2 -inf, 3 NaN, elementwise."""
    a = np.asarray(a, np.float64)
    return np.where(np.isnan(a), 3, np.where(np.isposinf(a), 1, np.where(np.isneginf(a), 2, 0)))


def _tril(L, d):
    return np.concatenate([L[j:, j] for j in range(d)])


def _leaf_overflow(leaves):
    """The float64 literal is finite in every leaf and one is past float32's
    range (magnitude above 1e37)."""
    flat = np.concatenate([np.atleast_1d(np.asarray(x, np.float64)).ravel() for x in leaves])
    return bool(np.isfinite(flat).all() and (np.abs(flat) > 1e37).any())


# the step anchors' scenario: hostile_adapt with its top ends shrunk.  With the
# full cycles 49 (ARWMH) and 56 (ASSS) of the 160 chains had a finite float64
# leaf past 1e37, above the 25 % cap, and shrinking the factor scales alone
# (1e8 .. 1e25 -> 1e4 .. 1e15) left 47 and 64: the leaves past 1e37 are
# as_change ~ L e^lambda at lambda = 88 / 89 (and 45 next to loc = 1e19) and the
# ASSS potential ~ (1e19)^2 of the upper half.  So the step sizes stop at 45
# and loc moves by 1e17 here; no chain is ignored then.
ANCHOR_FACTORS = (1e-30, 1e-20, 1e-8, 1.0, 1e4, 1e8, 1e12, 1e15)
ANCHOR_STEP_SIZES = (-110.0, -90.0, -20.0, 0.0, 20.0, 30.0, 40.0, 45.0)
ANCHOR_LOC_SHIFT = 1e17


def _hostile_d8(orc, algo):
    _, _, om, ost, _ = edge_init("gaussian", 8, C, orc)
    if algo == "asss":
        orc.asss_step(om, ost, 5, num_warmup=HOSTILE_WARMUP)
    else:
        orc.step(om, ost, 5, num_warmup=HOSTILE_WARMUP)
    hostile_adapt(ost, step_size=algo == "arwmh", factors=ANCHOR_FACTORS, step_sizes=ANCHOR_STEP_SIZES,
                  loc_shift=ANCHOR_LOC_SHIFT)
    return om, ost


def _signature(decisions, leaves):
    return tuple(decisions) + tuple(_cls(x).tobytes() for x in leaves)


def _anchor(C_, per_chain):
    """per_chain(c) -> None (skip) or (oracle signature, literal signature at
    float64, literal signature at float32, float64 literal leaves).  The
    oracle must carry the float64 literal's decisions and classes wherever the
    literal gives the same ones in float64 and in float32 ("in range"); where
    the two literals part, float32's range decides the step (an intermediate
    such as delta^2 ~ 1e38, the scan b ~ gamma w^2 / (L_jj)^2 or a squared pivot
    below 1e-38 over- or underflows) and the oracle must carry the float32
    literal's, the reference's own dtype.  Only chains whose float64 literal
    has a finite leaf past 1e37 are ignored, at most 25 %; a chain whose
    accept decision lies within 1e-4 of its uniform (per_chain returns None)
    is not compared either, at most 2 of them."""
    n = {"ignored": 0, "in range": 0, "float32 range": 0, "at the threshold": 0}
    bad = []
    for c in range(C_):
        r = per_chain(c)
        if r is None:
            n["at the threshold"] += 1
            continue
        got, want64, want32, leaves64 = r
        if _leaf_overflow(leaves64):
            n["ignored"] += 1
            continue
        kind = "in range" if want64 == want32 else "float32 range"
        n[kind] += 1
        if got != want32:
            bad.append((c, kind, [i for i, (a, b) in enumerate(zip(got, want32)) if a != b]))
    return n, bad


def test_arwmh_step_anchor(orc):
    """One oracle ARWMH step from hostile_adapt states of the d = 8 Gaussian
    against arwmh_np.sample fed the oracle's noise: per chain the accept
    decision, the keep-L decision and the finite / +inf / -inf / NaN class of
    every state leaf (z, pe, mean_accept_prob, loc, scale, log_step_size,
    as_change), by the rule of _anchor.  Measured: 65 chains in range, 95
    decided by float32's range, none ignored or at the threshold (ASSS: 112
    and 48); every one of the 160 agrees with the float32 literal."""
    om, st = _hostile_d8(orc, "arwmh")
    d = om.d
    before = st.copy()
    acc = np.zeros(C, np.int32)
    orc.step(om, st, 1, num_warmup=HOSTILE_WARMUP, accept_count=acc)
    U = lit_potential("gaussian", om)
    bits, ubits = lit.step_noise(before.rng_key, before.i, d)

    def per_chain(c):
        xi = lit.normal_from_bits(bits[c])
        u = float(lit.unif01_from_bits(ubits[c]))
        L0 = unpack(before.scale[c], d)
        s0 = lit.ARWMHState(int(before.i[c]), before.z[c].astype(np.float64), float(before.potential_energy[c]),
                            float(before.mean_accept_prob[c]),
                            lit.ARWMHAdaptState(before.loc[c].astype(np.float64), L0, float(before.log_step_size[c])),
                            0.0, None)
        sigs = []
        for dt in (np.float64, np.float32):
            new, accepted, alpha = lit.sample(s0, U, xi, u, num_warmup=HOSTILE_WARMUP, dtype=dt)
            if abs(u - float(alpha)) < 1e-4:
                return None  # decision within rounding of the threshold
            a = new.adapt_state
            leaves = [new.z, new.potential_energy, new.mean_accept_prob, a.loc, _tril(np.asarray(a.scale), d),
                      a.log_step_size, new.as_change]
            kept = np.array_equal(np.asarray(a.scale, np.float64), L0)
            sigs.append((_signature((bool(accepted), kept), leaves), leaves))
        kept_orc = np.array_equal(st.scale[c].view(np.uint32), before.scale[c].view(np.uint32))
        got = _signature((bool(acc[c]), kept_orc),
                         [st.z[c], st.potential_energy[c], st.mean_accept_prob[c], st.loc[c], st.scale[c],
                          st.log_step_size[c], st.as_change[c]])
        return got, sigs[0][0], sigs[1][0], sigs[0][1]

    n, bad = _anchor(C, per_chain)
    print(f"arwmh step anchor: {n}")
    assert not bad, (len(bad), bad[:8])
    assert n["ignored"] <= C // 4 and n["at the threshold"] <= 2, n
    assert n["in range"] >= C // 4, n


def test_asss_step_anchor(orc):
    """The same for one ASSS step (asss_np.sample, the oracle's draws), by the
    rule of _anchor; there is no accept decision: keep-L and the class of
    every leaf (z, pe, loc, scale, as_change).  asss_np evaluates every
    statement in the selected dtype, so the chains decided by float32's range
    -- |y|^2 of the whitened start past 2^24, where 1 - z_d = 2 / (|y|^2 + 1)
    is below float32's spacing at 1 and the reference's own (ns - 1) /
    (ns + 1), z / (1 - z_d) (asss.py:40-56) lose x; squared pivots below
    1e-38 -- are compared with the float32 literal, not dropped.  On the
    collapsed-factor chains of the lower half the values are compared too:
    the transition lands next to mu, not at x, in the oracle exactly as in the
    float32 literal."""
    om, st = _hostile_d8(orc, "asss")
    d = om.d
    before = st.copy()
    orc.asss_step(om, st, 1, num_warmup=HOSTILE_WARMUP)
    U = lit_potential("gaussian", om)

    def per_chain(c):
        v, ut, th0, uks = alit.draws(before.rng_key[c], int(before.i[c]), d)
        L0 = unpack(before.scale[c], d)
        s0 = alit.ASSSState(int(before.i[c]), before.z[c].astype(np.float64), float(before.potential_energy[c]),
                            alit.ASSSAdaptState(before.loc[c].astype(np.float64), L0), 0.0, None)
        sigs = []
        for dt in (np.float64, np.float32):
            with np.errstate(all="ignore"):
                new, _ = alit.sample(s0, lambda x: U(np.asarray(x, np.float64)), v, ut, th0, uks,
                                     num_warmup=HOSTILE_WARMUP, dtype=dt)
            a = new.adapt_state
            leaves = [new.z, new.potential_energy, a.loc, _tril(np.asarray(a.scale), d), new.as_change]
            kept = np.array_equal(np.asarray(a.scale, np.float64), L0)
            sigs.append((_signature((kept,), leaves), leaves))
        with np.errstate(all="ignore"):
            y = np.linalg.solve((L0 + 1e-6 * np.eye(d)) * np.sqrt(d), s0.z - s0.adapt_state.loc)
        if c < C // 2 and y @ y > 2.0 ** 24:  # collapsed factor, finite mean: the sphere cannot resolve x
            collapsed.append((c, float(np.abs(st.z[c] - sigs[1][1][0]).max()),
                              float(np.abs(st.z[c] - before.loc[c]).max()),
                              float(np.abs(before.z[c] - before.loc[c]).max())))
        kept_orc = np.array_equal(st.scale[c].view(np.uint32), before.scale[c].view(np.uint32))
        got = _signature((kept_orc,), [st.z[c], st.potential_energy[c], st.loc[c], st.scale[c], st.as_change[c]])
        return got, sigs[0][0], sigs[1][0], sigs[0][1]

    collapsed = []
    n, bad = _anchor(C, per_chain)
    print(f"asss step anchor: {n}; {len(collapsed)} collapsed-factor chains")
    assert not bad, (len(bad), bad[:8])
    # values, not only classes, where float32 loses x on the sphere: the oracle's x' is the float32
    # literal's (measured: equal) and sits within 1e-4 of mu (measured: < 4e-5), x having been 0.04 - 1.8 away
    assert len(collapsed) >= C // 8
    for c, d_lit, d_mu, d_x in collapsed:
        assert d_lit <= 1e-6 and d_mu <= 1e-4 < d_x, (c, d_lit, d_mu, d_x)
    assert n["ignored"] <= C // 4 and n["at the threshold"] <= 2, n
    assert n["in range"] >= C // 4, n


# -------------------------------------------- host undefined-behaviour run ----
def test_oracle_edge_steps_under_sanitizers():
    """oracle/edge_ubsan.c (own main, no Python): 12 ARWMH and 12 ASSS oracle
    steps of a d = 8 and a d = 100 Gaussian, a d = 8 logistic and a d = 32
    Poisson regression (N = 77) from hostile_adapt states, built
    with -fsanitize=address,undefined,float-cast-overflow and no recovery; a
    report (an out-of-range float -> int cast, say) would mark a point where
    host and device may legitimately differ.  Exit status 0 expected."""
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "edge_ubsan"], check=True)
    r = subprocess.run([os.path.join(ROOT, "oracle", "build", "edge_ubsan")], capture_output=True, text=True,
                       timeout=300)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, tail
