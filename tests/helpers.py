"""Shared test helpers: the same model in product form (posteriors) and in
oracle form (oracle/orc.py), built from the same packed float32 data."""
from __future__ import annotations

import numpy as np


def make_case(kind: str, d: int = None):
    """-> (product kwargs for ARWMH, model_kwargs, orc.Model)"""
    import orc
    import posteriors as P
    if kind == "gaussian":
        g = P.correlated_gaussian(d or 64)
        data, _ = g.pack("cpu")
        return dict(potential_fn=g), {}, orc.Model(orc.GAUSSIAN, g.dim, data.numpy())
    if kind == "eight_schools":
        mk = dict(P.EIGHT_SCHOOLS_DATA)
        arr, ip = P.eight_schools.pack_fn(mk)
        return dict(model=P.eight_schools), mk, orc.Model(orc.EIGHT_SCHOOLS, ip[0] + 2, arr)
    if kind == "kidiq":
        mk = P.synthetic_kidiq()
        arr, ip = P.kidiq.pack_fn(mk)
        return dict(model=P.kidiq), mk, orc.Model(orc.KIDIQ, 4, arr, n_data=ip[0])
    if kind == "diamonds":
        mk = P.synthetic_diamonds(N=500)
        arr, ip = P.diamonds.pack_fn(mk)
        N, K = ip
        return dict(model=P.diamonds), mk, orc.Model(orc.DIAMONDS, K + 1, arr, n_data=N, k_data=K)
    if kind == "diamonds_ss":
        mk = P.synthetic_diamonds(N=500)
        arr, ip = P.diamonds_suffstat.pack_fn(mk)
        N, K = ip
        return dict(model=P.diamonds_suffstat), mk, orc.Model(orc.DIAMONDS_SS, K + 1, arr, n_data=N, k_data=K)
    if kind == "mixture":  # asumptions_check.ipynb cell 61, on every coordinate
        mx = P.notebook_mixture() if (d or 1) == 1 else P.mixture([0.5, 0.5], [-1.0, 1.0], [0.1, 0.1], dim=d)
        data, ip = mx.pack("cpu")
        return dict(potential_fn=mx), {}, orc.Model(orc.MIXTURE, mx.dim, data.numpy(), n_data=ip[0])
    if kind in ("logistic", "poisson"):
        return glm_case(kind, d or 8, GLM_N)
    raise ValueError(kind)


# rows of make_case's GLM data: ten 32-row tiles, the last one ragged
GLM_N = 300
# column scale of that data.  Every |X_nk| stays below 1, so a single
# coefficient of 3e38 (helpers.edge_points) leaves every eta finite: the row
# terms stay finite or overflow to +inf, b'b overflows, and U is +inf, not NaN.
# Poisson's smaller scale keeps |eta| below amh_expf's range at a coefficient
# of +-200, which the finite share of test_edge_points_reach needs.
GLM_X_SCALE = {"logistic": 0.25, "poisson": 0.0625}


def glm_case(kind, d, N, seed=None):
    """make_case for the GLM models at any N: posteriors.synthetic_logistic /
    synthetic_poisson (with offsets) at K = d - 1, the columns scaled by
    GLM_X_SCALE and clipped to [-1, 1]; the oracle reads the entry's own packed
    float32 data."""
    import orc
    import posteriors as P
    K = d - 1
    seed = 100 * d + N % 100 if seed is None else seed
    mk = P.synthetic_logistic(N, K, seed) if kind == "logistic" else P.synthetic_poisson(N, K, seed)
    X = np.clip(mk["X"] * np.float32(GLM_X_SCALE[kind]), -1.0, 1.0).astype(np.float32)
    if kind == "logistic":
        e = P.logistic_regression(X, mk["y"])
    else:
        e = P.poisson_regression(X, mk["y"], mk["offset"])
    arr, (N_, K_) = e.pack_fn(None)
    return dict(model=e), {}, orc.Model(orc.LOGISTIC if kind == "logistic" else orc.POISSON, K + 1, arr,
                                        n_data=N_, k_data=K_)


def state_to_orc(state):
    import orc
    s = state
    return orc.State(s.i.cpu().numpy().copy(), s.z.cpu().numpy().copy(), s.potential_energy.cpu().numpy().copy(),
                     s.mean_accept_prob.cpu().numpy().copy(), s.adapt_state.loc.cpu().numpy().copy(),
                     s.adapt_state.scale.cpu().numpy().copy(), s.adapt_state.log_step_size.cpu().numpy().copy(),
                     s.as_change.cpu().numpy().copy(), s.rng_key.cpu().numpy().view(np.uint32).copy())


FIELDS = ("i", "z", "potential_energy", "mean_accept_prob", "loc", "scale", "log_step_size", "as_change", "rng_key")


def assert_state_bitequal(gpu_state, orc_state, what=""):
    g = state_to_orc(gpu_state)
    for f in FIELDS:
        a = np.asarray(getattr(g, f))
        b = np.asarray(getattr(orc_state, f))
        assert a.shape == b.shape, (what, f, a.shape, b.shape)
        av = a.view(np.uint32) if a.dtype in (np.float32, np.int32, np.uint32) else a
        bv = b.view(np.uint32) if b.dtype in (np.float32, np.int32, np.uint32) else b
        bad = np.flatnonzero((av != bv).reshape(-1))
        assert bad.size == 0, (f"{what}: field {f} differs in {bad.size} of {av.size} entries; "
                               f"first at {bad[:5]}: gpu {a.reshape(-1)[bad[:5]]} oracle {b.reshape(-1)[bad[:5]]}")


# ------------------------------------------------- NaN-aware bit comparison --
ASSS_FIELDS = ("i", "z", "potential_energy", "loc", "scale", "as_change", "rng_key")


def assert_bitequal_nan(a, b, what=""):
    """Plain arrays: identical NaN positions, every other entry bit-identical
    (sign of zero, +-inf and subnormals included).  NaN payload and sign are
    not compared: x86 and gfx950 produce different default NaNs."""
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    b = b.detach().cpu().numpy() if hasattr(b, "detach") else np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if b.dtype != a.dtype and a.dtype.kind in "iu" and b.dtype.kind in "iu":
        b = b.astype(a.dtype)  # rng keys: int32 on the product side, uint32 on the oracle's
    assert a.dtype.itemsize == b.dtype.itemsize and a.dtype.itemsize in (4, 8), (what, a.dtype, b.dtype)
    bits = np.uint32 if a.dtype.itemsize == 4 else np.uint64
    a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
    ok = np.ones(a.size, bool)
    if a.dtype.kind == "f" or b.dtype.kind == "f":
        assert a.dtype == b.dtype, (what, a.dtype, b.dtype)
        na, nb = np.isnan(a), np.isnan(b)
        bad = np.flatnonzero(na != nb)
        assert bad.size == 0, (f"{what}: NaN positions differ in {bad.size} of {a.size} entries; first at "
                               f"{bad[:5]}: gpu {a[bad[:5]]} oracle {b[bad[:5]]}")
        ok = ~na
    bad = np.flatnonzero((a.view(bits) != b.view(bits)) & ok)
    assert bad.size == 0, (f"{what}: differs in {bad.size} of {a.size} entries; first at {bad[:5]}: "
                           f"gpu {a[bad[:5]]} oracle {b[bad[:5]]}")


def _leaf(state, f):
    """Field f of a product state (ARWMH or ASSS namedtuple) or of an orc.State."""
    if hasattr(state, "adapt_state") and f in ("loc", "scale", "log_step_size"):
        return getattr(state.adapt_state, f)
    return getattr(state, f)


def assert_state_bitequal_nan(gpu_state, orc_state, what="", fields=FIELDS):
    """assert_state_bitequal for states that may hold NaN: per field the NaN
    positions agree and every non-NaN entry is bit-identical.  `fields` takes
    ASSS_FIELDS for an ASSS state (no step-size leaves)."""
    for f in fields:
        assert_bitequal_nan(_leaf(gpu_state, f), _leaf(orc_state, f), f"{what}: field {f}")


# -------------------------------------------------------- edge scenarios ----
EDGE_VALUES = (0.0, -0.0, 1e-45, -1e-45, 1e-38, 1e-20, 1.0, -1.0, 20.0, -20.0, 87.0, 88.8, 89.0, -87.0, -104.0,
               200.0, -200.0, 1e4, -1e4, 1e19, -1e19, 3e38, -3e38, np.inf, -np.inf, np.nan)
EDGE_ROW_VALUES = (1e-45, 1e19, 3e38, np.inf, np.nan)
EDGE_REPS = 5  # seeded positions per value

STEP_SIZE_CYCLE = (-110.0, -90.0, -20.0, 0.0, 20.0, 45.0, 88.0, 89.0)
FACTOR_CYCLE = (1e-30, 1e-20, 1e-8, 1.0, 1e8, 1e15, 1e19, 1e25)
# num_warmup of the hostile scenarios: hostile_adapt is applied at i = 5, so
# steps 6-8 run with gamma_6..8 < 1 from the hostile values (loc decays from
# 1e19 slowly), step 9 is the warmup reset (gamma_1 = 1: sqrt(1 - gamma) L = 0
# -> keep L, loc jumps), and the schedule restarts after it
HOSTILE_WARMUP = 8


def log_scale_coords(kind, d):
    """Coordinates a model exponentiates (log tau / log sigma)."""
    return {"eight_schools": (1,), "kidiq": (3,), "diamonds": (d - 1,), "diamonds_ss": (d - 1,)}.get(kind, ())


def edge_points(d, seed, hit=()):
    """-> (torch [n, d], numpy [n, d]) float32, the same values: N(0, 1) rows
    with one coordinate replaced in turn by each of EDGE_VALUES, at EDGE_REPS
    seeded positions among the coordinates outside `hit` and once at every
    coordinate of `hit` (log_scale_coords: each value reaches the exponentiated
    coordinate exactly once per row set, so most rows keep a finite potential),
    then rows with every coordinate at one of EDGE_ROW_VALUES."""
    import torch
    rng = np.random.default_rng(seed)
    rows = []
    with np.errstate(over="ignore", under="ignore"):
        for v in EDGE_VALUES:
            free = [r for r in range(d) if r not in hit] or list(range(d))
            pos = [free[int(p)] for p in rng.integers(0, len(free), size=EDGE_REPS)] + [int(h) for h in hit]
            for p in pos:
                r = rng.normal(size=d).astype(np.float32)
                r[p] = np.float32(v)
                rows.append(r)
        for v in EDGE_ROW_VALUES:
            rows.append(np.full(d, v, np.float32))
    z = np.stack(rows).astype(np.float32)
    return torch.from_numpy(z.copy()), z


def wild_starts(C, d, seed):
    """-> (torch [C, d], numpy [C, d]) float32: N(0, 1) * 10^k with one seeded
    integer k in [-3, 20] per chain."""
    import torch
    rng = np.random.default_rng(seed)
    k = rng.integers(-3, 21, size=C)
    z = (rng.normal(size=(C, d)) * (10.0 ** k)[:, None]).astype(np.float32)
    return torch.from_numpy(z.copy()), z


def hostile_adapt(state, step_size=True, factors=FACTOR_CYCLE, step_sizes=STEP_SIZE_CYCLE, loc_shift=1e19):
    """Push the adaptation state of an orc.State (numpy, edited in place) or of
    a product state (GPU tensors, edited in place from the same host
    arithmetic, so both sides hold the same bits) to hostile values:
    log_step_size cycles over STEP_SIZE_CYCLE by chain index, the packed factor
    is multiplied per chain by factors[(chain // 8) % 8], loc += 1e19 on
    the upper half of the chains.  step_size=False (ASSS) skips the step-size
    leaf; factors / step_sizes / loc_shift replace the cycles and the shift
    (the float64 step anchors of tests/test_edges.py shrink their top ends).
    Returns the state."""
    product = hasattr(state, "adapt_state")
    loc, scale = _leaf(state, "loc"), _leaf(state, "scale")
    C = loc.shape[0]
    c = np.arange(C)
    mult = np.asarray(factors, np.float32)[(c // 8) % 8]
    lam = np.asarray(step_sizes, np.float32)[c % 8]

    def edit(t, fn):
        if product:
            import torch
            a = t.detach().cpu().numpy().copy()
            fn(a)
            t.copy_(torch.from_numpy(a))  # in place: bumps the version counter
        else:
            fn(t)

    def mul_scale(a):
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            a *= mult[:, None]

    def add_loc(a):
        a[C // 2:] += np.float32(loc_shift)

    edit(scale, mul_scale)
    edit(loc, add_loc)
    if step_size:
        def set_lam(a):
            a[:] = lam
        edit(_leaf(state, "log_step_size"), set_lam)
    return state


# the model matrix of the edge tests (tests/test_edges.py, tests/test_gpu_edges.py)
EDGE_MATRIX = [("gaussian", 1), ("gaussian", 5), ("gaussian", 33), ("gaussian", 64), ("gaussian", 72),
               ("gaussian", 100), ("gaussian", 128), ("gaussian", 256), ("eight_schools", None), ("kidiq", None),
               ("diamonds", None), ("diamonds_n77", None), ("diamonds_ss", None), ("mixture", 1), ("mixture", 3),
               ("logistic", 8), ("logistic", 32), ("logistic_n77", 8), ("logistic_n77", 32),
               ("poisson", 9), ("poisson", 32), ("poisson_n77", 9), ("poisson_n77", 32)]


def make_edge_case(kind, d=None):
    """make_case plus "diamonds_n77": the literal diamonds model off the
    compile-time fast path (N = 77, K = 10; the generic split transition), and
    "logistic_n77" / "poisson_n77": the GLM models off the 32-row tile (N = 77)."""
    if kind in ("logistic_n77", "poisson_n77"):
        return glm_case(kind[:-4], d or 8, 77)
    if kind == "diamonds_n77":
        import orc
        import posteriors as P
        mk = P.synthetic_diamonds(N=77, K=10, seed=5)
        arr, (N, K) = P.diamonds.pack_fn(mk)
        return dict(model=P.diamonds), mk, orc.Model(orc.DIAMONDS, K + 1, arr, n_data=N, k_data=K)
    return make_case(kind, d)


def edge_init(kind, d, C, orc, seed=0, start="uniform"):
    """Oracle-side start of an edge scenario -> (kw, mk, om, ost, z0): z0 is
    uniform(-2, 2) (the benign start of tests/test_gpu_parity.py) or
    wild_starts; every model takes it as flat init_params."""
    kw, mk, om = make_edge_case(kind, d)
    if start == "wild":
        z0 = wild_starts(C, om.d, seed)[1]
    else:
        z0 = np.random.default_rng(seed).uniform(-2, 2, size=(C, om.d)).astype(np.float32)
    from kernels_amd import PRNGKey
    ost = orc.init(om, PRNGKey(seed), C, init_z=z0)
    return kw, mk, om, ost, z0


# ------------------------------------------- pooled mode, float64 reference --
POOLED_LEAVES = ("i", "macc", "mu", "L", "lam", "asc", "cov")


def pooled_ref_model(kind, om):
    """The float64 potential and its float32 forward bound (oracle/pooled_np.py)
    of an orc.Model."""
    import pooled_np as pnp
    if kind == "gaussian":
        return pnp.gaussian_model(om.data, om.d)
    if kind == "eight_schools":
        return pnp.eight_schools_model(om.data, om.d)
    raise ValueError(kind)


def pooled_warm_start(kind, d, C, seed, K=1):
    """-> (z0 float32 [C, d], shared): a pooled state in the typical set, so
    that a block accepts a fair share of its proposals at every d (from the
    uniform(-2, 2) start with the identity factor almost none are accepted at
    large d).  shared has the leaves of orc.pooled_init_shared:
    i, macc, mu, L, lam, asc, cov.

    gaussian: z0 ~ N(m, P^-1), L = chol(P^-1) in float32, cov = P^-1 packed in
    float64, lam = log(2.38 / sqrt(d)) (the optimal random-walk scale), mu = m
    + 0.05, macc = 0.2, i = 20 K.  eight_schools: the oracle's own shared
    state and z after 300 pooled CPU steps from uniform(-2, 2)."""
    import orc
    import pooled_np as pnp
    from kernels_amd import PRNGKey
    _, _, om = make_case(kind, d)
    d = om.d
    rng = np.random.default_rng(seed)
    if kind == "gaussian":
        ref = pooled_ref_model(kind, om)
        cov = np.linalg.inv(ref.P)
        cov = 0.5 * (cov + cov.T)
        Lc = np.linalg.cholesky(cov)
        z0 = (ref.m + rng.normal(size=(C, d)) @ Lc.T).astype(np.float32)
        sh = dict(i=np.array([20 * K], np.int32), macc=np.array([0.2], np.float32),
                  mu=(ref.m + 0.05).astype(np.float32), L=pnp.pack(Lc).astype(np.float32),
                  lam=np.array([np.log(2.38 / np.sqrt(d))], np.float32), asc=np.zeros(1, np.float32),
                  cov=pnp.pack(cov).astype(np.float64))
        return z0, sh
    if kind == "eight_schools":
        z0 = rng.uniform(-2, 2, size=(C, d)).astype(np.float32)
        st = orc.init(om, PRNGKey(seed), C, init_z=z0)
        z, pe, keys = st.z, st.potential_energy, st.rng_key
        sh = orc.pooled_init_shared(d)
        for _ in range(300):
            z, pe, sums = orc.pooled_stats(om, int(sh["i"][0]), z, pe, keys, sh["mu"], sh["L"], float(sh["lam"][0]))
            orc.pooled_update(om, sums, sh)
        return z.copy(), {k: np.array(v) for k, v in sh.items()}
    raise ValueError(kind)


def pooled_leaves(state):
    """The shared leaves of a PooledState by their orc names."""
    return dict(i=state.i, macc=state.mean_accept_prob, mu=state.adapt_state.loc, L=state.adapt_state.scale,
                lam=state.adapt_state.log_step_size, asc=state.as_change, cov=state.cov)


def apply_shared(state, sh):
    """Copy a shared dict into the leaves of a PooledState, in place (the same
    bits on both sides of a comparison).  Returns the state."""
    import torch
    for name, t in pooled_leaves(state).items():
        t.copy_(torch.as_tensor(np.asarray(sh[name])).to(t.dtype))  # (same dtype on both sides: no rounding)
    return state


def shared_to_host(state):
    return {k: v.detach().cpu().numpy().copy() for k, v in pooled_leaves(state).items()}


def pooled_reference_shares(model, keys, z0, sh, K, W, blocks, lr_decay=2 / 3):
    """The float64 reference alone, `blocks` blocks from the warm start: the
    share of chain-steps that moved in each block."""
    import pooled_np as pnp
    cur = {k: np.array(v, np.float64 if k != "i" else np.int64) for k, v in sh.items()}
    z, pe, out = np.asarray(z0, np.float64), None, []
    for _ in range(blocks):
        s = pnp.stats(model.U, int(cur["i"][0]), z, pe, keys, cur["mu"], cur["L"], float(cur["lam"][0]), K=K)
        out.append(pnp.accepted_share(s))
        up = pnp.update(pnp.pack_sums(s.S_d, s.S_dd, s.S_a, s.N), cur, K=K, num_warmup=W, lr_decay=lr_decay)
        z, pe = s.z, s.pe
        cur = dict(i=np.array([up.i]), macc=np.array([up.macc]), mu=up.mu, L=pnp.pack(up.L), lam=np.array([up.lam]),
                   asc=np.array([up.asc]), cov=pnp.pack(up.cov))
    return out


class OraclePooled:
    """The C oracle behind the interface pooled_f64_blocks drives."""

    def __init__(self, orc, kind, d, C, K, W, seed, z0, sh):
        from kernels_amd import PRNGKey
        self.orc, self.K, self.W = orc, K, W
        _, _, self.om = make_case(kind, d)
        st = orc.init(self.om, PRNGKey(seed), C, init_z=z0)
        self.z, self.pe, self.keys = st.z, st.potential_energy, st.rng_key
        self.sh = {k: np.array(v) for k, v in sh.items()}

    def shared(self):
        return {k: np.array(v) for k, v in self.sh.items()}

    def history(self):
        """z after each of the K frozen single steps of the next block."""
        z, pe, sh, out = self.z, self.pe, self.sh, []
        for t in range(self.K):
            z, pe, _ = self.orc.pooled_stats(self.om, int(sh["i"][0]) + t, z, pe, self.keys, sh["mu"], sh["L"],
                                             float(sh["lam"][0]))
            out.append(z)
        return out, pe

    def block(self):
        sh = self.sh
        z, pe, sums = self.orc.pooled_stats(self.om, int(sh["i"][0]), self.z, self.pe, self.keys, sh["mu"], sh["L"],
                                            float(sh["lam"][0]), k_steps=self.K)
        self.orc.pooled_update(self.om, sums, sh, num_warmup=self.W, k_steps=self.K)
        self.z, self.pe = z, pe
        return z, pe, sums


def pooled_f64_blocks(impl, model, keys, K, W, blocks=3):
    """Drive `impl` (OraclePooled, or the GPU twin of tests/test_gpu_pooled_f64.py)
    for `blocks` blocks and compare each with the float64 restatement
    (pooled_np.check_block).  K > 1: the block's intermediate z is not
    observable, so the K frozen steps are first run one by one; the block's z
    and pe must equal the last of them byte for byte, and its sums are bounded
    against the float64 sums of that history.  Returns the per-block results
    {quantity: error / bound}."""
    import pooled_np as pnp
    res = []
    for b in range(blocks):
        before = impl.shared()
        z_in = np.array(impl.z_host() if hasattr(impl, "z_host") else impl.z)
        hist = impl.history() if K > 1 else None
        z, pe, sums = impl.block()
        z, pe, sums = np.asarray(z), np.asarray(pe), np.asarray(sums)
        if hist is not None:
            zs, pe_last = hist
            assert zs[-1].tobytes() == z.tobytes(), f"block {b + 1}: z is not that of {K} single steps"
            assert np.asarray(pe_last).tobytes() == pe.tobytes(), f"block {b + 1}: pe is not that of {K} single steps"
            zs = np.stack([z_in] + [np.asarray(x) for x in zs])
        else:
            zs = np.stack([z_in, z])
        r = pnp.check_block(model, keys, before, zs, pe, sums, impl.shared(), K=K, num_warmup=W)
        print(f"block {b + 1}: " + " ".join(f"{k}={v:.3g}" for k, v in r.items()))
        C = z.shape[0]
        assert r["skipped"] <= max(2, C / 100), (b, r["skipped"])
        assert not pnp.worst(r), (f"block {b + 1}", pnp.worst(r))
        res.append(r)
    return res


# ------------------------------------------- grid caps and item hand-over ----
# One pass of a capped grid-stride launch, in items (tests/test_gpu_steady.py,
# tests/test_gpu_steady_pnx.py).  Read from the launchers; every test that
# relies on one asserts that its size crosses it, so a raised cap fails there.
BIG_CAP = 4096 * 4    # amh_big.hip wave_grid: 4,096 blocks x 4 waves, one chain per wave
GROUP_CAP = 8192 * 4  # amh_kernels.hip grid_for and its copies in amh_asss.hip, amh_asss_ext.hip and
#                       amh_split.hip: 8,192 blocks x 4 waves, one item of CPW = 64 / G chains per wave


def items_per_wave(C, cap, cpw=1):
    """Items the busiest wave of a capped launch takes for C chains at cpw
    chains per item: wave w walks items w, w + cap, ..."""
    n_items = -(-C // cpw)
    return -(-n_items // cap)


def state_rows(state, lo, hi):
    """Chains [lo, hi) of a product state (ARWMH or ASSS namedtuples): the same
    types, every leaf sliced on the device, so only the slice reaches the host."""
    a = state.adapt_state
    return type(state)(*[type(a)(*[t[lo:hi] for t in a]) if f is a else f[lo:hi] for f in state])


def assert_chains_bitequal(got, ref, cap, cpw, what=""):
    """[C, d] (or [C]) arrays bit for bit; a mismatch is reported by chain with
    the item, the wave and the pass of the capped launch that produced it."""
    got = got.detach().cpu().numpy() if hasattr(got, "detach") else np.asarray(got)
    ref = np.asarray(ref)
    C = got.shape[0]
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    ne = (got.view(np.uint32) != ref.view(np.uint32)).reshape(C, -1).any(axis=1)
    bad = np.flatnonzero(ne)
    where = [f"chain {c}: item {c // cpw} = wave {(c // cpw) % cap}, pass {(c // cpw) // cap}" for c in bad[:4]]
    assert bad.size == 0, f"{what}: {bad.size} of {C} chains differ; first {where}"
