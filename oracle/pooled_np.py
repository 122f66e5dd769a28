"""Literal float64 restatement of one pooled block (regime B) and the forward
error bounds that pin the kernels and the C oracle to it.

TEST INFRASTRUCTURE ONLY (never imported by the product package).

Written from the formulas of the pooled header comment of oracle/amh_oracle.c
and DESIGN.md §3.5, not from the oracle's loops: there are no chunks, waves,
tiles or accumulation orders here, only sums over all chain-steps in float64.

    proposal   z' = z + e^lam L xi + eps xi
    accept     alpha = min(1, exp(U(z) - U(z'))), NaN U(z') -> +inf; u < alpha
    sums       delta = z_new - mu (the frozen mu of the block)
               S_d = sum delta, S_dd = sum delta delta^T, S_a = sum alpha,
               N = K C, over the K C chain-steps of a block
    update     n = block count (i / K + 1, restarting at num_warmup)
               gamma = n^-a
               mu'  = mu + gamma S_d / N
               Sig' = (1 - gamma) Sig + gamma S_dd / N, L' = chol(Sig') or keep
               lam' = lam + gamma (S_a / N - target)
               macc' = macc + (S_a / N - macc) / n
               as_change = ||L' e^lam' - L e^lam||_F,  i' = i + K

Layouts as oracle/orc.py: packed lower triangle column-major, sums vector
[S_d (d) | S_dd packed (P) | S_a | N].
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

import arwmh_np as lit

U32 = 2.0 ** -24          # unit roundoff of float32
U64 = 2.0 ** -53          # ... of float64
THRESHOLD = 1e-4          # |u - alpha| below which a decision is not compared (tests/test_oracle.py)
NORMAL_ERR = 2e-6 * 5     # |float32 normal - float64 normal| (tests/test_rng_math.py::test_normal_stream)
GAMMA_ULPS = 1.5          # float32 gamma against n^-a (tests/test_rng_math.py::test_lr_gamma)
EXPF_ULPS = 1.5           # amh_expf (tests/test_rng_math.py::test_expf)
PE_TOL = (2e-5, 1e-3)     # (rtol, atol) of a float32 potential, TOL["pe"] of tests/test_oracle.py
COV_RTOL = 1e-12          # Sigma' (tests/test_pooled.py::test_block_update_counts_blocks)
PIVOT_RATIO = 1e-3        # the keep / refactorise decision is compared from this conditioning up


def gam(n, u=U32):
    """gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability, Lemma 3.1):
    the product of n factors (1 + e_i), |e_i| <= u, is 1 + t with |t| <= gamma_n."""
    n = np.asarray(n, np.float64)
    return n * u / (1.0 - n * u)


# ----------------------------------------------------------------- layout --
def packed_size(d):
    return d * (d + 1) // 2


def unpack(p, d):
    """packed lower triangle (column-major) -> [d, d] lower-triangular float64."""
    M = np.zeros((d, d), np.float64)
    k = 0
    for j in range(d):
        M[j:, j] = np.asarray(p[k:k + d - j], np.float64)
        k += d - j
    return M


def pack(M):
    d = M.shape[0]
    return np.concatenate([M[j:, j] for j in range(d)])


def unpack_sym(p, d):
    M = unpack(p, d)
    return M + np.tril(M, -1).T


def pack_sums(S_d, S_dd, S_a, N):
    return np.concatenate([np.asarray(S_d, np.float64), pack(np.asarray(S_dd, np.float64)), [S_a, N]])


def split_sums(v, d):
    """sums vector -> (S_d [d], S_dd [d, d] symmetric, S_a, N)."""
    v = np.asarray(v, np.float64)
    P = packed_size(d)
    return v[:d], unpack_sym(v[d:d + P], d), float(v[d + P]), float(v[d + P + 1])


# ----------------------------------------------------------------- models --
def gaussian_model(data, d):
    """The dense Gaussian of the packed float32 data [m (d) | P (d d) | c0]:
    U(x) = 1/2 (x - m)^T P (x - m) + c0, over rows of x.

    tau(x): forward bound of a float32 evaluation.  The quadratic form is 2 d
    products and sums of (x - m) and P, each operand rounded once; with the
    subtraction, the halving and the final add that is at most 2 d + 4 factors
    (1 + e) on every term, in any summation order (Higham §3.1):
        |fl(U) - U| <= gamma_{2d+4} (1/2 |x-m|^T |P| |x-m| + |c0|)."""
    data = np.asarray(data, np.float64)
    m, P, c0 = data[:d], data[d:d + d * d].reshape(d, d), float(data[d + d * d])
    aP = np.abs(P)

    def U(x):
        y = np.asarray(x, np.float64) - m
        return 0.5 * np.einsum("cr,cr->c", y @ P, y) + c0

    def tau(x):
        y = np.abs(np.asarray(x, np.float64) - m)
        return gam(2 * d + 4) * (0.5 * np.einsum("cr,cr->c", y @ aP, y) + abs(c0))

    return SimpleNamespace(U=U, tau=tau, d=d, m=m, P=P, c0=c0)


def eight_schools_model(data, d=10):
    """Non-centred eight schools on the packed data [y (J) | sigma (J)];
    tau is TOL["pe"] of tests/test_oracle.py (rtol |U| + atol)."""
    data = np.asarray(data, np.float64)
    J = d - 2
    y, s = data[:J], data[J:2 * J]

    def U(x):
        x = np.asarray(x, np.float64)
        with np.errstate(all="ignore"):
            return np.array([lit.eight_schools_potential(r, y, s) for r in x])

    def tau(x):
        return PE_TOL[0] * np.abs(U(x)) + PE_TOL[1]

    return SimpleNamespace(U=U, tau=tau, d=d)


# ------------------------------------------------------------------ stats --
def _f64(a):
    return np.asarray(a, np.float64)


def _factor(L, d):
    L = _f64(L)
    return unpack(L, d) if L.ndim == 1 else L


def stats(U, i, z, pe, keys, mu, L, lam, K=1, eps=1e-6):
    """K frozen pooled transitions of every chain, in float64.

    z [C, d]; pe [C] or None (then U(z)); keys [C, 2] uint32; mu [d]; L packed
    or [d, d]; the noise of step t sits at stream position i + t.  Returns a
    namespace: z, pe after the block; per step t the arrays zs [K + 1, C, d]
    (zs[0] = z), prop [K, C, d], xi [K, C, d], u, alpha, accept [K, C],
    pe_prop [K, C]; and the sums S_d, S_dd (full matrix), S_a, N with the
    companions A_d = sum |delta|, A_dd = sum |delta| |delta|^T."""
    z = _f64(z).copy()
    C, d = z.shape
    mu, Lm = _f64(mu), _factor(L, d)
    el = math.exp(float(lam))
    eps = float(np.float32(eps))
    pe = U(z) if pe is None else _f64(pe).copy()
    zs, prop, xis, us, als, acs, pps = [z.copy()], [], [], [], [], [], []
    S_d, S_dd, A_d, A_dd, S_a = np.zeros(d), np.zeros((d, d)), np.zeros(d), np.zeros((d, d)), 0.0
    for t in range(K):
        bits, ubits = lit.step_noise(keys, int(i) + t, d)
        xi = lit.normal_from_bits(bits)
        u = lit.unif01_from_bits(ubits).astype(np.float64)
        zp = z + el * (xi @ Lm.T) + eps * xi
        with np.errstate(all="ignore"):
            pp = U(zp)
            pp = np.where(np.isnan(pp), np.inf, pp)
            alpha = np.minimum(1.0, np.exp(pe - pp))
        acc = u < alpha
        z = np.where(acc[:, None], zp, z)
        pe = np.where(acc, pp, pe)
        delta = z - mu
        S_d += delta.sum(0)
        S_dd += delta.T @ delta
        A_d += np.abs(delta).sum(0)
        A_dd += np.abs(delta).T @ np.abs(delta)
        S_a += float(alpha.sum())
        for lst, v in ((zs, z.copy()), (prop, zp), (xis, xi), (us, u), (als, alpha), (acs, acc), (pps, pp)):
            lst.append(v)
    return SimpleNamespace(z=z, pe=pe, zs=np.stack(zs), prop=np.stack(prop), xi=np.stack(xis), u=np.stack(us),
                           alpha=np.stack(als), accept=np.stack(acs), pe_prop=np.stack(pps), S_d=S_d, S_dd=S_dd,
                           S_a=S_a, N=float(K * C), A_d=A_d, A_dd=A_dd, K=K, C=C, d=d)


def sums_of(zs, mu):
    """The float64 sums of a given history of states zs [T, C, d] (the z after
    each of T steps) against the frozen mu -> (S_d, S_dd, A_d, A_dd)."""
    zs = _f64(zs)
    d = zs.shape[-1]
    delta = (zs - _f64(mu)).reshape(-1, d)
    a = np.abs(delta)
    return delta.sum(0), delta.T @ delta, a.sum(0), a.T @ a


# ----------------------------------------------------------------- update --
def block_n(i, K, W):
    """The block count of the learning rate: blocks since the start, or since
    num_warmup once i has reached it."""
    return i // K + 1 if i < W else (i - W) // K + 1


def update(sums, shared, K=1, num_warmup=0, lr_decay=2 / 3, target=0.234, gamma=None, n=None):
    """The shared-state update from a sums vector, in float64.  `shared` holds
    i, macc, mu, L (packed), lam, cov (packed) as orc.pooled_init_shared; it
    is not modified.  gamma / n override the schedule (the float32 gamma a
    kernel used; a deliberately wrong n in the checker's self-test).
    Returns a namespace: n, gamma, mu, cov [d, d], L [d, d] (the old factor if
    Sigma' has no Cholesky factor), refactored, pivot_ratio (smallest / largest
    squared diagonal of L', 0 if none), lam, macc, asc, i."""
    d = np.asarray(shared["mu"]).shape[0]
    i = int(np.asarray(shared["i"]).reshape(-1)[0])
    S_d, S_dd, S_a, N = split_sums(sums, d)
    n = block_n(i, K, int(num_warmup)) if n is None else n
    a = float(np.float32(lr_decay))
    g = float(lit.lr_gamma(n, a)) if gamma is None else float(gamma)
    mu0, lam0, macc0 = _f64(shared["mu"]), float(np.asarray(shared["lam"]).reshape(-1)[0]), \
        float(np.asarray(shared["macc"]).reshape(-1)[0])
    L0, cov0 = unpack(shared["L"], d), unpack_sym(shared["cov"], d)
    abar = S_a / N
    mu = mu0 + g * S_d / N
    cov = (1.0 - g) * cov0 + g * S_dd / N
    try:
        with np.errstate(all="ignore"):
            L = np.linalg.cholesky(cov)
        ok = bool(np.all(np.isfinite(L)))
    except np.linalg.LinAlgError:
        ok = False
    if ok:
        piv = np.diagonal(L) ** 2
        ratio = float(piv.min() / piv.max())
    else:
        L, ratio = L0, 0.0
    lam = lam0 + g * (abar - float(np.float32(target)))
    macc = macc0 + (abar - macc0) / n
    asc = float(np.linalg.norm(L * math.exp(lam) - L0 * math.exp(lam0), "fro"))
    return SimpleNamespace(n=n, gamma=g, mu=mu, cov=cov if ok else cov0, cov_new=cov, L=L, refactored=ok,
                           pivot_ratio=ratio, lam=lam, macc=macc, asc=asc, i=i + K, abar=abar,
                           terms=dict(mu=np.abs(mu0) + g * np.abs(S_d / N),
                                      lam=abs(lam0) + g * (abs(abar) + float(np.float32(target))),
                                      macc=abs(macc0) + (abs(abar) + abs(macc0)) / n))


def gamma_candidates(n, lr_decay=2 / 3):
    """The float32 values a kernel may hold for gamma_n: those within
    GAMMA_ULPS of n^-a in float64 (a rounded to float32), the slack
    tests/test_rng_math.py::test_lr_gamma asserts; gamma_1 = 1 exactly."""
    g = float(lit.lr_gamma(n, float(np.float32(lr_decay))))
    if n == 1:
        return [1.0]
    c = np.float32(g)
    ulp = float(np.spacing(c))
    out, x = [], c
    for _ in range(3):
        x = np.nextafter(x, np.float32(0))
    for _ in range(7):
        if abs(float(x) - g) <= GAMMA_ULPS * ulp:
            out.append(float(x))
        x = np.nextafter(x, np.float32(2))
    return out


# ----------------------------------------------------------------- bounds --
class bounds:
    """Forward-error bounds of a float32 pooled block against this module's
    float64 values.  Every bound is computed from reference quantities; u =
    2^-24, gamma_n = n u / (1 - n u)."""

    @staticmethod
    def acc_len(d, C, K):
        """Length n of one float32 accumulation chain of the sums.
        d >= 64: a 128-chain chunk, one step (blocks above d = 64 add the
        per-step sums in double); d = 64 in a K-block: the chunk's 128 K
        chain-steps.  d < 64: one wave's chains (cpw = ceil(C / 4096), at most
        16) times K, then the 4-level float32 tree over the 16 waves."""
        if d > 64:
            return 128
        if d == 64:
            return 128 * K
        cpw = min(16, max(1, -(-C // 4096)))
        return cpw * K + 4

    @staticmethod
    def n_double_adds(d, C, K):
        """Double-precision adds behind one component: chunks in groups of 16,
        the groups, and above d = 64 the K per-step sums."""
        chunk = 128 if d >= 64 else 16 * min(16, max(1, -(-C // 4096)))
        chunks = -(-C // chunk)
        return 16 + -(-chunks // 16) + (K if d > 64 else 0)

    @staticmethod
    def S_dd(A_dd, d, C, K):
        """|S_dd - ref| <= (gamma_{n+3} + gamma^(64)_g) sum |delta_r| |delta_k|.
        Each delta is one rounded subtraction of exact inputs (two factors per
        product), the fused multiply-add chain of n terms adds at most n
        factors on the first term (Higham (3.3)), and one more covers the
        conversion and the symmetric write: n + 3.  The g double adds
        contribute gamma_g at u = 2^-53.  Worst case, so no margin."""
        n = bounds.acc_len(d, C, K)
        return (gam(n + 3) + gam(bounds.n_double_adds(d, C, K), U64)) * A_dd

    @staticmethod
    def S_d(A_d, d, C, K):
        """As S_dd against sum |delta_r| (one rounded delta, n adds)."""
        n = bounds.acc_len(d, C, K)
        return (gam(n + 3) + gam(bounds.n_double_adds(d, C, K), U64)) * A_d

    @staticmethod
    def S_a(alpha, tau_z, tau_prop):
        """|S_a - sum alpha| <= sum_c alpha_c (tau_U(z_c) + tau_U(z'_c)) + 4 u
        per chain-step.  alpha = exp(U - U') moves by a relative e^t - 1 ~ t
        when its exponent moves by t <= tau_U + tau_U' (where alpha is clipped
        at 1 the move is no larger); 4 u per term covers amh_expf (1.5 ulp = 3
        u) and the rounded add."""
        return float(np.sum(alpha * (tau_z + tau_prop)) + alpha.size * 4 * U32)

    @staticmethod
    def z_moved(z, xi, L, lam, eps, d):
        """|z'_kernel - z'| <= gamma_{d+3} (|z| + e^lam |L| |xi| + eps |xi|)
        + NORMAL_ERR (e^lam |L| 1 + eps): d fused multiply-adds of the row of
        L, then the scaling by e^lam, the eps term and the add (+ 3); the float32 normals sit within NORMAL_ERR of the float64
        ones (tests/test_rng_math.py::test_normal_stream), which moves L xi by
        at most NORMAL_ERR times the row sums of |L| (+ eps)."""
        aL = np.abs(L)
        el = math.exp(float(lam))
        mag = np.abs(z) + el * (np.abs(xi) @ aL.T) + eps * np.abs(xi)
        return gam(d + 3) * mag + NORMAL_ERR * (el * aL.sum(1) + eps)

    @staticmethod
    def pe(U):
        """TOL["pe"] of tests/test_oracle.py."""
        return PE_TOL[0] * np.abs(U) + PE_TOL[1]

    @staticmethod
    def scalar(terms):
        """mu', lam', macc': at most four roundings (the float32 mean, the
        product with gamma, the difference, the sum), each at most u of a
        term's magnitude: 4 u (sum of the magnitudes of the terms)."""
        return 4 * U32 * terms

    @staticmethod
    def factor(Lk, cov, d):
        """|L' L'^T - Sigma'| <= gamma_{d+6} |L'| |L'|^T + u |Sigma'|.
        Higham Theorem 10.3 gives gamma_{d+1} for Cholesky with correctly
        rounded sqrt and divide.  The d >= 64 update scales column j by y =
        amh_rsqrt_nr(pivot) (relative error e, |e| <= 1.2 ulp <= 2.4 u) with
        L_jj = fl(pivot y): then L_jj^2 = pivot (1+e)^2 (1+e1)^2 and L_rj L_jj
        = a_rj (1+e)^2 (1+e1)(1+e2), i.e. 2 e <= 4.8 u beyond the two
        roundings the theorem already counts: d + 1 + 5.  u |Sigma'| is the
        rounding of Sigma' to float32 before the factorisation; below d = 64
        the factor is computed in double and rounded once, which the same
        bound covers."""
        aL = np.abs(Lk)
        return gam(d + 6) * (aL @ aL.T) + U32 * np.abs(cov)

    @staticmethod
    def as_change(Lk, lamk, L0, lam0, ref, d):
        """Each entry fl(fl(L' e') - fl(L e)) is off by at most (1 + 1 + 2
        EXPF_ULPS) u (|L'| e' + |L| e) (product, difference, amh_expf), so the
        norm by 5 u || |L'| e' + |L| e ||_F (triangle inequality); the float32
        sum of the d (d + 1) / 2 squares and the root add gamma_P relative."""
        m = np.abs(Lk) * math.exp(lamk) + np.abs(L0) * math.exp(lam0)
        return (2 + 2 * EXPF_ULPS) * U32 * float(np.linalg.norm(m, "fro")) + float(gam(packed_size(d) + 1)) * ref


# ---------------------------------------------------------------- checker --
def accepted_share(res):
    """Share of a block's chain-steps that moved, in the reference run."""
    return float(res.accept.mean())


def check_block(model, keys, shared, zs, pe_out, sums, after, K=1, num_warmup=0, lr_decay=2 / 3, target=0.234,
                eps=1e-6):
    """Compare one block of an implementation with the float64 reference.

    shared: the shared state the block ran with (orc layout, float32 / packed);
    zs [K + 1, C, d] float32: the block's input z and the z after each of its
    K frozen steps; pe_out [C]; sums [V] float64; after: the shared state
    after the update (same layout as shared).  Everything is teacher-forced:
    each step is restated from the z the implementation held before it, the
    sums from the z history it wrote, the update from its own sums vector.
    Returns {quantity: max error / bound} (exact quantities: 0 or inf) and
    `skipped`, the chains within THRESHOLD of a decision; all <= 1 passes."""
    zs = np.asarray(zs)
    C, d = zs.shape[1:]
    mu32, lam32 = np.asarray(shared["mu"]), float(np.asarray(shared["lam"]).reshape(-1)[0])
    L0 = unpack(shared["L"], d)
    i0 = int(np.asarray(shared["i"]).reshape(-1)[0])
    r = {}
    # ---- per-chain state, step by step ----
    near = np.zeros(C, bool)
    zerr = np.zeros(C)
    flips = np.zeros(C, bool)
    S_a_ref, S_a_bound = 0.0, 0.0
    for t in range(K):
        s = stats(model.U, i0 + t, zs[t], None, keys, mu32, L0, lam32, K=1, eps=eps)
        near |= np.abs(s.u[0] - s.alpha[0]) < THRESHOLD
        moved = np.any(zs[t + 1].view(np.uint32) != zs[t].view(np.uint32), axis=1)
        flips |= moved != s.accept[0]
        b = bounds.z_moved(_f64(zs[t]), s.xi[0], L0, lam32, float(np.float32(eps)), d)
        e = np.abs(_f64(zs[t + 1]) - s.prop[0]) / b
        zerr = np.maximum(zerr, np.where(moved, e.max(1), 0.0))
        S_a_ref += s.S_a
        with np.errstate(invalid="ignore"):
            tp = np.where(np.isfinite(s.pe_prop[0]), model.tau(s.prop[0]), 0.0)
        S_a_bound += bounds.S_a(s.alpha[0], model.tau(zs[t]), tp)
    ok = ~near
    r["skipped"] = int(near.sum())
    r["decisions"] = float(np.inf) if np.any(flips & ok) else 0.0
    r["z"] = float(zerr[ok].max()) if ok.any() else 0.0
    Uo = model.U(zs[K])
    r["pe"] = float(np.max(np.abs(_f64(pe_out) - Uo) / bounds.pe(Uo)))
    # ---- sums against the z history ----
    S_d, S_dd, S_a, N = split_sums(sums, d)
    R_d, R_dd, A_d, A_dd = sums_of(zs[1:], mu32)
    r["N"] = 0.0 if N == float(K * C) else float(np.inf)
    r["S_dd"] = float(np.max(np.abs(S_dd - R_dd) / bounds.S_dd(A_dd, d, C, K)))
    r["S_d"] = float(np.max(np.abs(S_d - R_d) / bounds.S_d(A_d, d, C, K)))
    r["S_a"] = abs(S_a - S_a_ref) / S_a_bound
    # ---- update from the implementation's own sums ----
    i1 = int(np.asarray(after["i"]).reshape(-1)[0])
    r["i"] = 0.0 if i1 == i0 + K else float(np.inf)
    n = block_n(i0, K, int(num_warmup))
    best = None
    for g in gamma_candidates(n, lr_decay):
        up = update(sums, shared, K, num_warmup, lr_decay, target, gamma=g, n=n)
        q = dict(mu=float(np.max(np.abs(_f64(after["mu"]) - up.mu) / bounds.scalar(up.terms["mu"]))),
                 lam=abs(float(np.asarray(after["lam"]).reshape(-1)[0]) - up.lam) / bounds.scalar(up.terms["lam"]),
                 macc=abs(float(np.asarray(after["macc"]).reshape(-1)[0]) - up.macc)
                 / bounds.scalar(up.terms["macc"]))
        Lk = unpack(after["L"], d)
        kept = np.array_equal(np.asarray(after["L"]), np.asarray(shared["L"])) and \
            np.array_equal(np.asarray(after["cov"]), np.asarray(shared["cov"]))
        if kept:
            q["cov"] = 0.0
            q["factor"] = 0.0
            q["keep"] = float(np.inf) if up.refactored and up.pivot_ratio >= PIVOT_RATIO else 0.0
        else:
            covk = unpack_sym(after["cov"], d)
            q["cov"] = float(np.max(np.abs(covk - up.cov_new) / (COV_RTOL * np.abs(up.cov_new))))
            q["factor"] = float(np.max(np.abs(Lk @ Lk.T - up.cov_new) / bounds.factor(Lk, up.cov_new, d)))
            if not np.all(np.diagonal(Lk) > 0):
                q["factor"] = float(np.inf)
            q["keep"] = 0.0
        lamk = float(np.asarray(after["lam"]).reshape(-1)[0])
        asc_ref = float(np.linalg.norm(Lk * math.exp(lamk) - L0 * math.exp(lam32), "fro"))
        q["asc"] = abs(float(np.asarray(after["asc"]).reshape(-1)[0]) - asc_ref) / \
            bounds.as_change(Lk, lamk, L0, lam32, asc_ref, d)
        if best is None or max(q.values()) < max(best.values()):
            best = q
    r.update(best)
    return r


def worst(r):
    """The quantities of a check_block result above their bound."""
    return {k: v for k, v in r.items() if k != "skipped" and not v <= 1.0}
