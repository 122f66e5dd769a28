"""numpy mirror of the streaming-summary bit spec: the
accumulators and the histogram that csrc/amh_summary.hip must reproduce byte
for byte, and the float64 finalisation that StreamingSummary.summary() must
match to rounding."""
import math

import numpy as np


def calibration(center, half_width, nbins):
    """[3][k] float32: center, lo = center - hw, inv_w = nbins / (2 hw), each
    computed in float64 and rounded once."""
    c = np.asarray(center, np.float64)
    hw = np.asarray(half_width, np.float64)
    lo = c - hw
    w = 2.0 * hw / nbins
    return np.stack([c, lo, 1.0 / w]).astype(np.float32)


class State:
    def __init__(self, C, k, batch, nbins, calib):
        self.C, self.k, self.batch, self.nbins = C, k, int(batch), int(nbins)
        self.calib = np.asarray(calib, np.float32).reshape(3, k)
        self.acc = np.zeros((5, C, k), np.float64)  # S1, S2, bs, S1b, Q
        self.hist = np.zeros((k, nbins + 3), np.int64)
        self.n = 0


def bins(x, calib, nbins):
    """The bin of every element of x [..., k] (float32 arithmetic)."""
    x = np.asarray(x, np.float32)
    lo, inv_w = calib[1].astype(np.float32), calib[2].astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (x - lo).astype(np.float32)
        t = (d * inv_w).astype(np.float32)
    inner = (t >= 0) & (t < np.float32(nbins))
    idx = 1 + np.where(inner, t, 0).astype(np.int64)  # C's (int): truncation
    out = np.where(t < 0, 0, np.where(t >= np.float32(nbins), nbins + 1, idx))
    return np.where(np.isnan(t), nbins + 2, out).astype(np.int64)


def update(st, block):
    """Fold block [B][C][k] float32 into st, in draw order."""
    x = np.asarray(block, np.float32)
    if x.ndim == 2:
        x = x[None]
    assert x.shape[1:] == (st.C, st.k)
    S1, S2, bs, S1b, Q = st.acc
    center = st.calib[0].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(x.shape[0]):
            y = x[t].astype(np.float64) - center
            S1 += y
            S2 += y * y
            bs += y
            if (st.n + t + 1) % st.batch == 0:
                S1b += bs
                Q += bs * bs
                bs[...] = 0.0
    b = bins(x, st.calib, st.nbins)
    for j in range(st.k):
        st.hist[j] += np.bincount(b[..., j].ravel(), minlength=st.nbins + 3)
    st.n += x.shape[0]
    return st


def finalise(st, probs=(0.05, 0.5, 0.95)):
    C, N, b, nb = st.C, st.n, st.batch, st.nbins
    S1, S2, _, S1b, Q = st.acc
    cal = st.calib.astype(np.float64)
    nan = np.full(st.k, np.nan)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ybar = S1 / N
        ss = np.maximum(S2 - S1 * ybar, 0.0)
        grand = ybar.mean(axis=0)
        dev2 = (ybar - grand) ** 2
        var0 = (ss.sum(axis=0) + N * dev2.sum(axis=0)) / (C * N)
        W = ss.mean(axis=0) / (N - 1) if N > 1 else nan
        var_plus = W * (N - 1) / N
        if C > 1:
            Bv = dev2.sum(axis=0) / (C - 1)
            var_plus = var_plus + Bv
            r_hat = np.sqrt(var_plus / W)
            between = C * var_plus / Bv
        else:
            r_hat = np.sqrt(var_plus / var_plus)
            between = nan
        a = N // b
        if a >= 2:
            sig2 = (b / (a - 1)) * (Q / (b * b) - S1b * S1b / (a * b * b))
            n_eff = C * N * W / sig2.mean(axis=0)
        else:
            n_eff = nan
    lo, w = cal[1], 1.0 / cal[2]
    q = np.empty((len(probs), st.k))
    for j in range(st.k):
        n = C * N - int(st.hist[j, nb + 2])
        cum = np.cumsum(st.hist[j, :nb + 2])
        for i, p in enumerate(probs):
            if n == 0:
                q[i, j] = np.nan
                continue
            r = max(1, math.ceil(p * n))
            bin_ = int(np.argmax(cum >= r))
            if bin_ == 0:
                q[i, j] = -np.inf
            elif bin_ == nb + 1:
                q[i, j] = np.inf
            else:
                q[i, j] = lo[j] + w[j] * ((bin_ - 1) + (r - int(cum[bin_ - 1])) / int(st.hist[j, bin_]))
    return {"mean": cal[0] + grand, "std": np.sqrt(var0), "r_hat": r_hat, "n_eff": n_eff, "n_eff_between": between,
            "quantiles": q, "n_draws": N, "below": st.hist[:, 0].copy(), "above": st.hist[:, nb + 1].copy(),
            "nan": st.hist[:, nb + 2].copy()}
