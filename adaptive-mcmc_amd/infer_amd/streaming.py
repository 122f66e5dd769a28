"""Streaming posterior summaries: running statistics of many chains whose
memory does not grow with the number of draws.

`StreamingSummary` folds blocks of draws x [B, C, k] (the layout of the
collect buffer that ARWMH.run / ASSS.run / PooledARWMH.run fill) into

  acc  [5, C, k] float64   S1, S2, bs, S1b, Q per (chain, column): sums of the
                           centred draws y = x - center, of y^2, the open
                           batch's sum, and the sums of the closed batches'
                           sums and of their squares (batch length b)
  hist [k, nbins + 3] int64  per column, pooled over chains: an under bin,
                           nbins equal bins over [lo, lo + nbins w), an over
                           bin and a NaN bin

with one pass of one HIP kernel per block (csrc/amh_summary.hip,
amh_summary_update; DESIGN.md 7.1 is the bit spec and tests/summary_np.py its
numpy mirror).  The moments of an element are summed in draw order and the
counts are integers, so the state after a stream does not depend on how the
draws were split into blocks, and a state_dict round trip resumes exactly.

`summary()` finalises in float64, with N draws per chain, C chains,
ybar_c = S1 / N and ss_c = max(S2 - S1 ybar_c, 0):

  mean           center + mean_c ybar_c
  std            sqrt([sum_c ss_c + N sum_c (ybar_c - mean_c ybar_c)^2] / (C N))
                 (ddof 0 over all draws, as numpyro's table)
  r_hat          sqrt(var+ / W), W = mean_c ss_c / (N - 1),
                 B = var_c(ybar_c, ddof 1), var+ = W (N - 1) / N + B
                 (diagnostics.gelman_rubin, its C = 1 branch included)
  n_eff          C N W / mean_c sigma2_c with the batch-means variance
                 sigma2_c = b / (a - 1) (Q / b^2 - S1b^2 / (a b^2)) over the
                 a = N // b complete batches; NaN when a < 2
  n_eff_between  C var+ / B, from the spread of the chain means; NaN at C = 1
  quantiles      from the pooled histogram: with n = C N - nan and
                 r = ceil(p n), the bin where the cumulative count first
                 reaches r, interpolated linearly inside it; -inf / +inf when
                 that is the under / over bin

Three differences from `diagnostics.summary` (the stored-draws table):
the interval printed from quantiles is EQUAL-TAILED, not the HPDI; `r_hat` is
NOT SPLIT (chains are not halved); `n_eff` is BATCH MEANS, not Geyer's
initial-sequence estimator.  A quantile is exact to one bin width w = 2 hw /
nbins (calibrate: hw = 8 std by default, so w = std / 32 at 512 bins).

Multi-rank merging of summaries is not provided.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from kernels_amd import _lib

__all__ = ["StreamingSummary", "format_streaming_summary", "SUMMARY_NOTE"]

SUMMARY_NOTE = ("streaming summary: the interval is equal-tailed (not the HPDI), r_hat is not split, "
                "n_eff is batch means (not Geyer's estimator)")


def _as_f64(a, k, name):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.asarray(a, dtype=np.float64)
    if a.shape != (k,):
        raise ValueError(f"{name} must have shape ({k},), got {a.shape}")
    return a


class StreamingSummary:
    """Running mean / std / r_hat / n_eff / quantiles of C chains x k columns."""

    def __init__(self, num_chains, num_cols, *, batch, nbins=512, device):
        C, k, b, nb = int(num_chains), int(num_cols), int(batch), int(nbins)
        if C < 1:
            raise ValueError("num_chains must be >= 1")
        if not 1 <= k <= 1024:
            raise ValueError("num_cols must be in 1 .. 1024")
        if b < 1:
            raise ValueError("batch must be >= 1")
        if nb < 64 or nb > 2048 or nb & (nb - 1):
            raise ValueError("nbins must be a power of two in 64 .. 2048")
        self.num_chains, self.num_cols, self.batch, self.nbins = C, k, b, nb
        self.device = torch.device(device)
        self.acc = torch.zeros(5, C, k, dtype=torch.float64, device=self.device)
        self.hist = torch.zeros(k, nb + 3, dtype=torch.int64, device=self.device)
        self.calib = None  # [3, k] float32 on the device: center, lo, inv_w
        self.n_draws = 0

    # ----------------------------------------------------------- calibration --
    def set_range(self, center, half_width):
        """Histogram of column j over [center_j - hw_j, center_j + hw_j); the
        moments are centred at center_j."""
        if self.n_draws:
            raise ValueError("set_range after update: the accumulators are tied to the calibration")
        k = self.num_cols
        c = _as_f64(center, k, "center")
        hw = _as_f64(half_width, k, "half_width")
        for j in range(k):
            if not math.isfinite(c[j]):
                raise ValueError(f"column {j}: center {c[j]} is not finite")
            if not (math.isfinite(hw[j]) and hw[j] > 0):
                raise ValueError(f"column {j}: half_width {hw[j]} must be finite and > 0")
        lo = c - hw
        w = 2.0 * hw / self.nbins
        with np.errstate(over="ignore", divide="ignore"):
            cal = np.stack([c, lo, 1.0 / w]).astype(np.float32)  # rounded once
        for j in range(k):
            if not (np.isfinite(cal[:, j]).all() and cal[2, j] > 0):
                raise ValueError(f"column {j}: the calibration (center {c[j]}, half_width {hw[j]}) leaves float32")
        self.calib = torch.as_tensor(cal, device=self.device)
        return self

    def calibrate(self, x, span=8.0):
        """center = mean, half_width = span * std (ddof 0) of every value of a
        column of x [..., k]."""
        if not isinstance(x, torch.Tensor) or x.ndim < 1 or x.shape[-1] != self.num_cols:
            raise ValueError(f"calibrate needs a tensor [..., {self.num_cols}]")
        x64 = x.detach().reshape(-1, self.num_cols).to(torch.float64)
        if x64.shape[0] < 1:
            raise ValueError("calibrate needs at least one row")
        center = x64.mean(dim=0)
        std = x64.std(dim=0, unbiased=False).cpu().numpy()
        for j in range(self.num_cols):
            if not (math.isfinite(std[j]) and std[j] > 0):
                raise ValueError(f"column {j}: std {std[j]} of the calibration draws is zero or not finite")
        return self.set_range(center.cpu().numpy(), float(span) * std)

    # ---------------------------------------------------------------- update --
    def update(self, block):
        """Fold in B draws of every chain: block [B, C, k] (or [C, k])."""
        C, k = self.num_chains, self.num_cols
        if not isinstance(block, torch.Tensor):
            raise ValueError("block must be a torch tensor")
        if block.dtype != torch.float32:
            raise ValueError(f"block must be float32, got {block.dtype}")
        if block.ndim == 2:
            block = block.unsqueeze(0)
        if block.ndim != 3 or block.shape[0] < 1 or tuple(block.shape[1:]) != (C, k):
            raise ValueError(f"block must be [B >= 1, {C}, {k}] or [{C}, {k}], got {tuple(block.shape)}")
        if not block.is_contiguous():
            raise ValueError("block must be contiguous")
        if self.calib is None:
            raise ValueError("not calibrated: call set_range() or calibrate() first")
        if block.device != self.acc.device:
            raise ValueError(f"block is on {block.device}, the summary on {self.acc.device}")
        _lib.require_gpu(block)
        B = int(block.shape[0])
        dev = block.device.index
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().amh_summary_update(_lib.ptr(block), B, C, k, _lib.ptr(self.calib), self.nbins,
                                                     self.batch, self.n_draws, _lib.ptr(self.acc),
                                                     _lib.ptr(self.hist), _lib.stream_ptr(dev)))
        self.n_draws += B
        return self

    # --------------------------------------------------------------- results --
    def summary(self, probs=(0.05, 0.5, 0.95)):
        """dict of float64 numpy arrays [k] (quantiles: [len(probs), k])."""
        if self.calib is None or self.n_draws < 1:
            raise RuntimeError("no draws folded in yet")
        C, N, b = self.num_chains, self.n_draws, self.batch
        S1, S2, _, S1b, Q = self.acc.unbind(0)
        cal = self.calib.to(torch.float64)
        nan = torch.full_like(cal[0], float("nan"))
        ybar = S1 / N
        ss = torch.clamp(S2 - S1 * ybar, min=0.0)
        grand = ybar.mean(dim=0)
        dev2 = (ybar - grand) ** 2
        var0 = (ss.sum(dim=0) + N * dev2.sum(dim=0)) / (C * N)
        W = ss.mean(dim=0) / (N - 1) if N > 1 else nan
        var_plus = W * (N - 1) / N
        if C > 1:
            Bv = dev2.sum(dim=0) / (C - 1)
            var_plus = var_plus + Bv
            r_hat = torch.sqrt(var_plus / W)
            n_eff_between = C * var_plus / Bv
        else:
            r_hat = torch.sqrt(var_plus / var_plus)
            n_eff_between = nan
        a = N // b
        if a >= 2:
            sig2 = (b / (a - 1)) * (Q / (b * b) - S1b * S1b / (a * b * b))
            n_eff = C * N * W / sig2.mean(dim=0)
        else:
            n_eff = nan
        hist = self.hist.cpu().numpy()
        lo = cal[1].cpu().numpy()
        w = 1.0 / cal[2].cpu().numpy()
        nb = self.nbins
        n = C * N - hist[:, nb + 2]
        cum = np.cumsum(hist[:, :nb + 2], axis=1)
        q = np.empty((len(probs), self.num_cols), np.float64)
        for i, p in enumerate(probs):
            if not 0.0 <= float(p) <= 1.0:
                raise ValueError("probs must lie in [0, 1]")
            for j in range(self.num_cols):
                if n[j] == 0:
                    q[i, j] = np.nan
                    continue
                r = max(1, math.ceil(float(p) * int(n[j])))
                bin_ = int(np.searchsorted(cum[j], r, side="left"))
                if bin_ == 0:
                    q[i, j] = -np.inf
                elif bin_ >= nb + 1:
                    q[i, j] = np.inf
                else:
                    before = int(cum[j, bin_ - 1])
                    q[i, j] = lo[j] + w[j] * ((bin_ - 1) + (r - before) / int(hist[j, bin_]))

        def host(t):
            return t.cpu().numpy()

        return {"mean": host(cal[0] + grand), "std": host(torch.sqrt(var0)), "r_hat": host(r_hat),
                "n_eff": host(n_eff), "n_eff_between": host(n_eff_between), "quantiles": q, "n_draws": N,
                "below": hist[:, 0].copy(), "above": hist[:, nb + 1].copy(), "nan": hist[:, nb + 2].copy()}

    # ----------------------------------------------------------------- state --
    def state_dict(self):
        return {"num_chains": self.num_chains, "num_cols": self.num_cols, "batch": self.batch, "nbins": self.nbins,
                "n_draws": self.n_draws, "acc": self.acc.detach().cpu().clone(),
                "hist": self.hist.detach().cpu().clone(),
                "calib": None if self.calib is None else self.calib.detach().cpu().clone()}

    def load_state_dict(self, sd):
        for name in ("num_chains", "num_cols", "batch", "nbins"):
            if int(sd[name]) != getattr(self, name):
                raise ValueError(f"state_dict has {name}={sd[name]}, this summary {getattr(self, name)}")
        if tuple(sd["acc"].shape) != tuple(self.acc.shape) or tuple(sd["hist"].shape) != tuple(self.hist.shape):
            raise ValueError("state_dict: accumulator shapes do not match")
        self.acc.copy_(sd["acc"])
        self.hist.copy_(sd["hist"])
        self.calib = None if sd["calib"] is None else sd["calib"].to(device=self.device, dtype=torch.float32).clone()
        self.n_draws = int(sd["n_draws"])
        return self


def format_streaming_summary(summary, labels, prob=0.9, cols=None):
    """The table layout of diagnostics.format_summary from a summary() whose
    quantiles are those at (1 - prob) / 2, 0.5, (1 + prob) / 2, followed by
    the note on the three differences.  labels name the columns `cols`
    (default: all, in order)."""
    cols = list(range(len(labels))) if cols is None else list(cols)
    lo_name, hi_name = "{:.1f}%".format(50 * (1 - prob)), "{:.1f}%".format(50 * (1 + prob))
    w = max(max(len(s) for s in labels), 10)
    name_f = "{:>" + str(w) + "}"
    lines = ["", (name_f + " {:>9}" * 7).format("", "mean", "std", "median", lo_name, hi_name, "n_eff", "r_hat")]
    row_f = name_f + " {:>9.2f}" * 7
    q = summary["quantiles"]
    for name, j in zip(labels, cols):
        lines.append(row_f.format(name, summary["mean"][j], summary["std"][j], q[1, j], q[0, j], q[2, j],
                                  summary["n_eff"][j], summary["r_hat"][j]))
    lines.append("")
    lines.append(SUMMARY_NOTE)
    lines.append("")
    return "\n".join(lines)
