"""Pooled ASSS: the stereographic slice sampler with one adapt state shared by
all chains of all ranks (include/amh.h "pooled ASSS").

Every chain runs ASSS.sample (asss.py:210-244) with the shared (loc, scale)
in place of its own.  The adaptation (asss.py:246-255) then consumes the
pooled statistics of PooledARWMH,

    S_d = sum_c delta_c,  S_dd = sum_c delta_c delta_c^T,  S_a = sum_c a_c,

with a_c = 1 for a chain that moved and 0 for one that kept its point (the
shrinkage reached its cap, or the tangent was degenerate): mu moves by gamma *
mean delta, Sigma = L L^T is blended with the mean outer product and
refactorised (kept if not positive definite), and mean_accept_prob becomes
the running share of chain-steps that moved.  There is no step size:
log_step_size is carried unchanged.  as_change is ASSS's, ||mu' - mu|| +
||L' - L||_F.  With one chain in total this is the reference's recurrence.

The sums vector, its reduction, the all-reduce, sync_every blocks, overlap,
run and checkpoints are PooledARWMH's; only the transition
(amh_pooled_asss_stats_k) and the update (amh_pooled_asss_update_k) differ.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from .asss import ASSS
from .pooled import PooledARWMH


class PooledASSS(PooledARWMH):
    """ASSS with one adapt state shared by every chain (and every rank).

    Constructor and init arguments as PooledARWMH without the step-size
    target.  States are PooledState, so kernels_amd.checkpoint and
    infer_amd.MCMC take them unchanged.

    Limits (ValueError): d <= 64; registry potentials only (a model, or a
    posteriors.Gaussian as potential_fn), since the slice transition needs the
    potential inside the kernel; no exact_sums."""

    def __init__(self, model=None, potential_fn=None, lr_decay=2 / 3, eps=1e-6, num_chains=None, device=None,
                 chain_offset=0, group=None, sync_every: int = 1, overlap: bool = False, exact_sums: bool = False):
        if potential_fn is not None and not hasattr(potential_fn, "model_id"):
            raise ValueError("PooledASSS takes registry potentials only: the slice transition evaluates the "
                             "potential inside the kernel")
        if exact_sums:
            raise ValueError("PooledASSS has no exact fixed-point sums (exact_sums=True)")
        super().__init__(model=model, potential_fn=potential_fn, lr_decay=lr_decay, eps=eps, num_chains=num_chains,
                         device=device, chain_offset=chain_offset, group=group, sync_every=sync_every,
                         overlap=overlap)
        if self._external():
            raise ValueError("PooledASSS takes registry potentials only (not an external potential)")

    def init(self, rng_key, num_warmup, init_params, model_args, model_kwargs):
        """PooledARWMH.init: per-chain z0 / pe0 / keys, shared mu = 0, L =
        Sigma = I, i = 0."""
        d = self._model.dim(dict(model_kwargs or {})) if self._model is not None else self._potential_fn.dim
        if d > 64:
            raise ValueError(f"PooledASSS supports d <= 64, not d = {d}")
        return super().init(rng_key, num_warmup, init_params, model_args, model_kwargs)

    def _stats(self, L, cin, sout, b, C):
        dev = sout.z.device.index
        _lib.check(L.amh_pooled_asss_stats_k(self._handle.h, C, ctypes.byref(cin), self.sync_every, _lib.ptr(sout.z),
                                             _lib.ptr(sout.potential_energy), _lib.ptr(self._bufs[b]),
                                             _lib.stream_ptr(dev)), self._handle.h)

    def _update(self, L, buf, cin, cout):
        dev = buf.device.index
        _lib.check(L.amh_pooled_asss_update_k(self._handle.h, _lib.ptr(buf), ctypes.byref(cin), ctypes.byref(cout),
                                              self.sync_every, _lib.stream_ptr(dev)), self._handle.h)

    def sample_(self, state, n_steps: int = 1):
        """n_steps pooled transitions in place (a multiple of sync_every)."""
        C = self._check(state)
        K = self.sync_every
        if int(n_steps) % K != 0:
            raise ValueError(f"n_steps ({n_steps}) must be a multiple of sync_every ({K})")
        if self._world() == 1 and not self.overlap and not self.force_collective:
            dev = state.z.device.index
            c = self._c(state)
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().amh_pooled_asss_step_k(self._handle.h, C, ctypes.byref(c), ctypes.byref(c),
                                                             int(n_steps), K, _lib.ptr(self._bufs[0]),
                                                             _lib.stream_ptr(dev)), self._handle.h)
            self._sums = self._bufs[0]
            return state
        for _ in range(int(n_steps) // K):
            self._one(state, state)
        return state

    def get_diagnostics_str(self, state):
        return ASSS.get_diagnostics_str(self, state)

    def sample_Pnx(self, rng_key, x, adapt_state, n=1, n_samples=1000, jit_inner=True):
        """ASSS.sample_Pnx: a frozen shared state is exactly its argument;
        adapt_state is (loc, scale) or a PooledAdaptState."""
        return ASSS.sample_Pnx(self, rng_key, x, adapt_state, n=n, n_samples=n_samples, jit_inner=jit_inner)
