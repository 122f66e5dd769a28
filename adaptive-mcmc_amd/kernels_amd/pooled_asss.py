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

A `potential_fn` that is any other callable runs with `host_shrink=True`, as
on ASSS: each transition of a block is amh_pooled_asss_ext_begin (the shared
factor from LDS, the candidates and the chains' records), the host-driven
shrink loop of ASSS around the callable (amh_asss_ext_shrink, unchanged), and
amh_pooled_asss_ext_finish (the outcome and the transition's sums, in the
fused kernel's chunks).  With sync_every = K the block's sums are s_0 + s_1 +
... in step order (PooledARWMH's rule for a callable); the update is
amh_pooled_asss_ext_update.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from .asss import ASSS
from .pooled import PooledARWMH


class PooledASSS(PooledARWMH):
    """ASSS with one adapt state shared by every chain (and every rank).

    Constructor and init arguments as PooledARWMH without the step-size
    target.  States are PooledState, so kernels_amd.checkpoint and
    infer_amd.MCMC take them unchanged.

    host_shrink : bool (default False), as on ASSS: True is for a
        `potential_fn` that is neither a model nor a registry potential (any
        batched torch callable z [n, d] -> U [n]); the transition then runs as
        begin / {U; shrink round} / finish launches with one host <-> device
        synchronisation per shrink round.  `shrink_rounds` is the number of
        evaluations of the candidate block in the most recent transition
        (1 .. 51).

    Limits (ValueError): d <= 64; a callable potential_fn needs
    host_shrink=True (the fused slice transition evaluates the potential
    inside the kernel), and host_shrink=True needs a callable; no
    exact_sums; not the logistic_regression model (the pooled slice kernel has
    no instantiation for it; poisson_regression has one)."""

    def __init__(self, model=None, potential_fn=None, lr_decay=2 / 3, eps=1e-6, num_chains=None, device=None,
                 chain_offset=0, group=None, sync_every: int = 1, overlap: bool = False, exact_sums: bool = False,
                 host_shrink: bool = False):
        callable_fn = potential_fn is not None and not hasattr(potential_fn, "model_id")
        self._host_shrink = bool(host_shrink)
        if callable_fn and not self._host_shrink:
            raise ValueError("PooledASSS evaluates a registry potential inside the slice kernel; a callable "
                             "potential_fn needs host_shrink=True")
        if self._host_shrink and not callable_fn:
            raise ValueError("host_shrink=True is for a callable potential_fn; a model or a registry potential "
                             "runs inside the slice kernel")
        if model is not None and getattr(model, "model_id", None) == _lib.AMH_MODEL_LOGISTIC:
            raise ValueError("PooledASSS has no slice kernel for the logistic_regression model (the pooled slice "
                             "kernels are instantiated per model); use ASSS, PooledARWMH, or its potential as a "
                             "callable with host_shrink=True")
        if exact_sums:
            raise ValueError("PooledASSS has no exact fixed-point sums (exact_sums=True)")
        super().__init__(model=model, potential_fn=potential_fn, lr_decay=lr_decay, eps=eps, num_chains=num_chains,
                         device=device, chain_offset=chain_offset, group=group, sync_every=sync_every,
                         overlap=overlap)
        self.shrink_rounds = 0  # evaluations of the candidate block in the last transition (host_shrink)
        self._ext_buf = None    # ASSS._ext_buffers: cand, work, pe, active of the host-driven loop

    def init(self, rng_key, num_warmup, init_params, model_args, model_kwargs):
        """PooledARWMH.init: per-chain z0 / pe0 / keys, shared mu = 0, L =
        Sigma = I, i = 0."""
        if self._model is None and init_params is None:
            raise ValueError("Valid value of `init_params` must be provided with `potential_fn`.")
        d = self._model.dim(dict(model_kwargs or {})) if self._model is not None else self._potential_fn.dim
        if d is None:  # a callable: its dimension is init_params' (ARWMH.init)
            x = init_params.cpu() if hasattr(init_params, "cpu") else np.asarray(init_params)
            d = int(np.asarray(x).shape[-1]) if np.ndim(x) else 1
        if d > 64:
            raise ValueError(f"PooledASSS supports d <= 64, not d = {d}")
        return super().init(rng_key, num_warmup, init_params, model_args, model_kwargs)

    # (ASSS.sample_Pnx's host-driven form, borrowed with the method below)
    _sample_pnx_host_shrink = ASSS._sample_pnx_host_shrink
    _ext_buffers = ASSS._ext_buffers
    _shrink_loop = ASSS._shrink_loop

    def _stats_host_shrink(self, L, cin, sout, b, C):
        """A callable potential: the block's K transitions, each
        amh_pooled_asss_ext_begin, ASSS's shrink loop around the caller's U
        and amh_pooled_asss_ext_finish, whose sums are added to the block's in
        step order.  Transitions after the first read the z / pe the previous
        finish wrote, with the frozen shared state of `cin`."""
        dev = sout.z.device
        h, st = self._handle.h, _lib.stream_ptr(dev.index)
        bufs = self._ext_buffers(C, self._dim, dev)
        cand, work, _, active = bufs
        cur = cin
        for t in range(self.sync_every):
            _lib.check(L.amh_pooled_asss_ext_begin(h, C, ctypes.byref(cur), t, _lib.ptr(cand), _lib.ptr(work),
                                                   _lib.ptr(active), st), h)
            self._shrink_loop(C, self._dim, bufs, st)
            _lib.check(L.amh_pooled_asss_ext_finish(h, C, ctypes.byref(cur), _lib.ptr(cand), _lib.ptr(work),
                                                    _lib.ptr(sout.z), _lib.ptr(sout.potential_energy),
                                                    _lib.ptr(self._bufs[b]), int(t > 0), st), h)
            if t == 0 and self.sync_every > 1:
                cur = _lib.AmhPooledState.from_buffer_copy(cin)
                cur.z, cur.potential_energy = sout.z.data_ptr(), sout.potential_energy.data_ptr()

    def _stats(self, L, cin, sout, b, C):
        dev = sout.z.device.index
        if self._host_shrink:
            return self._stats_host_shrink(L, cin, sout, b, C)
        _lib.check(L.amh_pooled_asss_stats_k(self._handle.h, C, ctypes.byref(cin), self.sync_every, _lib.ptr(sout.z),
                                             _lib.ptr(sout.potential_energy), _lib.ptr(self._bufs[b]),
                                             _lib.stream_ptr(dev)), self._handle.h)

    def _update(self, L, buf, cin, cout):
        dev = buf.device.index
        entry = L.amh_pooled_asss_ext_update if self._host_shrink else L.amh_pooled_asss_update_k
        _lib.check(entry(self._handle.h, _lib.ptr(buf), ctypes.byref(cin), ctypes.byref(cout), self.sync_every,
                         _lib.stream_ptr(dev)), self._handle.h)

    def sample_(self, state, n_steps: int = 1):
        """n_steps pooled transitions in place (a multiple of sync_every)."""
        C = self._check(state)
        K = self.sync_every
        if int(n_steps) % K != 0:
            raise ValueError(f"n_steps ({n_steps}) must be a multiple of sync_every ({K})")
        if self._world() == 1 and not self.overlap and not self.force_collective and not self._host_shrink:
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
