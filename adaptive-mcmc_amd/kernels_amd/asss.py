"""ASSS: adaptive stereographic slice sampler on MI355X.

Drop-in for the reference kernel python/kernels/asss.py (savelovme/
adaptive-mcmc): same constructor arguments (model XOR potential_fn, lr_decay,
eps, init_strategy), method names (init, sample, postprocess_fn,
get_diagnostics_str, sample_Pnx, get_init_adapt_state) and state namedtuples
ASSSState / ASSSAdaptState, with a leading chain axis on every leaf.  Every
transition of every chain runs in the HIP kernel amh_asss.hip (C-ABI
amh_asss_step / amh_asss_sample_pnx, include/amh.h); there is no CPU path.

A `potential_fn` that is any other callable (asss.py:105-131 takes an
arbitrary one) runs with `host_shrink=True`: the transition is cut at every
potential evaluation (amh_asss_ext.hip, C-ABI amh_asss_ext_*), the callable is
evaluated on the candidates between the launches, and the host reads once per
shrink round whether any chain still continues.

Differences a caller can see are those of ARWMH (kernels_amd/arwmh.py): torch
leaves on the GPU, packed column-major `scale`, counter-based Philox noise
(`rng_key` fixed per chain, stream position `i`), registry models.
"""
from __future__ import annotations

import ctypes
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .arwmh import ARWMH, ARWMHAdaptState, ARWMHState, _device_index, init_to_uniform, pack_scale, packed_size
from .random import as_key

ASSSState = namedtuple(
    "ASSSState",
    [
        "i",  # Iteration                                   [C] int32
        "z",  # Current point (unconstrained, flat)         [C, d]
        "potential_energy",  # Current potential energy     [C]
        "adapt_state",  # Mean & Cholesky factor estimates
        "as_change",  # ||mu' - mu|| + ||L' - L||_F           [C]
        "rng_key",  # Per-chain Philox key                  [C, 2] int32 (uint32 bits)
    ],
)

ASSSAdaptState = namedtuple("ASSSAdaptState", ["loc", "scale"])


class ASSS(ARWMH):
    """
    Adaptive Stereographic Slice Sampler kernel (reference: python/kernels/
    asss.py:99-303), batched over chains.

    Parameters (asss.py:106-136): model XOR potential_fn, lr_decay (gamma_n =
    1 / n^lr_decay, default 2/3), eps (default 1e-6), init_strategy
    (init_to_uniform only); plus num_chains, device, chain_offset as ARWMH.

    host_shrink : bool (default False).  With a `potential_fn` that is neither
        a registry potential nor a model (any torch callable z [n, d] -> U [n])
        the slice kernel cannot evaluate U inside; host_shrink=True runs the
        transition as begin / {U; shrink round} / finish launches with one
        host <-> device synchronisation per shrink round (d <= 64).  The one
        keyword the reference's constructor does not have: without it such a
        potential_fn is refused by `sample` ("device potential").
        `shrink_rounds` is the number of evaluations of the candidate block
        in the most recent transition (1 .. 51).
    """

    sample_field = "z"

    def __init__(self, model=None, potential_fn=None, lr_decay=2 / 3, eps=1e-6, init_strategy=init_to_uniform,
                 num_chains=None, device=None, chain_offset=0, host_shrink: bool = False):
        super().__init__(model=model, potential_fn=potential_fn, lr_decay=lr_decay, eps=eps,
                         init_strategy=init_strategy, num_chains=num_chains, device=device,
                         chain_offset=chain_offset)
        self._host_shrink = bool(host_shrink)
        if self._host_shrink and not self._external():
            raise ValueError("host_shrink=True is for a callable potential_fn; a model or a registry potential "
                             "runs inside the slice kernel")
        self.shrink_rounds = 0  # evaluations of the candidate block in the last transition (host_shrink)
        self._ext_buf = None    # (C, d, device) -> cand, work, pe, active of the host-driven loop

    # ------------------------------------------------------------------ state --
    @staticmethod
    def _to_asss(s: ARWMHState) -> ASSSState:
        a = s.adapt_state
        return ASSSState(s.i, s.z, s.potential_energy, ASSSAdaptState(a.loc, a.scale), s.as_change, s.rng_key)

    @staticmethod
    def _c_state(s) -> _lib.AmhState:
        if isinstance(s, ARWMHState):  # ARWMH.init's output, before conversion
            return ARWMH._c_state(s)
        a = s.adapt_state
        return _lib.AmhState(s.i.data_ptr(), s.z.data_ptr(), s.potential_energy.data_ptr(), None,
                             a.loc.data_ptr(), a.scale.data_ptr(), None, s.as_change.data_ptr(),
                             s.rng_key.data_ptr())

    def _alloc(self, C: int, d: int, device) -> ASSSState:
        f = dict(dtype=torch.float32, device=device)
        return ASSSState(torch.empty(C, dtype=torch.int32, device=device), torch.empty(C, d, **f),
                         torch.empty(C, **f), ASSSAdaptState(torch.empty(C, d, **f), torch.empty(C, packed_size(d), **f)),
                         torch.empty(C, **f), torch.empty(C, 2, dtype=torch.int32, device=device))

    def _check(self, s: ASSSState) -> int:
        if self._handle is None:
            raise RuntimeError("call init() first")
        d, C = self._dim, s.z.shape[0]
        leaves = [(s.i, (C,), torch.int32), (s.z, (C, d), torch.float32), (s.potential_energy, (C,), torch.float32),
                  (s.adapt_state.loc, (C, d), torch.float32),
                  (s.adapt_state.scale, (C, packed_size(d)), torch.float32), (s.as_change, (C,), torch.float32),
                  (s.rng_key, (C, 2), torch.int32)]
        for t, shape, dt in leaves:
            _lib.require_gpu(t)
            if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous():
                raise ValueError(f"state leaf has shape {tuple(t.shape)} {t.dtype}, expected {shape} {dt}")
        return C

    # -------------------------------------------------------------------- API --
    def init(self, rng_key, num_warmup, init_params, model_args, model_kwargs):
        """asss.py:138-189: z0 (init_to_uniform unless init_params), pe0 = U(z0),
        loc = z0, scale = I, i = 0, as_change = 0."""
        if self._model is None and init_params is None:
            raise ValueError("Valid value of `init_params` must be provided with `potential_fn`.")
        st = super().init(rng_key, num_warmup, init_params, model_args, model_kwargs)
        if self._host_shrink and self._dim > 64:
            raise ValueError("ASSS(host_shrink=True) supports d <= 64")
        if self._dim > 64 and not self._big_ok():
            raise ValueError("ASSS supports d <= 64, or the dense Gaussian up to d = 256")
        return self._to_asss(st)

    def _big_ok(self) -> bool:
        """64 < d <= 256: the large-d kernel (amh_big.hip asss_big_step_kernel)
        takes the dense Gaussian at any such d (the reference has no dimension
        limit, asss.py:192-269; other models stop at d = 64)."""
        mid = self._model.model_id if self._model is not None else getattr(self._potential_fn, "model_id", None)
        return mid == _lib.AMH_MODEL_GAUSSIAN and self._dim <= 256

    def sample(self, state, model_args=(), model_kwargs=None):
        """asss.py:191-258: one transition of every chain; returns a new state."""
        C = self._check(state)
        out = self._alloc(C, self._dim, state.z.device)
        self._launch(state, out, 1, None)
        return out

    def sample_(self, state, n_steps: int = 1):
        """In-place variant: advance `state` by n_steps (one fused launch)."""
        self._check(state)
        self._launch(state, state, n_steps, None)
        return state

    def run(self, state, n_steps: int, thinning: int = 1, collect_z: bool = True, collect_pe: bool = False):
        """Fused n_steps transitions; returns (new_state, z [n_steps // thinning, C, d]
        or None, pe or None)."""
        C = self._check(state)
        out = self._alloc(C, self._dim, state.z.device)
        keep = n_steps // thinning
        dev = state.z.device
        cz = torch.empty(keep, C, self._dim, dtype=torch.float32, device=dev) if collect_z and keep else None
        cp = torch.empty(keep, C, dtype=torch.float32, device=dev) if collect_pe and keep else None
        self._launch(state, out, n_steps, (cz, cp, thinning))
        return out, cz, cp

    # ----------------------------------------- host-driven shrink loop --
    def _ext_buffers(self, C: int, d: int, dev):
        """cand [2, C, d], work [C, amh_asss_ext_work_size(d)], pe [2, C] and
        active [51]: allocated once per (C, d, device) and reused."""
        key = (C, d, dev)
        if self._ext_buf is None or self._ext_buf[0] != key:
            n = ctypes.c_int64(0)
            _lib.check(_lib.lib().amh_asss_ext_work_size(d, ctypes.byref(n)))
            f = dict(dtype=torch.float32, device=dev)
            self._ext_buf = (key, torch.empty(2, C, d, **f), torch.empty(C, n.value, **f), torch.empty(2, C, **f),
                             torch.zeros(_lib.AMH_ASSS_EXT_ROUNDS, dtype=torch.int32, device=dev))
        return self._ext_buf[1:]

    def _shrink_loop(self, C, d, bufs, st):
        """U of cand [2C, d], round 0, then U of cand[1] and the next round
        while any chain continued: one read of active[r] per round."""
        cand, work, pe, active = bufs
        L, h = _lib.lib(), self._handle.h
        pe.view(-1).copy_(self._potential_fn.evaluate(cand.view(2 * C, d)))
        r = 0
        while True:
            _lib.check(L.amh_asss_ext_shrink(h, C, _lib.ptr(pe), r, _lib.ptr(cand), _lib.ptr(work), _lib.ptr(active),
                                             st), h)
            if int(active[r]) == 0:  # the round's one host <-> device synchronisation
                break
            if r + 1 >= _lib.AMH_ASSS_EXT_ROUNDS:
                raise RuntimeError("ASSS host shrink loop: chains still continue after the last round")
            r += 1
            pe[1].copy_(self._potential_fn.evaluate(cand[1]))
        self.shrink_rounds = r + 1

    def _launch_host_shrink(self, sin, sout, n_steps, collect):
        """Per transition: amh_asss_ext_begin, the shrink loop around the
        caller's U, amh_asss_ext_finish; collection as the fused launch."""
        cz, cp, thin = collect if collect is not None else (None, None, 1)
        C, d, dev = sin.z.shape[0], self._dim, sin.z.device
        bufs = self._ext_buffers(C, d, dev)
        cand, work, _, active = bufs
        L, h = _lib.lib(), self._handle.h
        with torch.cuda.device(dev.index):
            st = _lib.stream_ptr(dev.index)
            for t in range(int(n_steps)):
                src = self._c_state(sin if t == 0 else sout)
                _lib.check(L.amh_asss_ext_begin(h, C, src, _lib.ptr(cand), _lib.ptr(work), _lib.ptr(active), st), h)
                self._shrink_loop(C, d, bufs, st)
                keep = (t + 1) % thin == 0
                k = t // thin
                col = _lib.AmhCollect(cz[k].data_ptr() if (keep and cz is not None) else None,
                                      cp[k].data_ptr() if (keep and cp is not None) else None, None, 1)
                _lib.check(L.amh_asss_ext_finish(h, C, src, self._c_state(sout), _lib.ptr(cand), _lib.ptr(work), col,
                                                 st), h)

    def _launch(self, sin, sout, n_steps, collect):
        if self._host_shrink:
            return self._launch_host_shrink(sin, sout, n_steps, collect)
        cz, cp, thin = collect if collect is not None else (None, None, 1)
        col = _lib.AmhCollect(cz.data_ptr() if cz is not None else None,
                              cp.data_ptr() if cp is not None else None, None, thin)
        dev = sin.z.device.index
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().amh_asss_step(self._handle.h, sin.z.shape[0], self._c_state(sin),
                                                self._c_state(sout), n_steps, col, _lib.stream_ptr(dev)),
                       self._handle.h)

    def get_diagnostics_str(self, state):
        """asss.py:264-265 (chain-averaged potential energy for a batch)."""
        return f"Iteration: {int(state.i.max())}, Potential Energy: {float(state.potential_energy.mean()):.2f}"

    def sample_Pnx(self, rng_key, x, adapt_state, n=1, n_samples=1000, jit_inner=True):
        """asss.py:267-296: n frozen-kernel transitions from every x[i] for
        n_samples chains each, sharing adapt_state = (loc, scale); returns
        [n_points, n_samples, d]."""
        host_shrink = getattr(self, "_host_shrink", False)  # (PooledASSS borrows this method)
        if host_shrink and self._handle is None and self._potential_fn.dim is None:
            # no init() (asss.py:271-303 needs none): a callable's dimension is the adapt state's
            shape = tuple(np.shape(adapt_state[0].cpu() if hasattr(adapt_state[0], "cpu") else adapt_state[0]))
            self._potential_fn.dim = int(shape[-1]) if shape else 1
        self._ensure_bound()
        dev = torch.device("cuda", _device_index(self._device))
        d = self._dim

        def host(a):
            return torch.as_tensor(a.cpu() if hasattr(a, "cpu") else np.asarray(a), dtype=torch.float32)

        x = host(x).reshape(-1, d).to(dev).contiguous()
        loc, scale = adapt_state[0], adapt_state[1]
        scale = host(scale)
        if scale.dim() >= 2 and scale.shape[-1] == d and scale.shape[-2] == d:
            scale = pack_scale(scale.reshape(-1, d, d)[0])
        scale = scale.reshape(-1)[:packed_size(d)].to(dev).contiguous()
        loc = host(loc).reshape(-1)[:d].to(dev).contiguous()
        if host_shrink:
            return self._sample_pnx_host_shrink(rng_key, x, loc, scale, int(n), int(n_samples), dev)
        out = torch.empty(x.shape[0], n_samples, d, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev.index):
            _lib.check(_lib.lib().amh_asss_sample_pnx(self._handle.h, _lib.key_arr(as_key(rng_key)), _lib.ptr(x),
                                                      x.shape[0], n_samples, _lib.ptr(loc), _lib.ptr(scale), n,
                                                      _lib.ptr(out), _lib.stream_ptr(dev.index)), self._handle.h)
        return out

    def _sample_pnx_host_shrink(self, rng_key, x, loc, scale, n, n_samples, dev):
        """sample_Pnx with the caller's potential: transition t of every chain
        is amh_asss_ext_pnx_begin, the shrink loop, amh_asss_ext_pnx_finish."""
        d, npts = self._dim, x.shape[0]
        C = npts * n_samples
        z = x.repeat_interleave(n_samples, dim=0).contiguous()  # chain p * n_samples + s starts at x[p]
        bufs = self._ext_buffers(C, d, dev)
        cand, work, _, active = bufs
        key = _lib.key_arr(as_key(rng_key))
        L, h = _lib.lib(), self._handle.h
        with torch.cuda.device(dev.index):
            st = _lib.stream_ptr(dev.index)
            for t in range(n):
                _lib.check(L.amh_asss_ext_pnx_begin(h, key, _lib.ptr(z), C, _lib.ptr(loc), _lib.ptr(scale), t,
                                                    _lib.ptr(cand), _lib.ptr(work), _lib.ptr(active), st), h)
                self._shrink_loop(C, d, bufs, st)
                _lib.check(L.amh_asss_ext_pnx_finish(h, C, _lib.ptr(cand), _lib.ptr(work), _lib.ptr(z), st), h)
        return z.reshape(npts, n_samples, d)

    def get_init_adapt_state(self, rng_key, init_params, model_args=(), model_kwargs={}):
        """asss.py:298-303."""
        return self.init(rng_key, 0, init_params, model_args, model_kwargs).adapt_state
