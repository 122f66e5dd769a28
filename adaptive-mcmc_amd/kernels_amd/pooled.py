"""Pooled-covariance ARWMH (regime B): one shared adapt state for all chains
of all ranks (include/amh.h, amh_pooled_*).

Every chain proposes with the shared (loc, scale, log_step_size) exactly as
ARWMH.sample does with its own (arwmh.py:162-178).  The adaptation
(arwmh.py:180-197) then consumes the pooled statistics

    S_d = sum_c delta_c,  S_dd = sum_c delta_c delta_c^T,  S_a = sum_c alpha_c

so mu moves by gamma * mean delta, Sigma = L L^T is blended with the mean
outer product and refactorised (kept if not positive definite), and lambda
follows the mean acceptance.  With one chain in total this is the
reference's recurrence.  Across ranks the sums vector (d + d(d+1)/2 + 2
doubles) is the only exchange: one all-reduce(sum) per step (per K steps
with sync_every = K) over RCCL on xGMI, on this package's own communicator
(distributed.RcclComm) through the C ABI's amh_pooled_allreduce.
"""
from __future__ import annotations

import ctypes
import weakref
from collections import namedtuple

import torch
import torch.distributed as dist

from . import _lib
from .arwmh import ARWMH, packed_size
from .random import as_key

PooledState = namedtuple("PooledState", ["i", "z", "potential_energy", "mean_accept_prob", "adapt_state",
                                         "as_change", "rng_key", "cov"])
PooledAdaptState = namedtuple("PooledAdaptState", ["loc", "scale", "log_step_size"])


AmhPooledState = _lib.AmhPooledState


def sums_size(d: int) -> int:
    return d + packed_size(d) + 2


def pooled_chunk(dim: int, total_chains: int) -> int:
    """Chains per chunk of the pooled sums in a run of `total_chains` chains
    over all ranks (amh_pooled_chunk_chains): with exact_sums=True every
    rank's chain_offset must be a multiple, e.g. from
    distributed.shard_range(total_chains, rank, world, align=pooled_chunk(...))."""
    n = ctypes.c_int64(0)
    _lib.check(_lib.lib().amh_pooled_chunk_chains(int(dim), int(total_chains), ctypes.byref(n)))
    return n.value


def exact_size(d: int) -> int:
    """int64 words of the exact sums (amh_pooled_exact_size)."""
    n = ctypes.c_int64(0)
    _lib.check(_lib.lib().amh_pooled_exact_size(int(d), ctypes.byref(n)))
    return n.value


class PooledARWMH(ARWMH):
    """ARWMH with one adapt state shared by every chain (and every rank).

    Same constructor and init arguments as ARWMH; `group` is the
    torch.distributed process group whose chains are pooled (default: the
    default group when initialised, else this process alone).

    potential_fn may be a registry potential (fused into the pooled kernels)
    or any batched torch callable z [n, d] -> U [n], at the pooled mode's
    dimensions (d <= 64 or a multiple of 32 up to 256).  A callable runs
    between two launches per transition: amh_pooled_propose writes every
    chain's proposal with the shared state, the callable evaluates U there,
    and amh_pooled_stats_external accepts and forms the step's sums, bit for
    bit what the fused kernels give for the same U.  A block of sync_every =
    K steps is K such rounds, the block's sums s_0 + s_1 + ... in step order
    (up to d = 64 the fused kernels associate a block's sums
    differently).  Everything after the sums (all-reduce, update, overlap) is
    shared with the registry path.

    sync_every = K pools every K transitions: the shared
    state is frozen for a block of K transitions of every chain, the sums
    (and, across ranks, the one all-reduce) cover the block's K * C
    chain-steps, and one update ends it, with gamma counting blocks.  Then
    `sample` advances one block and `sample_(n)` needs n % K == 0;
    num_warmup must be a multiple of K.

    The all-reduce (RCCL, the package's own communicator) is enqueued on the
    compute stream between the stats and update launches; with overlap it
    runs on a side stream and the compute stream waits on its event only
    where the sums are consumed.

    overlap = True (the all-reduce overlapped with the next
    proposal) pools with a lag of one block: block b+1 runs with the shared
    state that block b-1's sums produced while block b's sums are still being
    all-reduced, i.e.

        theta_{b+1} = update(theta_b, sums_{b-1}),   theta_1 = theta_0,

    with the noise position advancing every block as usual.  The update rule
    is unchanged (delta measured from the mean of the block the sums come
    from); only which sums it consumes differs, so this is a delayed
    stochastic-approximation step.  The sums of the last block stay pending
    in the sampler and are applied by the next call.  Results do not depend on
    the rank count (up to the association order of the sums across ranks).

    exact_sums = True removes that parenthesis: every chunk partial of the
    stats kernels is mapped to fixed-point int64 limbs (include/amh.h "exact
    sums"), integers are all that is added -- within a rank, over the steps of
    a block and in the all-reduce -- and the totals are rounded to the usual
    float64 sums once, after the exchange.  A run is then byte-identical for
    every rank count whose shards start at multiples of
    pooled_chunk(d, total chains) (init raises ValueError otherwise;
    distributed.shard_range(..., align=) makes such shards), one rank
    included; it differs from the default run as two association orders do.
    The message grows from 8 to 40 bytes per component."""

    pooled = True  # adapt-state leaves carry no chain axis

    def __init__(self, model=None, potential_fn=None, lr_decay=2 / 3, target_accept_prob=0.234, eps=1e-6,
                 num_chains=None, device=None, chain_offset=0, group=None, sync_every: int = 1,
                 overlap: bool = False, exact_sums: bool = False, **kw):
        super().__init__(model=model, potential_fn=potential_fn, lr_decay=lr_decay,
                         target_accept_prob=target_accept_prob, eps=eps, num_chains=num_chains, device=device,
                         chain_offset=chain_offset, **kw)
        if int(sync_every) < 1:
            raise ValueError("sync_every must be >= 1")
        self._group = group
        self._sums = None
        self._bufs = None
        self._pending = None  # overlap: (buffer index, all-reduce event or None) not yet applied
        self._last_out = None  # overlap: weak reference to the z leaf of the state the pending sums belong to
        self._comm = None
        self.sync_every = int(sync_every)
        self.overlap = bool(overlap)
        self.exact_sums = bool(exact_sums)
        self._acc = None   # exact_sums: the int64 words of each sums buffer
        self._total = None  # exact_sums: chains of all ranks (cuts the chunks below d = 64)
        # testing / profiling: run the multi-rank step (stats launch, the
        # all-reduce on the side stream, update launch) even in a world of one
        # rank, so the RCCL branch can be exercised and timed on one GPU
        self.force_collective = False
        # A/B: the non-overlapped all-reduce through torch.distributed on its
        # side stream (the round-4 path) instead of RCCL on the compute stream
        self.torch_stream_collective = False
        self._rccl_comm = None

    def _world(self) -> int:
        if not dist.is_available() or not dist.is_initialized():
            return 1
        return dist.get_world_size(self._group)

    def init(self, rng_key, num_warmup, init_params, model_args, model_kwargs):
        """Per-chain z0 / pe0 / keys as ARWMH.init (arwmh.py:84-138); shared
        state mu = 0, L = Sigma = I, lambda = 0, i = 0 (mu_0 is irrelevant
        after step 1, where gamma_1 = 1)."""
        if int(num_warmup) % self.sync_every != 0:
            raise ValueError(f"num_warmup ({num_warmup}) must be a multiple of sync_every ({self.sync_every})")
        st = super().init(rng_key, num_warmup, init_params, model_args, model_kwargs)
        d, dev = self._dim, st.z.device
        if d > 64 and d % 32 != 0:  # the pooled MFMA tiles (amh_pooled_stats returns AMH_EINVAL)
            raise ValueError(f"the pooled mode takes d <= 64 or a multiple of 32 up to 256, not d = {d}")
        f = dict(dtype=torch.float32, device=dev)
        eye = torch.eye(d, dtype=torch.float64, device=dev)
        from .arwmh import pack_scale
        cov = pack_scale(eye)
        adapt = PooledAdaptState(torch.zeros(d, **f), cov.to(torch.float32), torch.zeros(1, **f))
        self._bufs = torch.zeros(2, sums_size(d), dtype=torch.float64, device=dev)
        self._sums = self._bufs[0]
        if self.exact_sums:
            self._total = self._total_chains(st.z.shape[0], dev)
            chunk = pooled_chunk(d, self._total)
            if self._chain_offset % chunk != 0:
                raise ValueError(f"exact_sums needs chain_offset ({self._chain_offset}) to be a multiple of the "
                                 f"chunk of {chunk} chains (pooled_chunk({d}, {self._total}))")
            self._acc = torch.zeros(2, exact_size(d), dtype=torch.int64, device=dev)
        self._pending = None
        self._last_out = None
        return PooledState(torch.zeros(1, dtype=torch.int32, device=dev), st.z, st.potential_energy,
                           torch.zeros(1, **f), adapt, torch.zeros(1, **f), st.rng_key, cov)

    def _total_chains(self, local: int, dev) -> int:
        """The chain count of all ranks: one all-reduce of the local counts."""
        if self._world() == 1:
            return int(local)
        on_dev = dist.get_backend(self._group) == "nccl"
        t = torch.tensor([int(local)], dtype=torch.int64, device=dev if on_dev else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self._group)
        return int(t.item())

    @staticmethod
    def _c(s: PooledState) -> AmhPooledState:
        a = s.adapt_state
        return AmhPooledState(s.i.data_ptr(), s.z.data_ptr(), s.potential_energy.data_ptr(), s.rng_key.data_ptr(),
                              s.mean_accept_prob.data_ptr(), a.loc.data_ptr(), a.scale.data_ptr(),
                              a.log_step_size.data_ptr(), s.as_change.data_ptr(), s.cov.data_ptr())

    def _check(self, s: PooledState):
        if self._handle is None:
            raise RuntimeError("call init() first")
        d = self._dim
        C = s.z.shape[0]
        want = [(s.i, (1,), torch.int32), (s.z, (C, d), torch.float32), (s.potential_energy, (C,), torch.float32),
                (s.mean_accept_prob, (1,), torch.float32), (s.adapt_state.loc, (d,), torch.float32),
                (s.adapt_state.scale, (packed_size(d),), torch.float32),
                (s.adapt_state.log_step_size, (1,), torch.float32), (s.as_change, (1,), torch.float32),
                (s.rng_key, (C, 2), torch.int32), (s.cov, (packed_size(d),), torch.float64)]
        for t, shape, dt in want:
            _lib.require_gpu(t)
            if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous():
                raise ValueError(f"pooled state leaf has shape {tuple(t.shape)} {t.dtype}, expected {shape} {dt}")
        return C

    def _new_like(self, s: PooledState) -> PooledState:
        a = s.adapt_state
        return PooledState(torch.empty_like(s.i), torch.empty_like(s.z), torch.empty_like(s.potential_energy),
                           torch.empty_like(s.mean_accept_prob),
                           PooledAdaptState(torch.empty_like(a.loc), torch.empty_like(a.scale),
                                            torch.empty_like(a.log_step_size)),
                           torch.empty_like(s.as_change), s.rng_key, torch.empty_like(s.cov))

    # ------------------------------------------------------- the exchange --
    def _exchange(self, b: int, dev: int):
        """The exchange of sums buffer b; returns what _allreduce does.
        exact_sums: the all-reduce carries the buffer's int64 words, and the
        conversion to the float64 sums follows it on the stream where it
        completes, in every world (so one rank and N ranks run the same
        arithmetic)."""
        if not self.exact_sums:
            return self._allreduce(self._bufs[b], dev)

        def convert():
            _lib.check(_lib.lib().amh_pooled_exact_to_sums(self._handle.h, _lib.ptr(self._acc[b]),
                                                           _lib.ptr(self._bufs[b]), _lib.stream_ptr(dev)),
                       self._handle.h)
        return self._allreduce(self._acc[b], dev, then=convert)

    def _allreduce(self, buf: torch.Tensor, dev: int, then=None):
        """all_reduce(sum) of one sums buffer.  RCCL without overlap: on the
        compute stream itself (kernels_amd.distributed.rccl_allreduce_sum:
        the update follows in stream order, no cross-stream event); returns
        None.  RCCL with overlap: enqueued on the side stream after the
        compute stream's work so far; returns the event the consumer waits
        on.  gloo (ranks sharing a device, CPU tests): done in place,
        host-synchronous; returns None.  `then` (exact_sums: the conversion) is
        called where the reduced buffer is next available in stream order:
        on the current stream, or on the side stream before the event."""
        then = then or (lambda: None)
        if self._world() == 1 and not (self.force_collective and dist.is_available() and dist.is_initialized()):
            then()
            return None
        if dist.get_backend(self._group) != "nccl":
            dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self._group)
            then()
            return None
        if not self.overlap and not self.torch_stream_collective:
            # this package's own communicator (distributed.RcclComm), the
            # collective on the compute stream.  Setup (the id broadcast and
            # ncclCommInitRank) runs on every rank in the same host order;
            # any RCCL error raises -- no fallback once a collective may have
            # been issued.  Only a process without RCCL mapped (OSError, the
            # same on every rank) takes torch's stream instead.
            from .distributed import RcclComm
            if self._rccl_comm is None:
                try:
                    self._rccl_comm = RcclComm(self._group, buf.device)
                except OSError as e:
                    import warnings
                    warnings.warn(f"RCCL not mapped ({e}); using torch.distributed's stream", RuntimeWarning)
                    self.torch_stream_collective = True
            if self._rccl_comm is not None:
                self._rccl_comm.all_reduce_sum(buf, torch.cuda.current_stream(dev), handle=self._handle)
                then()
                return None
        if self._comm is None:
            self._comm = torch.cuda.Stream(device=dev)
        self._comm.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(self._comm):
            dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self._group)
            then()
            ev = torch.cuda.Event()
            ev.record(self._comm)
        return ev

    def close_comm(self):
        """Destroy this sampler's own RCCL communicator (collective over the
        group's ranks in the same host order; a later multi-rank step creates
        a new one)."""
        if self._rccl_comm is not None:
            c, self._rccl_comm = self._rccl_comm, None
            c.close()

    def _stats_external(self, L, cin, sout, b, C):
        """AMH_MODEL_EXTERNAL: the block's K transitions as K rounds of
        amh_pooled_propose, the caller's U of the proposals, and
        amh_pooled_stats_external (accept + the round's sums, added to the
        block's in step order).  Rounds after the first read the z / pe the
        previous one wrote, with the frozen shared state of `cin`."""
        dev = sout.z.device
        h, st = self._handle.h, _lib.stream_ptr(dev.index)
        zp = torch.empty(C, self._dim, dtype=torch.float32, device=dev)
        cur = cin
        for t in range(self.sync_every):
            _lib.check(L.amh_pooled_propose(h, C, ctypes.byref(cur), t, _lib.ptr(zp), st), h)
            pe = self._potential_fn.evaluate(zp)
            out = (_lib.ptr(zp), _lib.ptr(pe), _lib.ptr(sout.z), _lib.ptr(sout.potential_energy))
            if self.exact_sums:  # (integer words: the order of the rounds no longer matters)
                rc = L.amh_pooled_stats_external_exact(h, C, self._total, ctypes.byref(cur), t, *out,
                                                       _lib.ptr(self._acc[b]), int(t > 0), st)
            else:
                rc = L.amh_pooled_stats_external(h, C, ctypes.byref(cur), t, *out, _lib.ptr(self._bufs[b]),
                                                 int(t > 0), st)
            _lib.check(rc, h)
            if t == 0 and self.sync_every > 1:
                cur = AmhPooledState.from_buffer_copy(cin)
                cur.z, cur.potential_energy = sout.z.data_ptr(), sout.potential_energy.data_ptr()

    def _step_order_block(self) -> bool:
        """Logistic and Poisson regression at sync_every > 1: the block runs as K
        single-step stats launches whose completely reduced sums are added in
        step order -- the callable path's association (include/amh.h,
        amh_pooled_stats_external), so PooledARWMH(model=entry) equals
        PooledARWMH(potential_fn=its potential) bit for bit at every
        sync_every.  The other registry models keep the one-launch block, whose
        sums are associated inside the chunk."""
        return self.sync_every > 1 and self._model is not None and \
            self._model.model_id in (_lib.AMH_MODEL_LOGISTIC, _lib.AMH_MODEL_POISSON)

    def _stats_step_order(self, L, cin, sout, b, C):
        dev = sout.z.device
        h, st = self._handle.h, _lib.stream_ptr(dev.index)
        cur = AmhPooledState.from_buffer_copy(cin)
        total = self._acc[b] if self.exact_sums else self._bufs[b]
        part = torch.empty_like(total)
        for t in range(self.sync_every):
            it = self._block_i + t  # the step's noise position; the shared state stays frozen
            cur.i = it.data_ptr()
            into = total if t == 0 else part
            out = (_lib.ptr(sout.z), _lib.ptr(sout.potential_energy), _lib.ptr(into), st)
            if self.exact_sums:
                rc = L.amh_pooled_stats_k_exact(h, C, self._total, ctypes.byref(cur), 1, *out)
            else:
                rc = L.amh_pooled_stats_k(h, C, ctypes.byref(cur), 1, *out)
            _lib.check(rc, h)
            if t > 0:
                total += part
            cur.z, cur.potential_energy = sout.z.data_ptr(), sout.potential_energy.data_ptr()

    def _stats(self, L, cin, sout, b, C):
        """The block's transitions and this rank's sums into buffer b (its
        float64 sums, or with exact_sums its int64 words)."""
        dev = sout.z.device.index
        if self._external():
            return self._stats_external(L, cin, sout, b, C)
        if self._step_order_block():
            return self._stats_step_order(L, cin, sout, b, C)
        if self.exact_sums:
            _lib.check(L.amh_pooled_stats_k_exact(self._handle.h, C, self._total, ctypes.byref(cin), self.sync_every,
                                                  _lib.ptr(sout.z), _lib.ptr(sout.potential_energy),
                                                  _lib.ptr(self._acc[b]), _lib.stream_ptr(dev)), self._handle.h)
            return
        _lib.check(L.amh_pooled_stats_k(self._handle.h, C, ctypes.byref(cin), self.sync_every, _lib.ptr(sout.z),
                                        _lib.ptr(sout.potential_energy), _lib.ptr(self._bufs[b]),
                                        _lib.stream_ptr(dev)), self._handle.h)

    def _update(self, L, buf, cin, cout):
        dev = buf.device.index
        _lib.check(L.amh_pooled_update_k(self._handle.h, _lib.ptr(buf), ctypes.byref(cin), ctypes.byref(cout),
                                         self.sync_every, _lib.stream_ptr(dev)), self._handle.h)

    def _one(self, sin: PooledState, sout: PooledState):
        L = _lib.lib()
        dev = sin.z.device.index
        C = sin.z.shape[0]
        cin, cout = self._c(sin), self._c(sout)
        self._block_i = sin.i  # the block's first noise position (_stats_step_order)
        with torch.cuda.device(dev):
            if not self.overlap:
                buf = self._bufs[0]
                self._stats(L, cin, sout, 0, C)
                ev = self._exchange(0, dev)
                if ev is not None:
                    torch.cuda.current_stream(dev).wait_event(ev)
                self._update(L, buf, cin, cout)
                self._sums = buf
                return
            last = self._last_out() if self._last_out is not None else None
            if self._pending is not None and last is not sin.z:
                # a state this sampler did not just produce: the pending sums
                # belong to another trajectory, so this block starts afresh
                # (theta_1 = theta_0).  A checkpoint carries them instead
                # (checkpoint.state_dict(state, kernel)).
                self._pending = None
            b = 0 if self._pending is None else 1 - self._pending[0]
            buf = self._bufs[b]
            self._stats(L, cin, sout, b, C)
            ev = self._exchange(b, dev)  # in flight while the next block computes
            if self._pending is not None:
                pb, pev = self._pending
                if pev is not None:
                    torch.cuda.current_stream(dev).wait_event(pev)
                self._update(L, self._bufs[pb], cin, cout)
            else:  # first block: theta_1 = theta_0, the noise position advances
                if sout is not sin:
                    for a, c in ((sin.adapt_state.loc, sout.adapt_state.loc),
                                 (sin.adapt_state.scale, sout.adapt_state.scale),
                                 (sin.adapt_state.log_step_size, sout.adapt_state.log_step_size),
                                 (sin.mean_accept_prob, sout.mean_accept_prob), (sin.as_change, sout.as_change),
                                 (sin.cov, sout.cov)):
                        c.copy_(a)
                torch.add(sin.i, self.sync_every, out=sout.i)
            self._pending = (b, ev)
            self._last_out = weakref.ref(sout.z)
            self._sums = buf

    # ------------------------------------------------ checkpoint (overlap) --
    def pending_sums(self):
        """overlap = True: the all-reduced sums of the last block, not yet
        applied (they update the shared state at the start of the next block),
        as a host float64 array; None when nothing is pending."""
        if self._pending is None:
            return None
        b, ev = self._pending
        if ev is not None:
            ev.synchronize()
        torch.cuda.synchronize(self._bufs.device)
        return self._bufs[b].detach().cpu().numpy().copy()

    def set_pending_sums(self, state, sums):
        """Make `sums` the pending sums of `state` (resume of an overlap run:
        the next block applies them exactly as the uninterrupted run would)."""
        if not self.overlap:
            raise ValueError("pending sums exist only with overlap=True")
        if self._bufs is None:
            raise RuntimeError("call init() first")
        self._bufs[0].copy_(torch.as_tensor(sums, dtype=torch.float64))
        self._pending = (0, None)
        self._last_out = weakref.ref(state.z)

    def check_device(self, synchronize: bool = True):
        """Raise if a launch of this sampler flagged a device-side failure (the
        d = 64 update's bounded wait ran out, so that update kept the shared
        factor: amh_check_device).  synchronize=False reads the flag without
        waiting, which covers every launch that has already finished; sample,
        sample_ and run call it that way after each call (and run, which
        synchronises anyway, with True); the handle's destruction reports what
        is left as a RuntimeWarning."""
        if self._handle is None:
            return
        if synchronize:
            torch.cuda.synchronize(self._handle.device)
        _lib.check(_lib.lib().amh_check_device(self._handle.h), self._handle.h)

    def sample(self, state, model_args=(), model_kwargs=None):
        """One pooled transition of every chain (sync_every > 1: one block of
        them); returns a new state."""
        self._check(state)
        out = self._new_like(state)
        self._one(state, out)
        self.check_device(synchronize=False)
        return out

    def sample_(self, state, n_steps: int = 1):
        """n_steps pooled transitions in place (a multiple of sync_every)."""
        C = self._check(state)
        K = self.sync_every
        if int(n_steps) % K != 0:
            raise ValueError(f"n_steps ({n_steps}) must be a multiple of sync_every ({K})")
        if (self._world() == 1 and not self.overlap and not self.force_collective and not self._external()
                and not self.exact_sums and not self._step_order_block()):
            L = _lib.lib()
            dev = state.z.device.index
            c = self._c(state)
            with torch.cuda.device(dev):
                _lib.check(L.amh_pooled_step_k(self._handle.h, C, ctypes.byref(c), ctypes.byref(c), int(n_steps), K,
                                               _lib.ptr(self._bufs[0]), _lib.stream_ptr(dev)), self._handle.h)
            self._sums = self._bufs[0]
            self.check_device(synchronize=False)
            return state
        for _ in range(int(n_steps) // K):
            self._one(state, state)
        self.check_device(synchronize=False)
        return state

    def run(self, state, n_steps: int, thinning: int = 1, collect_z: bool = True, collect_pe: bool = False):
        """n_steps pooled transitions (numpyro fori_collect over sample):
        returns (new_state, z [n_steps // thinning, C, d] or None, pe or None).
        Draws are taken at block ends, so thinning must be a multiple of
        sync_every (and n_steps of both)."""
        C = self._check(state)
        K = self.sync_every
        if int(thinning) < 1 or int(thinning) % K != 0 or int(n_steps) % K != 0:
            raise ValueError(f"thinning ({thinning}) and n_steps ({n_steps}) must be multiples of sync_every ({K})")
        out = self._new_like(state)  # (shares the constant rng_key leaf)
        for t, src in ((out.i, state.i), (out.z, state.z), (out.potential_energy, state.potential_energy),
                       (out.mean_accept_prob, state.mean_accept_prob), (out.as_change, state.as_change),
                       (out.cov, state.cov)) + tuple(zip(out.adapt_state, state.adapt_state)):
            t.copy_(src)
        if self._last_out is not None and self._last_out() is state.z:
            self._last_out = weakref.ref(out.z)  # the pending sums continue with the copy
        keep = int(n_steps) // int(thinning)
        dev = state.z.device
        cz = torch.empty(keep, C, self._dim, dtype=torch.float32, device=dev) if collect_z and keep else None
        cp = torch.empty(keep, C, dtype=torch.float32, device=dev) if collect_pe and keep else None
        done = 0
        for k in range(keep):
            self.sample_(out, int(thinning))
            done += int(thinning)
            if cz is not None:
                cz[k].copy_(out.z)
            if cp is not None:
                cp[k].copy_(out.potential_energy)
        if int(n_steps) > done:
            self.sample_(out, int(n_steps) - done)
        self.check_device(synchronize=True)
        return out, cz, cp

    def get_diagnostics_str(self, state):
        acc = float(state.mean_accept_prob[0])
        step = float(torch.exp(state.adapt_state.log_step_size[0]))
        return f"Acceptance rate: {acc:.2f}, Step size: {step:.3f}"
