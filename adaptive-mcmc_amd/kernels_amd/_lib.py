"""ctypes binding of libamh.so (include/amh.h).

The product path has exactly one implementation of the transition: the HIP
kernels in libamh.so.  If the library is missing, or no GPU is visible, every
compute entry point raises -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import torch  # noqa: F401  (loads the HIP runtime libamh.so binds against)

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("AMH_LIB_PATH") or os.path.join(_PKG, "lib", "libamh.so")
CSRC = os.path.join(_PKG, "csrc")

AMH_MODEL_GAUSSIAN = 1
AMH_MODEL_EIGHT_SCHOOLS = 2
AMH_MODEL_KIDIQ = 3
AMH_MODEL_DIAMONDS = 4
AMH_MODEL_DIAMONDS_SS = 5
AMH_MODEL_MIXTURE = 6
AMH_MODEL_EXTERNAL = 7  # the caller's potential (amh_propose / amh_step_external)
AMH_MODEL_LOGISTIC = 8  # logistic regression on the caller's data (posteriors.logistic_regression)
AMH_MODEL_POISSON = 9  # Poisson regression on the caller's data (posteriors.poisson_regression)
AMH_STEP_PROPOSAL_READY = 1
AMH_STEP_KEEP_PROPOSAL = 2
AMH_ASSS_EXT_ROUNDS = 51  # shrink rounds 0 .. 50 of the external slice sampler (amh_asss_ext_shrink)


class AmhConfig(ctypes.Structure):
    _fields_ = [("dim", ctypes.c_int32), ("num_warmup", ctypes.c_int32), ("lr_decay", ctypes.c_float),
                ("target_accept_prob", ctypes.c_float), ("eps", ctypes.c_float),
                ("reserved", ctypes.c_int32 * 3)]


class AmhState(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("i", "z", "potential_energy", "mean_accept_prob", "loc", "scale",
                                               "log_step_size", "as_change", "rng_key")]


class AmhCollect(ctypes.Structure):
    _fields_ = [("z", ctypes.c_void_p), ("potential_energy", ctypes.c_void_p), ("accept_count", ctypes.c_void_p),
                ("thinning", ctypes.c_int32)]


class AmhPooledState(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("i", "z", "potential_energy", "rng_key", "mean_accept_prob", "loc",
                                               "scale", "log_step_size", "as_change", "cov")]


def _signatures():
    P, I, I32, I64, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    KEY = ctypes.POINTER(ctypes.c_uint32)
    S, COL, PS = ctypes.POINTER(AmhState), ctypes.POINTER(AmhCollect), ctypes.POINTER(AmhPooledState)
    return {
        # core
        "amh_version": (I, []),
        "amh_last_error": (ctypes.c_char_p, [P]),
        "amh_create": (I, [ctypes.POINTER(AmhConfig), I, ctypes.POINTER(P)]),
        "amh_destroy": (I, [P]),
        "amh_check_device": (I, [P]),
        "amh_step_order": (I, [P, ctypes.POINTER(I32)]),
        "amh_step64_schedule": (I, [I32, I32, ctypes.POINTER(I32), ctypes.POINTER(I32)]),
        "amh_step64_steal_schedule": (I, [I32, I32, I32, I32, I32] + [ctypes.POINTER(I32)] * 5),
        "amh_step64_set_steal": (I, [P, I32]),
        "amh_step64_stolen": (I, [P, ctypes.POINTER(I64), P]),
        "amh_bind_model": (I, [P, I32, P, I64, ctypes.POINTER(I64), I32]),
        "amh_init": (I, [P, KEY, I64, I64, P, S, P]),
        "amh_step": (I, [P, I64, S, S, I32, COL, P]),
        "amh_step_chained": (I, [P, I64, S, S, I32, COL, I32, P]),
        "amh_potential": (I, [P, P, P, I64, P]),
        "amh_sample_pnx": (I, [P, KEY, P, I64, I64, P, P, F, I32, P, P]),
        "amh_chain_keys": (I, [KEY, I64, I64, P, P]),
        # external potential
        "amh_propose": (I, [P, I64, S, P, P]),
        "amh_step_external": (I, [P, I64, S, S, P, P, P, COL, P]),
        "amh_pnx_propose": (I, [P, KEY, P, I64, P, F, I32, P, P]),
        "amh_pnx_accept": (I, [P, KEY, P, P, I64, P, P, I32, P]),
        # ASSS
        "amh_asss_step": (I, [P, I64, S, S, I32, COL, P]),
        "amh_asss_sample_pnx": (I, [P, KEY, P, I64, I64, P, P, I32, P, P]),
        # ASSS, external potential (host-driven shrink loop)
        "amh_asss_ext_work_size": (I, [I32, ctypes.POINTER(I64)]),
        "amh_asss_ext_begin": (I, [P, I64, S, P, P, P, P]),
        "amh_asss_ext_shrink": (I, [P, I64, P, I32, P, P, P, P]),
        "amh_asss_ext_finish": (I, [P, I64, S, S, P, P, COL, P]),
        "amh_asss_ext_pnx_begin": (I, [P, KEY, P, I64, P, P, I32, P, P, P, P]),
        "amh_asss_ext_pnx_finish": (I, [P, I64, P, P, P, P]),
        # evaluation
        "amh_kernel_sum_scratch": (I64, [I64, I64]),
        "amh_kernel_sum": (I, [P, I64, P, I64, I32, F, I32, P, P, P]),
        "amh_pairwise_dist2": (I, [P, I64, P, I64, I32, P, P]),
        "amh_normals": (I, [KEY, I64, P, P]),
        "amh_sinkhorn_lse": (I, [P, I64, I64, P, F, F, P, P]),
        # linear assignment (auction)
        "amh_assign_work_size": (I, [I64, ctypes.POINTER(I64)]),
        "amh_assign_begin": (I, [P, I64, P, P]),
        "amh_assign_quantum": (I, [P, I64, ctypes.POINTER(I32), ctypes.POINTER(I64), P]),
        "amh_assign_phase": (I, [P, I64, P]),
        "amh_assign_rounds": (I, [P, I64, P, I64, I64, I64, I32, P]),
        "amh_assign_status": (I, [P, I64, I64, ctypes.POINTER(I64), ctypes.POINTER(I64), P]),
        "amh_assign_result": (I, [P, I64, P, P, P]),
        # streaming summaries
        "amh_summary_update": (I, [P, I64, I64, I32, P, I32, I64, I64, P, P, P]),
        # pooled covariance
        "amh_pooled_sums_size": (I, [I32, ctypes.POINTER(I64)]),
        "amh_pooled_stats": (I, [P, I64, PS, P, P, P, P]),
        "amh_pooled_update": (I, [P, P, PS, PS, P]),
        "amh_pooled_step": (I, [P, I64, PS, PS, I32, P, P]),
        "amh_pooled_stats_k": (I, [P, I64, PS, I32, P, P, P, P]),
        "amh_pooled_update_k": (I, [P, P, PS, PS, I32, P]),
        "amh_pooled_step_k": (I, [P, I64, PS, PS, I32, I32, P, P]),
        "amh_pooled_allreduce": (I, [P, P, I64, P, P]),
        "amh_pooled_propose": (I, [P, I64, PS, I32, P, P]),
        "amh_pooled_stats_external": (I, [P, I64, PS, I32, P, P, P, P, P, I32, P]),
        # pooled ASSS
        "amh_pooled_asss_stats_k": (I, [P, I64, PS, I32, P, P, P, P]),
        "amh_pooled_asss_update_k": (I, [P, P, PS, PS, I32, P]),
        "amh_pooled_asss_step_k": (I, [P, I64, PS, PS, I32, I32, P, P]),
        # pooled ASSS, external potential (the shrink rounds are amh_asss_ext_shrink)
        "amh_pooled_asss_ext_begin": (I, [P, I64, PS, I32, P, P, P, P]),
        "amh_pooled_asss_ext_finish": (I, [P, I64, PS, P, P, P, P, P, I32, P]),
        "amh_pooled_asss_ext_update": (I, [P, P, PS, PS, I32, P]),
        # pooled covariance, exact sums
        "amh_pooled_exact_size": (I, [I32, ctypes.POINTER(I64)]),
        "amh_pooled_chunk_chains": (I, [I32, I64, ctypes.POINTER(I64)]),
        "amh_pooled_stats_k_exact": (I, [P, I64, I64, PS, I32, P, P, P, P]),
        "amh_pooled_stats_external_exact": (I, [P, I64, I64, PS, I32, P, P, P, P, P, I32, P]),
        "amh_pooled_exact_to_sums": (I, [P, P, P, P]),
        "amh_pooled_allreduce_i64": (I, [P, P, I64, P, P]),
        "amh_pooled_exact_quantise": (I, [P, I64, I64, P, I32]),
        "amh_pooled_exact_to_double": (I, [P, I64, P]),
    }


# every symbol include/amh.h declares: name -> (restype, argtypes)
SIGNATURES = _signatures()
EXPORTS = tuple(SIGNATURES)


class AmhError(RuntimeError):
    pass


_lib = None


def build(arch: str = "gfx950") -> str:
    """Compile libamh.so in-tree (hipcc, gfx950)."""
    subprocess.run(["make", "-s", "-C", CSRC, f"ARCH={arch}"], check=True)
    return LIB_PATH


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AmhError(f"libamh.so not built ({LIB_PATH}); run `make -C {CSRC}` or __graft_entry__.build()")
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = L
    return L


def check(rc: int, handle=None):
    if rc != 0:
        msg = lib().amh_last_error(handle)
        raise AmhError(f"libamh error {rc}: {msg.decode() if msg else ''}")


def require_gpu(t: torch.Tensor):
    if not t.is_cuda:
        raise AmhError("libamh operates on device tensors; no CPU fallback exists (is a GPU visible?)")


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream_ptr(device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def key_arr(key) -> "ctypes.Array":
    k = [int(v) & 0xFFFFFFFF for v in key]
    return (ctypes.c_uint32 * 2)(*k)


class Handle:
    """Owns one amh_handle (one device, one model binding)."""

    def __init__(self, dim: int, num_warmup: int, lr_decay: float, target_accept_prob: float, eps: float,
                 device: int):
        self._lib = lib()
        cfg = AmhConfig(dim, num_warmup, lr_decay, target_accept_prob, eps, (ctypes.c_int32 * 3)(0, 0, 0))
        h = ctypes.c_void_p()
        with torch.cuda.device(device):
            check(self._lib.amh_create(ctypes.byref(cfg), device, ctypes.byref(h)))
        self.h = h
        self.device = device
        self.dim = dim
        self._data = None

    def bind_model(self, model_id: int, data: torch.Tensor, iparams=()):
        require_gpu(data)
        ip = (ctypes.c_int64 * max(1, len(iparams)))(*iparams)
        with torch.cuda.device(self.device):
            # the library may copy `data` on the null stream: let the stream
            # that produced it finish first
            torch.cuda.current_stream(data.device).synchronize()
            check(self._lib.amh_bind_model(self.h, model_id, ptr(data), data.numel(), ip, len(iparams)), self.h)
        self._data = data  # keep alive

    def step_order(self) -> int:
        """Chain order of the last d = 64 step launch: 0 ascending, 1 descending, -1 none yet."""
        order = ctypes.c_int32(-2)
        check(self._lib.amh_step_order(self.h, ctypes.byref(order)), self.h)
        return order.value

    def set_steal(self, steal: int):
        """Stealable-tail length of the single-step d = 64 launches (0: none); changes no result."""
        check(self._lib.amh_step64_set_steal(self.h, int(steal)), self.h)

    def stolen(self) -> int:
        """Chains of the last single-step d = 64 launch that a block took from another block's tail."""
        n = ctypes.c_int64(-1)
        with torch.cuda.device(self.device):
            check(self._lib.amh_step64_stolen(self.h, ctypes.byref(n), stream_ptr(self.device)), self.h)
        return n.value

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            rc = self._lib.amh_destroy(self.h)
            self.h = None
            if rc != 0:  # a device-side failure nobody had collected (amh_check_device)
                import warnings
                msg = self._lib.amh_last_error(None)
                warnings.warn(f"libamh: {msg.decode() if msg else rc}", RuntimeWarning)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
