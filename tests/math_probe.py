"""ctypes loader for the test-only probe library libamh_probe.so
(adaptive-mcmc_amd/csrc/amh_probe.hip): elementwise device maps of the
functions of include/amh_math.h and of the row terms of amh_device.h, and the
amh_probe_host_* twins (hipcc's host compile of the same header, no device).

Test infrastructure: the product package never imports this."""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# AMH_PROBE_LIB selects another build of the same source (sensitivity checks)
LIB_PATH = os.environ.get("AMH_PROBE_LIB") or os.path.join(ROOT, "adaptive-mcmc_amd", "lib", "libamh_probe.so")
MAKE = "make -C adaptive-mcmc_amd/csrc ARCH=gfx950"

F2F = {"logf": 0, "expf": 1, "log1pf": 2, "log1p_sqf": 3, "log1p_sq3f": 4, "sin": 5, "cos": 6, "rsqrt_nr": 7,
       "erfinvf": 8}
U2F = {"unif01": 0, "normal_from_bits": 1, "normal_split": 2}
F2I = {"pivot_ok": 0, "isfinite": 1, "isnan": 2}
FF2F = {"logistic_term": 0, "poisson_term": 1, "lp_student3_intercept": 2, "lp_student3_sigma": 3}
D2D = {"log_d": 0, "exp_d": 1}

_P, _I, _I64, _F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
_lib = None


def lib():
    """The library, or an AssertionError that names the build command: a test
    that needs the probe fails without it, it does not skip."""
    global _lib
    if _lib is None:
        assert os.path.exists(LIB_PATH), f"{LIB_PATH} is missing: build it with `{MAKE}`"
        L = ctypes.CDLL(LIB_PATH)
        for name in ("amh_probe_f2f", "amh_probe_u2f", "amh_probe_f2i", "amh_probe_d2d"):
            getattr(L, name).argtypes = [_I, _P, _P, _I64, _P]
        L.amh_probe_ff2f.argtypes = [_I, _P, _P, _P, _I64, _P]
        L.amh_probe_lr_gamma.argtypes = [_P, _F, _P, _I64, _P]
        L.amh_probe_host_lr_gamma.argtypes = [_P, _F, _P, _I64]
        L.amh_probe_host_lr_gamma.restype = None
        for name in ("log_d", "exp_d", "expf", "logf"):
            fn = getattr(L, "amh_probe_host_" + name)
            fn.argtypes = [_P, _P, _I64]
            fn.restype = None
        _lib = L
    return _lib


# ------------------------------------------------------------- host twins --
def host(name, x, a=None):
    """amh_probe_host_<name> over a numpy array (lr_gamma: int32 n and the rate a)."""
    L = lib()
    if name == "lr_gamma":
        x = np.ascontiguousarray(x, np.int32)
        y = np.empty(x.shape, np.float32)
        L.amh_probe_host_lr_gamma(x.ctypes.data, a, y.ctypes.data, x.size)
        return y
    x = np.ascontiguousarray(x, np.float64 if name.endswith("_d") else np.float32)
    y = np.empty_like(x)
    getattr(L, "amh_probe_host_" + name)(x.ctypes.data, y.ctypes.data, x.size)
    return y


# ---------------------------------------------------------- device probes --
def _run(dev, out_dtype, call, *arrays):
    """Copies the numpy inputs to the device, launches on torch's current
    stream, returns the output as numpy."""
    import torch
    with torch.cuda.device(dev.index):
        ins = [torch.tensor(np.ascontiguousarray(a), device=dev) for a in arrays]  # a copy: the sets are read-only
        out = torch.empty(ins[0].shape, dtype=out_dtype, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev.index).cuda_stream)
        rc = call(*[ctypes.c_void_p(t.data_ptr()) for t in ins], ctypes.c_void_p(out.data_ptr()), ins[0].numel(),
                  stream)
        assert rc == 0, f"probe launch failed with status {rc}"
        torch.cuda.synchronize(dev)
        return out.cpu().numpy()


def _signed(a):
    # torch has no uint32 arithmetic; the bits travel as int32
    return np.ascontiguousarray(a, np.uint32).view(np.int32)


def device(dev, name, x, y=None, a=None):
    """One probe over numpy input(s) on torch device `dev`."""
    import torch
    L = lib()
    if name in F2F:
        return _run(dev, torch.float32, lambda *p: L.amh_probe_f2f(F2F[name], *p), np.asarray(x, np.float32))
    if name in U2F:
        return _run(dev, torch.float32, lambda *p: L.amh_probe_u2f(U2F[name], *p), _signed(x))
    if name in F2I:
        return _run(dev, torch.int32, lambda *p: L.amh_probe_f2i(F2I[name], *p), np.asarray(x, np.float32))
    if name in ("logistic_term", "poisson_term"):
        return _run(dev, torch.float32, lambda *p: L.amh_probe_ff2f(FF2F[name], *p), np.asarray(x, np.float32),
                    np.asarray(y, np.float32))
    if name in FF2F:
        return _run(dev, torch.float32, lambda px, po, n, s: L.amh_probe_ff2f(FF2F[name], px, None, po, n, s),
                    np.asarray(x, np.float32))
    if name in D2D:
        return _run(dev, torch.float64, lambda *p: L.amh_probe_d2d(D2D[name], *p), np.asarray(x, np.float64))
    if name == "lr_gamma":
        return _run(dev, torch.float32, lambda pn, po, n, s: L.amh_probe_lr_gamma(pn, a, po, n, s),
                    np.asarray(x, np.int32))
    raise KeyError(name)
