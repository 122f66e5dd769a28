"""Sample-quality metrics of the reference (python/utils/evaluation.py) on the
GPU, same function names and arguments.

  pth_moment_rmse          evaluation.py:13-40    column means of x^p (device)
  wasserstein_dist11_p     evaluation.py:43-67    optimal 1-1 coupling; the
                                                   reference runs scipy's
                                                   Hungarian on the host, and
                                                   so does method="hungarian"
                                                   (the default);
                                                   method="auction" builds the
                                                   cost matrix and solves the
                                                   assignment on the device
  linear_assignment        (no reference analogue) square assignment problem by
                                                   an integer auction with
                                                   epsilon-scaling in HIP
                                                   (amh_assign_*): within 2
                                                   quanta (each <= 2^-29 x the
                                                   largest cost) of the optimum
  wasserstein_1d           evaluation.py:139-162  sorted differences (device)
  max_sliced_wasserstein   evaluation.py:165-206  projections = one GEMM
                                                   (hipBLASLt through torch),
                                                   per-direction sorts
  gaussian_kernel          evaluation.py:209-230  exp(-gamma D2), D2 from the
                                                   HIP pairwise-distance kernel
  mmd2_unbiased            evaluation.py:233-266  three HIP Gaussian-kernel
                                                   sums (amh_kernel_sum,
                                                   diagonal skipped in-kernel)
  mmd_heuristic            evaluation.py:269-294  median bandwidth from the
                                                   HIP distance matrix

  wasserstein_sinkhorn     evaluation.py:69-101   log-domain Sinkhorn (the
                                                   solver ott-jax's linear.solve
                                                   runs), half-iterations on
                                                   the HIP row log-sum-exp
                                                   kernel (amh_sinkhorn_lse)
  wasserstein_sinkhorn_unbiased  evaluation.py:104-130

ott-jax is not importable here (and unpinned in the reference's
environment.yml), so the Sinkhorn pair follows ott's published algorithm and
defaults -- Euclidean cost, epsilon = 0.05 x std of the cost matrix when not
given, marginal-error threshold 1e-3 checked every 10 iterations, at most
2,000 iterations, cost = <a, f> + <b, g> + eps (1 - mass) -- and is pinned only
against a float64 restatement (oracle/sinkhorn_np.py): parity unpinned
against ott itself.

Pins against the reference's own printed outputs (wasserstein-computation
.ipynb on the stored python/mcmc_runs/diamonds-example-*.pkl, extracted
byte-wise into tests/golden/diamonds_example_*.npz):
  * pth_moment_rmse: cell 12's 3.4000627994537354 is reproduced to rel 2e-6
    on the device (tests/test_gpu_eval.py) from the stored references and
    cell 10's printed samples moments.  The notebook's value is the
    mean-square form; evaluation.py:37 now takes the vector norm (sqrt(d)
    times larger), and this module follows the code, not the older notebook.
  * cells 19, 21-24, 31 and 38 (Hungarian W1, Sinkhorn, MMD^2) were computed
    on a samples file the reference no longer holds: the stored one differs
    from cell 10's samples column in 26/26 second moments (b[2]: 122.7 vs
    29.6) and gives Hungarian W1 = 2.933 at n = 30, d = 5 against the table's
    0.596.  Those metrics stay pinned to float64 restatements, now also on the
    full-size stored draws (MMD^2 over 3 x 10^8 pairs).

Inputs may be numpy arrays or torch tensors; they are moved to the current
CUDA device as float32.  Directions for max_sliced_wasserstein come from the
build's Philox stream (the reference uses jax.random.normal), so values agree
with the reference in distribution, not bit for bit.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from kernels_amd import _lib
from kernels_amd.random import as_key

__all__ = ["pth_moment_rmse", "wasserstein_dist11_p", "linear_assignment", "wasserstein_1d", "max_sliced_wasserstein",
           "gaussian_kernel", "mmd2_unbiased", "mmd_heuristic", "wasserstein_sinkhorn", "wasserstein_sinkhorn_unbiased"]


def _dev(x) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        t = x.detach()
    else:
        t = torch.as_tensor(np.asarray(x))
    dev = t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())
    return t.to(device=dev, dtype=torch.float32).contiguous()


def _stream(t: torch.Tensor):
    return _lib.stream_ptr(t.device.index)


def _kernel_sum(a: torch.Tensor, b: torch.Tensor, gamma: float, skip_diag: bool) -> float:
    L = _lib.lib()
    n, d = a.shape
    m = b.shape[0]
    scratch = torch.empty(max(1, int(L.amh_kernel_sum_scratch(n, m))), dtype=torch.float64, device=a.device)
    out = torch.empty(1, dtype=torch.float64, device=a.device)
    with torch.cuda.device(a.device.index):
        _lib.check(L.amh_kernel_sum(_lib.ptr(a), n, _lib.ptr(b), m, d, float(gamma), int(bool(skip_diag)),
                                    _lib.ptr(scratch), _lib.ptr(out), _stream(a)))
    return float(out.item())


def _dist2(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    L = _lib.lib()
    n, d = a.shape
    m = b.shape[0]
    out = torch.empty(n, m, dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device.index):
        _lib.check(L.amh_pairwise_dist2(_lib.ptr(a), n, _lib.ptr(b), m, d, _lib.ptr(out), _stream(a)))
    return out


def pth_moment_rmse(x, y, p=2.0) -> float:
    """||mean(x^p) - mean(y^p)||_2 over columns (evaluation.py:13-40)."""
    x, y = _dev(x), _dev(y)
    return float(torch.linalg.vector_norm(torch.mean(x ** p, dim=0) - torch.mean(y ** p, dim=0)))


ASSIGN_THETA = 4       # epsilon-scaling factor of linear_assignment (DESIGN.md §8 holds the sweep)
ASSIGN_BATCH = 64      # rounds queued between two reads of the unassigned count
ASSIGN_MAX_N = 65536
ASSIGN_MAX_ROUNDS = None  # the default cap on rounds; None: 64 n + 4096


def linear_assignment(cost, *, theta=None, max_rounds=None) -> dict:
    """Minimum-cost perfect matching of a square device cost matrix [n][n]
    (float32, finite, >= 0; 1 <= n <= 65536) by the integer auction of
    csrc/amh_assign.hip: costs quantised to quantum = 2^e <= cmax 2^-29,
    epsilon-scaling by `theta` (default ASSIGN_THETA) down to epsilon = 1.
    The matching's mean cost exceeds the optimum's by at most 2 quantum.

    Returns dict(perm: device int64 person -> object, cost: mean of the
    caller's costs along perm (float64 sum), rounds, phases, quantum, e,
    price: device int64 final prices, converged).  `max_rounds` (default
    64 n + 4096) caps the rounds; when it runs out, converged is False and
    perm holds -1 for the persons left unassigned."""
    if not isinstance(cost, torch.Tensor):
        raise TypeError("linear_assignment takes a torch tensor on the device")
    if cost.dim() != 2 or cost.shape[0] != cost.shape[1] or cost.shape[0] < 1:
        raise ValueError(f"linear_assignment needs a square cost matrix, got {tuple(cost.shape)}")
    n = int(cost.shape[0])
    if n > ASSIGN_MAX_N:
        raise ValueError(f"linear_assignment: n = {n} exceeds {ASSIGN_MAX_N}")
    theta = ASSIGN_THETA if theta is None else int(theta)
    if theta < 2:
        raise ValueError("theta must be an integer >= 2")
    if max_rounds is None:
        max_rounds = 64 * n + 4096 if ASSIGN_MAX_ROUNDS is None else ASSIGN_MAX_ROUNDS
    max_rounds = int(max_rounds)
    if max_rounds < 0:
        raise ValueError("max_rounds must be >= 0")
    _lib.require_gpu(cost)
    cost = cost.detach().to(torch.float32).contiguous()
    L = _lib.lib()
    dev = cost.device
    nbytes = ctypes.c_int64()
    _lib.check(L.amh_assign_work_size(n, ctypes.byref(nbytes)))
    work = torch.empty(nbytes.value // 8, dtype=torch.int64, device=dev)
    perm = torch.empty(n, dtype=torch.int64, device=dev)
    price = torch.empty(n, dtype=torch.int64, device=dev)
    e, qmax = ctypes.c_int32(), ctypes.c_int64()
    left, done = ctypes.c_int64(), ctypes.c_int64()
    with torch.cuda.device(dev.index):
        s = _stream(cost)
        _lib.check(L.amh_assign_begin(_lib.ptr(cost), n, _lib.ptr(work), s))
        if L.amh_assign_quantum(_lib.ptr(work), n, ctypes.byref(e), ctypes.byref(qmax), s) != 0:
            raise ValueError(L.amh_last_error(None).decode())
        eps = max(1, qmax.value // 2)
        rounds = phases = 0
        converged = True
        while True:
            phases += 1
            _lib.check(L.amh_assign_phase(_lib.ptr(work), n, s))
            bound, queued = n, 0
            while bound > 0:
                batch = min(ASSIGN_BATCH, max_rounds - rounds)
                if batch == 0:
                    converged = False
                    break
                _lib.check(L.amh_assign_rounds(_lib.ptr(cost), n, _lib.ptr(work), eps, bound, queued, batch, s))
                queued += batch
                _lib.check(L.amh_assign_status(_lib.ptr(work), n, queued, ctypes.byref(left), ctypes.byref(done), s))
                bound, rounds = left.value, done.value
            if not converged or eps == 1:
                break
            eps = max(1, eps // theta)
        _lib.check(L.amh_assign_result(_lib.ptr(work), n, _lib.ptr(perm), _lib.ptr(price), s))
        mean = float("nan")
        if converged:
            mean = float(cost.gather(1, perm[:, None]).double().sum().item()) / n
    return dict(perm=perm, cost=mean, rounds=rounds, phases=phases, quantum=math.ldexp(1.0, e.value) if qmax.value else 0.0,
                e=e.value, price=price, converged=converged)


def _wasserstein_auction(u_values, v_values, ord) -> float:
    nu, nv = len(u_values), len(v_values)
    if nu != nv:
        raise ValueError(f'method="auction" needs equally many samples, got {nu} and {nv}')
    u, v = _dev(u_values), _dev(v_values)
    if float(ord) == 2.0:
        cost = _dist2(u, v).clamp_(min=0.0).sqrt_()
    else:
        cost = torch.cdist(u, v, p=float(ord))
    res = linear_assignment(cost)
    if not res["converged"]:
        raise RuntimeError(f"linear_assignment: no matching within {res['rounds']} rounds (n = {nu})")
    return res["cost"]


def wasserstein_dist11_p(u_values, v_values, ord=2.0, method="hungarian") -> float:
    """Optimal 1-1 coupling cost (evaluation.py:43-67).  method="hungarian":
    scipy's Hungarian algorithm on the host in float64, as the reference.
    method="auction": cost matrix and matching on the device
    (linear_assignment; float32 costs, within 2 quantum of their optimum)."""
    if method == "auction":
        return _wasserstein_auction(u_values, v_values, ord)
    if method != "hungarian":
        raise ValueError(f'method must be "hungarian" or "auction", got {method!r}')
    from scipy.optimize import linear_sum_assignment
    from scipy.spatial import distance_matrix
    u = np.asarray(u_values.cpu() if hasattr(u_values, "cpu") else u_values)
    v = np.asarray(v_values.cpu() if hasattr(v_values, "cpu") else v_values)
    cost = distance_matrix(u, v, p=ord)
    r, c = linear_sum_assignment(cost)
    return float(cost[r, c].mean())


def _lse_half(cost: torch.Tensor, pot: torch.Tensor, log_w: float, eps: float) -> torch.Tensor:
    """out_i = -eps log sum_j exp((pot_j - cost_ij) / eps + log_w) (HIP)."""
    L = _lib.lib()
    rows, cols = cost.shape
    out = torch.empty(rows, dtype=torch.float32, device=cost.device)
    with torch.cuda.device(cost.device.index):
        _lib.check(L.amh_sinkhorn_lse(_lib.ptr(cost), rows, cols, _lib.ptr(pot), float(log_w), float(eps),
                                      _lib.ptr(out), _stream(cost)))
    return out


def _cost_mode(cost_fn) -> str:
    """'euclidean' / 'sqeuclidean' from a name, or from an ott cost object
    (`costs.Euclidean()`, the reference's default at evaluation.py:69, or
    `costs.SqEuclidean()`) by its class name."""
    name = cost_fn if isinstance(cost_fn, str) else type(cost_fn).__name__
    key = name.lower()
    if key in ("euclidean", "sqeuclidean"):
        return key
    raise ValueError(f"cost_fn must be 'euclidean' / 'sqeuclidean' or an ott Euclidean / SqEuclidean cost, got {cost_fn!r}")


def sinkhorn(u_values, v_values, cost_fn="euclidean", epsilon=None, threshold=1e-3, max_iterations=2000,
             inner_iterations=10, relative_epsilon="std"):
    """Log-domain Sinkhorn between the uniform empirical measures of u (n, d)
    and v (m, d).  Returns dict(cost=ent_reg_cost, f, g, epsilon, iterations,
    error, converged).  Each iteration: f <- -eps LSE_j((g_j - C_ij)/eps + log b),
    then h <- -eps LSE_i((f_i - C_ij)/eps + log a); the column-marginal error
    sum_j b |exp((g_j - h_j)/eps) - 1| is checked every `inner_iterations`
    iterations before g <- h.  The cost matrix is materialised once (and its
    transpose for the column half).

    The default epsilon is 0.05 x the standard deviation of the cost matrix
    (ott's `relative_epsilon="std"` of newer releases); older ott releases
    scaled by the mean (`relative_epsilon="mean"` here).  The reference pins no
    ott version, so which one it saw is unpinned."""
    x, y = _dev(u_values), _dev(v_values)
    if x.shape[1] != y.shape[1]:
        raise ValueError("u_values and v_values need the same dimension")
    C = _dist2(x, y)
    mode = _cost_mode(cost_fn)
    if mode == "euclidean":
        C = C.clamp_(min=0.0).sqrt_()
    if epsilon is None:
        scale = C.double().std(correction=0) if relative_epsilon == "std" else C.double().mean()
        epsilon = 0.05 * float(scale)
    eps = float(epsilon)
    if not eps > 0:
        raise ValueError("epsilon must be positive")
    Ct = C.t().contiguous()
    n, m = C.shape
    la, lb = -math.log(n), -math.log(m)
    g = torch.zeros(m, dtype=torch.float32, device=C.device)
    f = torch.zeros(n, dtype=torch.float32, device=C.device)
    err, it, converged = float("inf"), 0, False
    while it < max_iterations:
        f = _lse_half(C, g, lb, eps)
        h = _lse_half(Ct, f, la, eps)
        it += 1
        if it % inner_iterations == 0 or it == max_iterations:
            err = float(((torch.exp((g.double() - h.double()) / eps) - 1.0).abs().sum() / m).item())
            if err < threshold:
                converged = True
                g = h
                break
        g = h
    cost = float(f.double().mean() + g.double().mean())
    return dict(cost=cost, f=f, g=g, epsilon=eps, iterations=it, error=err, converged=converged)


def wasserstein_sinkhorn(u_values, v_values, cost_fn="euclidean", epsilon=None) -> float:
    """Entropy-regularised OT cost (evaluation.py:69-101: ott PointCloud with
    the Euclidean cost, linear.solve, ent_reg_cost)."""
    return sinkhorn(u_values, v_values, cost_fn=cost_fn, epsilon=epsilon)["cost"]


def wasserstein_sinkhorn_unbiased(u_values, v_values, cost_fn="euclidean", epsilon=None) -> float:
    """W(u, v) - (W(u, u) + W(v, v)) / 2 (evaluation.py:104-130); each term
    with its own default epsilon when epsilon is None, as in the reference."""
    wuv = wasserstein_sinkhorn(u_values, v_values, cost_fn=cost_fn, epsilon=epsilon)
    wuu = wasserstein_sinkhorn(u_values, u_values, cost_fn=cost_fn, epsilon=epsilon)
    wvv = wasserstein_sinkhorn(v_values, v_values, cost_fn=cost_fn, epsilon=epsilon)
    return wuv - (wuu + wvv) / 2


def wasserstein_1d(mu, nu, p=1.0):
    """mean(|sort(mu) - sort(nu)|^p)^(1/p) along the last axis (evaluation.py:139-162)."""
    mu, nu = _dev(mu), _dev(nu)
    diff = torch.abs(torch.sort(mu, dim=-1).values - torch.sort(nu, dim=-1).values)
    return torch.mean(diff ** p, dim=-1) ** (1.0 / p)


def _directions(rng_key, n_directions: int, d: int, device) -> torch.Tensor:
    """n_directions unit vectors: normals of the build's Philox stream
    (amh_normals), each row normalised (evaluation.py:189-190)."""
    z = torch.empty(n_directions, d, dtype=torch.float32, device=device)
    with torch.cuda.device(device.index):
        _lib.check(_lib.lib().amh_normals(_lib.key_arr(as_key(rng_key)), n_directions * d, _lib.ptr(z),
                                          _lib.stream_ptr(device.index)))
    return z / torch.linalg.norm(z, dim=1, keepdim=True)


def max_sliced_wasserstein(mu, nu, rng_key, p=1.0, n_directions=1000) -> float:
    """max over random unit directions of the 1-D Wasserstein-p distance of the
    projections (evaluation.py:165-206)."""
    mu, nu = _dev(mu), _dev(nu)
    dirs = _directions(rng_key, int(n_directions), mu.shape[1], mu.device)
    pm = (mu @ dirs.T).T.contiguous()  # [n_dir, n]
    pn = (nu @ dirs.T).T.contiguous()
    return float(torch.max(wasserstein_1d(pm, pn, p=p)))


def gaussian_kernel(x, y, gamma):
    """exp(-gamma ||x_i - y_j||^2) as an [n, m] device matrix (evaluation.py:209-230)."""
    x, y = _dev(x), _dev(y)
    return torch.exp(-float(gamma) * _dist2(x, y))


def mmd2_unbiased(x, y, gamma=1.0) -> float:
    """Unbiased MMD^2 with a Gaussian kernel (evaluation.py:233-266)."""
    x, y = _dev(x), _dev(y)
    n, m = x.shape[0], y.shape[0]
    sxx = _kernel_sum(x, x, gamma, True)
    syy = _kernel_sum(y, y, gamma, True)
    sxy = _kernel_sum(x, y, gamma, False)
    return sxx / (n * (n - 1)) + syy / (m * (m - 1)) - 2.0 * sxy / (n * m)


def mmd_heuristic(x, y) -> float:
    """Biased MMD with the median heuristic bandwidth gamma = 4 / median of the
    reference sample's squared distances (evaluation.py:269-294)."""
    x, y = _dev(x), _dev(y)
    n, m = x.shape[0], y.shape[0]
    d2 = _dist2(y, y).reshape(-1)
    k = d2.numel()
    lo = torch.kthvalue(d2, (k + 1) // 2).values
    hi = torch.kthvalue(d2, k // 2 + 1).values
    med = float(0.5 * (lo.double() + hi.double())) if k % 2 == 0 else float(lo)
    gamma = 4.0 / med
    sxx = _kernel_sum(x, x, gamma, False)
    syy = _kernel_sum(y, y, gamma, False)
    sxy = _kernel_sum(x, y, gamma, False)
    return math.sqrt(max(sxx / n ** 2 + syy / m ** 2 - 2.0 * sxy / (n * m), 0.0))
