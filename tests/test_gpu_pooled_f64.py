"""The pooled kernels (amh_pooled_*, amh_big_pooled, amh_pooled_ext,
amh_pooled_exact) against the float64 restatement oracle/pooled_np.py, with
many chains and from a warm start in the typical set.  The C oracle is not in
the loop: per-chain state, the sums (teacher-forced on the z the kernel wrote)
and the update (teacher-forced on the kernel's own sums) sit within the
bounds of pooled_np.bounds, which come from the reference and the number
formats alone.  tests/test_pooled_f64.py holds the oracle to the same
reference and shows that the bounds reject six shared misreadings."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import (apply_shared, make_case, pooled_f64_blocks, pooled_ref_model, pooled_reference_shares,
                     pooled_warm_start, shared_to_host)

pytestmark = pytest.mark.gpu

SEED = 7
SHARE = (0.10, 0.50)


class GpuPooled:
    """PooledARWMH behind the interface helpers.pooled_f64_blocks drives."""

    def __init__(self, kind, d, C, K, W, z0, sh, external=False, **opts):
        from kernels_amd import PooledARWMH, PRNGKey
        kw, mk, om = make_case(kind, d)
        if external:
            kw = dict(potential_fn=_torch_gaussian(om))
        self.k = PooledARWMH(num_chains=C, sync_every=K, **opts, **kw)
        self.K, self.C, self.d = K, C, om.d
        self.st = apply_shared(self.k.init(PRNGKey(SEED), W, torch.as_tensor(z0), (), mk), sh)
        for name, v in shared_to_host(self.st).items():  # the warm state arrived bit for bit
            assert v.tobytes() == np.asarray(sh[name]).astype(v.dtype).tobytes(), name

    def keys(self):
        return self.st.rng_key.cpu().numpy().view(np.uint32)

    def shared(self):
        torch.cuda.synchronize()
        return shared_to_host(self.st)

    def z_host(self):
        return self.st.z.cpu().numpy()

    def history(self):
        """The block's K frozen transitions as K single amh_pooled_stats
        launches at noise positions i + t (the shared leaves untouched)."""
        from kernels_amd import _lib
        st, dev = self.st, self.st.z.device
        a = st.adapt_state
        z, pe, out = st.z, st.potential_energy, []
        sums = torch.zeros(self.k._sums.shape[0], dtype=torch.float64, device=dev)
        for t in range(self.K):
            it = st.i + t
            ps = _lib.AmhPooledState(it.data_ptr(), z.data_ptr(), pe.data_ptr(), st.rng_key.data_ptr(),
                                     st.mean_accept_prob.data_ptr(), a.loc.data_ptr(), a.scale.data_ptr(),
                                     a.log_step_size.data_ptr(), st.as_change.data_ptr(), st.cov.data_ptr())
            zo, po = torch.empty_like(z), torch.empty_like(pe)
            rc = _lib.lib().amh_pooled_stats(self.k._handle.h, self.C, ctypes.byref(ps), _lib.ptr(zo), _lib.ptr(po),
                                             _lib.ptr(sums), _lib.stream_ptr(dev.index))
            _lib.check(rc, self.k._handle.h)
            torch.cuda.synchronize()
            z, pe = zo, po
            out.append(zo.cpu().numpy())
        return out, pe.cpu().numpy()

    def block(self):
        self.st = self.k.sample(self.st)
        torch.cuda.synchronize()
        return self.st.z.cpu().numpy(), self.st.potential_energy.cpu().numpy(), self.k._sums.cpu().numpy()


def _torch_gaussian(om):
    """The case's Gaussian as a caller's torch potential: float64 arithmetic
    on the chains' float32 z, rounded once (inside any float32 bound)."""
    d = om.d
    data = torch.as_tensor(np.asarray(om.data, np.float64))
    cache = {}

    def U(z):
        if z.device not in cache:
            t = data.to(z.device)
            cache[z.device] = (t[:d], t[d:d + d * d].reshape(d, d), t[d + d * d])
        m, P, c0 = cache[z.device]
        y = z.to(torch.float64) - m
        return (0.5 * ((y @ P) * y).sum(1) + c0).to(torch.float32)
    return U


def _run(kind, d, C, K, W=0, external=False, **opts):
    import arwmh_np as lit
    from kernels_amd import PRNGKey
    _, _, om = make_case(kind, d)
    model = pooled_ref_model(kind, om)
    z0, sh = pooled_warm_start(kind, d, C, SEED, K)
    keys = lit.chain_keys(PRNGKey(SEED), 0, C)
    # the condition, on the float64 reference alone and before any kernel runs
    shares = pooled_reference_shares(model, keys, z0, sh, K, W, 3)
    print("reference accepted share per block:", " ".join(f"{s:.3f}" for s in shares))
    assert all(SHARE[0] <= s <= SHARE[1] for s in shares), shares
    impl = GpuPooled(kind, d, C, K, W, z0, sh, external=external, **opts)
    assert np.array_equal(impl.keys(), keys)
    return pooled_f64_blocks(impl, model, keys, K, W)


@pytest.mark.parametrize("kind,d,C,K", [("gaussian", 7, 517, 1), ("gaussian", 7, 517, 4),
                                        ("eight_schools", None, 70, 1),
                                        ("gaussian", 64, 300, 1), ("gaussian", 64, 300, 4),
                                        ("gaussian", 96, 257, 1),
                                        ("gaussian", 128, 300, 1), ("gaussian", 128, 300, 3),
                                        ("gaussian", 256, 257, 1)])
def test_pooled_against_float64(kind, d, C, K, gpu):
    """d = 7: pooled_stats_kernel (wave tree, 33 chunks with a ragged last
    one) and the double Cholesky; eight schools: a non-Gaussian potential;
    d = 64: pooled_fused64_kernel (2 chunks + 44 chains) and
    pooled_update64_kernel; d = 96 / 128 / 256: pooled_fused_big_kernel at NT =
    3 (a last chunk of one chain), 4 (blocks summed in step order) and 8
    (panel Cholesky with look-ahead)."""
    _run(kind, d, C, K)


def test_pooled_against_float64_at_the_reset(gpu):
    """num_warmup = 21 from i = 20: the second block is the schedule's reset,
    gamma = 1, so Sigma' = S_dd / N alone (C >= 2 d keeps it positive
    definite) and mu' = mu + S_d / N."""
    _run("gaussian", 64, 300, 1, W=21)


def test_pooled_exact_sums_against_float64(gpu):
    """exact_sums = True: the sums converted back from the fixed-point words
    obey the bounds of the default path."""
    _run("gaussian", 64, 300, 1, exact_sums=True)


@pytest.mark.parametrize("d", [40, 128])
def test_pooled_external_against_float64(d, gpu):
    """A caller's torch potential: pooled_ext_* (propose, then accept and
    sums) below and above d = 64."""
    _run("gaussian", d, 300, 1, external=True)
