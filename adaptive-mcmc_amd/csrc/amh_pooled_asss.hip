// amh_pooled_asss.hip -- pooled ASSS (include/amh.h "pooled ASSS"): every
// chain runs the stereographic slice transition of asss.py:210-244 with one
// shared (mu, L) staged in LDS, and the block's sums S_d, S_dd, S_a, N feed
// the pooled update (amh_pooled.hip pooled_update_kernel<true>).
//
//   pooled_asss_stats_kernel  the lane-per-row form of pooled_stats_kernel:
//                             16 waves per block, one chain per wave at a
//                             time, lane r = coordinate r; the sums leave
//                             through pooled_chunk_out / pooled_reduce, in the
//                             d < 64 ARWMH order at every d <= 64
//
// Noise: the per-chain ASSS stream of amh_asss.h at position i + t with the
// chain's key (oracle/asss_np.draws).
#include "amh_device.h"
#include "amh_pooled_asss.h"

namespace amh {

namespace {

// One ASSS transition (asss.py:210-244) of the wave's chain at stream position
// `it` against the shared state; x / pe are replaced by x' / pe'.  Returns
// whether the chain moved: false when the shrinkage reached its cap or the
// tangent was degenerate (theta = 0, the point re-projected).  The sphere
// arithmetic is that of asss_transition (amh_asss.h) with S read from LDS.
template <template <int> class M>
__device__ __forceinline__ bool pooled_asss_transition(const SharedRow& sh, float& x, float& pe, int32_t it,
                                                       uint32_t k0, uint32_t k1, int d, int r, bool act,
                                                       const typename M<64>::Ctx& mctx, const float* lds) {
  constexpr int G = 64;
  using Gp = Grp<G>;
  const float fd = (float)d;
  const float mu = sh.mu;
  // ---- draws (asss.py:207, 219, 225, 60)
  const amh_u32x4 o = amh_philox4x32_10((uint32_t)r, (uint32_t)it, 0u, AMH_TAG_ASSS, k0, k1);
  float v = act ? amh_normal_from_bits(o.v[0]) : 0.0f;
  float vd = amh_normal_from_bits(Gp::template bcast_u<0>(o.v[1]));
  const float ut = amh_unif01_from_bits(Gp::template bcast_u<0>(o.v[2]));
  const float th0 = 6.28318548f * amh_unif01_from_bits(Gp::template bcast_u<0>(o.v[3]));

  // ---- y = S^-1 (x - mu) and its stereographic projection (asss.py:40-45)
  float zr, zd;
  pooled_asss_project(sh, x, d, r, act, zr, zd);

  // ---- v orthogonal to z on S^d (asss.py:219-222), projected with fmaf and
  // with the degenerate tangent's fallback theta = 0, as amh_asss.h
  const float dot = Gp::sum(act ? v * zr : 0.0f) + (vd * zd);
  v = act ? fmaf(-dot, zr, v) : 0.0f;
  vd = fmaf(-dot, zd, vd);
  const float nv = sqrtf(Gp::sum(v * v) + (vd * vd));
  const bool degen = !(nv > 0.0f);  // wave-uniform
  v = degen ? 0.0f : v / nv;
  vd = degen ? 0.0f : vd / nv;

  // ---- S z_1d and S v_1d (asss.py:48-56 for both circle directions)
  float Sz, Sv;
  pooled_asss_circle(sh, zr, v, d, act, Sz, Sv);

  // x on the circle at angle (c, s); om = 1 - z_d(th)
  auto x_at = [&](float c, float s, float& om) -> float {
    const float zdt = (zd * c) + (vd * s);
    om = 1.0f - zdt;
    return act ? (((Sz * c) + (Sv * s)) / om) + mu : 0.0f;
  };

  // ---- slice level at z (asss.py:216-217, 224-226)
  float om0;
  const float x0 = x_at(1.0f, 0.0f, om0);
  const float U0 = M<G>::potential(x0, r, d, mctx, lds);
  const float tpe = (U0 + fd * amh_logf(om0)) - amh_logf(ut);

  // ---- shrinkage (asss.py:59-96)
  float th = th0, thmin = th0 - 6.28318548f, thmax = th0;
  int32_t iter = 0;
  float xt, ux;
  bool cont;
  {
    float s, c, om;
    amh_sincosf(th, &s, &c);
    xt = x_at(c, s, om);
    ux = M<G>::potential(xt, r, d, mctx, lds);
    float pt = ux + fd * amh_logf(om);
    if (amh_isnan(pt)) pt = INFINITY;
    cont = !degen && ((pt > tpe) || (om < sh.eps));
  }
  while (__ballot(cont) != 0ull) {
    const float thmin_n = (th < 0.0f) ? th : thmin;
    const float thmax_n = (th >= 0.0f) ? th : thmax;
    const amh_u32x4 ok = amh_philox4x32_10((uint32_t)iter, (uint32_t)it, 1u, AMH_TAG_ASSS, k0, k1);
    const float th_n = thmin_n + (thmax_n - thmin_n) * amh_unif01_from_bits(ok.v[0]);
    float s, c, om;
    amh_sincosf(th_n, &s, &c);
    const float xn = x_at(c, s, om);
    const float un = M<G>::potential(xn, r, d, mctx, lds);
    float pt = un + fd * amh_logf(om);
    if (amh_isnan(pt)) pt = INFINITY;
    if (cont) {
      thmin = thmin_n;
      thmax = thmax_n;
      th = th_n;
      xt = xn;
      ux = un;
      iter += 1;
      cont = (iter < kAsssMaxIter) && ((pt > tpe) || (om < sh.eps));
    }
  }
  const bool capped = degen || iter >= kAsssMaxIter;  // asss.py:94: theta = 0
  x = capped ? x0 : xt;
  float pen = capped ? U0 : ux;
  if (amh_isnan(pen)) pen = INFINITY;  // asss.py:234
  pe = pen;
  return !capped;
}

}  // namespace

// EXACT: d = 64 at compile time (the Gaussian at d = 64, as pooled_stats_kernel)
template <template <int> class M, bool EXACT>
__global__ __launch_bounds__(kPoolWaves * 64) void pooled_asss_stats_kernel(PooledStatsParams p) {
  constexpr int G = 64;
  extern __shared__ float lds[];
  const int d = EXACT ? 64 : p.d;
  const int ld = pooled_ld(d);
  const int64_t P = (int64_t)d * (d + 1) / 2;
  const int64_t V = d + P + 2;
  float* lrow = lds + pooled_lds_model_floats<M>(p.model, d);
  float* tree = lrow + (size_t)d * ld;

  M<G>::stage(lds, p.model, d);
  pooled_stage_factor(lrow, p.L, d);
  __syncthreads();

  const int r = lane_id();
  const bool act = r < d;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64));
  const auto mctx = M<G>::prepare(p.model, d, r);
  const int32_t it = __builtin_amdgcn_readfirstlane(p.i[0]);
  const SharedRow sh = pooled_asss_shared_row(lrow, p.mu, p.eps, d, r, act);

  const int cpw = p.cpw;
  const int64_t chunk0 = (int64_t)blockIdx.x * kPoolWaves * cpw;
  const int64_t base = chunk0 + (int64_t)w * cpw;
  float S[64];
  static_for<64>([&](auto K) { S[K] = 0.0f; });
  float sd = 0.0f, sa = 0.0f;
  // this wave's chains [base, end); the next chain's z / pe / key are loaded
  // while the current one is computed (as pooled_stats_kernel)
  const int64_t end = (base + cpw < p.C) ? base + cpw : p.C;
  const uint32_t vr = 4u * (uint32_t)r;
  auto load_chain = [&](int64_t c, float& zz, float& pp, uint32_t& q0, uint32_t& q1) {
    const Buf bz(uniform_ptr(p.z + c * d), 4u * (uint32_t)d);
    zz = bz.ld(vr, 0);
    pp = p.pe[c];
    q0 = p.keys[2 * c];
    q1 = p.keys[2 * c + 1];
  };
  float zq = 0.0f, peq = 0.0f;
  uint32_t k0q = 0, k1q = 0;
  if (base < end) load_chain(base, zq, peq, k0q, k1q);
  const int K = p.k_steps;
  for (int64_t c = base; c < end; ++c) {
    float z = zq, pe = peq;
    const uint32_t k0 = k0q, k1 = k1q;
    if (c + 1 < end) load_chain(c + 1, zq, peq, k0q, k1q);
    // K transitions with the frozen shared state
    for (int t = 0; t < K; ++t) {
      const bool moved = pooled_asss_transition<M>(sh, z, pe, it + t, k0, k1, d, r, act, mctx, lds);
      // pooled statistics, in the order of pooled_stats_kernel
      const float delta = act ? z - sh.mu : 0.0f;
      pooled_accumulate(S, sd, delta, d);
      sa = sa + (moved ? 1.0f : 0.0f);
    }
    const Buf bo(uniform_ptr(p.z_out + c * d), 4u * (uint32_t)d);
    bo.st(z, vr, 0);
    if (r == 0) p.pe_out[c] = pe;
  }
  const int64_t left = p.C - chunk0;
  const int64_t full = (int64_t)kPoolWaves * cpw;
  pooled_chunk_out(S, sd, sa, tree, r, act, w, d, p.partials + (int64_t)blockIdx.x * V,
                   (double)K * (double)(left < full ? left : full));
}

namespace {

template <template <int> class M, bool EXACT = false>
hipError_t launch_pooled_asss_stats(const PooledStatsParams& p, double* sums, hipStream_t s) {
  const size_t shm = pooled_lds_bytes<M>(p.model, p.d);
  if (shm > 163840) return hipErrorInvalidConfiguration;
  const int64_t chunk = (int64_t)kPoolWaves * p.cpw;
  const int64_t n_chunks = (p.C + chunk - 1) / chunk;
  hipLaunchKernelGGL((pooled_asss_stats_kernel<M, EXACT>), dim3((unsigned)n_chunks), dim3(kPoolWaves * 64), shm, s, p);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return pooled_reduce(p.partials, n_chunks, pooled_sums_len(p.d), sums, 0, s);
}

}  // namespace

bool pooled_asss_model(int model_id, int d) {
  switch (model_id) {
    case AMH_MODEL_GAUSSIAN:
    case AMH_MODEL_EIGHT_SCHOOLS:
    case AMH_MODEL_KIDIQ:
    case AMH_MODEL_DIAMONDS:
      return d >= 1 && d <= 64;
    case AMH_MODEL_DIAMONDS_SS:
      return d >= 3 && d <= 32;
    case AMH_MODEL_POISSON:
      return d >= 2 && d <= 32;
    default:
      return false;
  }
}

hipError_t run_pooled_asss_stats(int model_id, const PooledStatsParams& p, double* sums, hipStream_t s) {
  if (!pooled_asss_model(model_id, p.d)) return hipErrorInvalidValue;
  switch (model_id) {
    case AMH_MODEL_GAUSSIAN:
      return p.d == 64 ? launch_pooled_asss_stats<GaussianM, true>(p, sums, s)
                       : launch_pooled_asss_stats<GaussianM>(p, sums, s);
    case AMH_MODEL_EIGHT_SCHOOLS:
      return launch_pooled_asss_stats<EightSchoolsM>(p, sums, s);
    case AMH_MODEL_KIDIQ:
      return launch_pooled_asss_stats<KidiqM>(p, sums, s);
    case AMH_MODEL_DIAMONDS:
      return launch_pooled_asss_stats<DiamondsM>(p, sums, s);
    case AMH_MODEL_POISSON:
      return launch_pooled_asss_stats<PoissonM>(p, sums, s);
    default:
      return launch_pooled_asss_stats<DiamondsSSM>(p, sums, s);
  }
}

}  // namespace amh
