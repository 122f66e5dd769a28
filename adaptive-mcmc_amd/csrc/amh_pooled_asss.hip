// amh_pooled_asss.hip -- pooled ASSS (include/amh.h "pooled ASSS"): every
// chain runs the stereographic slice transition of asss.py:210-244 with one
// shared (mu, L) staged in LDS, and the block's sums S_d, S_dd, S_a, N feed
// the pooled update (amh_pooled.hip pooled_update_kernel<true>).
//
//   pooled_asss_stats_kernel  the lane-per-row form of pooled_stats_kernel:
//                             16 waves per block, one chain per wave at a
//                             time, lane r = coordinate r, on the chunk
//                             scaffold of amh_pooled_device.h
//                             (pooled_chunk_walk); the sums leave through
//                             pooled_chunk_out / pooled_reduce, in the d < 64
//                             ARWMH order at every d <= 64
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
// tangent was degenerate (theta = 0, the point re-projected).  The pieces are
// those of asss_transition (amh_asss.h), the slice walk included, with S read
// from LDS (amh_pooled_asss.h).
template <template <int> class M>
__device__ __forceinline__ bool pooled_asss_transition(const SharedRow& sh, float& x, float& pe, int32_t it,
                                                       uint32_t k0, uint32_t k1, int d, int r, bool act,
                                                       const typename M<64>::Ctx& mctx, const float* lds) {
  constexpr int G = 64;
  float v, vd, ut, th0, zr, zd, Sz, Sv;
  asss_draws<G>(r, it, k0, k1, act, v, vd, ut, th0);
  pooled_asss_project(sh, x, d, r, act, zr, zd);
  const bool degen = asss_tangent<G>(act, zr, zd, v, vd);
  pooled_asss_circle(sh, zr, v, d, act, Sz, Sv);
  const int32_t iter = asss_slice_walk(
      Sz, Sv, zd, vd, sh.mu, act, degen, ut, th0, (float)d, sh.eps, it, k0, k1,
      [&](float xx) __attribute__((always_inline)) { return M<G>::potential(xx, r, d, mctx, lds); }, x, pe);
  return asss_moved(degen, iter);
}

}  // namespace

// EXACT: d = 64 at compile time (the Gaussian at d = 64, as pooled_stats_kernel)
template <template <int> class M, bool EXACT>
__global__ __launch_bounds__(kPoolWaves * 64) void pooled_asss_stats_kernel(PooledStatsParams p) {
  constexpr int G = 64;
  extern __shared__ float lds[];
  const int d = EXACT ? 64 : p.d;
  const int ld = pooled_ld(d);
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

  // the next chain's z / pe / key are loaded while the current one is computed
  struct Q {
    float z, pe;
    uint32_t k0, k1;
  };
  pooled_chunk_walk<Q>(
      p, d, p.k_steps, sh.mu, r, act, w, tree,
      [&](const WaveRows& rows, int64_t c, Q& q) __attribute__((always_inline)) {
        q.z = rows.ld(p.z, c);
        q.pe = p.pe[c];
        q.k0 = p.keys[2 * c];
        q.k1 = p.keys[2 * c + 1];
      },
      // one transition with the frozen shared state; S_a counts the moves
      [&](const Q& q, int t, float& z, float& pe) __attribute__((always_inline)) {
        return pooled_asss_transition<M>(sh, z, pe, it + t, q.k0, q.k1, d, r, act, mctx, lds) ? 1.0f : 0.0f;
      });
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
