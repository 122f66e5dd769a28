// amh_pooled_asss_ext.hip -- pooled ASSS (include/amh.h "pooled ASSS") with
// the caller's potential (AMH_MODEL_EXTERNAL), d <= 64 on gfx950: the
// transition of amh_pooled_asss.hip cut at every potential evaluation, as
// amh_asss_ext.hip cuts the per-chain one.
//
//   pooled_asss_ext_begin_kernel   draws, y = S^-1 (x - mu) from the LDS-staged
//                                  shared factor, projection, tangent, S z, S v,
//                                  x(theta = 0) -> cand[0], x(theta_0) -> cand[1]
//                                  and the chain's record
//   the caller's U of cand, then amh_asss_ext_shrink round by round, unchanged:
//   it has no cross-lane arithmetic, and the record is amh_asss_ext_begin's
//   (S z [d], S v [d], mu [d] -- the shared mu copied per chain -- and the
//   scalars kZd .. kKey1 of amh_asss.h)
//   pooled_asss_ext_finish_kernel  the outcome (asss_outcome), z' / pe' out, and
//                                  the transition's pooled sums on the chunk
//                                  scaffold of pooled_asss_stats_kernel
//                                  (pooled_chunk_walk), so that
//                                  one transition's sums are that kernel's at
//                                  k_steps = 1 byte for byte
//
// Per chain the float operations are those of pooled_asss_transition (the
// shared pieces of amh_pooled_asss.h and amh_asss.h) with U read instead of
// computed.
#include "amh_pooled_asss.h"

namespace amh {

// ------------------------------------------------------------------ begin ----
// Wave w of block b takes the chains b * 16 + w, + 16 gridDim.x, ..: a chain's
// record depends on no other chain, so any assignment gives the same bits.  The
// next chain's z row and key are loaded while the current one is computed.
// LDS: the staged factor alone.  EXACT: d = 64 at compile time.
template <bool EXACT>
__global__ __launch_bounds__(kPoolWaves * 64) void pooled_asss_ext_begin_kernel(PooledAsssExtParams q) {
  constexpr int G = 64;
  extern __shared__ float lds[];
  const PooledExtParams& p = q.sp;
  const int d = EXACT ? 64 : p.d;
  const int64_t C = p.C;
  const int64_t WS = asss_ext_work_floats(d);
  pooled_stage_factor(lds, p.L, d);
  __syncthreads();

  const int r = lane_id();
  const bool act = r < d;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64));
  const int32_t it = __builtin_amdgcn_readfirstlane(p.i[0] + p.t);
  const SharedRow sh = pooled_asss_shared_row(lds, p.mu, p.eps, d, r, act);
  const uint32_t vr = 4u * (uint32_t)r;
  const uint32_t row = 4u * (uint32_t)d;

  auto load_chain = [&](int64_t c, float& zz, uint32_t& q0, uint32_t& q1) {
    const Buf bz(uniform_ptr(p.z + c * d), row);
    zz = bz.ld(vr, 0);
    q0 = p.keys[2 * c];
    q1 = p.keys[2 * c + 1];
  };
  const int64_t stride = (int64_t)gridDim.x * kPoolWaves;
  int64_t c = (int64_t)blockIdx.x * kPoolWaves + w;
  float zq = 0.0f;
  uint32_t k0q = 0, k1q = 0;
  if (c < C) load_chain(c, zq, k0q, k1q);
  for (; c < C; c += stride) {
    const float x = zq;
    const uint32_t k0 = k0q, k1 = k1q;
    if (c + stride < C) load_chain(c + stride, zq, k0q, k1q);

    float v, vd, ut, th0, zr, zd, Sz, Sv;
    asss_draws<G>(r, it, k0, k1, act, v, vd, ut, th0);
    pooled_asss_project(sh, x, d, r, act, zr, zd);
    const bool degen = asss_tangent<G>(act, zr, zd, v, vd);
    pooled_asss_circle(sh, zr, v, d, act, Sz, Sv);
    float om0, om, s, cs;
    const float x0 = asss_x_at(Sz, Sv, zd, vd, sh.mu, act, 1.0f, 0.0f, om0);
    amh_sincosf(th0, &s, &cs);
    const float xt = asss_x_at(Sz, Sv, zd, vd, sh.mu, act, cs, s, om);

    // (buffer descriptors with a wave-uniform base: lanes r >= d store nothing)
    const Buf b0(uniform_ptr(q.cand + c * d), row);
    const Buf b1(uniform_ptr(q.cand + (C + c) * d), row);
    b0.st(x0, vr, 0);
    b1.st(xt, vr, 0);
    float* wk = q.work + c * WS;
    if (act) {
      wk[r] = Sz;
      wk[d + r] = Sv;
      wk[2 * d + r] = sh.mu;
    }
    if (r == 0) asss_ext_record_init(wk + 3 * d, zd, vd, th0, ut, om0, om, degen, it, k0, k1);
  }
}

// ----------------------------------------------------------------- finish ----
// The chunk layout of pooled_asss_stats_kernel: block b is chunk b, wave w
// takes its chains [b 16 cpw + w cpw, + cpw) in order (pooled_ext_stats_kernel
// with asss_outcome in place of accept), on pooled_chunk_walk: the next chain's
// candidates and record are loaded while the current one is accumulated.
template <bool EXACT>
__global__ __launch_bounds__(kPoolWaves * 64) void pooled_asss_ext_finish_kernel(PooledAsssExtParams q) {
  extern __shared__ float tree[];
  const PooledExtParams& p = q.sp;
  const int d = EXACT ? 64 : p.d;
  const int64_t C = p.C;
  const int64_t WS = asss_ext_work_floats(d);
  const int r = lane_id();
  const bool act = r < d;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64));
  const float mu = act ? p.mu[r] : 0.0f;

  // a chain's state is the point at theta = 0 and its U until the outcome
  struct Q {
    float z, pe, xt, ux;
    int32_t degen, iter;
  };
  pooled_chunk_walk<Q>(
      p, d, 1, mu, r, act, w, tree,
      [&](const WaveRows& rows, int64_t c, Q& n) __attribute__((always_inline)) {
        n.z = rows.ld(q.cand, c);
        n.xt = rows.ld(q.cand, C + c);
        const float* sc = q.work + c * WS + 3 * d;
        const int32_t* si = (const int32_t*)sc;
        n.degen = si[kDegen];
        n.iter = si[kIter];
        n.pe = sc[kU0];
        n.ux = sc[kUx];
      },
      [&](const Q& n, int, float& z, float& pe) __attribute__((always_inline)) {
        asss_outcome(n.degen != 0, n.iter, n.z, n.xt, n.pe, n.ux, z, pe);
        return asss_moved(n.degen != 0, n.iter) ? 1.0f : 0.0f;
      });
}

// -------------------------------------------------------------- launchers ----
hipError_t run_pooled_asss_ext_begin(const PooledAsssExtParams& q, hipStream_t s) {
  const int d = q.sp.d;
  if (d < 1 || d > 64 || q.sp.C < 1) return hipErrorInvalidValue;
  // the kernel holds no sums, so the grid is not the chunks': enough blocks
  // for every chain to have its wave, at most two per CU -- what 16-wave blocks
  // fit -- so that a block stages the factor once and then strides over chains
  const size_t shm = (size_t)d * pooled_ld(d) * sizeof(float);
  const int64_t want = (q.sp.C + kPoolWaves - 1) / kPoolWaves;
  const int cus = cu_count();
  const int64_t cap = 2 * (int64_t)(cus > 0 ? cus : 1);
  const dim3 grid((unsigned)(want < cap ? want : cap)), block(kPoolWaves * 64);
  if (d == 64) {
    hipLaunchKernelGGL(pooled_asss_ext_begin_kernel<true>, grid, block, shm, s, q);
  } else {
    hipLaunchKernelGGL(pooled_asss_ext_begin_kernel<false>, grid, block, shm, s, q);
  }
  return hipGetLastError();
}

hipError_t run_pooled_asss_ext_finish(const PooledAsssExtParams& q, double* sums, int accumulate, hipStream_t s) {
  const int d = q.sp.d;
  if (d < 1 || d > 64 || q.sp.C < 1 || q.sp.cpw < 1) return hipErrorInvalidValue;
  const int64_t chunk = (int64_t)kPoolWaves * q.sp.cpw;
  const int64_t n_chunks = (q.sp.C + chunk - 1) / chunk;
  const dim3 grid((unsigned)n_chunks), block(kPoolWaves * 64);
  const size_t shm = kPooledTreeFloats * sizeof(float);
  if (d == 64) {
    hipLaunchKernelGGL(pooled_asss_ext_finish_kernel<true>, grid, block, shm, s, q);
  } else {
    hipLaunchKernelGGL(pooled_asss_ext_finish_kernel<false>, grid, block, shm, s, q);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return pooled_reduce(q.sp.partials, n_chunks, pooled_sums_len(d), sums, accumulate, s);
}

}  // namespace amh
