// amh_pooled_device.h -- device pieces of the pooled mode's lane-per-row form
// (d < 64, and the d = 64 registry models off the MFMA path) shared by the
// fused kernels (amh_pooled.hip, amh_pooled_asss.hip) and the kernels split
// around the caller's potential (amh_pooled_ext.hip, amh_pooled_asss_ext.hip):
// the shared factor's row dot from LDS, a chain-step's contribution to the
// wave's sums, the chunk's combine tree, and the chunk scaffold around them
// (PooledChunk, pooled_chunk_walk).  Every order here is part of the bit spec
// (oracle: orc_pooled_stats_k).
#pragma once
#include "amh_device.h"

namespace amh {

// Shared-factor row r as stored in LDS (dense, zero above the diagonal, rows
// padded like the Gaussian precision) dotted with v broadcast from lane j:
// partial sums over j mod 4, read 16 columns at a time.
__device__ __forceinline__ float lds_row_dot64(uint32_t prow, int d, float v, bool act) {
  using Gp = Grp<64>;
  f32x2v y01 = {0.0f, 0.0f}, y23 = {0.0f, 0.0f};
  static_for<4>([&](auto B) {
    constexpr int b = B;
    if (16 * b < d) {
      f32x4 pv[4];
      static_for<4>([&](auto Q) {
        pv[Q] = (4 * (4 * b + Q) < d) ? lds_ld4<16 * (4 * b + Q)>(prow) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      });
      lds_wait(pv[0], pv[1], pv[2], pv[3]);
      // columns (j, j+1) through one v_pk_fma_f32 into accumulators (j mod 4,
      // j+1 mod 4); a column past d adds 0 * 0 (padded row, inactive lane)
      static_for<8>([&](auto K2) {
        constexpr int j = 16 * b + 2 * K2;
        if (j < d) {
          const f32x4 q = pv[K2 / 2];
          const f32x2v pp = (K2 % 2 == 0) ? f32x2v{q[0], q[1]} : f32x2v{q[2], q[3]};
          const f32x2v pa = act ? pp : f32x2v{0.0f, 0.0f};
          const f32x2v bp = {Gp::template bcast<j>(v), Gp::template bcast<j + 1>(v)};
          if constexpr (K2 % 2 == 0) {
            y01 = __builtin_elementwise_fma(pa, bp, y01);
          } else {
            y23 = __builtin_elementwise_fma(pa, bp, y23);
          }
        }
      });
      __builtin_amdgcn_sched_barrier(0);
    }
  });
  return (y01[0] + y01[1]) + (y23[0] + y23[1]);
}

// LDS row stride of the staged factor
__host__ __device__ inline int pooled_ld(int d) { return ((d + 3) & ~3) + 4; }

// the shared factor (packed lower) -> dense LDS rows of stride pooled_ld(d),
// zero above the diagonal and in the padding; block-cooperative, no barrier
__device__ __forceinline__ void pooled_stage_factor(float* lrow, const float* __restrict__ L, int d) {
  const int ld = pooled_ld(d);
  for (int k = threadIdx.x; k < d * ld; k += blockDim.x) {
    const int row = k / ld, col = k - row * ld;
    lrow[k] = (col <= row && col < d) ? L[col_off(d, col) + (row - col)] : 0.0f;
  }
}

// combine-tree slot: rows r = 0..63 as [S_r0 .. S_rr, sd_r], then sa
constexpr int kTreeSlot = 64 * 65 / 2 + 64 + 1;
constexpr size_t kPooledTreeFloats = (size_t)(kPoolWaves / 2) * kTreeSlot;

// LDS of a lane-per-row stats block: the model's staged data (rounded up to
// 16 bytes), the factor's d rows, the combine tree
template <template <int> class M>
__host__ __device__ inline size_t pooled_lds_model_floats(const ModelArgs& m, int d) {
  return (M<64>::lds_bytes(m, d) / sizeof(float) + 3) & ~(size_t)3;
}
template <template <int> class M>
__host__ __device__ inline size_t pooled_lds_bytes(const ModelArgs& m, int d) {
  const size_t f = pooled_lds_model_floats<M>(m, d) + (size_t)d * pooled_ld(d);
  return (f + kPooledTreeFloats) * sizeof(float);
}

// One chain-step's delta (lane r = row r; 0 in lanes r >= d) into the wave's
// float32 sums: sd += delta_r, (S_k, S_k+1) += delta_r (delta_k, delta_k+1)
// through one v_pk_fma_f32 per pair (each half is the same fmaf; past d the
// broadcast delta is 0).
__device__ __forceinline__ void pooled_accumulate(float (&S)[64], float& sd, float delta, int d) {
  using Gp = Grp<64>;
  sd = sd + delta;
  static_for<32>([&](auto K2) {
    constexpr int k = 2 * K2;
    if (k < d) {
      const f32x2v bp = {Gp::template bcast<k>(delta), Gp::template bcast<k + 1>(delta)};
      const f32x2v sp = __builtin_elementwise_fma(f32x2v{delta, delta}, bp, f32x2v{S[k], S[k + 1]});
      S[k] = sp[0];
      S[k + 1] = sp[1];
    }
    column_fence<k + 1>();
  });
}

// The chunk's 16 wave partials are combined by a fixed pairwise tree in
// float32 (h = 8, 4, 2, 1: wave w < h adds wave w + h), through LDS slots
// holding each row r as [S_r0 .. S_rr, sd_r] (row offset r(r+3)/2) and sa
// last; the chunk total is then written in double (oracle mirror) to `out`
// ([S_d | S_dd packed | S_a | N], N = count).  Block-wide: every wave calls it.
__device__ __forceinline__ void pooled_chunk_out(float (&S)[64], float sd, float sa, float* tree, int r, bool act,
                                                 int w, int d, double* out, double count) {
  const int lane = r;
  const int64_t P = (int64_t)d * (d + 1) / 2;
  const uint32_t rowoff = (uint32_t)(r * (r + 3) / 2);
  static_for<4>([&](auto H) {
    constexpr int h = 8 >> H;
    if (w >= h && w < 2 * h) {
      float* slot = tree + (size_t)(w - h) * kTreeSlot;
      if (act) {
        static_for<64>([&](auto K) {
          constexpr int k = K;
          if (k <= r) slot[rowoff + k] = S[k];
        });
        slot[rowoff + r + 1] = sd;
      }
      if (lane == 0) slot[kTreeSlot - 1] = sa;
    }
    __syncthreads();
    if (w < h) {
      const float* slot = tree + (size_t)w * kTreeSlot;
      if (act) {
        static_for<64>([&](auto K) {
          constexpr int k = K;
          if (k <= r) S[k] = S[k] + slot[rowoff + k];
        });
        sd = sd + slot[rowoff + r + 1];
      }
      sa = sa + slot[kTreeSlot - 1];
    }
    __syncthreads();
  });
  if (w == 0) {
    if (act) {
      static_for<64>([&](auto K) {
        constexpr int k = K;
        if (k <= r) out[d + col_off(d, k) + (r - k)] = (double)S[k];
      });
      out[r] = (double)sd;
    }
    if (lane == 0) {
      out[d + P] = (double)sa;
      out[d + P + 1] = count;
    }
  }
}

// Row c of a [C][d] array as the wave sees it, lane r = coordinate r, through
// a buffer descriptor with a wave-uniform base: no 64-bit per-lane addresses
// to keep live, lanes r >= d read 0 / store nothing.
struct WaveRows {
  int d;
  uint32_t vr, bytes;
  __device__ __forceinline__ WaveRows(const int& d_, const int& r) : d(d_), vr(4u * (uint32_t)r), bytes(4u * (uint32_t)d_) {}
  __device__ __forceinline__ float ld(const float* a, const int64_t& c) const {
    return Buf(uniform_ptr(a + c * d), bytes).ld(vr, 0);
  }
  __device__ __forceinline__ void st(float* a, const int64_t& c, const float& v) const {
    Buf(uniform_ptr(a + c * d), bytes).st(v, vr, 0);
  }
};

// The chunk scaffold of the lane-per-row stats kernels, as pooled_stats_kernel
// (amh_pooled.hip) and pooled_ext_stats_kernel (amh_pooled_ext.hip) write it
// out and pooled_asss_stats_kernel and pooled_asss_ext_finish_kernel take it
// from here: block b is chunk b, wave w takes its chains [base, end) = [b 16 cpw + w cpw,
// + cpw) in order, adds every chain-step to its float32 sums and stores the
// chain; the sums leave through pooled_chunk_out with N = K * the chunk's
// chains.  `p` (PooledStatsParams / PooledExtParams) gives C, cpw, z_out,
// pe_out and partials.  The order of the chains, and of a chain's steps, is
// part of the bit spec.  (Scalars come by reference throughout: these kernels
// run 1024-thread blocks at the 128-VGPR cap, and a by-value copy at an inlined
// call moves their register allocation.)
struct PooledChunk {
  int64_t chunk0, base, end;
  float S[64], sd, sa;
  WaveRows rows;
  template <class Params>
  __device__ __forceinline__ PooledChunk(const Params& p, const int& d, const int& r, const int& w)
      : chunk0((int64_t)blockIdx.x * kPoolWaves * p.cpw), base(chunk0 + (int64_t)w * p.cpw), rows(d, r) {
    static_for<64>([&](auto J) { S[J] = 0.0f; });
    sd = sa = 0.0f;
    end = (base + p.cpw < p.C) ? base + p.cpw : p.C;
  }
  // one chain-step: the state z after it and its share `a` of S_a
  __device__ __forceinline__ void add(const float& z, const float& mu, const float& a, const bool& act, const int& d) {
    const float delta = act ? z - mu : 0.0f;
    pooled_accumulate(S, sd, delta, d);
    sa = sa + a;
  }
  // chain c after its steps
  template <class Params>
  __device__ __forceinline__ void store(const Params& p, const int64_t& c, const float& z, const float& pe, const int& r) const {
    rows.st(p.z_out, c, z);
    if (r == 0) p.pe_out[c] = pe;
  }
  // the 16 wave partials -> the chunk's partial row (fixed float32 tree, then
  // double), K steps per chain.  Block-wide: every wave calls it.
  template <class Params>
  __device__ __forceinline__ void out(const Params& p, float* tree, const int& K, const int& r, const bool& act, const int& w,
                                  const int& d) {
    const int64_t left = p.C - chunk0;
    const int64_t full = (int64_t)kPoolWaves * p.cpw;
    pooled_chunk_out(S, sd, sa, tree, r, act, w, d, p.partials + (int64_t)blockIdx.x * pooled_sums_len(d),
                     (double)K * (double)(left < full ? left : full));
  }
};

// The whole scaffold around two callables, per chain
//   load(rows, c, q)    fetches what chain c needs into q, a Q whose z / pe are
//                       the chain's state; it runs one chain ahead, while the
//                       current chain is computed
//   step(q, t, z, pe)   step t < K of the chain: replaces z / pe and returns the
//                       step's share of S_a
template <class Q, class Params, class Load, class Step>
__device__ __forceinline__ void pooled_chunk_walk(const Params& p, const int& d, const int& K, const float& mu,
                                                  const int& r, const bool& act, const int& w, float* tree,
                                                  Load&& load, Step&& step) {
  PooledChunk ck(p, d, r, w);
  Q nxt{};
  if (ck.base < ck.end) load(ck.rows, ck.base, nxt);
  for (int64_t c = ck.base; c < ck.end; ++c) {
    const Q cur = nxt;
    if (c + 1 < ck.end) load(ck.rows, c + 1, nxt);
    float z = cur.z, pe = cur.pe;
    for (int t = 0; t < K; ++t) {
      const float a = step(cur, t, z, pe);
      ck.add(z, mu, a, act, d);
    }
    ck.store(p, c, z, pe, r);
  }
  ck.out(p, tree, K, r, act, w, d);
}

}  // namespace amh
