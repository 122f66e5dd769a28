// amh_pooled_device.h -- device pieces of the pooled mode's lane-per-row form
// (d < 64, and the d = 64 registry models off the MFMA path) shared by the
// fused kernel (amh_pooled.hip) and the kernels split around the caller's
// potential (amh_pooled_ext.hip): the shared factor's row dot from LDS, a
// chain-step's contribution to the wave's sums, and the chunk's combine tree.
// Every order here is part of the bit spec (oracle: orc_pooled_stats_k).
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

}  // namespace amh
