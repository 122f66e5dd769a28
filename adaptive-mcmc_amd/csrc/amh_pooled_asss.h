// amh_pooled_asss.h -- the pieces of the pooled ASSS transition that read the
// shared factor from LDS, written once: the fused transition
// (amh_pooled_asss.hip pooled_asss_transition) runs them with the model's
// potential behind them, the begin kernel around a caller's potential
// (amh_pooled_asss_ext.hip) runs them and stops where the first U is needed.
// A wave owns the chain, lane r = coordinate r, G = 64 at every d; the draws,
// the tangent, the circle's points and the slice walk (the fused transition)
// are amh_asss.h's own pieces at G = 64.
#pragma once
#include "amh_asss.h"
#include "amh_pooled_device.h"

namespace amh {

// The frozen shared state as one lane sees it: S = (L + eps I) sqrt(d) with
// row r of L in LDS at prow (asss.py:213).
struct SharedRow {
  uint32_t prow;  // LDS address of row r of the staged factor (row 0 in lanes r >= d)
  float mu;       // mu_r
  float invD;     // 1 / S_rr
  float sd;       // sqrt(d)
  float epsd;     // eps sqrt(d)
  float eps;
};

// lane r's view of the factor staged at lrow (pooled_stage_factor, after the
// block's barrier) and of the shared mean
__device__ __forceinline__ SharedRow pooled_asss_shared_row(const float* lrow, const float* __restrict__ mu, float eps,
                                                            int d, int r, bool act) {
  const int ld = pooled_ld(d);
  SharedRow sh;
  sh.sd = sqrtf((float)d);
  sh.eps = eps;
  sh.epsd = eps * sh.sd;
  sh.mu = act ? mu[r] : 0.0f;
  sh.prow = lds_addr(lrow + (act ? r : 0) * ld);
  sh.invD = act ? 1.0f / ((lrow[r * ld + r] + eps) * sh.sd) : 0.0f;
  return sh;
}

// ---- y = S^-1 (x - mu) and its stereographic projection (zr, zd) on S^d
// (asss.py:40-45, 214).  Forward substitution as a column sweep over the LDS
// rows, 16 columns per batch (zero above the diagonal: lanes r <= j are left
// alone, lane j's own b is spent once y_j is taken)
__device__ __forceinline__ void pooled_asss_project(const SharedRow& sh, float x, int d, int r, bool act, float& zr,
                                                    float& zd) {
  constexpr int G = 64;
  using Gp = Grp<G>;
  float b = act ? x - sh.mu : 0.0f;
  float y = 0.0f;
  static_for<4>([&](auto B) {
    constexpr int bq = B;
    if (16 * bq < d) {
      f32x4 pv[4];
      static_for<4>([&](auto Q) {
        pv[Q] = (4 * (4 * bq + Q) < d) ? lds_ld4<16 * (4 * bq + Q)>(sh.prow) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      });
      lds_wait(pv[0], pv[1], pv[2], pv[3]);
      static_for<16>([&](auto Q) {
        constexpr int j = 16 * bq + Q;
        if (j < d) {
          const float yj = Gp::template bcast<j>(b * sh.invD);
          y = capture<G, j>(y, yj, r);
          b = fmaf(-pv[Q / 4][Q % 4], yj * sh.sd, b);
        }
      });
      __builtin_amdgcn_sched_barrier(0);
    }
  });
  const float ns = Gp::sum(act ? y * y : 0.0f);
  const float den = ns + 1.0f;
  zr = act ? (2.0f * y) / den : 0.0f;
  zd = (ns - 1.0f) / den;
}

// ---- S z_1d and S v_1d (asss.py:48-56 for both circle directions)
__device__ __forceinline__ void pooled_asss_circle(const SharedRow& sh, float zr, float v, int d, bool act, float& Sz,
                                                   float& Sv) {
  Sz = lds_row_dot64(sh.prow, d, sh.sd * zr, act) + sh.epsd * zr;
  Sv = lds_row_dot64(sh.prow, d, sh.sd * v, act) + sh.epsd * v;
}

}  // namespace amh
