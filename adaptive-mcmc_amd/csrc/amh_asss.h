// amh_asss.h -- one ASSS transition (python/kernels/asss.py:197-251) of a
// lane group's chain, shared by the ASSS kernels (amh_asss.hip), the d = 64
// persistent step kernel's ASSS instantiation (amh_step64.hip), pooled ASSS
// (amh_pooled_asss.hip) and, piece by piece, the kernels around a caller's
// potential (amh_asss_ext.hip, amh_pooled_asss_ext.hip).  Bit spec:
// oracle/amh_oracle.c orc_asss_step.
#pragma once
#include "amh_device.h"

namespace amh {

constexpr int kAsssMaxIter = 50;  // asss.py:59 max_iterations

// The scalar slots of a chain's record in the transition cut around a caller's
// potential (after S z, S v and mu; asss_ext_work_floats): written by the begin
// kernels of amh_asss_ext.hip and amh_pooled_asss_ext.hip, advanced by
// asss_ext_shrink_kernel, read by the finish kernels.
enum : int {
  kZd, kVd, kTh, kThmin, kThmax, kIter, kUt, kOm0, kOm, kDegen, kCont, kTpe, kU0, kUx, kIt, kKey0, kKey1, kNumScalars
};
static_assert(kNumScalars <= kAsssExtScalars, "record too small");

// The pieces of one transition (asss.py:197-251), each written once: the fused
// transitions (asss_transition below, pooled_asss_transition of
// amh_pooled_asss.hip) run them back to back, with the model's potential
// inside asss_slice_walk; asss_big_chain (amh_big.hip) runs the scalar ones in
// a wave-uniform loop of its own; the external-potential kernels
// (amh_asss_ext.hip) run the same pieces cut at every potential evaluation,
// with the caller's U in between.  A group of G lanes owns the chain, lane r
// holds row r; `act` = r < d.

// ---- the chain's factor from its packed lower triangle L (column j holds
// rows j .. d-1): lane r gets dl = L_rr and row r in unit-lower form, U[j] =
// L_rj / L_jj below the diagonal, U_rr = 1, 0 above (as the ARWMH kernel)
template <int DMAX>
__device__ __forceinline__ void asss_load_factor(const float* Lin, int d, int r, int rr, bool act, float (&U)[DMAX],
                                                 float& dl) {
  constexpr int G = DMAX;
  using Gp = Grp<G>;
  dl = act ? Lin[col_off(d, r)] : 0.0f;
  const float inv = (amh_isfinite(dl) && dl != 0.0f) ? 1.0f / dl : 0.0f;
  static_for<DMAX>([&](auto J) {
    constexpr int j = J;
    U[j] = 0.0f;
    if (j < d) {
      const float lv = (act && r > j) ? Lin[col_off(d, j) + (r - j)] : 0.0f;
      U[j] = set_one_at<G, j>(keep_above<G, j>(lv * Gp::template bcast<j>(inv), rr), rr);
    }
  });
}

// ... and back: L = U diag(dl) if a step updated it, else the input verbatim
// (nothing to write when Lout is Lin)
template <int DMAX>
__device__ __forceinline__ void asss_store_factor(float* Lout, const float* Lin, const float (&U)[DMAX], float dl,
                                                  bool updated, int d, int r, bool act) {
  using Gp = Grp<DMAX>;
  static_for<DMAX>([&](auto J) {
    constexpr int j = J;
    if (j < d) {
      const float dj = Gp::template bcast<j>(dl);
      if (act && r >= j) {
        const int64_t o = col_off(d, j) + (r - j);
        if (updated) {
          Lout[o] = U[j] * dj;
        } else if (Lout != Lin) {
          Lout[o] = Lin[o];
        }
      }
    }
  });
}

// ---- draws at stream position `it` (asss.py:207, 219, 225, 60): lane r of
// Philox(r, it, 0) gives v_r; lane 0's other words give v_d, u_t and th_0
template <int G>
__device__ __forceinline__ void asss_draws(int r, int32_t it, uint32_t k0, uint32_t k1, bool act, float& v, float& vd,
                                           float& ut, float& th0) {
  using Gp = Grp<G>;
  const amh_u32x4 o = amh_philox4x32_10((uint32_t)r, (uint32_t)it, 0u, AMH_TAG_ASSS, k0, k1);
  v = act ? amh_normal_from_bits(o.v[0]) : 0.0f;
  vd = amh_normal_from_bits(Gp::template bcast_u<0>(o.v[1]));
  ut = amh_unif01_from_bits(Gp::template bcast_u<0>(o.v[2]));
  th0 = 6.28318548f * amh_unif01_from_bits(Gp::template bcast_u<0>(o.v[3]));
}

// ---- y = S^-1 (x - mu), S = (L + eps I) sqrt(d) (S_rj = U_rj e_j below the
// diagonal, S_rr = D_r; sd = sqrt(d)), and its stereographic projection
// (zr, zd) on S^d (asss.py:40-45, 214)
template <int DMAX>
__device__ __forceinline__ void asss_project(const float (&U)[DMAX], float dl, float sd, float eps, float x, float mu,
                                             int d, int rr, bool act, float& zr, float& zd) {
  constexpr int G = DMAX;
  using Gp = Grp<G>;
  const float e = dl * sd;
  const float Dr = (dl + eps) * sd;
  const float invD = 1.0f / Dr;
  float b = act ? x - mu : 0.0f;
  float y = 0.0f;
  static_for<DMAX>([&](auto J) {
    constexpr int j = J;
    if (j < d) {
      const float yl = b * invD;
      y = capture<G, j>(y, Gp::template bcast<j>(yl), rr);
      const float gj = Gp::template bcast<j>(yl * e);
      b = fmaf(-U[j], gj, b);
    }
    column_fence<j>();
  });
  const float ns = Gp::sum(act ? y * y : 0.0f);
  const float den = ns + 1.0f;
  zr = act ? (2.0f * y) / den : 0.0f;
  zd = (ns - 1.0f) / den;
}

// ---- v orthogonal to z on S^d (asss.py:219-222); returns `degen`
// v - (v.z) z with one rounding per component (fmaf): with the product
// rounded first, a draw numerically parallel to z (about 1e-9 per
// transition at d = 1) cancelled to exactly 0 -- a mitigation, not a cure:
// if every component still rounds to 0 (|v| = 0, where the reference's
// v / norm(v) is NaN and would poison the chain), the transition is the
// shrinkage's own fallback, theta = 0 (asss.py:94): the state is kept
// (re-projected), the adaptation runs as usual.  Oracle: asss_chain_step.
template <int G>
__device__ __forceinline__ bool asss_tangent(bool act, float zr, float zd, float& v, float& vd) {
  using Gp = Grp<G>;
  const float dot = Gp::sum(act ? v * zr : 0.0f) + (vd * zd);
  v = act ? fmaf(-dot, zr, v) : 0.0f;
  vd = fmaf(-dot, zd, vd);
  const float nv = sqrtf(Gp::sum(v * v) + (vd * vd));
  const bool degen = !(nv > 0.0f);  // group-uniform
  const float vn = v / nv, vdn = vd / nv;
  v = degen ? 0.0f : vn;
  vd = degen ? 0.0f : vdn;
  return degen;
}

// ---- S z_1d and S v_1d (asss.py:48-56 for both circle directions)
template <int DMAX>
__device__ __forceinline__ void asss_circle(const float (&U)[DMAX], float dl, float sd, float eps, float zr, float v,
                                            int d, float& Sz, float& Sv) {
  using Gp = Grp<DMAX>;
  const float e = dl * sd;
  const float epsd = eps * sd;
  float sz4[4] = {0.0f, 0.0f, 0.0f, 0.0f}, sv4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  const float hz = e * zr, hv = e * v;
  static_for<DMAX>([&](auto J) {
    if (J < d) {
      sz4[J & 3] = fmaf(U[J], Gp::template bcast<J>(hz), sz4[J & 3]);
      sv4[J & 3] = fmaf(U[J], Gp::template bcast<J>(hv), sv4[J & 3]);
    }
    column_fence<J, 16>();
  });
  Sz = ((sz4[0] + sz4[1]) + (sz4[2] + sz4[3])) + epsd * zr;
  Sv = ((sv4[0] + sv4[1]) + (sv4[2] + sv4[3])) + epsd * v;
}

// x_r on the circle at angle (c, s); om = 1 - z_d(th)
__device__ __forceinline__ float asss_x_at(float Sz, float Sv, float zd, float vd, float mu, bool act, float c,
                                           float s, float& om) {
  const float zdt = (zd * c) + (vd * s);
  om = 1.0f - zdt;
  return act ? (((Sz * c) + (Sv * s)) / om) + mu : 0.0f;
}

// ---- slice level at z (asss.py:216-217, 224-226), U0 = U(x(th = 0))
__device__ __forceinline__ float asss_level(float U0, float fd, float om0, float ut) {
  return (U0 + fd * amh_logf(om0)) - amh_logf(ut);
}

// the slice test's left side for a candidate with potential u (asss.py:72-76):
// U~ = u + d log(om), NaN -> +inf; the candidate is off the slice when
// U~ > tpe or om < eps
__device__ __forceinline__ float asss_slice_pt(float u, float fd, float om) {
  float pt = u + fd * amh_logf(om);
  if (amh_isnan(pt)) pt = INFINITY;
  return pt;
}

// shrink step `iter` (asss.py:78-92): the bracket narrowed to the rejected
// angle th, and the next angle, drawn from Philox(iter, it, 1)
__device__ __forceinline__ float asss_narrow(float th, float thmin, float thmax, int32_t iter, int32_t it, uint32_t k0,
                                             uint32_t k1, float& thmin_n, float& thmax_n) {
  thmin_n = (th < 0.0f) ? th : thmin;
  thmax_n = (th >= 0.0f) ? th : thmax;
  const amh_u32x4 ok = amh_philox4x32_10((uint32_t)iter, (uint32_t)it, 1u, AMH_TAG_ASSS, k0, k1);
  return thmin_n + (thmax_n - thmin_n) * amh_unif01_from_bits(ok.v[0]);
}

// whether the transition left theta = 0: not when the tangent was degenerate
// or the shrinkage hit its cap after `iter` rounds (asss.py:94)
__device__ __forceinline__ bool asss_moved(bool degen, int32_t iter) { return !(degen || iter >= kAsssMaxIter); }

// the transition's outcome: theta = 0 (the point x0, its U0) when it did not
// move, else the accepted candidate; NaN -> +inf (asss.py:234)
__device__ __forceinline__ void asss_outcome(bool degen, int32_t iter, float x0, float xt, float U0, float ux,
                                             float& xnew, float& pen) {
  const bool capped = !asss_moved(degen, iter);
  xnew = capped ? x0 : xt;
  pen = capped ? U0 : ux;
  if (amh_isnan(pen)) pen = INFINITY;
}

// The initial scalar slots kZd .. kKey1 of a chain's record around a caller's
// potential (one lane writes them): the bracket of the first candidate th0,
// whose om is `om`, no round run yet.
__device__ __forceinline__ void asss_ext_record_init(float* sc, float zd, float vd, float th0, float ut, float om0,
                                                     float om, bool degen, int32_t it, uint32_t k0, uint32_t k1) {
  int32_t* si = (int32_t*)sc;
  sc[kZd] = zd;
  sc[kVd] = vd;
  sc[kTh] = th0;
  sc[kThmin] = th0 - 6.28318548f;
  sc[kThmax] = th0;
  si[kIter] = 0;
  sc[kUt] = ut;
  sc[kOm0] = om0;
  sc[kOm] = om;
  si[kDegen] = degen ? 1 : 0;
  si[kCont] = 1;
  sc[kTpe] = 0.0f;
  sc[kU0] = 0.0f;
  sc[kUx] = 0.0f;
  si[kIt] = it;
  si[kKey0] = (int32_t)k0;
  si[kKey1] = (int32_t)k1;
}

// ---- the slice walk (asss.py:216-226, 59-96) on the circle (Sz, Sv, zd, vd,
// mu) with the potential `Uof`: x -> U (lane r's coordinate in, the group's U
// out): the level at theta = 0, the first candidate th0, the shrinkage -- every
// lane of the wave stays in the loop until no group continues, a group that
// has stopped keeps its point -- and the outcome (xnew, pen).  Returns the
// shrink count.  (The inputs come by reference: copied by value, the pooled
// kernel's DiamondsSS instance, at the 128-VGPR cap, spills 16 bytes more.)
template <class UF>
__device__ __forceinline__ int32_t asss_slice_walk(const float& Sz, const float& Sv, const float& zd, const float& vd,
                                                   const float& mu, const bool& act, const bool& degen,
                                                   const float& ut, const float& th0, const float& fd,
                                                   const float& eps, const int32_t& it, const uint32_t& k0,
                                                   const uint32_t& k1, UF&& Uof, float& xnew, float& pen) {
  // ---- slice level at z
  float om0;
  const float x0 = asss_x_at(Sz, Sv, zd, vd, mu, act, 1.0f, 0.0f, om0);
  const float U0 = Uof(x0);
  const float tpe = asss_level(U0, fd, om0, ut);

  // ---- shrinkage (asss.py:59-96)
  float th = th0, thmin = th0 - 6.28318548f, thmax = th0;
  int32_t iter = 0;
  float xt, ux;
  bool cont;
  {
    float s, c, om;
    amh_sincosf(th, &s, &c);
    xt = asss_x_at(Sz, Sv, zd, vd, mu, act, c, s, om);
    ux = Uof(xt);
    const float pt = asss_slice_pt(ux, fd, om);
    cont = !degen && ((pt > tpe) || (om < eps));
  }
  while (__ballot(cont) != 0ull) {
    float thmin_n, thmax_n;
    const float th_n = asss_narrow(th, thmin, thmax, iter, it, k0, k1, thmin_n, thmax_n);
    float s, c, om;
    amh_sincosf(th_n, &s, &c);
    const float xn = asss_x_at(Sz, Sv, zd, vd, mu, act, c, s, om);
    const float un = Uof(xn);
    const float pt = asss_slice_pt(un, fd, om);
    if (cont) {
      thmin = thmin_n;
      thmax = thmax_n;
      th = th_n;
      xt = xn;
      ux = un;
      iter += 1;
      cont = (iter < kAsssMaxIter) && ((pt > tpe) || (om < eps));
    }
  }
  asss_outcome(degen, iter, x0, xt, U0, ux, xnew, pen);
  return iter;
}

// ---- adaptation (asss.py:237-251) with the new point xnew: as ARWMH
// without the step size.  U, dl (only if `updated` is set), mu and asc are
// replaced.
template <int DMAX>
__device__ __forceinline__ void asss_adapt(const StepParams& p, float (&U)[DMAX], float& dl, float& mu, float& asc,
                                           bool& updated, int32_t it, float xnew, int d, int rr, bool act) {
  constexpr int G = DMAX;
  using Gp = Grp<G>;
  const int32_t itr = it + 1;
  const int32_t n = (it < p.W) ? itr : itr - p.W;
  const float gamma = lookup_gamma<G>(p, n);
  const float delta = act ? xnew - mu : 0.0f;
  const float mun = act ? mu + gamma * delta : 0.0f;
  const float dmu = mun - mu;
  const float locd = sqrtf(Gp::sum(dmu * dmu));

  const float sq = sqrtf(1.0f - gamma);
  const float ajj = sq * dl;
  const float Dg = ajj * ajj;
  const float one = (amh_isfinite(ajj) && ajj != 0.0f) ? 1.0f : __int_as_float(0x7FC00000);
  float w = delta;
  float ws = 0.0f;
  static_for<DMAX>([&](auto J) {
    if (J < d) {
      const float wj = Gp::template bcast<J>(w);
      ws = capture<G, J>(ws, wj, rr);
      w = fmaf(-wj, U[J], w);
    }
    column_fence<J>();
  });
  const float gw2 = act ? gamma * (ws * ws) : 0.0f;
  const float tsc = act ? gw2 / Dg : 0.0f;
  const float bb = 1.0f + Gp::excl_scan(tsc, rr);
  const float g2 = (bb * Dg) + gw2;
  const float dn = g2 / bb;
  const float cc = (gamma * ws) / g2;
  const float q = sqrtf(dn);
  const float dnew = fmaf(cc, 0.0f, one) * q;
  const bool revert = Gp::any(act && amh_isnan(dnew));
  float sdiff = 0.0f;
  if (!revert) {
    // U'_rj = U_rj + c_j w_r^(j+1);  L'_rj - L_rj = U_rj (q_j - dl_j) + (c_j q_j) w_r^(j+1)
    const float ac = q - dl;
    const float bc = cc * q;
    float s4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    w = delta;
    static_for<DMAX>([&](auto J) {
      if (J < d) {
        const float wj = Gp::template bcast<J>(ws);
        const float cj = Gp::template bcast<J>(cc);
        const float aj = Gp::template bcast<J>(ac);
        const float bj = Gp::template bcast<J>(bc);
        const float uo = U[J];
        w = fmaf(-wj, uo, w);
        const float un = fmaf(cj, w, uo);
        const float tt = fmaf(uo, aj, bj * w);
        s4[J & 3] = fmaf(tt, tt, s4[J & 3]);
        U[J] = un;
      }
      column_fence<J>();
    });
    const float sacc = (s4[0] + s4[1]) + (s4[2] + s4[3]);
    sdiff = sqrtf(Gp::sum(act ? sacc : 0.0f));
    dl = act ? q : 0.0f;
    updated = true;
  }
  asc = locd + sdiff;  // asss.py:248-250
  mu = mun;
}

// One ASSS transition of the group's chain (asss.py:197-251) at stream
// position `it`.  ADAPT = false is the frozen kernel of sample_Pnx
// (asss.py:281-296): the shared (U, dl, mu) are used and left unchanged.
template <int DMAX, template <int> class M, bool ADAPT>
__device__ __forceinline__ void asss_transition(const StepParams& p, float (&U)[DMAX], float& dl, float& x,
                                                float& mu, float& pe, float& asc, bool& updated, int32_t it,
                                                uint32_t k0, uint32_t k1, int d, int r, int rr, bool act,
                                                const typename M<DMAX>::Ctx& mctx, const float* lds) {
  constexpr int G = DMAX;
  const float sd = sqrtf((float)d);
  const float fd = (float)d;
  float v, vd, ut, th0, zr, zd, Sz, Sv;
  asss_draws<G>(r, it, k0, k1, act, v, vd, ut, th0);
  asss_project<DMAX>(U, dl, sd, p.eps, x, mu, d, rr, act, zr, zd);
  const bool degen = asss_tangent<G>(act, zr, zd, v, vd);
  asss_circle<DMAX>(U, dl, sd, p.eps, zr, v, d, Sz, Sv);

  float xnew, pen;
  asss_slice_walk(Sz, Sv, zd, vd, mu, act, degen, ut, th0, fd, p.eps, it, k0, k1,
                  [&](float xx) __attribute__((always_inline)) { return M<G>::potential(xx, r, d, mctx, lds); }, xnew,
                  pen);
  if constexpr (ADAPT) asss_adapt<DMAX>(p, U, dl, mu, asc, updated, it, xnew, d, rr, act);
  x = xnew;
  pe = pen;
}

}  // namespace amh
