// amh_asss_ext.hip -- ASSS (python/kernels/asss.py:197-251) with the caller's
// potential (AMH_MODEL_EXTERNAL), d <= 64 on gfx950: the transition of
// amh_asss.h cut at every potential evaluation.
//
// The transition evaluates U only on the slice circle: at theta = 0 (the
// current point re-projected, x0) and at each candidate of the shrinkage.
// Every point of the circle is O(d) once S z and S v are formed, so a
// transition is
//
//   begin     draws, y = S^-1 (x - mu), projection, tangent, S z, S v, x0 and
//             the first candidate -> cand[0], cand[1] and the chain's record
//   the caller's U of cand[0] and cand[1]
//   shrink 0  the slice level from U(x0); tests the first candidate; a chain
//             that is off the slice narrows its bracket, draws and writes the
//             next candidate to cand[1]
//   the caller's U of cand[1]; shrink 1; ... until no chain continues (round
//             50 stops every chain: asss.py:59 max_iterations)
//   finish    the outcome (x0 when capped or degenerate), the adaptation and
//             the store of the state, as asss_step_kernel
//
// with the float operations of amh_asss.h (the same inline functions as the
// fused kernels, the same lane mapping and group width G = dispatch_dim's), so
// given the same U the bits are those of asss_step_kernel / orc_asss_step.
//
// A chain that has stopped is not touched again: its cand[1] row keeps the
// accepted point and its record keeps the U of the round that accepted it, so
// later evaluations of that row (every round evaluates all rows) are ignored.
//
// The record of chain c is asss_ext_work_floats(d) floats at work + c * that:
// S z [d], S v [d], mu [d], then the scalars kZd .. kKey1 of amh_asss.h (the
// pooled begin kernel of amh_pooled_asss_ext.hip writes the same record).
#include "amh_asss.h"

namespace amh {

namespace {

template <int G>
__device__ __forceinline__ int64_t wave_items(int64_t C, int64_t& wave0, int64_t& wstride) {
  wave0 = (int64_t)blockIdx.x * (kBlock / 64) + threadIdx.x / 64;
  wstride = (int64_t)gridDim.x * (kBlock / 64);
  return (C + Geo<G>::CPW - 1) / Geo<G>::CPW;
}

}  // namespace

// ------------------------------------------------------------------ begin ----
// FROZEN: sample_Pnx (asss.py:271-303), transition q.t of chain c from
// x_cur[c] with the shared (loc, scale) and the key split(key)[c]
template <int DMAX, bool FROZEN>
__global__ __launch_bounds__(kBlock) void asss_ext_begin_kernel(AsssExtParams q) {
  constexpr int G = DMAX;
  const StepParams& p = q.sp;
  const int d = p.d;
  const int64_t C = p.C;
  const int64_t P = (int64_t)d * (d + 1) / 2;
  const int64_t WS = asss_ext_work_floats(d);
  const float sd = sqrtf((float)d);
  int64_t wave0, wstride;
  const int64_t n_items = wave_items<G>(C, wave0, wstride);
  for (int64_t item = wave0; item < n_items; item += wstride) {
    int lane = lane_id();
    asm volatile("" : "+v"(lane));  // keep per-column lane masks inside the item loop
    const int r = lane & (G - 1);
    const bool act = r < d;
    const int64_t chain = item_chain<G>(item);
    const bool chain_ok = chain < C;
    const int64_t cl = chain_ok ? chain : C - 1;

    float dl, U[DMAX];
    asss_load_factor<DMAX>(FROZEN ? q.scale : p.in.scale + cl * P, d, r, r, act, U, dl);
    const float x = act ? (FROZEN ? q.x_cur[cl * d + r] : p.in.z[cl * d + r]) : 0.0f;
    const float mu = act ? (FROZEN ? q.loc[r] : p.in.loc[cl * d + r]) : 0.0f;
    int32_t it;
    uint32_t k0, k1;
    if constexpr (FROZEN) {
      const amh_u32x4 kk = amh_philox4x32_10((uint32_t)cl, (uint32_t)((uint64_t)cl >> 32), 0u, AMH_TAG_SPLIT,
                                             q.key0, q.key1);
      it = q.t;
      k0 = kk.v[0];
      k1 = kk.v[1];
    } else {
      it = p.in.i[cl];
      k0 = (uint32_t)p.in.rng_key[2 * cl];
      k1 = (uint32_t)p.in.rng_key[2 * cl + 1];
    }

    float v, vd, ut, th0, zr, zd, Sz, Sv;
    asss_draws<G>(r, it, k0, k1, act, v, vd, ut, th0);
    asss_project<DMAX>(U, dl, sd, p.eps, x, mu, d, r, act, zr, zd);
    const bool degen = asss_tangent<G>(act, zr, zd, v, vd);
    asss_circle<DMAX>(U, dl, sd, p.eps, zr, v, d, Sz, Sv);
    float om0, om, s, c;
    const float x0 = asss_x_at(Sz, Sv, zd, vd, mu, act, 1.0f, 0.0f, om0);
    amh_sincosf(th0, &s, &c);
    const float xt = asss_x_at(Sz, Sv, zd, vd, mu, act, c, s, om);

    if (chain_ok) {
      float* w = q.work + chain * WS;
      if (act) {
        q.cand[chain * d + r] = x0;
        q.cand[(C + chain) * d + r] = xt;
        w[r] = Sz;
        w[d + r] = Sv;
        w[2 * d + r] = mu;
      }
      if (r == 0) asss_ext_record_init(w + 3 * d, zd, vd, th0, ut, om0, om, degen, it, k0, k1);
    }
  }
}

// ----------------------------------------------------------------- shrink ----
// Round q.round of the shrinkage (asss.py:59-96) for the chains still
// continuing: q.pe[C + c] is the caller's U of cand[1][c], candidate number
// q.round; round 0 also reads q.pe[c] = U(x0) and forms the slice level.
template <int G>
__global__ __launch_bounds__(kBlock) void asss_ext_shrink_kernel(AsssExtParams q) {
  const StepParams& p = q.sp;
  const int d = p.d;
  const int64_t C = p.C;
  const int64_t WS = asss_ext_work_floats(d);
  const float fd = (float)d;
  const int32_t round = q.round;
  int64_t wave0, wstride;
  const int64_t n_items = wave_items<G>(C, wave0, wstride);
  for (int64_t item = wave0; item < n_items; item += wstride) {
    const int r = lane_id() & (G - 1);
    const bool act = r < d;
    const int64_t chain = item_chain<G>(item);
    const bool chain_ok = chain < C;
    const int64_t cl = chain_ok ? chain : C - 1;
    float* w = q.work + cl * WS;
    float* sc = w + 3 * d;
    int32_t* si = (int32_t*)sc;
    const bool on = chain_ok && si[kCont] != 0;  // group-uniform
    if (!on) continue;  // a stopped chain is not touched again (no cross-lane work below)

    const float un = q.pe[C + cl];
    float tpe, U0 = 0.0f;
    if (round == 0) {
      U0 = q.pe[cl];
      tpe = asss_level(U0, fd, sc[kOm0], sc[kUt]);
    } else {
      tpe = sc[kTpe];
    }
    const float om_c = sc[kOm];
    const float pt = asss_slice_pt(un, fd, om_c);
    const bool off = (pt > tpe) || (om_c < p.eps);
    const bool cont = (round == 0) ? (si[kDegen] == 0 && off) : ((round < kAsssMaxIter) && off);

    float th_n = 0.0f, thmin_n = 0.0f, thmax_n = 0.0f, om = 0.0f;
    if (cont) {
      const int32_t it = si[kIt];
      const uint32_t k0 = (uint32_t)si[kKey0], k1 = (uint32_t)si[kKey1];
      th_n = asss_narrow(sc[kTh], sc[kThmin], sc[kThmax], round, it, k0, k1, thmin_n, thmax_n);
      float s, c;
      amh_sincosf(th_n, &s, &c);
      const float Sz = act ? w[r] : 0.0f, Sv = act ? w[d + r] : 0.0f, mu = act ? w[2 * d + r] : 0.0f;
      const float xn = asss_x_at(Sz, Sv, sc[kZd], sc[kVd], mu, act, c, s, om);
      if (act) q.cand[(C + cl) * d + r] = xn;
    }
    if (r == 0) {
      // the group's lanes sit in one wave and have used what they read of the
      // record above, so these stores cannot overtake a read
      sc[kUx] = un;  // the U of this round: kept when the chain stops here
      si[kIter] = round;
      si[kCont] = cont ? 1 : 0;
      if (round == 0) {
        sc[kTpe] = tpe;
        sc[kU0] = U0;
      }
      if (cont) {
        sc[kTh] = th_n;
        sc[kThmin] = thmin_n;
        sc[kThmax] = thmax_n;
        sc[kOm] = om;
        atomicAdd(&q.active[round], 1);
      }
    }
  }
}

// ----------------------------------------------------------------- finish ----
template <int DMAX>
__global__ __launch_bounds__(kBlock) void asss_ext_finish_kernel(AsssExtParams q) {
  constexpr int G = DMAX;
  const StepParams& p = q.sp;
  const int d = p.d;
  const int64_t C = p.C;
  const int64_t P = (int64_t)d * (d + 1) / 2;
  const int64_t WS = asss_ext_work_floats(d);
  int64_t wave0, wstride;
  const int64_t n_items = wave_items<G>(C, wave0, wstride);
  for (int64_t item = wave0; item < n_items; item += wstride) {
    int lane = lane_id();
    asm volatile("" : "+v"(lane));
    const int r = lane & (G - 1);
    const bool act = r < d;
    const int64_t chain = item_chain<G>(item);
    const bool chain_ok = chain < C;
    const int64_t cl = chain_ok ? chain : C - 1;

    const float* Lin = p.in.scale + cl * P;
    float dl, U[DMAX];
    asss_load_factor<DMAX>(Lin, d, r, r, act, U, dl);
    float mu = act ? p.in.loc[cl * d + r] : 0.0f;
    const int32_t it = p.in.i[cl];
    float asc = p.in.as_change[cl];
    const uint32_t k0 = (uint32_t)p.in.rng_key[2 * cl], k1 = (uint32_t)p.in.rng_key[2 * cl + 1];
    bool updated = false;

    const float* sc = q.work + cl * WS + 3 * d;
    const int32_t* si = (const int32_t*)sc;
    const float x0 = act ? q.cand[cl * d + r] : 0.0f;
    const float xt = act ? q.cand[(C + cl) * d + r] : 0.0f;
    float x, pe;
    asss_outcome(si[kDegen] != 0, si[kIter], x0, xt, sc[kU0], sc[kUx], x, pe);
    asss_adapt<DMAX>(p, U, dl, mu, asc, updated, it, x, d, r, act);

    if (chain_ok) {
      if (p.col_z != nullptr && act) p.col_z[chain * d + r] = x;
      if (p.col_pe != nullptr && r == 0) p.col_pe[chain] = pe;
      asss_store_factor<DMAX>(p.out.scale + chain * P, Lin, U, dl, updated, d, r, act);
      if (act) {
        p.out.z[chain * d + r] = x;
        p.out.loc[chain * d + r] = mu;
      }
      if (r == 0) {
        p.out.i[chain] = it + 1;
        p.out.potential_energy[chain] = pe;
        p.out.as_change[chain] = asc;
        p.out.rng_key[2 * chain] = k0;
        p.out.rng_key[2 * chain + 1] = k1;
      }
    }
  }
}

// sample_Pnx: the outcome back to x_cur, nothing else
template <int G>
__global__ __launch_bounds__(kBlock) void asss_ext_pnx_finish_kernel(AsssExtParams q) {
  const int d = q.sp.d;
  const int64_t C = q.sp.C;
  const int64_t WS = asss_ext_work_floats(d);
  int64_t wave0, wstride;
  const int64_t n_items = wave_items<G>(C, wave0, wstride);
  for (int64_t item = wave0; item < n_items; item += wstride) {
    const int r = lane_id() & (G - 1);
    const bool act = r < d;
    const int64_t chain = item_chain<G>(item);
    if (chain >= C || !act) continue;
    const float* sc = q.work + chain * WS + 3 * d;
    const int32_t* si = (const int32_t*)sc;
    float x, pe;
    asss_outcome(si[kDegen] != 0, si[kIter], q.cand[chain * d + r], q.cand[(C + chain) * d + r], sc[kU0], sc[kUx], x,
                 pe);
    q.x_cur[chain * d + r] = x;
  }
}

// -------------------------------------------------------------- launchers ----
namespace {

template <class K>
hipError_t launch_ext(K kern, int cpw, const AsssExtParams& q, hipStream_t s) {
  const int64_t n_items = (q.sp.C + cpw - 1) / cpw;
  int64_t blocks = (n_items + kBlock / 64 - 1) / (kBlock / 64);
  if (blocks > 256 * 32) blocks = 256 * 32;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(kBlock), 0, s, q);
  return hipGetLastError();
}

// the group width of dimension d is dispatch_dim's, as the fused kernels'
struct ExtF {
  const AsssExtParams& q;
  int pass;  // 0 begin, 1 shrink, 2 finish
  bool frozen;
  hipStream_t s;
  template <int D, template <int> class M, bool E>
  hipError_t operator()() const {
    constexpr int cpw = Geo<D>::CPW;
    if (pass == 0)
      return frozen ? launch_ext(asss_ext_begin_kernel<D, true>, cpw, q, s)
                    : launch_ext(asss_ext_begin_kernel<D, false>, cpw, q, s);
    if (pass == 1) return launch_ext(asss_ext_shrink_kernel<D>, cpw, q, s);
    return frozen ? launch_ext(asss_ext_pnx_finish_kernel<D>, cpw, q, s)
                  : launch_ext(asss_ext_finish_kernel<D>, cpw, q, s);
  }
};

}  // namespace

hipError_t run_asss_ext_begin(const AsssExtParams& q, bool frozen, hipStream_t s) {
  if (q.sp.C < 1) return hipErrorInvalidValue;
  return dispatch_dim<ExtPotM>(q.sp.d, false, ExtF{q, 0, frozen, s});
}

hipError_t run_asss_ext_shrink(const AsssExtParams& q, hipStream_t s) {
  if (q.sp.C < 1 || q.round < 0 || q.round > kAsssMaxIter) return hipErrorInvalidValue;
  return dispatch_dim<ExtPotM>(q.sp.d, false, ExtF{q, 1, false, s});
}

hipError_t run_asss_ext_finish(const AsssExtParams& q, bool frozen, hipStream_t s) {
  if (q.sp.C < 1) return hipErrorInvalidValue;
  return dispatch_dim<ExtPotM>(q.sp.d, false, ExtF{q, 2, frozen, s});
}

}  // namespace amh
