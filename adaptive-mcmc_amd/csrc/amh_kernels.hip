// amh_kernels.hip -- gfx950 (CDNA4) kernels for the ARWMH hot path.
//
// Reference: savelovme/adaptive-mcmc python/kernels/arwmh.py (ARWMH.sample
// :140-207, ARWMH.init :84-138, ARWMH.sample_Pnx :230-270) and the NumPyro
// rank-one cholesky_update it calls at :190.  This is not a translation: the
// reference runs one chain per XLA:CPU program; here one wavefront lane-group
// owns one chain and the whole transition (RNG, proposal, potential, accept,
// mean / Cholesky / step-size adaptation) runs in registers.
//
// Lane mapping ("lane = row"): a chain of dimension d <= DMAX is owned by a
// group of G = DMAX lanes (G in {1,..,64}); lane r holds row r of the packed
// lower-triangular factor L in DMAX registers A[0..DMAX-1] (A[j] = L_rj, zero
// above the diagonal), plus z_r, mu_r and the per-column scalars of the
// rank-one update.  Column j of L is stored contiguously in HBM (packed,
// column-major), so the load of register j is one coalesced dword access over
// lanes j..d-1 -- no LDS staging and no transposition.
//
// Bit spec: the arithmetic order here is mirrored exactly by the C oracle
// oracle/amh_oracle.c; both compile with -ffp-contract=off and take every
// transcendental from include/amh_math.h.  See DESIGN.md "bit spec".
#include "amh_device.h"
#include "amh_step_stage.h"

#include <cstdlib>

namespace amh {

typedef __attribute__((address_space(3))) float lds_float;

// ------------------------------------------------------- phase stamps --
// Diagnostic build only (-DAMH_STAMPS, tools/stamps.py): per-wave cycle
// totals of the step kernel's phases, read back with amh_diag_stamps().
#ifdef AMH_STAMPS
constexpr int kStampWaves = 1 << 16;
constexpr int kStampSlots = 8;  // wait, store, lds->reg, prefetch, compute, tail, items, wall
__device__ unsigned long long g_stamps[kStampWaves * kStampSlots];
hipError_t diag_stamps_copy(void* host, size_t bytes) {
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_stamps), bytes, 0, hipMemcpyDeviceToHost);
}
#define AMH_STAMP_INIT                             \
  unsigned long long st_acc[kStampSlots] = {0};    \
  unsigned long long st_t0 = __builtin_amdgcn_s_memtime(); \
  unsigned long long st_prev = st_t0;
#define AMH_STAMP(k)                                          \
  {                                                           \
    const unsigned long long t_ = __builtin_amdgcn_s_memtime(); \
    st_acc[k] += t_ - st_prev;                                \
    st_prev = t_;                                             \
  }
#define AMH_STAMP_COUNT(k) st_acc[k] += 1;
#define AMH_STAMP_FLUSH(w)                                                                         \
  {                                                                                                \
    st_acc[7] = __builtin_amdgcn_s_memtime() - st_t0;                                              \
    if ((w) < kStampWaves && lane_id() < kStampSlots) g_stamps[(w) * kStampSlots + lane_id()] = 0; \
    if ((w) < kStampWaves && lane_id() == 0)                                                       \
      for (int k_ = 0; k_ < kStampSlots; ++k_) g_stamps[(w) * kStampSlots + k_] = st_acc[k_];      \
  }
#else
#define AMH_STAMP_INIT
#define AMH_STAMP(k)
#define AMH_STAMP_COUNT(k)
#define AMH_STAMP_FLUSH(w)
#endif

// -------------------------------------------------------------- step kernel --
// One or more ARWMH transitions (arwmh.py:140-207) per chain with the state
// held in registers between steps.
//
// Persistent waves walk the chain groups; while a wave computes one group
// (state in registers) the DMA engine streams the next group's state from HBM
// into the wave's LDS buffer (buffer_load ... lds), so the HBM traffic of
// the state round trip overlaps the arithmetic.
//
// Between steps the factor lives in registers in unit-lower form: U[j] holds
// U_rj = L_rj / L_jj (U_rr = 1 exactly, zero above the diagonal) and `dl`
// holds L_rr.  numpyro's cholesky_update works on exactly this pair (it
// divides the scaled factor by its diagonal, arwmh.py:190), so the update
// needs no per-column masks: the w_r of a row is zeroed exactly when its own
// column passes (w - w*1), which keeps the upper triangle at exact zeros.
// L = U diag(dl) is formed only when the state is written back.
// Step-kernel LDS, in floats: [ model data | WPB wave buffers | ticket ]
template <int G, template <int> class M>
__host__ __device__ __forceinline__ size_t step_wbuf_off(const ModelArgs& m, int d) {
  return (M<G>::lds_bytes(m, d) / sizeof(float) + 3) & ~(size_t)3;
}
template <int G, template <int> class M>
__host__ __device__ __forceinline__ size_t tickets_off(const ModelArgs& m, int d) {
  return step_wbuf_off<G, M>(m, d) + (size_t)(kBlockStep / 64) * wbuf_floats(Geo<G>::CPW, d);
}
// G = 32: per-wave broadcast scratch (64 lanes x 4 floats) after the ticket --
// the column sweeps read a column's four per-column scalars with one
// ds_read_b128 instead of four DPP + permlane16 broadcasts (three
// instructions each at this width)
template <int G, template <int> class M>
__host__ __device__ __forceinline__ size_t bcast_off(const ModelArgs& m, int d) {
  return (tickets_off<G, M>(m, d) + 4 + 3) & ~(size_t)3;
}
constexpr int kBcastFloats = 64 * 4;
template <int G, template <int> class M>
__host__ __device__ __forceinline__ size_t step_lds_bytes(const ModelArgs& m, int d) {
  if (G == 32) return (bcast_off<G, M>(m, d) + (size_t)(kBlockStep / 64) * kBcastFloats) * sizeof(float);
  return (tickets_off<G, M>(m, d) + 4) * sizeof(float);
}
__device__ __forceinline__ void lds_st4(uint32_t a, f32x4 v) {
  asm volatile("ds_write_b128 %0, %1" : : "v"(a), "v"(v) : "memory");
}

// DFIX > 0: d fixed at compile time below the group width (the diamonds
// split path, d = 26 in groups of 32): column offsets become immediates.
template <int DMAX, template <int> class M, bool EXACT, int DFIX = 0>
__global__ __launch_bounds__(kBlockStep) void arwmh_step_kernel(StepParams p) {
  const StepParams& p_outer = p;
  constexpr int G = DMAX;
  constexpr int CPW = Geo<G>::CPW;
  constexpr bool kExt = is_external<M<G>>::value;
  using Gp = Grp<G>;
  extern __shared__ float lds[];
  const int d = EXACT ? DMAX : (DFIX > 0 ? DFIX : p.d);
  M<G>::stage(lds, p.model, d);
  if (threadIdx.x == 0) lds[tickets_off<G, M>(p.model, d)] = 0.0f;  // ticket counter (bits 0)
  __syncthreads();
  const auto mctx = M<G>::prepare(p.model, d, lane_id() & (G - 1));

  const int64_t C = p.C;
  const uint32_t P = (uint32_t)(d * (d + 1) / 2);
  const int64_t n_items = (C + CPW - 1) / CPW;
  [[maybe_unused]] const int64_t wave = (int64_t)blockIdx.x * (kBlockStep / 64) + threadIdx.x / 64;
  const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64));  // wave-uniform
  float* wb = lds + step_wbuf_off<G, M>(p.model, d) + (size_t)wave_in_block * wbuf_floats(CPW, d);
  const float* wL = wb;
  const float* wz = wb + wbuf_L(CPW, d);
  const float* wm = wz + wbuf_zd(CPW, d);
  const float* wsc = wm + wbuf_zd(CPW, d);
  const uint32_t oob = kOOB;
  // G = 32 at a fixed d: sweep 2 and the next proposal's broadcasts through
  // the wave's LDS scratch (the next-proposal form spilled in the ExtPotM
  // instance, 128 VGPRs, so it keeps the one-swap DPP broadcasts there)
  constexpr bool kLdsS2 = G == 32 && DFIX > 0;
  constexpr bool kLdsSP = G == 32 && DFIX > 0 && !kExt;
  constexpr int NB = 4;  // columns per LDS wait
  [[maybe_unused]] const uint32_t bs_a =
      lds_addr(lds + bcast_off<G, M>(p.model, d) + (size_t)wave_in_block * kBcastFloats);

  // Registers carry one chain group at a time.  Iteration k: wait for the
  // DMA of item k, write item k-1 back (its registers are still live), read
  // item k from LDS, start the DMA of item k+1, compute item k.  Stores are
  // issued after the wait, so the next wait never has to drain them.
  float U[DMAX];
  float dl = 0.0f, z = 0.0f, mu = 0.0f, pe = 0.0f, macc = 0.0f, lam = 0.0f, asc = 0.0f;
  [[maybe_unused]] float pe_ext = 0.0f;  // split path: U(z') computed outside
  // split path: the proposal U(z') was evaluated at, read from the split
  // buffer (loaded for the next item while this one computes) instead of
  // formed again -- the same bits (the propose pass / the previous step
  // pass made it from this state), one column sweep and the normals fewer
  [[maybe_unused]] float zp_nx = 0.0f, zp_cur = 0.0f;
  auto load_zp = [&](const StepParams& p, int64_t it_item, int ln) {
    const int rq = ln & (G - 1);
    const int64_t ch = it_item * CPW + ln / G;
    zp_nx = (rq < d && ch < C) ? p.ext_z[ch * d + rq] : 0.0f;
  };
  int32_t it = 0, nacc = 0, acc0 = 0;
  uint32_t k0 = 0, k1 = 0;
  bool updated = false;
  int64_t prev = -1;  // item whose state the registers hold
  static_for<DMAX>([&](auto J) { U[J] = 0.0f; });

  // write the registers' chain group (item `it_item`) back to HBM
  auto store_item = [&](const StepParams& p, int64_t it_item, int lane) {
    const int r = lane & (G - 1);
    const int rr = r;
    const bool act = r < d;
    const int g = lane / G;
    const int64_t first = it_item * CPW;
    const int64_t chain = first + g;
    const bool chain_ok = chain < C;
    // L = U diag(dl); factors no step of this launch updated are copied from
    // the launch input verbatim
    const bool any_upd = Gp::any(updated);
    const uint32_t vrow = (act && chain_ok) ? ((uint32_t)g * P + (uint32_t)r) * 4u : kOOB;
    const uint32_t wave_bytes = (uint32_t)CPW * P * 4u;
    const Buf Lout(uniform_ptr(p.out.scale + first * P), wave_bytes);
    const Buf Lin(uniform_ptr(p.in.scale + first * P), wave_bytes);
    // (the branch is outside the column loop: a per-column select between a
    // load and a product made the compiler wait vmcnt(0) before every store)
    if (any_upd) {
      const auto dls = Gp::src(dl);
      static_for<DMAX>([&](auto J) {
        constexpr int j = J;
        if (j < d) {
          const uint32_t so = (uint32_t)(col_off(d, j) - j) * 4u;
          const float v = U[j] * Gp::template bcast<j>(dls);
          if constexpr (EXACT || DFIX > 0) {
            // d fixed: the column offset as the instruction's immediate (an
            // SGPR offset costs an s_movk + hazard nop per column; kOOB + so
            // stays out of range)
            Lout.st(v, off_from<G, j>(vrow, oob, rr) + so, 0u);
          } else {
            Lout.st(v, off_from<G, j>(vrow, oob, rr), so);
          }
        }
        column_fence<j>();
      });
    } else {
      // verbatim copy: all loads first (into the now dead U registers), then
      // all stores, so the copy waits for memory once
      static_for<(DMAX + 15) / 16>([&](auto B) {  // batches of 16 columns
        static_for<16>([&](auto K) {
          constexpr int j = 16 * B + K;
          if constexpr (j < DMAX) {
            if (j < d) U[j] = Lin.ld(off_from<G, j>(vrow, oob, rr), (uint32_t)(col_off(d, j) - j) * 4u);
          }
        });
        static_for<16>([&](auto K) {
          constexpr int j = 16 * B + K;
          if constexpr (j < DMAX) {
            if (j < d) Lout.st(U[j], off_from<G, j>(vrow, oob, rr), (uint32_t)(col_off(d, j) - j) * 4u);
          }
        });
        __builtin_amdgcn_sched_barrier(0);
      });
    }
    if (chain_ok) {
      if (act) {
        p.out.z[chain * d + r] = z;
        p.out.loc[chain * d + r] = mu;
      }
      if (r == 0) {
        p.out.i[chain] = it;
        p.out.potential_energy[chain] = pe;
        p.out.mean_accept_prob[chain] = macc;
        p.out.log_step_size[chain] = lam;
        p.out.as_change[chain] = asc;
        p.out.rng_key[2 * chain] = k0;
        p.out.rng_key[2 * chain + 1] = k1;
        if (p.accept_count != nullptr) p.accept_count[chain] = acc0 + nacc;  // loaded with the item
      }
    }
  };

  // Chain groups are split into one contiguous range per block; inside a
  // block the waves take groups from an LDS ticket counter, so waves that
  // lose the SIMD's issue arbitration simply process fewer groups (static
  // striding left the slowest wave ~1.4x behind the mean).  The ticket for
  // the group after next is drawn right after a prefetch is issued.  (A
  // single device-wide counter was tried: its global atomics serialise and
  // stall the memory pipeline behind them.)
  const int64_t blk_lo = n_items * (int64_t)blockIdx.x / gridDim.x;
  const int64_t blk_hi = n_items * ((int64_t)blockIdx.x + 1) / gridDim.x;
  const uint32_t tk_addr = lds_addr(lds) + (uint32_t)(tickets_off<G, M>(p.model, d) * sizeof(float));
  auto ticket = [&]() -> int64_t {
    uint32_t v = 0;
    if (lane_id() == 0) {
      asm volatile("ds_add_rtn_u32 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(tk_addr), "v"(1u) : "memory");
    }
    return blk_lo + (int64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)v);
  };
  AMH_STAMP_INIT
  int64_t item = ticket();
  int64_t nxt = item < blk_hi ? ticket() : blk_hi;

  if (item < blk_hi) {
    prefetch_item<G, kExt>(p, item * CPW, d, wb, lane_id());
    if constexpr (kExt) load_zp(p, item, lane_id());
  }
  for (; item < blk_hi;) {
    // Every lane-dependent quantity is derived from an opaque copy of the lane
    // id inside the loop: otherwise the compiler hoists dozens of per-column
    // addresses and masks out of this persistent loop and runs out of VGPRs.
    int lane = lane_id();
    asm volatile("" : "+v"(lane));
    // the launch parameters re-read from the kernarg segment each item
    // (scalar loads through an opaque pointer): kept live across the loop,
    // their ~60 SGPRs spilled to VGPR lanes and every item paid hundreds of
    // v_readlane / v_writelane + hazard nops
    const StepParams& p = reload_kernarg(p_outer);
    const int r = lane & (G - 1);
    const int rr = r;
    const bool act = r < d;
    const int64_t first = item * CPW;
    const int g = lane / G;
    const int64_t chain = first + g;
    const bool chain_ok = chain < C;

    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this item's DMA has landed
    __builtin_amdgcn_s_setprio(3);  // hand-over phase first (as arwmh_step64_kernel): diamonds_ss +1.8 %
    AMH_STAMP(0)
    if (prev >= 0) store_item(p, prev, lane);
    AMH_STAMP(1)

    // ---- state: LDS -> registers
    {
      // LDS addresses made opaque per item so the 64 column addresses are
      // not hoisted out of the chain loop (one base VGPR + immediate offsets)
      lds_float* Lrow = (lds_float*)(wL + g * P + r);
      asm volatile("" : "+v"(Lrow));
      const lds_float* Lg = (const lds_float*)(wL + g * P);
      dl = act ? Lg[col_off(d, r)] : 0.0f;
      const float inv = (amh_isfinite(dl) && dl != 0.0f) ? 1.0f / dl : 0.0f;
      const auto invs = Gp::src(inv);
      static_for<DMAX>([&](auto J) {
        constexpr int j = J;
        U[j] = 0.0f;
        if (j < d) {
          const float x = Lrow[col_off(d, j) - j];  // garbage for r < j: masked below
          U[j] = set_one_at<G, j>(keep_above<G, j>(x * Gp::template bcast<j>(invs), rr), rr);
        }
        column_fence<j>();
      });
      z = act ? wz[g * d + r] : 0.0f;
      mu = act ? wm[g * d + r] : 0.0f;
      it = __float_as_int(wsc[0 * CPW + g]);
      if constexpr (G == 64) it = __builtin_amdgcn_readfirstlane(it);  // wave-uniform: scalar table lookups
      acc0 = (p.accept_count != nullptr && chain_ok && r == 0) ? p.accept_count[chain] : 0;
      pe = wsc[1 * CPW + g];
      macc = wsc[2 * CPW + g];
      lam = wsc[3 * CPW + g];
      asc = wsc[4 * CPW + g];
      k0 = (uint32_t)__float_as_int(wsc[5 * CPW + 2 * g]);
      k1 = (uint32_t)__float_as_int(wsc[5 * CPW + 2 * g + 1]);
      if constexpr (kExt) {
        pe_ext = wsc[7 * CPW + g];
        zp_cur = zp_nx;
      }
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): buffer consumed before it is refilled
    AMH_STAMP(2)
    int64_t nxt2 = blk_hi;
    if (nxt < blk_hi) {
      prefetch_item<G, kExt>(p, nxt * CPW, d, wb, lane);
      if constexpr (kExt) load_zp(p, nxt, lane);
      nxt2 = ticket();
    }
    __builtin_amdgcn_s_setprio(0);
    AMH_STAMP(3)

    nacc = 0;
    updated = false;
    for (int32_t t = 0; t < p.n_steps; ++t) {
      // ---- noise (arwmh.py:162-165, 174): stream position = state.i
      float u, zp;
      const float el = amh_expf(lam);
      if constexpr (kExt) {
        // split path (n_steps == 1): z' from the split buffer, u = U(W_d)
        u = amh_unif01_from_bits(amh_step_word((uint32_t)d, (uint32_t)it, k0, k1));
        zp = act ? zp_cur : 0.0f;
      } else {
        float xi;
        step_noise<G>(r, d, (uint32_t)it, k0, k1, xi, u);
        xi = act ? xi : 0.0f;

        // ---- proposal z' = z + (L e^lam + eps I) xi  (arwmh.py:166-167),
        //      L xi = U (dl * xi)
        const float eta = dl * xi;
        // four interleaved partial sums (columns j mod 4): four independent
        // FMA chains instead of one 64-long dependency chain
        float a4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        static_for<DMAX>([&](auto J) {
          if (J < d) a4[J & 3] = fmaf(U[J], Gp::template bcast<J>(eta), a4[J & 3]);
          column_fence<J, 16>();
        });
        const float acc = (a4[0] + a4[1]) + (a4[2] + a4[3]);
        zp = act ? z + fmaf(el, acc, p.eps * xi) : 0.0f;
      }

      // ---- potential, NaN -> +inf (arwmh.py:169-171)
      float pep;
      if constexpr (kExt) {
        pep = pe_ext;  // n_steps == 1 (host-enforced)
      } else {
        pep = M<G>::potential(zp, r, d, mctx, lds);
      }
      if (amh_isnan(pep)) pep = INFINITY;

      // ---- accept / reject (arwmh.py:173-178)
      const float ex = amh_expf(pe - pep);
      const float alpha = (ex > 1.0f) ? 1.0f : ex;
      const bool accept = u < alpha;
      const float zn = accept ? zp : z;
      const float pen = accept ? pep : pe;
      nacc += accept ? 1 : 0;

      // ---- schedule (arwmh.py:180-185)
      const int32_t itr = it + 1;
      const int32_t n = (it < p.W) ? itr : itr - p.W;
      const float gamma = lookup_gamma<G>(p, n);
      const float maccn = macc + (alpha - macc) / (float)n;

      // ---- mean and step size (arwmh.py:188-189, 193)
      const float delta = act ? zn - mu : 0.0f;
      const float mun = act ? mu + gamma * delta : 0.0f;
      const float lamn = lam + gamma * (alpha - p.target);
      const float e1 = amh_expf(lamn);

      // ---- rank-one update of sqrt(1-gamma) L by (delta, gamma)
      //      (arwmh.py:190-191 -> numpyro cholesky_update), NaN -> keep L.
      const float sq = sqrtf(1.0f - gamma);
      const float ajj = sq * dl;
      const float Dg = ajj * ajj;
      const float one = (amh_isfinite(ajj) && ajj != 0.0f) ? 1.0f : __int_as_float(0x7FC00000);

      // sweep 1: w*_j = w_j when column j is applied (forward solve U w* = delta)
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

      // per-column scalars, one column per lane; b_j by exclusive scan
      const float gw2 = act ? gamma * (ws * ws) : 0.0f;
      const float tsc = act ? gw2 / Dg : 0.0f;
      const float b = 1.0f + Gp::excl_scan(tsc, rr);
      const float g2 = (b * Dg) + gw2;
      const float dn = g2 / b;
      const float c = (gamma * ws) / g2;
      const float q = sqrtf(dn);
      const float dnew = fmaf(c, 0.0f, one) * q;  // new diagonal of column r

      // A NaN anywhere in numpyro's updated factor shows up in its new diagonal
      // (fmaf(c, 0, U_jj) q_j): c_j, q_j and U_jj = A_jj / A_jj are the only
      // per-column quantities, and every off-diagonal entry is finite whenever
      // they are ("keep-L rule").  So the keep-L test of
      // arwmh.py:191 is decided before the factor is touched.
      const bool revert = Gp::any(act && amh_isnan(dnew));
      float sacc = 0.0f;
      float s4[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // as_change partial sums (columns j mod 4)
      if (!revert) {
        // sweep 2: U'_rj = U_rj + c_j w_r^{(j+1)};  as_change terms
        //   L'_rj e1 - L_rj e0 = U'_rj (q_j e1) - U_rj (dl_j e0)
        //   = U_rj (q_j e1 - dl_j e0) + (c_j q_j e1) w_r^{(j+1)}
        const float ac = (q * e1) - (dl * el);
        const float bc = (c * q) * e1;
        w = delta;
        auto col2 = [&](auto J, float wj, float cj, float aj, float bj) {
          const float uo = U[J];
          w = fmaf(-wj, uo, w);
          const float un = fmaf(cj, w, uo);
          const float tt = fmaf(uo, aj, bj * w);
          s4[J & 3] = fmaf(tt, tt, s4[J & 3]);
          U[J] = un;
        };
        if constexpr (kLdsS2) {
          // the group's (ws, c, ac, bc) through the wave's LDS scratch, four
          // columns per wait (asm reads: no vmcnt wait on the DMA prefetch)
          lds_st4(bs_a + 16u * (uint32_t)lane, f32x4{ws, c, ac, bc});
          const uint32_t ga = bs_a + 16u * (uint32_t)(g * G);
          static_for<(DMAX + NB - 1) / NB>([&](auto B) {
            f32x4 qv[NB];
            static_for<NB>([&](auto Q) {
              constexpr int j = NB * B + Q;
              qv[Q] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
              if (j < d) qv[Q] = lds_ld4<16 * j>(ga);
            });
            lds_wait_n<NB>(qv);
            static_for<NB>([&](auto Q) {
              constexpr int j = NB * B + Q;
              if (j < d) col2(std::integral_constant<int, j>{}, qv[Q][0], qv[Q][1], qv[Q][2], qv[Q][3]);
            });
            column_fence<NB * B + NB - 1>();
          });
        } else {
          static_for<DMAX>([&](auto J) {
            if (J < d) {
              col2(J, Gp::template bcast<J>(ws), Gp::template bcast<J>(c), Gp::template bcast<J>(ac),
                   Gp::template bcast<J>(bc));
            }
            column_fence<J>();
          });
        }
        sacc = (s4[0] + s4[1]) + (s4[2] + s4[3]);
        asc = sqrtf(Gp::sum(act ? sacc : 0.0f));
        dl = act ? q : 0.0f;
        updated = true;
      } else {
        // factor unchanged: as_change = || L (e1 - e0) ||_F, L_rj = U_rj dl_j
        const float ac = (dl * e1) - (dl * el);
        static_for<DMAX>([&](auto J) {
          if (J < d) {
            const float tt = U[J] * Gp::template bcast<J>(ac);
            s4[J & 3] = fmaf(tt, tt, s4[J & 3]);
          }
          column_fence<J>();
        });
        sacc = (s4[0] + s4[1]) + (s4[2] + s4[3]);
        asc = sqrtf(Gp::sum(act ? sacc : 0.0f));
      }

      // ---- commit (arwmh.py:199-207)
      it = itr;
      z = zn;
      pe = pen;
      macc = maccn;
      mu = mun;
      lam = lamn;

      if (p.col_z != nullptr || p.col_pe != nullptr) {
        if ((t + 1) % p.thinning == 0 && chain_ok) {
          const int64_t k = t / p.thinning;
          if (p.col_z != nullptr && act) p.col_z[(k * C + chain) * d + r] = z;
          if (p.col_pe != nullptr && r == 0) p.col_pe[k * C + chain] = pe;
        }
      }
    }
    if constexpr (kExt) {
      // split path: the next transition's proposal, exactly as propose_kernel
      // forms it from the state this launch stores -- L = U diag(dl) if a step
      // updated the factor (else the input factor, whose U these registers
      // already are), reloaded as U = L / L_jj -- so the batched potential of
      // the next launch can run without a propose pass over the factor
      if (p.xprop_next != nullptr) {
        const bool any_upd = Gp::any(updated);
        const float inv = (amh_isfinite(dl) && dl != 0.0f) ? 1.0f / dl : 0.0f;
        float xi, u_unused;
        step_noise<G>(r, d, (uint32_t)it, k0, k1, xi, u_unused);
        xi = act ? xi : 0.0f;
        const float el = amh_expf(lam);
        const float eta = dl * xi;
        float a4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        auto colp = [&](auto J, float dj, float ij, float ej) {
          constexpr int j = J;
          const float un = set_one_at<G, j>(keep_above<G, j>((U[j] * dj) * ij, rr), rr);
          a4[j & 3] = fmaf(any_upd ? un : U[j], ej, a4[j & 3]);
        };
        if constexpr (kLdsSP) {
          // (dl, 1 / dl, eta) through the LDS scratch, as sweep 2
          lds_st4(bs_a + 16u * (uint32_t)lane, f32x4{dl, inv, eta, 0.0f});
          const uint32_t ga = bs_a + 16u * (uint32_t)(g * G);
          static_for<(DMAX + NB - 1) / NB>([&](auto B) {
            f32x4 qv[NB];
            static_for<NB>([&](auto Q) {
              constexpr int j = NB * B + Q;
              qv[Q] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
              if (j < d) qv[Q] = lds_ld4<16 * j>(ga);
            });
            lds_wait_n<NB>(qv);
            static_for<NB>([&](auto Q) {
              constexpr int j = NB * B + Q;
              if (j < d) colp(std::integral_constant<int, j>{}, qv[Q][0], qv[Q][1], qv[Q][2]);
            });
            column_fence<NB * B + NB - 1, 16>();
          });
        } else {
          const auto dls = Gp::src(dl), invs = Gp::src(inv), etas = Gp::src(eta);
          static_for<DMAX>([&](auto J) {
            constexpr int j = J;
            if (j < d) {
              // the broadcasts run with every lane of the group active (a
              // broadcast under a lane-dependent branch would read an inactive
              // source lane); then the load path's own masking
              colp(J, Gp::template bcast<j>(dls), Gp::template bcast<j>(invs), Gp::template bcast<j>(etas));
            }
            column_fence<j, 16>();
          });
        }
        const float acc = (a4[0] + a4[1]) + (a4[2] + a4[3]);
        const float zp = act ? z + fmaf(el, acc, p.eps * xi) : 0.0f;
        if (chain_ok && act) p.xprop_next[chain * d + r] = zp;
      }
    }

    prev = item;
    item = nxt;
    nxt = nxt2;
    AMH_STAMP(4)
    AMH_STAMP_COUNT(6)
  }
  if (prev >= 0) {
    int lane = lane_id();
    asm volatile("" : "+v"(lane));
    store_item(p, prev, lane);
  }
  __builtin_amdgcn_s_waitcnt(0);
  AMH_STAMP(5)
  AMH_STAMP_FLUSH(wave)
}

// -------------------------------------------------------------- init kernel --
// arwmh.py:84-138 with numpyro init_to_uniform (U(-2,2) per coordinate).
template <int DMAX, template <int> class M, bool EXACT>
__global__ __launch_bounds__(kBlock) void arwmh_init_kernel(InitParams p) {
  constexpr int G = DMAX;
  using Gp = Grp<G>;
  extern __shared__ float lds[];
  const int d = EXACT ? DMAX : p.d;
  M<G>::stage(lds, p.model, d);
  __syncthreads();
  const auto mctx = M<G>::prepare(p.model, d, lane_id() & (G - 1));
  const int r = Gp::r();
  const bool act = r < d;
  const int64_t C = p.C;
  const int64_t P = (int64_t)d * (d + 1) / 2;
  const int64_t n_items = (C + Geo<G>::CPW - 1) / Geo<G>::CPW;
  const int64_t wave0 = (int64_t)blockIdx.x * (kBlock / 64) + threadIdx.x / 64;
  const int64_t wstride = (int64_t)gridDim.x * (kBlock / 64);
  for (int64_t item = wave0; item < n_items; item += wstride) {
    const int64_t chain = item_chain<G>(item);
    const bool chain_ok = chain < C;
    const int64_t cl = chain_ok ? chain : C - 1;
    const uint64_t gc = (uint64_t)(p.chain_offset + cl);
    const amh_u32x4 kk = amh_philox4x32_10((uint32_t)gc, (uint32_t)(gc >> 32), 0u, AMH_TAG_CHAINKEY,
                                           p.key0, p.key1);
    float z0 = 0.0f;
    if (act) {
      if (p.init_z != nullptr) {
        z0 = p.init_z[cl * d + r];
      } else {
        const amh_u32x4 o = amh_philox4x32_10((uint32_t)r, 0u, 0u, AMH_TAG_INIT, kk.v[0], kk.v[1]);
        const float v = (amh_unif01_from_bits(o.v[0]) * 4.0f) + (-2.0f);
        z0 = (v < -2.0f) ? -2.0f : v;
      }
    }
    const float pe0 = M<G>::potential(z0, r, d, mctx, lds);
    if (chain_ok) {
      float* Lout = p.out.scale + chain * P;
      if (act) {
        p.out.z[chain * d + r] = z0;
        p.out.loc[chain * d + r] = z0;
        // row r of the identity: entries (r, j), j <= r
        for (int j = 0; j <= r; ++j) Lout[col_off(d, j) + (r - j)] = (j == r) ? 1.0f : 0.0f;
      }
      if (r == 0) {
        p.out.i[chain] = 0;
        p.out.potential_energy[chain] = pe0;
        p.out.mean_accept_prob[chain] = 0.0f;
        p.out.log_step_size[chain] = 0.0f;
        p.out.as_change[chain] = 0.0f;
        p.out.rng_key[2 * chain] = kk.v[0];
        p.out.rng_key[2 * chain + 1] = kk.v[1];
      }
    }
  }
}

// --------------------------------------------------------- potential kernel --
template <int DMAX, template <int> class M, bool EXACT>
__global__ __launch_bounds__(kBlock) void potential_kernel(PotParams p) {
  constexpr int G = DMAX;
  using Gp = Grp<G>;
  extern __shared__ float lds[];
  const int d = EXACT ? DMAX : p.d;
  M<G>::stage(lds, p.model, d);
  __syncthreads();
  const auto mctx = M<G>::prepare(p.model, d, lane_id() & (G - 1));
  const int r = Gp::r();
  const bool act = r < d;
  const int64_t C = p.n;
  const int64_t n_items = (C + Geo<G>::CPW - 1) / Geo<G>::CPW;
  const int64_t wave0 = (int64_t)blockIdx.x * (kBlock / 64) + threadIdx.x / 64;
  const int64_t wstride = (int64_t)gridDim.x * (kBlock / 64);
  for (int64_t item = wave0; item < n_items; item += wstride) {
    const int64_t chain = item_chain<G>(item);
    const bool chain_ok = chain < C;
    const int64_t cl = chain_ok ? chain : C - 1;
    const float x = act ? p.z[cl * d + r] : 0.0f;
    const float pe = M<G>::potential(x, r, d, mctx, lds);
    if (chain_ok && r == 0) p.pe[chain] = pe;
  }
}

// -------------------------------------------------------- sample_Pnx kernel --
// arwmh.py:230-270: all chains share one frozen adapt state; chain c = (pt, s)
// starts at x[pt] with key split(rng_key, C)[c] and runs n steps, noise at
// stream position t.  L stays in registers for every chain the wave visits.
template <int DMAX, template <int> class M, bool EXACT>
__global__ __launch_bounds__(kBlock) void sample_pnx_kernel(PnxParams p) {
  constexpr int G = DMAX;
  using Gp = Grp<G>;
  extern __shared__ float lds[];
  const int d = EXACT ? DMAX : p.d;
  M<G>::stage(lds, p.model, d);
  __syncthreads();
  const auto mctx = M<G>::prepare(p.model, d, lane_id() & (G - 1));
  const int r = Gp::r();
  const bool act = r < d;
  const int64_t C = p.n_points * p.n_samples;
  const int64_t n_items = (C + Geo<G>::CPW - 1) / Geo<G>::CPW;
  const int64_t wave0 = (int64_t)blockIdx.x * (kBlock / 64) + threadIdx.x / 64;
  const int64_t wstride = (int64_t)gridDim.x * (kBlock / 64);
  float A[DMAX];
#pragma unroll
  for (int j = 0; j < DMAX; ++j) {
    A[j] = 0.0f;
    if (j < d) {
      if (r >= j && act) A[j] = p.scale[col_off(d, j) + (r - j)];
    }
  }
  const float el = amh_expf(p.log_step_size);
  for (int64_t item = wave0; item < n_items; item += wstride) {
    const int64_t chain = item_chain<G>(item);
    const bool chain_ok = chain < C;
    const int64_t cl = chain_ok ? chain : C - 1;
    const int64_t pt = cl / p.n_samples;
    const amh_u32x4 kk = amh_philox4x32_10((uint32_t)cl, (uint32_t)((uint64_t)cl >> 32), 0u, AMH_TAG_SPLIT,
                                           p.key0, p.key1);
    float z = act ? p.x[pt * d + r] : 0.0f;
    float pe = M<G>::potential(z, r, d, mctx, lds);
    for (int32_t t = 0; t < p.n; ++t) {
      float xi, u;
      step_noise<G>(r, d, (uint32_t)t, kk.v[0], kk.v[1], xi, u);
      xi = act ? xi : 0.0f;
      float acc = 0.0f;
      static_for<DMAX>([&](auto J) {
        if (J < d) acc = fmaf(A[J], Gp::template bcast<J>(xi), acc);
      });
      const float zp = act ? z + fmaf(el, acc, p.eps * xi) : 0.0f;
      float pep = M<G>::potential(zp, r, d, mctx, lds);
      if (amh_isnan(pep)) pep = INFINITY;
      const float ex = amh_expf(pe - pep);
      const float alpha = (ex > 1.0f) ? 1.0f : ex;
      const bool accept = u < alpha;
      z = accept ? zp : z;
      pe = accept ? pep : pe;
    }
    if (chain_ok && act) p.out[cl * d + r] = z;
  }
}

// ------------------------------------------------------------ chain keys ----
__global__ void chain_keys_kernel(uint32_t key0, uint32_t key1, int64_t offset, int64_t n, uint32_t* out) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  const uint64_t g = (uint64_t)(offset + c);
  const amh_u32x4 o = amh_philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), 0u, AMH_TAG_CHAINKEY, key0, key1);
  out[2 * c] = o.v[0];
  out[2 * c + 1] = o.v[1];
}

// ------------------------------------------------------------- launchers ----
static int grid_for(int64_t n_items, int waves_per_block) {
  // enough waves to cover 256 CUs x 8 waves/CU several times; grid-stride past it
  const int64_t blocks = (n_items + waves_per_block - 1) / waves_per_block;
  const int64_t cap = 256 * 32;
  return (int)(blocks < cap ? (blocks > 0 ? blocks : 1) : cap);
}

template <int DMAX, template <int> class M, bool EXACT, int DFIX = 0>
hipError_t launch_step(const StepParams& p, hipStream_t s) {
  constexpr int CPW = Geo<DMAX>::CPW;
  constexpr int WPB = kBlockStep / 64;
  const int d = EXACT ? DMAX : p.d;
  const int64_t n_items = (p.C + CPW - 1) / CPW;
  const size_t shm = step_lds_bytes<DMAX, M>(p.model, d);
  if (shm > 163840) return hipErrorInvalidConfiguration;
  auto kern = arwmh_step_kernel<DMAX, M, EXACT, DFIX>;
  // persistent grid: as many blocks as are co-resident (each wave then walks
  // chain groups wave, wave + total_waves, ...)
  int per_cu = 0;
  hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, kBlockStep, shm);
  if (e != hipSuccess) return e;
  const int cus = cu_count();
  if (per_cu < 1) per_cu = 1;
  const int64_t need = (n_items + WPB - 1) / WPB;
  int64_t blocks = (int64_t)cus * per_cu;
  if (blocks > need) blocks = need;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(kBlockStep), shm, s, p);
  return hipGetLastError();
}

template <int DMAX, template <int> class M, bool EXACT>
hipError_t launch_init(const InitParams& p, hipStream_t s) {
  const int64_t n_items = (p.C + Geo<DMAX>::CPW - 1) / Geo<DMAX>::CPW;
  const size_t shm = M<DMAX>::lds_bytes(p.model, EXACT ? DMAX : p.d);
  hipLaunchKernelGGL((arwmh_init_kernel<DMAX, M, EXACT>), dim3(grid_for(n_items, kBlock / 64)), dim3(kBlock),
                     shm, s, p);
  return hipGetLastError();
}

template <int DMAX, template <int> class M, bool EXACT>
hipError_t launch_pot(const PotParams& p, hipStream_t s) {
  const int64_t n_items = (p.n + Geo<DMAX>::CPW - 1) / Geo<DMAX>::CPW;
  const size_t shm = M<DMAX>::lds_bytes(p.model, EXACT ? DMAX : p.d);
  hipLaunchKernelGGL((potential_kernel<DMAX, M, EXACT>), dim3(grid_for(n_items, kBlock / 64)), dim3(kBlock),
                     shm, s, p);
  return hipGetLastError();
}

// sample_pnx_kernel's step t split around the caller's potential
// (AMH_MODEL_EXTERNAL): ACCEPT = false forms every chain's proposal from the
// shared factor (the same fmaf chain over j as sample_pnx_kernel), ACCEPT =
// true takes U(z') from memory and applies the test with the step's u
template <int G, bool ACCEPT>
__global__ __launch_bounds__(kBlock) void pnx_ext_kernel(PnxExtParams p) {
  using Gp = Grp<G>;
  const int d = p.d;
  const int r = Gp::r();
  const bool act = r < d;
  const int64_t C = p.C;
  const int64_t n_items = (C + Geo<G>::CPW - 1) / Geo<G>::CPW;
  const int64_t wave0 = (int64_t)blockIdx.x * (kBlock / 64) + threadIdx.x / 64;
  const int64_t wstride = (int64_t)gridDim.x * (kBlock / 64);
  float A[G];
  if constexpr (!ACCEPT) {
    static_for<G>([&](auto J) {
      constexpr int j = J;
      A[j] = (j < d && r >= j && act) ? p.scale[col_off(d, j) + (r - j)] : 0.0f;
    });
  }
  const float el = amh_expf(p.log_step_size);
  for (int64_t item = wave0; item < n_items; item += wstride) {
    const int64_t chain = item_chain<G>(item);
    const bool chain_ok = chain < C;
    const int64_t cl = chain_ok ? chain : C - 1;
    const amh_u32x4 kk = amh_philox4x32_10((uint32_t)cl, (uint32_t)((uint64_t)cl >> 32), 0u, AMH_TAG_SPLIT,
                                           p.key0, p.key1);
    const float z = act ? p.z[cl * d + r] : 0.0f;
    if constexpr (!ACCEPT) {
      float xi, u;
      step_noise<G>(r, d, (uint32_t)p.t, kk.v[0], kk.v[1], xi, u);
      xi = act ? xi : 0.0f;
      float acc = 0.0f;
      static_for<G>([&](auto J) {
        if (J < d) acc = fmaf(A[J], Gp::template bcast<J>(xi), acc);
      });
      const float zp = act ? z + fmaf(el, acc, p.eps * xi) : 0.0f;
      if (chain_ok && act) p.zprop[cl * d + r] = zp;
    } else {
      const float u = amh_unif01_from_bits(amh_step_word((uint32_t)d, (uint32_t)p.t, kk.v[0], kk.v[1]));  // W_d
      const float pe = p.pe[cl];
      float pep = p.pe_prop[cl];
      if (amh_isnan(pep)) pep = INFINITY;
      const float ex = amh_expf(pe - pep);
      const float alpha = (ex > 1.0f) ? 1.0f : ex;
      if (u < alpha && chain_ok) {  // group-uniform: one chain per group
        if (act) p.z[cl * d + r] = p.zprop[cl * d + r];
        if (r == 0) p.pe[cl] = pep;
      }
    }
  }
}

hipError_t run_pnx_ext(const PnxExtParams& p, bool accept, hipStream_t s) {
  if (p.d < 1 || p.d > 64 || p.C < 1) return hipErrorInvalidValue;
  auto go = [&](auto kern, int64_t cpw) {
    const int64_t n_items = (p.C + cpw - 1) / cpw;
    hipLaunchKernelGGL(kern, dim3(grid_for(n_items, kBlock / 64)), dim3(kBlock), 0, s, p);
    return hipGetLastError();
  };
  if (p.d <= 32) return accept ? go(pnx_ext_kernel<32, true>, Geo<32>::CPW) : go(pnx_ext_kernel<32, false>, Geo<32>::CPW);
  return accept ? go(pnx_ext_kernel<64, true>, Geo<64>::CPW) : go(pnx_ext_kernel<64, false>, Geo<64>::CPW);
}

template <int DMAX, template <int> class M, bool EXACT>
hipError_t launch_pnx(const PnxParams& p, hipStream_t s) {
  const int64_t n_items = (p.n_points * p.n_samples + Geo<DMAX>::CPW - 1) / Geo<DMAX>::CPW;
  const size_t shm = M<DMAX>::lds_bytes(p.model, EXACT ? DMAX : p.d);
  hipLaunchKernelGGL((sample_pnx_kernel<DMAX, M, EXACT>), dim3(grid_for(n_items, kBlock / 64)), dim3(kBlock),
                     shm, s, p);
  return hipGetLastError();
}

struct StepF {
  const StepParams& p;
  hipStream_t s;
  template <int D, template <int> class M, bool E>
  hipError_t operator()() { return launch_step<D, M, E>(p, s); }
};
struct InitF {
  const InitParams& p;
  hipStream_t s;
  template <int D, template <int> class M, bool E>
  hipError_t operator()() { return launch_init<D, M, E>(p, s); }
};
struct PotF {
  const PotParams& p;
  hipStream_t s;
  template <int D, template <int> class M, bool E>
  hipError_t operator()() { return launch_pot<D, M, E>(p, s); }
};
struct PnxF {
  const PnxParams& p;
  hipStream_t s;
  template <int D, template <int> class M, bool E>
  hipError_t operator()() { return launch_pnx<D, M, E>(p, s); }
};

// A/B switches (the general kernel for d = 64; the data movement alone) exist
// only in the diagnostic build (-DAMH_DIAG, `make stamps`): the release
// library never reads the environment, so no setting can change its work.
static bool step64_enabled() {
#ifdef AMH_DIAG
  static const bool on = [] {
    const char* e = getenv("AMH_STEP64");
    return !(e != nullptr && e[0] == '0');
  }();
  return on;
#else
  return true;
#endif
}

hipError_t run_step(int model_id, const StepParams& p, hipStream_t s) {
  // the headline shape: d = 64 Gaussian, LDS-staged write-back (amh_step64.hip)
  if (model_id == AMH_MODEL_GAUSSIAN && p.d == 64 && p.ext_pe == nullptr && step64_enabled()) {
#ifdef AMH_DIAG
    static const bool move_only = [] {  // diagnostic: the data movement alone (tools/membound.py)
      const char* e = getenv("AMH_S64_MOVE_ONLY");
      return e != nullptr && e[0] == '1';
    }();
    if (move_only) {
      StepParams q = p;
      q.n_steps = 0;
      return run_step64(q, s);
    }
#endif
    return run_step64(p, s);
  }
  // diamonds at the reference shape: compile-time d (immediate offsets)
  if (model_id == AMH_MODEL_DIAMONDS_SS && p.d == kDiamondsD) return launch_step<32, DiamondsSSM, false, kDiamondsD>(p, s);
  return dispatch(model_id, p.d, StepF{p, s});
}

hipError_t run_init(int model_id, const InitParams& p, hipStream_t s) {
  return dispatch(model_id, p.d, InitF{p, s});
}
hipError_t run_potential(int model_id, const PotParams& p, hipStream_t s) {
  return dispatch(model_id, p.d, PotF{p, s});
}
hipError_t run_pnx(int model_id, const PnxParams& p, hipStream_t s) {
  return dispatch(model_id, p.d, PnxF{p, s});
}
// split path (amh_split.hip): the step kernel with U(z') read from p.ext_pe,
// and init without the potential (filled by the batched potential kernel)
hipError_t run_step_ext(const StepParams& p, hipStream_t s) {
  if (p.d < 1 || p.d > 64 || p.n_steps != 1 || p.ext_pe == nullptr) return hipErrorInvalidValue;
  if (p.d == kDiamondsD) return launch_step<32, ExtPotM, false, kDiamondsD>(p, s);
  if (p.d > 32) return launch_step<64, ExtPotM, false>(p, s);  // the external potential's 33..64
  return launch_step<32, ExtPotM, false>(p, s);
}
hipError_t run_init_nopot(const InitParams& p, hipStream_t s) {
  if (p.d < 1 || p.d > 64) return hipErrorInvalidValue;
  if (p.d > 32) return launch_init<64, ExtPotM, false>(p, s);
  return launch_init<32, ExtPotM, false>(p, s);
}

hipError_t run_chain_keys(uint32_t k0, uint32_t k1, int64_t offset, int64_t n, uint32_t* out, hipStream_t s) {
  const int blocks = (int)((n + 255) / 256);
  hipLaunchKernelGGL(chain_keys_kernel, dim3(blocks > 0 ? blocks : 1), dim3(256), 0, s, k0, k1, offset, n, out);
  return hipGetLastError();
}

}  // namespace amh
