// amh_step_stage.h -- shared by arwmh_step_kernel (amh_kernels.hip) and
// arwmh_step64_kernel (amh_step64.hip): a work item's LDS staging buffer and its DMA.
#pragma once
#include "amh_device.h"

namespace amh {

typedef __attribute__((address_space(3))) void lds_void;
__device__ __forceinline__ lds_void* to_lds(const float* p) { return (lds_void*)(p); }

// Per-wave LDS staging buffer of the step kernel, in floats:
//   [ L: CPW*P (rounded to 4) | z: CPW*d | loc: CPW*d | scalars: 8 x CPW ]
__host__ __device__ __forceinline__ int wbuf_L(int cpw, int d) { return ((cpw * d * (d + 1) / 2) + 3) & ~3; }
__host__ __device__ __forceinline__ int wbuf_zd(int cpw, int d) { return ((cpw * d) + 3) & ~3; }
__host__ __device__ __forceinline__ int wbuf_floats(int cpw, int d) {
  return wbuf_L(cpw, d) + 2 * wbuf_zd(cpw, d) + 8 * cpw;
}

// Issue the DMA of one work item's chain state (global -> this wave's LDS
// buffer).  Out-of-range bytes (past C) read as zero.
template <int G, bool EXT>
__device__ __forceinline__ void prefetch_item_small(const StepParams& p, int64_t first, int d, float* wb, int lane);
template <int G, bool EXT, int AUX = kLoadAux>  // AUX: cache policy of the factor's DMA loads
__device__ __forceinline__ void prefetch_item(const StepParams& p, int64_t first, int d, float* wb, int lane) {
  constexpr int CPW = Geo<G>::CPW;
  const uint32_t P = (uint32_t)(d * (d + 1) / 2);
  const int64_t nvalid = (p.C - first) < CPW ? (p.C - first) : CPW;  // chains of this item in range
  float* wL = wb;
  {
    const uint32_t bytes = (uint32_t)nvalid * P * 4u;
    const Buf b(uniform_ptr(p.in.scale + first * P), bytes);
    const bool vec = ((P * 4u) % 16u) == 0u;  // 16-B aligned chain blocks
    const uint32_t total = (uint32_t)CPW * P * 4u;
    // whole 1 KB pieces as dwordx4, the tail as dwords; exec masks keep every
    // DMA inside this wave's buffer (an LDS-DMA writes base + 4*size*lane)
    const uint32_t n16 = vec ? (total / 1024u) * 1024u : 0u;
    for (uint32_t o = 0; o < n16; o += 1024u)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(b.rs, to_lds(wL + o / 4u), 16, (int)(o + 16u * lane), 0, 0, AUX);
    for (uint32_t o = n16; o < total; o += 256u) {
      if (o + 4u * lane < total)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(b.rs, to_lds(wL + o / 4u), 4, (int)(o + 4u * lane), 0, 0, AUX);
    }
  }
  prefetch_item_small<G, EXT>(p, first, d, wb, lane);
}
// ... everything but the factor: z, loc, the scalars and the key words
template <int G, bool EXT>
__device__ __forceinline__ void prefetch_item_small(const StepParams& p, int64_t first, int d, float* wb, int lane) {
  constexpr int CPW = Geo<G>::CPW;
  const int64_t nvalid = (p.C - first) < CPW ? (p.C - first) : CPW;
  float* wz = wb + wbuf_L(CPW, d);
  float* wm = wz + wbuf_zd(CPW, d);
  float* ws = wm + wbuf_zd(CPW, d);
  {
    const uint32_t bytes = (uint32_t)(nvalid * d) * 4u;
    const uint32_t total = (uint32_t)(CPW * d) * 4u;
    const Buf bz(uniform_ptr(p.in.z + first * d), bytes);
    const Buf bm(uniform_ptr(p.in.loc + first * d), bytes);
    for (uint32_t o = 0; o < total; o += 256u) {
      if (o + 4u * lane < total) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(bz.rs, to_lds(wz + o / 4u), 4, (int)(o + 4u * lane), 0, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(bm.rs, to_lds(wm + o / 4u), 4, (int)(o + 4u * lane), 0, 0, 0);
      }
    }
  }
  if (lane < CPW) {
    const uint32_t bytes = (uint32_t)nvalid * 4u;
    const uint32_t vo = 4u * lane;
    const Buf b0(uniform_ptr(p.in.i + first), bytes);
    const Buf b1(uniform_ptr(p.in.potential_energy + first), bytes);
    // (ASSS states have no mean_accept_prob / log_step_size: an empty range, so
    // those DMAs read zeros and touch no memory)
    const Buf b2(p.in.mean_accept_prob ? uniform_ptr(p.in.mean_accept_prob + first) : p.in.i,
                 p.in.mean_accept_prob ? bytes : 0u);
    const Buf b3(p.in.log_step_size ? uniform_ptr(p.in.log_step_size + first) : p.in.i,
                 p.in.log_step_size ? bytes : 0u);
    const Buf b4(uniform_ptr(p.in.as_change + first), bytes);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(b0.rs, to_lds(ws + 0 * CPW), 4, (int)vo, 0, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(b1.rs, to_lds(ws + 1 * CPW), 4, (int)vo, 0, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(b2.rs, to_lds(ws + 2 * CPW), 4, (int)vo, 0, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(b3.rs, to_lds(ws + 3 * CPW), 4, (int)vo, 0, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(b4.rs, to_lds(ws + 4 * CPW), 4, (int)vo, 0, 0, 0);
  }
  {
    // 2 CPW key words: two DMAs of 64 lanes when a wave holds 64 chains (G = 1)
    const Buf bk(uniform_ptr(p.in.rng_key + 2 * first), (uint32_t)nvalid * 8u);
    static_for<(2 * CPW + 63) / 64>([&](auto H) {
      constexpr int o = 64 * H;
      if (lane + o < 2 * CPW)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(bk.rs, to_lds(ws + 5 * CPW + o), 4, (int)(4u * (lane + o)), 0, 0, 0);
    });
  }
  if (EXT && lane < CPW) {  // split path: U(z') of the batched potential kernel
    const Buf be(uniform_ptr(p.ext_pe + first), (uint32_t)nvalid * 4u);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(be.rs, to_lds(ws + 7 * CPW), 4, (int)(4u * lane), 0, 0, 0);
  }
}

}  // namespace amh
