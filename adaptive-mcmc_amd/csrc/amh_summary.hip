// amh_summary.hip -- streaming posterior summaries (infer_amd/streaming.py):
// one pass over a block of draws x[B][C][k] feeds the per-(chain, column)
// float64 moments and the per-column pooled histogram (DESIGN.md §7.1 holds
// the bit spec; tests/summary_np.py is its numpy mirror).
//
//   summary_update_kernel   1024 threads = cpp chains x TK columns, TK a power
//                           of two <= 32 (16 at 2048 bins).  A thread owns one
//                           (c, j): it loads the five accumulators, walks the
//                           B draws of its element in draw order with the
//                           loads of four draws in flight, and stores the five
//                           back, so the accumulator traffic is paid once per
//                           block of draws.  A wave's load is 64 / TK segments
//                           of 4 TK contiguous bytes (two 128-byte segments at
//                           TK = 32).  Bin counts go to an LDS table of 32-bit
//                           counters [TK][nbins + 3] (ds_add_u32, no return);
//                           a block walks `passes` chain groups against one
//                           table and flushes its non-zero counters with
//                           64-bit global atomic adds.
//
// The moments of an element are summed by one thread in draw order and the
// counts are integers, so the result depends neither on the grid nor on how
// the draws are split into blocks.
//
// Bound: HBM (4 bytes read per element; 80 bytes of accumulators per (c, j)
// and launch).  The lanes of a wave sit on different columns, so at most
// 64 / TK of them meet on one LDS word: draws that all fall into one bin per
// column measured no slower than spread ones at k = 64.
#include "amh_device.h"

namespace amh {

namespace {

constexpr int kSummaryThreads = 1024;
constexpr int kSummaryLdsBytes = 160 * 1024;

struct SummaryBin {
  float lo, inv_w, top;  // top = (float)nbins
  int nbins;
};

__device__ __forceinline__ int summary_bin(float x, const SummaryBin& s) {
  const float t = (x - s.lo) * s.inv_w;
  if (t != t) return s.nbins + 2;
  if (t < 0.0f) return 0;
  if (t >= s.top) return s.nbins + 1;
  return 1 + (int)t;
}

struct SummaryAcc {
  double s1, s2, bs, s1b, q;
};

__device__ __forceinline__ void summary_push(SummaryAcc& a, float x, double center, int64_t& phase, int64_t batch) {
  const double y = (double)x - center;
  a.s1 += y;
  const double yy = y * y;
  a.s2 += yy;
  a.bs += y;
  if (++phase == batch) {
    a.s1b += a.bs;
    const double bb = a.bs * a.bs;
    a.q += bb;
    a.bs = 0.0;
    phase = 0;
  }
}

}  // namespace

// grid (column tiles, chain groups); a chain group is passes * cpp chains,
// cpp = 1024 >> tk_log2
__global__ __launch_bounds__(kSummaryThreads) void summary_update_kernel(
    const float* __restrict__ x, int64_t B, int64_t C, int k, const float* __restrict__ calib, int nbins,
    int64_t batch, int64_t phase0, double* __restrict__ acc, unsigned long long* __restrict__ hist, int tk_log2,
    int passes) {
  extern __shared__ uint32_t summary_tab[];  // [TK][nbins + 3]
  const int tid = threadIdx.x;
  const int tk = 1 << tk_log2;
  const int nb3 = nbins + 3;
  const int cells = tk * nb3;
  for (int i = tid; i < cells; i += kSummaryThreads) summary_tab[i] = 0u;
  __syncthreads();

  const int col = tid & (tk - 1);
  const int j0 = (int)blockIdx.x * tk;
  const int j = j0 + col;
  const int64_t cpp = kSummaryThreads >> tk_log2;
  const int64_t cbase = (int64_t)blockIdx.y * passes * cpp + (tid >> tk_log2);
  const int64_t plane = C * (int64_t)k;  // one draw of every chain; one accumulator

  if (j < k) {
    const double center = (double)calib[j];
    const SummaryBin sb{calib[k + j], calib[2 * k + j], (float)nbins, nbins};
    uint32_t* tab = summary_tab + col * nb3;
    for (int p = 0; p < passes; ++p) {
      const int64_t c = cbase + p * cpp;
      if (c >= C) break;
      const int64_t e = c * k + j;
      SummaryAcc a{acc[e], acc[plane + e], acc[2 * plane + e], acc[3 * plane + e], acc[4 * plane + e]};
      int64_t phase = phase0;
      const float* px = x + e;
      int64_t t = 0;
      for (; t + 4 <= B; t += 4) {
        const float x0 = px[0], x1 = px[plane], x2 = px[2 * plane], x3 = px[3 * plane];
        px += 4 * plane;
        atomicAdd(&tab[summary_bin(x0, sb)], 1u);
        atomicAdd(&tab[summary_bin(x1, sb)], 1u);
        atomicAdd(&tab[summary_bin(x2, sb)], 1u);
        atomicAdd(&tab[summary_bin(x3, sb)], 1u);
        summary_push(a, x0, center, phase, batch);
        summary_push(a, x1, center, phase, batch);
        summary_push(a, x2, center, phase, batch);
        summary_push(a, x3, center, phase, batch);
      }
      for (; t < B; ++t) {
        const float x0 = px[0];
        px += plane;
        atomicAdd(&tab[summary_bin(x0, sb)], 1u);
        summary_push(a, x0, center, phase, batch);
      }
      acc[e] = a.s1;
      acc[plane + e] = a.s2;
      acc[2 * plane + e] = a.bs;
      acc[3 * plane + e] = a.s1b;
      acc[4 * plane + e] = a.q;
    }
  }
  __syncthreads();

  // columns past k hold zeros only (their threads never counted)
  for (int i = tid; i < cells; i += kSummaryThreads) {
    const uint32_t v = summary_tab[i];
    if (v) {
      const int cl = i / nb3;
      atomicAdd(&hist[(int64_t)(j0 + cl) * nb3 + (i - cl * nb3)], (unsigned long long)v);
    }
  }
}

hipError_t run_summary_update(const float* x, int64_t B, int64_t C, int k, const float* calib, int nbins,
                              int64_t batch, int64_t n_before, double* acc, int64_t* hist, hipStream_t s) {
  // the column tile: the smallest power of two >= k, at most what the table leaves room for
  const int tk_max = (4 * 32 * (nbins + 3) <= kSummaryLdsBytes) ? 32 : 16;
  int tk_log2 = 0;
  while ((1 << tk_log2) < k && (1 << tk_log2) < tk_max) ++tk_log2;
  const int tk = 1 << tk_log2;
  const int64_t cpp = kSummaryThreads >> tk_log2;
  const int64_t tiles = (k + tk - 1) / tk;
  const int64_t groups_all = (C + cpp - 1) / cpp;
  // about 1024 blocks (four per CU) when there are that many chain groups: the
  // flush of a table is then shared by `passes` groups.  A block's 32-bit
  // counters see at most passes * cpp * B draws of a column.
  int64_t want = (1024 + tiles - 1) / tiles;
  int64_t passes = (groups_all + want - 1) / want;
  const int64_t room = (int64_t)0xFFFFFFFFll / B / cpp;
  if (room < 1) return hipErrorInvalidValue;
  if (passes > room) passes = room;
  if (passes > groups_all) passes = groups_all;
  const int64_t groups = (groups_all + passes - 1) / passes;
  if (groups > 65535) return hipErrorInvalidValue;
  const size_t lds = sizeof(uint32_t) * (size_t)tk * (size_t)(nbins + 3);
  if (lds > 64 * 1024) {  // per device, so asked for at every such launch
    const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(summary_update_kernel),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, kSummaryLdsBytes);
    if (attr != hipSuccess) return attr;
  }
  hipLaunchKernelGGL(summary_update_kernel, dim3((unsigned)tiles, (unsigned)groups), dim3(kSummaryThreads), lds, s, x,
                     B, C, k, calib, nbins, batch, n_before % batch, acc, (unsigned long long*)hist, tk_log2,
                     (int)passes);
  return hipGetLastError();
}

}  // namespace amh
