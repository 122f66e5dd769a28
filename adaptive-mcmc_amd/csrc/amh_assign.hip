// amh_assign.hip -- the linear-assignment solver behind
// wasserstein_dist11_p(method="auction"): the forward auction in Jacobi form
// with epsilon-scaling, on costs quantised to a power-of-two quantum
// (DESIGN.md §8 holds the bit spec; tests/assign_np.py is its numpy mirror).
// Every quantity after the quantisation is an integer, so the permutation,
// the prices and the round count do not depend on launch geometry or on the
// order in which bids arrive.
//
//   assign_scan_kernel   max of the cost matrix (as float bits: the order of
//                        non-negative floats is the order of their bits) and
//                        the refusal flag (NaN, inf, negative)
//   assign_init_kernel   e and qmax from that maximum, prices to 0
//   assign_phase_kernel  every person unassigned, list 0 = 0 .. n-1
//   assign_bid_kernel    one 256-thread block per unassigned person: streams
//                        the person's cost row once (16-byte loads between a
//                        ragged head and tail), quantises on the fly, keeps a
//                        per-lane (best, its index, second best), reduces
//                        over the wave by DPP and permlane swaps and over the
//                        four waves through LDS, and posts the bid by a 64-bit
//                        atomic max on the object's bid word
//   assign_claim_kernel  of the persons whose bid equals the object's maximum
//                        the lowest index claims it (atomic min)
//   assign_award_kernel  the claimant takes the object at its bid, the
//                        previous owner and every loser go to the next
//                        round's list (appended through one counter: the
//                        list's order is arbitrary, and nothing depends on it)
//
// A round is these last three launches; a launch after the phase has ended
// finds the count at 0 and exits.  The bid and its winner stay apart (an
// atomic max on the value, then the claim) because no bound is proved on the
// prices that would let (bid, person) share one 64-bit word.
//
// Bound: HBM / L2 for the bid kernel (4 bytes of cost and 8 of price per
// element, the prices L2-resident); the rounds at the end of a phase, with a
// handful of bidders, are launch-latency bound.
#include "amh_device.h"

#include <climits>

namespace amh {

namespace {

constexpr int kBidThreads = 256;
constexpr int kListThreads = 256;
constexpr int64_t kNone = INT64_MIN;

// header words of the work buffer (int64 each)
enum { kHdrCmaxBits = 0, kHdrBad = 1, kHdrE = 2, kHdrQmax = 3, kHdrRounds = 4, kHdrCount0 = 5, kHdrCount1 = 6 };

struct AssignWork {
  int64_t* hdr;
  int64_t* price;               // [n]
  unsigned long long* bidmax;   // [n] highest bid of the round, 0: none (a bid is >= 1)
  int64_t* pbid;                // [n] person's bid of the round
  int32_t* owner;               // [n] object -> person, -1 free
  int32_t* obj;                 // [n] person -> object, -1 free
  int32_t* claim;               // [n] lowest person among an object's highest bidders, INT_MAX: none
  int32_t* pj;                  // [n] the object the person bid for
  int32_t* list;                // [2][n] unassigned persons of this round / the next
};

__host__ __device__ inline AssignWork assign_work(void* work, int64_t n) {
  AssignWork w;
  w.hdr = (int64_t*)work;
  w.price = w.hdr + kAssignHdrWords;
  w.bidmax = (unsigned long long*)(w.price + n);
  w.pbid = (int64_t*)(w.bidmax + n);
  w.owner = (int32_t*)(w.pbid + n);
  w.obj = w.owner + n;
  w.claim = w.obj + n;
  w.pj = w.claim + n;
  w.list = w.pj + n;
  return w;
}

__device__ __forceinline__ int64_t quantise(float c, int e) { return (int64_t)rintf(ldexpf(c, -e)); }

// (v1, j1): the best value and the lowest index attaining it; v2: the best of the rest
struct Top2 {
  int64_t v1, v2;
  int32_t j1;
};

__device__ __forceinline__ void top2_push(Top2& t, int64_t v, int32_t j) {
  if (v > t.v1 || (v == t.v1 && j < t.j1)) {
    t.v2 = t.v1;
    t.v1 = v;
    t.j1 = j;
  } else if (v > t.v2) {
    t.v2 = v;
  }
}

__device__ __forceinline__ void top2_merge(Top2& t, int64_t v1, int32_t j1, int64_t v2) {
  if (v1 > t.v1 || (v1 == t.v1 && j1 < t.j1)) {
    t.v2 = t.v1 > v2 ? t.v1 : v2;
    t.v1 = v1;
    t.j1 = j1;
  } else {
    t.v2 = t.v2 > v1 ? t.v2 : v1;
  }
}

// lane exchanges of the wave reduction.  top2_merge is symmetric in its two
// triples, so every step may hand a lane either partner as long as the two
// lanes of a pair see each other: quad swaps and row mirrors by DPP inside a
// row of 16 lanes, then the row pairs and the wave halves by permlane swaps
// (with both operands the same register, the swap's two results are the
// lane's own value and its partner's, in an order that does not matter here).
template <int kCtrl>
__device__ __forceinline__ int32_t dpp32(int32_t x) {
  return __builtin_amdgcn_update_dpp(x, x, kCtrl, 0xF, 0xF, false);
}
template <int kCtrl>
__device__ __forceinline__ int64_t dpp64(int64_t x) {
  const uint32_t lo = (uint32_t)dpp32<kCtrl>((int32_t)(uint32_t)x);
  const uint32_t hi = (uint32_t)dpp32<kCtrl>((int32_t)((uint64_t)x >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
template <int kCtrl>
__device__ __forceinline__ void top2_dpp_step(Top2& t) {
  const int64_t ov1 = dpp64<kCtrl>(t.v1), ov2 = dpp64<kCtrl>(t.v2);
  const int32_t oj1 = dpp32<kCtrl>(t.j1);
  top2_merge(t, ov1, oj1, ov2);
}

struct Swapped32 {
  uint32_t a, b;
};
template <bool kHalves>
__device__ __forceinline__ Swapped32 swap32(uint32_t x) {
  if constexpr (kHalves) {
    const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
    return {r[0], r[1]};
  } else {
    const auto r = __builtin_amdgcn_permlane16_swap(x, x, false, false);
    return {r[0], r[1]};
  }
}
template <bool kHalves>
__device__ __forceinline__ void top2_swap_step(Top2& t) {
  const Swapped32 v1l = swap32<kHalves>((uint32_t)t.v1), v1h = swap32<kHalves>((uint32_t)((uint64_t)t.v1 >> 32));
  const Swapped32 v2l = swap32<kHalves>((uint32_t)t.v2), v2h = swap32<kHalves>((uint32_t)((uint64_t)t.v2 >> 32));
  const Swapped32 j = swap32<kHalves>((uint32_t)t.j1);
  t.v1 = (int64_t)(((uint64_t)v1h.a << 32) | v1l.a);
  t.v2 = (int64_t)(((uint64_t)v2h.a << 32) | v2l.a);
  t.j1 = (int32_t)j.a;
  top2_merge(t, (int64_t)(((uint64_t)v1h.b << 32) | v1l.b), (int32_t)j.b, (int64_t)(((uint64_t)v2h.b << 32) | v2l.b));
}

// every lane ends with the wave's triple
__device__ __forceinline__ void top2_wave_reduce(Top2& t) {
  top2_dpp_step<0xB1>(t);    // quad_perm [1, 0, 3, 2]
  top2_dpp_step<0x4E>(t);    // quad_perm [2, 3, 0, 1]
  top2_dpp_step<0x141>(t);   // row_half_mirror
  top2_dpp_step<0x140>(t);   // row_mirror
  top2_swap_step<false>(t);  // rows 0 <-> 1, 2 <-> 3
  top2_swap_step<true>(t);   // lanes 0 .. 31 <-> 32 .. 63
}

}  // namespace

__global__ __launch_bounds__(256) void assign_scan_kernel(const float* __restrict__ cost, int64_t total,
                                                          int64_t* __restrict__ hdr) {
  uint32_t mx = 0u;
  int bad = 0;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < total; k += stride) {
    const float c = cost[k];
    if (!(c >= 0.0f) || c == INFINITY) {
      bad = 1;
    } else {
      const uint32_t b = __float_as_uint(fabsf(c));  // fabsf: -0.0f counts as 0
      mx = b > mx ? b : mx;
    }
  }
  for (int off = 32; off >= 1; off >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)mx, off, 64);
    mx = o > mx ? o : mx;
    bad |= __shfl_xor(bad, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (mx) atomicMax((unsigned long long*)&hdr[kHdrCmaxBits], (unsigned long long)mx);
    if (bad) atomicMax((unsigned long long*)&hdr[kHdrBad], 1ull);
  }
}

__global__ __launch_bounds__(256) void assign_init_kernel(void* work, int64_t n) {
  const AssignWork w = assign_work(work, n);
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k < n) w.price[k] = 0;
  if (k == 0) {
    const float cmax = __uint_as_float((uint32_t)w.hdr[kHdrCmaxBits]);
    int e = 0;
    if (cmax > 0.0f) {
      // cmax = m 2^x, 1/2 <= m < 1: the smallest e with cmax 2^-e <= 2^30
      int x;
      const float m = frexpf(cmax, &x);
      e = (m == 0.5f) ? x - 31 : x - 30;
    }
    w.hdr[kHdrE] = e;
    w.hdr[kHdrQmax] = quantise(cmax, e);
    w.hdr[kHdrRounds] = 0;
  }
}

__global__ __launch_bounds__(256) void assign_phase_kernel(void* work, int64_t n) {
  const AssignWork w = assign_work(work, n);
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k < n) {
    w.owner[k] = -1;
    w.obj[k] = -1;
    w.claim[k] = INT_MAX;
    w.bidmax[k] = 0ull;
    w.list[k] = (int32_t)k;
  }
  if (k == 0) {
    w.hdr[kHdrCount0] = n;
    w.hdr[kHdrCount1] = 0;
  }
}

__global__ __launch_bounds__(kBidThreads) void assign_bid_kernel(const float* __restrict__ cost, void* work,
                                                                 int64_t n, int64_t eps, int cur) {
  const AssignWork w = assign_work(work, n);
  if ((int64_t)blockIdx.x >= w.hdr[kHdrCount0 + cur]) return;
  const int32_t i = w.list[(int64_t)cur * n + blockIdx.x];
  const int e = (int)w.hdr[kHdrE];
  const float* row = cost + (int64_t)i * n;
  const int64_t* __restrict__ price = w.price;

  // [0, head) up to the first 16-byte boundary, [head, head + 4 nv) in float4s, then the tail
  int64_t head = (int64_t)((16u - (uint32_t)((uintptr_t)row & 15u)) & 15u) >> 2;
  if (head > n) head = n;
  const int64_t nv = (n - head) >> 2;
  const int64_t tail0 = head + 4 * nv;

  Top2 t{kNone, kNone, INT_MAX};
  const int tid = threadIdx.x;
  if (tid < head) top2_push(t, -quantise(row[tid], e) - price[tid], tid);
  const f32x4* body = (const f32x4*)(row + head);
  for (int64_t k = tid; k < nv; k += kBidThreads) {
    const f32x4 c = body[k];
    const int64_t j = head + 4 * k;
    top2_push(t, -quantise(c[0], e) - price[j], (int32_t)j);
    top2_push(t, -quantise(c[1], e) - price[j + 1], (int32_t)(j + 1));
    top2_push(t, -quantise(c[2], e) - price[j + 2], (int32_t)(j + 2));
    top2_push(t, -quantise(c[3], e) - price[j + 3], (int32_t)(j + 3));
  }
  if (tail0 + tid < n) top2_push(t, -quantise(row[tail0 + tid], e) - price[tail0 + tid], (int32_t)(tail0 + tid));

  top2_wave_reduce(t);
  __shared__ int64_t sv1[kBidThreads / 64], sv2[kBidThreads / 64];
  __shared__ int32_t sj1[kBidThreads / 64];
  if ((tid & 63) == 0) {
    sv1[tid >> 6] = t.v1;
    sv2[tid >> 6] = t.v2;
    sj1[tid >> 6] = t.j1;
  }
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < kBidThreads / 64; ++k) top2_merge(t, sv1[k], sj1[k], sv2[k]);
    const int64_t gap = (n > 1) ? t.v1 - t.v2 : 0;
    const int64_t bid = price[t.j1] + gap + eps;
    w.pbid[i] = bid;
    w.pj[i] = t.j1;
    atomicMax(&w.bidmax[t.j1], (unsigned long long)bid);
  }
}

__global__ __launch_bounds__(kListThreads) void assign_claim_kernel(void* work, int64_t n, int cur) {
  const AssignWork w = assign_work(work, n);
  const int64_t k = (int64_t)blockIdx.x * kListThreads + threadIdx.x;
  if (k == 0) w.hdr[kHdrCount0 + (cur ^ 1)] = 0;  // the list the award kernel appends to
  if (k >= w.hdr[kHdrCount0 + cur]) return;
  const int32_t i = w.list[(int64_t)cur * n + k];
  const int32_t j = w.pj[i];
  if ((unsigned long long)w.pbid[i] == w.bidmax[j]) atomicMin(&w.claim[j], i);
}

__global__ __launch_bounds__(kListThreads) void assign_award_kernel(void* work, int64_t n, int cur) {
  const AssignWork w = assign_work(work, n);
  const int64_t k = (int64_t)blockIdx.x * kListThreads + threadIdx.x;
  const int64_t count = w.hdr[kHdrCount0 + cur];
  if (k == 0 && count > 0) w.hdr[kHdrRounds] += 1;
  if (k >= count) return;
  const int32_t i = w.list[(int64_t)cur * n + k];
  const int32_t j = w.pj[i];
  int32_t next = i;  // a loser bids again
  if (w.claim[j] == i) {
    next = w.owner[j];  // the evicted owner, if any
    w.owner[j] = i;
    w.obj[i] = j;
    w.price[j] = w.pbid[i];
    w.bidmax[j] = 0ull;
    w.claim[j] = INT_MAX;
    if (next >= 0) w.obj[next] = -1;
  }
  if (next >= 0) {
    const unsigned long long at = atomicAdd((unsigned long long*)&w.hdr[kHdrCount0 + (cur ^ 1)], 1ull);
    w.list[(int64_t)(cur ^ 1) * n + (int64_t)at] = next;
  }
}

__global__ __launch_bounds__(256) void assign_result_kernel(const void* work, int64_t n, int64_t* __restrict__ perm,
                                                            int64_t* __restrict__ price) {
  const AssignWork w = assign_work(const_cast<void*>(work), n);
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  if (perm) perm[k] = w.obj[k];
  if (price) price[k] = w.price[k];
}

int64_t assign_work_bytes(int64_t n) { return (int64_t)sizeof(int64_t) * (kAssignHdrWords + 3 * n) + 4 * 6 * n; }

hipError_t run_assign_begin(const float* cost, int64_t n, void* work, hipStream_t s) {
  hipError_t err = hipMemsetAsync(work, 0, sizeof(int64_t) * kAssignHdrWords, s);
  if (err != hipSuccess) return err;
  const int64_t total = n * n;
  const int64_t want = (total + 256 * 16 - 1) / (256 * 16);  // about 16 elements per thread
  const unsigned blocks = (unsigned)(want < 1 ? 1 : (want > 4096 ? 4096 : want));
  hipLaunchKernelGGL(assign_scan_kernel, dim3(blocks), dim3(256), 0, s, cost, total, (int64_t*)work);
  err = hipGetLastError();
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(assign_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, work, n);
  return hipGetLastError();
}

hipError_t run_assign_phase(void* work, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(assign_phase_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, work, n);
  return hipGetLastError();
}

hipError_t run_assign_rounds(const float* cost, int64_t n, void* work, int64_t eps, int64_t bound, int64_t first,
                             int32_t rounds, hipStream_t s) {
  const unsigned lblocks = (unsigned)((bound + kListThreads - 1) / kListThreads);
  for (int32_t r = 0; r < rounds; ++r) {
    const int cur = (int)((first + r) & 1);
    hipLaunchKernelGGL(assign_bid_kernel, dim3((unsigned)bound), dim3(kBidThreads), 0, s, cost, work, n, eps, cur);
    hipLaunchKernelGGL(assign_claim_kernel, dim3(lblocks), dim3(kListThreads), 0, s, work, n, cur);
    hipLaunchKernelGGL(assign_award_kernel, dim3(lblocks), dim3(kListThreads), 0, s, work, n, cur);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
  }
  return hipSuccess;
}

hipError_t run_assign_header(const void* work, int64_t* host8, hipStream_t s) {
  hipError_t err = hipMemcpyAsync(host8, work, sizeof(int64_t) * kAssignHdrWords, hipMemcpyDeviceToHost, s);
  if (err != hipSuccess) return err;
  return hipStreamSynchronize(s);
}

hipError_t run_assign_result(const void* work, int64_t n, int64_t* perm, int64_t* price, hipStream_t s) {
  hipLaunchKernelGGL(assign_result_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, work, n, perm, price);
  return hipGetLastError();
}

}  // namespace amh
