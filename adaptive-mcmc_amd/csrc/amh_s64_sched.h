// amh_s64_sched.h -- the block-local schedule of arwmh_step64_kernel, stated
// once for the kernel (amh_step64.hip) and for the host (amh_capi.hip
// amh_step64_schedule, tests/test_step64_schedule.py).
//
// A block owns n chains, local indices 0 ... n - 1, and its waves draw them
// from one counter in the block's LDS.  An ascending launch draws 0, 1, 2, ...,
// a descending one n - 1, n - 2, ..., 0, and consecutive launches on the same
// state alternate (amh_capi.hip step64_order), so what one launch wrote last
// the next one reads first, while the memory-side cache still holds it
// (DESIGN.md 3.1).  That splits a launch's draws by position:
//   hot   the first h = floor(n * kS64HotNum / kS64HotDen) draws of a launch
//         that is chained to the previous one: what that launch drew last;
//   tail  the last h draws of any launch: what a chained next launch draws
//         first;
//   mid   the rest.
// h <= n / 2, so no chain is both hot and tail; h = 0 for n < 3, and then every
// chain is mid.  The class picks the cache policy of
// the chain's factor traffic (kS64LoadAux* / kS64StoreAux*, amh_step64.hip);
// it changes no result.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace amh {

constexpr uint32_t kS64HotNum = 3, kS64HotDen = 8;  // the hot (and the tail) fraction of a block's range
static_assert(2 * kS64HotNum <= kS64HotDen, "hot and tail parts must not overlap");
constexpr uint32_t kS64Hot = 1u, kS64Tail = 2u;     // class bits

struct S64Sched {
  uint32_t first, step;      // the counter's first value and its increment (1 or 2^32 - 1)
  uint32_t hot_lo, hot_n;    // local indices [hot_lo, hot_lo + hot_n) are hot
  uint32_t tail_lo, tail_n;  // ... [tail_lo, tail_lo + tail_n) are the tail
};

__host__ __device__ constexpr uint32_t s64_hot_count(uint32_t n) {
  return (uint32_t)((uint64_t)n * kS64HotNum / kS64HotDen);
}

// chained: the launch reads what the previous launch wrote (opposite order), so it has a hot part
__host__ __device__ inline S64Sched s64_sched(uint32_t n, int descending, int chained) {
  const uint32_t h = s64_hot_count(n);
  S64Sched s;
  s.first = descending ? n - 1u : 0u;
  s.step = descending ? ~0u : 1u;
  s.hot_lo = descending ? n - h : 0u;
  s.hot_n = chained ? h : 0u;
  s.tail_lo = descending ? 0u : n - h;
  s.tail_n = h;
  return s;
}

// The k-th value of the counter.  Past the last chain it reads n, n + 1, ... or
// wraps to 2^32 - 1, 2^32 - 2, ...: either way a value >= n, "no chain".
__host__ __device__ inline uint32_t s64_draw(const S64Sched& s, uint32_t k) { return s.first + k * s.step; }

// Class bits of the local index v the counter handed out; 0 for every v >= n
// (unsigned differences: a v below a range's start wraps to a large number).
__host__ __device__ inline uint32_t s64_class(uint32_t v, uint32_t hot_lo, uint32_t hot_n, uint32_t tail_lo,
                                              uint32_t tail_n) {
  return (v - hot_lo < hot_n ? kS64Hot : 0u) | (v - tail_lo < tail_n ? kS64Tail : 0u);
}

}  // namespace amh
