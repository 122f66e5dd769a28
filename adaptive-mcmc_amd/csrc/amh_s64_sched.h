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

// ---- stealable block tails (the single-step ARWMH launch) ----
// The draw order above is split in two.  The first n - T draws, the own part,
// come from the block's LDS counter.  The last T, the stealable tail, come from
// the block's head word in global memory, which any block may draw from: a
// block that has run out of work takes tail chains of blocks that are behind.
// T = s64_tail_len(n, steal); steal = 0 is the schedule without a tail.  A head
// word holds tag << 16 | count: the launch's 16-bit tag and the tail draws
// handed out so far.  A draw is a returning add of 1; it is valid only if the
// old value carries the launch's tag and a count below T (s64_head_valid).
constexpr uint32_t kS64StealDefault = 16;    // the launch's default stealable-tail length
constexpr uint32_t kS64StealTries = 4;       // victims a wave visits before it gives up
constexpr uint32_t kS64StealStride = 8;      // victims b + 8, b + 16, ...: the same b % 8 (speed only)
constexpr uint32_t kS64StealMax = 1u << 15;  // the count stays inside 16 bits whatever fails after the last draw
constexpr uint32_t kS64HeadSlots = 1024;     // head words the handle owns: one per possible block
constexpr uint32_t kS64HeadStride = 32;      // in words: every head on its own 128-B line, [head, stolen, pad]
// at the headline shape (256 chains per block) the default tail lies inside the tail class
static_assert(kS64StealDefault <= 256 * kS64HotNum / kS64HotDen && kS64StealDefault <= kS64StealMax,
              "default stealable tail: every chain of it has class kS64Tail");

__host__ __device__ constexpr uint32_t s64_tail_len(uint32_t n, uint32_t steal) {
  const uint32_t t = steal < kS64StealMax ? steal : kS64StealMax;
  return t < n ? t : n;
}

// local index of tail draw c (c < T): draw position n - T + c of the block's order
__host__ __device__ inline uint32_t s64_tail_index(const S64Sched& s, uint32_t n, uint32_t T, uint32_t c) {
  return s64_draw(s, n - T + c);
}

// The own part as a range of local indices [lo, lo + n - T): what the LDS
// counter hands out is an own draw iff it lies inside.
__host__ __device__ inline uint32_t s64_own_lo(uint32_t T, int descending) { return descending ? T : 0u; }

// the k-th victim of block b in a grid of `grid` blocks, k = 1 ... kS64StealTries;
// `grid` ("none") once the sequence would come back to b
__host__ __device__ inline uint32_t s64_victim(uint32_t b, uint32_t grid, uint32_t k) {
  const uint32_t v = (uint32_t)(((uint64_t)b + (uint64_t)kS64StealStride * k) % grid);
  return v == b ? grid : v;
}

__host__ __device__ inline bool s64_head_valid(uint32_t old, uint32_t tag, uint32_t T) {
  return (old >> 16) == tag && (old & 0xFFFFu) < T;
}

}  // namespace amh
