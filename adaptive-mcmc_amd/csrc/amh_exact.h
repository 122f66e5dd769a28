// amh_exact.h -- the fixed-point format of the pooled mode's exact sums
// (PooledARWMH(exact_sums=True); include/amh.h "exact sums"), stated once for
// the kernels (amh_pooled_exact.hip) and for the host entries (amh_capi.hip
// amh_pooled_exact_quantise / amh_pooled_exact_to_double,
// tests/test_pooled_exact.py).
//
// A component of the sums vector is kExactWords int64 words:
//   words 0 .. kExactLimbs - 1   limbs, value = sum_j limb_j 2^(kExactBits j - kExactFrac)
//   word  kExactLimbs            the number of partials that had no fixed-point
//                                image (+-inf, NaN, |p| >= 2^kExactRange)
// exact_add maps ONE float32 partial to limbs that carry its sign (the integer
// trunc(p 2^kExactFrac) cut into kExactBits-bit pieces, no carry, no
// normalisation) and adds them word by word.  Word-wise int64 addition is all
// that ever happens to the words afterwards -- within a rank, over the steps
// of a block, across ranks -- so the totals depend on the multiset of
// partials and on nothing else.  A float32 whose lowest set bit is at least
// 2^-kExactFrac is represented exactly; lower bits are cut toward zero, per
// partial.  A limb holds |piece| < 2^kExactBits, so 2^(63 - kExactBits)
// summands (kExactMaxSummands) cannot overflow a word.
//
// exact_to_double rounds the exact rational value of the limb totals to the
// nearest double (ties to even) through a wide integer; a non-zero count word
// makes it NaN, whatever the limbs hold.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/amh.h"

namespace amh {

constexpr int kExactBits = AMH_EXACT_BITS;    // B: payload bits of a limb
constexpr int kExactLimbs = AMH_EXACT_LIMBS;  // L
constexpr int kExactFrac = AMH_EXACT_FRAC;    // F: the grid is 2^-F
constexpr int kExactRange = kExactBits * kExactLimbs - kExactFrac;  // |p| < 2^80
constexpr int kExactWords = kExactLimbs + 1;                        // limbs + the count of partials out of range
constexpr int64_t kExactMaxSummands = (int64_t)1 << (63 - kExactBits);
static_assert(kExactWords == AMH_EXACT_WORDS && kExactMaxSummands == AMH_EXACT_MAX_SUMMANDS, "include/amh.h");
static_assert(kExactBits == 40 && kExactLimbs == 4, "exact_add / exact_to_double are written for four 40-bit limbs");
static_assert(kExactBits + 24 <= 64, "a shifted float32 significand must fit one 64-bit word");

__host__ __device__ inline uint32_t exact_f32_bits(float p) { return __builtin_bit_cast(uint32_t, p); }

// w[0 .. kExactWords) += the image of p.  Every word is updated once, at the
// one exit, and none is indexed by a run-time value, so the words stay in
// registers (early exits that update different words get merged into a store
// through a selected address, i.e. into stack traffic).
__host__ __device__ inline void exact_add(int64_t (&w)[kExactWords], float p) {
  const uint32_t b = exact_f32_bits(p);
  const int ex = (int)((b >> 23) & 0xFFu);
  const int e = ex - 150;  // ex > 0: |p| = m 2^e, 2^23 <= m < 2^24
  // inf, NaN, |p| >= 2^kExactRange
  const bool bad = ex == 255 || e + 24 > kExactRange;
  const int s = e + kExactFrac;  // trunc(|p| 2^F) = m 2^s; s <= 136 unless bad
  // zero and the denormals (< 2^-126, far below the grid), and what the cut leaves nothing of
  const bool none = ex == 0 || s <= -24;
  uint64_t m = (bad || none) ? 0 : (uint64_t)((b & 0x7FFFFFu) | 0x800000u);
  const int down = (s < 0 && s > -24) ? -s : 0;  // the bits below the grid, cut toward zero
  m >>= down;
  const int up = (s > 0 && !bad) ? s : 0;
  const int j = up / kExactBits, r = up - kExactBits * j;
  const uint64_t x = m << r;  // < 2^63
  int64_t lo = (int64_t)(x & (((uint64_t)1 << kExactBits) - 1)), hi = (int64_t)(x >> kExactBits);
  if (b >> 31) {
    lo = -lo;
    hi = -hi;
  }
  // (j = 3 leaves hi = 0: s <= 136 there, so m 2^r < 2^40)
  w[0] += (j == 0) ? lo : 0;
  w[1] += (j == 1) ? lo : (j == 0) ? hi : 0;
  w[2] += (j == 2) ? lo : (j == 1) ? hi : 0;
  w[3] += (j == 3) ? lo : (j == 2) ? hi : 0;
  w[kExactLimbs] += bad ? 1 : 0;
}

__host__ __device__ inline int exact_clz64(uint64_t x) { return __builtin_clzll(x); }  // x != 0

// The limb totals -> the nearest double of sum_j w_j 2^(40 j - 80) (ties to
// even).  |w_j| < 2^63 (the summand bound), so the value is below 2^104.
__host__ __device__ inline double exact_to_double(const int64_t (&w)[kExactWords]) {
  if (w[kExactLimbs] != 0) return __builtin_nan("");
  constexpr uint64_t mask = ((uint64_t)1 << kExactBits) - 1;
  // carries up the limbs: digits dg[0..3] in [0, 2^40), signed top; a negative
  // total is negated limb by limb and carried again, so top >= 0 in the end
  uint64_t dg[kExactLimbs + 1];
  bool neg = false;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    int64_t carry = 0;
#pragma unroll
    for (int j = 0; j < kExactLimbs; ++j) {
      const int64_t lj = neg ? (int64_t)(0 - (uint64_t)w[j]) : w[j];
      // floor division by 2^40 without overflow: split before adding the carry
      const int64_t q = lj >> kExactBits;
      const int64_t rem = (int64_t)((uint64_t)lj & mask) + carry;  // carry in (-2^24, 2^24): may leave [0, 2^40)
      dg[j] = (uint64_t)rem & mask;
      carry = q + (rem >> kExactBits);
    }
    dg[kExactLimbs] = (uint64_t)carry;
    if (carry >= 0) break;
    neg = true;
  }
  // the leading non-zero digit k to the top slot (fixed trip count and
  // constant indices: the digits stay in registers)
  int k = kExactLimbs;
#pragma unroll
  for (int t = 0; t < kExactLimbs; ++t) {
    if (dg[4] == 0) {
      dg[4] = dg[3];
      dg[3] = dg[2];
      dg[2] = dg[1];
      dg[1] = dg[0];
      dg[0] = 0;
      --k;
    }
  }
  if (dg[4] == 0) return 0.0;
  // a 128-bit window over digits k, k - 1, k - 2 (at least 81 significant
  // bits), the digits below it as a sticky bit
  const uint64_t d1 = dg[3], d2 = dg[2];
  const bool sticky = (dg[1] | dg[0]) != 0;
  uint64_t hi = (dg[4] << 24) | (d1 >> 16);
  uint64_t lo = ((d1 & 0xFFFFu) << 48) | (d2 << 8);
  const int lz = exact_clz64(hi);
  if (lz > 0) {
    hi = (hi << lz) | (lo >> (64 - lz));
    lo <<= lz;
  }
  uint64_t mant = hi >> 11;  // 53 bits
  const uint64_t rem = hi & 0x7FFu;
  if (rem > 0x400u || (rem == 0x400u && (lo != 0 || sticky || (mant & 1u)))) mant += 1;
  // value = mant 2^(40 k - 93 - lz): an exact product (mant <= 2^53, the power normal)
  const int e2 = kExactBits * k - 93 - lz;
  const double scale = __builtin_bit_cast(double, (uint64_t)(e2 + 1023) << 52);
  const double v = (double)mant * scale;
  return neg ? -v : v;
}

}  // namespace amh
