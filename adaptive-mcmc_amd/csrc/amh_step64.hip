// amh_step64.hip -- the d = 64 persistent step kernel (arwmh_step64_kernel,
// ARWMH and ASSS), the headline of bench.py.  In order: LDS layout and piece
// table, the swap's group statements, batch readers / sweep 1 / scratch
// writers, the row-replicated forms of a single-step launch (s64_rows,
// s64_matvec_rows, s64_gauss_pot_rows), the pieces both transitions use
// (s64_matvec, s64_gauss_pot, s64_rank_one_coef, s64_sweep2),
// asss_transition64 and arwmh_transition64,
// the kernel, its launcher and the entry points run_step64 / run_asss_step64.
#include "amh_asss.h"
#include "amh_device.h"
#include "amh_s64_sched.h"
#include "amh_step_stage.h"

namespace amh {

// Diagnostic build only (-DAMH_STAMPS; tools/s64_tail.py, tools/s64_phases.py):
// one record per wave on the constant 100 MHz clock, read back with
// amh_diag_s64_stamps() -- [start, end, items, block, phase (a) .. (d) totals,
// the ARWMH compute phase's parts: noise, proposal, potential, accept +
// schedule, sweep 1 + coefficients, sweep 2 (each stamp is a scalar-memory
// round trip of its own: the parts sum to more than the release build's (d))].
#ifdef AMH_STAMPS
constexpr int kS64StampWaves = 1 << 16;
constexpr int kS64StampSlots = 16;
constexpr int kS64SubPhases = 6;
__device__ unsigned long long g_s64_stamps[kS64StampWaves * kS64StampSlots];
hipError_t diag_s64_stamps_copy(void* host, size_t bytes) {
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_s64_stamps), bytes, 0, hipMemcpyDeviceToHost);
}
#define AMH_S64_PHASE_INIT                                  \
  unsigned long long st_ph[4] = {0, 0, 0, 0}, st_pt = 0; \
  S64Sub st_sub = {{0, 0, 0, 0, 0, 0}, 0};
#define AMH_S64_PHASE_MARK st_pt = __builtin_amdgcn_s_memrealtime();
#define AMH_S64_PHASE(k)                                             \
  {                                                                  \
    const unsigned long long t_ = __builtin_amdgcn_s_memrealtime();  \
    st_ph[k] += t_ - st_pt;                                          \
    st_pt = t_;                                                      \
  }
struct S64Sub {
  unsigned long long ph[kS64SubPhases], pt;
};
#define AMH_S64_SUB_PARAM , S64Sub& st_sub
#define AMH_S64_SUB_ARG , st_sub
#define AMH_S64_SUB_MARK st_sub.pt = __builtin_amdgcn_s_memrealtime();
#define AMH_S64_SUB(k)                                               \
  {                                                                  \
    const unsigned long long t_ = __builtin_amdgcn_s_memrealtime();  \
    st_sub.ph[k] += t_ - st_sub.pt;                                  \
    st_sub.pt = t_;                                                  \
  }
#else
#define AMH_S64_PHASE_INIT
#define AMH_S64_PHASE_MARK
#define AMH_S64_PHASE(k)
#define AMH_S64_SUB_PARAM
#define AMH_S64_SUB_ARG
#define AMH_S64_SUB_MARK
#define AMH_S64_SUB(k)
#endif

// ------------------------------------------------------ d = 64 step kernel --
// The headline shape (BASELINE configs[1]: the d = 64 Gaussian, one chain per
// wave).  The same transition and the same float operations as
// arwmh_step_kernel<64, GaussianM, true> (bit-identical, oracle: orc_step);
// what differs is how data moves between HBM, LDS and registers:
//
// * Write-back through LDS.  After the DMA of item k has landed, one pass over
//   the columns reads item k's column j from the wave's LDS buffer and, at the
//   same addresses, writes item k-1's column j of L' = U diag(dl) (LDS is in
//   order within a wave, so the read sees the input).  The buffer then holds
//   item k-1's factor in the packed layout and goes to HBM as 9 full-lane
//   buffer_store_dwordx4 instead of 64 partially masked buffer_store_dword.
// * Exec-masked column ops.  Column j's LDS read and its normalisation touch
//   lanes r > j only (exec set by one SALU shift inside the asm), so the unit
//   diagonal and the zeros above it stay in the registers from the previous
//   chain; sweep 1 runs on lanes r > j, so lane r keeps its w_r when its own
//   column passes -- that is the forward-solve value the general kernel
//   captures with a v_writelane per column.
// * Broadcasts.  The per-column values every lane needs (dl_j and 1/l_j in
//   the swap, eta_j of the proposal, diff_j of the potential) are written once
//   per lane into a 1 KiB per-wave scratch and read back four columns at a
//   time with broadcast ds_read_b128, in place of v_readlane + s_nop per
//   column.  Sweep 1, whose w_j is serial, uses v_readlane.  Sweep 2's four
//   coefficients per column go through the scratch a quarter at a time into
//   every row of 16 lanes and reach the FMAs as DPP row broadcasts
//   (s64_rows_quarter, s64_sweep2_group).
// * Row-replicated registers, in a single-step ARWMH launch.  Its compute
//   phase runs beside the factor traffic and is bound by latency per wave,
//   where an LDS round trip costs the launch 0.25 us (0.68 us inside sweep 2's
//   serial chain).  There eta, diff and sweep 2's four coefficient vectors are
//   copied into every row of 16 lanes by permlane swaps (s64_rows: no scratch,
//   no LDS, no wait) and every column's FMA takes its value as a DPP
//   row_newbcast operand (s64_matvec_rows, s64_gauss_pot_rows,
//   s64_sweep2<true>).  A fused launch is bound by VALU issue and lost 4 %
//   with the proposal's rows form and 4 % with sweep 2's, ASSS 2 % with the
//   proposal's: they keep the scratch forms.
constexpr int kS64Waves = 16;
// Cache policy of this kernel's factor traffic (its own: kLoadAux / kStoreAux
// serve the other kernels), by the chain's place in the block's schedule
// (amh_s64_sched.h): 0 plain, 2 nt.  The DMA loads are nt everywhere (read
// once per launch; plain DMA loads lost on the kernel, for hot chains too).
// The flush's stores are plain so that the next, oppositely ordered launch
// finds what this one wrote last in the memory-side cache -- but for the hot
// chains, the first of a chained launch: nothing written that early survives
// the launch, and a store that does not allocate leaves the previous launch's
// last writes in the cache until they are read.  Plain stores for the tail
// alone lost, as did every other split tried (DESIGN.md 3.1 and its retired
// table, tools/ic_reuse.hip).
constexpr int kS64LoadAuxHot = 2, kS64LoadAuxCold = 2;
constexpr int kS64StoreAuxHot = 2, kS64StoreAuxMid = 0, kS64StoreAuxTail = 0;
// a drawn chain travels as its global index with the class bits above it
constexpr int kS64TagShift = 60;
constexpr int64_t kS64IdxMask = ((int64_t)1 << kS64TagShift) - 1;
// the class bits of a ticket -> the policy of the chain's factor loads / stores,
// handed to f as std::integral_constant<int, AUX> (an immediate of the
// instruction); equal policies need no branch
__device__ __forceinline__ int s64_cls(int64_t t) { return (int)(t >> kS64TagShift); }
template <class F>
__device__ __forceinline__ void s64_load_policy(int cls, F&& f) {
  using std::integral_constant;
  if constexpr (kS64LoadAuxHot == kS64LoadAuxCold) {
    f(integral_constant<int, kS64LoadAuxCold>{});
  } else {
    if (cls & (int)kS64Hot) f(integral_constant<int, kS64LoadAuxHot>{});
    else f(integral_constant<int, kS64LoadAuxCold>{});
  }
}
template <class F>
__device__ __forceinline__ void s64_store_policy(int cls, F&& f) {
  using std::integral_constant;
  if constexpr (kS64StoreAuxHot == kS64StoreAuxMid && kS64StoreAuxTail == kS64StoreAuxMid) {
    f(integral_constant<int, kS64StoreAuxMid>{});
  } else {
    if (cls & (int)kS64Hot) f(integral_constant<int, kS64StoreAuxHot>{});
    else if (cls & (int)kS64Tail) f(integral_constant<int, kS64StoreAuxTail>{});
    else f(integral_constant<int, kS64StoreAuxMid>{});
  }
}
constexpr int kS64EB = 8;   // proposal, vector from the scratch: broadcast columns per LDS wait
constexpr int kS64PB = 8;   // potential, vector from the scratch: columns per LDS wait
static_assert(kS64EB == 8 && kS64PB == 8, "the batch readers (lds_ld4x2w / lds_ld4x4w) read two quarter-vectors per stream");
typedef uint32_t uint32x4_t_ __attribute__((ext_vector_type(4)));
constexpr int kS64P = 2080;                   // d(d+1)/2
constexpr int kS64Z = 2080, kS64M = 2144, kS64S = 2208, kS64X = 2216;  // wave-buffer offsets (floats)
constexpr int kS64WB = kS64X + 64;            // floats per wave buffer (9,120 B): 64-float scratch
constexpr int kS64Model = 64 * 68;            // GaussianM<64> rows (lds_bytes / 4)
static_assert(kS64Z == 2080 && kS64S == kS64M + 64, "layout of prefetch_item<64>");
// + 32 floats: the ticket, the hot / tail ranges after it, the own part, n and T of a single-step launch (amh_s64_sched.h), and slack for flush_factor's 9 KiB read of the last wave buffer
template <int WPB = kS64Waves>
constexpr size_t s64_lds_bytes() { return ((size_t)kS64Model + (size_t)WPB * kS64WB + 32) * sizeof(float); }

constexpr int s64_col(int j) { return j * 64 - j * (j - 1) / 2; }  // packed column offset

// The factor moves between the wave buffer and HBM in kS64Pieces pieces: eight
// of 256 floats (1 KB: 16 B per lane) and the 32-float tail.  The swap walks
// the columns in 16 groups of four; after group g every float below
// s64_col(4 g + 4) holds the outgoing chain's L' and the incoming chain's are
// in registers, so a piece that ends at or below it can leave and be refilled.
constexpr int kS64Pieces = 9;
constexpr int s64_piece_end(int m) { return m < kS64Pieces - 1 ? 256 * (m + 1) : kS64P; }
constexpr int s64_piece_group(int m) {  // the swap group after which piece m is finished
  for (int g = 0; g < 16; ++g)
    if (s64_col(4 * g + 4) >= s64_piece_end(m)) return g;
  return -1;
}
constexpr int s64_piece_after(int g) {  // the piece that swap group g finishes, or -1
  for (int m = 0; m < kS64Pieces; ++m)
    if (s64_piece_group(m) == g) return m;
  return -1;
}
constexpr bool s64_pieces_ok() {
  int n = 0;
  for (int g = 0; g < 16; ++g) n += s64_piece_after(g) >= 0;
  for (int m = 0; m + 1 < kS64Pieces; ++m)
    if (s64_piece_group(m) < 0 || s64_piece_group(m) >= s64_piece_group(m + 1)) return false;
  return n == kS64Pieces;  // no group finishes two pieces
}
static_assert(256 * (kS64Pieces - 1) <= kS64P && kS64P - 256 * (kS64Pieces - 1) <= 64, "eight 1-KB pieces and a one-DMA tail");
static_assert(s64_col(64) == kS64P && s64_pieces_ok(), "every piece is finished by its own swap group, in order");
static_assert(s64_piece_group(0) == 1 && s64_piece_group(4) == 6 && s64_piece_group(7) == 14 &&
                  s64_piece_group(kS64Pieces - 1) == 15,
              "the table of DESIGN.md 3.1");

// The swap's group of four columns j = 4 G .. 4 G + 3 as whole statements:
// one s_lshl_b64 exec per mask and ONE exec restore per masked statement, where a
// statement per masked operation saves, shifts and restores exec around it
// and has hipcc's boundary pad after it (80 instructions per group).  exec is
// restored with s_mov_b64 exec, -1 and not from a saved pair (no SGPR pair
// live across the statement): valid only because every wave of the kernel is
// full (the block is WPB whole waves, asserted in the kernel) and the swap
// runs under wave-uniform control only.  None of the pairs inside a string
// needs a wait state: SALU write of exec -> DS / VALU, VALU write of a VGPR
// -> DS read of it as data.
//
// s64_group_read: [dl | 1/l] quarter-vectors of the group, the piece the
// previous group finished (MP >= 0: 16 B per lane at la16), the group's
// columns of the incoming factor, in that order, and their one wait.  The
// column reads carry no mask: column j's address la + (s64_col(j) - j) 4 lies
// inside the wave buffer for every lane (s64_col(j) >= j, and lane 63 of
// column 63 is the factor's last float), and t[k] is consumed on lanes r > j
// only (s64_group_norm), so what the lanes r <= j read is never used -- one
// s_lshl_b64 exec per column less than the masked read.
#define AMH_SWG_RD(k) "ds_read_b32 %[t" #k "], %[la] offset:%[o" #k "]\n\t"
#define AMH_SWG_RD_HEAD "ds_read_b128 %[dl], %[zm] offset:%[od]\n\tds_read_b128 %[in], %[zm] offset:%[oi]\n\t"
#define AMH_SWG_RD_PIECE "ds_read_b128 %[pv], %[lp] offset:%[op]\n\t"
#define AMH_SWG_RD_TAIL "s_waitcnt lgkmcnt(0)"
template <int G, int MP>
__device__ __forceinline__ void s64_group_read(f32x4& dl4, f32x4& in4, f32x4& pv, float (&t)[4], uint32_t zm_a,
                                               uint32_t la16, uint32_t la) {
  constexpr int j = 4 * G;
  static_assert(G < 15 || MP >= 0, "the last group reads the piece that group 14 finished");
  static_assert(s64_col(j) >= j && s64_col(j + 3) - (j + 3) + 63 < kS64P, "unmasked column reads stay inside the factor");
#define AMH_SWG_RD_OPS3                                                                          \
  [zm] "v"(zm_a), [la] "v"(la), [od] "n"(16 * G), [oi] "n"(256 + 16 * G),                       \
      [o0] "n"((s64_col(j) - j) * 4), [o1] "n"((s64_col(j + 1) - (j + 1)) * 4),                 \
      [o2] "n"((s64_col(j + 2) - (j + 2)) * 4)
  if constexpr (G == 15) {  // column 63 has nothing below its diagonal
    asm volatile(AMH_SWG_RD_HEAD AMH_SWG_RD_PIECE AMH_SWG_RD(0) AMH_SWG_RD(1) AMH_SWG_RD(2) AMH_SWG_RD_TAIL
                 : [dl] "=&v"(dl4), [in] "=&v"(in4), [pv] "=&v"(pv), [t0] "=&v"(t[0]), [t1] "=&v"(t[1]),
                   [t2] "=&v"(t[2])
                 : AMH_SWG_RD_OPS3, [lp] "v"(la16), [op] "n"(1024 * MP));
  } else if constexpr (MP >= 0) {
    asm volatile(AMH_SWG_RD_HEAD AMH_SWG_RD_PIECE AMH_SWG_RD(0) AMH_SWG_RD(1) AMH_SWG_RD(2) AMH_SWG_RD(3)
                     AMH_SWG_RD_TAIL
                 : [dl] "=&v"(dl4), [in] "=&v"(in4), [pv] "=&v"(pv), [t0] "=&v"(t[0]), [t1] "=&v"(t[1]),
                   [t2] "=&v"(t[2]), [t3] "=&v"(t[3])
                 : AMH_SWG_RD_OPS3, [o3] "n"((s64_col(j + 3) - (j + 3)) * 4), [lp] "v"(la16), [op] "n"(1024 * MP));
  } else {
    asm volatile(AMH_SWG_RD_HEAD AMH_SWG_RD(0) AMH_SWG_RD(1) AMH_SWG_RD(2) AMH_SWG_RD(3) AMH_SWG_RD_TAIL
                 : [dl] "=&v"(dl4), [in] "=&v"(in4), [t0] "=&v"(t[0]), [t1] "=&v"(t[1]), [t2] "=&v"(t[2]),
                   [t3] "=&v"(t[3])
                 : AMH_SWG_RD_OPS3, [o3] "n"((s64_col(j + 3) - (j + 3)) * 4));
  }
#undef AMH_SWG_RD_OPS3
}
// L' = U diag(dl) of the outgoing chain, columns j on lanes r >= j, into the
// addresses just read (the products take dl's registers, on every lane)
#define AMH_SWG_LP                                                                      \
  "v_mul_f32 %[d0], %[u0], %[d0]\n\tv_mul_f32 %[d1], %[u1], %[d1]\n\t"                  \
  "v_mul_f32 %[d2], %[u2], %[d2]\n\tv_mul_f32 %[d3], %[u3], %[d3]\n\t"
#define AMH_SWG_WR(k) "ds_write_b32 %[la], %[d" #k "] offset:%[o" #k "]\n\t"
#define AMH_SWG_NRM(k) "v_mul_f32 %[u" #k "], %[t" #k "], %[i" #k "]\n\t"
#define AMH_SWG_SH(k) "s_lshl_b64 exec, -1, %[m" #k "]\n\t"
#define AMH_SWG_OFFS                                                                                          \
  [o0] "n"((s64_col(j) - j) * 4), [o1] "n"((s64_col(j + 1) - (j + 1)) * 4),                                   \
      [o2] "n"((s64_col(j + 2) - (j + 2)) * 4), [o3] "n"((s64_col(j + 3) - (j + 3)) * 4), [m0] "n"(j),        \
      [m1] "n"(j + 1), [m2] "n"(j + 2), [m3] "n"(j + 3)
// the L' writes (also of the last item of a wave, where nothing comes in)
template <int G>
__device__ __forceinline__ void s64_group_write(const float (&U)[64], uint32_t la, const f32x4& dl4) {
  constexpr int j = 4 * G;
  float d0 = dl4[0], d1 = dl4[1], d2 = dl4[2], d3 = dl4[3];
  asm volatile(AMH_SWG_LP AMH_SWG_SH(0) AMH_SWG_WR(0) AMH_SWG_SH(1) AMH_SWG_WR(1) AMH_SWG_SH(2) AMH_SWG_WR(2)
                   AMH_SWG_SH(3) AMH_SWG_WR(3) "s_mov_b64 exec, -1"
               : [d0] "+v"(d0), [d1] "+v"(d1), [d2] "+v"(d2), [d3] "+v"(d3)
               : [la] "v"(la), [u0] "v"(U[j]), [u1] "v"(U[j + 1]), [u2] "v"(U[j + 2]), [u3] "v"(U[j + 3]), AMH_SWG_OFFS
               : "memory");
}
// the normalisation U_rj = t_j / l_j of the incoming chain on lanes r > j.  (The
// L' writes interleaved with it share masks, five shifts for eight operations,
// but the swap writes only under `wr`: two statements that define U on the two
// sides of a branch cost copies and, on this kernel, 51 spilled VGPRs.)
template <int G>
__device__ __forceinline__ void s64_group_norm(float (&U)[64], const f32x4& in4, const float (&t)[4]) {
  constexpr int j = 4 * G;
  if constexpr (G < 15) {
    asm volatile(AMH_SWG_SH(1) AMH_SWG_NRM(0) AMH_SWG_SH(2) AMH_SWG_NRM(1) AMH_SWG_SH(3) AMH_SWG_NRM(2) AMH_SWG_SH(4)
                     AMH_SWG_NRM(3) "s_mov_b64 exec, -1"
                 : [u0] "+v"(U[j]), [u1] "+v"(U[j + 1]), [u2] "+v"(U[j + 2]), [u3] "+v"(U[j + 3])
                 : [t0] "v"(t[0]), [t1] "v"(t[1]), [t2] "v"(t[2]), [t3] "v"(t[3]), [i0] "v"(in4[0]), [i1] "v"(in4[1]),
                   [i2] "v"(in4[2]), [i3] "v"(in4[3]), [m1] "n"(j + 1), [m2] "n"(j + 2), [m3] "n"(j + 3),
                   [m4] "n"(j + 4));
  } else {
    asm volatile(AMH_SWG_SH(1) AMH_SWG_NRM(0) AMH_SWG_SH(2) AMH_SWG_NRM(1) AMH_SWG_SH(3) AMH_SWG_NRM(2)
                 "s_mov_b64 exec, -1"
                 : [u0] "+v"(U[j]), [u1] "+v"(U[j + 1]), [u2] "+v"(U[j + 2])
                 : [t0] "v"(t[0]), [t1] "v"(t[1]), [t2] "v"(t[2]), [i0] "v"(in4[0]), [i1] "v"(in4[1]),
                   [i2] "v"(in4[2]), [m1] "n"(j + 1), [m2] "n"(j + 2), [m3] "n"(j + 3));
  }
}
// LDS batches read and waited for in ONE statement (outputs "=&v"): per
// batch one boundary pad instead of two (separate read and wait statements
// each have hipcc's pad around them).
template <int O0, int O1>
__device__ __forceinline__ void lds_ld4x2w(f32x4& a, f32x4& b, uint32_t addr) {
  asm volatile("ds_read_b128 %0, %2 offset:%3\n\tds_read_b128 %1, %2 offset:%4\n\ts_waitcnt lgkmcnt(0)"
               : "=&v"(a), "=&v"(b)
               : "v"(addr), "n"(O0), "n"(O1));
}
// a, b from addr0 (offsets O0, O1); c, d from addr1 (O2, O3)
template <int O0, int O1, int O2, int O3>
__device__ __forceinline__ void lds_ld4x4w(f32x4& a, f32x4& b, f32x4& c, f32x4& d, uint32_t addr0, uint32_t addr1) {
  asm volatile("ds_read_b128 %0, %4 offset:%6\n\tds_read_b128 %1, %4 offset:%7\n\t"
               "ds_read_b128 %2, %5 offset:%8\n\tds_read_b128 %3, %5 offset:%9\n\ts_waitcnt lgkmcnt(0)"
               : "=&v"(a), "=&v"(b), "=&v"(c), "=&v"(d)
               : "v"(addr0), "v"(addr1), "n"(O0), "n"(O1), "n"(O2), "n"(O3));
}

// sweep 1 (column J: w_J broadcast, then w -= w_J U_rJ on lanes r > J) over
// eight columns J0 .. J0 + 7 (seven when J0 = 56: columns up to 62) in one
// statement: exec saved once and restored once, each column s_lshl exec
// (lanes r > J) / v_readlane / s_nop 1 / v_fma / s_nop 0.  A VALU read of an
// SGPR written by v_readlane needs two wait states, and SALU instructions in
// between do not provide them (measured: with only the exec setup in
// between, a few chains per thousand read the previous column's w_j), so the
// s_nop 1 stays.  The s_nop 0 is the VALU-write -> v_readlane wait state of
// the next column (one statement per column has hipcc's boundary pad there,
// plus an exec save and restore per column: 8 slots per column, here 5).
#define AMH_SW1_COL(k)                                                          \
  "s_lshl_b64 exec, -1, %[s" #k "]\n\tv_readlane_b32 %[t], %[w], %[l" #k "]\n\t" \
  "s_nop 1\n\tv_fma_f32 %[w], -%[t], %[u" #k "], %[w]\n\ts_nop 0\n\t"
template <int J0>
__device__ __forceinline__ void s64_sweep1x8(float& w, const float (&U)[64]) {
  uint64_t sv;
  uint32_t t;
  if constexpr (J0 + 7 <= 62) {
    asm volatile("s_mov_b64 %[sv], exec\n\t" AMH_SW1_COL(0) AMH_SW1_COL(1) AMH_SW1_COL(2) AMH_SW1_COL(3)
                 AMH_SW1_COL(4) AMH_SW1_COL(5) AMH_SW1_COL(6) AMH_SW1_COL(7) "s_mov_b64 exec, %[sv]"
                 : [w] "+v"(w), [t] "=&s"(t), [sv] "=&s"(sv)
                 : [u0] "v"(U[J0]), [u1] "v"(U[J0 + 1]), [u2] "v"(U[J0 + 2]), [u3] "v"(U[J0 + 3]),
                   [u4] "v"(U[J0 + 4]), [u5] "v"(U[J0 + 5]), [u6] "v"(U[J0 + 6]), [u7] "v"(U[J0 + 7]),
                   [s0] "n"(J0 + 1), [s1] "n"(J0 + 2), [s2] "n"(J0 + 3), [s3] "n"(J0 + 4), [s4] "n"(J0 + 5),
                   [s5] "n"(J0 + 6), [s6] "n"(J0 + 7), [s7] "n"(J0 + 8), [l0] "n"(J0), [l1] "n"(J0 + 1),
                   [l2] "n"(J0 + 2), [l3] "n"(J0 + 3), [l4] "n"(J0 + 4), [l5] "n"(J0 + 5), [l6] "n"(J0 + 6),
                   [l7] "n"(J0 + 7));
  } else {
    static_assert(J0 == 56, "sweep 1 covers columns 0 .. 62");
    asm volatile("s_mov_b64 %[sv], exec\n\t" AMH_SW1_COL(0) AMH_SW1_COL(1) AMH_SW1_COL(2) AMH_SW1_COL(3)
                 AMH_SW1_COL(4) AMH_SW1_COL(5) AMH_SW1_COL(6) "s_mov_b64 exec, %[sv]"
                 : [w] "+v"(w), [t] "=&s"(t), [sv] "=&s"(sv)
                 : [u0] "v"(U[J0]), [u1] "v"(U[J0 + 1]), [u2] "v"(U[J0 + 2]), [u3] "v"(U[J0 + 3]),
                   [u4] "v"(U[J0 + 4]), [u5] "v"(U[J0 + 5]), [u6] "v"(U[J0 + 6]), [s0] "n"(J0 + 1),
                   [s1] "n"(J0 + 2), [s2] "n"(J0 + 3), [s3] "n"(J0 + 4), [s4] "n"(J0 + 5), [s5] "n"(J0 + 6),
                   [s6] "n"(J0 + 7), [l0] "n"(J0), [l1] "n"(J0 + 1), [l2] "n"(J0 + 2), [l3] "n"(J0 + 3),
                   [l4] "n"(J0 + 4), [l5] "n"(J0 + 5), [l6] "n"(J0 + 6));
  }
}
#undef AMH_SW1_COL
// the whole sweep 1 (columns 0 .. 62)
__device__ __forceinline__ void s64_sweep1_all(float& w, const float (&U)[64]) {
  static_for<8>([&](auto B) {
    s64_sweep1x8<8 * B>(w, U);
    __builtin_amdgcn_sched_barrier(0);
  });
}

__device__ __forceinline__ void s64_wr(uint32_t a, float v) {  // this lane's dword at a
  asm volatile("ds_write_b32 %0, %1" : : "v"(a), "v"(v) : "memory");
}
template <int OFF>
__device__ __forceinline__ void s64_wr_off(uint32_t a, float v) {
  asm volatile("ds_write_b32 %0, %1 offset:%2" : : "v"(a), "v"(v), "n"(OFF) : "memory");
}
__device__ __forceinline__ void s64_wait() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
template <class T>
__device__ __forceinline__ void s64_tie(T& a) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a)); }
template <class T>
__device__ __forceinline__ void s64_tie(T& a, T& b) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b)); }

// lane J takes v (its own value), the others keep old -- capture<64, J> of a
// broadcast of lane J's own value, without the v_readlane / v_writelane pair
template <int J>
__device__ __forceinline__ float s64_keep_at(float old, float v) {
  float out;
  unsigned long long m;
  asm("s_lshl_b64 %1, 1, %4\n\tv_cndmask_b32_e64 %0, %2, %3, %1" : "=v"(out), "=&s"(m) : "v"(old), "v"(v), "n"(J));
  return out;
}

// v, one value per lane, copied into every row of 16 lanes: lane r of e[Q]
// holds v of lane 16 Q + r mod 16.  permlane16_swap(v, v) gives rows 0 0 2 2
// and rows 1 1 3 3, a permlane32_swap of each with itself the four quarters:
// three swaps and three copies, no scratch, no LDS, no wait.  A column's FMA
// then takes its value as a DPP row_newbcast operand (s64_dot16,
// s64_sweep2_group) and needs no broadcast instruction.  Bit copies.
__device__ __forceinline__ void s64_rows(float v, float (&e)[4]) {
  const int iv = __float_as_int(v);
  const auto a = __builtin_amdgcn_permlane16_swap(iv, iv, false, false);
  const auto b = __builtin_amdgcn_permlane32_swap(a[0], a[0], false, false);
  const auto c = __builtin_amdgcn_permlane32_swap(a[1], a[1], false, false);
  e[0] = __int_as_float((int)b[0]);
  e[1] = __int_as_float((int)c[0]);
  e[2] = __int_as_float((int)b[1]);
  e[3] = __int_as_float((int)c[1]);
}
// a[k & 3] = fma(e_k, x_k, a[k & 3]) for k = 0 .. 15, e_k the value of lane k of
// this lane's row of 16 in e (one quarter of s64_rows), x(k) this lane's
// factor: sixteen v_fmac_f32_dpp.  The s_nop 1 are the two wait states of a
// DPP read of a VGPR that a VALU instruction (a swap's copy) may have written
// right in front of the statement; inside it e is not written.
#define AMH_ROW_FMAC(k, a) \
  "v_fmac_f32_dpp %[a" #a "], %[e], %[x" #k "] row_newbcast:" #k " row_mask:0xf bank_mask:0xf\n\t"
template <class X>
__device__ __forceinline__ void s64_dot16(float (&a)[4], float e, X&& x) {
  using std::integral_constant;
#define AMH_ROW_X(k) [x##k] "v"(x(integral_constant<int, k>{}))
  asm("s_nop 1\n\t" AMH_ROW_FMAC(0, 0) AMH_ROW_FMAC(1, 1) AMH_ROW_FMAC(2, 2) AMH_ROW_FMAC(3, 3) AMH_ROW_FMAC(4, 0)
          AMH_ROW_FMAC(5, 1) AMH_ROW_FMAC(6, 2) AMH_ROW_FMAC(7, 3) AMH_ROW_FMAC(8, 0) AMH_ROW_FMAC(9, 1)
              AMH_ROW_FMAC(10, 2) AMH_ROW_FMAC(11, 3) AMH_ROW_FMAC(12, 0) AMH_ROW_FMAC(13, 1) AMH_ROW_FMAC(14, 2)
                  AMH_ROW_FMAC(15, 3)
      : [a0] "+v"(a[0]), [a1] "+v"(a[1]), [a2] "+v"(a[2]), [a3] "+v"(a[3])
      : [e] "v"(e), AMH_ROW_X(0), AMH_ROW_X(1), AMH_ROW_X(2), AMH_ROW_X(3), AMH_ROW_X(4), AMH_ROW_X(5), AMH_ROW_X(6),
        AMH_ROW_X(7), AMH_ROW_X(8), AMH_ROW_X(9), AMH_ROW_X(10), AMH_ROW_X(11), AMH_ROW_X(12), AMH_ROW_X(13),
        AMH_ROW_X(14), AMH_ROW_X(15));
#undef AMH_ROW_X
}
#undef AMH_ROW_FMAC
// ... for k = L0 .. L0 + 7 (L0 = 0 or 8): half a row
#define AMH_ROW_FMAC(k, a) \
  "v_fmac_f32_dpp %[a" #a "], %[e], %[x" #k "] row_newbcast:%[l" #k "] row_mask:0xf bank_mask:0xf\n\t"
template <int L0, class X>
__device__ __forceinline__ void s64_dot8(float (&a)[4], float e, X&& x) {
  using std::integral_constant;
  static_assert(L0 == 0 || L0 == 8, "k & 3 = (L0 + k) & 3");
#define AMH_ROW_X(k) [x##k] "v"(x(integral_constant<int, k>{})), [l##k] "n"(L0 + k)
  asm("s_nop 1\n\t" AMH_ROW_FMAC(0, 0) AMH_ROW_FMAC(1, 1) AMH_ROW_FMAC(2, 2) AMH_ROW_FMAC(3, 3) AMH_ROW_FMAC(4, 0)
          AMH_ROW_FMAC(5, 1) AMH_ROW_FMAC(6, 2) AMH_ROW_FMAC(7, 3)
      : [a0] "+v"(a[0]), [a1] "+v"(a[1]), [a2] "+v"(a[2]), [a3] "+v"(a[3])
      : [e] "v"(e), AMH_ROW_X(0), AMH_ROW_X(1), AMH_ROW_X(2), AMH_ROW_X(3), AMH_ROW_X(4), AMH_ROW_X(5), AMH_ROW_X(6),
        AMH_ROW_X(7));
#undef AMH_ROW_X
}
#undef AMH_ROW_FMAC

// U h, h one element per lane: column j's h_j from the row-replicated
// registers of h.  The accumulators and the final sum are s64_matvec's, the
// products have their factors swapped: the same bits.
__device__ __forceinline__ float s64_matvec_rows(const float (&U)[64], float h) {
  float e[4];
  s64_rows(h, e);
  float a4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  static_for<4>([&](auto Q) {
    s64_dot16(a4, e[(int)Q], [&](auto K) { return U[16 * (int)Q + (int)K]; });
    __builtin_amdgcn_sched_barrier(0);
  });
  return (a4[0] + a4[1]) + (a4[2] + a4[3]);
}

// The d = 64 Gaussian potential (GaussianM<64>::potential, the same float
// operations and order) with diff_j from the row-replicated registers of diff.
// This lane's row of P comes eight columns per LDS wait with the next eight in
// flight behind them: each half of pv is read again as soon as its FMAs have
// taken it (LDS returns in order: at most two reads outstanding means the
// older two have landed).  The four accumulators are the packed form's
// (column j adds to y[j & 3]), so the bits are s64_gauss_pot's.
__device__ __forceinline__ float s64_gauss_pot_rows(float diff, uint32_t prow, float c0) {
  f32x4 pv[4];
  static_for<4>([&](auto Q) { pv[(int)Q] = lds_ld4<16 * (int)Q>(prow); });
  float dq[4];
  s64_rows(diff, dq);
  float y4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  static_for<8>([&](auto B) {
    constexpr int b = B, h = 2 * (b % 2);  // columns 8 b .. 8 b + 7 in pv[h], pv[h + 1]
    if constexpr (b < 7) {
      asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(pv[h]), "+v"(pv[h + 1]));
    } else {
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(pv[h]), "+v"(pv[h + 1]));
    }
    s64_dot8<4 * h>(y4, dq[b / 2], [&](auto K) { return pv[h + (int)K / 4][(int)K % 4]; });
    if constexpr (b + 2 < 8) {
      pv[h] = lds_ld4<16 * (2 * (b + 2))>(prow);
      pv[h + 1] = lds_ld4<16 * (2 * (b + 2) + 1)>(prow);
    }
    __builtin_amdgcn_sched_barrier(0);
  });
  const float y = (y4[0] + y4[1]) + (y4[2] + y4[3]);
  const float S = Grp<64>::sum(diff * y);
  return (0.5f * S) + c0;
}

// U h through the wave's scratch: lane r writes h_r to x_a and reads the vector
// back kS64EB columns per LDS wait (16-B broadcast reads).  WAIT: every lane's
// reads are done before the caller writes the scratch again (the wait sits
// before the final sums, as the ASSS transition had it).
template <bool WAIT = false>
__device__ __forceinline__ float s64_matvec(const float (&U)[64], float h, uint32_t x_a, uint32_t r) {
  s64_wr(x_a + r * 4u, h);
  float a4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  static_for<64 / kS64EB>([&](auto B) {
    constexpr int b = B;
    f32x4 e[kS64EB / 4];
    lds_ld4x2w<16 * (2 * b), 16 * (2 * b + 1)>(e[0], e[1], x_a);
    static_for<kS64EB>([&](auto K) {
      constexpr int j = kS64EB * b + K;
      a4[j & 3] = fmaf(U[j], e[(int)K / 4][(int)K % 4], a4[j & 3]);
    });
    __builtin_amdgcn_sched_barrier(0);
  });
  if constexpr (WAIT) s64_wait();
  return (a4[0] + a4[1]) + (a4[2] + a4[3]);
}

// The d = 64 Gaussian potential (GaussianM<64>::potential, the same float
// operations and order) with diff_j read back from the wave's scratch x_a
// (one ds_write, then 16-B broadcast reads) instead of 64 v_readlane.
__device__ __forceinline__ float s64_gauss_pot(float diff, uint32_t x_a, uint32_t prow, uint32_t r, float c0) {
  s64_wr(x_a + r * 4u, diff);
  f32x2v y01 = {0.0f, 0.0f}, y23 = {0.0f, 0.0f};
  static_for<64 / kS64PB>([&](auto B) {
    constexpr int b = B;
    constexpr int NQ = kS64PB / 4;
    f32x4 pv[NQ], dv[NQ];
    lds_ld4x4w<16 * (2 * b), 16 * (2 * b + 1), 16 * (2 * b), 16 * (2 * b + 1)>(pv[0], pv[1], dv[0], dv[1], prow, x_a);
    static_for<2 * NQ>([&](auto K2) {
      const f32x4 q = pv[(int)K2 / 2];
      const f32x4 dq = dv[(int)K2 / 2];
      const f32x2v pp = (K2 % 2 == 0) ? f32x2v{q[0], q[1]} : f32x2v{q[2], q[3]};
      const f32x2v bp = (K2 % 2 == 0) ? f32x2v{dq[0], dq[1]} : f32x2v{dq[2], dq[3]};
      if constexpr (K2 % 2 == 0) {
        y01 = __builtin_elementwise_fma(pp, bp, y01);
      } else {
        y23 = __builtin_elementwise_fma(pp, bp, y23);
      }
    });
    __builtin_amdgcn_sched_barrier(0);
  });
  const float y = (y01[0] + y01[1]) + (y23[0] + y23[1]);
  const float S = Grp<64>::sum(diff * y);
  return (0.5f * S) + c0;
}

// The rank-one update's column coefficients after sweep 1 (lane r holds
// ws = w*_r, Dg = (sqrt(1 - gamma) dl_r)^2, one = 1 or NaN for a bad pivot)
// and the wave's NaN vote: revert -> keep L.
struct S64Coef {
  bool revert;  // wave-uniform
  float c, q;   // c_r and the new diagonal q_r
};
__device__ __forceinline__ S64Coef s64_rank_one_coef(float ws, float Dg, float one, float gamma, int r) {
  using Gp = Grp<64>;
  const float gw2 = gamma * (ws * ws);
  const float tsc = gw2 / Dg;
  const float b = 1.0f + Gp::excl_scan(tsc, r);
  const float g2 = (b * Dg) + gw2;
  const float dn = g2 / b;
  const float c = (gamma * ws) / g2;
  const float q = sqrtf(dn);
  const float dnew = fmaf(c, 0.0f, one) * q;
  return {Gp::any(amh_isnan(dnew)), c, q};
}
// Quarter Q of the four coefficient vectors to every row of 16 lanes: lanes
// 16Q .. 16Q+15 write v0..v3 at a, a+64, a+128, a+192 (a = scratch + 4 (r mod
// 16)) and every lane reads its slot back, so that lane r holds the values of
// lane 16Q + r mod 16 (LDS is in order within a wave); one round trip.
template <int Q>
__device__ __forceinline__ void s64_rows_quarter(uint32_t a, float v0, float v1, float v2, float v3, float& o0,
                                                 float& o1, float& o2, float& o3) {
  uint64_t sv;
  asm volatile("s_mov_b64 %[sv], exec\n\ts_bfm_b64 exec, 16, %[q]\n\tds_write_b32 %[a], %[v0]\n\t"
               "ds_write_b32 %[a], %[v1] offset:64\n\tds_write_b32 %[a], %[v2] offset:128\n\t"
               "ds_write_b32 %[a], %[v3] offset:192\n\ts_mov_b64 exec, %[sv]\n\t"
               "ds_read_b32 %[o0], %[a]\n\tds_read_b32 %[o1], %[a] offset:64\n\t"
               "ds_read_b32 %[o2], %[a] offset:128\n\tds_read_b32 %[o3], %[a] offset:192\n\t"
               "s_waitcnt lgkmcnt(0)"
               : [sv] "=&s"(sv), [o0] "=&v"(o0), [o1] "=&v"(o1), [o2] "=&v"(o2), [o3] "=&v"(o3)
               : [a] "v"(a), [v0] "v"(v0), [v1] "v"(v1), [v2] "v"(v2), [v3] "v"(v3), [q] "n"(16 * Q)
               : "memory");
}
// Columns j = 4 G .. 4 G + 3 of sweep 2, the coefficients of column j taken from
// lane j mod 16 of the lane's own row (DPP row_newbcast on the first source
// of v_fmac / v_mul: no broadcast instruction of its own).  Per column
//   w  = fma(-ws_j, u, w);  t = bc_j w;  t = fma(ac_j, u, t);  u = fma(c_j, w, u)
// -- the generic kernel's operations with the factors of a product swapped:
// the same bits.  The s_nop 1 are the two wait states of a DPP read of a VGPR
// that a VALU wrote, should the compiler have copied a coefficient in front
// of the statement; inside it the DPP operands are never written.
#define AMH_SW2_COL(k)                                                                              \
  "v_fmac_f32_dpp %[w], -%[cw], %[u" #k "] row_newbcast:%[l" #k "] row_mask:0xf bank_mask:0xf\n\t"  \
  "v_mul_f32_dpp %[t" #k "], %[cb], %[w] row_newbcast:%[l" #k "] row_mask:0xf bank_mask:0xf\n\t"    \
  "v_fmac_f32_dpp %[t" #k "], %[ca], %[u" #k "] row_newbcast:%[l" #k "] row_mask:0xf bank_mask:0xf\n\t" \
  "v_fmac_f32_dpp %[u" #k "], %[cc], %[w] row_newbcast:%[l" #k "] row_mask:0xf bank_mask:0xf\n\t"
template <int G>
__device__ __forceinline__ void s64_sweep2_group(float (&U)[64], float& w, float (&t)[4], float cw, float cc, float ca,
                                                 float cb) {
  constexpr int j = 4 * G, l = j % 16;
  asm("s_nop 1\n\t" AMH_SW2_COL(0) AMH_SW2_COL(1) AMH_SW2_COL(2) AMH_SW2_COL(3)
      : [w] "+v"(w), [u0] "+v"(U[j]), [u1] "+v"(U[j + 1]), [u2] "+v"(U[j + 2]), [u3] "+v"(U[j + 3]), [t0] "=&v"(t[0]),
        [t1] "=&v"(t[1]), [t2] "=&v"(t[2]), [t3] "=&v"(t[3])
      : [cw] "v"(cw), [cc] "v"(cc), [ca] "v"(ca), [cb] "v"(cb), [l0] "n"(l), [l1] "n"(l + 1), [l2] "n"(l + 2),
        [l3] "n"(l + 3));
}
#undef AMH_SW2_COL
// Sweep 2 of the rank-one update: U'_rj = U_rj + c_j w_r^{(j+1)} in 16 groups of
// four columns, the coefficient vectors (this lane's ws, c, ac, bc) a quarter
// at a time to every row through the quarter-vector scratch: four LDS round
// trips per item and no broadcast read (the broadcast 16-B reads it replaces
// took sixteen, and 64 ds_read_b128).  kRows: all four quarters of the four
// vectors by permlane swaps in front of the serial chain instead (s64_rows:
// sixteen registers, no round trip).  Returns the wave sum of the as_change
// terms (U_rj ac_j + bc_j w_r^{(j+1)})^2; ac and bc are where the transitions
// differ.
template <bool kRows>
__device__ __forceinline__ float s64_sweep2(float (&U)[64], float delta, float ws, float c, float ac, float bc,
                                            uint32_t xq_a) {
  float s4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  float w = delta;
  float rw[4], rc[4], ra[4], rb[4];
  if constexpr (kRows) {
    s64_rows(ws, rw);
    s64_rows(c, rc);
    s64_rows(ac, ra);
    s64_rows(bc, rb);
  }
  static_for<16>([&](auto G4) {
    constexpr int g = G4, q = kRows ? g / 4 : 0;
    float t[4];
    if constexpr (!kRows && g % 4 == 0) s64_rows_quarter<g / 4>(xq_a, ws, c, ac, bc, rw[0], rc[0], ra[0], rb[0]);
    s64_sweep2_group<g>(U, w, t, rw[q], rc[q], ra[q], rb[q]);
    static_for<4>([&](auto Q) { s4[(int)Q] = fmaf(t[(int)Q], t[(int)Q], s4[(int)Q]); });
    column_fence<g, 2>();
  });
  const float sacc = (s4[0] + s4[1]) + (s4[2] + s4[3]);
  return Grp<64>::sum(sacc);
}

// asss_transition<64, GaussianM, true> (amh_asss.h; asss.py:197-251) for the
// d = 64 persistent kernel: the same float operations in the same order (so
// the same bits as the generic transition and orc_asss_step), with the
// column broadcasts of the step64 ARWMH path -- the matrix-vector products
// S z, S v and every potential read their broadcast vector from the wave's
// LDS scratch, sweep 1 is s64_sweep1_all, sweep 2 the quarter-vector LDS scheme,
// and the forward solve keeps one v_readlane per column (its own y_j by a
// select).  The generic form spent ~576 + 64 (shrink steps + 2) v_readlane per
// transition.
__device__ __forceinline__ void asss_transition64(const StepParams& p, float (&U)[64], float& dl, float& x, float& mu,
                                                  float& pe, float& asc, bool& updated, int32_t it, uint32_t k0,
                                                  uint32_t k1, int r, const GaussianM<64>::Ctx& mctx, uint32_t x_a,
                                                  uint32_t xq_a, uint32_t prow) {
  using Gp = Grp<64>;
  constexpr int d = 64;
  const float sd = sqrtf((float)d);
  const float epsd = p.eps * sd;
  const float fd = (float)d;
  const uint32_t ur = (uint32_t)r;
  // ---- draws (asss.py:207, 219, 225, 60)
  const amh_u32x4 o = amh_philox4x32_10((uint32_t)r, (uint32_t)it, 0u, AMH_TAG_ASSS, k0, k1);
  float v = amh_normal_from_bits(o.v[0]);
  float vd = amh_normal_from_bits(Gp::template bcast_u<0>(o.v[1]));
  const float ut = amh_unif01_from_bits(Gp::template bcast_u<0>(o.v[2]));
  const float th0 = 6.28318548f * amh_unif01_from_bits(Gp::template bcast_u<0>(o.v[3]));

  // ---- y = S^-1 (x - mu)
  const float e = dl * sd;
  const float Dr = (dl + p.eps) * sd;
  const float invD = 1.0f / Dr;
  float b = x - mu;
  float y = 0.0f;
  static_for<d>([&](auto J) {
    constexpr int j = J;
    const float yl = b * invD;
    y = s64_keep_at<j>(y, yl);
    const float gj = Gp::template bcast<j>(yl * e);
    b = fmaf(-U[j], gj, b);
    column_fence<j>();
  });

  // ---- stereographic projection (asss.py:40-45)
  const float ns = Gp::sum(y * y);
  const float den = ns + 1.0f;
  const float zr = (2.0f * y) / den;
  const float zd = (ns - 1.0f) / den;

  // ---- v orthogonal to z on S^d (asss.py:219-222), as amh_asss.h
  const float dot = Gp::sum(v * zr) + (vd * zd);
  v = fmaf(-dot, zr, v);
  vd = fmaf(-dot, zd, vd);
  const float nv = sqrtf(Gp::sum(v * v) + (vd * vd));
  const bool degen = !(nv > 0.0f);
  v = degen ? 0.0f : v / nv;
  vd = degen ? 0.0f : vd / nv;

  // ---- S z_1d and S v_1d: U times the broadcast vectors hz, hv from the scratch
  const float Sz = s64_matvec<true>(U, e * zr, x_a, ur) + epsd * zr;
  const float Sv = s64_matvec<true>(U, e * v, x_a, ur) + epsd * v;

  auto x_at = [&](float c, float s, float& om) -> float {
    const float zdt = (zd * c) + (vd * s);
    om = 1.0f - zdt;
    return (((Sz * c) + (Sv * s)) / om) + mu;
  };
  auto pot = [&](float xv) -> float {
    const float u = s64_gauss_pot(xv - mctx.mr, x_a, prow, ur, mctx.c0);
    s64_wait();
    return u;
  };

  // ---- slice level at z (asss.py:216-217, 224-226)
  float om0;
  const float x0 = x_at(1.0f, 0.0f, om0);
  const float U0 = pot(x0);
  const float tpe = (U0 + fd * amh_logf(om0)) - amh_logf(ut);

  // ---- shrinkage (asss.py:59-96)
  float th = th0, thmin = th0 - 6.28318548f, thmax = th0;
  int32_t iter = 0;
  float xt, ux;
  bool cont;
  {
    float s, c, om;
    amh_sincosf(th, &s, &c);
    xt = x_at(c, s, om);
    ux = pot(xt);
    float pt = ux + fd * amh_logf(om);
    if (amh_isnan(pt)) pt = INFINITY;
    cont = !degen && ((pt > tpe) || (om < p.eps));
  }
  while (cont) {  // wave-uniform: one chain per wave
    const float thmin_n = (th < 0.0f) ? th : thmin;
    const float thmax_n = (th >= 0.0f) ? th : thmax;
    const amh_u32x4 ok = amh_philox4x32_10((uint32_t)iter, (uint32_t)it, 1u, AMH_TAG_ASSS, k0, k1);
    const float th_n = thmin_n + (thmax_n - thmin_n) * amh_unif01_from_bits(ok.v[0]);
    float s, c, om;
    amh_sincosf(th_n, &s, &c);
    const float xn = x_at(c, s, om);
    const float un = pot(xn);
    float pt = un + fd * amh_logf(om);
    if (amh_isnan(pt)) pt = INFINITY;
    thmin = thmin_n;
    thmax = thmax_n;
    th = th_n;
    xt = xn;
    ux = un;
    iter += 1;
    cont = (iter < kAsssMaxIter) && ((pt > tpe) || (om < p.eps));
  }
  const bool capped = degen || iter >= kAsssMaxIter;  // asss.py:94: theta = 0
  const float xnew = capped ? x0 : xt;
  float pen = capped ? U0 : ux;
  if (amh_isnan(pen)) pen = INFINITY;  // asss.py:234

  // ---- adaptation (asss.py:237-251)
  const int32_t itr = it + 1;
  const int32_t n = (it < p.W) ? itr : itr - p.W;
  const float gamma = lookup_gamma<64>(p, n);
  const float delta = xnew - mu;
  const float mun = mu + gamma * delta;
  const float dmu = mun - mu;
  const float locd = sqrtf(Gp::sum(dmu * dmu));

  const float sq = sqrtf(1.0f - gamma);
  const float ajj = sq * dl;
  const float Dg = ajj * ajj;
  const float one = (amh_isfinite(ajj) && ajj != 0.0f) ? 1.0f : __int_as_float(0x7FC00000);
  float ws = delta;  // sweep 1: lane r ends with w*_r (s64_sweep1_all)
  s64_sweep1_all(ws, U);
  const S64Coef k = s64_rank_one_coef(ws, Dg, one, gamma, r);
  float sdiff = 0.0f;
  if (!k.revert) {
    sdiff = sqrtf(s64_sweep2<false>(U, delta, ws, k.c, k.q - dl, k.c * k.q, xq_a));
    dl = k.q;
    updated = true;
  }
  asc = locd + sdiff;  // asss.py:248-250
  x = xnew;
  pe = pen;
  mu = mun;
}

// One ARWMH transition (arwmh.py:140-207) on the d = 64 persistent kernel's
// registers: the same float operations in the same order as
// arwmh_step_kernel<64, GaussianM, true> (oracle: orc_step), with the column
// broadcasts read from the wave's LDS scratch or, sg (a single-step launch:
// its own instance of the kernel), the proposal's, the potential's and
// sweep 2's from row-replicated registers.
template <bool sg>
__device__ __forceinline__ void arwmh_transition64(const StepParams& p, float (&U)[64], float& dl, float& z, float& mu,
                                                   float& pe, float& macc, float& lam, float& asc, bool& updated,
                                                   int32_t& nacc, int32_t it, uint32_t k0, uint32_t k1, int r,
                                                   const GaussianM<64>::Ctx& mctx, uint32_t x_a, uint32_t xq_a,
                                                   uint32_t prow AMH_S64_SUB_PARAM) {
  using Gp = Grp<64>;
  AMH_S64_SUB_MARK
  // ---- noise (arwmh.py:162-165, 174): stream position = state.i
  float xi, u;
  step_noise_w64(r, (uint32_t)it, k0, k1, xi, u);  // bit spec: amh_step_word

  AMH_S64_SUB(0)
  // ---- proposal z' = z + (L e^lam + eps I) xi  (arwmh.py:166-167), L xi = U (dl * xi)
  const float el = amh_expf(lam);
  const float eta = dl * xi;
  const float acc = sg ? s64_matvec_rows(U, eta) : s64_matvec(U, eta, x_a, (uint32_t)r);
  const float zp = z + fmaf(el, acc, p.eps * xi);

  AMH_S64_SUB(1)
  // ---- potential (GaussianM<64>::potential with diff_j from the scratch or the rows of diff), NaN -> +inf
  float pep = sg ? s64_gauss_pot_rows(zp - mctx.mr, prow, mctx.c0)
                 : s64_gauss_pot(zp - mctx.mr, x_a, prow, (uint32_t)r, mctx.c0);
  if (amh_isnan(pep)) pep = INFINITY;
  AMH_S64_SUB(2)

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
  const float gamma = lookup_gamma<64>(p, n);
  const float maccn = macc + (alpha - macc) / (float)n;

  // ---- mean and step size (arwmh.py:188-189, 193)
  const float delta = zn - mu;
  const float mun = mu + gamma * delta;
  const float lamn = lam + gamma * (alpha - p.target);
  const float e1 = amh_expf(lamn);

  // ---- rank-one update of sqrt(1-gamma) L by (delta, gamma), NaN -> keep L
  const float sq = sqrtf(1.0f - gamma);
  const float ajj = sq * dl;
  const float Dg = ajj * ajj;
  const float one = (amh_isfinite(ajj) && ajj != 0.0f) ? 1.0f : __int_as_float(0x7FC00000);

  AMH_S64_SUB(3)
  // sweep 1 (lanes r > j): afterwards lane r holds w*_r (forward solve U w* = delta)
  float ws = delta;
  s64_sweep1_all(ws, U);

  const S64Coef k = s64_rank_one_coef(ws, Dg, one, gamma, r);
  AMH_S64_SUB(4)
  if (!k.revert) {
    // sweep 2 with the as_change terms U_rj (q_j e1 - dl_j e0) + (c_j q_j e1) w_r^{(j+1)}
    const float ac = (k.q * e1) - (dl * el);
    const float bc = (k.c * k.q) * e1;
    asc = sqrtf(s64_sweep2<sg>(U, delta, ws, k.c, ac, bc, xq_a));
    dl = k.q;
    updated = true;
  } else {
    // factor unchanged: as_change = || L (e1 - e0) ||_F, L_rj = U_rj dl_j
    const float ac = (dl * e1) - (dl * el);
    float s4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    static_for<64>([&](auto J) {
      const float tt = U[J] * Gp::template bcast<J>(ac);
      s4[J & 3] = fmaf(tt, tt, s4[J & 3]);
      column_fence<J>();
    });
    const float sacc = (s4[0] + s4[1]) + (s4[2] + s4[3]);
    asc = sqrtf(Gp::sum(sacc));
  }

  AMH_S64_SUB(5)
  // ---- commit (arwmh.py:199-207); the caller advances `it`
  z = zn;
  pe = pen;
  macc = maccn;
  mu = mun;
  lam = lamn;
}

// kASSS: the same persistent data movement around one ASSS transition
// (asss_transition, amh_asss.h; asss.py:197-251) instead of the ARWMH one --
// the state is the same but for mean_accept_prob / log_step_size (absent).
// kSG: a single-step ARWMH launch (p.n_steps == 1, run_step64), whose proposal,
// potential and sweep 2 take their vectors from row-replicated registers: an
// instance of its own, so that neither instance carries the other's forms
// behind a branch.
template <int WPB, bool kASSS = false, bool kSG = false>
__global__ __launch_bounds__(WPB * 64) void arwmh_step64_kernel(StepParams p) {
  static_assert(!(kASSS && kSG), "the row-replicated forms are the single-step ARWMH launch's");
  const StepParams& p_outer = p;
  constexpr int D = 64;
  constexpr uint32_t P = kS64P;
  // the swap's statements restore exec to all ones (s64_group_read): the block is whole waves
  static_assert(WPB >= 1 && (WPB * 64) % 64 == 0, "d = 64 step kernel: every wave of the block is full");
  using Gp = Grp<64>;
  using M = GaussianM<64>;
  extern __shared__ float lds[];
  // kSG with a stealable tail: the block re-arms its head word (and its count
  // of stolen chains beside it) to tag << 16.  The exchanges return nothing;
  // the wait for them stands in front of the barrier below, behind the model's
  // staging, so that no wave of the block draws from the head before it.
  if constexpr (kSG) {
    if (threadIdx.x == 0 && p.steal > 0) {
      uint32_t* head = p.heads + (size_t)blockIdx.x * kS64HeadStride;
      const uint32_t armed = (uint32_t)p.tag << 16;
      (void)__hip_atomic_exchange(head, armed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      (void)__hip_atomic_exchange(head + 1, armed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  M::stage(lds, p.model, D);
  float* tick = lds + kS64Model + WPB * kS64WB;
  // The block's ticket counter hands out the block-local chain index: 0, 1,
  // 2, ... in an ascending launch, n - 1, n - 2, ..., 0 in a descending one
  // (n = the block's chain count), so that what one launch wrote last is what
  // the next one reads first and the memory-side cache still holds it
  // (amh_s64_sched.h).  Chains are independent: the order
  // changes no bit.  The four words after the counter's 16 B hold the hot and
  // the tail range for s64_class.
  const int64_t blk_lo = p.C * (int64_t)blockIdx.x / gridDim.x;  // one chain per wave
  const int64_t blk_hi = p.C * ((int64_t)blockIdx.x + 1) / gridDim.x;
  const uint32_t tk_step = p.descending ? ~0u : 1u;
  if (threadIdx.x == 0) {
    const S64Sched sch = s64_sched((uint32_t)(blk_hi - blk_lo), p.descending, p.chained);
    tick[0] = __uint_as_float(sch.first);
    tick[4] = __uint_as_float(sch.hot_lo);
    tick[5] = __uint_as_float(sch.hot_n);
    tick[6] = __uint_as_float(sch.tail_lo);
    tick[7] = __uint_as_float(sch.tail_n);
    if constexpr (kSG) {  // the own part (amh_s64_sched.h), the block's chain count and its tail length
      const uint32_t n = (uint32_t)(blk_hi - blk_lo), T = s64_tail_len(n, (uint32_t)p.steal);
      tick[8] = __uint_as_float(s64_own_lo(T, p.descending));
      tick[9] = __uint_as_float(n - T);
      tick[10] = __uint_as_float(n);
      tick[11] = __uint_as_float(T);
      __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the head is re-armed
    }
  }
  __syncthreads();
  const auto mctx = M::prepare(p.model, D, lane_id());
#ifdef AMH_STAMPS
  // diagnostic build: per-wave start / end on the constant 100 MHz clock and
  // the items taken (tools/s64_tail.py: how long the launch drains)
  const unsigned long long st_start = __builtin_amdgcn_s_memrealtime();
  int st_items = 0;
#endif
  AMH_S64_PHASE_INIT

  const int64_t C = p.C;
  const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64));
  float* wb = lds + kS64Model + wave_in_block * kS64WB;
  const uint32_t wb_a = lds_addr(wb);
  const uint32_t x_a = wb_a + kS64X * 4;            // scratch (64 floats: broadcast vectors)
  const uint32_t zm_a = wb_a + kS64Z * 4;           // z / loc region (swap vectors once read)
  const uint32_t xq_a = x_a + (uint32_t)(lane_id() & 15) * 4u;  // sweep-2 quarter slot
  const uint32_t prow = lds_addr(lds) + (uint32_t)lane_id() * (uint32_t)(M::ld(D) * 4);  // row r of P

  float U[D];  // row r of U = L / diag(L): unit diagonal, zeros above (kept between chains)
  static_for<D>([&](auto J) { U[J] = set_one_at<64, J>(0.0f, lane_id()); });
  float dl = 0.0f, z = 0.0f, mu = 0.0f, pe = 0.0f, macc = 0.0f, lam = 0.0f, asc = 0.0f;
  int32_t it = 0, nacc = 0, acc0 = 0;
  uint32_t k0 = 0, k1 = 0;
  int64_t prev = -1;
  bool prev_upd = false;

  const int64_t kEnd = blk_hi;  // "no item" sentinel
  const uint32_t tk_addr = lds_addr(tick);
  // The draw and its class in lane 0's registers (they die before the
  // readfirstlane): bits 30-31 of the word carry the class, a "no chain" value
  // is clamped below them and stays >= n.  The result is the global chain index
  // with the class at kS64TagShift; kEnd and -1 carry no class.
  // kSG: a draw from the head word of block vb, whose n chains start at lo
  // (amh_s64_sched.h).  The ticket is the add's own return value and the chain
  // it names was written by an earlier launch: no fence.  Everything comes from
  // the kernarg segment and dies here; -1 when the head is exhausted, was armed
  // by another launch or is not armed yet.
  auto head_draw = [&](const StepParams& q, uint32_t vb, int64_t lo, uint32_t n) -> int64_t {
    const uint32_t T = s64_tail_len(n, (uint32_t)q.steal);
    uint32_t old = 0;
    if (lane_id() == 0)
      old = __hip_atomic_fetch_add(q.heads + (size_t)vb * kS64HeadStride, 1u, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    old = (uint32_t)__builtin_amdgcn_readfirstlane((int)old);
    if (!s64_head_valid(old, (uint32_t)q.tag, T)) return -1;
    const S64Sched s = s64_sched(n, q.descending, q.chained);
    const uint32_t v = s64_tail_index(s, n, T, old & 0xFFFFu);
    const uint32_t cls = s64_class(v, s.hot_lo, s.hot_n, s.tail_lo, s.tail_n);
    return (lo + (int64_t)v) | ((int64_t)cls << kS64TagShift);
  };
  // kSG, the LDS counter is spent: the own head, then the heads of blocks
  // b + 8, b + 16, ... (mod the grid), at most kS64StealTries of them.  A wave
  // gets "no item" (-1) only after a failing draw on its own head, and draws no
  // more after that, so a head is exhausted when its block has ended.
  auto tail_ticket = [&]() -> int64_t {
    const StepParams& q = reload_kernarg(p_outer);
    if (q.steal <= 0) return -1;
    uint32_t nn = 0;
    if (lane_id() == 0) {
      asm volatile("ds_read_b32 %0, %1 offset:40\n\ts_waitcnt lgkmcnt(0)" : "=&v"(nn) : "v"(tk_addr) : "memory");
    }
    nn = (uint32_t)__builtin_amdgcn_readfirstlane((int)nn);
    const uint32_t b = blockIdx.x, grid = gridDim.x;
    int64_t t = head_draw(q, b, blk_lo, nn);
    for (uint32_t k = 1; t < 0 && k <= kS64StealTries; ++k) {
      const uint32_t vb = s64_victim(b, grid, k);
      if (vb == grid) break;
      const int64_t lo = q.C * (int64_t)vb / grid, hi = q.C * ((int64_t)vb + 1) / grid;
      t = head_draw(q, vb, lo, (uint32_t)(hi - lo));
      if (t >= 0 && lane_id() == 0)  // for amh_step64_stolen: this block took a chain of another's
        (void)__hip_atomic_fetch_add(q.heads + (size_t)b * kS64HeadStride + 1, 1u, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
    }
    return t;
  };
  auto ticket = [&]() -> int64_t {
    uint32_t v = 0;
    if constexpr (kSG) {
      // the own part from the LDS counter; a value outside it sends the wave to the heads
      if (lane_id() == 0) {
        uint32x4_t_ b;
        uint32_t o_lo, o_n;
        asm volatile("ds_add_rtn_u32 %0, %4, %5\n\tds_read_b128 %1, %4 offset:16\n\tds_read_b32 %2, %4 offset:32\n\t"
                     "ds_read_b32 %3, %4 offset:36\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(v), "=&v"(b), "=&v"(o_lo), "=&v"(o_n) : "v"(tk_addr), "v"(tk_step) : "memory");
        const uint32_t cls = s64_class(v, b[0], b[1], b[2], b[3]);
        v = (v - o_lo < o_n) ? (v | (cls << 30)) : ~0u;
      }
      const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
      if (w == ~0u) return tail_ticket();
      return (blk_lo + (int64_t)(w & 0x3FFFFFFFu)) | ((int64_t)(w >> 30) << kS64TagShift);
    }
    if (lane_id() == 0) {
      uint32x4_t_ b;
      asm volatile("ds_add_rtn_u32 %0, %2, %3\n\tds_read_b128 %1, %2 offset:16\n\ts_waitcnt lgkmcnt(0)"
                   : "=&v"(v), "=&v"(b) : "v"(tk_addr), "v"(tk_step) : "memory");
      const uint32_t cls = s64_class(v, b[0], b[1], b[2], b[3]);
      v = (v < 0x3FFFFFFFu ? v : 0x3FFFFFFFu) | (cls << 30);
    }
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
    return (blk_lo + (int64_t)(w & 0x3FFFFFFFu)) | ((int64_t)(w >> 30) << kS64TagShift);
  };
  auto ix = [](int64_t t) -> int64_t { return t & kS64IdxMask; };
  // is t a chain?  kSG: a ticket may name any block's chain, "no item" is -1
  auto valid = [&](int64_t t) -> bool {
    if constexpr (kSG) return t >= 0;
    else return ix(t) < kEnd;
  };
  // the DMA of a drawn chain, at its class's load policy
  auto prefetch = [&](int64_t t, int ln) {
    s64_load_policy(s64_cls(t), [&](auto AUX) { prefetch_item<64, false, decltype(AUX)::value>(p, ix(t), D, wb, ln); });
  };

  // z, loc and the scalars of chain `c` from registers
  auto store_small = [&](int64_t c, int r) {
    const StepParams& p = reload_kernarg(p_outer);
    p.out.z[c * D + r] = z;
    p.out.loc[c * D + r] = mu;
    if (r == 0) {
      p.out.i[c] = it;
      p.out.potential_energy[c] = pe;
      if constexpr (!kASSS) {
        p.out.mean_accept_prob[c] = macc;
        p.out.log_step_size[c] = lam;
      }
      p.out.as_change[c] = asc;
      p.out.rng_key[2 * c] = k0;
      p.out.rng_key[2 * c + 1] = k1;
      if (!kASSS && p.accept_count != nullptr) p.accept_count[c] = acc0 + nacc;
    }
  };
  // factor of chain `c` copied verbatim from the launch input (no step of this
  // launch updated it); U is used as scratch and reset to the unit pattern
  auto copy_verbatim = [&](int64_t c, int r) {
    const uint32_t vrow = (uint32_t)r * 4u;
    const Buf Lout(uniform_ptr(p.out.scale + c * P), P * 4u);
    const Buf Lin(uniform_ptr(p.in.scale + c * P), P * 4u);
    static_for<4>([&](auto B) {
      static_for<16>([&](auto K) {
        constexpr int j = 16 * B + K;
        U[j] = Lin.ld(off_from<64, j>(vrow, kOOB, r), (uint32_t)(s64_col(j) - j) * 4u);
      });
      static_for<16>([&](auto K) {
        constexpr int j = 16 * B + K;
        Lout.st(U[j], off_from<64, j>(vrow, kOOB, r), (uint32_t)(s64_col(j) - j) * 4u);
      });
      __builtin_amdgcn_sched_barrier(0);
    });
    __builtin_amdgcn_s_waitcnt(0);  // loads landed and store data read before U is reused
    static_for<D>([&](auto J) { U[J] = set_one_at<64, J>(0.0f, r); });
  };
  // the wave buffer's factor region (packed, column-major) -> chain `c` in HBM
  auto flush_aux = [&](int64_t c, auto AUX) {
    const Buf Lout(uniform_ptr(p.out.scale + c * P), P * 4u);
    const uint32_t la = wb_a + (uint32_t)lane_id() * 16u;
    static_for<3>([&](auto G) {  // three dwordx4 per lane in flight per wait
      f32x4 v[3];
      static_for<3>([&](auto Q) { v[(int)Q] = lds_ld4<1024 * (3 * G + Q)>(la); });
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]));
      static_for<3>([&](auto Q) {
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uint32x4_t_, v[(int)Q]), Lout.rs,
                                               (int)(1024u * (3 * G + Q) + 16u * (uint32_t)lane_id()), 0,
                                               (int)AUX);
      });
    });
  };
  // ... for a drawn chain, at its class's store policy
  auto flush_factor = [&](int64_t t) {
    s64_store_policy(s64_cls(t), [&](auto AUX) { flush_aux(ix(t), AUX); });
  };

  // The fused and the ASSS instance draw two items ahead (nxt2 below).  kSG
  // draws one ahead, at the top of the hand-over whose DMA the draw feeds: the
  // waves of a block that is behind then hold no reserved chains, which other
  // blocks can take from its head instead, and the draw is not live across the
  // loop.
  int64_t item = ticket();
  int64_t nxt = kEnd;
  if constexpr (!kSG) nxt = valid(item) ? ticket() : kEnd;
  if (valid(item)) prefetch(item, lane_id());
  for (; valid(item);) {
    int lane = lane_id();
    asm volatile("" : "+v"(lane));
    const int r = lane;
    const uint32_t la = wb_a + (uint32_t)r * 4u;  // this lane's dword in the factor region

    AMH_S64_PHASE_MARK
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): item k has landed
    AMH_S64_PHASE(0)  // (a) the wait for item k
    // the hand-over phase (stores, LDS -> registers, the next DMA) at high
    // wave priority so the memory queue is re-armed before other waves'
    // compute: 239 -> 236 us per launch (tools/gpu_prio.sh A/B)
    __builtin_amdgcn_s_setprio(3);
    // kSG: nothing is outstanding on vector memory here, so a draw from a head
    // word (a global round trip, tail chains only) waits for itself alone
    if constexpr (kSG) nxt = ticket();
    // ---- item k-1's z / loc / scalars leave from registers
    if (prev >= 0) store_small(ix(prev), r);
    const bool wr = prev >= 0 && prev_upd;
    if (prev >= 0 && !prev_upd) copy_verbatim(ix(prev), r);

    // ---- diagonal of item k
    float lnew = lds_ld1<0>(wb_a + (uint32_t)s64_col(r) * 4u);
    s64_tie(lnew);
    const float inv = (amh_isfinite(lnew) && lnew != 0.0f) ? 1.0f / lnew : 0.0f;
    // ---- item k's z / loc / scalars: LDS -> registers
    {
      float zz = lds_ld1<kS64Z * 4>(la), mm = lds_ld1<kS64M * 4>(la);
      const uint32_t sa = wb_a + kS64S * 4;
      float s0 = lds_ld1<0>(sa), s1 = lds_ld1<4>(sa), s2 = lds_ld1<8>(sa), s3 = lds_ld1<12>(sa);
      float s4v = lds_ld1<16>(sa), s5 = lds_ld1<20>(sa), s6 = lds_ld1<24>(sa);
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(zz), "+v"(mm), "+v"(s0), "+v"(s1), "+v"(s2), "+v"(s3), "+v"(s4v),
                   "+v"(s5), "+v"(s6));
      z = zz;
      mu = mm;
      it = __builtin_amdgcn_readfirstlane(__float_as_int(s0));
      pe = s1;
      macc = s2;
      lam = s3;
      asc = s4v;
      k0 = (uint32_t)__builtin_amdgcn_readfirstlane(__float_as_int(s5));
      k1 = (uint32_t)__builtin_amdgcn_readfirstlane(__float_as_int(s6));
      // broadcast vectors [dl of k-1 | 1 / l of k] over item k's z / loc, now in registers
      s64_wr(zm_a + (uint32_t)r * 4u, dl);
      s64_wr_off<256>(zm_a + (uint32_t)r * 4u, inv);
      dl = lnew;
      acc0 = (!kASSS && p.accept_count != nullptr && r == 0) ? p.accept_count[ix(item)] : 0;
    }

    // ---- swap: read item k's column j (lanes > j), write item k-1's column j
    //      of L' = U diag(dl) (lanes >= j) at the same addresses, normalise.
    //      The factor streams out and in while the swap runs: as soon as a
    //      group has finished a piece (s64_piece_after), the piece's 16 B per
    //      lane are read with the next group's [dl | 1/l] quarter-vectors (one
    //      LDS round trip), stored to item k-1 in HBM, and the DMA of the same
    //      piece of item k+1 is issued into the addresses just read.  The wait
    //      at the top of the loop stays the only one on vector memory: every
    //      LDS access from here to there is inline asm.
    const bool have_nxt = valid(nxt);
    const Buf Lnx(uniform_ptr(p.in.scale + ix(nxt) * P), P * 4u);  // (unused without a next item)
    auto piece_in = [&](auto M) {  // DMA of piece M of item k+1, at its class's load policy
      constexpr int m = M;
      if (!have_nxt) return;
      // The piece's LDS address (M0) is one scalar add from the wave buffer's
      // base, made opaque here: nine loop-invariant addresses would otherwise
      // be kept across the loop, spilled to VGPR lanes and read back with
      // v_readlane at every use.
      uint32_t base = wb_a;
      asm volatile("" : "+s"(base));
      lds_void* dst = (lds_void*)(uintptr_t)(base + 1024u * m);
      s64_load_policy(s64_cls(nxt), [&](auto AUX) {
        if constexpr (m < kS64Pieces - 1) {
          __builtin_amdgcn_raw_ptr_buffer_load_lds(Lnx.rs, dst, 16, (int)(16u * lane), 1024 * m, 0, (int)AUX);
        } else {
          if (256 * m + lane < kS64P)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(Lnx.rs, dst, 4, (int)(4u * lane), 1024 * m, 0, (int)AUX);
        }
      });
    };
    const Buf Lout(uniform_ptr(p.out.scale + ix(wr ? prev : item) * P), P * 4u);  // (unused unless wr)
    const int cls = s64_cls(prev);
    const uint32_t la16 = wb_a + (uint32_t)lane * 16u;
    auto piece_out = [&](auto M, const f32x4& v) {  // piece M of L' -> item k-1, at its class's store policy
      constexpr int m = M;
      s64_store_policy(cls, [&](auto AUX) {
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uint32x4_t_, v), Lout.rs,
                                               (int)(16u * (uint32_t)lane), 1024 * m, (int)AUX);
      });
    };
    // One LDS round trip per group: the group's [dl | 1/l] quarter-vectors,
    // the piece the previous group finished and the group's four columns are
    // read together; L' columns are written after the wait and need none.
    // `wr` (is there an L' to write) guards one block per group; without it
    // (the first item, or a factor no step updated, copied verbatim above)
    // the columns are only read and the whole factor's DMA follows the swap.
    static_for<16>([&](auto G4) {
      constexpr int g = G4;
      constexpr int mp = g > 0 ? s64_piece_after(g - 1) : -1;  // the piece the previous group finished
      f32x4 dl4, in4, pv;
      float t[4];  // no initial value: what lanes r <= j hold is never consumed
      s64_group_read<g, mp>(dl4, in4, pv, t, zm_a, la16, la);
      if (wr) {
        if constexpr (mp >= 0) {
          piece_out(std::integral_constant<int, mp>{}, pv);
          piece_in(std::integral_constant<int, mp>{});
          if constexpr (mp == 0) {
            AMH_S64_PHASE(1)  // (b) hand-over start -> first factor store
          }
        }
        s64_group_write<g>(U, la, dl4);
      }
      s64_group_norm<g>(U, in4, t);
    });
    if (wr) {
      constexpr int mp = s64_piece_after(15);  // the tail: 16 B of lanes 0 .. 7 (the store is clipped at P)
      static_assert(mp == kS64Pieces - 1, "the last group finishes the tail");
      f32x4 pv = lds_ld4<1024 * mp>(la16);
      s64_tie(pv);
      piece_out(std::integral_constant<int, mp>{}, pv);
      piece_in(std::integral_constant<int, mp>{});
    } else {
      AMH_S64_PHASE(1)
      s64_wait();
      static_for<kS64Pieces>([&](auto M) { piece_in(M); });
    }

    // ---- z / loc / scalars of item k+1 (their region carried the swap's
    //      vectors until the last group) and the ticket after it
    s64_wait();  // every LDS read of the buffer is done before the DMA refills it
    int64_t nxt2 = kEnd;
    if (have_nxt) {
      prefetch_item_small<64, false>(p, ix(nxt), D, wb, lane);
      if constexpr (!kSG) nxt2 = ticket();
    }
    __builtin_amdgcn_s_setprio(0);
    AMH_S64_PHASE(2)  // (c) -> last DMA issued

    nacc = 0;
    bool updated = false;
    for (int32_t t = 0; t < p.n_steps; ++t) {
      if constexpr (kASSS) {
        asss_transition64(p, U, dl, z, mu, pe, asc, updated, it, k0, k1, r, mctx, x_a, xq_a, prow);
      } else {
        arwmh_transition64<kSG>(p, U, dl, z, mu, pe, macc, lam, asc, updated, nacc, it, k0, k1, r, mctx, x_a, xq_a,
                                prow AMH_S64_SUB_ARG);
      }
      it += 1;
      if (p.col_z != nullptr || p.col_pe != nullptr) {
        if ((t + 1) % p.thinning == 0) {
          const int64_t kk = t / p.thinning;
          if (p.col_z != nullptr) p.col_z[(kk * C + ix(item)) * D + r] = z;
          if (p.col_pe != nullptr && r == 0) p.col_pe[kk * C + ix(item)] = pe;
        }
      }
    }
    prev = item;
    prev_upd = Gp::any(updated);
    item = nxt;
    if constexpr (!kSG) nxt = nxt2;
    AMH_S64_PHASE(3)  // (d) compute
#ifdef AMH_STAMPS
    ++st_items;
#endif
  }
  if (prev >= 0) {
    int lane = lane_id();
    asm volatile("" : "+v"(lane));
    const uint32_t la = wb_a + (uint32_t)lane * 4u;
    store_small(ix(prev), lane);
    if (prev_upd) {
      s64_wr(x_a + (uint32_t)lane * 4u, dl);
      static_for<16>([&](auto G4) {
        constexpr int g = G4;
        f32x4 dl4 = lds_ld4<16 * g>(x_a);
        s64_tie(dl4);
        s64_group_write<g>(U, la, dl4);
      });
      flush_factor(prev);
    } else {
      copy_verbatim(ix(prev), lane);
    }
  }
  __builtin_amdgcn_s_waitcnt(0);
#ifdef AMH_STAMPS
  {
    const unsigned long long st_end = __builtin_amdgcn_s_memrealtime();
    const int64_t w = (int64_t)blockIdx.x * WPB + wave_in_block;
    if (w < kS64StampWaves && lane_id() == 0) {
      unsigned long long* row = g_s64_stamps + w * kS64StampSlots;
      row[0] = st_start;
      row[1] = st_end;
      row[2] = (unsigned long long)st_items;
      row[3] = (unsigned long long)blockIdx.x;
      for (int k_ = 0; k_ < 4; ++k_) row[4 + k_] = st_ph[k_];
      for (int k_ = 0; k_ < kS64SubPhases; ++k_) row[8 + k_] = st_sub.ph[k_];
    }
  }
#endif
}

template <int WPB, bool kASSS = false, bool kSG = false>
hipError_t launch_step64(const StepParams& p, hipStream_t s) {
  constexpr size_t shm = s64_lds_bytes<WPB>();
  static_assert(shm <= 163840, "d = 64 step kernel: LDS budget");
  auto kern = arwmh_step64_kernel<WPB, kASSS, kSG>;
  int per_cu = 0;
  hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, WPB * 64, shm);
  if (e != hipSuccess) return e;
  const int cus = cu_count();
  if (per_cu < 1) per_cu = 1;
  const int64_t need = (p.C + WPB - 1) / WPB;
  int64_t blocks = (int64_t)cus * per_cu;
  if (blocks > need) blocks = need;
  if (blocks < 1) blocks = 1;
  if constexpr (kSG) {
    // a stealable tail needs a head word per block and a tag (amh_capi.hip); without them no tail
    if (p.heads == nullptr || blocks > (int64_t)kS64HeadSlots || p.tag < 1 || p.tag > 0xFFFF || p.steal < 0) {
      StepParams q = p;
      q.steal = 0;
      hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(WPB * 64), shm, s, q);
      return hipGetLastError();
    }
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(WPB * 64), shm, s, p);
  return hipGetLastError();
}

// ARWMH at the d = 64 Gaussian (amh_kernels.hip run_step)
hipError_t run_step64(const StepParams& p, hipStream_t s) {
  return p.n_steps == 1 ? launch_step64<kS64Waves, false, true>(p, s) : launch_step64<kS64Waves>(p, s);
}
// ASSS at the d = 64 Gaussian (amh_asss.hip run_asss_step): the same kernel
// around the ASSS transition.  16 waves (128 VGPRs, 64 B of spill) measured
// 0.343 ms per sample() against 0.363 ms at 12 waves (170 VGPRs, no spill):
// the occupancy pays for the spill
constexpr int kAsss64Waves = 16;
hipError_t run_asss_step64(const StepParams& p, hipStream_t s) {
  return launch_step64<kAsss64Waves, true>(p, s);
}

}  // namespace amh
