// amh_internal.h -- kernel parameter blocks shared by the kernel files and the
// C-ABI layer amh_capi.hip.  Not part of the public ABI (include/amh.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/amh.h"

// the phase-stamp build is a diagnostic build: it also honours the A/B
// environment switches (amh_kernels.hip, amh_capi.hip)
#if defined(AMH_STAMPS) && !defined(AMH_DIAG)
#define AMH_DIAG 1
#endif

namespace amh {

// Learning-rate table size: gamma_n for n < 2^20 is precomputed on the host
// with the same amh_lr_gamma the device would run (bit-identical); larger n
// fall back to the device routine.
constexpr int32_t kGammaTab = 1 << 20;

// compute units of the current device (persistent grids are sized by it)
inline int cu_count() {
  int dev = 0, cus = 0;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  return cus;
}

struct ModelArgs {
  const float* data;  // device, model-specific layout (include/amh.h)
  int64_t n;          // N rows (regression models)
  int64_t k;          // K columns (diamonds, logistic, poisson)
};

struct StepParams {
  amh_state in, out;
  int64_t C;
  int32_t d, W;
  float a, target, eps;
  int32_t n_steps;
  float* col_z;            // [n_keep][C][d] or null
  float* col_pe;           // [n_keep][C] or null
  int32_t* accept_count;   // [C] or null
  int32_t thinning;
  const float* gamma_tab;  // gamma_n = amh_lr_gamma(n, a) for n < gamma_tab_n
  int32_t gamma_tab_n;
  ModelArgs model;
  const float* ext_pe;     // split path: U(z') per chain from the batched potential (n_steps == 1)
  const float* ext_z;      // split path: the proposals z' [C][d] that U(z') was evaluated at
  float* xprop_next;       // split path: the NEXT transition's proposal [C][d] (or null), formed as
                           // the propose pass would form it from the stored state
  int32_t descending;      // d = 64 step kernel: every block walks its chain range from the top (launch-
                           // uniform; the results do not depend on it, amh_capi.hip step64_order)
  int32_t chained;         // ... and its input is what the previous d = 64 launch wrote, in the opposite order:
                           // the launch has a hot part (amh_s64_sched.h)
  uint32_t* heads;         // d = 64 single-step launch: the handle's head words (amh_s64_sched.h: kS64HeadSlots
                           // lines of kS64HeadStride words), or null
  int32_t steal;           // ... its stealable-tail length (0: no tail, the heads are not touched)
  int32_t tag;             // ... and its 16-bit launch tag, 1 ... 65535
};

struct InitParams {
  amh_state out;
  int64_t C, chain_offset;
  int32_t d;
  uint32_t key0, key1;
  const float* init_z;
  ModelArgs model;
};

struct PotParams {
  const float* z;
  float* pe;
  int64_t n;
  int32_t d;
  ModelArgs model;
  const float* xpack = nullptr;  // diamonds, logistic, poisson: the design matrix in MFMA tile order (glm_pack_kernel)
};

struct PnxParams {
  const float* x;
  int64_t n_points, n_samples;
  const float* scale;  // packed shared factor
  float log_step_size, eps;
  int32_t n, d;
  uint32_t key0, key1;
  float* out;
  ModelArgs model;
};

// ASSS.sample_Pnx (amh_asss.hip): frozen shared (loc, scale) for every chain
struct AsssPnxParams {
  const float* x;
  int64_t n_points, n_samples;
  const float* loc;    // shared mu [d]
  const float* scale;  // shared packed factor
  float eps;
  int32_t n, d;
  uint32_t key0, key1;
  float* out;
  ModelArgs model;
};

// pooled covariance (amh_pooled.hip)
constexpr int kPoolWaves = 16;  // waves (of one chain each) per chunk block

// the pooled sums [S_d (d) | S_dd packed (d(d+1)/2) | S_a | N] (amh_pooled_sums_size)
constexpr int64_t pooled_sums_len(int d) { return d + (int64_t)d * (d + 1) / 2 + 2; }
// the d >= 64 update's staging: the factor in the 4-row-aligned layout, then
// ok, gamma, e^lam, e^lam', 4 spare, d column sums (PooledUpdateParams::scratch)
constexpr size_t pooled_factor_floats(int d) { return (size_t)d * (d + 4) / 2; }
constexpr size_t pooled_update_scratch_floats(int d) { return pooled_factor_floats(d) + 8 + (size_t)d; }
// d >= 64 noise drawn ahead: `cap` records (i, key0, key1, u bits), then xi [cap][d]
constexpr size_t kNoiseRecordBytes = sizeof(uint4);
constexpr size_t noise_row_bytes(int d) { return kNoiseRecordBytes + (size_t)d * sizeof(float); }
inline float* noise_xi(float* buf, int64_t cap) { return buf + (kNoiseRecordBytes / sizeof(float)) * cap; }

// chains each wave of a chunk takes (bit spec: fixes the summation order)
__host__ __device__ inline int pooled_cpw(int64_t C) {
  const int64_t c = (C + 4095) / 4096;
  return c < 1 ? 1 : (c > 16 ? 16 : (int)c);
}

// pooled_final_kernel may also form the large-d update's Sigma' (what
// pooled_big_prep_kernel does) when the update follows in the same library
// call with no exchange in between (amh_pooled_step_k, one rank): scratch
// non-null, N = the chain-steps the sums cover
struct FinalPrep {
  const double* cov;
  const int32_t* i;
  float* scratch;
  double N;
  int32_t W, K;
  float a;
};

struct PooledStatsParams {
  int64_t C;
  int32_t d;
  const int32_t* i;
  const float *z, *pe;
  const uint32_t* keys;
  const float *mu, *L, *lam;
  float eps;
  float *z_out, *pe_out;
  double* partials;  // [n_chunks][V]
  ModelArgs model;
  int32_t k_steps;     // d <= 64: transitions per chain with the frozen shared state
  int32_t i_add;       // d > 64: this launch is step i + i_add of the block
  int32_t accumulate;  // d > 64: sums += this launch's sums (steps after the first)
  // d > 64: noise made ahead of time (pooled_big_update_kernel's extra
  // blocks): xi [cap][d] and per-chain records (i, key0, key1, u bits); a
  // chain uses them only if its record matches (i, its key), else it draws
  const float* xi;
  const uint4* xrec;
  int64_t xi_cap;
  FinalPrep prep;  // scratch == nullptr: none
  // d = 64: the chunk partials are left for the update launch to reduce
  // (amh_pooled_step_k on one rank: the update follows with no exchange)
  int32_t defer_reduce;
  // d > 64: the A-operand copies are current (the previous update's post
  // kernel wrote the factor's tiles; the precision's are from the first pack)
  int32_t pack_ready;
  // d <= 64, lane-per-row form: chains each wave of a chunk takes.
  // pooled_cpw(C), or with exact sums pooled_cpw of the chain count of all
  // ranks, so that every rank cuts the same chunks (amh_pooled_stats_k_exact)
  int32_t cpw;
};

// Pool-every-K: the update after a block of K transitions that started at
// shared iteration it counts blocks, n = it / K + 1 (reset at W, W % K == 0);
// K = 1 is arwmh.py:181.
__host__ __device__ inline int32_t pooled_block_n(int32_t it, int32_t W, int32_t K) {
  return (it < W) ? it / K + 1 : (it - W) / K + 1;
}

struct PooledUpdateParams {
  int32_t d, W;
  float a, target;
  const double* sums;
  amh_pooled_state in, out;
  float* scratch;  // d >= 64: pooled_update_scratch_floats(d)
  int32_t K;       // transitions per pooled update (the sums cover K * C chain-steps)
  // d > 64: the next step's noise for chains [0, noise_C) is drawn by the
  // update launch's extra blocks into xi / xrec (PooledStatsParams)
  int64_t noise_C;
  const uint32_t* keys;
  float* xi;
  uint4* xrec;
  // d = 64, red_blocks > 0: the launch first reduces the stats launch's chunk
  // partials into sums_out (== sums; the last reduce block to finish runs
  // the update)
  const float* red_partials;
  int64_t red_chunks;
  int32_t red_accumulate, red_blocks;
  double* sums_out;
  // host-mapped flag (the handle's): set when the d = 64 update's bounded
  // wait on an earlier wave's columns runs out (the factor is then kept);
  // the next library call on the handle reports it (amh_capi.hip)
  int* err_flag;
  // d > 64, one rank (amh_pooled_step_k): pooled_big_post_kernel also writes
  // the new factor's lower tiles in A-operand order here, for the next
  // step's stats launch (its pooled_pack_kernel launch is then skipped)
  float* pack_out;
};
int pooled_reduce64_blocks(int64_t V);  // reduce blocks of the d = 64 partial rows

// sums == nullptr (here, run_pooled_big_stats and run_pooled_ext_stats): the
// chunk partial rows are left unreduced for run_pooled_exact_reduce
hipError_t run_pooled_stats(int model_id, const PooledStatsParams& p, double* sums, hipStream_t s);
// large dimensions (amh_big_pooled.hip): chunks of 256 chains
int64_t pooled_big_chunks(int64_t C, int d);
int64_t pooled_big_pack_floats(int d);  // scratch floats of the fused large-d stats (A-operand tiles)
int64_t pooled_big_tile_V(int d);       // partial row length of the fused large-d stats (d > 64)
int64_t pooled_scratch_rows(int64_t n_chunks);  // partials + group sums of pooled_reduce
// pack: pooled_big_pack_floats(d) floats of scratch (d > 64; unused at d = 64)
hipError_t run_pooled_big_stats(const PooledStatsParams& p, float* pack, double* sums, hipStream_t s);
hipError_t run_pooled_big_update(const PooledUpdateParams& p, hipStream_t s, bool sigma_ready = false);
// chunk partials -> this rank's sums (accumulate: sums += them), d < 64:
// double rows, group sums after the partials (pooled_scratch_rows); d >= 64:
// float32 rows in the tile layout (pooled_big_tile_V)
hipError_t pooled_reduce(const double* partials, int64_t n_chunks, int64_t V, double* sums, int accumulate,
                         hipStream_t s, int tile_d = 0, FinalPrep fp = FinalPrep{});
hipError_t launch_reduce_tiles(const float* partials, int64_t n_chunks, int64_t V, double* sums, int accumulate,
                               int tile_d, const FinalPrep& fp, hipStream_t s);
// The pooled transition split around the caller's potential
// (AMH_MODEL_EXTERNAL; amh_pooled_ext.hip): step t of a block, proposals
// written by the propose pass and read back, with U(zprop), by the stats pass
struct PooledExtParams {
  int64_t C;
  int32_t d;
  const int32_t* i;
  int32_t t;
  const float *z, *pe;
  const uint32_t* keys;
  const float *mu, *L, *lam;
  float eps;
  float* zprop;          // [C][d]
  const float* pe_prop;  // [C] (stats)
  float *z_out, *pe_out; // (stats; may alias z / pe)
  double* partials;      // (stats) chunk partial rows + the reduction's scratch
  int32_t cpw;           // (stats, d < 64) chains per wave of a chunk, as PooledStatsParams::cpw
};
int64_t pooled_ext_chunks(int64_t C, int d, int cpw);
hipError_t run_pooled_ext_propose(const PooledExtParams& p, hipStream_t s);
hipError_t run_pooled_ext_stats(const PooledExtParams& p, double* sums, int accumulate, hipStream_t s);
// exact sums (amh_pooled_exact.hip, amh_exact.h): a rank's chunk partial rows
// (f32_rows: float32 rows in the tile layout of d = tile_d, else double rows
// of the sums' own layout, tile_d = 0) -> acc [V][kExactWords] int64
// (accumulate: acc += them), and the words -> the V doubles of the sums
hipError_t run_pooled_exact_reduce(const void* partials, bool f32_rows, int64_t n_chunks, int64_t Vrow, int tile_d,
                                   int64_t* acc, int accumulate, hipStream_t s);
hipError_t run_pooled_exact_convert(const int64_t* acc, int64_t V, double* sums, hipStream_t s);
hipError_t run_asss_step(int model_id, const StepParams& p, hipStream_t s);  // amh_asss.hip
hipError_t run_asss_step64(const StepParams& p, hipStream_t s);  // amh_step64.hip (d = 64 Gaussian)
hipError_t run_step64(const StepParams& p, hipStream_t s);       // amh_step64.hip (ARWMH, d = 64 Gaussian: run_step)
hipError_t run_asss_pnx(int model_id, const AsssPnxParams& p, hipStream_t s);
// ASSS with the caller's potential (AMH_MODEL_EXTERNAL, d <= 64; amh_asss_ext.hip):
// one transition as begin, shrink rounds 0 .. kAsssMaxIter around the caller's
// U, finish.  A chain's record in the caller's workspace: S z [d], S v [d],
// mu [d] and kAsssExtScalars scalar slots.
constexpr int kAsssExtScalars = 20;
constexpr int64_t asss_ext_work_floats(int d) { return 3 * (int64_t)d + kAsssExtScalars; }
struct AsssExtParams {
  StepParams sp;        // the states, C, d, the schedule and the finish pass's collection slot
  float* cand;          // [2][C][d]: x(theta = 0), then the current candidate
  float* work;          // [C][asss_ext_work_floats(d)]
  int32_t* active;      // [kAsssMaxIter + 1]: chains that continued after each round
  const float* pe;      // (shrink) [2][C]: the caller's U of cand
  int32_t round;        // (shrink)
  // sample_Pnx (frozen = true): the shared adapt state, the chains' points,
  // the run's key and the transition number
  const float *loc, *scale;
  float* x_cur;
  uint32_t key0, key1;
  int32_t t;
};
hipError_t run_asss_ext_begin(const AsssExtParams& q, bool frozen, hipStream_t s);
hipError_t run_asss_ext_shrink(const AsssExtParams& q, hipStream_t s);
hipError_t run_asss_ext_finish(const AsssExtParams& q, bool frozen, hipStream_t s);
// Pooled ASSS with the caller's potential (d <= 64; amh_pooled_asss_ext.hip):
// transition t of a block as begin, the shrink rounds of run_asss_ext_shrink on
// the same record layout, finish (the outcome and the transition's sums,
// `accumulate`: added to the block's)
struct PooledAsssExtParams {
  PooledExtParams sp;  // the shared state, the chains, t; the finish pass's z_out / pe_out / partials / cpw
  float* cand;         // [2][C][d]: x(theta = 0), then the current candidate
  float* work;         // [C][asss_ext_work_floats(d)]
};
hipError_t run_pooled_asss_ext_begin(const PooledAsssExtParams& q, hipStream_t s);
hipError_t run_pooled_asss_ext_finish(const PooledAsssExtParams& q, double* sums, int accumulate, hipStream_t s);
// evaluation metrics (amh_eval.hip)
int64_t kernel_sum_blocks(int64_t n, int64_t m);
hipError_t run_kernel_sum(const float* A, int64_t n, const float* B, int64_t m, int d, float gamma, int skip_diag,
                          double* partials, double* out, hipStream_t s);
hipError_t run_dist2(const float* A, int64_t n, const float* B, int64_t m, int d, float* out, hipStream_t s);
hipError_t run_normals(uint32_t k0, uint32_t k1, int64_t n, float* out, hipStream_t s);
// linear assignment by auction (amh_assign.hip); the work buffer opens with
// kAssignHdrWords int64 words: cmax bits, refusal flag, e, qmax, rounds run,
// the two list counts, one spare
constexpr int kAssignHdrWords = 8;
constexpr int64_t kAssignMaxN = 65536;
int64_t assign_work_bytes(int64_t n);
hipError_t run_assign_begin(const float* cost, int64_t n, void* work, hipStream_t s);
hipError_t run_assign_phase(void* work, int64_t n, hipStream_t s);
// `rounds` rounds (bid, claim, award) over at most `bound` unassigned persons,
// `first` rounds having been queued since run_assign_phase
hipError_t run_assign_rounds(const float* cost, int64_t n, void* work, int64_t eps, int64_t bound, int64_t first,
                             int32_t rounds, hipStream_t s);
// the header to host memory; waits for the stream
hipError_t run_assign_header(const void* work, int64_t* host8, hipStream_t s);
hipError_t run_assign_result(const void* work, int64_t n, int64_t* perm, int64_t* price, hipStream_t s);
// streaming summaries (amh_summary.hip): folds x [B][C][k] into acc [5][C][k]
// and hist [k][nbins + 3]; calib [3][k] = center, lo, inv_w
hipError_t run_summary_update(const float* x, int64_t B, int64_t C, int k, const float* calib, int nbins,
                              int64_t batch, int64_t n_before, double* acc, int64_t* hist, hipStream_t s);
// asss: the pooled ASSS update (log_step_size copied through, as_change of asss.py:259-260)
hipError_t run_pooled_update(const PooledUpdateParams& p, hipStream_t s, bool asss = false);
// pooled ASSS (amh_pooled_asss.hip): the slice transition against the shared
// factor, d <= 64, registry models; p.lam is not read
bool pooled_asss_model(int model_id, int d);
hipError_t run_pooled_asss_stats(int model_id, const PooledStatsParams& p, double* sums, hipStream_t s);

hipError_t run_step(int model_id, const StepParams& p, hipStream_t s);
hipError_t run_lse_rows(const float* Cm, int64_t rows, int64_t cols, const float* pot, float logw, float eps,
                        float* out, hipStream_t s);
hipError_t run_init(int model_id, const InitParams& p, hipStream_t s);
hipError_t run_potential(int model_id, const PotParams& p, hipStream_t s);
hipError_t run_pnx(int model_id, const PnxParams& p, hipStream_t s);
// sample_Pnx with the caller's potential (AMH_MODEL_EXTERNAL, d <= 64): one
// step t of every chain in two launches around the caller's U
struct PnxExtParams {
  float* z;              // [C][d] current points (accept: updated)
  float* pe;             // [C] their U (accept: updated)
  float* zprop;          // [C][d] proposals (propose: written)
  const float* pe_prop;  // [C] U(zprop) (accept)
  int64_t C;
  const float* scale;    // shared packed factor
  float log_step_size, eps;
  int32_t t, d;
  uint32_t key0, key1;
};
hipError_t run_pnx_ext(const PnxExtParams& p, bool accept, hipStream_t s);
// large dimensions (64 < d <= 256, Gaussian; amh_big.hip)
struct BigParams {
  amh_state in, out;
  int64_t C;
  int32_t d, W;
  float a, target, eps;
  const float* gamma_tab;
  int32_t gamma_tab_n;
  float *xprop, *wa, *wr;  // propose -> step scratch [C][d]
  float* dg;               // the factor's diagonal [C][d] (propose / step<NEXT> -> step)
  const float* pep;        // U(z') [C]
  int32_t* accept_count;   // [C] or null
  float* col_z;            // this step's collection slot [C][d] or null
  float* col_pe;           // [C] or null
};
bool big_model(int model_id, int d);
bool pooled_big_model(int model_id, int d);
hipError_t run_big_init(const InitParams& p, hipStream_t s);
hipError_t run_big_propose(const BigParams& p, hipStream_t s);
// next: also form the next transition's proposal and solves (multi-step launches)
hipError_t run_big_step(const BigParams& p, hipStream_t s, bool next = false);
hipError_t run_big_potential(const PotParams& p, hipStream_t s);
// ASSS for the large-d Gaussian (big_model): one transition per launch; the
// frozen kernel of sample_Pnx
hipError_t run_asss_big_step(const StepParams& p, hipStream_t s);
// ARWMH.sample_Pnx for the large-d Gaussian (big_model)
hipError_t run_big_pnx(const PnxParams& p, hipStream_t s);
hipError_t run_asss_big_pnx(const AsssPnxParams& p, hipStream_t s);

// split path for data-heavy models (diamonds): proposal kernel, lane-per-chain
// batched potential, then the step kernel reading U(z') (amh_split.hip)
bool split_model(int model_id, int d);
constexpr int kDiaMfmaKc = 24;  // diamonds on MFMA: the reference data set's Kc (amh_split.hip)
// the MFMA potentials' tile copy of X and the per-row side vectors (diamonds: Y;
// logistic: y; Poisson: y and the offset), for diamonds at Kc = kDiaMfmaKc and
// the two regressions at any 1 <= K <= 31 (amh_split.hip)
int64_t model_pack_floats(int model_id, int64_t N, int64_t K);  // 0: no MFMA path for this model or shape
hipError_t run_model_pack(int model_id, const ModelArgs& m, float* xp, hipStream_t s);
// the reference diamonds data (K = 25 columns): d = 26, compiled as a fixed
// dimension on the split path
constexpr int kDiamondsD = 26;
hipError_t run_propose(const StepParams& p, float* xprop, hipStream_t s);
hipError_t run_step_ext(const StepParams& p, hipStream_t s);
hipError_t run_init_nopot(const InitParams& p, hipStream_t s);
hipError_t run_potential_lane(int model_id, const PotParams& p, hipStream_t s);
hipError_t run_chain_keys(uint32_t k0, uint32_t k1, int64_t offset, int64_t n, uint32_t* out,
                          hipStream_t s);
#ifdef AMH_STAMPS
hipError_t diag_stamps_copy(void* host, size_t bytes);
hipError_t diag_s64_stamps_copy(void* host, size_t bytes);
hipError_t diag_upd_stamps_copy(void* host);
hipError_t diag_f64_stamps_copy(void* host);
hipError_t diag_u64_timeline_copy(void* host);
#endif

}  // namespace amh
