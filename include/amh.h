/*
 * amh.h -- C ABI of libamh.so, the MI355X (gfx950) adaptive random-walk
 * Metropolis-Hastings engine.
 *
 * The reference (savelovme/adaptive-mcmc) has no FFI: its boundary is the
 * NumPyro MCMCKernel object python/kernels/arwmh.py:31.  Each entry point
 * below replaces one method of that object for a whole batch of chains; the
 * Python mirror (adaptive-mcmc_amd/kernels_amd/arwmh.py, _lib.py) binds them with ctypes.
 *
 *   amh_create / amh_bind_model   ARWMH.__init__        arwmh.py:43-78
 *                                 + model plug-in        arwmh.py:109-116
 *   amh_init                      ARWMH.init            arwmh.py:84-138
 *   amh_step                      ARWMH.sample          arwmh.py:140-207
 *                                 (n_steps > 1: numpyro fori_collect over
 *                                 sample, kernel_utils.py:29-33)
 *   amh_potential                 potential_fn          arwmh.py:121,170
 *   amh_sample_pnx                ARWMH.sample_Pnx      arwmh.py:230-270
 *   amh_pooled_*                  build-defined pooled-covariance mode
 *                                 (SURVEY.md §8(e)); ARWMH.sample's
 *                                 adaptation (arwmh.py:180-197) driven by
 *                                 the statistics of all chains
 *
 * Conventions
 *   - Every pointer in amh_state / model data / outputs is a DEVICE pointer
 *     owned by the caller (PyTorch allocates them).  The library never frees
 *     caller memory.
 *   - Layout is chain-major: z/loc [C][d], scale [C][d(d+1)/2] (lower
 *     triangle packed column by column: column j holds rows j..d-1),
 *     scalars [C], rng_key [C][2] uint32.
 *   - All work is enqueued on `stream` (a hipStream_t; NULL = default
 *     stream).  No call synchronises the device (amh_destroy's hipFree
 *     calls wait for outstanding device work as HIP defines).
 *   - Return value: 0 on success, a negative AMH_E* code on failure;
 *     amh_last_error(h) describes the failure (thread-local when h is NULL).
 *   - One handle per device; handles are not shared between host threads.
 */
#ifndef AMH_H
#define AMH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AMH_ABI_VERSION 1

enum {
  AMH_OK = 0,
  AMH_EINVAL = -1,   /* bad argument (shape, pointer, unsupported d)     */
  AMH_ENOMODEL = -2, /* amh_step/amh_init before amh_bind_model          */
  AMH_EHIP = -3,     /* HIP runtime error (message in amh_last_error)    */
  AMH_ENOMEM = -4
};

/* Model plug-in registry (PosteriorDB models of the reference + Gaussian). */
enum {
  AMH_MODEL_GAUSSIAN = 1,      /* data: [m (d) | P (d*d) | c0]; U = .5 (x-m)'P(x-m) + c0   */
  AMH_MODEL_EIGHT_SCHOOLS = 2, /* data: [y (J) | sigma (J) | log sigma (J)], d = J + 2     */
  AMH_MODEL_KIDIQ = 3,         /* data: [kid (N) | mom_hs (N) | mom_iq (N)], d = 4          */
  AMH_MODEL_DIAMONDS = 4,      /* data: [Xc (N*Kc) | Y (N)], d = Kc + 2, Kc = K - 1        */
  AMH_MODEL_DIAMONDS_SS = 5,   /* diamonds through float64 sufficient statistics, passed as
                                  2 floats each: [N, ybar, A, sT, t (Kc), sx (Kc), Gm (Kc*Kc)],
                                  n_data = 2 (4 + 2 Kc + Kc^2), iparams {N, K}, 3 <= d <= 32 */
  AMH_MODEL_MIXTURE = 6,       /* K-component univariate normal mixture on every coordinate
                                  (asumptions_check.ipynb cells 61-62): data [c (K) | m (K) |
                                  s (K)], c_k = log w_k - log(sqrt(2 pi) s_k); iparams {K},
                                  1 <= K <= 8, n_data = 3 K, 1 <= d <= 16 */
  AMH_MODEL_EXTERNAL = 7,      /* the caller's potential (arwmh.py:69-70 potential_fn, any
                                  callable): the library never evaluates U; amh_init leaves
                                  pe0 = 0 for the caller to fill, transitions run through
                                  amh_propose / amh_step_external; data ignored (non-null,
                                  n_data >= 0, no iparams), 1 <= d <= 256 */
  AMH_MODEL_LOGISTIC = 8,      /* Bayesian logistic regression on the caller's data (no
                                  counterpart in the reference): y_n ~ Bernoulli(logit^-1(I +
                                  X_n b)), I ~ N(0, s_I), b_k ~ N(0, s_b).  z = [Intercept,
                                  b_0 .. b_{K-1}] (unconstrained = constrained), d = K + 1,
                                  1 <= K <= 31, N >= 1; iparams {N, K}; data [X (N*K,
                                  row-major) | y (N, 0.0 or 1.0) | iI2, ib2, c0], n_data =
                                  N K + N + 3, iI2 = 1 / s_I^2, ib2 = 1 / s_b^2, c0 =
                                  log(s_I sqrt(2 pi)) + K log(s_b sqrt(2 pi)) (host, float64,
                                  then rounded).  Bit spec (explicit fmaf and amh_math.h only):
                                    m_n   = fmaf(X[n][k], b_k, m) from m = 0, k ascending
                                    eta_n = I + m_n
                                    t_n   = (fmaxf(eta_n, 0) + amh_log1pf(amh_expf(-|eta_n|)))
                                            - y_n * eta_n
                                    part[n mod 32] = part[n mod 32] + t_n, from 0, in row order
                                    S = the 32-lane xor butterfly of part (offsets 1, 2, 4, 8, 16)
                                    B = the same butterfly of x_r^2 over r = 1 .. K (0 elsewhere)
                                    U = ((S + (0.5 B) ib2) + (0.5 (I I)) iI2) + c0
                                  every kernel runs it at lane-group width 32 (the pooled
                                  ARWMH kernels at 64 with +0 in the upper half, same bits);
                                  amh_step / amh_init / amh_potential evaluate it on MFMA
                                  from a tile copy made by amh_bind_model.  Not accepted by
                                  amh_pooled_asss_* (AMH_EINVAL). */
  AMH_MODEL_POISSON = 9        /* Bayesian Poisson regression with log link on the caller's
                                  data (no counterpart in the reference): y_n ~ Poisson(exp(I
                                  + X_n b + o_n)), I ~ N(0, s_I), b_k ~ N(0, s_b), o the
                                  per-row offset (log exposure).  z = [Intercept, b_0 ..
                                  b_{K-1}] (unconstrained = constrained), d = K + 1, 1 <= K
                                  <= 31, N >= 1; iparams {N, K}; data [X (N*K, row-major) |
                                  y (N) | o (N) | iI2, ib2, c0], n_data = N K + 2 N + 3; y
                                  non-negative integers that float32 holds exactly (y <=
                                  2^24), o all +0 without an offset; iI2 = 1 / s_I^2, ib2 =
                                  1 / s_b^2, c0 = log(s_I sqrt(2 pi)) + K log(s_b sqrt(2 pi))
                                  + sum_n lgamma(y_n + 1), so that U is the full -log joint
                                  (host, float64, then rounded once).  Bit spec (explicit
                                  fmaf and amh_math.h only, no contraction):
                                    m_n   = fmaf(X[n][k], b_k, m) from m = +0, k ascending
                                    eta_n = (I + m_n) + o_n
                                    t_n   = amh_expf(eta_n) - (y_n * eta_n)   (the product is
                                            rounded, then the difference)
                                    part[n mod 32] = part[n mod 32] + t_n, from 0, in row order
                                    S = the 32-lane xor butterfly of part (offsets 1, 2, 4, 8, 16)
                                    B = the same butterfly of x_r^2 over r = 1 .. K (0 elsewhere)
                                    U = ((S + (0.5 B) ib2) + (0.5 (I I)) iI2) + c0
                                  A NaN U is +inf to every accept or slice test (the
                                  kernels' rule); an overflowing amh_expf gives U = +inf,
                                  which rejects: there is no guard.  Every kernel runs it at
                                  lane-group width 32 (the pooled kernels at 64 with +0 in
                                  the upper half, same bits); amh_step / amh_init /
                                  amh_potential evaluate it on MFMA from a tile copy made by
                                  amh_bind_model.  Accepted by amh_pooled_asss_*. */
};

typedef struct amh_config {
  int32_t dim;                /* d, flat unconstrained dimension: 1..64 for
                                 every model (each within its own range in
                                 the registry above: logistic and poisson 2..32,
                                 ...);
                                 64 < d <= 256 for the dense
                                 Gaussian (regime A, sample_Pnx and ASSS; the
                                 pooled mode needs d % 32 == 0) */
  int32_t num_warmup;         /* W (ARWMH.init's num_warmup)                 */
  float lr_decay;             /* a: gamma_n = 1 / n^a          (default 2/3) */
  float target_accept_prob;   /*                               (default .234)*/
  float eps;                  /* eps added to the scaled factor (default 1e-6)*/
  int32_t reserved[3];
} amh_config;

typedef struct amh_state {
  int32_t* i;                 /* [C]      iteration                          */
  float* z;                   /* [C][d]   current point (unconstrained)      */
  float* potential_energy;    /* [C]                                          */
  float* mean_accept_prob;    /* [C]                                          */
  float* loc;                 /* [C][d]   adapt_state.loc                    */
  float* scale;               /* [C][P]   adapt_state.scale, packed lower    */
  float* log_step_size;       /* [C]      adapt_state.log_step_size          */
  float* as_change;           /* [C]                                          */
  uint32_t* rng_key;          /* [C][2]   per-chain Philox key               */
} amh_state;

/* Optional per-launch collection (numpyro fori_collect / extra_fields). */
typedef struct amh_collect {
  float* z;                   /* [n_keep][C][d] or NULL                      */
  float* potential_energy;    /* [n_keep][C] or NULL                         */
  int32_t* accept_count;      /* [C] incremented per accepted step, or NULL  */
  int32_t thinning;           /* keep every `thinning`-th step (>= 1)        */
} amh_collect;

typedef struct amh_handle amh_handle;

int amh_version(void);
const char* amh_last_error(const amh_handle* h);

/* arwmh.py:43-78 (constructor config). */
int amh_create(const amh_config* cfg, int device, amh_handle** out);
int amh_destroy(amh_handle* h);

/* A device-side failure flagged by a completed launch of this handle (the
 * d = 64 pooled update's bounded wait running out: that update kept the shared
 * factor, so the run no longer follows the bit spec).  Returns AMH_EHIP with
 * the message in amh_last_error and clears the flag, else AMH_OK.  Reads a
 * host-mapped word, no synchronisation: a launch still in flight is covered
 * by a call after the caller has synchronised its stream (amh_destroy reads
 * the flag as it stands, without synchronising, and returns the same code
 * when it is set).  No counterpart in the reference,
 * whose guards (arwmh.py:171, :191) cannot fail this way. */
int amh_check_device(amh_handle* h);

/* The chain order of the handle's last d = 64 Gaussian step launch (amh_step,
 * amh_step_chained, amh_asss_step): *order = 0 when every block walked its
 * chains ascending, 1 when descending, -1 when the handle has launched none
 * yet.  A launch whose input factor buffer (in->scale) and chain count are
 * those the previous such launch wrote runs in the opposite order, so that it
 * first reads what that launch wrote last (still held by the memory-side
 * cache); any other launch runs ascending.  The order changes no result; this
 * entry only makes the choice observable.  No counterpart in the reference. */
int amh_step_order(amh_handle* h, int32_t* order);

/* The schedule the d = 64 step kernel gives a block of n chains (host only, no
 * device needed): index[k] is the block-local chain drawn k-th, 0 ... n - 1
 * ascending or n - 1 ... 0 when descending is non-zero, and cls[k] its place
 * class in a launch chained to an oppositely ordered previous launch: bit 0
 * "hot", one of the first floor(3 n / 8) draws (what the previous launch drew
 * last, so likely still in the memory-side cache), bit 1 "tail", one of the
 * last floor(3 n / 8) draws (what the next launch draws first).  The class only
 * picks the cache policy of the chain's factor traffic; an unchained launch has
 * the same order and tail and no hot part.  Both arrays hold n entries.  No
 * counterpart in the reference. */
int amh_step64_schedule(int32_t n, int32_t descending, int32_t* index, int32_t* cls);

/* The same schedule with a stealable tail of `steal` chains, as a single-step
 * d = 64 launch (amh_step with n_steps = 1) runs it (host only).  The draw
 * order is that of amh_step64_schedule; its first *n_own = n - T draws, T =
 * min(n, steal, 32768), come from the block's own counter, the last T from the
 * block's head word in device memory, from which blocks that have run out of
 * work may draw too.  index and cls hold n entries, the own part first.
 * victims receives the blocks whose head words block `block` of a grid of
 * `grid` visits, in order, once its own is exhausted: at most
 * AMH_S64_STEAL_TRIES entries, *n_victims of them, never `block` itself.  No
 * counterpart in the reference. */
#define AMH_S64_STEAL_TRIES 4
int amh_step64_steal_schedule(int32_t n, int32_t descending, int32_t steal, int32_t block, int32_t grid,
                              int32_t* n_own, int32_t* index, int32_t* cls, int32_t* victims, int32_t* n_victims);

/* The stealable-tail length of the handle's single-step d = 64 launches, 0 ...
 * 65535: 0 is the schedule without a tail (no block takes another's chains).
 * It changes which block computes a chain and no result.  A handle's launches
 * must be ordered on the device (one stream, or streams ordered by events): the
 * head words are the handle's.  No counterpart in the reference. */
int amh_step64_set_steal(amh_handle* h, int32_t steal);

/* *stolen = the chains of the handle's last single-step d = 64 launch that a
 * block took from another block's tail.  Synchronises `stream`, on which that
 * launch was enqueued.  A measurement aid. */
int amh_step64_stolen(amh_handle* h, int64_t* stolen, void* stream);

/* Model plug-in (arwmh.py:109-116 / the scripts' numpyro models).
 * data: device pointer, n_data floats; iparams model-specific:
 *   GAUSSIAN: none.  EIGHT_SCHOOLS: {J}.  KIDIQ: {N}.  DIAMONDS: {N, K}.
 *   LOGISTIC: {N, K}.  POISSON: {N, K}. */
int amh_bind_model(amh_handle* h, int32_t model_id, const float* data, int64_t n_data,
                   const int64_t* iparams, int32_t n_iparams);

/* arwmh.py:84-138 for chains [chain_offset, chain_offset + C) of the run
 * keyed by key[2] (host memory).  init_z: device [C][d] starting points, or
 * NULL for init_to_uniform (U(-2, 2) per coordinate).  Writes *out. */
int amh_init(amh_handle* h, const uint32_t key[2], int64_t chain_offset, int64_t num_chains,
             const float* init_z, const amh_state* out, void* stream);

/* arwmh.py:140-207 applied n_steps times to every chain.  `in` and `out` may
 * alias (in-place update).  collect may be NULL. */
int amh_step(amh_handle* h, int64_t num_chains, const amh_state* in, const amh_state* out,
             int32_t n_steps, const amh_collect* collect, void* stream);

/* amh_step with flags (64 < d <= 256 and the split transition of the literal
 * diamonds model, of logistic and of Poisson regression; other shapes ignore them).  The step pass of those paths forms
 * the next transition's proposal while it streams L' out (so the factor is
 * read once per transition); AMH_STEP_KEEP_PROPOSAL keeps the one after the last step in
 * the handle, and AMH_STEP_PROPOSAL_READY tells the next call that its `in` is
 * that unchanged output (same chains), so its propose pass is skipped.  The
 * handle drops a kept proposal whenever its scratch is used otherwise, and
 * READY without one falls back to the propose pass.  Same bits either way. */
enum { AMH_STEP_PROPOSAL_READY = 1, AMH_STEP_KEEP_PROPOSAL = 2 };
int amh_step_chained(amh_handle* h, int64_t num_chains, const amh_state* in, const amh_state* out,
                     int32_t n_steps, const amh_collect* collect, int32_t flags, void* stream);

/* AMH_MODEL_EXTERNAL: ARWMH.sample (arwmh.py:140-207) with U evaluated by the
 * caller between two launches.  amh_propose writes every chain's proposal
 * z' = z + (L e^lam + eps I) xi (arwmh.py:162-167, the step stream at in.i)
 * to zprop[C][d].  amh_step_external then runs the rest of the transition
 * (accept with pe_prop[C] = U(zprop), NaN -> +inf as arwmh.py:171; the
 * schedule, mean, rank-one update and step size) from `in` to `out`; with
 * zprop_next non-null it also writes the NEXT transition's proposals (from
 * `out`, in the same pass over the factor; zprop_next may equal zprop), so a
 * chain of transitions is propose once, then {U; step_external}.  collect:
 * z / potential_energy after the transition (thinning 1) and accept_count.
 * `in` and `out` may alias.  Same bits as the fused kernels with the same U.
 * d > 64: the solves of the proposals stay in the handle, so amh_step_external
 * takes only the state the last amh_propose / amh_step_external formed them
 * from, and zprop_next must be null or zprop (AMH_EINVAL otherwise). */
int amh_propose(amh_handle* h, int64_t num_chains, const amh_state* in, float* zprop, void* stream);
int amh_step_external(amh_handle* h, int64_t num_chains, const amh_state* in, const amh_state* out,
                      const float* zprop, const float* pe_prop, float* zprop_next, const amh_collect* collect,
                      void* stream);

/* ARWMH.sample_Pnx (arwmh.py:230-270) with AMH_MODEL_EXTERNAL, d <= 64: step
 * t of every chain c (key split(key)[c], as amh_sample_pnx) in two calls
 * around the caller's U.  The caller starts z[C][d] at the points (chain
 * p * n_samples + s at x[p]) and pe[C] = U(z); per step t = 0..n-1:
 * amh_pnx_propose writes zprop from z and the shared (scale_packed,
 * log_step_size), the caller evaluates pe_prop = U(zprop), amh_pnx_accept
 * moves accepted chains (u < min(1, exp(pe - pe_prop)), NaN -> +inf) into z,
 * pe.  Same bits as amh_sample_pnx given the same U. */
int amh_pnx_propose(amh_handle* h, const uint32_t key[2], const float* z, int64_t num_chains,
                    const float* scale_packed, float log_step_size, int32_t t, float* zprop, void* stream);
int amh_pnx_accept(amh_handle* h, const uint32_t key[2], float* z, float* pe, int64_t num_chains,
                   const float* zprop, const float* pe_prop, int32_t t, void* stream);

/* potential_fn(z) for n points: pe[n] from z[n][d] (arwmh.py:121). */
int amh_potential(amh_handle* h, const float* z, float* pe, int64_t n, void* stream);

/* arwmh.py:230-270.  x: device [n_points][d]; adapt state (loc[d],
 * scale_packed[P], log_step_size) shared by every chain; out: device
 * [n_points][n_samples][d].  key[2] in host memory. */
int amh_sample_pnx(amh_handle* h, const uint32_t key[2], const float* x, int64_t n_points,
                   int64_t n_samples, const float* loc, const float* scale_packed,
                   float log_step_size, int32_t n, float* out, void* stream);

/* Per-chain key derivation used by amh_init (device out[n][2]); exposed so
 * callers can reproduce chain streams. */
int amh_chain_keys(const uint32_t key[2], int64_t chain_offset, int64_t n, uint32_t* out,
                   void* stream);

/* ------------------------------------------------------------------ ASSS ----
 * asss.py:197-251 (ASSS.sample) applied n_steps times to every chain: the
 * adaptive stereographic slice sampler with the same adaptation as ARWMH
 * (mean, rank-one Cholesky update, NaN -> keep L) and as_change =
 * ||mu' - mu|| + ||L' - L||_F.  Uses i, z, potential_energy, loc, scale,
 * as_change and rng_key of the states (mean_accept_prob / log_step_size are
 * not read or written and may be NULL).  Initial states come from amh_init
 * (asss.py:134-189 equals arwmh.py:84-138 on these leaves).  d <= 64.
 * `in` and `out` may alias.  collect: as amh_step (z / potential_energy). */
int amh_asss_step(amh_handle* h, int64_t num_chains, const amh_state* in, const amh_state* out,
                  int32_t n_steps, const amh_collect* collect, void* stream);

/* asss.py:271-303 (ASSS.sample_Pnx): n transitions with the frozen shared
 * adapt state (loc[d], scale_packed[P]) from every x[pt] for n_samples chains
 * each; out: device [n_points][n_samples][d].  Chain keys as amh_sample_pnx;
 * transition t draws at stream position t.  key[2] in host memory. */
int amh_asss_sample_pnx(amh_handle* h, const uint32_t key[2], const float* x, int64_t n_points,
                        int64_t n_samples, const float* loc, const float* scale_packed, int32_t n,
                        float* out, void* stream);

/* ------------------------------------------ ASSS, the caller's potential ----
 * AMH_MODEL_EXTERNAL (any other model: AMH_EINVAL), d <= 64: ASSS.sample
 * (asss.py:197-251) with U evaluated by the caller.  The transition evaluates
 * U only on its slice circle -- at theta = 0 (asss.py:216-217) and at every
 * candidate of the shrinkage (asss.py:59-96) -- so it is cut there:
 *   amh_asss_ext_begin    the draws at stream position in.i (asss.py:207,
 *                         219, 225), y = S^-1 (x - mu) and its projection
 *                         (asss.py:40-45, 214), the tangent (asss.py:219-222)
 *                         and the circle through S; writes cand[0][c] =
 *                         x(theta = 0), cand[1][c] = the first candidate
 *                         x(theta_0) (cand: device [2][C][d]), every chain's
 *                         record in work (device, C times
 *                         amh_asss_ext_work_size floats) and zeroes active
 *                         (device, AMH_ASSS_EXT_ROUNDS int32)
 *   the caller            pe[0][c] = U(cand[0][c]), pe[1][c] = U(cand[1][c])
 *                         (pe: device [2][C])
 *   amh_asss_ext_shrink   round 0: the slice level t = (U(x(0)) + d log(1 -
 *                         z_d)) - log u (asss.py:224-226) from pe[0], and the
 *                         test of the first candidate (asss.py:72-76, NaN ->
 *                         +inf).  A chain whose candidate is off the slice
 *                         (and whose tangent is not degenerate) narrows its
 *                         bracket (asss.py:78-92), draws Philox(round, i, 1),
 *                         writes the next candidate over cand[1][c] and adds 1
 *                         to active[round].
 *   while active[round] > 0 (the caller reads it: one synchronisation per
 *   round): round += 1, the caller's pe[1][c] = U(cand[1][c]) for every c,
 *   amh_asss_ext_shrink(round).  Round r >= 1 tests candidate r with pe[1]
 *   alone; round 50 stops every chain (asss.py:59 max_iterations), so
 *   active[50] stays 0 and the loop ends after at most AMH_ASSS_EXT_ROUNDS
 *   evaluations of cand[1].
 *   amh_asss_ext_finish   the outcome (theta = 0 for a chain that hit the cap
 *                         or whose tangent was degenerate, asss.py:94; its
 *                         energy NaN -> +inf, asss.py:234), the adaptation
 *                         (asss.py:237-251) and the state to `out` (may alias
 *                         `in`); collect: z / potential_energy after the
 *                         transition (thinning 1), as amh_step_external.
 * A chain that has stopped is not touched by later rounds: cand[1][c] keeps
 * its accepted point and the record keeps the pe[1][c] of the round that
 * accepted it; what the caller returns for that row in later rounds is
 * ignored, so a potential that is not bit-reproducible from call to call
 * cannot change a stored energy.  Given the same U the bits are those of
 * amh_asss_step with n_steps = 1.
 * Contract: amh_asss_ext_finish takes the state amh_asss_ext_begin read,
 * unmodified, with the cand / work that begin and the shrink rounds wrote for
 * it (same num_chains).  Nothing is kept in the handle, so the library cannot
 * check this; a caller that breaks it gets wrong numbers, not a fault (every
 * index is formed from num_chains and d alone). */
#define AMH_ASSS_EXT_ROUNDS 51
int amh_asss_ext_work_size(int32_t dim, int64_t* floats_per_chain);
int amh_asss_ext_begin(amh_handle* h, int64_t num_chains, const amh_state* in, float* cand, float* work,
                       int32_t* active, void* stream);
int amh_asss_ext_shrink(amh_handle* h, int64_t num_chains, const float* pe, int32_t round, float* cand, float* work,
                        int32_t* active, void* stream);
int amh_asss_ext_finish(amh_handle* h, int64_t num_chains, const amh_state* in, const amh_state* out,
                        const float* cand, const float* work, const amh_collect* collect, void* stream);
/* ASSS.sample_Pnx (asss.py:271-303) likewise: transition t = 0 .. n-1 of every
 * chain c (key split(key)[c], as amh_asss_sample_pnx; the draws at stream
 * position t) from x_cur[c] (device [C][d]; the caller starts chain p *
 * n_samples + s at x[p]) with the frozen shared (loc[d], scale_packed[P]):
 * amh_asss_ext_pnx_begin, the rounds of amh_asss_ext_shrink as above, then
 * amh_asss_ext_pnx_finish writes the outcome back to x_cur and nothing else.
 * Same bits as amh_asss_sample_pnx given the same U. */
int amh_asss_ext_pnx_begin(amh_handle* h, const uint32_t key[2], const float* x_cur, int64_t num_chains,
                           const float* loc, const float* scale_packed, int32_t t, float* cand, float* work,
                           int32_t* active, void* stream);
int amh_asss_ext_pnx_finish(amh_handle* h, int64_t num_chains, const float* cand, const float* work, float* x_cur,
                            void* stream);

/* ----------------------------------------------------------- evaluation ----
 * python/utils/evaluation.py:223-294 (gaussian_kernel / mmd2_unbiased /
 * mmd_heuristic).  No handle: work goes to `stream` on the current device.
 * amh_kernel_sum: *out (device double) = sum over i < n, j < m of
 * exp(-gamma ||a_i - b_j||^2), pairs i == j skipped if skip_diag; a [n][d],
 * b [m][d] device float; scratch: amh_kernel_sum_scratch(n, m) device
 * doubles.  Deterministic (fixed-order reduction). */
int64_t amh_kernel_sum_scratch(int64_t n, int64_t m);
int amh_kernel_sum(const float* a, int64_t n, const float* b, int64_t m, int32_t d, float gamma,
                   int32_t skip_diag, double* scratch, double* out, void* stream);
/* out[i] = standard normal i of the stream keyed by key[2] (host memory),
 * for the random directions of max_sliced_wasserstein (evaluation.py:189). */
/* One half-iteration of log-domain Sinkhorn (the OT solver behind
 * wasserstein_sinkhorn, python/utils/evaluation.py:69-101, ott-jax linear.solve):
 * out[i] = -eps * log sum_j exp((pot[j] - cost[i][j]) / eps + log_w), cost
 * row-major [rows][cols] on the device.  The other half runs on the
 * transposed cost matrix. */
int amh_sinkhorn_lse(const float* cost, int64_t rows, int64_t cols, const float* pot, float log_w, float eps,
                     float* out, void* stream);
int amh_normals(const uint32_t key[2], int64_t n, float* out, void* stream);
/* out [n][m] = ||a_i - b_j||^2 (the median bandwidth heuristic, evaluation.py:286). */
int amh_pairwise_dist2(const float* a, int64_t n, const float* b, int64_t m, int32_t d, float* out,
                       void* stream);

/* Linear assignment of a square cost matrix (the optimal 1-1 coupling of
 * wasserstein_dist11_p, evaluation.py:43-67) on the device: the forward
 * auction, Jacobi form, with epsilon-scaling, on costs quantised to the
 * quantum 2^e (DESIGN.md §8 is the bit spec; all integers, so the result does
 * not depend on launch geometry).  cost: row-major [n][n] device float32,
 * 1 <= n <= 65536, every entry finite and >= 0; work: amh_assign_work_size
 * bytes of device memory, 8-byte aligned, that the caller keeps from begin to
 * result.  Nothing is kept in the library: the caller passes the same cost,
 * n and work to every call of one solve.
 *   amh_assign_begin    queues the scan (maximum, refusal flag) and zeroes
 *                       the prices
 *   amh_assign_quantum  waits; AMH_EINVAL if an entry is a NaN, an infinity or
 *                       negative, else e and qmax = the largest quantised
 *                       cost.  The phases run at eps_1 = max(1, qmax / 2),
 *                       eps_{k+1} = max(1, eps_k / theta), the last at eps = 1
 *   amh_assign_phase    every person unassigned, prices kept
 *   amh_assign_rounds   queues `rounds` rounds (three launches each) for at
 *                       most `bound` unassigned persons -- the count that
 *                       amh_assign_status last returned in this phase, n at its
 *                       start; `first`: rounds queued since amh_assign_phase.
 *                       A round that finds nobody unassigned does nothing
 *   amh_assign_status   waits; the unassigned count after the `queued` rounds
 *                       queued in this phase, and the rounds that did work
 *                       since amh_assign_begin
 *   amh_assign_result   perm [n] (person -> object, -1 if unassigned) and / or
 *                       the prices [n], device int64 */
int amh_assign_work_size(int64_t n, int64_t* bytes);
int amh_assign_begin(const float* cost, int64_t n, void* work, void* stream);
int amh_assign_quantum(const void* work, int64_t n, int32_t* e, int64_t* qmax, void* stream);
int amh_assign_phase(void* work, int64_t n, void* stream);
int amh_assign_rounds(const float* cost, int64_t n, void* work, int64_t eps, int64_t bound, int64_t first,
                      int32_t rounds, void* stream);
int amh_assign_status(const void* work, int64_t n, int64_t queued, int64_t* unassigned, int64_t* rounds,
                      void* stream);
int amh_assign_result(const void* work, int64_t n, int64_t* perm, int64_t* price, void* stream);

/* Streaming posterior summaries (infer_amd/streaming.py; DESIGN.md §7.1 is the
 * bit spec): folds one block of draws x [num_draws][num_chains][num_cols]
 * (device float32, contiguous: the layout of the collect buffer of amh_step)
 * into caller-owned running state, in one pass.  No handle; nothing is kept
 * in the library.
 *   calib [3][num_cols] float32: center, lo, inv_w per column
 *   acc   [5][num_chains][num_cols] float64: S1, S2, bs, S1b, Q per (chain,
 *         column), in draw order: y = (double)x - (double)center; S1 += y;
 *         S2 += y*y; bs += y; when (n_before + t + 1) % batch == 0:
 *         S1b += bs, Q += bs*bs, bs = 0.  No fma.  Non-finite draws propagate
 *   hist  [num_cols][nbins + 3] int64, pooled over chains: t = (x - lo) * inv_w
 *         in float32; bin nbins + 2 if t is a NaN, 0 if t < 0, nbins + 1 if
 *         t >= nbins, else 1 + (int)t
 * 1 <= num_cols <= 1024; nbins a power of two in 64 .. 2048; batch >= 1;
 * n_before: the draws per chain already folded in.  acc and hist start at
 * zero.  The result does not depend on how the draws are split into blocks. */
int amh_summary_update(const float* x, int64_t num_draws, int64_t num_chains, int32_t num_cols, const float* calib,
                       int32_t nbins, int64_t batch, int64_t n_before, double* acc, int64_t* hist, void* stream);

/* ---------------------------------------------------- pooled covariance ----
 * Regime B (build-defined, no reference analogue): every chain
 * proposes with ONE shared adapt state, and the adaptation of arwmh.py:180-197
 * consumes the statistics of all chains (of all ranks):
 *   mu'  = mu + gamma S_d / N,   Sig' = (1 - gamma) Sig + gamma S_dd / N,
 *   L'   = chol(Sig') (kept, with Sig, if Sig' is not positive definite),
 *   lam' = lam + gamma (S_a / N - target), macc' = macc + (S_a / N - macc) / n
 * where S_d = sum delta_c, S_dd = sum delta_c delta_c^T, S_a = sum alpha_c,
 * delta_c = z_c' - mu.  With N = 1 this is the reference recurrence.
 * A step is amh_pooled_stats (per-chain transition + local sums), an
 * all-reduce(sum) of the sums across ranks by the caller (RCCL through
 * torch.distributed), then amh_pooled_update on every rank. */
typedef struct amh_pooled_state {
  int32_t* i;                 /* [1]      shared iteration                   */
  float* z;                   /* [C][d]   per chain                          */
  float* potential_energy;    /* [C]                                         */
  uint32_t* rng_key;          /* [C][2]   per-chain Philox key               */
  float* mean_accept_prob;    /* [1]                                         */
  float* loc;                 /* [d]      shared mu                          */
  float* scale;               /* [P]      shared L, packed lower             */
  float* log_step_size;       /* [1]                                         */
  float* as_change;           /* [1]                                         */
  double* cov;                /* [P]      shared Sigma (= L L^T), packed     */
} amh_pooled_state;

/* Number of doubles in the sums vector: d + d(d+1)/2 + 2, laid out as
 * [S_d (d) | S_dd packed lower (P) | S_a | N]. */
int amh_pooled_sums_size(int32_t dim, int64_t* v);

/* Per-chain transition with the shared state `in`, z / pe written to
 * z_out / pe_out (may alias in), and this rank's sums (device, V doubles). */
int amh_pooled_stats(amh_handle* h, int64_t num_chains, const amh_pooled_state* in, float* z_out,
                     float* pe_out, double* sums, void* stream);

/* Shared-state update from the (all-reduced) sums; writes i, mean accept,
 * loc, scale, log_step_size, as_change, cov of `out` (may alias `in`). */
int amh_pooled_update(amh_handle* h, const double* sums, const amh_pooled_state* in,
                      const amh_pooled_state* out, void* stream);

/* Single-process convenience: n_steps of stats + update (no all-reduce).
 * sums: device scratch of amh_pooled_sums_size doubles. */
int amh_pooled_step(amh_handle* h, int64_t num_chains, const amh_pooled_state* in,
                    const amh_pooled_state* out, int32_t n_steps, double* sums, void* stream);

/* Pool every K steps (one exchange per K transitions).  The
 * shared state stays frozen for a block of K transitions of every chain
 * (noise positions i .. i+K-1), the sums cover all K * C chain-steps (delta
 * against the frozen mu, N = K * C), and one update ends the block: i += K,
 * gamma = 1 / n^a with n = the block count (i / K + 1, reset at num_warmup,
 * which must be a multiple of K).  K = 1 is amh_pooled_stats / _update. */
int amh_pooled_stats_k(amh_handle* h, int64_t num_chains, const amh_pooled_state* in, int32_t k_steps,
                       float* z_out, float* pe_out, double* sums, void* stream);
int amh_pooled_update_k(amh_handle* h, const double* sums, const amh_pooled_state* in,
                        const amh_pooled_state* out, int32_t k_steps, void* stream);
/* n_steps (a multiple of sync_every) transitions, one update per sync_every. */
int amh_pooled_step_k(amh_handle* h, int64_t num_chains, const amh_pooled_state* in,
                      const amh_pooled_state* out, int32_t n_steps, int32_t sync_every, double* sums,
                      void* stream);

/* The pooled transition with the caller's potential (AMH_MODEL_EXTERNAL; any
 * other model returns AMH_EINVAL): amh_pooled_stats split around U, the pooled
 * counterpart of amh_propose / amh_step_external.  d <= 64, or a multiple of
 * 32 up to 256.  Step t of a block (t = 0 when sync_every = 1):
 *   amh_pooled_propose         zprop[C][d] = z + fmaf(e^lam, L xi, eps xi) with
 *                              the shared (L, lam) of `in`, the noise of every
 *                              chain at stream position in->i[0] + t
 *                              (arwmh.py:162-167)
 *   the caller                 pe_prop[C] = U(zprop)
 *   amh_pooled_stats_external  accept (NaN -> +inf, arwmh.py:171-178; u from
 *                              the same stream position), z / pe to z_out /
 *                              pe_out (may alias in->z / in->potential_energy)
 *                              and this rank's sums of the step, S_d, S_dd,
 *                              S_a, N; accumulate != 0: sums += them.
 * Per chain and per sum the result is amh_pooled_stats' with pe_prop in place
 * of the in-kernel potential (d < 64 the lane-per-row form, d >= 64 the MFMA
 * form with 128-chain chunks), and amh_pooled_update_k consumes the sums
 * unchanged.  A block of K = sync_every steps is K rounds propose -> U ->
 * accept, `in` the frozen shared state with z / pe of the previous round,
 * accumulate = (t > 0): each round reduces its own s_t completely and
 * sums = s_0, then sums + s_t in step order.  That is amh_pooled_stats_k's
 * order above d = 64; up to d = 64 the fused kernels associate a block's sums
 * differently (chain-steps inside the chunk), so there an external block
 * equals K single-step calls added in step order, not amh_pooled_stats_k.
 * Nothing is kept in the handle between the calls: the shared L makes the
 * proposal a product over chains with no per-chain solves to remember, so
 * (unlike amh_step_external above d = 64) there is no "proposals of this
 * state" contract -- any zprop / pe_prop pair formed from `in` at step t is
 * taken. */
int amh_pooled_propose(amh_handle* h, int64_t num_chains, const amh_pooled_state* in, int32_t t,
                       float* zprop, void* stream);
int amh_pooled_stats_external(amh_handle* h, int64_t num_chains, const amh_pooled_state* in, int32_t t,
                              const float* zprop, const float* pe_prop, float* z_out, float* pe_out,
                              double* sums, int32_t accumulate, void* stream);

/* The exchange between amh_pooled_stats_k and amh_pooled_update_k on N > 1
 * ranks (SURVEY.md §8(b) amh_pooled_allreduce; no counterpart in the
 * reference, whose adaptation is per chain): in-place ncclAllReduce(sum) of
 * the n = amh_pooled_sums_size doubles at `sums` on `stream`, over the
 * caller's RCCL communicator `rccl_comm` (an ncclComm_t made by
 * ncclCommInitRank in the same RCCL instance; kernels_amd.distributed.RcclComm
 * does that).  The RCCL already loaded in the process is used (looked up by
 * soname), else the system librccl.so.1.  An RCCL error returns AMH_EHIP with
 * its text in amh_last_error; nothing is retried. */
int amh_pooled_allreduce(amh_handle* h, double* sums, int64_t n, void* rccl_comm, void* stream);

/* ----------------------------------------------------------- pooled ASSS ----
 * The slice sampler in regime B (build-defined): all chains
 * share mu (loc[d]), L (scale[P]), Sigma = L L^T (cov[P], double) and i.
 * A block is K = k_steps transitions of every chain with the shared state
 * frozen.  Transition t of chain c is asss.py:210-244 with the shared mu and
 * L in place of the chain's own:
 *   S = (L + eps I) sqrt(d);  y = S^-1 (x - mu) projected to z on S^d;
 *   tangent v orthogonal to z;  level t = U~(z) - log u;  shrinkage on
 *   z cos(theta) + v sin(theta) for at most 50 rounds (capped, or a
 *   degenerate tangent: theta = 0);  x' = S z'_{1:d} / (1 - z'_{d+1}) + mu;
 *   pe' = U(x'), NaN -> +inf.
 * Noise: the per-chain ASSS stream at position i + t with the chain's key:
 * Philox(r, i + t, 0, TAG_ASSS) for v, v_d, u_t, theta_0 and
 * Philox(k, i + t, 1, TAG_ASSS) for shrink round k.
 * The sums are the pooled vector [S_d | S_dd packed | S_a | N]:
 *   delta = x' - mu (the frozen mu),  S_d = sum delta,  S_dd = sum delta
 *   delta^T over the block's K C chain-steps,  N = K C,  S_a = sum a with
 *   a = 0 for a transition that kept its point (cap reached or degenerate
 *   tangent) and 1 otherwise, so mean_accept_prob is the running share of
 *   chain-steps that moved.
 * The update, from the all-reduced sums (amh_pooled_allreduce as it is):
 *   n = the block count (i / K + 1, reset at num_warmup), gamma = 1 / n^a,
 *   mu'  = mu + gamma S_d / N,   Sig' = (1 - gamma) Sig + gamma S_dd / N,
 *   L'   = chol(Sig') in double, rounded once (L and Sig kept if Sig' is not
 *          positive definite),
 *   macc' = macc + (S_a / N - macc) / n,   log_step_size copied through,
 *   as_change = ||mu' - mu||_2 + ||L' - L||_F (asss.py:259-260),  i += K.
 * With one chain in total this is the reference's recurrence (asss.py:246-255).
 * Arguments, in-place aliasing and errors as amh_pooled_stats_k / _update_k /
 * _step_k.  d <= 64 and a device potential (Gaussian, eight schools, kidiq,
 * diamonds, diamonds_suffstat, poisson): AMH_EINVAL otherwise (the logistic
 * model has no instantiation of this kernel). */
int amh_pooled_asss_stats_k(amh_handle* h, int64_t num_chains, const amh_pooled_state* in, int32_t k_steps,
                            float* z_out, float* pe_out, double* sums, void* stream);
int amh_pooled_asss_update_k(amh_handle* h, const double* sums, const amh_pooled_state* in,
                             const amh_pooled_state* out, int32_t k_steps, void* stream);
int amh_pooled_asss_step_k(amh_handle* h, int64_t num_chains, const amh_pooled_state* in,
                           const amh_pooled_state* out, int32_t n_steps, int32_t sync_every, double* sums,
                           void* stream);

/* Pooled ASSS with the caller's potential (AMH_MODEL_EXTERNAL, d <= 64): the
 * transition above cut at every potential evaluation, as amh_asss_ext_* cut
 * the per-chain one.  Transition t of a block, shared state of `in` frozen:
 *   amh_pooled_asss_ext_begin   for every chain at stream position in.i + t
 *                         with the chain's key: the draws, y = S^-1 (x - mu)
 *                         with the shared factor, projection, tangent, S z,
 *                         S v; x(theta = 0) -> cand[0], x(theta_0) -> cand[1]
 *                         (cand [2][C][d]); the chain's record -> work, in the
 *                         layout of amh_asss_ext_begin (amh_asss_ext_work_size
 *                         floats per chain; the shared mu copied per chain);
 *                         zeroes active (AMH_ASSS_EXT_ROUNDS int32)
 *   the caller's U of cand [2C, d], then amh_asss_ext_shrink(round 0), and
 *   U of cand[1] and amh_asss_ext_shrink(round r + 1) while active[r] != 0,
 *   exactly as for the per-chain sampler
 *   amh_pooled_asss_ext_finish  per chain the outcome (x(0) with its U when
 *                         capped or degenerate, else the accepted candidate
 *                         with the U of the round that accepted it, NaN ->
 *                         +inf) -> z_out / pe_out (may alias in's), and the
 *                         transition's sums [S_d | S_dd | S_a | N = C] into
 *                         sums (accumulate != 0: added to them), cut into the
 *                         chunks of amh_pooled_asss_stats_k: with the same U
 *                         the sums are that entry's at k_steps = 1 byte for
 *                         byte.  `in` is the state begin read.
 * A block of K transitions is K such sequences, t = 0 .. K - 1, the later ones
 * reading the z / pe the previous finish wrote, accumulate = (t > 0): the
 * block's sums are s_0 + s_1 + ... in step order (each transition's sums fully
 * reduced first, as amh_pooled_stats_external below d = 64; not the fused
 * kernel's in-chunk association).  After the exchange
 *   amh_pooled_asss_ext_update  is amh_pooled_asss_update_k for an external
 *                         handle.
 * Nothing is kept in the handle between the calls.  AMH_EINVAL: a handle not
 * bound to AMH_MODEL_EXTERNAL, dim > 64, null pointers, t < 0. */
int amh_pooled_asss_ext_begin(amh_handle* h, int64_t num_chains, const amh_pooled_state* in, int32_t t, float* cand,
                              float* work, int32_t* active, void* stream);
int amh_pooled_asss_ext_finish(amh_handle* h, int64_t num_chains, const amh_pooled_state* in, const float* cand,
                               const float* work, float* z_out, float* pe_out, double* sums, int32_t accumulate,
                               void* stream);
int amh_pooled_asss_ext_update(amh_handle* h, const double* sums, const amh_pooled_state* in,
                               const amh_pooled_state* out, int32_t k_steps, void* stream);

/* -------------------------------------------------------- exact sums ----
 * The sums above are added in double, in an order that depends on how many
 * chunks a rank holds, so two partitions of the same chains over ranks round
 * differently.  The entries below replace everything between the chunk partial
 * rows of the stats kernels (float32 values, each a function of its chunk's
 * chains alone) and the update by integer arithmetic, which no partition can
 * change (no counterpart in the reference, whose adaptation is
 * per chain).  The format (csrc/amh_exact.h, compiled into the kernels and into
 * the two host entries at the end):
 *   - a component of the sums vector is AMH_EXACT_WORDS = AMH_EXACT_LIMBS + 1
 *     int64 words.  Words 0 .. AMH_EXACT_LIMBS - 1 are signed limbs,
 *       value = sum_j limb_j 2^(AMH_EXACT_BITS j - AMH_EXACT_FRAC);
 *   - a finite float32 partial p with |p| < 2^80 adds the integer
 *     trunc(p 2^AMH_EXACT_FRAC), cut into AMH_EXACT_BITS-bit pieces that carry
 *     p's sign, to the limbs: no carry, no normalisation.  A partial whose
 *     lowest set bit is at least 2^-AMH_EXACT_FRAC is represented exactly, bits
 *     below that grid are cut toward zero (per partial, so the same for every
 *     partition);
 *   - a partial that is +-inf, NaN or has |p| >= 2^80 adds 1 to the last word
 *     and nothing to the limbs.  A component whose last word is non-zero
 *     converts to NaN, whatever its limbs hold; the other components are
 *     untouched;
 *   - only word-wise int64 addition ever happens to the words (within a rank,
 *     over the steps of a block, in the all-reduce).  A piece is below
 *     2^AMH_EXACT_BITS in magnitude, so AMH_EXACT_MAX_SUMMANDS partials per
 *     component cannot overflow a word (8 ranks x 512 chunks x 16 steps =
 *     65,536);
 *   - the conversion rounds the exact rational value of the limb totals to the
 *     nearest double (ties to even) through a wide integer.
 * A run through these entries is byte-identical for every number of ranks whose
 * shards start at multiples of amh_pooled_chunk_chains (a ragged tail only on
 * the last rank); one rank goes the same way.  The exchanged message is
 * amh_pooled_exact_size int64 words: 5 (d + d(d+1)/2 + 2) * 8 bytes, 86 KB at
 * d = 64 and 1.3 MB at d = 256. */
#define AMH_EXACT_BITS 40
#define AMH_EXACT_LIMBS 4
#define AMH_EXACT_FRAC 80
#define AMH_EXACT_WORDS 5
#define AMH_EXACT_MAX_SUMMANDS 8388608 /* 2^(63 - AMH_EXACT_BITS) */

/* Number of int64 words of the exact sums, [V][AMH_EXACT_WORDS] with V =
 * amh_pooled_sums_size (component-major). */
int amh_pooled_exact_size(int32_t dim, int64_t* n);

/* The chains per chunk of the pooled sums in a run of total_chains chains over
 * all ranks: 16 * min(16, ceil(total_chains / 4096)) below d = 64, 128 above;
 * at d = 64, where the Gaussian and a caller's potential run in 128-chain
 * chunks and the other registry models in those of d < 64, the least common
 * multiple of the two.  A rank's first global chain id must be a multiple. */
int amh_pooled_chunk_chains(int32_t dim, int64_t total_chains, int64_t* n);

/* amh_pooled_stats_k with the sums left as exact words: acc (device,
 * amh_pooled_exact_size int64) is overwritten with this rank's words of the
 * block.  total_chains >= num_chains is the chain count of all ranks; it cuts
 * the chunks below d = 64 (amh_pooled_stats_k cuts them by num_chains), so a
 * rank's chunks are those of the one-rank run.  Per chain the same bits as
 * amh_pooled_stats_k (given the same chunks). */
int amh_pooled_stats_k_exact(amh_handle* h, int64_t num_chains, int64_t total_chains, const amh_pooled_state* in,
                             int32_t k_steps, float* z_out, float* pe_out, int64_t* acc, void* stream);

/* amh_pooled_stats_external likewise; accumulate != 0: acc += the step's words
 * (the K rounds of a block, in any order). */
int amh_pooled_stats_external_exact(amh_handle* h, int64_t num_chains, int64_t total_chains,
                                    const amh_pooled_state* in, int32_t t, const float* zprop, const float* pe_prop,
                                    float* z_out, float* pe_out, int64_t* acc, int32_t accumulate, void* stream);

/* The (all-reduced) words -> the V doubles amh_pooled_update_k consumes. */
int amh_pooled_exact_to_sums(amh_handle* h, const int64_t* acc, double* sums, void* stream);

/* amh_pooled_allreduce for the exact words: ncclAllReduce(sum, ncclInt64) of
 * the n int64 at `acc`, RCCL resolved and errors reported the same way. */
int amh_pooled_allreduce_i64(amh_handle* h, int64_t* acc, int64_t n, void* rccl_comm, void* stream);

/* The format on the host (no handle, no device; host memory): the float32
 * partial rows partials[rows][v] into acc[v][AMH_EXACT_WORDS] (accumulate != 0:
 * added to what is there), and the words to out[v] doubles.  The same header
 * functions the kernels compile. */
int amh_pooled_exact_quantise(const float* partials, int64_t rows, int64_t v, int64_t* acc, int32_t accumulate);
int amh_pooled_exact_to_double(const int64_t* acc, int64_t v, double* out);

#ifdef __cplusplus
}
#endif

#endif /* AMH_H */
