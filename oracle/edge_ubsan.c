/*
 * edge_ubsan.c -- TEST INFRASTRUCTURE ONLY.  Stand-alone driver (own main, no
 * Python) that runs the C oracle's ARWMH and ASSS transitions from hostile
 * adaptation states, for a sanitizer build (make -C oracle edge_ubsan:
 * AddressSanitizer, UBSan and -fsanitize=float-cast-overflow, no recovery).
 *
 * A report from it (an out-of-range float -> int cast, say) marks a point
 * where the host's value is undefined while the device's is not, i.e. where
 * the oracle and the kernels may legitimately part; the oracle is then fixed
 * so the value is defined.  tests/test_edges.py builds and runs it and expects
 * exit status 0.
 *
 * Scenario (tests/helpers.py hostile_adapt, restated in C): a d = 8 and a
 * d = 100 Gaussian (tridiagonal precision), 160 chains, 5 benign steps, then
 * log_step_size cycling over {-110, -90, -20, 0, 20, 45, 88, 89} by chain,
 * the packed factor times {1e-30, .., 1e25} by (chain / 8) % 8, loc += 1e19
 * on the upper half of the chains, then 12 single steps and a fused launch
 * of 4.  num_warmup = 8 as in the Python scenarios (HOSTILE_WARMUP), so step 9
 * is the warmup reset from hostile values (gamma = 1, sqrt(1 - gamma) L = 0).
 * Two more d = 8 runs, ARWMH and ASSS, start every other chain from a point
 * scaled by 10^k, k in [-3, 20] (wild_starts).
 * The GLM models (ids 8 and 9: logistic at d = 8, Poisson with offsets at
 * d = 32, N = 77 rows, |X| < 1/4) run the hostile scenario with both samplers
 * and the wild starts with ARWMH.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>

typedef struct {
  int32_t model_id;
  int32_t d;
  int32_t num_warmup;
  float lr_decay;
  float target_accept_prob;
  float eps;
  const float* data;
  int64_t n_data;
  int64_t k_data;
} orc_cfg;

void orc_init(const orc_cfg* cfg, const uint32_t* key, int64_t chain_offset, int64_t C, const float* init_z,
              int32_t* i_, float* z, float* pe, float* macc, float* mu, float* L, float* lam, float* asc,
              uint32_t* keys);
void orc_step(const orc_cfg* cfg, int64_t C, int32_t n_steps, int32_t* i_, float* z, float* pe, float* macc,
              float* mu, float* L, float* lam, float* asc, const uint32_t* keys, int32_t* accept_count,
              float* collect_z);
void orc_asss_step(const orc_cfg* cfg, int64_t C, int32_t n_steps, int32_t* i_, float* z, float* pe, float* mu,
                   float* L, float* asc, const uint32_t* keys, float* collect_z, float* collect_pe);

static const float kLam[8] = {-110.0f, -90.0f, -20.0f, 0.0f, 20.0f, 45.0f, 88.0f, 89.0f};
static const float kMul[8] = {1e-30f, 1e-20f, 1e-8f, 1.0f, 1e8f, 1e15f, 1e19f, 1e25f};

static uint32_t lcg(uint32_t* s) { *s = *s * 1664525u + 1013904223u; return *s; }
static float unif(uint32_t* s) { return (float)(lcg(s) >> 8) * (1.0f / 16777216.0f); }

typedef struct {
  int32_t* i;
  float *z, *pe, *macc, *mu, *L, *lam, *asc;
  uint32_t* keys;
} state_t;

static state_t alloc_state(int64_t C, int d) {
  const int64_t P = (int64_t)d * (d + 1) / 2;
  state_t s;
  s.i = calloc(C, sizeof(int32_t));
  s.z = calloc(C * d, sizeof(float));
  s.pe = calloc(C, sizeof(float));
  s.macc = calloc(C, sizeof(float));
  s.mu = calloc(C * d, sizeof(float));
  s.L = calloc(C * P, sizeof(float));
  s.lam = calloc(C, sizeof(float));
  s.asc = calloc(C, sizeof(float));
  s.keys = calloc(2 * C, sizeof(uint32_t));
  return s;
}

static void free_state(state_t* s) {
  free(s->i); free(s->z); free(s->pe); free(s->macc); free(s->mu); free(s->L); free(s->lam); free(s->asc);
  free(s->keys);
}

static void hostile_adapt(state_t* s, int64_t C, int d, int step_size) {
  const int64_t P = (int64_t)d * (d + 1) / 2;
  for (int64_t c = 0; c < C; ++c) {
    const float m = kMul[(c / 8) % 8];
    for (int64_t k = 0; k < P; ++k) s->L[c * P + k] *= m;
    if (c >= C / 2)
      for (int r = 0; r < d; ++r) s->mu[c * d + r] += 1e19f;
    if (step_size) s->lam[c] = kLam[c % 8];
  }
}

enum { GAUSSIAN = 1, LOGISTIC = 8, POISSON = 9 };
#define GLM_N 77

/* [X (N x K) | y (N) | o (N, Poisson) | iI2, ib2, c0]: |X| < 1/4, y in {0, 1}
 * (logistic) or {0 .. 7} (Poisson), o in (-1, 1); priors N(0, 10), N(0, 2.5) */
static float* glm_data(int model, int d) {
  const int K = d - 1, side = model == POISSON ? 2 : 1;
  float* data = calloc((size_t)GLM_N * (size_t)(K + side) + 3, sizeof(float));
  uint32_t seed = 777u + (uint32_t)d;
  for (int k = 0; k < GLM_N * K; ++k) data[k] = unif(&seed) * 0.5f - 0.25f;
  float* y = data + GLM_N * K;
  for (int n = 0; n < GLM_N; ++n) y[n] = (float)(lcg(&seed) >> (model == POISSON ? 29 : 31));
  if (model == POISSON)
    for (int n = 0; n < GLM_N; ++n) y[GLM_N + n] = unif(&seed) * 2.0f - 1.0f;
  float* pr = y + side * GLM_N;
  pr[0] = 0.01f;
  pr[1] = 0.16f;
  pr[2] = 3.2215f + (float)K * 1.8352f;
  return data;
}

static int run(int model, int d, int asss, int wild) {
  const int64_t C = 160;
  float* data;
  if (model == GAUSSIAN) {
    data = calloc((size_t)d + (size_t)d * d + 1, sizeof(float));
    float* Pm = data + d;
    for (int r = 0; r < d; ++r) {
      Pm[r * d + r] = 2.0f + 0.01f * (float)r;
      if (r + 1 < d) Pm[r * d + r + 1] = Pm[(r + 1) * d + r] = -0.5f;
    }
  } else {
    data = glm_data(model, d);
  }
  orc_cfg cfg = {model, d, 8 /* HOSTILE_WARMUP */, 2.0f / 3.0f, 0.234f, 1e-6f, data,
                 model == GAUSSIAN ? 0 : GLM_N, model == GAUSSIAN ? 0 : d - 1};
  state_t s = alloc_state(C, d);
  float* z0 = calloc(C * d, sizeof(float));
  uint32_t seed = 12345u + (uint32_t)d;
  for (int64_t c = 0; c < C; ++c) {
    float sc = 1.0f;
    if (wild && (c & 1)) {
      const int k = (int)(lcg(&seed) % 24u) - 3;
      sc = powf(10.0f, (float)k);
    }
    for (int r = 0; r < d; ++r) z0[c * d + r] = (unif(&seed) * 4.0f - 2.0f) * sc;
  }
  const uint32_t key[2] = {0u, 7u};
  orc_init(&cfg, key, 0, C, z0, s.i, s.z, s.pe, s.macc, s.mu, s.L, s.lam, s.asc, s.keys);
  int32_t* acc = calloc(C, sizeof(int32_t));
  if (asss) orc_asss_step(&cfg, C, 5, s.i, s.z, s.pe, s.mu, s.L, s.asc, s.keys, NULL, NULL);
  else orc_step(&cfg, C, 5, s.i, s.z, s.pe, s.macc, s.mu, s.L, s.lam, s.asc, s.keys, acc, NULL);
  hostile_adapt(&s, C, d, !asss);
  for (int t = 0; t < 12; ++t) {
    if (asss) orc_asss_step(&cfg, C, 1, s.i, s.z, s.pe, s.mu, s.L, s.asc, s.keys, NULL, NULL);
    else orc_step(&cfg, C, 1, s.i, s.z, s.pe, s.macc, s.mu, s.L, s.lam, s.asc, s.keys, acc, NULL);
  }
  /* a fused launch on top (the in-launch (U, dl) carry) */
  if (asss) orc_asss_step(&cfg, C, 4, s.i, s.z, s.pe, s.mu, s.L, s.asc, s.keys, NULL, NULL);
  else orc_step(&cfg, C, 4, s.i, s.z, s.pe, s.macc, s.mu, s.L, s.lam, s.asc, s.keys, acc, NULL);
  int64_t nonfinite = 0, moved = 0;
  const int64_t P = (int64_t)d * (d + 1) / 2;
  for (int64_t c = 0; c < C; ++c) {
    int bad = 0;
    for (int64_t k = 0; k < P; ++k) bad |= !isfinite(s.L[c * P + k]);
    nonfinite += bad;
    moved += memcmp(s.z + c * d, z0 + c * d, sizeof(float) * (size_t)d) != 0;
  }
  printf("model %d d=%d %s%s: %lld of %lld chains with a non-finite factor, %lld moved\n", model, d, asss ? "asss" : "arwmh",
         wild ? " wild" : "", (long long)nonfinite, (long long)C, (long long)moved);
  const int ok = s.i[0] == 21;
  free(acc); free(z0); free_state(&s); free(data);
  return ok ? 0 : 1;
}

int main(void) {
  int rc = 0;
  for (int asss = 0; asss < 2; ++asss) {
    rc |= run(GAUSSIAN, 8, asss, 0);
    rc |= run(GAUSSIAN, 100, asss, 0);
    rc |= run(LOGISTIC, 8, asss, 0);
    rc |= run(POISSON, 32, asss, 0);
  }
  rc |= run(GAUSSIAN, 8, 0, 1);
  rc |= run(GAUSSIAN, 8, 1, 1);
  rc |= run(LOGISTIC, 8, 0, 1);
  rc |= run(POISSON, 32, 0, 1);
  return rc;
}
