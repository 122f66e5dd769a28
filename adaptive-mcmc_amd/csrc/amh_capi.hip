// amh_capi.hip -- the extern "C" boundary of libamh.so (include/amh.h).
// Validates arguments, keeps per-handle configuration and model binding, and
// enqueues the kernels of amh_kernels.hip, amh_step64.hip and the other
// csrc/*.hip files on the caller's stream.
// Layout: the handle and its helpers, then one extern "C" region per family
// (core, external potential, ASSS, evaluation, pooled covariance, pooled ASSS, diagnostics),
// each preceded by the helpers only that family uses.
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/amh.h"
#include "../../include/amh_math.h"
#include "amh_exact.h"
#include "amh_internal.h"
#include "amh_s64_sched.h"

namespace amh {

// device scratch owned by a handle: grown on demand, never shrunk
struct Scratch {
  void* ptr = nullptr;
  size_t bytes = 0;

  template <class T>
  T* as() const { return static_cast<T*>(ptr); }
  // at least `need` bytes, reported as `who`; zero_fresh: a new allocation starts zeroed
  int grow(amh_handle* h, size_t need, void* stream, const char* who, bool zero_fresh = false);
  void release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    bytes = 0;
  }
};

}  // namespace amh

struct amh_handle {
  amh_config cfg;
  int device = 0;
  int model_id = 0;
  amh::ModelArgs model{nullptr, 0, 0};
  int64_t n_data = 0;
  float* gamma_tab = nullptr;  // device, kGammaTab entries
  float* xpack = nullptr;      // diamonds, logistic, poisson: design matrix in MFMA tile order (made by amh_bind_model)
  amh::Scratch partials;       // pooled mode: chunk partial sums
  amh::Scratch split;          // split path: proposals [C][d] then U(z') [C]; d > 64: xprop, wa, wr, dg [C][d]
                               // then U(z') [C]; pooled d > 64: the A-operand copies (pooled_big_pack_floats)
  int64_t big_ready_C = -1;    // d > 64: split holds the next proposal of the last output state (C chains)
  amh_state big_ready_out{};   // ... and that output state's buffers: READY is honoured only for these
  int64_t ext_ready_C = -1;    // external potential, d > 64: split holds the solves (wa, wr, dg) of
  amh_state ext_ready_in{};    // the proposals formed from this state (amh_propose / amh_step_external)
  amh::Scratch upd;            // pooled d >= 64: Sigma' / L' staging (pooled_update_scratch_floats)
  amh::Scratch noise;          // pooled d >= 64: [cap] records (i, key0, key1, u bits) then xi [cap][d]
  int64_t noise_cap = 0;       // chains the noise buffer holds
  int64_t noise_C = 0;         // chains of the last stats call, whose keys are at noise_keys
  const uint32_t* noise_keys = nullptr;
  int* err_host = nullptr;     // pooled d = 64: host-mapped device error flag (PooledUpdateParams::err_flag)
  int* err_dev = nullptr;      // ... its device address
  const float* s64_scale = nullptr;  // d = 64 step kernel: the factor buffer its last launch wrote,
  int64_t s64_C = 0;                 // that launch's chain count
  int32_t s64_order = -1;            // and chain order (0 ascending, 1 descending; -1: no launch yet)
  uint32_t* s64_heads = nullptr;     // d = 64 single-step launch: a head word per possible block (amh_s64_sched.h),
                                     // allocated and zeroed once by amh_bind_model
  int32_t s64_steal = (int32_t)amh::kS64StealDefault;  // its stealable-tail length (amh_step64_set_steal)
  uint32_t s64_tag = 0;              // the last such launch's tag, 1 ... 65535 (0: none yet)
  std::string err;
};

namespace {

thread_local std::string g_err;

int fail(amh_handle* h, int code, const std::string& msg) {
  if (h) h->err = msg; else g_err = msg;
  return code;
}

int hip_fail(amh_handle* h, hipError_t e, const std::string& where) {
  return fail(h, AMH_EHIP, where + ": " + hipGetErrorString(e));
}

}  // namespace

// a queued launch may still read the old buffer, so the stream drains before the free
int amh::Scratch::grow(amh_handle* h, size_t need, void* stream, const char* who, bool zero_fresh) {
  if (need <= bytes) return AMH_OK;
  if (ptr) (void)hipStreamSynchronize((hipStream_t)stream);
  release();
  hipError_t e = hipMalloc(&ptr, need);
  if (e != hipSuccess) return hip_fail(h, e, std::string(who) + "/hipMalloc");
  bytes = need;
  if (zero_fresh) {
    e = hipMemsetAsync(ptr, 0, bytes, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(h, e, std::string(who) + "/hipMemsetAsync");
  }
  return AMH_OK;
}

namespace {

const char* const kUpdateStuck =
    "amh_pooled_update (d = 64): a factoring wave's bounded wait for an earlier wave's columns ran out in an "
    "earlier launch; that update kept the factor and covariance (the run no longer follows the bit spec)";

// a device-side failure flagged by an earlier (asynchronous) launch: reported
// by the handle's next pooled call and by amh_last_error, then cleared
int check_device_flag(amh_handle* h) {
  if (h && h->err_host && *(volatile int*)h->err_host != 0) {
    *(volatile int*)h->err_host = 0;
    return fail(h, AMH_EHIP, kUpdateStuck);
  }
  return AMH_OK;
}

// every entry's first checks, reported under the entry's public name `who`
int enter(amh_handle* h, const char* who, bool needs_model) {
  if (!h) return fail(nullptr, AMH_EINVAL, std::string(who) + ": null handle");
  if (needs_model && !h->model_id) return fail(h, AMH_ENOMODEL, std::string(who) + ": no model bound");
  return AMH_OK;
}

// ... and its last one before it enqueues work: after the argument checks, so
// that a refused call leaves the thread's current device alone
int use_device(amh_handle* h, const char* who) {
  const hipError_t e = hipSetDevice(h->device);
  if (e != hipSuccess) return hip_fail(h, e, std::string(who) + "/hipSetDevice");
  return AMH_OK;
}

bool same_buffers(const amh_state& a, const amh_state& b) {
  return a.i == b.i && a.z == b.z && a.potential_energy == b.potential_energy &&
         a.mean_accept_prob == b.mean_accept_prob && a.loc == b.loc && a.scale == b.scale &&
         a.log_step_size == b.log_step_size && a.as_change == b.as_change && a.rng_key == b.rng_key;
}

bool state_ok(const amh_state* s) {
  return s && s->i && s->z && s->potential_energy && s->mean_accept_prob && s->loc && s->scale &&
         s->log_step_size && s->as_change && s->rng_key;
}

// a GLM's checks (amh_device.h): data = [X (N x K) | nside vectors of N | 3 prior constants]
int glm_dim(const char* name, int nside, int64_t n_data, const int64_t* ip, int nip, std::string* why) {
  const std::string who(name);
  if (nip < 2) { *why = who + " needs iparams {N, K}"; return -1; }
  const int64_t N = ip[0], K = ip[1];
  if (K < 1 || K > 31) { *why = who + " needs 1 <= K <= 31 predictors"; return -1; }
  if (N < 1) { *why = who + " needs N >= 1 rows"; return -1; }
  if (n_data != N * K + nside * N + 3) {
    *why = who + " data must hold N*K + " + (nside == 1 ? "" : std::to_string(nside) + "*") + "N + 3 floats";
    return -1;
  }
  return (int)(K + 1);
}

int expected_dim(int model_id, int64_t n_data, const int64_t* ip, int nip, int d, std::string* why) {
  switch (model_id) {
    case AMH_MODEL_GAUSSIAN:
      if (n_data != (int64_t)d + (int64_t)d * d + 1) { *why = "gaussian data must hold d + d*d + 1 floats"; return -1; }
      return d;
    case AMH_MODEL_EIGHT_SCHOOLS: {
      if (nip < 1) { *why = "eight_schools needs iparams {J}"; return -1; }
      const int64_t J = ip[0];
      if (n_data != 3 * J) { *why = "eight_schools data must hold 3*J floats"; return -1; }
      return (int)(J + 2);
    }
    case AMH_MODEL_KIDIQ: {
      if (nip < 1) { *why = "kidiq needs iparams {N}"; return -1; }
      if (n_data != 3 * ip[0]) { *why = "kidiq data must hold 3*N floats"; return -1; }
      return 4;
    }
    case AMH_MODEL_DIAMONDS: {
      if (nip < 2) { *why = "diamonds needs iparams {N, K}"; return -1; }
      const int64_t N = ip[0], K = ip[1];
      if (n_data != N * (K - 1) + N) { *why = "diamonds data must hold N*(K-1) + N floats"; return -1; }
      return (int)(K + 1);
    }
    case AMH_MODEL_DIAMONDS_SS: {
      if (nip < 2) { *why = "diamonds_suffstat needs iparams {N, K}"; return -1; }
      const int64_t Kc = ip[1] - 1;
      if (Kc < 1 || Kc > 30) { *why = "diamonds_suffstat needs 2 <= K <= 31"; return -1; }
      if (n_data != 2 * (4 + 2 * Kc + Kc * Kc)) { *why = "diamonds_suffstat data must hold 2 (4 + 2 Kc + Kc^2) floats"; return -1; }
      return (int)(Kc + 2);
    }
    case AMH_MODEL_LOGISTIC:
      return glm_dim("logistic", 1, n_data, ip, nip, why);
    case AMH_MODEL_POISSON:
      return glm_dim("poisson", 2, n_data, ip, nip, why);
    case AMH_MODEL_MIXTURE: {
      if (nip < 1) { *why = "mixture needs iparams {K}"; return -1; }
      if (ip[0] < 1 || ip[0] > 8) { *why = "mixture needs 1 <= K <= 8 components"; return -1; }
      if (n_data != 3 * ip[0]) { *why = "mixture data must hold 3*K floats"; return -1; }
      if (d < 1 || d > 16) { *why = "mixture needs 1 <= d <= 16"; return -1; }
      return d;
    }
    case AMH_MODEL_EXTERNAL:
      if (n_data < 0 || nip != 0) { *why = "external potential takes no data or iparams"; return -1; }
      if (d < 1 || d > 256) { *why = "external potential needs 1 <= d <= 256"; return -1; }
      return d;
    default:
      *why = "unknown model id";
      return -1;
  }
}

// ---- kernel parameters from the handle ----
// the fields StepParams and BigParams share: the configuration, the state
// buffers of one call over C chains and its optional collection
template <class P>
P handle_params(const amh_handle* h, int64_t C, const amh_state& in, const amh_state& out,
                const amh_collect* collect) {
  P p{};
  p.in = in;
  p.out = out;
  p.C = C;
  p.d = h->cfg.dim;
  p.W = h->cfg.num_warmup;
  p.a = h->cfg.lr_decay;
  p.target = h->cfg.target_accept_prob;
  p.eps = h->cfg.eps;
  p.gamma_tab = h->gamma_tab;
  p.gamma_tab_n = amh::kGammaTab;
  p.col_z = collect ? collect->z : nullptr;
  p.col_pe = collect ? collect->potential_energy : nullptr;
  p.accept_count = collect ? collect->accept_count : nullptr;
  return p;
}

amh::StepParams step_params(const amh_handle* h, int64_t C, const amh_state& in, const amh_state& out,
                            int32_t n_steps, const amh_collect* collect) {
  amh::StepParams p = handle_params<amh::StepParams>(h, C, in, out, collect);
  p.n_steps = n_steps;
  p.thinning = collect ? collect->thinning : 1;
  p.model = h->model;
  return p;
}

// The d = 64 Gaussian step kernel (arwmh_step64_kernel, ARWMH and ASSS) walks
// each block's chain range in either order with the same results.  A launch
// whose input is what the handle's last such launch wrote (the same factor
// buffer and chain count) takes the opposite order: its first reads are that
// launch's last writes, which the memory-side cache still holds (DESIGN.md
// 3.1).  Any other launch runs ascending.
bool step64_shape(const amh_handle* h) { return h->model_id == AMH_MODEL_GAUSSIAN && h->cfg.dim == 64; }

int32_t step64_order(const amh_handle* h, const amh::StepParams& p) {
  return (h->s64_order >= 0 && p.in.scale == h->s64_scale && p.C == h->s64_C) ? 1 - h->s64_order : 0;
}

// ... and only such a launch has a hot part (amh_s64_sched.h): one that runs
// ascending because it is unrelated to the previous launch finds nothing of
// its input in the cache.
int32_t step64_chained(const amh_handle* h, const amh::StepParams& p) {
  return h->s64_order >= 0 && p.in.scale == h->s64_scale && p.C == h->s64_C;
}

static_assert(AMH_S64_STEAL_TRIES == amh::kS64StealTries, "include/amh.h states the victim count");
constexpr size_t kS64HeadBytes =(size_t)amh::kS64HeadSlots * amh::kS64HeadStride * sizeof(uint32_t);

// The head words, the tail length and the next tag of a single-step launch.
// No launch and no memset of its own: every block re-arms its word, and
// between launches every word is exhausted or carries another tag.  Only when
// the 16-bit tag wraps are the words zeroed on the stream (tag 0 is never a
// launch's), so that a word some launch of the last 65,535 left behind cannot
// carry the new launch's tag.
hipError_t step64_heads(amh_handle* h, amh::StepParams& p, hipStream_t s) {
  if (!h->s64_heads || p.n_steps != 1) return hipSuccess;
  if (++h->s64_tag > 0xFFFFu) {
    const hipError_t e = hipMemsetAsync(h->s64_heads, 0, kS64HeadBytes, s);
    if (e != hipSuccess) return e;
    h->s64_tag = 1;
  }
  p.heads = h->s64_heads;
  p.steal = h->s64_steal;
  p.tag = (int32_t)h->s64_tag;
  return hipSuccess;
}

void step64_launched(amh_handle* h, const amh::StepParams& p) {
  h->s64_scale = p.out.scale;
  h->s64_C = p.C;
  h->s64_order = p.descending;
}

// the scratch pointers (xprop, wa, wr, dg, pep) are the caller's to set
amh::BigParams big_params(const amh_handle* h, int64_t C, const amh_state& in, const amh_state& out,
                          const amh_collect* collect) {
  return handle_params<amh::BigParams>(h, C, in, out, collect);
}

// ---- one transition per launch sequence ----
// collection of a call `p` that is issued one transition at a time: step t
// keeps slot t / thinning iff (t + 1) % thinning == 0, and writes none otherwise
struct Slot {
  float *z, *pe;
};

Slot collect_slot(const amh::StepParams& p, int32_t t) {
  if ((t + 1) % p.thinning != 0) return {nullptr, nullptr};
  const size_t k = (size_t)(t / p.thinning);
  return {p.col_z ? p.col_z + k * (size_t)p.C * p.d : nullptr, p.col_pe ? p.col_pe + k * (size_t)p.C : nullptr};
}

// The call `p` as n_steps chained transitions over the handle's split scratch
// of floats_per_chain floats per chain (d > 64, and the literal diamonds split
// path).  transition(in, slot, propose, next) enqueues one transition from
// state `in`: the propose pass if `propose`, the potential of the proposals,
// and the step pass, which also forms the next transition's proposal if `next`
// (so the factor is read once per transition).  Only the first transition of
// a call may need the propose pass: not when the caller vouches
// (AMH_STEP_PROPOSAL_READY) that `in` is the unchanged output of the previous
// call, which kept its next proposal in the scratch (AMH_STEP_KEEP_PROPOSAL),
// and `in` is the very buffers that call wrote.
template <class Transition>
int run_chained(amh_handle* h, const amh::StepParams& p, size_t floats_per_chain, int32_t flags, void* stream,
                const char* where, Transition transition) {
  const size_t need = (size_t)p.C * floats_per_chain * sizeof(float);
  // a proposal kept for C chains means the scratch held `need` bytes already; it
  // can have grown since only if an allocation failed, and then holds nothing
  const bool grown = need > h->split.bytes;
  if (int rc = h->split.grow(h, need, stream, "amh_step")) return rc;
  const bool ready = !grown && (flags & AMH_STEP_PROPOSAL_READY) && h->big_ready_C == p.C &&
                     same_buffers(p.in, h->big_ready_out);
  const bool keep_next = (flags & AMH_STEP_KEEP_PROPOSAL) != 0;
  h->big_ready_C = -1;
  for (int32_t t = 0; t < p.n_steps; ++t) {
    const hipError_t e =
        transition(t == 0 ? p.in : p.out, collect_slot(p, t), t == 0 && !ready, t + 1 < p.n_steps || keep_next);
    if (e != hipSuccess) return hip_fail(h, e, where);
  }
  h->big_ready_C = keep_next ? p.C : -1;
  h->big_ready_out = p.out;
  return AMH_OK;
}

// A/B switches of the diagnostic build only (-DAMH_DIAG, `make stamps`; the
// bits are the same either way, the release library reads no environment):
// NAME=0 turns the optimisation off
bool diag_env_off(const char* name) {
#ifdef AMH_DIAG
  const char* e = getenv(name);
  return e != nullptr && e[0] == '0';
#else
  (void)name;
  return false;
#endif
}

}  // namespace

// -------------------------------------------------------------------- core --
extern "C" {

int amh_version(void) { return AMH_ABI_VERSION; }

const char* amh_last_error(const amh_handle* h) {
  if (h && h->err_host && *(volatile int*)h->err_host != 0) const_cast<amh_handle*>(h)->err = kUpdateStuck;
  return h ? h->err.c_str() : g_err.c_str();
}

int amh_create(const amh_config* cfg, int device, amh_handle** out) {
  if (!cfg || !out) return fail(nullptr, AMH_EINVAL, "amh_create: null argument");
  if (cfg->dim < 1 || cfg->dim > 256) return fail(nullptr, AMH_EINVAL, "amh_create: dim must be in [1, 256]");
  if (cfg->num_warmup < 0) return fail(nullptr, AMH_EINVAL, "amh_create: num_warmup < 0");
  amh_handle* h = new (std::nothrow) amh_handle();
  if (!h) return fail(nullptr, AMH_ENOMEM, "amh_create: out of memory");
  h->cfg = *cfg;
  h->device = device;
  // gamma_n = 1 / n^a for n < kGammaTab, evaluated on the host by the same
  // routine the kernels use for larger n (include/amh_math.h).
  std::vector<float> tab(amh::kGammaTab);
  tab[0] = 1.0f;
  for (int32_t n = 1; n < amh::kGammaTab; ++n) tab[n] = amh_lr_gamma(n, cfg->lr_decay);
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipMalloc(&h->gamma_tab, sizeof(float) * tab.size());
  if (e == hipSuccess) e = hipMemcpy(h->gamma_tab, tab.data(), sizeof(float) * tab.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    const int rc = hip_fail(nullptr, e, "amh_create");
    if (h->gamma_tab) (void)hipFree(h->gamma_tab);
    delete h;
    return rc;
  }
  *out = h;
  return AMH_OK;
}

int amh_check_device(amh_handle* h) {
  if (int rc = enter(h, "amh_check_device", false)) return rc;
  return check_device_flag(h);
}

int amh_step_order(amh_handle* h, int32_t* order) {
  if (int rc = enter(h, "amh_step_order", false)) return rc;
  if (!order) return fail(h, AMH_EINVAL, "amh_step_order: null argument");
  *order = h->s64_order;
  return AMH_OK;
}

int amh_step64_schedule(int32_t n, int32_t descending, int32_t* index, int32_t* cls) {
  if (n < 0 || (n > 0 && (!index || !cls))) return fail(nullptr, AMH_EINVAL, "amh_step64_schedule: bad arguments");
  const amh::S64Sched s = amh::s64_sched((uint32_t)n, descending != 0, 1);
  for (int32_t k = 0; k < n; ++k) {
    const uint32_t v = amh::s64_draw(s, (uint32_t)k);
    index[k] = (int32_t)v;
    cls[k] = (int32_t)amh::s64_class(v, s.hot_lo, s.hot_n, s.tail_lo, s.tail_n);
  }
  return AMH_OK;
}

int amh_step64_steal_schedule(int32_t n, int32_t descending, int32_t steal, int32_t block, int32_t grid,
                              int32_t* n_own, int32_t* index, int32_t* cls, int32_t* victims, int32_t* n_victims) {
  if (n < 0 || steal < 0 || grid < 1 || block < 0 || block >= grid || !n_own || !victims || !n_victims ||
      (n > 0 && (!index || !cls)))
    return fail(nullptr, AMH_EINVAL, "amh_step64_steal_schedule: bad arguments");
  const amh::S64Sched s = amh::s64_sched((uint32_t)n, descending != 0, 1);
  const uint32_t T = amh::s64_tail_len((uint32_t)n, (uint32_t)steal);
  const uint32_t own = (uint32_t)n - T, lo = amh::s64_own_lo(T, descending != 0);
  *n_own = (int32_t)own;
  // the own part: what the LDS counter hands out, while it lies inside [lo, lo + own)
  int32_t k = 0;
  for (uint32_t v = amh::s64_draw(s, 0); v - lo < own; v = amh::s64_draw(s, (uint32_t)++k)) {
    index[k] = (int32_t)v;
    cls[k] = (int32_t)amh::s64_class(v, s.hot_lo, s.hot_n, s.tail_lo, s.tail_n);
  }
  if (k != (int32_t)own) return fail(nullptr, AMH_EINVAL, "amh_step64_steal_schedule: the own part is not a prefix");
  // the tail: head counts 0 ... T - 1, as long as the word says they are valid
  for (uint32_t c = 0; amh::s64_head_valid((1u << 16) | c, 1u, T); ++c, ++k) {
    const uint32_t v = amh::s64_tail_index(s, (uint32_t)n, T, c);
    index[k] = (int32_t)v;
    cls[k] = (int32_t)amh::s64_class(v, s.hot_lo, s.hot_n, s.tail_lo, s.tail_n);
  }
  *n_victims = 0;
  for (uint32_t t = 1; t <= amh::kS64StealTries; ++t) {
    const uint32_t v = amh::s64_victim((uint32_t)block, (uint32_t)grid, t);
    if (v == (uint32_t)grid) break;
    victims[(*n_victims)++] = (int32_t)v;
  }
  return AMH_OK;
}

int amh_step64_set_steal(amh_handle* h, int32_t steal) {
  if (int rc = enter(h, "amh_step64_set_steal", false)) return rc;
  if (steal < 0 || steal > 0xFFFF) return fail(h, AMH_EINVAL, "amh_step64_set_steal: steal must be in [0, 65535]");
  h->s64_steal = steal;
  return AMH_OK;
}

int amh_step64_stolen(amh_handle* h, int64_t* stolen, void* stream) {
  if (int rc = enter(h, "amh_step64_stolen", false)) return rc;
  if (!stolen) return fail(h, AMH_EINVAL, "amh_step64_stolen: null argument");
  *stolen = 0;
  if (!h->s64_heads || h->s64_tag == 0) return AMH_OK;
  if (int rc = use_device(h, "amh_step64_stolen")) return rc;
  std::vector<uint32_t> w(kS64HeadBytes / sizeof(uint32_t));
  hipError_t e = hipStreamSynchronize((hipStream_t)stream);
  if (e == hipSuccess) e = hipMemcpy(w.data(), h->s64_heads, kS64HeadBytes, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return hip_fail(h, e, "amh_step64_stolen");
  // a block's count is beside its head and was armed with the launch's tag
  for (uint32_t b = 0; b < amh::kS64HeadSlots; ++b) {
    const uint32_t c = w[(size_t)b * amh::kS64HeadStride + 1];
    if ((c >> 16) == h->s64_tag) *stolen += (int64_t)(c & 0xFFFFu);
  }
  return AMH_OK;
}

int amh_destroy(amh_handle* h) {
  int rc = AMH_OK;
  if (h) {
    (void)hipSetDevice(h->device);
    // no device-wide synchronisation here (destroy runs from
    // finalisers): the flag is read as it stands; a launch still in flight is
    // covered by amh_check_device after the caller synchronised its stream.
    // hipFree below orders the frees after outstanding work as HIP defines.
    if (h->err_host && *(volatile int*)h->err_host != 0) rc = fail(nullptr, AMH_EHIP, kUpdateStuck);
    if (h->gamma_tab) (void)hipFree(h->gamma_tab);
    if (h->xpack) (void)hipFree(h->xpack);
    if (h->s64_heads) (void)hipFree(h->s64_heads);
    for (amh::Scratch* s : {&h->partials, &h->split, &h->upd, &h->noise}) s->release();
    if (h->err_host) (void)hipHostFree(h->err_host);
  }
  delete h;
  return rc;
}

int amh_bind_model(amh_handle* h, int32_t model_id, const float* data, int64_t n_data, const int64_t* iparams,
                   int32_t n_iparams) {
  if (int rc = enter(h, "amh_bind_model", false)) return rc;
  if (!data) return fail(h, AMH_EINVAL, "amh_bind_model: null data");
  std::string why;
  const int dm = expected_dim(model_id, n_data, iparams, n_iparams, h->cfg.dim, &why);
  if (dm < 0) return fail(h, AMH_EINVAL, "amh_bind_model: " + why);
  if (dm != h->cfg.dim)
    return fail(h, AMH_EINVAL, "amh_bind_model: model dimension " + std::to_string(dm) + " != config dim " +
                                   std::to_string(h->cfg.dim));
  if (dm > 64 && !amh::big_model(model_id, dm) && model_id != AMH_MODEL_EXTERNAL)
    return fail(h, AMH_EINVAL, "amh_bind_model: d > 64 needs the Gaussian model or an external potential (d <= 256)");
  // the handle's device for everything below (the caller -- Handle.bind_model --
  // holds it current and restores its own afterwards)
  if (int rc = use_device(h, "amh_bind_model")) return rc;
  if (h->xpack) {
    (void)hipDeviceSynchronize();  // a queued launch may still read the old copy
    (void)hipFree(h->xpack);
    h->xpack = nullptr;
  }
  h->model_id = 0;  // unbound until the whole binding has succeeded
  h->model.data = data;
  const bool dia = model_id == AMH_MODEL_DIAMONDS || model_id == AMH_MODEL_DIAMONDS_SS ||
                   model_id == AMH_MODEL_LOGISTIC || model_id == AMH_MODEL_POISSON;  // iparams {N, K}
  h->model.n = (model_id == AMH_MODEL_KIDIQ || model_id == AMH_MODEL_MIXTURE || dia) ? iparams[0] : 0;
  h->model.k = dia ? iparams[1] : 0;
  h->n_data = n_data;
  if (amh::split_model(model_id, dm)) {  // diamonds, logistic, poisson
    // the MFMA potential's tile copy of the design matrix and the response, made
    // once here (synchronous, on the null stream: the caller has synchronised the
    // stream that wrote data)
    const int64_t nf = amh::model_pack_floats(model_id, h->model.n, h->model.k);
    if (nf > 0) {
      hipError_t e = hipMalloc(&h->xpack, (size_t)nf * sizeof(float));
      if (e == hipSuccess) e = amh::run_model_pack(model_id, h->model, h->xpack, nullptr);
      if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
      if (e != hipSuccess) {
        if (h->xpack) (void)hipFree(h->xpack);
        h->xpack = nullptr;
        return hip_fail(h, e, "amh_bind_model(tile copy)");
      }
    }
  }
  if (model_id == AMH_MODEL_GAUSSIAN && dm == 64 && !h->s64_heads) {
    // the d = 64 single-step launch's head words, zeroed once: tag 0 is no launch's
    hipError_t e = hipMalloc(&h->s64_heads, kS64HeadBytes);
    if (e == hipSuccess) e = hipMemset(h->s64_heads, 0, kS64HeadBytes);
    if (e != hipSuccess) {
      if (h->s64_heads) (void)hipFree(h->s64_heads);
      h->s64_heads = nullptr;
      return hip_fail(h, e, "amh_bind_model(d = 64 head words)");
    }
  }
  h->model_id = model_id;
  return AMH_OK;
}

int amh_init(amh_handle* h, const uint32_t key[2], int64_t chain_offset, int64_t num_chains, const float* init_z,
             const amh_state* out, void* stream) {
  if (int rc = enter(h, "amh_init", true)) return rc;
  if (!key || !state_ok(out) || num_chains < 1 || chain_offset < 0)
    return fail(h, AMH_EINVAL, "amh_init: bad arguments");
  h->big_ready_C = -1;  // a kept proposal belongs to a state this call may overwrite
  h->ext_ready_C = -1;
  if (int rc = use_device(h, "amh_init")) return rc;
  amh::InitParams p{};
  p.out = *out;
  p.C = num_chains;
  p.chain_offset = chain_offset;
  p.d = h->cfg.dim;
  p.key0 = key[0];
  p.key1 = key[1];
  p.init_z = init_z;
  p.model = h->model;
  hipError_t e;
  if (h->model_id == AMH_MODEL_EXTERNAL && p.d > 64) {
    e = amh::run_big_init(p, (hipStream_t)stream);  // pe0 = 0: the caller evaluates U(z0)
  } else if (amh::big_model(h->model_id, p.d)) {
    e = amh::run_big_init(p, (hipStream_t)stream);
    if (e == hipSuccess) {
      amh::PotParams q{out->z, out->potential_energy, num_chains, p.d, h->model};
      e = amh::run_big_potential(q, (hipStream_t)stream);
    }
  } else if (h->model_id == AMH_MODEL_EXTERNAL) {
    e = amh::run_init_nopot(p, (hipStream_t)stream);  // pe0 = 0: the caller evaluates U(z0)
  } else if (amh::split_model(h->model_id, p.d)) {
    // pe0 = U(z0) from the lane-per-chain potential (bit-identical to the group one)
    e = amh::run_init_nopot(p, (hipStream_t)stream);
    if (e == hipSuccess) {
      amh::PotParams q{out->z, out->potential_energy, num_chains, p.d, h->model, h->xpack};
      e = amh::run_potential_lane(h->model_id, q, (hipStream_t)stream);
    }
  } else {
    e = amh::run_init(h->model_id, p, (hipStream_t)stream);
  }
  if (e != hipSuccess) return hip_fail(h, e, "amh_init");
  return AMH_OK;
}

int amh_step_chained(amh_handle* h, int64_t num_chains, const amh_state* in, const amh_state* out,
                     int32_t n_steps, const amh_collect* collect, int32_t flags, void* stream) {
  if (int rc = enter(h, "amh_step", true)) return rc;
  if (!state_ok(in) || !state_ok(out) || num_chains < 1 || n_steps < 0)
    return fail(h, AMH_EINVAL, "amh_step: bad arguments");
  if (h->model_id == AMH_MODEL_EXTERNAL)
    return fail(h, AMH_EINVAL, "amh_step: an external potential runs through amh_propose / amh_step_external");
  if (n_steps == 0) {
    h->big_ready_C = -1;  // a kept proposal never survives a call it was not used in
    return AMH_OK;
  }
  if (collect && collect->thinning < 1) return fail(h, AMH_EINVAL, "amh_step: thinning must be >= 1");
  if (int rc = use_device(h, "amh_step")) return rc;
  amh::StepParams p = step_params(h, num_chains, *in, *out, n_steps, collect);
  const int64_t C = num_chains;
  const hipStream_t s = (hipStream_t)stream;
  if (amh::big_model(h->model_id, p.d)) {
    // d > 64: propose pass, MFMA potential, step pass per transition
    amh::BigParams q = big_params(h, C, *in, *out, collect);
    return run_chained(h, p, 4 * (size_t)p.d + 1, flags, stream, "amh_step(d > 64)",
                       [&](const amh_state& from, Slot slot, bool propose, bool next) {
                         q.xprop = h->split.as<float>();
                         q.wa = q.xprop + (size_t)C * p.d;
                         q.wr = q.wa + (size_t)C * p.d;
                         q.dg = q.wr + (size_t)C * p.d;
                         float* pep = q.dg + (size_t)C * p.d;
                         q.pep = pep;
                         q.in = from;
                         q.col_z = slot.z;
                         q.col_pe = slot.pe;
                         hipError_t e = propose ? amh::run_big_propose(q, s) : hipSuccess;
                         if (e == hipSuccess) {
                           amh::PotParams pp{q.xprop, pep, C, p.d, h->model};
                           e = amh::run_big_potential(pp, s);
                         }
                         if (e == hipSuccess) e = amh::run_big_step(q, s, next);
                         return e;
                       });
  }
  if (amh::split_model(h->model_id, p.d)) {
    // one transition = propose, batched potential, step(U(z') from memory)
    amh::StepParams q = p;
    q.n_steps = 1;
    q.thinning = 1;
    return run_chained(h, p, (size_t)p.d + 1, flags, stream, "amh_step(split)",
                       [&](const amh_state& from, Slot slot, bool propose, bool next) {
                         float* xprop = h->split.as<float>();
                         float* peprop = xprop + (size_t)C * p.d;
                         q.ext_z = xprop;
                         q.ext_pe = peprop;
                         q.in = from;
                         q.col_z = slot.z;
                         q.col_pe = slot.pe;
                         q.xprop_next = next ? xprop : nullptr;
                         hipError_t e = propose ? amh::run_propose(q, xprop, s) : hipSuccess;
                         if (e == hipSuccess) {
                           amh::PotParams pp{xprop, peprop, C, p.d, h->model, h->xpack};
                           e = amh::run_potential_lane(h->model_id, pp, s);
                         }
                         if (e == hipSuccess) e = amh::run_step_ext(q, s);
                         return e;
                       });
  }
  if (step64_shape(h)) {
    p.descending = step64_order(h, p);
    p.chained = step64_chained(h, p);
    const hipError_t eh = step64_heads(h, p, s);
    if (eh != hipSuccess) return hip_fail(h, eh, "amh_step(d = 64 head words)");
  }
  const hipError_t e = amh::run_step(h->model_id, p, s);
  if (e != hipSuccess) return hip_fail(h, e, "amh_step");
  if (step64_shape(h)) step64_launched(h, p);
  return AMH_OK;
}

int amh_step(amh_handle* h, int64_t num_chains, const amh_state* in, const amh_state* out, int32_t n_steps,
             const amh_collect* collect, void* stream) {
  return amh_step_chained(h, num_chains, in, out, n_steps, collect, 0, stream);
}

int amh_potential(amh_handle* h, const float* z, float* pe, int64_t n, void* stream) {
  if (int rc = enter(h, "amh_potential", true)) return rc;
  if (!z || !pe || n < 1) return fail(h, AMH_EINVAL, "amh_potential: bad arguments");
  if (h->model_id == AMH_MODEL_EXTERNAL) return fail(h, AMH_EINVAL, "amh_potential: the potential is external");
  if (int rc = use_device(h, "amh_potential")) return rc;
  amh::PotParams p{z, pe, n, h->cfg.dim, h->model, h->xpack};
  const hipError_t e = amh::big_model(h->model_id, p.d) ? amh::run_big_potential(p, (hipStream_t)stream)
                       : amh::split_model(h->model_id, p.d)
                           ? amh::run_potential_lane(h->model_id, p, (hipStream_t)stream)
                           : amh::run_potential(h->model_id, p, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(h, e, "amh_potential");
  return AMH_OK;
}

int amh_sample_pnx(amh_handle* h, const uint32_t key[2], const float* x, int64_t n_points, int64_t n_samples,
                   const float* loc, const float* scale_packed, float log_step_size, int32_t n, float* out,
                   void* stream) {
  (void)loc;  // the frozen kernel's proposal does not read the mean (arwmh.py:166-167)
  if (int rc = enter(h, "amh_sample_pnx", true)) return rc;
  if (!key || !x || !scale_packed || !out || n_points < 1 || n_samples < 1 || n < 0)
    return fail(h, AMH_EINVAL, "amh_sample_pnx: bad arguments");
  if (h->cfg.dim > 64 && !amh::big_model(h->model_id, h->cfg.dim))
    return fail(h, AMH_EINVAL, "amh_sample_pnx: d > 64 needs the dense Gaussian (d <= 256)");
  if (h->model_id == AMH_MODEL_EXTERNAL)
    return fail(h, AMH_EINVAL, "amh_sample_pnx: an external potential runs through amh_pnx_propose / amh_pnx_accept");
  if (int rc = use_device(h, "amh_sample_pnx")) return rc;
  amh::PnxParams p{};
  p.x = x;
  p.n_points = n_points;
  p.n_samples = n_samples;
  p.scale = scale_packed;
  p.log_step_size = log_step_size;
  p.eps = h->cfg.eps;
  p.n = n;
  p.d = h->cfg.dim;
  p.key0 = key[0];
  p.key1 = key[1];
  p.out = out;
  p.model = h->model;
  const hipError_t e =
      (p.d > 64) ? amh::run_big_pnx(p, (hipStream_t)stream) : amh::run_pnx(h->model_id, p, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(h, e, "amh_sample_pnx");
  return AMH_OK;
}

int amh_chain_keys(const uint32_t key[2], int64_t chain_offset, int64_t n, uint32_t* out, void* stream) {
  if (!key || !out || n < 1 || chain_offset < 0) return fail(nullptr, AMH_EINVAL, "amh_chain_keys: bad arguments");
  hipError_t e = amh::run_chain_keys(key[0], key[1], chain_offset, n, out, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(nullptr, e, "amh_chain_keys");
  return AMH_OK;
}

}  // extern "C"

// ------------------------------------------------------ external potential --
// AMH_MODEL_EXTERNAL: the split transition (amh_split.hip propose_kernel,
// the step kernel with U(z') read from memory -- the diamonds path's two
// launches) with the caller's U in between.
namespace {

// d > 64: big_propose_kernel / big_step_kernel with the caller's U(z'); the
// proposals live in the caller's zprop, the solves (wa, wr) and the diagonal
// in the handle's scratch, tied to the state they were formed from
int ext_big_params(amh_handle* h, int64_t C, const amh_state* in, const amh_state* out, float* zprop,
                   const amh_collect* collect, void* stream, amh::BigParams* q) {
  const int d = h->cfg.dim;
  const size_t need = (size_t)C * (size_t)(3 * d) * sizeof(float);
  const bool grown = need > h->split.bytes;
  if (int rc = h->split.grow(h, need, stream, "amh_propose")) return rc;
  if (grown) h->ext_ready_C = -1;
  h->big_ready_C = -1;  // the scratch now holds the external path's solves
  *q = big_params(h, C, *in, *out, collect);
  q->xprop = zprop;
  q->wa = h->split.as<float>();
  q->wr = q->wa + (size_t)C * d;
  q->dg = q->wr + (size_t)C * d;
  return AMH_OK;
}

// sample_Pnx around the caller's potential (d <= 64): the propose or the accept pass of step t
int pnx_ext(amh_handle* h, const uint32_t key[2], float* z, float* pe, int64_t C, const float* scale, float lam,
            int32_t t, float* zprop, const float* pe_prop, bool accept, void* stream, const char* who) {
  if (int rc = enter(h, who, false)) return rc;
  if (h->model_id != AMH_MODEL_EXTERNAL) return fail(h, AMH_EINVAL, std::string(who) + ": needs AMH_MODEL_EXTERNAL");
  if (h->cfg.dim > 64) return fail(h, AMH_EINVAL, std::string(who) + ": an external sample_Pnx needs d <= 64");
  if (!key || !z || !zprop || C < 1 || t < 0 || (accept ? (!pe || !pe_prop) : !scale))
    return fail(h, AMH_EINVAL, std::string(who) + ": bad arguments");
  if (int rc = use_device(h, who)) return rc;
  amh::PnxExtParams p{};
  p.z = z;
  p.pe = pe;
  p.zprop = zprop;
  p.pe_prop = pe_prop;
  p.C = C;
  p.scale = scale;
  p.log_step_size = lam;
  p.eps = h->cfg.eps;
  p.t = t;
  p.d = h->cfg.dim;
  p.key0 = key[0];
  p.key1 = key[1];
  const hipError_t e = amh::run_pnx_ext(p, accept, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(h, e, who);
  return AMH_OK;
}

}  // namespace

extern "C" {

int amh_propose(amh_handle* h, int64_t num_chains, const amh_state* in, float* zprop, void* stream) {
  if (int rc = enter(h, "amh_propose", false)) return rc;
  if (h->model_id != AMH_MODEL_EXTERNAL) return fail(h, AMH_EINVAL, "amh_propose: needs AMH_MODEL_EXTERNAL");
  if (!state_ok(in) || !zprop || num_chains < 1) return fail(h, AMH_EINVAL, "amh_propose: bad arguments");
  if (int rc = use_device(h, "amh_propose")) return rc;
  if (h->cfg.dim > 64) {
    amh::BigParams q;
    if (int rc = ext_big_params(h, num_chains, in, in, zprop, nullptr, stream, &q)) return rc;
    const hipError_t e = amh::run_big_propose(q, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(h, e, "amh_propose(d > 64)");
    h->ext_ready_C = num_chains;
    h->ext_ready_in = *in;
    return AMH_OK;
  }
  const amh::StepParams p = step_params(h, num_chains, *in, *in, 1, nullptr);
  const hipError_t e = amh::run_propose(p, zprop, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(h, e, "amh_propose");
  return AMH_OK;
}

int amh_step_external(amh_handle* h, int64_t num_chains, const amh_state* in, const amh_state* out,
                      const float* zprop, const float* pe_prop, float* zprop_next, const amh_collect* collect,
                      void* stream) {
  if (int rc = enter(h, "amh_step_external", false)) return rc;
  if (h->model_id != AMH_MODEL_EXTERNAL)
    return fail(h, AMH_EINVAL, "amh_step_external: needs AMH_MODEL_EXTERNAL");
  if (!state_ok(in) || !state_ok(out) || !zprop || !pe_prop || num_chains < 1)
    return fail(h, AMH_EINVAL, "amh_step_external: bad arguments");
  if (collect && collect->thinning != 1) return fail(h, AMH_EINVAL, "amh_step_external: thinning must be 1");
  if (int rc = use_device(h, "amh_step_external")) return rc;
  if (h->cfg.dim > 64) {
    // the step pass reads the solves amh_propose (or the previous step) formed
    // for exactly this state, and writes the next proposals in place
    if (h->ext_ready_C != num_chains || !same_buffers(*in, h->ext_ready_in))
      return fail(h, AMH_EINVAL, "amh_step_external: d > 64 needs the proposals of this state (amh_propose first)");
    if (zprop_next && zprop_next != zprop)
      return fail(h, AMH_EINVAL, "amh_step_external: d > 64 forms the next proposals in place (zprop_next == zprop)");
    amh::BigParams q;
    if (int rc = ext_big_params(h, num_chains, in, out, const_cast<float*>(zprop), collect, stream, &q)) return rc;
    q.pep = pe_prop;
    h->ext_ready_C = -1;
    const hipError_t e = amh::run_big_step(q, (hipStream_t)stream, zprop_next != nullptr);
    if (e != hipSuccess) return hip_fail(h, e, "amh_step_external(d > 64)");
    if (zprop_next) {
      h->ext_ready_C = num_chains;
      h->ext_ready_in = *out;
    }
    return AMH_OK;
  }
  amh::StepParams p = step_params(h, num_chains, *in, *out, 1, collect);
  p.ext_z = zprop;
  p.ext_pe = pe_prop;
  p.xprop_next = zprop_next;
  const hipError_t e = amh::run_step_ext(p, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(h, e, "amh_step_external");
  return AMH_OK;
}

int amh_pnx_propose(amh_handle* h, const uint32_t key[2], const float* z, int64_t num_chains,
                    const float* scale_packed, float log_step_size, int32_t t, float* zprop, void* stream) {
  return pnx_ext(h, key, const_cast<float*>(z), nullptr, num_chains, scale_packed, log_step_size, t, zprop, nullptr,
                 false, stream, "amh_pnx_propose");
}

int amh_pnx_accept(amh_handle* h, const uint32_t key[2], float* z, float* pe, int64_t num_chains,
                   const float* zprop, const float* pe_prop, int32_t t, void* stream) {
  return pnx_ext(h, key, z, pe, num_chains, nullptr, 0.0f, t, const_cast<float*>(zprop), pe_prop, true, stream,
                 "amh_pnx_accept");
}

}  // extern "C"

// -------------------------------------------------------------------- ASSS --
namespace {

bool asss_state_ok(const amh_state* s) {
  return s && s->i && s->z && s->potential_energy && s->loc && s->scale && s->as_change && s->rng_key;
}

}  // namespace

extern "C" {

int amh_asss_step(amh_handle* h, int64_t num_chains, const amh_state* in, const amh_state* out, int32_t n_steps,
                  const amh_collect* collect, void* stream) {
  if (int rc = enter(h, "amh_asss_step", true)) return rc;
  if (!asss_state_ok(in) || !asss_state_ok(out) || num_chains < 1 || n_steps < 0)
    return fail(h, AMH_EINVAL, "amh_asss_step: bad arguments");
  const bool big = amh::big_model(h->model_id, h->cfg.dim);
  if (h->cfg.dim > 64 && !big)
    return fail(h, AMH_EINVAL, "amh_asss_step: dim must be <= 64, or a dense Gaussian up to 256");
  if (h->model_id == AMH_MODEL_EXTERNAL)
    return fail(h, AMH_EINVAL, "amh_asss_step: the slice sampler needs a device potential (not external)");
  if (collect && collect->thinning < 1) return fail(h, AMH_EINVAL, "amh_asss_step: thinning must be >= 1");
  if (n_steps == 0) return AMH_OK;
  if (int rc = use_device(h, "amh_asss_step")) return rc;
  amh::StepParams p = step_params(h, num_chains, *in, *out, n_steps, collect);
  p.accept_count = nullptr;
  if (big) {
    // large d: one launch per transition (the factor streamed four times),
    // the first from `in`, the rest in place on `out`
    for (int32_t t = 0; t < n_steps; ++t) {
      amh::StepParams q = p;
      if (t > 0) q.in = *out;
      q.n_steps = 1;
      const Slot slot = collect_slot(p, t);
      q.col_z = slot.z;
      q.col_pe = slot.pe;
      const hipError_t e = amh::run_asss_big_step(q, (hipStream_t)stream);
      if (e != hipSuccess) return hip_fail(h, e, "amh_asss_step(large d)");
    }
    return AMH_OK;
  }
  if (step64_shape(h)) {
    p.descending = step64_order(h, p);
    p.chained = step64_chained(h, p);
  }
  const hipError_t e = amh::run_asss_step(h->model_id, p, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(h, e, "amh_asss_step");
  if (step64_shape(h)) step64_launched(h, p);
  return AMH_OK;
}

int amh_asss_sample_pnx(amh_handle* h, const uint32_t key[2], const float* x, int64_t n_points, int64_t n_samples,
                        const float* loc, const float* scale_packed, int32_t n, float* out, void* stream) {
  if (int rc = enter(h, "amh_asss_sample_pnx", true)) return rc;
  if (!key || !x || !loc || !scale_packed || !out || n_points < 1 || n_samples < 1 || n < 0)
    return fail(h, AMH_EINVAL, "amh_asss_sample_pnx: bad arguments");
  const bool big = amh::big_model(h->model_id, h->cfg.dim);
  if (h->cfg.dim > 64 && !big)
    return fail(h, AMH_EINVAL, "amh_asss_sample_pnx: dim must be <= 64, or a dense Gaussian up to 256");
  if (h->model_id == AMH_MODEL_EXTERNAL)
    return fail(h, AMH_EINVAL, "amh_asss_sample_pnx: the slice sampler needs a device potential (not external)");
  if (int rc = use_device(h, "amh_asss_sample_pnx")) return rc;
  amh::AsssPnxParams p{};
  p.x = x;
  p.n_points = n_points;
  p.n_samples = n_samples;
  p.loc = loc;
  p.scale = scale_packed;
  p.eps = h->cfg.eps;
  p.n = n;
  p.d = h->cfg.dim;
  p.key0 = key[0];
  p.key1 = key[1];
  p.out = out;
  p.model = h->model;
  const hipError_t e =
      big ? amh::run_asss_big_pnx(p, (hipStream_t)stream) : amh::run_asss_pnx(h->model_id, p, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(h, e, "amh_asss_sample_pnx");
  return AMH_OK;
}

}  // extern "C"

// ------------------------------------------- ASSS, the caller's potential --
// amh_asss_ext.hip: the transition cut at every potential evaluation
namespace {

// every entry's checks of the handle, reported under its public name `who`
int asss_ext_enter(amh_handle* h, const char* who) {
  if (int rc = enter(h, who, false)) return rc;
  if (h->model_id != AMH_MODEL_EXTERNAL) return fail(h, AMH_EINVAL, std::string(who) + ": needs AMH_MODEL_EXTERNAL");
  if (h->cfg.dim > 64) return fail(h, AMH_EINVAL, std::string(who) + ": the external slice sampler needs d <= 64");
  return AMH_OK;
}

amh::AsssExtParams asss_ext_params(const amh_handle* h, int64_t C, const amh_state& in, const amh_state& out,
                                   const amh_collect* collect, const float* cand, const float* work,
                                   int32_t* active) {
  amh::AsssExtParams q{};
  q.sp = step_params(h, C, in, out, 1, collect);
  q.sp.accept_count = nullptr;
  q.cand = const_cast<float*>(cand);
  q.work = const_cast<float*>(work);
  q.active = active;
  return q;
}

int asss_ext_begin(amh_handle* h, amh::AsssExtParams& q, bool frozen, void* stream, const char* who) {
  if (int rc = use_device(h, who)) return rc;
  hipError_t e = hipMemsetAsync(q.active, 0, AMH_ASSS_EXT_ROUNDS * sizeof(int32_t), (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(h, e, std::string(who) + "/hipMemsetAsync");
  e = amh::run_asss_ext_begin(q, frozen, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(h, e, who);
  return AMH_OK;
}

}  // namespace

extern "C" {

int amh_asss_ext_work_size(int32_t dim, int64_t* floats_per_chain) {
  if (dim < 1 || dim > 64 || !floats_per_chain)
    return fail(nullptr, AMH_EINVAL, "amh_asss_ext_work_size: dim must be in [1, 64]");
  *floats_per_chain = amh::asss_ext_work_floats(dim);
  return AMH_OK;
}

int amh_asss_ext_begin(amh_handle* h, int64_t num_chains, const amh_state* in, float* cand, float* work,
                       int32_t* active, void* stream) {
  if (int rc = asss_ext_enter(h, "amh_asss_ext_begin")) return rc;
  if (!asss_state_ok(in) || !cand || !work || !active || num_chains < 1)
    return fail(h, AMH_EINVAL, "amh_asss_ext_begin: bad arguments");
  amh::AsssExtParams q = asss_ext_params(h, num_chains, *in, *in, nullptr, cand, work, active);
  return asss_ext_begin(h, q, false, stream, "amh_asss_ext_begin");
}

int amh_asss_ext_shrink(amh_handle* h, int64_t num_chains, const float* pe, int32_t round, float* cand, float* work,
                        int32_t* active, void* stream) {
  if (int rc = asss_ext_enter(h, "amh_asss_ext_shrink")) return rc;
  if (!pe || !cand || !work || !active || num_chains < 1)
    return fail(h, AMH_EINVAL, "amh_asss_ext_shrink: bad arguments");
  if (round < 0 || round >= AMH_ASSS_EXT_ROUNDS)
    return fail(h, AMH_EINVAL, "amh_asss_ext_shrink: round must be in [0, 50]");
  if (int rc = use_device(h, "amh_asss_ext_shrink")) return rc;
  amh::AsssExtParams q = asss_ext_params(h, num_chains, amh_state{}, amh_state{}, nullptr, cand, work, active);
  q.pe = pe;
  q.round = round;
  const hipError_t e = amh::run_asss_ext_shrink(q, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(h, e, "amh_asss_ext_shrink");
  return AMH_OK;
}

int amh_asss_ext_finish(amh_handle* h, int64_t num_chains, const amh_state* in, const amh_state* out,
                        const float* cand, const float* work, const amh_collect* collect, void* stream) {
  if (int rc = asss_ext_enter(h, "amh_asss_ext_finish")) return rc;
  if (!asss_state_ok(in) || !asss_state_ok(out) || !cand || !work || num_chains < 1)
    return fail(h, AMH_EINVAL, "amh_asss_ext_finish: bad arguments");
  if (collect && collect->thinning != 1) return fail(h, AMH_EINVAL, "amh_asss_ext_finish: thinning must be 1");
  if (int rc = use_device(h, "amh_asss_ext_finish")) return rc;
  const amh::AsssExtParams q = asss_ext_params(h, num_chains, *in, *out, collect, cand, work, nullptr);
  const hipError_t e = amh::run_asss_ext_finish(q, false, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(h, e, "amh_asss_ext_finish");
  return AMH_OK;
}

int amh_asss_ext_pnx_begin(amh_handle* h, const uint32_t key[2], const float* x_cur, int64_t num_chains,
                           const float* loc, const float* scale_packed, int32_t t, float* cand, float* work,
                           int32_t* active, void* stream) {
  if (int rc = asss_ext_enter(h, "amh_asss_ext_pnx_begin")) return rc;
  if (!key || !x_cur || !loc || !scale_packed || !cand || !work || !active || num_chains < 1 || t < 0)
    return fail(h, AMH_EINVAL, "amh_asss_ext_pnx_begin: bad arguments");
  amh::AsssExtParams q = asss_ext_params(h, num_chains, amh_state{}, amh_state{}, nullptr, cand, work, active);
  q.x_cur = const_cast<float*>(x_cur);
  q.loc = loc;
  q.scale = scale_packed;
  q.key0 = key[0];
  q.key1 = key[1];
  q.t = t;
  return asss_ext_begin(h, q, true, stream, "amh_asss_ext_pnx_begin");
}

int amh_asss_ext_pnx_finish(amh_handle* h, int64_t num_chains, const float* cand, const float* work, float* x_cur,
                            void* stream) {
  if (int rc = asss_ext_enter(h, "amh_asss_ext_pnx_finish")) return rc;
  if (!cand || !work || !x_cur || num_chains < 1)
    return fail(h, AMH_EINVAL, "amh_asss_ext_pnx_finish: bad arguments");
  if (int rc = use_device(h, "amh_asss_ext_pnx_finish")) return rc;
  amh::AsssExtParams q = asss_ext_params(h, num_chains, amh_state{}, amh_state{}, nullptr, cand, work, nullptr);
  q.x_cur = x_cur;
  const hipError_t e = amh::run_asss_ext_finish(q, true, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(h, e, "amh_asss_ext_pnx_finish");
  return AMH_OK;
}

}  // extern "C"

// -------------------------------------------------------------- evaluation --
extern "C" {

int64_t amh_kernel_sum_scratch(int64_t n, int64_t m) { return n > 0 && m > 0 ? amh::kernel_sum_blocks(n, m) : 0; }

int amh_kernel_sum(const float* a, int64_t n, const float* b, int64_t m, int32_t d, float gamma, int32_t skip_diag,
                   double* scratch, double* out, void* stream) {
  if (!a || !b || !scratch || !out || n < 1 || m < 1 || d < 1)
    return fail(nullptr, AMH_EINVAL, "amh_kernel_sum: bad arguments");
  const hipError_t e = amh::run_kernel_sum(a, n, b, m, d, gamma, skip_diag, scratch, out, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(nullptr, e, "amh_kernel_sum");
  return AMH_OK;
}

int amh_pairwise_dist2(const float* a, int64_t n, const float* b, int64_t m, int32_t d, float* out, void* stream) {
  if (!a || !b || !out || n < 1 || m < 1 || d < 1) return fail(nullptr, AMH_EINVAL, "amh_pairwise_dist2: bad arguments");
  const hipError_t e = amh::run_dist2(a, n, b, m, d, out, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(nullptr, e, "amh_pairwise_dist2");
  return AMH_OK;
}

int amh_sinkhorn_lse(const float* cost, int64_t rows, int64_t cols, const float* pot, float log_w, float eps,
                     float* out, void* stream) {
  if (!cost || !pot || !out || rows < 1 || cols < 1 || !(eps > 0.0f) || rows > 0x7FFFFFFF)
    return fail(nullptr, AMH_EINVAL, "amh_sinkhorn_lse: bad arguments");
  const hipError_t e = amh::run_lse_rows(cost, rows, cols, pot, log_w, eps, out, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(nullptr, e, "amh_sinkhorn_lse");
  return AMH_OK;
}

int amh_normals(const uint32_t key[2], int64_t n, float* out, void* stream) {
  if (!key || !out || n < 0) return fail(nullptr, AMH_EINVAL, "amh_normals: bad arguments");
  if (n == 0) return AMH_OK;
  const hipError_t e = amh::run_normals(key[0], key[1], n, out, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(nullptr, e, "amh_normals");
  return AMH_OK;
}

// linear assignment by auction (amh_assign.hip)
int amh_assign_work_size(int64_t n, int64_t* bytes) {
  if (!bytes || n < 1 || n > amh::kAssignMaxN)
    return fail(nullptr, AMH_EINVAL, "amh_assign_work_size: n must be in 1 .. 65536");
  *bytes = amh::assign_work_bytes(n);
  return AMH_OK;
}

namespace {
bool assign_args_ok(const void* work, int64_t n) {
  return work && ((uintptr_t)work & 7u) == 0 && n >= 1 && n <= amh::kAssignMaxN;
}
}  // namespace

int amh_assign_begin(const float* cost, int64_t n, void* work, void* stream) {
  if (!cost || ((uintptr_t)cost & 3u) != 0 || !assign_args_ok(work, n))
    return fail(nullptr, AMH_EINVAL, "amh_assign_begin: bad arguments (square float32 costs, 1 <= n <= 65536)");
  const hipError_t e = amh::run_assign_begin(cost, n, work, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(nullptr, e, "amh_assign_begin");
  return AMH_OK;
}

int amh_assign_quantum(const void* work, int64_t n, int32_t* e_out, int64_t* qmax, void* stream) {
  if (!assign_args_ok(work, n) || !e_out || !qmax) return fail(nullptr, AMH_EINVAL, "amh_assign_quantum: bad arguments");
  int64_t hdr[amh::kAssignHdrWords];
  const hipError_t e = amh::run_assign_header(work, hdr, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(nullptr, e, "amh_assign_quantum");
  if (hdr[1] != 0)
    return fail(nullptr, AMH_EINVAL, "amh_assign_quantum: the cost matrix holds a NaN, an infinity or a negative entry");
  *e_out = (int32_t)hdr[2];
  *qmax = hdr[3];
  return AMH_OK;
}

int amh_assign_phase(void* work, int64_t n, void* stream) {
  if (!assign_args_ok(work, n)) return fail(nullptr, AMH_EINVAL, "amh_assign_phase: bad arguments");
  const hipError_t e = amh::run_assign_phase(work, n, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(nullptr, e, "amh_assign_phase");
  return AMH_OK;
}

int amh_assign_rounds(const float* cost, int64_t n, void* work, int64_t eps, int64_t bound, int64_t first,
                      int32_t rounds, void* stream) {
  if (!cost || ((uintptr_t)cost & 3u) != 0 || !assign_args_ok(work, n) || eps < 1 || bound < 1 || bound > n ||
      first < 0 || rounds < 0 || rounds > 65536)
    return fail(nullptr, AMH_EINVAL, "amh_assign_rounds: bad arguments");
  const hipError_t e = amh::run_assign_rounds(cost, n, work, eps, bound, first, rounds, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(nullptr, e, "amh_assign_rounds");
  return AMH_OK;
}

int amh_assign_status(const void* work, int64_t n, int64_t queued, int64_t* unassigned, int64_t* rounds,
                      void* stream) {
  if (!assign_args_ok(work, n) || queued < 0 || !unassigned || !rounds)
    return fail(nullptr, AMH_EINVAL, "amh_assign_status: bad arguments");
  int64_t hdr[amh::kAssignHdrWords];
  const hipError_t e = amh::run_assign_header(work, hdr, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(nullptr, e, "amh_assign_status");
  *unassigned = hdr[5 + (queued & 1)];
  *rounds = hdr[4];
  return AMH_OK;
}

int amh_assign_result(const void* work, int64_t n, int64_t* perm, int64_t* price, void* stream) {
  if (!assign_args_ok(work, n) || (!perm && !price)) return fail(nullptr, AMH_EINVAL, "amh_assign_result: bad arguments");
  const hipError_t e = amh::run_assign_result(work, n, perm, price, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(nullptr, e, "amh_assign_result");
  return AMH_OK;
}

// streaming posterior summaries (amh_summary.hip)
int amh_summary_update(const float* x, int64_t num_draws, int64_t num_chains, int32_t num_cols, const float* calib,
                       int32_t nbins, int64_t batch, int64_t n_before, double* acc, int64_t* hist, void* stream) {
  if (!x || !calib || !acc || !hist || ((uintptr_t)x & 3u) != 0 || ((uintptr_t)calib & 3u) != 0 ||
      ((uintptr_t)acc & 7u) != 0 || ((uintptr_t)hist & 7u) != 0)
    return fail(nullptr, AMH_EINVAL, "amh_summary_update: null or misaligned buffer");
  if (num_draws < 1 || num_chains < 1 || num_cols < 1 || num_cols > 1024)
    return fail(nullptr, AMH_EINVAL, "amh_summary_update: num_draws >= 1, num_chains >= 1, 1 <= num_cols <= 1024");
  if (nbins < 64 || nbins > 2048 || (nbins & (nbins - 1)) != 0)
    return fail(nullptr, AMH_EINVAL, "amh_summary_update: nbins must be a power of two in 64 .. 2048");
  if (batch < 1 || n_before < 0) return fail(nullptr, AMH_EINVAL, "amh_summary_update: batch >= 1, n_before >= 0");
  if (num_draws > INT64_MAX / num_chains / num_cols)
    return fail(nullptr, AMH_EINVAL, "amh_summary_update: the block's element count overflows int64");
  const hipError_t e = amh::run_summary_update(x, num_draws, num_chains, num_cols, calib, nbins, batch, n_before, acc,
                                               hist, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(nullptr, e, "amh_summary_update");
  return AMH_OK;
}

}  // extern "C"

// ------------------------------------------------------- pooled covariance --
namespace {

bool pooled_ok(const amh_pooled_state* s) {
  return s && s->i && s->z && s->potential_energy && s->rng_key && s->mean_accept_prob && s->loc && s->scale &&
         s->log_step_size && s->as_change && s->cov;
}

// the handle's chunk-partial scratch: n_chunks rows plus the reduction's group
// sums, a row being the sums themselves or, at d >= 64 (`big`), their tile layout
int reserve_partials(amh_handle* h, int64_t n_chunks, bool big, void* stream, const char* who) {
  const int64_t vrow = big ? amh::pooled_big_tile_V(h->cfg.dim) : amh::pooled_sums_len(h->cfg.dim);
  return h->partials.grow(h, (size_t)amh::pooled_scratch_rows(n_chunks) * (size_t)vrow * sizeof(double), stream, who);
}

// d >= 64: the update's staging; the post kernel's arrival ticket in it starts
// at zero (its last block resets it)
int reserve_update_scratch(amh_handle* h, void* stream, const char* who) {
  return h->upd.grow(h, amh::pooled_update_scratch_floats(h->cfg.dim) * sizeof(float), stream, who, true);
}

// d >= 64: room for the noise the update launch draws ahead for C chains; the
// records of a new buffer say i = -1, which matches no chain
int reserve_noise(amh_handle* h, int64_t C, void* stream, const char* who) {
  const size_t need = (size_t)C * amh::noise_row_bytes(h->cfg.dim);
  if (need <= h->noise.bytes) return AMH_OK;
  if (int rc = h->noise.grow(h, need, stream, who)) return rc;
  h->noise_cap = C;
  const hipError_t e = hipMemsetAsync(h->noise.ptr, 0xFF, (size_t)C * amh::kNoiseRecordBytes, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(h, e, std::string(who) + "/hipMemsetAsync");
  return AMH_OK;
}

// d = 64 with prep_for_update: the last step's chunk partials are left
// unreduced; *deferred describes them for the update launch, which reduces
// them first (one launch fewer per pooled block)
struct DeferredReduce {
  const float* partials = nullptr;
  int64_t n_chunks = 0;
  int32_t accumulate = 0;
};

// exact sums: the chunk a rank must be aligned to, from the chain count of all
// ranks.  The lane-per-row form cuts 16 pooled_cpw(total) chains, the MFMA
// form 128; d = 64 has both (the Gaussian and a caller's potential on MFMA,
// the other registry models lane per row), and a multiple of either serves
int64_t exact_chunk_chains(int d, int64_t total_chains) {
  const int64_t lane = (int64_t)amh::kPoolWaves * amh::pooled_cpw(total_chains);
  if (d < 64) return lane;
  if (d > 64) return 128;
  int64_t m = 128;
  while (m % lane != 0) m += 128;
  return m;
}

// the entry's partial rows, as the stats launch has just left them, into the
// exact words
int exact_reduce(amh_handle* h, int64_t n_chunks, bool big, int64_t* acc, int accumulate, void* stream,
                 const char* who) {
  const int d = h->cfg.dim;
  const int64_t vrow = big ? amh::pooled_big_tile_V(d) : amh::pooled_sums_len(d);
  const hipError_t e = amh::run_pooled_exact_reduce(h->partials.ptr, big, n_chunks, vrow, big ? d : 0, acc, accumulate,
                                                    (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(h, e, std::string(who) + "(exact reduce)");
  return AMH_OK;
}

// The chains and the shared state of `in` as a stats-side kernel's parameters
// (PooledStatsParams, PooledExtParams): the fields both carry.  The
// lane-per-row chunks are cut by total_chains (the chains of all ranks under
// exact sums, else num_chains).
template <class P>
P pooled_params(const amh_handle* h, int64_t num_chains, const amh_pooled_state* in, int64_t total_chains) {
  P p{};
  p.C = num_chains;
  p.cpw = amh::pooled_cpw(total_chains);
  p.d = h->cfg.dim;
  p.i = in->i;
  p.z = in->z;
  p.pe = in->potential_energy;
  p.keys = in->rng_key;
  p.mu = in->loc;
  p.L = in->scale;
  p.lam = in->log_step_size;
  p.eps = h->cfg.eps;
  return p;
}

// ... and the update's, from the handle's adaptation settings
amh::PooledUpdateParams pooled_update_params(const amh_handle* h, const double* sums, const amh_pooled_state* in,
                                             const amh_pooled_state* out, int32_t k_steps) {
  amh::PooledUpdateParams p{};
  p.d = h->cfg.dim;
  p.W = h->cfg.num_warmup;
  p.a = h->cfg.lr_decay;
  p.target = h->cfg.target_accept_prob;
  p.sums = sums;
  p.in = *in;
  p.out = *out;
  p.K = k_steps;
  return p;
}

// prep_for_update: the update follows in the same library call with no
// exchange in between (amh_pooled_step_k on one rank), so the large-d
// reduction's last kernel also forms that update's Sigma'.
// exact_acc: the partial rows go to the exact words there instead of `sums`
// (unused), the lane-per-row chunks cut by total_chains, the chains of all ranks
int pooled_stats_impl(amh_handle* h, int64_t num_chains, const amh_pooled_state* in, int32_t k_steps, float* z_out,
                      float* pe_out, double* sums, void* stream, bool prep_for_update, bool* sigma_ready,
                      DeferredReduce* deferred = nullptr, bool pack_ready = false, int64_t* exact_acc = nullptr,
                      int64_t total_chains = 0) {
  const char* const who = exact_acc ? "amh_pooled_stats_k_exact" : "amh_pooled_stats";
  if (sigma_ready) *sigma_ready = false;
  if (deferred) *deferred = DeferredReduce{};
  if (int rc = enter(h, who, true)) return rc;
  if (!pooled_ok(in) || !z_out || !pe_out || (!sums && !exact_acc) || num_chains < 1 || k_steps < 1)
    return fail(h, AMH_EINVAL, std::string(who) + ": bad arguments");
  if (exact_acc) {
    sums = nullptr;
    if (total_chains < num_chains) return fail(h, AMH_EINVAL, std::string(who) + ": total_chains < num_chains");
    // N of a chunk, k_steps * its chains, must be a float32 value like every other partial
    if ((int64_t)k_steps * amh::kPoolWaves * 16 > ((int64_t)1 << 24))
      return fail(h, AMH_EINVAL, std::string(who) + ": k_steps too large for exact sums");
  } else {
    total_chains = num_chains;
  }
  if (int rc = check_device_flag(h)) return rc;
  if (int rc = use_device(h, who)) return rc;
  const int d = h->cfg.dim;
  const bool big = amh::pooled_big_model(h->model_id, d);
  if (d > 64 && !big) return fail(h, AMH_EINVAL, "amh_pooled_stats: d > 64 needs d % 32 == 0 in the pooled mode");
  if (h->model_id == AMH_MODEL_EXTERNAL)
    return fail(h, AMH_EINVAL, "amh_pooled_stats: the pooled mode needs a device potential (not external)");
  const int cpw = amh::pooled_cpw(total_chains);
  const int64_t chunk = (int64_t)amh::kPoolWaves * cpw;
  const int64_t n_chunks = big ? amh::pooled_big_chunks(num_chains, d) : (num_chains + chunk - 1) / chunk;
  if (int rc = reserve_partials(h, n_chunks, big, stream, who)) return rc;
  amh::PooledStatsParams p = pooled_params<amh::PooledStatsParams>(h, num_chains, in, total_chains);
  p.z_out = z_out;
  p.pe_out = pe_out;
  p.partials = h->partials.as<double>();
  p.model = h->model;
  p.k_steps = k_steps;
  if (!big) {
    const hipError_t e = amh::run_pooled_stats(h->model_id, p, sums, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(h, e, "amh_pooled_stats");
    return exact_acc ? exact_reduce(h, n_chunks, false, exact_acc, 0, stream, who) : AMH_OK;
  }
  // the fused path's A-operand copies
  h->big_ready_C = -1;
  void* const split_was = h->split.ptr;
  if (int rc = h->split.grow(h, (size_t)amh::pooled_big_pack_floats(d) * sizeof(float), stream, who)) return rc;
  // the copies are current only when the previous update of this call wrote
  // them into this very buffer (amh_pooled_step_k; d > 64 fused path)
  p.pack_ready = (pack_ready && d != 64 && h->split.ptr == split_was) ? 1 : 0;
  // noise drawn ahead by the update launch (records checked per chain
  // by the stats kernel, so a stale or foreign buffer is never used)
  if (int rc = reserve_noise(h, num_chains, stream, who)) return rc;
  p.xrec = h->noise.as<const uint4>();
  p.xi = amh::noise_xi(h->noise.as<float>(), h->noise_cap);
  p.xi_cap = h->noise_cap;
  h->noise_C = num_chains;
  h->noise_keys = in->rng_key;
  if (prep_for_update)  // grown here: pooled_update_impl's grow is then a no-op
    if (int rc = reserve_update_scratch(h, stream, who)) return rc;
  // one launch sequence per step of the block, the sums accumulated; d = 64:
  // the block's K steps in one launch (pooled_fused64_kernel, p.k_steps)
  const int32_t n_launch = (d == 64) ? 1 : k_steps;
  for (int32_t t0 = 0; t0 < n_launch; ++t0) {
    const int32_t t = (d == 64) ? k_steps - 1 : t0;  // the step the launch ends with
    p.i_add = (d == 64) ? 0 : t;
    p.accumulate = (d == 64) ? 0 : t > 0;
    if (prep_for_update && d != 64 && t == k_steps - 1) {
      p.prep.cov = in->cov;
      p.prep.i = in->i;
      p.prep.scratch = h->upd.as<float>();
      p.prep.N = (double)num_chains * (double)k_steps;
      p.prep.W = h->cfg.num_warmup;
      p.prep.K = k_steps;
      p.prep.a = h->cfg.lr_decay;
      if (sigma_ready) *sigma_ready = true;
    }
    if (t0 > 0) {
      p.z = z_out;
      p.pe = pe_out;
    }
    p.defer_reduce = (prep_for_update && deferred && d == 64 && t == k_steps - 1 &&
                      !diag_env_off("AMH_POOLED_FUSED_REDUCE"))  // =0 keeps the d = 64 reduction in its own launch
                         ? 1
                         : 0;
    if (p.defer_reduce) {
      deferred->partials = h->partials.as<const float>();
      deferred->n_chunks = n_chunks;
      deferred->accumulate = p.accumulate;
    }
    const hipError_t e = amh::run_pooled_big_stats(p, h->split.as<float>(), sums, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(h, e, "amh_pooled_stats(MFMA path)");
    if (exact_acc)
      if (int rc = exact_reduce(h, n_chunks, true, exact_acc, p.accumulate, stream, who)) return rc;
    p.pack_ready = 1;  // the K steps of a pooled block share the frozen factor
  }
  return AMH_OK;
}

int pooled_update_impl(amh_handle* h, const double* sums, const amh_pooled_state* in, const amh_pooled_state* out,
                       int32_t k_steps, void* stream, bool sigma_ready, const DeferredReduce* deferred = nullptr,
                       float* pack_out = nullptr) {
  const char* const who = "amh_pooled_update";
  if (int rc = enter(h, who, false)) return rc;
  if (!sums || !pooled_ok(in) || !pooled_ok(out)) return fail(h, AMH_EINVAL, "amh_pooled_update: bad arguments");
  if (k_steps < 1 || h->cfg.num_warmup % k_steps != 0)
    return fail(h, AMH_EINVAL, "amh_pooled_update: k_steps must be >= 1 and divide num_warmup");
  if (h->cfg.dim > 64 && !amh::pooled_big_model(h->model_id, h->cfg.dim))
    return fail(h, AMH_EINVAL, "amh_pooled_update: d > 64 needs d % 32 == 0 in the pooled mode");
  if (int rc = check_device_flag(h)) return rc;
  if (int rc = use_device(h, who)) return rc;
  amh::PooledUpdateParams p = pooled_update_params(h, sums, in, out, k_steps);
  hipError_t e;
  if (amh::pooled_big_model(h->model_id, p.d)) {
    if (int rc = reserve_update_scratch(h, stream, who)) return rc;
    p.scratch = h->upd.as<float>();
    if (p.d == 64 && h->err_host == nullptr) {
      e = hipHostMalloc((void**)&h->err_host, sizeof(int), hipHostMallocMapped);
      if (e == hipSuccess) {
        *h->err_host = 0;
        e = hipHostGetDevicePointer((void**)&h->err_dev, h->err_host, 0);
      }
      if (e != hipSuccess) return hip_fail(h, e, "amh_pooled_update/hipHostMalloc");
    }
    p.err_flag = h->err_dev;
    p.pack_out = (p.d > 64) ? pack_out : nullptr;
    if (h->noise.ptr && h->noise_C > 0 && h->noise_C <= h->noise_cap && in->rng_key == h->noise_keys &&
        !diag_env_off("AMH_POOLED_NOISE_AHEAD")) {  // =0 draws no noise ahead (each stats kernel draws its own)
      p.noise_C = h->noise_C;  // the chains (and keys) of the stats call this update follows
      p.keys = (const uint32_t*)in->rng_key;
      p.xrec = h->noise.as<uint4>();
      p.xi = amh::noise_xi(h->noise.as<float>(), h->noise_cap);
    }
    if (deferred && deferred->partials) {
      p.red_partials = deferred->partials;
      p.red_chunks = deferred->n_chunks;
      p.red_accumulate = deferred->accumulate;
      p.red_blocks = amh::pooled_reduce64_blocks(amh::pooled_big_tile_V(p.d));
      p.sums_out = const_cast<double*>(sums);
    }
    e = amh::run_pooled_big_update(p, (hipStream_t)stream, sigma_ready);
  } else {
    e = amh::run_pooled_update(p, (hipStream_t)stream);
  }
  if (e != hipSuccess) return hip_fail(h, e, "amh_pooled_update");
  return AMH_OK;
}

// The pooled transition around the caller's potential.  Nothing is kept in
// the handle between the two calls: with the shared L the proposal is a
// product over chains (no per-chain solves), and the accept pass reads the
// proposals and regenerates u from (key, i + t).
int pooled_ext_params(amh_handle* h, int64_t num_chains, const amh_pooled_state* in, int32_t t, const char* who,
                      amh::PooledExtParams* p) {
  if (int rc = enter(h, who, false)) return rc;
  if (h->model_id != AMH_MODEL_EXTERNAL) return fail(h, AMH_EINVAL, std::string(who) + ": needs AMH_MODEL_EXTERNAL");
  const int d = h->cfg.dim;
  if (d > 64 && !amh::pooled_big_model(h->model_id, d))
    return fail(h, AMH_EINVAL, std::string(who) + ": d > 64 needs d % 32 == 0 in the pooled mode");
  if (!pooled_ok(in) || num_chains < 1 || t < 0) return fail(h, AMH_EINVAL, std::string(who) + ": bad arguments");
  *p = pooled_params<amh::PooledExtParams>(h, num_chains, in, num_chains);
  p->t = t;
  return AMH_OK;
}

// the accept pass of `p` and its sums: the double reduction into `sums`, or
// (acc non-null) the partial rows into the exact words
int pooled_ext_stats(amh_handle* h, amh::PooledExtParams& p, const float* zprop, const float* pe_prop, float* z_out,
                     float* pe_out, double* sums, int64_t* acc, int32_t accumulate, void* stream, const char* who) {
  const bool big = amh::pooled_big_model(h->model_id, p.d);
  const int64_t n_chunks = amh::pooled_ext_chunks(p.C, p.d, p.cpw);
  if (int rc = reserve_partials(h, n_chunks, big, stream, who)) return rc;
  p.zprop = const_cast<float*>(zprop);
  p.pe_prop = pe_prop;
  p.z_out = z_out;
  p.pe_out = pe_out;
  p.partials = h->partials.as<double>();
  const hipError_t e = amh::run_pooled_ext_stats(p, acc ? nullptr : sums, accumulate != 0, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(h, e, who);
  return acc ? exact_reduce(h, n_chunks, big, acc, accumulate != 0, stream, who) : AMH_OK;
}

// ncclAllReduce / ncclGetErrorString of the RCCL instance already in the
// process (the caller created `comm` with it: torch's librccl.so.1, found by
// soname without loading anything), else the system librccl.so.1
typedef int (*nccl_allreduce_fn)(const void*, void*, size_t, int, int, void*, void*);
typedef const char* (*nccl_errstr_fn)(int);
void* rccl_handle() {
  static void* hd = nullptr;
  if (hd == nullptr) {
    hd = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
    if (hd == nullptr) hd = dlopen("librccl.so", RTLD_NOW | RTLD_NOLOAD);
    if (hd == nullptr) hd = dlopen("librccl.so.1", RTLD_NOW);
  }
  return hd;
}

// in-place ncclAllReduce(sum) of n elements of RCCL type `dtype`, as the entry `who`
int pooled_allreduce(amh_handle* h, void* buf, int64_t n, int dtype, void* rccl_comm, void* stream, const char* who) {
  if (int rc = enter(h, who, false)) return rc;
  if (!buf || !rccl_comm || n < 0) return fail(h, AMH_EINVAL, std::string(who) + ": null sums / communicator");
  void* hd = rccl_handle();
  auto ar = hd ? (nccl_allreduce_fn)dlsym(hd, "ncclAllReduce") : nullptr;
  if (ar == nullptr) return fail(h, AMH_EHIP, std::string(who) + ": librccl not found");
  constexpr int kNcclSum = 0;
  const int rc = ar(buf, buf, (size_t)n, dtype, kNcclSum, rccl_comm, stream);
  if (rc != 0) {
    auto es = (nccl_errstr_fn)dlsym(hd, "ncclGetErrorString");
    return fail(h, AMH_EHIP, std::string(who) + ": ncclAllReduce: " + (es ? es(rc) : "error") + " (ncclResult " +
                                 std::to_string(rc) + ")");
  }
  return AMH_OK;
}

}  // namespace

extern "C" {

int amh_pooled_sums_size(int32_t dim, int64_t* v) {
  if (dim < 1 || dim > 256 || !v) return fail(nullptr, AMH_EINVAL, "amh_pooled_sums_size: bad arguments");
  *v = amh::pooled_sums_len(dim);
  return AMH_OK;
}

int amh_pooled_stats_k(amh_handle* h, int64_t num_chains, const amh_pooled_state* in, int32_t k_steps,
                       float* z_out, float* pe_out, double* sums, void* stream) {
  return pooled_stats_impl(h, num_chains, in, k_steps, z_out, pe_out, sums, stream, false, nullptr);
}

int amh_pooled_stats(amh_handle* h, int64_t num_chains, const amh_pooled_state* in, float* z_out, float* pe_out,
                     double* sums, void* stream) {
  return amh_pooled_stats_k(h, num_chains, in, 1, z_out, pe_out, sums, stream);
}

int amh_pooled_update_k(amh_handle* h, const double* sums, const amh_pooled_state* in, const amh_pooled_state* out,
                        int32_t k_steps, void* stream) {
  return pooled_update_impl(h, sums, in, out, k_steps, stream, false);
}

int amh_pooled_update(amh_handle* h, const double* sums, const amh_pooled_state* in, const amh_pooled_state* out,
                      void* stream) {
  return amh_pooled_update_k(h, sums, in, out, 1, stream);
}

int amh_pooled_step_k(amh_handle* h, int64_t num_chains, const amh_pooled_state* in, const amh_pooled_state* out,
                      int32_t n_steps, int32_t sync_every, double* sums, void* stream) {
  if (int rc = enter(h, "amh_pooled_step", false)) return rc;
  if (n_steps < 0 || sync_every < 1 || n_steps % sync_every != 0)
    return fail(h, AMH_EINVAL, "amh_pooled_step: n_steps must be a non-negative multiple of sync_every");
  if (!pooled_ok(in) || !pooled_ok(out) || !sums) return fail(h, AMH_EINVAL, "amh_pooled_step: bad arguments");
  const amh_pooled_state* src = in;
  const bool big = h->model_id && amh::pooled_big_model(h->model_id, h->cfg.dim) && h->cfg.dim > 64;
  for (int32_t t = 0; t < n_steps; t += sync_every) {
    bool ready = false;  // one rank, no exchange: the reduction also forms Sigma'
    DeferredReduce dr;   // (d = 64: or is left to the update launch)
    // d > 64: from the second block on, the stats launch's A-operand copy of
    // the factor was written by the previous update's post kernel
    int rc = pooled_stats_impl(h, num_chains, src, sync_every, out->z, out->potential_energy, sums, stream, true,
                               &ready, &dr, t > 0);
    if (rc != AMH_OK) return rc;
    rc = pooled_update_impl(h, sums, src, out, sync_every, stream, ready, &dr,
                            (big && t + sync_every < n_steps) ? h->split.as<float>() : nullptr);
    if (rc != AMH_OK) return rc;
    src = out;
  }
  return AMH_OK;
}

int amh_pooled_step(amh_handle* h, int64_t num_chains, const amh_pooled_state* in, const amh_pooled_state* out,
                    int32_t n_steps, double* sums, void* stream) {
  return amh_pooled_step_k(h, num_chains, in, out, n_steps, 1, sums, stream);
}

int amh_pooled_propose(amh_handle* h, int64_t num_chains, const amh_pooled_state* in, int32_t t, float* zprop,
                       void* stream) {
  amh::PooledExtParams p;
  if (int rc = pooled_ext_params(h, num_chains, in, t, "amh_pooled_propose", &p)) return rc;
  if (!zprop) return fail(h, AMH_EINVAL, "amh_pooled_propose: bad arguments");
  if (int rc = use_device(h, "amh_pooled_propose")) return rc;
  p.zprop = zprop;
  const hipError_t e = amh::run_pooled_ext_propose(p, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(h, e, "amh_pooled_propose");
  return AMH_OK;
}

int amh_pooled_stats_external(amh_handle* h, int64_t num_chains, const amh_pooled_state* in, int32_t t,
                              const float* zprop, const float* pe_prop, float* z_out, float* pe_out, double* sums,
                              int32_t accumulate, void* stream) {
  const char* const who = "amh_pooled_stats_external";
  amh::PooledExtParams p;
  if (int rc = pooled_ext_params(h, num_chains, in, t, who, &p)) return rc;
  if (!zprop || !pe_prop || !z_out || !pe_out || !sums)
    return fail(h, AMH_EINVAL, "amh_pooled_stats_external: bad arguments");
  if (int rc = use_device(h, who)) return rc;
  return pooled_ext_stats(h, p, zprop, pe_prop, z_out, pe_out, sums, nullptr, accumulate, stream, who);
}

int amh_pooled_stats_external_exact(amh_handle* h, int64_t num_chains, int64_t total_chains,
                                    const amh_pooled_state* in, int32_t t, const float* zprop, const float* pe_prop,
                                    float* z_out, float* pe_out, int64_t* acc, int32_t accumulate, void* stream) {
  const char* const who = "amh_pooled_stats_external_exact";
  amh::PooledExtParams p;
  if (int rc = pooled_ext_params(h, num_chains, in, t, who, &p)) return rc;
  if (!zprop || !pe_prop || !z_out || !pe_out || !acc || total_chains < num_chains)
    return fail(h, AMH_EINVAL, "amh_pooled_stats_external_exact: bad arguments");
  if (int rc = use_device(h, who)) return rc;
  p.cpw = amh::pooled_cpw(total_chains);
  return pooled_ext_stats(h, p, zprop, pe_prop, z_out, pe_out, nullptr, acc, accumulate, stream, who);
}

int amh_pooled_allreduce(amh_handle* h, double* sums, int64_t n, void* rccl_comm, void* stream) {
  constexpr int kNcclFloat64 = 8;
  return pooled_allreduce(h, sums, n, kNcclFloat64, rccl_comm, stream, "amh_pooled_allreduce");
}

int amh_pooled_allreduce_i64(amh_handle* h, int64_t* acc, int64_t n, void* rccl_comm, void* stream) {
  constexpr int kNcclInt64 = 4;
  return pooled_allreduce(h, acc, n, kNcclInt64, rccl_comm, stream, "amh_pooled_allreduce_i64");
}

int amh_pooled_exact_size(int32_t dim, int64_t* n) {
  if (dim < 1 || dim > 256 || !n) return fail(nullptr, AMH_EINVAL, "amh_pooled_exact_size: bad arguments");
  *n = amh::pooled_sums_len(dim) * amh::kExactWords;
  return AMH_OK;
}

int amh_pooled_chunk_chains(int32_t dim, int64_t total_chains, int64_t* n) {
  if (dim < 1 || dim > 256 || (dim > 64 && dim % 32 != 0) || total_chains < 1 || !n)
    return fail(nullptr, AMH_EINVAL, "amh_pooled_chunk_chains: bad arguments");
  *n = exact_chunk_chains(dim, total_chains);
  return AMH_OK;
}

int amh_pooled_stats_k_exact(amh_handle* h, int64_t num_chains, int64_t total_chains, const amh_pooled_state* in,
                             int32_t k_steps, float* z_out, float* pe_out, int64_t* acc, void* stream) {
  if (h && !acc) return fail(h, AMH_EINVAL, "amh_pooled_stats_k_exact: bad arguments");
  return pooled_stats_impl(h, num_chains, in, k_steps, z_out, pe_out, nullptr, stream, false, nullptr, nullptr, false,
                           acc, total_chains);
}

int amh_pooled_exact_to_sums(amh_handle* h, const int64_t* acc, double* sums, void* stream) {
  const char* const who = "amh_pooled_exact_to_sums";
  if (int rc = enter(h, who, false)) return rc;
  if (!acc || !sums) return fail(h, AMH_EINVAL, "amh_pooled_exact_to_sums: bad arguments");
  if (int rc = use_device(h, who)) return rc;
  const hipError_t e = amh::run_pooled_exact_convert(acc, amh::pooled_sums_len(h->cfg.dim), sums, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(h, e, who);
  return AMH_OK;
}

int amh_pooled_exact_quantise(const float* partials, int64_t rows, int64_t v, int64_t* acc, int32_t accumulate) {
  if (rows < 0 || v < 0 || !acc || (rows > 0 && v > 0 && !partials))
    return fail(nullptr, AMH_EINVAL, "amh_pooled_exact_quantise: bad arguments");
  for (int64_t c = 0; c < v; ++c) {
    int64_t w[amh::kExactWords];
    for (int j = 0; j < amh::kExactWords; ++j) w[j] = accumulate ? acc[c * amh::kExactWords + j] : 0;
    for (int64_t r = 0; r < rows; ++r) amh::exact_add(w, partials[r * v + c]);
    for (int j = 0; j < amh::kExactWords; ++j) acc[c * amh::kExactWords + j] = w[j];
  }
  return AMH_OK;
}

int amh_pooled_exact_to_double(const int64_t* acc, int64_t v, double* out) {
  if (v < 0 || (v > 0 && (!acc || !out))) return fail(nullptr, AMH_EINVAL, "amh_pooled_exact_to_double: bad arguments");
  for (int64_t c = 0; c < v; ++c) {
    int64_t w[amh::kExactWords];
    for (int j = 0; j < amh::kExactWords; ++j) w[j] = acc[c * amh::kExactWords + j];
    out[c] = amh::exact_to_double(w);
  }
  return AMH_OK;
}

}  // extern "C"

// ------------------------------------------------------------- pooled ASSS --
// The slice transition against the shared factor (amh_pooled_asss.hip) and
// the ASSS form of the d <= 64 update; the sums, their reduction and the
// exchange are the pooled mode's own.
namespace {

// the checks the three entries share, reported as `who`
int pooled_asss_enter(amh_handle* h, const char* who) {
  if (int rc = enter(h, who, true)) return rc;
  if (h->model_id == AMH_MODEL_EXTERNAL)
    return fail(h, AMH_EINVAL, std::string(who) + ": the slice sampler needs a device potential (not external)");
  if (h->cfg.dim > 64) return fail(h, AMH_EINVAL, std::string(who) + ": dim must be <= 64");
  if (!amh::pooled_asss_model(h->model_id, h->cfg.dim))
    return fail(h, AMH_EINVAL, std::string(who) + ": no pooled slice kernel for this model and dim");
  return AMH_OK;
}

int pooled_asss_stats_impl(amh_handle* h, int64_t num_chains, const amh_pooled_state* in, int32_t k_steps,
                           float* z_out, float* pe_out, double* sums, void* stream, const char* who) {
  if (!pooled_ok(in) || !z_out || !pe_out || !sums || num_chains < 1 || k_steps < 1)
    return fail(h, AMH_EINVAL, std::string(who) + ": bad arguments");
  if (int rc = use_device(h, who)) return rc;
  const int cpw = amh::pooled_cpw(num_chains);
  const int64_t chunk = (int64_t)amh::kPoolWaves * cpw;
  const int64_t n_chunks = (num_chains + chunk - 1) / chunk;
  if (int rc = reserve_partials(h, n_chunks, false, stream, who)) return rc;
  amh::PooledStatsParams p = pooled_params<amh::PooledStatsParams>(h, num_chains, in, num_chains);
  p.z_out = z_out;
  p.pe_out = pe_out;
  p.partials = h->partials.as<double>();
  p.model = h->model;
  p.k_steps = k_steps;
  const hipError_t e = amh::run_pooled_asss_stats(h->model_id, p, sums, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(h, e, who);
  return AMH_OK;
}

int pooled_asss_update_impl(amh_handle* h, const double* sums, const amh_pooled_state* in,
                            const amh_pooled_state* out, int32_t k_steps, void* stream, const char* who) {
  if (!sums || !pooled_ok(in) || !pooled_ok(out)) return fail(h, AMH_EINVAL, std::string(who) + ": bad arguments");
  if (k_steps < 1 || h->cfg.num_warmup % k_steps != 0)
    return fail(h, AMH_EINVAL, std::string(who) + ": k_steps must be >= 1 and divide num_warmup");
  if (int rc = use_device(h, who)) return rc;
  const amh::PooledUpdateParams p = pooled_update_params(h, sums, in, out, k_steps);
  const hipError_t e = amh::run_pooled_update(p, (hipStream_t)stream, true);
  if (e != hipSuccess) return hip_fail(h, e, who);
  return AMH_OK;
}

// ... and the checks of the entries around a caller's potential
int pooled_asss_ext_enter(amh_handle* h, const char* who) {
  if (int rc = enter(h, who, false)) return rc;
  if (h->model_id != AMH_MODEL_EXTERNAL) return fail(h, AMH_EINVAL, std::string(who) + ": needs AMH_MODEL_EXTERNAL");
  if (h->cfg.dim > 64) return fail(h, AMH_EINVAL, std::string(who) + ": dim must be <= 64");
  return AMH_OK;
}

}  // namespace

extern "C" {

int amh_pooled_asss_ext_begin(amh_handle* h, int64_t num_chains, const amh_pooled_state* in, int32_t t, float* cand,
                              float* work, int32_t* active, void* stream) {
  const char* const who = "amh_pooled_asss_ext_begin";
  if (int rc = pooled_asss_ext_enter(h, who)) return rc;
  amh::PooledAsssExtParams q{};
  if (int rc = pooled_ext_params(h, num_chains, in, t, who, &q.sp)) return rc;
  if (!cand || !work || !active) return fail(h, AMH_EINVAL, std::string(who) + ": bad arguments");
  if (int rc = use_device(h, who)) return rc;
  q.cand = cand;
  q.work = work;
  hipError_t e = hipMemsetAsync(active, 0, AMH_ASSS_EXT_ROUNDS * sizeof(int32_t), (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(h, e, std::string(who) + "/hipMemsetAsync");
  e = amh::run_pooled_asss_ext_begin(q, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(h, e, who);
  return AMH_OK;
}

int amh_pooled_asss_ext_finish(amh_handle* h, int64_t num_chains, const amh_pooled_state* in, const float* cand,
                               const float* work, float* z_out, float* pe_out, double* sums, int32_t accumulate,
                               void* stream) {
  const char* const who = "amh_pooled_asss_ext_finish";
  if (int rc = pooled_asss_ext_enter(h, who)) return rc;
  amh::PooledAsssExtParams q{};
  if (int rc = pooled_ext_params(h, num_chains, in, 0, who, &q.sp)) return rc;
  if (!cand || !work || !z_out || !pe_out || !sums) return fail(h, AMH_EINVAL, std::string(who) + ": bad arguments");
  if (int rc = use_device(h, who)) return rc;
  const int64_t chunk = (int64_t)amh::kPoolWaves * q.sp.cpw;
  const int64_t n_chunks = (num_chains + chunk - 1) / chunk;
  if (int rc = reserve_partials(h, n_chunks, false, stream, who)) return rc;
  q.cand = const_cast<float*>(cand);
  q.work = const_cast<float*>(work);
  q.sp.z_out = z_out;
  q.sp.pe_out = pe_out;
  q.sp.partials = h->partials.as<double>();
  const hipError_t e = amh::run_pooled_asss_ext_finish(q, sums, accumulate != 0, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(h, e, who);
  return AMH_OK;
}

int amh_pooled_asss_ext_update(amh_handle* h, const double* sums, const amh_pooled_state* in,
                               const amh_pooled_state* out, int32_t k_steps, void* stream) {
  const char* const who = "amh_pooled_asss_ext_update";
  if (int rc = pooled_asss_ext_enter(h, who)) return rc;
  return pooled_asss_update_impl(h, sums, in, out, k_steps, stream, who);
}

int amh_pooled_asss_stats_k(amh_handle* h, int64_t num_chains, const amh_pooled_state* in, int32_t k_steps,
                            float* z_out, float* pe_out, double* sums, void* stream) {
  const char* const who = "amh_pooled_asss_stats_k";
  if (int rc = pooled_asss_enter(h, who)) return rc;
  return pooled_asss_stats_impl(h, num_chains, in, k_steps, z_out, pe_out, sums, stream, who);
}

int amh_pooled_asss_update_k(amh_handle* h, const double* sums, const amh_pooled_state* in,
                             const amh_pooled_state* out, int32_t k_steps, void* stream) {
  const char* const who = "amh_pooled_asss_update_k";
  if (int rc = pooled_asss_enter(h, who)) return rc;
  return pooled_asss_update_impl(h, sums, in, out, k_steps, stream, who);
}

int amh_pooled_asss_step_k(amh_handle* h, int64_t num_chains, const amh_pooled_state* in, const amh_pooled_state* out,
                           int32_t n_steps, int32_t sync_every, double* sums, void* stream) {
  const char* const who = "amh_pooled_asss_step_k";
  if (int rc = pooled_asss_enter(h, who)) return rc;
  if (n_steps < 0 || sync_every < 1 || n_steps % sync_every != 0)
    return fail(h, AMH_EINVAL, std::string(who) + ": n_steps must be a non-negative multiple of sync_every");
  if (!pooled_ok(in) || !pooled_ok(out) || !sums) return fail(h, AMH_EINVAL, std::string(who) + ": bad arguments");
  const amh_pooled_state* src = in;
  for (int32_t t = 0; t < n_steps; t += sync_every) {
    int rc = pooled_asss_stats_impl(h, num_chains, src, sync_every, out->z, out->potential_energy, sums, stream, who);
    if (rc != AMH_OK) return rc;
    rc = pooled_asss_update_impl(h, sums, src, out, sync_every, stream, who);
    if (rc != AMH_OK) return rc;
    src = out;
  }
  return AMH_OK;
}

}  // extern "C"

// ------------------------------------------------------------- diagnostics --
#ifdef AMH_STAMPS
extern "C" {

// diagnostic build only: copy the step kernel's per-wave phase stamps
int amh_diag_stamps(void* host, int64_t bytes) {
  return amh::diag_stamps_copy(host, (size_t)bytes) == hipSuccess ? 0 : -1;
}
// the d = 64 step kernel's per-wave records (amh_step64.hip: 8 x u64 per wave)
int amh_diag_s64_stamps(void* host, int64_t bytes) {
  return amh::diag_s64_stamps_copy(host, (size_t)bytes) == hipSuccess ? 0 : -1;
}
// pooled large-d update kernel phase totals (8 x u64)
int amh_diag_upd_stamps(void* host) { return amh::diag_upd_stamps_copy(host) == hipSuccess ? 0 : -1; }
// pooled d = 64 fused stats kernel phase totals (16 x u64, block 0 thread 0)
int amh_diag_f64_stamps(void* host) { return amh::diag_f64_stamps_copy(host) == hipSuccess ? 0 : -1; }
// pooled d = 64 update launch timeline (16 x u64, 100 MHz clock; copied, then cleared)
int amh_diag_u64_timeline(void* host) { return amh::diag_u64_timeline_copy(host) == hipSuccess ? 0 : -1; }

}  // extern "C"
#endif
