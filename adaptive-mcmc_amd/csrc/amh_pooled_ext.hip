// amh_pooled_ext.hip -- the pooled-covariance transition (regime B) split
// around the caller's potential (AMH_MODEL_EXTERNAL): amh_pooled_propose
// writes every chain's proposal with the shared (L, lambda), the caller
// evaluates U there, and amh_pooled_stats_external accepts and forms the
// step's sums.  Per chain and per sum the float operations and their order
// are those of the fused kernels with U(z') read instead of computed
// (oracle: orc_pooled_stats_k's lane-per-row form below d = 64,
// orc_pooled_stats_big from d = 64 up), so amh_pooled_update_k consumes the
// sums unchanged.
//
//   pooled_ext_propose_kernel      d < 64: the factor staged in LDS, one chain
//                                  per wave pass (pooled_stats_kernel up to zp)
//   pooled_ext_stats_kernel        d < 64: accept + the chunk's sums, registers
//                                  and the LDS tree of pooled_stats_kernel
//   pooled_ext_propose_big_kernel  d = 32 NT >= 64: Z' = Z + e^lam (L Xi) + eps Xi
//                                  over 64-chain tiles on v_mfma_f32_32x32x2_f32
//                                  (phases (1)-(2) of the fused kernels)
//   pooled_ext_stats_big_kernel    d = 32 NT >= 64: accept, then S_dd of a
//                                  128-chain chunk on MFMA, S_d / S_a sequential
//                                  (phases (4)-(6)), tile-order partial rows
// The chunk partials go through the reductions of the fused paths
// (pooled_reduce, launch_reduce_tiles), whose `accumulate` adds a step's sums
// to the block's.
#include "amh_device.h"
#include "amh_pooled_device.h"

namespace amh {

namespace {
typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int kLd = 65;        // LDS row stride of [k][chain] tiles
constexpr int kTile = 64;      // chains per proposal tile / stats half
constexpr int kPropWaves = 4;  // waves of the MFMA proposal block
constexpr int kStatWaves = 8;  // waves of the MFMA stats block
}  // namespace

// ---------------------------------------------------------------- d < 64 --
// Wave w of block b takes the chains b * 16 + w, + 16 gridDim.x, ..: the
// proposal of a chain depends on no other chain, so any assignment gives the
// same bits.
__global__ __launch_bounds__(kPoolWaves * 64) void pooled_ext_propose_kernel(PooledExtParams p) {
  constexpr int G = 64;
  extern __shared__ float lds[];
  const int d = p.d;
  const int ld = pooled_ld(d);
  pooled_stage_factor(lds, p.L, d);
  __syncthreads();

  const int r = lane_id();
  const bool act = r < d;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64));
  const int32_t it = __builtin_amdgcn_readfirstlane(p.i[0] + p.t);
  const float el = amh_expf(p.lam[0]);
  const uint32_t prow = lds_addr(lds + (act ? r : 0) * ld);
  const uint32_t vr = 4u * (uint32_t)r;
  const int64_t stride = (int64_t)gridDim.x * kPoolWaves;
  for (int64_t c = (int64_t)blockIdx.x * kPoolWaves + w; c < p.C; c += stride) {
    // (buffer descriptors with a wave-uniform base: lanes r >= d read 0 /
    // store nothing)
    const Buf bz(uniform_ptr(p.z + c * d), 4u * (uint32_t)d);
    const float z = bz.ld(vr, 0);
    const uint32_t k0 = p.keys[2 * c], k1 = p.keys[2 * c + 1];
    // noise at the shared stream position i + t (arwmh.py:162-165)
    float xi, u;
    step_noise<G>(r, d, (uint32_t)it, k0, k1, xi, u);
    xi = act ? xi : 0.0f;
    // proposal with the shared factor (arwmh.py:166-167)
    const float acc = lds_row_dot64(prow, d, xi, act);
    const float zp = act ? z + fmaf(el, acc, p.eps * xi) : 0.0f;
    const Buf bo(uniform_ptr(p.zprop + c * d), 4u * (uint32_t)d);
    bo.st(zp, vr, 0);
  }
}

// The chunk layout of pooled_stats_kernel: block b is chunk b, wave w takes
// its chains [b 16 cpw + w cpw, + cpw) in order.
__global__ __launch_bounds__(kPoolWaves * 64) void pooled_ext_stats_kernel(PooledExtParams p) {
  extern __shared__ float tree[];
  const int d = p.d;
  const int64_t V = pooled_sums_len(d);
  const int r = lane_id();
  const bool act = r < d;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64));
  const int32_t it = __builtin_amdgcn_readfirstlane(p.i[0] + p.t);
  const float mu = act ? p.mu[r] : 0.0f;

  const int cpw = p.cpw;
  const int64_t chunk0 = (int64_t)blockIdx.x * kPoolWaves * cpw;
  const int64_t base = chunk0 + (int64_t)w * cpw;
  const int64_t end = (base + cpw < p.C) ? base + cpw : p.C;
  float S[64];
  static_for<64>([&](auto K) { S[K] = 0.0f; });
  float sd = 0.0f, sa = 0.0f;
  const uint32_t vr = 4u * (uint32_t)r;
  for (int64_t c = base; c < end; ++c) {
    const Buf bz(uniform_ptr(p.z + c * d), 4u * (uint32_t)d);
    const Buf bp(uniform_ptr(p.zprop + c * d), 4u * (uint32_t)d);
    float z = bz.ld(vr, 0);
    const float zp = bp.ld(vr, 0);
    float pe = p.pe[c];
    float pep = p.pe_prop[c];
    // the accept uniform of the stream position the proposal was drawn at
    // (arwmh.py:174): word d of the step stream
    const float u = amh_unif01_from_bits(amh_step_word((uint32_t)d, (uint32_t)it, p.keys[2 * c], p.keys[2 * c + 1]));
    if (amh_isnan(pep)) pep = INFINITY;  // arwmh.py:171
    const float ex = amh_expf(pe - pep);
    const float alpha = (ex > 1.0f) ? 1.0f : ex;
    const bool accept = u < alpha;
    z = accept ? zp : z;
    pe = accept ? pep : pe;
    const float delta = act ? z - mu : 0.0f;
    pooled_accumulate(S, sd, delta, d);
    sa = sa + alpha;
    const Buf bo(uniform_ptr(p.z_out + c * d), 4u * (uint32_t)d);
    bo.st(z, vr, 0);
    if (r == 0) p.pe_out[c] = pe;
  }
  const int64_t left = p.C - chunk0;
  const int64_t full = (int64_t)kPoolWaves * cpw;
  pooled_chunk_out(S, sd, sa, tree, r, act, w, d, p.partials + (int64_t)blockIdx.x * V,
                   (double)(left < full ? left : full));
}

// --------------------------------------------------------------- d >= 64 --
// Proposal of 64-chain tiles, 4 waves; lane = (i, h), i = lane & 31, h = lane >> 5.
//   (1) noise of the chains w, w + 4, .. as a [k][chain] tile (lane =
//       coordinate k mod 64)
//   (2) acc = L xi on MFMA: job (T, hf) = row tile T, chain half hf; the A
//       operand (rows 32 T + i, columns 2 m + h of the packed factor, 0 above
//       the diagonal) straight from L2, 16 MFMAs' worth in flight; row r's
//       chain runs over k < 32 (T + 1) in k order.  Then e^lam acc + eps xi
//       over the noise tile in place, once every job has read it.
//   (3) z' = z + that, chain-major (coalesced rows of z and zprop).
template <int NT>
__global__ __launch_bounds__(64 * kPropWaves) void pooled_ext_propose_big_kernel(PooledExtParams p) {
  constexpr int D = 32 * NT;
  constexpr int NQ = (D + 63) / 64;                          // coordinates per lane, chain-major phases
  constexpr int NJ = (2 * NT + kPropWaves - 1) / kPropWaves;  // (T, hf) jobs per wave
  constexpr int CPW = kTile / kPropWaves;
  extern __shared__ float Xb[];  // [D][kLd]
  const int lane = lane_id();
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64));
  const int h = lane >> 5, i = lane & 31;
  const int32_t it = p.i[0] + p.t;
  const float el = amh_expf(p.lam[0]);
  const int64_t n_tiles = (p.C + kTile - 1) / kTile;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t c0 = tile * kTile;
    const int64_t left = p.C - c0;
    const int nv = left < kTile ? (int)left : kTile;
    // (1) (a chain past C repeats the last one: its column is never written out)
#pragma unroll 1
    for (int n = 0; n < CPW; ++n) {
      const int cc = w + kPropWaves * n;
      const int64_t ch = (cc < nv) ? c0 + cc : p.C - 1;
      float xr[NQ];
      step_noise_rows<NQ>(lane, D, (uint32_t)it, p.keys[2 * ch], p.keys[2 * ch + 1], xr);
      static_for<NQ>([&](auto Q) {
        const int k = 64 * Q + lane;
        if (k < D) Xb[k * kLd + cc] = xr[Q];
      });
    }
    __syncthreads();
    // (2)
    float v[NJ][16];
    static_for<NJ>([&](auto S) {
      const int job = w + kPropWaves * S;
      if (job < 2 * NT) {
        const int T = job >> 1, hf = job & 1;
        const int r = 32 * T + i;
        f32x16 acc = f32x16{};
#pragma unroll 1
        for (int J = 0; J <= T; ++J) {
          float a[16], b[16];
          static_for<16>([&](auto M) {
            const int k = 32 * J + 2 * M + h;
            a[M] = p.L[pk(D, r, k <= r ? k : r)];
            b[M] = Xb[k * kLd + 32 * hf + i];
          });
          static_for<16>([&](auto M) {
            const int k = 32 * J + 2 * M + h;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(k <= r ? a[M] : 0.0f, b[M], acc, 0, 0, 0);
          });
        }
        static_for<16>([&](auto R) {
          const int rr = 32 * T + mfma_row(R, h);
          v[S][R] = fmaf(el, acc[(int)R], p.eps * Xb[rr * kLd + 32 * hf + i]);
        });
      }
    });
    __syncthreads();
    static_for<NJ>([&](auto S) {
      const int job = w + kPropWaves * S;
      if (job < 2 * NT) {
        const int T = job >> 1, hf = job & 1;
        static_for<16>([&](auto R) { Xb[(32 * T + mfma_row(R, h)) * kLd + 32 * hf + i] = v[S][R]; });
      }
    });
    __syncthreads();
    // (3) xprop = z + (e^lam L xi + eps xi)
#pragma unroll 1
    for (int n = 0; n < CPW; ++n) {
      const int cc = w + kPropWaves * n;
      if (cc < nv) {
        const int64_t ch = c0 + cc;
        static_for<NQ>([&](auto Q) {
          const int k = 64 * Q + lane;
          if (k < D) p.zprop[ch * D + k] = p.z[ch * D + k] + Xb[k * kLd + cc];
        });
      }
    }
    __syncthreads();  // the next tile's noise overwrites Xb
  }
}

// Accept + sums of one 128-chain chunk per block pass, 8 waves, in two
// 64-chain halves (the S_dd accumulators stay in registers across them):
//   (4) accept (arwmh.py:173-178): wave w takes the chains w, w + 8, ..; the
//       decision is wave-uniform, lane = coordinate k mod 64
//   (5) z' out, delta = z' - mu as a [k][chain] tile (0 past the last chain)
//   (6) S_dd on MFMA, tile pairs w, w + 8, .. (pair I (I + 1) / 2 + J), each
//       accumulator an fmaf chain over the chunk's chains in order; S_d
//       (thread = coordinate) and S_a (one thread) sequential in chain order.
// The float32 partial row in the tile layout of the fused kernels: [S_d |
// S_dd tiles in register order | 2 pad | S_a | N].
template <int NT>
__global__ __launch_bounds__(64 * kStatWaves) void pooled_ext_stats_big_kernel(PooledExtParams p, int64_t n_chunks) {
  constexpr int D = 32 * NT;
  constexpr int NPAIR = NT * (NT + 1) / 2;
  constexpr int64_t V = D + (int64_t)NPAIR * 1024 + 4;
  constexpr int NS = (NPAIR + kStatWaves - 1) / kStatWaves;
  constexpr int NQ = (D + 63) / 64;
  constexpr int CPW = kTile / kStatWaves;
  extern __shared__ float lds[];
  float* Zb = lds;              // [D][kLd] delta
  float* alph = Zb + D * kLd;   // [64]
  const int tid = threadIdx.x;
  const int lane = lane_id();
  const int w = __builtin_amdgcn_readfirstlane((int)(tid / 64));
  const int h = lane >> 5, i = lane & 31;
  const int32_t it = p.i[0] + p.t;
  float mu_l[NQ];
  static_for<NQ>([&](auto Q) { mu_l[Q] = (64 * Q + lane < D) ? p.mu[64 * Q + lane] : 0.0f; });
  int sI[NS], sJ[NS];
  static_for<NS>([&](auto S) {
    const int u = w + kStatWaves * S;
    const int I = tile_pair_row(u);
    sI[S] = (u < NPAIR) ? I : -1;
    sJ[S] = u - I * (I + 1) / 2;
  });

  for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
    float* out = (float*)p.partials + chunk * V;
    f32x16 sacc[NS];
    static_for<NS>([&](auto S) { sacc[S] = f32x16{}; });
    float sd = 0.0f, sa = 0.0f;
    int cnt = 0;
#pragma unroll 1
    for (int half = 0; half < kBigChunk / kTile; ++half) {
      const int64_t c0 = chunk * kBigChunk + (int64_t)kTile * half;
      const int64_t left = p.C - c0;
      if (left <= 0) break;  // block-uniform
      const int nv = left < kTile ? (int)left : kTile;
      __syncthreads();  // the previous half's readers of Zb / alph are done
      // (4), (5)
#pragma unroll 1
      for (int n = 0; n < CPW; ++n) {
        const int cc = w + kStatWaves * n;
        if (cc < nv) {
          const int64_t ch = c0 + cc;
          const float pe = p.pe[ch];
          float pep = p.pe_prop[ch];
          const float u = amh_unif01_from_bits(amh_step_word((uint32_t)D, (uint32_t)it, p.keys[2 * ch], p.keys[2 * ch + 1]));
          if (amh_isnan(pep)) pep = INFINITY;  // arwmh.py:171
          const float ex = amh_expf(pe - pep);
          const float a = (ex > 1.0f) ? 1.0f : ex;
          const bool accept = u < a;
          const float* src = accept ? p.zprop : p.z;
          static_for<NQ>([&](auto Q) {
            const int k = 64 * Q + lane;
            if (k < D) {
              const float zn = src[ch * D + k];
              p.z_out[ch * D + k] = zn;
              Zb[k * kLd + cc] = zn - mu_l[Q];
            }
          });
          if (lane == 0) {
            p.pe_out[ch] = accept ? pep : pe;
            alph[cc] = a;
          }
        } else {
          static_for<NQ>([&](auto Q) {
            const int k = 64 * Q + lane;
            if (k < D) Zb[k * kLd + cc] = 0.0f;
          });
          if (lane == 0) alph[cc] = 0.0f;
        }
      }
      __syncthreads();
      // (6) sequential adds in chain order (the slots past nv hold +0, and
      // adding +0 to a sum that started at +0 changes no bit)
      if (tid < D) {
        static_for<4>([&](auto B) {
          float x[16];
          static_for<16>([&](auto Q) { x[Q] = Zb[tid * kLd + 16 * B + Q]; });
          static_for<16>([&](auto Q) { sd = sd + x[Q]; });
        });
      }
      if (tid == 64 * kStatWaves - 1) {
        static_for<4>([&](auto B) {
          float x[16];
          static_for<16>([&](auto Q) { x[Q] = alph[16 * B + Q]; });
          static_for<16>([&](auto Q) { sa = sa + x[Q]; });
        });
      }
      cnt += nv;
      // chain pairs (2 m, 2 m + 1) for 2 m < nv (a chain past nv in the last
      // pair holds delta = +0)
      static_for<NS>([&](auto S) {
        if (sI[S] >= 0) {
          const float* ap = Zb + (32 * sI[S] + i) * kLd + h;
          const float* bp = Zb + (32 * sJ[S] + i) * kLd + h;
          int kk = 0;
#pragma unroll 1
          for (; kk + 16 <= nv; kk += 16) {
            float a[8], b[8];
            static_for<8>([&](auto Q) {
              a[Q] = ap[kk + 2 * Q];
              b[Q] = bp[kk + 2 * Q];
            });
            static_for<8>([&](auto Q) { sacc[S] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[Q], b[Q], sacc[S], 0, 0, 0); });
          }
#pragma unroll 1
          for (; kk < nv; kk += 2) sacc[S] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk], bp[kk], sacc[S], 0, 0, 0);
        }
      });
    }
    // one coalesced 256-B row per accumulator register
    static_for<NS>([&](auto S) {
      if (sI[S] >= 0) {
        float* o = out + D + (int64_t)(w + kStatWaves * S) * 1024 + lane;
        static_for<16>([&](auto R) { o[64 * R] = sacc[S][(int)R]; });
      }
    });
    if (tid < D) out[tid] = sd;
    if (tid == 64 * kStatWaves - 1) {
      out[V - 2] = sa;
      out[V - 1] = (float)cnt;
    }
  }
}

// --------------------------------------------------------------- launchers --
namespace {
bool ext_big(int d) { return d >= 64 && d <= 256 && d % 32 == 0; }
int device_cus() {
  const int cus = cu_count();
  return cus > 0 ? cus : 1;
}
}  // namespace

hipError_t run_pooled_ext_propose(const PooledExtParams& p, hipStream_t s) {
  const int d = p.d;
  if (d < 1 || (d > 64 && !ext_big(d))) return hipErrorInvalidValue;
  if (!ext_big(d)) {
    const size_t shm = (size_t)d * pooled_ld(d) * sizeof(float);
    const int64_t want = (p.C + kPoolWaves - 1) / kPoolWaves;
    const int64_t cap = 8 * (int64_t)device_cus();
    hipLaunchKernelGGL(pooled_ext_propose_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(kPoolWaves * 64), shm,
                       s, p);
    return hipGetLastError();
  }
  const int64_t n_tiles = (p.C + kTile - 1) / kTile;
  const int64_t cap = 2 * (int64_t)device_cus();
  const unsigned grid = (unsigned)(n_tiles < cap ? n_tiles : cap);
  const size_t shm = (size_t)d * kLd * sizeof(float);
  switch (d / 32) {
#define AMH_PE(NT_)                                                                                              \
  case NT_:                                                                                                      \
    hipLaunchKernelGGL(pooled_ext_propose_big_kernel<NT_>, dim3(grid), dim3(64 * kPropWaves), shm, s, p);         \
    break;
    AMH_PE(2) AMH_PE(3) AMH_PE(4) AMH_PE(5) AMH_PE(6) AMH_PE(7) AMH_PE(8)
#undef AMH_PE
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

int64_t pooled_ext_chunks(int64_t C, int d, int cpw) {
  if (ext_big(d)) return (C + kBigChunk - 1) / kBigChunk;
  const int64_t chunk = (int64_t)kPoolWaves * cpw;
  return (C + chunk - 1) / chunk;
}

hipError_t run_pooled_ext_stats(const PooledExtParams& p, double* sums, int accumulate, hipStream_t s) {
  const int d = p.d;
  if (d < 1 || (d > 64 && !ext_big(d))) return hipErrorInvalidValue;
  const int64_t n_chunks = pooled_ext_chunks(p.C, d, p.cpw);
  if (!ext_big(d)) {
    const int64_t V = pooled_sums_len(d);
    hipLaunchKernelGGL(pooled_ext_stats_kernel, dim3((unsigned)n_chunks), dim3(kPoolWaves * 64),
                       kPooledTreeFloats * sizeof(float), s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || sums == nullptr) return e;
    return pooled_reduce(p.partials, n_chunks, V, sums, accumulate, s);
  }
  const int64_t cap = (int64_t)device_cus();
  const unsigned grid = (unsigned)(n_chunks < cap ? n_chunks : cap);
  const size_t shm = ((size_t)d * kLd + 64) * sizeof(float);
  switch (d / 32) {
#define AMH_SE(NT_)                                                                                              \
  case NT_:                                                                                                      \
    hipLaunchKernelGGL(pooled_ext_stats_big_kernel<NT_>, dim3(grid), dim3(64 * kStatWaves), shm, s, p, n_chunks); \
    break;
    AMH_SE(2) AMH_SE(3) AMH_SE(4) AMH_SE(5) AMH_SE(6) AMH_SE(7) AMH_SE(8)
#undef AMH_SE
    default:
      return hipErrorInvalidValue;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || sums == nullptr) return e;
  return launch_reduce_tiles((const float*)p.partials, n_chunks, pooled_big_tile_V(d), sums, accumulate, d, FinalPrep{},
                             s);
}

}  // namespace amh
