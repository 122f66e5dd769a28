// amh_probe.hip -- TEST-ONLY elementwise probes of the device compile of
// include/amh_math.h and of the row terms of amh_device.h (libamh_probe.so;
// not linked into libamh.so, never loaded by the product package).
//
// Every probe is a plain map, one thread per element, 256 threads per block,
// no LDS: out[i] = f(in[i]) with f the function exactly as the kernels call
// it.  tests/test_gpu_math.py compares the outputs with the gcc host compile
// (oracle/amh_oracle.c) bit for bit; the amh_probe_host_* entries are the same
// header compiled by hipcc's host clang, the compile that fills the gamma
// table in amh_create (amh_capi.hip), and need no device.
//
// Entries return 0, -1 for bad arguments or the hipError_t of the launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "amh_device.h"

namespace amh {
namespace probe {

enum F2F {
  kLogf = 0, kExpf, kLog1pf, kLog1pSqf, kLog1pSq3f, kSin, kCos, kRsqrtNr, kErfinvf, kNumF2F
};
enum U2F { kUnif01 = 0, kNormalFromBits, kNormalSplit, kNumU2F };
enum F2I { kPivotOk = 0, kIsFinite, kIsNan, kNumF2I };
enum FF2F { kLogisticTerm = 0, kPoissonTerm, kStudent3Intercept, kStudent3Sigma, kNumFF2F };
enum D2D { kLogD = 0, kExpD, kNumD2D };

// lp_student3's constant in DiamondsM / DiamondsSsM (amh_device.h)
constexpr float kStudent3C = -3.30347394261755545f;

template <int ID>
__device__ __forceinline__ float f2f(float x) {
  if constexpr (ID == kLogf) return amh_logf(x);
  if constexpr (ID == kExpf) return amh_expf(x);
  if constexpr (ID == kLog1pf) return amh_log1pf(x);
  if constexpr (ID == kLog1pSqf) return amh_log1p_sqf(x);
  if constexpr (ID == kLog1pSq3f) return amh_log1p_sq3f(x);
  if constexpr (ID == kSin || ID == kCos) {
    float s, c;
    amh_sincosf(x, &s, &c);
    return ID == kSin ? s : c;
  }
  if constexpr (ID == kRsqrtNr) return amh_rsqrt_nr(x);
  if constexpr (ID == kErfinvf) return amh_erfinvf(x);
}

template <int ID>
__device__ __forceinline__ float u2f(uint32_t b) {
  if constexpr (ID == kUnif01) return amh_unif01_from_bits(b);
  if constexpr (ID == kNormalFromBits) return amh_normal_from_bits(b);
  if constexpr (ID == kNormalSplit) {
    // amh_normal_head + amh_erfinv_tail recombined as draw_noise recombines
    // them (amh_big_pooled.hip:1556-1562), the wave-uniform test included
    float u, w0;
    float xv = amh_normal_head(b, &u, &w0);
    if (__builtin_amdgcn_ballot_w64(!(w0 < 5.0f)) != 0) {
      const float pl = amh_erfinv_tail(w0);
      xv = (w0 < 5.0f) ? xv : pl;
    }
    return 1.41421356f * (xv * u);
  }
}

template <int ID>
__device__ __forceinline__ int32_t f2i(float x) {
  if constexpr (ID == kPivotOk) return amh_pivot_ok(x);
  if constexpr (ID == kIsFinite) return amh_isfinite(x);
  if constexpr (ID == kIsNan) return amh_isnan(x);
}

template <int ID>
__device__ __forceinline__ float ff2f(float a, float b) {
  if constexpr (ID == kLogisticTerm) return logistic_term(a, b);
  if constexpr (ID == kPoissonTerm) return poisson_term(a, b);
  if constexpr (ID == kStudent3Intercept) return lp_student3(a, 8.0f, 10.0f, kStudent3C);
  if constexpr (ID == kStudent3Sigma) return lp_student3(a, 0.0f, 10.0f, kStudent3C);
}

template <int ID>
__device__ __forceinline__ double d2d(double x) {
  if constexpr (ID == kLogD) return amh_log_d(x);
  if constexpr (ID == kExpD) return amh_exp_d(x);
}

template <int ID>
__global__ void f2f_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  y[i] = f2f<ID>(x[i]);
}

template <int ID>
__global__ void u2f_kernel(const uint32_t* __restrict__ b, float* __restrict__ y, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  y[i] = u2f<ID>(b[i]);
}

template <int ID>
__global__ void f2i_kernel(const float* __restrict__ x, int32_t* __restrict__ y, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  y[i] = f2i<ID>(x[i]);
}

// ids that take one argument (the lp_student3 pair) never read b
template <int ID>
__global__ void ff2f_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ y,
                            int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float bi = 0.0f;
  if constexpr (ID == kLogisticTerm || ID == kPoissonTerm) bi = b[i];
  y[i] = ff2f<ID>(a[i], bi);
}

template <int ID>
__global__ void d2d_kernel(const double* __restrict__ x, double* __restrict__ y, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  y[i] = d2d<ID>(x[i]);
}

__global__ void lr_gamma_kernel(const int32_t* __restrict__ nn, float a, float* __restrict__ y, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  y[i] = amh_lr_gamma(nn[i], a);
}

inline dim3 grid_for(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }
// one block index per 256 elements, in an unsigned grid dimension
inline bool count_ok(int64_t n) { return n >= 0 && n <= (int64_t)0x7FFFFFFF * 256; }

template <int ID = 0>
hipError_t launch_f2f(int id, const float* x, float* y, int64_t n, hipStream_t s) {
  if constexpr (ID < kNumF2F) {
    if (id != ID) return launch_f2f<ID + 1>(id, x, y, n, s);
    hipLaunchKernelGGL(f2f_kernel<ID>, grid_for(n), dim3(256), 0, s, x, y, n);
    return hipGetLastError();
  } else {
    return hipErrorInvalidValue;
  }
}

template <int ID = 0>
hipError_t launch_u2f(int id, const uint32_t* b, float* y, int64_t n, hipStream_t s) {
  if constexpr (ID < kNumU2F) {
    if (id != ID) return launch_u2f<ID + 1>(id, b, y, n, s);
    hipLaunchKernelGGL(u2f_kernel<ID>, grid_for(n), dim3(256), 0, s, b, y, n);
    return hipGetLastError();
  } else {
    return hipErrorInvalidValue;
  }
}

template <int ID = 0>
hipError_t launch_f2i(int id, const float* x, int32_t* y, int64_t n, hipStream_t s) {
  if constexpr (ID < kNumF2I) {
    if (id != ID) return launch_f2i<ID + 1>(id, x, y, n, s);
    hipLaunchKernelGGL(f2i_kernel<ID>, grid_for(n), dim3(256), 0, s, x, y, n);
    return hipGetLastError();
  } else {
    return hipErrorInvalidValue;
  }
}

template <int ID = 0>
hipError_t launch_ff2f(int id, const float* a, const float* b, float* y, int64_t n, hipStream_t s) {
  if constexpr (ID < kNumFF2F) {
    if (id != ID) return launch_ff2f<ID + 1>(id, a, b, y, n, s);
    hipLaunchKernelGGL(ff2f_kernel<ID>, grid_for(n), dim3(256), 0, s, a, b, y, n);
    return hipGetLastError();
  } else {
    return hipErrorInvalidValue;
  }
}

template <int ID = 0>
hipError_t launch_d2d(int id, const double* x, double* y, int64_t n, hipStream_t s) {
  if constexpr (ID < kNumD2D) {
    if (id != ID) return launch_d2d<ID + 1>(id, x, y, n, s);
    hipLaunchKernelGGL(d2d_kernel<ID>, grid_for(n), dim3(256), 0, s, x, y, n);
    return hipGetLastError();
  } else {
    return hipErrorInvalidValue;
  }
}

}  // namespace probe
}  // namespace amh

namespace pr = amh::probe;

extern "C" {

// float -> float; id: 0 logf, 1 expf, 2 log1pf, 3 log1p_sqf, 4 log1p_sq3f,
// 5 sin, 6 cos (the two outputs of amh_sincosf), 7 rsqrt_nr, 8 erfinvf
int amh_probe_f2f(int id, const float* x, float* y, int64_t n, void* stream) {
  if (!x || !y || id < 0 || id >= pr::kNumF2F || !pr::count_ok(n)) return -1;
  if (n == 0) return 0;
  return (int)pr::launch_f2f(id, x, y, n, (hipStream_t)stream);
}

// uint32 -> float; id: 0 unif01_from_bits, 1 normal_from_bits, 2 normal_split
int amh_probe_u2f(int id, const uint32_t* b, float* y, int64_t n, void* stream) {
  if (!b || !y || id < 0 || id >= pr::kNumU2F || !pr::count_ok(n)) return -1;
  if (n == 0) return 0;
  return (int)pr::launch_u2f(id, b, y, n, (hipStream_t)stream);
}

// float -> int32; id: 0 pivot_ok, 1 isfinite, 2 isnan
int amh_probe_f2i(int id, const float* x, int32_t* y, int64_t n, void* stream) {
  if (!x || !y || id < 0 || id >= pr::kNumF2I || !pr::count_ok(n)) return -1;
  if (n == 0) return 0;
  return (int)pr::launch_f2i(id, x, y, n, (hipStream_t)stream);
}

// (float, float) -> float; id: 0 logistic_term(a, b), 1 poisson_term(a, b),
// 2 lp_student3(a, 8, 10, c), 3 lp_student3(a, 0, 10, c) (b unused, may be null)
int amh_probe_ff2f(int id, const float* a, const float* b, float* y, int64_t n, void* stream) {
  if (!a || !y || id < 0 || id >= pr::kNumFF2F || !pr::count_ok(n)) return -1;
  if (!b && (id == pr::kLogisticTerm || id == pr::kPoissonTerm)) return -1;
  if (n == 0) return 0;
  return (int)pr::launch_ff2f(id, a, b, y, n, (hipStream_t)stream);
}

// double -> double; id: 0 log_d, 1 exp_d
int amh_probe_d2d(int id, const double* x, double* y, int64_t n, void* stream) {
  if (!x || !y || id < 0 || id >= pr::kNumD2D || !pr::count_ok(n)) return -1;
  if (n == 0) return 0;
  return (int)pr::launch_d2d(id, x, y, n, (hipStream_t)stream);
}

// (int32 n, float a) -> float: amh_lr_gamma
int amh_probe_lr_gamma(const int32_t* nn, float a, float* y, int64_t n, void* stream) {
  if (!nn || !y || !pr::count_ok(n)) return -1;
  if (n == 0) return 0;
  hipLaunchKernelGGL(pr::lr_gamma_kernel, pr::grid_for(n), dim3(256), 0, (hipStream_t)stream, nn, a, y, n);
  return (int)hipGetLastError();
}

// the host (clang) compile of the same header: plain loops over host memory
void amh_probe_host_lr_gamma(const int32_t* nn, float a, float* y, int64_t n) {
  for (int64_t i = 0; i < n; ++i) y[i] = amh_lr_gamma(nn[i], a);
}
void amh_probe_host_log_d(const double* x, double* y, int64_t n) {
  for (int64_t i = 0; i < n; ++i) y[i] = amh_log_d(x[i]);
}
void amh_probe_host_exp_d(const double* x, double* y, int64_t n) {
  for (int64_t i = 0; i < n; ++i) y[i] = amh_exp_d(x[i]);
}
void amh_probe_host_expf(const float* x, float* y, int64_t n) {
  for (int64_t i = 0; i < n; ++i) y[i] = amh_expf(x[i]);
}
void amh_probe_host_logf(const float* x, float* y, int64_t n) {
  for (int64_t i = 0; i < n; ++i) y[i] = amh_logf(x[i]);
}

}  // extern "C"
