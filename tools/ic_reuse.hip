// ic_reuse.hip -- does the 256 MiB Infinity Cache serve part of the d = 64 step
// kernel's reads when consecutive launches walk each block's chain range in
// opposite directions?  (tools/ic_reuse; diagnostic, not part of libamh.)
// The data movement of arwmh_step64_kernel alone: an in-place read-modify-write
// sweep of n records of 8,832 B (65,536 records = 579 MB), 256 persistent blocks
// of 16 waves, each block owning a contiguous range of records, one record per
// wave at a time, 16 B per lane, two records in flight per wave.  Launch t walks
// every block's range ascending; in the alternating cases launch t + 1 walks it
// descending, so what t wrote last is what t + 1 reads first.
// Cases: {ascending, alternating} x loads {plain, nt} x stores {plain, nt}, plus
// "sel" (loads nt, stores nt but for the last-visited eighth of each range), at
// 145 / 290 / 579 / 1,158 MB.  One line per case: ms per launch (50 back-to-back
// launches after 30 warm ones, HIP events) and TB/s of read + write traffic.
//   hipcc --offload-arch=gfx950 -O3 -o tools/ic_reuse tools/ic_reuse.hip
#include <hip/hip_runtime.h>

#include <cstdio>

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int kWaves = 16;        // waves per block
constexpr int kRecBytes = 8832;   // one chain's state in one direction, about
constexpr int kRecF4 = kRecBytes / 16;         // 552 f4 = 8 whole 64-lane pieces + 40 lanes
constexpr int kPieces = (kRecF4 + 63) / 64;    // 9
constexpr int kInFlight = 2;      // records loaded per wave before the first is stored

// LD / ST: 0 plain, 1 nt; ST 2: nt except the last-visited eighth of the block's range
template <int LD, int ST>
__global__ __launch_bounds__(kWaves * 64) void sweep_k(f4* __restrict__ buf, long n, int descending) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long lo = n * (long)blockIdx.x / gridDim.x;
  const long hi = n * ((long)blockIdx.x + 1) / gridDim.x;
  const int cnt = (int)(hi - lo);
  for (int v0 = wave; v0 < cnt; v0 += kWaves * kInFlight) {
    f4 r[kInFlight][kPieces];
#pragma unroll
    for (int u = 0; u < kInFlight; ++u) {
      const int v = v0 + u * kWaves;
      if (v < cnt) {
        const f4* rec = buf + (descending ? hi - 1 - v : lo + v) * kRecF4;
#pragma unroll
        for (int q = 0; q < kPieces; ++q) {
          const int o = q * 64 + lane;
          if (o < kRecF4) r[u][q] = LD ? __builtin_nontemporal_load(rec + o) : rec[o];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kInFlight; ++u) {
      const int v = v0 + u * kWaves;
      if (v < cnt) {
        f4* rec = buf + (descending ? hi - 1 - v : lo + v) * kRecF4;
        const bool nt = ST == 1 || (ST == 2 && v < cnt - cnt / 8);
#pragma unroll
        for (int q = 0; q < kPieces; ++q) {
          const int o = q * 64 + lane;
          if (o < kRecF4) {
            const f4 x = r[u][q] * 0.5f + 1.0f;
            if (nt) __builtin_nontemporal_store(x, rec + o);
            else rec[o] = x;
          }
        }
      }
    }
  }
}

template <int LD, int ST>
static void run_case(f4* buf, long n, bool alternate, const char* name) {
  hipEvent_t a, b;
  hipEventCreate(&a);
  hipEventCreate(&b);
  int t = 0;
  auto launch = [&] {
    hipLaunchKernelGGL((sweep_k<LD, ST>), dim3(256), dim3(kWaves * 64), 0, 0, buf, n, alternate ? (t & 1) : 0);
    ++t;
  };
  for (int i = 0; i < 30; ++i) launch();
  hipEventRecord(a);
  for (int i = 0; i < 50; ++i) launch();
  hipEventRecord(b);
  hipEventSynchronize(b);
  float ms = 0;
  hipEventElapsedTime(&ms, a, b);
  ms /= 50;
  const double bytes = (double)n * kRecBytes;
  printf("%7.0f MB  %-11s %-22s %8.4f ms  %6.3f TB/s\n", bytes / 1e6, alternate ? "alternating" : "ascending", name, ms,
         2 * bytes / ms / 1e9);
  hipEventDestroy(a);
  hipEventDestroy(b);
}

int main() {
  const long n_max = 131072;
  f4* buf;
  if (hipMalloc(&buf, (size_t)n_max * kRecBytes) != hipSuccess) {
    printf("hipMalloc failed\n");
    return 1;
  }
  hipMemset(buf, 0, (size_t)n_max * kRecBytes);
  for (long n : {16384L, 32768L, 65536L, 131072L}) {
    for (int alt = 0; alt < 2; ++alt) {
      run_case<0, 0>(buf, n, alt, "ld plain, st plain");
      run_case<0, 1>(buf, n, alt, "ld plain, st nt");
      run_case<1, 0>(buf, n, alt, "ld nt,    st plain");
      run_case<1, 1>(buf, n, alt, "ld nt,    st nt");
      run_case<1, 2>(buf, n, alt, "ld nt,    st sel");
    }
  }
  const hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    printf("error: %s\n", hipGetErrorString(e));
    return 1;
  }
  hipFree(buf);
  return 0;
}
