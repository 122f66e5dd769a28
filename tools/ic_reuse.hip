// ic_reuse.hip -- how much of the d = 64 step kernel's traffic can the 256 MiB
// Infinity Cache serve when consecutive launches walk each block's chain range
// in opposite directions, and which cache policy and visiting order make the
// most of it?  (tools/ic_reuse; diagnostic, not part of libamh.)
//
// The data movement of arwmh_step64_kernel alone: an in-place read-modify-write
// sweep of n records of 8,832 B (65,536 records = 579 MB), 256 persistent blocks
// of 16 waves, each block owning a contiguous range of records, one record per
// wave at a time, 16 B per lane as raw buffer instructions, two records in
// flight per wave.  Launch t walks every block's range ascending; in the
// alternating cases launch t + 1 walks it descending, so what t wrote last is
// what t + 1 reads first.
//
// Per position.  With h = floor(f * cnt) of a block's cnt records, a launch's
// first h visiting positions are *hot* (the previous launch wrote them last),
// its last h are the *tail* (the next launch reads them first), the rest is
// *mid*.  Loads take one policy for hot and one for the rest; stores one each
// for hot, mid and tail.  A policy string is five letters p(lain) / n(t):
// ld hot, ld cold, st hot, st mid, st tail (the step kernel ships "nnnpp" at
// f = 3/8; "nnppp" was its policy before the split by position).
// Order.  "hotfirst" visits the positions 0, 1, 2, ...; "interleaved" draws from
// the hot end and from the rest alternately at ratio f : (1 - f) through the
// whole launch (hot draws spread evenly, the first draw hot).
// Compute padding.  `pad` dependent v_fma per record between its load and its
// store (about the step kernel's issue slots per chain when pad ~ 1,000: four
// waves per SIMD share them), so that the phase that hits in the cache is bound
// by issue slots as it is in the kernel.  The padded cases use the largest pad
// of the ladder whose ascending nt / nt time stays at or below the kernel's
// ascending time (argv[1], ms; default 0.2233) or within 1 % of the unpadded
// time, whichever is larger; 250 when none does.
//
// One line per case: ms per launch (40 back-to-back launches after 20 warm
// ones, HIP events) and TB/s of read + write traffic.
//   hipcc --offload-arch=gfx950 -O3 -o tools/ic_reuse tools/ic_reuse.hip
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int kWaves = 16;        // waves per block
constexpr int kRecBytes = 8832;   // one chain's state in one direction, about
constexpr int kRecF4 = kRecBytes / 16;         // 552 f4 = 8 whole 64-lane pieces + 40 lanes
constexpr int kPieces = (kRecF4 + 63) / 64;    // 9
constexpr int kInFlight = 2;      // records loaded per wave before the first is stored

struct Sched {
  int descending;   // this launch walks the ranges from the top
  int f8;           // hot fraction in eighths (0: no hot part, no tail)
  int interleaved;  // 0 hot-first, 1 hot and cold draws alternating at f : 1 - f
  int pad;          // dependent VALU operations per record
  int ld_hot, ld_cold, st_hot, st_mid, st_tail;  // 0 plain, 1 nt
};

typedef unsigned int u4 __attribute__((ext_vector_type(4)));

// One record as a raw buffer (wave-uniform base in SGPRs), moved as the step
// kernel moves a factor: buffer instructions whose cache policy is the aux
// immediate (0 plain, 2 nt).  Two builtins with different immediates cannot be
// merged by the compiler, as a plain and a nontemporal access of the same
// address in the two arms of a branch are (the merge drops the hint).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rec_rsrc(const f4* rec) {
  const unsigned long long a = (unsigned long long)rec;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
  return __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long long)hi << 32) | lo), (short)0, kRecBytes,
                                           0x00020000);
}
template <int AUX>
__device__ __forceinline__ void load_rec(f4 (&r)[kPieces], const f4* rec, int lane) {
  const __amdgpu_buffer_rsrc_t rs = rec_rsrc(rec);
#pragma unroll
  for (int q = 0; q < kPieces; ++q) {
    const int o = q * 64 + lane;
    if (o < kRecF4) r[q] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rs, o * 16, 0, AUX));
  }
}
template <int AUX>
__device__ __forceinline__ void store_rec(const f4 (&r)[kPieces], f4* rec, int lane) {
  const __amdgpu_buffer_rsrc_t rs = rec_rsrc(rec);
#pragma unroll
  for (int q = 0; q < kPieces; ++q) {
    const int o = q * 64 + lane;
    if (o < kRecF4)
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, r[q] * 0.5f + 1.0f), rs, o * 16, 0, AUX);
  }
}

// visiting position -> place in the hot-first order (place < h: hot, place >= cnt - h: tail)
__device__ __forceinline__ int place_of(int pos, int cnt, int h, int interleaved) {
  if (!interleaved || h == 0) return pos;
  const int before = (pos * h + cnt - 1) / cnt;          // hot draws before this one
  const int after = ((pos + 1) * h + cnt - 1) / cnt;     // ... and including it
  return after > before ? before : h + (pos - before);
}

struct Block {
  f4* buf;
  long lo, hi;
  int cnt, h, lane;
  Sched s;
  __device__ __forceinline__ f4* rec(int place) const {
    return buf + (s.descending ? hi - 1 - place : lo + place) * kRecF4;
  }
  // the record at visiting position v: issue its loads
  __device__ __forceinline__ void load(f4 (&r)[kPieces], int v) const {
    const int place = place_of(v, cnt, h, s.interleaved);
    if (place < h ? s.ld_hot : s.ld_cold) load_rec<2>(r, rec(place), lane);
    else load_rec<0>(r, rec(place), lane);
  }
  // ... the padding on what was loaded, then its stores
  __device__ __forceinline__ void finish(f4 (&r)[kPieces], int v) const {
    const int place = place_of(v, cnt, h, s.interleaved);
    float x = r[0].x;
    for (int i = 0; i < s.pad; ++i) x = __builtin_fmaf(x, 0.999f, 0.001f);
    r[0].x = x;
    const int st = place < h ? s.st_hot : place >= cnt - h ? s.st_tail : s.st_mid;
    if (st) store_rec<2>(r, rec(place), lane);
    else store_rec<0>(r, rec(place), lane);
  }
};

// Each wave takes the visiting positions wave, wave + 16, ...  As in the step
// kernel the next record's loads are issued before the current one is padded
// and stored, so the padding overlaps the loads in flight.
__global__ __launch_bounds__(kWaves * 64) void sweep_k(f4* __restrict__ buf, long n, Sched s) {
  Block b;
  b.buf = buf;
  b.lane = threadIdx.x & 63;
  b.lo = n * (long)blockIdx.x / gridDim.x;
  b.hi = n * ((long)blockIdx.x + 1) / gridDim.x;
  b.cnt = (int)(b.hi - b.lo);
  b.h = b.cnt * s.f8 / 8;
  b.s = s;
  const int wave = threadIdx.x >> 6;
  f4 r0[kPieces], r1[kPieces];
  if (wave < b.cnt) b.load(r0, wave);
  for (int v = wave; v < b.cnt; v += kInFlight * kWaves) {
    const int v1 = v + kWaves, v2 = v1 + kWaves;
    if (v1 < b.cnt) b.load(r1, v1);
    b.finish(r0, v);
    if (v2 < b.cnt) b.load(r0, v2);
    if (v1 < b.cnt) b.finish(r1, v1);
  }
}

static float time_case(f4* buf, long n, bool alternate, Sched s) {
  hipEvent_t a, b;
  hipEventCreate(&a);
  hipEventCreate(&b);
  int t = 0;
  auto launch = [&] {
    s.descending = alternate ? (t & 1) : 0;
    hipLaunchKernelGGL(sweep_k, dim3(256), dim3(kWaves * 64), 0, 0, buf, n, s);
    ++t;
  };
  for (int i = 0; i < 20; ++i) launch();
  hipEventRecord(a);
  for (int i = 0; i < 40; ++i) launch();
  hipEventRecord(b);
  hipEventSynchronize(b);
  float ms = 0;
  hipEventElapsedTime(&ms, a, b);
  hipEventDestroy(a);
  hipEventDestroy(b);
  return ms / 40;
}

static Sched policy(const char* p, int f8, int interleaved, int pad) {
  Sched s{};
  s.f8 = f8;
  s.interleaved = interleaved;
  s.pad = pad;
  s.ld_hot = p[0] == 'n';
  s.ld_cold = p[1] == 'n';
  s.st_hot = p[2] == 'n';
  s.st_mid = p[3] == 'n';
  s.st_tail = p[4] == 'n';
  return s;
}

static void run_case(f4* buf, long n, bool alternate, const char* p, int f8, int interleaved, int pad) {
  const float ms = time_case(buf, n, alternate, policy(p, f8, interleaved, pad));
  const double bytes = (double)n * kRecBytes;
  printf("%5.0f MB  %-11s f=%d/8 %-11s pad %4d  %s  %8.4f ms  %6.3f TB/s\n", bytes / 1e6,
         alternate ? "alternating" : "ascending", f8, interleaved ? "interleaved" : "hotfirst", pad, p, ms,
         2 * bytes / ms / 1e9);
  fflush(stdout);
}

int main(int argc, char** argv) {
  const float target = argc > 1 ? (float)atof(argv[1]) : 0.2233f;
  const long n_max = 131072;
  f4* buf;
  if (hipMalloc(&buf, (size_t)n_max * kRecBytes) != hipSuccess) {
    printf("hipMalloc failed\n");
    return 1;
  }
  hipMemset(buf, 0, (size_t)n_max * kRecBytes);

  // the compute padding: ascending nt / nt at 579 MB over a ladder of pads
  int pad = 0;
  {
    float t0 = 0;
    for (int pd : {0, 125, 250, 375, 500, 625, 750, 875, 1000, 1250, 1500}) {
      const float ms = time_case(buf, 65536, false, policy("nnnnn", 0, 0, pd));
      if (pd == 0) t0 = ms;
      const float bar = target > 1.01f * t0 ? target : 1.01f * t0;
      if (ms <= bar) pad = pd;
      printf("# pad ladder: pad %4d  ascending nnnnn  %8.4f ms (bar %.4f)\n", pd, ms, bar);
    }
    if (pad == 0) {
      // no pad of the ladder stays under the bar: the sweep is bound by the
      // latency of its two records in flight, not by bandwidth, so padding
      // adds to its time.  The padded rows then use 250 and are read against
      // their own ascending rows.
      pad = 250;
      printf("# no pad of the ladder stays under the bar; ");
    }
    printf("# padded cases use pad %d\n", pad);
  }

  // every policy: ld hot, ld cold, st hot, st mid, st tail
  char pol[32][6];
  for (int m = 0; m < 32; ++m) {
    for (int b = 0; b < 5; ++b) pol[m][b] = (m >> (4 - b)) & 1 ? 'n' : 'p';
    pol[m][5] = 0;
  }
  const char* uniform[4] = {"ppppp", "ppnnn", "nnppp", "nnnnn"};

  for (int pd : {0, pad}) {
    // controls: the sizes where everything fits and where little does
    for (long n : {32768L, 131072L}) {
      for (const char* p : uniform) run_case(buf, n, false, p, 0, 0, pd);
      for (const char* p : uniform) run_case(buf, n, true, p, 2, 0, pd);
      for (const char* p : {"npnnp", "ppnnp", "nnnnp", "nnnpp"}) {
        run_case(buf, n, true, p, 2, 0, pd);
        run_case(buf, n, true, p, 2, 1, pd);
      }
    }
    // 579 MB: ascending at the four uniform policies, then the whole sweep
    for (const char* p : uniform) run_case(buf, 65536, false, p, 0, 0, pd);
    for (int f8 = 1; f8 <= 4; ++f8)
      for (int il = 0; il < 2; ++il)
        for (int m = 0; m < 32; ++m) run_case(buf, 65536, true, pol[m], f8, il, pd);
  }
  const hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    printf("error: %s\n", hipGetErrorString(e));
    return 1;
  }
  hipFree(buf);
  return 0;
}
