// amh_pooled_exact.hip -- the pooled mode's exact sums (include/amh.h "exact
// sums", PooledARWMH(exact_sums=True)): what happens to a rank's chunk partial
// rows once the stats kernels have written them, in place of the double
// reductions (pooled_reduce, launch_reduce_tiles).
//
//   pooled_exact_reduce_kernel   partial rows -> [V][kExactWords] int64: every
//                                partial through exact_add (amh_exact.h), the
//                                words added as integers
//   pooled_exact_convert_kernel  the (all-reduced) words -> the V doubles that
//                                amh_pooled_update_k consumes
//
// Integer addition is associative and commutative, so neither the order in
// which a block's waves take the chunks nor the way the chunks are spread
// over ranks can change a word: no order here is part of a bit spec.
#include "amh_device.h"
#include "amh_exact.h"

namespace amh {

namespace {

constexpr int kExactWaves = 16;    // waves of a reduce block
constexpr int kExactEntries = 16;  // row entries a block owns: a lane is (entry, one of 4 chunk slices)
constexpr int kExactSlices = kExactWaves * (64 / kExactEntries);  // every 64th chunk per lane
constexpr int kExactLoads = 8;     // loads a lane keeps in flight

// Block b owns the 16 row entries u = 16 b + e; lane (e, sub) of wave w adds
// the chunks 4 w + sub, + 64, ... of entry e (a wave's load is four 64-byte
// runs, one per row), the 64 slice totals meet in LDS, and thread (word j,
// entry e) writes word j.  The quantisation is the cost (some 150 integer
// instructions per partial), hence the many narrow blocks: 197 at d = 64.
// T = double: the rows of the lane-per-row stats kernels (float32 values
// stored as double, [S_d | S_dd packed | S_a | N]: u is the component);
// T = float: the tile rows from d = 64 up (tile_d = d, tile_to_packed).
template <typename T>
__global__ __launch_bounds__(64 * kExactWaves) void pooled_exact_reduce_kernel(const T* __restrict__ partials,
                                                                               int64_t n_chunks, int64_t Vrow,
                                                                               int tile_d, int64_t* acc,
                                                                               int accumulate) {
  __shared__ int64_t tot[kExactSlices][kExactWords][kExactEntries];
  const int lane = lane_id();
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64));
  const int e = lane % kExactEntries, slice = w * (64 / kExactEntries) + lane / kExactEntries;
  const int64_t u = (int64_t)blockIdx.x * kExactEntries + e;
  int64_t s[kExactWords];
#pragma unroll
  for (int j = 0; j < kExactWords; ++j) s[j] = 0;
  if (u < Vrow) {  // (entries that belong to no component are skipped at the write below)
    const T* col = partials + u;
    for (int64_t c = slice; c < n_chunks; c += (int64_t)kExactSlices * kExactLoads) {
      float x[kExactLoads];
      static_for<kExactLoads>([&](auto Q) {
        const int64_t cq = c + (int64_t)kExactSlices * Q;
        x[Q] = (cq < n_chunks) ? (float)col[cq * Vrow] : 0.0f;  // (a row entry is a float32 value; +0 adds nothing)
      });
      static_for<kExactLoads>([&](auto Q) { exact_add(s, x[Q]); });
    }
  }
#pragma unroll
  for (int j = 0; j < kExactWords; ++j) tot[slice][j][e] = s[j];
  __syncthreads();
  const int t = (int)threadIdx.x;
  if (t >= kExactWords * kExactEntries) return;
  const int j = t / kExactEntries, eo = t % kExactEntries;
  const int64_t uo = (int64_t)blockIdx.x * kExactEntries + eo;
  // the component this entry belongs to (-1: none -- past the row, the tile
  // layout's padding, or above the diagonal of a diagonal tile)
  const int64_t v = (uo >= Vrow) ? -1 : tile_d ? tile_to_packed(uo, Vrow, tile_d) : uo;
  if (v < 0) return;
  int64_t sum = 0;
#pragma unroll 8
  for (int q = 0; q < kExactSlices; ++q) sum += tot[q][j][eo];
  int64_t* const out = acc + v * kExactWords + j;
  *out = accumulate ? *out + sum : sum;
}

__global__ __launch_bounds__(256) void pooled_exact_convert_kernel(const int64_t* __restrict__ acc, int64_t V,
                                                                   double* __restrict__ sums) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  int64_t w[kExactWords];
#pragma unroll
  for (int j = 0; j < kExactWords; ++j) w[j] = acc[v * kExactWords + j];
  sums[v] = exact_to_double(w);
}

}  // namespace

hipError_t run_pooled_exact_reduce(const void* partials, bool f32_rows, int64_t n_chunks, int64_t Vrow, int tile_d,
                                   int64_t* acc, int accumulate, hipStream_t s) {
  if (n_chunks < 1 || Vrow < 1) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((Vrow + kExactEntries - 1) / kExactEntries)), block(64 * kExactWaves);
  if (f32_rows)
    hipLaunchKernelGGL(pooled_exact_reduce_kernel<float>, grid, block, 0, s, (const float*)partials, n_chunks, Vrow,
                       tile_d, acc, accumulate);
  else
    hipLaunchKernelGGL(pooled_exact_reduce_kernel<double>, grid, block, 0, s, (const double*)partials, n_chunks, Vrow,
                       tile_d, acc, accumulate);
  return hipGetLastError();
}

hipError_t run_pooled_exact_convert(const int64_t* acc, int64_t V, double* sums, hipStream_t s) {
  hipLaunchKernelGGL(pooled_exact_convert_kernel, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, s, acc, V, sums);
  return hipGetLastError();
}

}  // namespace amh
