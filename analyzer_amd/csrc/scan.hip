// Tile offsets: the one-workgroup exclusive scan between the count and the emit launch of
// K10 select and K15 pairs (kernels.h launch_tile_offsets).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "kernels.h"

namespace ana {

namespace {

constexpr int kOffsetThreads = 256;
constexpr int kOffsetWaves = kOffsetThreads / 64;

// lane l owns the tiles [l * per, (l + 1) * per); with fewer tiles than lanes the trailing
// lanes own none
__global__ void __launch_bounds__(kOffsetThreads) tile_offsets_kernel(const uint32_t* __restrict__ counts,
                                                                      int64_t tiles, int64_t* __restrict__ offsets) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t per = (tiles + kOffsetThreads - 1) / kOffsetThreads;
  const int64_t lo = (int64_t)t * per < tiles ? (int64_t)t * per : tiles;
  const int64_t hi = lo + per < tiles ? lo + per : tiles;
  int64_t own = 0;
  for (int64_t i = lo; i < hi; ++i) own += counts[i];
  int64_t incl = own;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int64_t v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  __shared__ int64_t wsum[kOffsetWaves];
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int64_t before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kOffsetWaves; ++w) {
    before += w < wave ? wsum[w] : 0;
    total += wsum[w];
  }
  int64_t run = before + incl - own;
  for (int64_t i = lo; i < hi; ++i) {
    offsets[i] = run;
    run += counts[i];
  }
  if (t == 0) offsets[tiles] = total;
}

}  // namespace

int launch_tile_offsets(const uint32_t* counts, int64_t tiles, int64_t* offsets, hipStream_t s) {
  if (tiles < 0 || offsets == nullptr || reinterpret_cast<uintptr_t>(offsets) % 8 != 0 ||
      (tiles > 0 && counts == nullptr))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(tile_offsets_kernel, dim3(1), dim3(kOffsetThreads), 0, s, counts, tiles, offsets);
  return (int)hipGetLastError();
}

}  // namespace ana
