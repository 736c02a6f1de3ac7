// K10 records_select: the records of a set of players out of a window of the resident
// record arena (runtime/records.py), in chronological order.
//
// The arena's rows hold no player ids -- those live in the match stream -- so a player's
// history is a join of a window's records rec [M][2K+2] with its output rows [M][W]:
// every occupied slot whose player is in the query bitmap and whose match has records
// (select_core.h) becomes one 48-B hit.  Hits come out in ascending (match, slot) order
// and the same bits on every run: no atomics, no communication between workgroups
// inside a launch.  Three launches:
//
//   count  one workgroup per fixed tile of kSelectTile matches, one lane per match per
//          iteration: the record is loaded with the widest vector loads its size allows
//          (16 / 24 / 32 / 40 / 48 B for K = 1..5: 16-B loads, 8-B loads for K = 2, 4),
//          the per-match hit mask popcounted and summed over the tile -> counts[tile]
//   scan   launch_tile_offsets: exclusive scan of the tile counts -> offsets[tile], the
//          total in offsets[tiles]
//   emit   the same tile walk; a hit's index is offsets[tile] + the hits of the tile's
//          earlier iterations + the waves before this one (LDS) + a shuffle scan over
//          the lanes' counts; each hit is three 16-B stores.  A tile without hits ends
//          at once, so a sparse query streams only rec (a quarter of the bytes of the
//          rows): a row is read only after one of its match's ids hit the bitmap.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "common.h"
#include "kernels.h"
#include "record_dev.h"
#include "scan_dev.h"
#include "select_core.h"

namespace ana {

namespace {

constexpr int kSelectThreads = 256;
constexpr int kSelectIters = kSelectTile / kSelectThreads;
static_assert(kSelectTile % kSelectThreads == 0, "a tile is a whole number of iterations");

// the hit mask of match m (0 past the window's end) and its status byte; the row is
// only touched when the mask is not empty
template <int K>
__device__ __forceinline__ uint32_t match_mask(const int32_t* __restrict__ rec, const uint32_t* __restrict__ rows,
                                               int64_t W, int64_t M, int64_t m, int64_t P,
                                               const uint32_t* __restrict__ bitmap, int32_t* r, uint32_t& st) {
  st = 0u;
  if (m >= M) return 0u;
  load_record<K>(rec, m, r);
  uint32_t mask = select_mask<K>(r, P, bitmap);
  if (mask) {
    st = select_row_status<K>(rows + m * W);
    if (!select_status(st)) mask = 0u;
  }
  return mask;
}

template <int K>
__global__ void __launch_bounds__(kSelectThreads) select_count_kernel(const int32_t* __restrict__ rec,
                                                                      const uint32_t* __restrict__ rows, int64_t W,
                                                                      int64_t M, int64_t P,
                                                                      const uint32_t* __restrict__ bitmap,
                                                                      uint32_t* __restrict__ counts) {
  const int t = threadIdx.x;
  const int64_t m0 = (int64_t)blockIdx.x * kSelectTile + t;
  uint32_t n = 0u;
#pragma unroll
  for (int i = 0; i < kSelectIters; ++i) {
    int32_t r[2 * K + 2];
    uint32_t st;
    n += (uint32_t)__popc(match_mask<K>(rec, rows, W, M, m0 + (int64_t)i * kSelectThreads, P, bitmap, r, st));
  }
  block_sum_store<kSelectThreads>(n, counts + blockIdx.x);
}

template <int K>
__global__ void __launch_bounds__(kSelectThreads) select_emit_kernel(const int32_t* __restrict__ rec,
                                                                     const uint32_t* __restrict__ rows, int64_t W,
                                                                     int64_t M, int64_t base, int64_t P,
                                                                     const uint32_t* __restrict__ bitmap,
                                                                     const int64_t* __restrict__ offsets,
                                                                     int32_t* __restrict__ hits, int64_t nhits) {
  constexpr int S = 2 * K;
  const int t = threadIdx.x, lane = t & 63;
  int64_t run = offsets[blockIdx.x];
  if (offsets[blockIdx.x + 1] == run) return;  // no hit in this tile (uniform over the workgroup)
  const int64_t m0 = (int64_t)blockIdx.x * kSelectTile + t;
  for (int i = 0; i < kSelectIters; ++i) {
    const int64_t m = m0 + (int64_t)i * kSelectThreads;
    int32_t r[S + 2];
    uint32_t st;
    const uint32_t mask = match_mask<K>(rec, rows, W, M, m, P, bitmap, r, st);
    const int own = __popc(mask);
    int incl = own;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o, 64);
      if (lane >= o) incl += v;
    }
    int total;
    const int before = block_offset<kSelectThreads>(i, incl, total);
    int64_t idx = run + before + incl - own;
    run += total;
    if (mask) {
      const uint32_t* row = rows + m * W;
#pragma unroll
      for (int j = 0; j < S; ++j) {
        if (!((mask >> j) & 1u)) continue;
        if (idx < nhits) {  // always, for unchanged inputs: the counts come from the same walk
          int32_t h[kHitWords];
          select_hit<K>(r, row, base + m, j, st, h);
          v4i* dst = reinterpret_cast<v4i*>(hits + idx * kHitWords);
#pragma unroll
          for (int q = 0; q < kHitWords / 4; ++q) {
            v4i x;
#pragma unroll
            for (int c = 0; c < 4; ++c) x[c] = h[4 * q + c];
            dst[q] = x;
          }
        }
        ++idx;
      }
    }
  }
}

}  // namespace

int64_t records_select_tiles(int64_t M) { return (M + kSelectTile - 1) / kSelectTile; }

int launch_records_select_count(int K, const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t P,
                                const uint32_t* bitmap, uint32_t* counts, int64_t* offsets, hipStream_t s) {
  const int64_t tiles = records_select_tiles(M);
  if (K < 1 || K > kMaxTeamSize || W < 5 * 2 * K + 2 || M < 0 || P < 0 || tiles > 0x7fffffffll) return (int)hipErrorInvalidValue;
  const uint32_t* rw = reinterpret_cast<const uint32_t*>(rows);
  if (tiles > 0) {
    with_team_size(K, [&](auto k) {
      hipLaunchKernelGGL(select_count_kernel<decltype(k)::value>, dim3((unsigned)tiles), dim3(kSelectThreads), 0, s,
                         rec, rw, W, M, P, bitmap, counts);
    });
  }
  return launch_tile_offsets(counts, tiles, offsets, s);
}

int launch_records_select_emit(int K, const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t base,
                               int64_t P, const uint32_t* bitmap, const int64_t* offsets, int32_t* hits,
                               int64_t nhits, hipStream_t s) {
  const int64_t tiles = records_select_tiles(M);
  if (K < 1 || K > kMaxTeamSize || W < 5 * 2 * K + 2 || M < 0 || P < 0 || tiles > 0x7fffffffll) return (int)hipErrorInvalidValue;
  if (tiles == 0 || nhits == 0) return 0;
  const uint32_t* rw = reinterpret_cast<const uint32_t*>(rows);
  with_team_size(K, [&](auto k) {
    hipLaunchKernelGGL(select_emit_kernel<decltype(k)::value>, dim3((unsigned)tiles), dim3(kSelectThreads), 0, s, rec,
                       rw, W, M, base, P, bitmap, offsets, hits, nhits);
  });
  return (int)hipGetLastError();
}

}  // namespace ana
