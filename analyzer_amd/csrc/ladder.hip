// K11 ladder: every player's rank by score on a set of tracks, from the roster alone.
//
//   ladder_keys   one pass over state [P][32] for all requested tracks (a bit mask).  A
//                 workgroup owns a tile of kLadderTile players.  Read side: lane l of a
//                 wave loads granule l & 7 of row l >> 3 as one 16-B load, so a wave
//                 instruction is 8 whole rows = 1 KiB contiguous, and a lane keeps its
//                 track over the whole tile.  The lane turns (mu, sigma) into the sort key
//                 (ladder_core.h) and writes it to an LDS image tile[track][player]; the
//                 track stride of kLadderTile + 4 words puts the 8 tracks x 4 rows of a
//                 half wave on 32 different banks.  Store side: per requested track the
//                 workgroup reads its LDS row 16 B per lane and stores keys[t] and the
//                 identity ids[t] (the sort's values) as 16 B per lane, 1 KiB per wave
//                 instruction: every track's keys leave as whole lines.  The ranked
//                 counts are integer sums (shuffle, LDS, one global atomic per track and
//                 workgroup): exact and the same on every run.
//   sort          launch_radix_sort_pairs (radix_sort.hip), 32 key bits, once per track
//   ladder_ranks  position i of the sorted arrays: rank[ids[i]] = i < R ? i : -1 (every
//                 element is written), and for i < R order[i] = ids[i], score[i] = the
//                 inverse of keys[i]
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "common.h"
#include "kernels.h"
#include "ladder_core.h"

namespace ana {

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef uint32_t v4u __attribute__((ext_vector_type(4)));

constexpr int kLadderThreads = 256;
constexpr int kLadderStride = kLadderTile + 4;                         // LDS words between tracks
constexpr int kLadderRowsPerLoad = kLadderThreads / kGranules;         // 32 rows per workgroup load
constexpr int kLadderLoads = kLadderTile / kLadderRowsPerLoad;         // loads per lane and tile
constexpr int kLadderBatch = 8;                                        // loads in flight per lane
static_assert(kLadderTile == 4 * kLadderThreads, "the store side moves 4 players per lane");
static_assert(kLadderLoads % kLadderBatch == 0, "a tile is a whole number of load batches");
static_assert(kLadderStride % 32 == 4, "bank of tile[g][r] = 4 g + r: a half wave's 8 x 4 writes differ");
static_assert((kLadderStride * 4) % 16 == 0, "16-B LDS reads of a track's row");

__global__ void __launch_bounds__(kLadderThreads) ladder_keys_kernel(const v4f* __restrict__ state, int64_t P,
                                                                    uint32_t mask, int32_t score, float max_sigma,
                                                                    uint32_t* __restrict__ keys,
                                                                    uint32_t* __restrict__ ids, int64_t stride,
                                                                    uint32_t* __restrict__ counts) {
  __shared__ __attribute__((aligned(16))) uint32_t tile[kGranules * kLadderStride];
  __shared__ uint32_t bcnt[kGranules];
  const int t = threadIdx.x;
  const int g = t & (kGranules - 1), r0 = t / kGranules;
  const int64_t base = (int64_t)blockIdx.x * kLadderTile;
  const bool want = ((mask >> g) & 1u) != 0u;
  if (t < kGranules) bcnt[t] = 0u;
  uint32_t n = 0u;
  for (int c = 0; c < kLadderLoads; c += kLadderBatch) {
    v4f v[kLadderBatch];
#pragma unroll
    for (int j = 0; j < kLadderBatch; ++j) {
      const int64_t p = base + (c + j) * kLadderRowsPerLoad + r0;
      v[j] = p < P ? state[p * kGranules + g] : v4f{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int j = 0; j < kLadderBatch; ++j) {
      const int row = (c + j) * kLadderRowsPerLoad + r0;
      const uint32_t key = want && base + row < P ? ladder_key(v[j][0], v[j][2], score, max_sigma) : kLadderUnranked;
      n += key != kLadderUnranked ? 1u : 0u;
      tile[g * kLadderStride + row] = key;
    }
  }
  // lanes l, l ^ 8, l ^ 16, l ^ 32 hold the same track
#pragma unroll
  for (int o = kGranules; o < 64; o <<= 1) n += __shfl_xor(n, o, 64);
  __syncthreads();  // bcnt zeroed, tile written
  if ((t & 63) < kGranules && n) atomicAdd(&bcnt[g], n);
#pragma unroll
  for (int tr = 0; tr < kTracks; ++tr) {
    if (!((mask >> tr) & 1u)) continue;  // uniform over the workgroup
    const int slot = __popc(mask & ((1u << tr) - 1u));
    const int64_t p4 = base + 4 * t;
    if (p4 < P) {  // stride is a multiple of 4 and >= P: the 4 words stay inside the track's row
      const v4u k = *reinterpret_cast<const v4u*>(&tile[tr * kLadderStride + 4 * t]);
      const uint32_t p = (uint32_t)p4;
      *reinterpret_cast<v4u*>(keys + slot * stride + p4) = k;
      *reinterpret_cast<v4u*>(ids + slot * stride + p4) = v4u{p, p + 1u, p + 2u, p + 3u};
    }
  }
  __syncthreads();
  if (t < kTracks && ((mask >> t) & 1u) && bcnt[t]) atomicAdd(&counts[__popc(mask & ((1u << t) - 1u))], bcnt[t]);
}

__global__ void __launch_bounds__(kLadderThreads) ladder_ranks_kernel(const uint32_t* __restrict__ keys,
                                                                     const uint32_t* __restrict__ ids, int64_t P,
                                                                     int64_t R, int32_t* __restrict__ order,
                                                                     float* __restrict__ score,
                                                                     int32_t* __restrict__ rank) {
  const int64_t i = (int64_t)blockIdx.x * kLadderThreads + threadIdx.x;
  if (i >= P) return;
  const uint32_t id = ids[i];
  if ((int64_t)id < P) rank[id] = i < R ? (int32_t)i : -1;  // always: ids is a permutation of [0, P)
  if (i < R) {
    order[i] = (int32_t)id;
    score[i] = ladder_key_score(keys[i]);
  }
}

}  // namespace

int launch_ladder_keys(const float* state, int64_t P, uint32_t mask, int score, float max_sigma, uint32_t* keys,
                       uint32_t* ids, int64_t stride, uint32_t* counts, hipStream_t s) {
  if (P < 0 || P > 0x7fffffffll || mask == 0u || (mask & ~kLadderTrackMask) || stride < P || stride % 4 != 0 ||
      (score != kLadderConservative && score != kLadderMu))
    return (int)hipErrorInvalidValue;
  if (reinterpret_cast<uintptr_t>(state) % 16 != 0 || reinterpret_cast<uintptr_t>(keys) % 16 != 0 ||
      reinterpret_cast<uintptr_t>(ids) % 16 != 0)
    return (int)hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(counts, 0, kTracks * sizeof(uint32_t), s);
  if (e != hipSuccess) return (int)e;
  if (P == 0) return 0;
  const int64_t tiles = (P + kLadderTile - 1) / kLadderTile;
  hipLaunchKernelGGL(ladder_keys_kernel, dim3((unsigned)tiles), dim3(kLadderThreads), 0, s,
                     reinterpret_cast<const v4f*>(state), P, mask, (int32_t)score, max_sigma, keys, ids, stride, counts);
  return (int)hipGetLastError();
}

int launch_ladder_ranks(const uint32_t* keys, const uint32_t* ids, int64_t P, int64_t R, int32_t* order, float* score,
                        int32_t* rank, hipStream_t s) {
  if (P < 0 || P > 0x7fffffffll || R < 0 || R > P) return (int)hipErrorInvalidValue;
  if (P == 0) return 0;
  const int64_t blocks = (P + kLadderThreads - 1) / kLadderThreads;
  hipLaunchKernelGGL(ladder_ranks_kernel, dim3((unsigned)blocks), dim3(kLadderThreads), 0, s, keys, ids, P, R, order,
                     score, rank);
  return (int)hipGetLastError();
}

}  // namespace ana
