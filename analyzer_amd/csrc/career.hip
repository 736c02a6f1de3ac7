// K13 careers: every player's career row (career_core.h) folded from one window of the
// match stream rec [M][2K+2] joined with its packed output rows [M][W].
//
// The table [P][kCareerWords] is updated in place, window by window.  Every field is an
// integer or a copied fp32 bit pattern and both combines are associative, so the result is
// the same bits for any grid, tile size or launch order.  No atomics: a career row has one
// writer per launch.  Four steps on one stream:
//
//   keys    one lane per match (the vector record loads of select.hip): per slot the sort
//           key -- the player id of a game, else P -- the slot index as the value, and the
//           game's 8-B event (score bits; quality term, win bit, status), so the fold gathers
//           8 B per game and never the 128-B row line.  The row is read only when a slot is
//           a candidate: the track's two fields and (quality, status), as 8-B loads.
//   sort    launch_radix_sort_pairs on bit_length(P) bits: stable, so each player's games
//           come out in (match, slot) order, and the slots that are no game sort last.
//   fold    one workgroup per tile of kCareerTile sorted elements, one lane per element per
//           iteration: the lane gathers its event and the segmented inclusive scan of
//           scan_dev.h under career_combine leaves a player's whole run in the lane of its
//           last element.
//           A run strictly inside the tile is folded into its row by that lane.  The runs
//           of the tile's first and last key go to edges[2 * tile + 0 / 1]: they may go on
//           in a neighbour tile.  Cost per element is the same for every key distribution.
//   stitch  one workgroup: the same segmented scan over the 2 * tiles edge runs in tile
//           order; the last edge of each player folds the stitched run into its row.  A
//           player cut by a tile edge is folded here and only here.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "career_core.h"
#include "common.h"
#include "kernels.h"
#include "record_dev.h"
#include "scan_dev.h"

namespace ana {

namespace {

constexpr int kCareerThreads = 256;
constexpr int kCareerIters = kCareerTile / kCareerThreads;
static_assert(kCareerTile % kCareerThreads == 0, "a tile is a whole number of iterations");
// an edge: [key, -, CareerRun]
constexpr int kEdgeWords = 20;
static_assert(sizeof(CareerRun) == 4 * (kEdgeWords - 2), "an edge holds a key and a run");

typedef unsigned int v2u __attribute__((ext_vector_type(2)));

template <int K>
__global__ void __launch_bounds__(kCareerThreads) career_keys_kernel(
    const int32_t* __restrict__ rec, const uint32_t* __restrict__ rows, int64_t W, int64_t M, int64_t P,
    int32_t track, int32_t score, uint32_t modes, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
    v2u* __restrict__ events) {
  constexpr int S = 2 * K;
  const int64_t m = (int64_t)blockIdx.x * kCareerThreads + threadIdx.x;
  if (m >= M) return;
  int32_t r[S + 2];
  load_record<K>(rec, m, r);
  uint32_t mask = career_mask<K>(r, P, modes);
  // of the row: the track's (mu, sigma) fields [2S] and (quality, status), as 8-B loads
  uint32_t ms[2 * S], quality = 0u, st = 0u;
  if (mask) {
    const uint32_t* row = rows + m * W;
    const v2u tail = *reinterpret_cast<const v2u*>(row + 5 * S);
    quality = tail[0];
    st = tail[1] & 0xffu;
    const v2u* src = reinterpret_cast<const v2u*>(row + career_field(track) * S);
#pragma unroll
    for (int c = 0; c < S; ++c) {
      const v2u x = src[c];
      ms[2 * c] = x[0];
      ms[2 * c + 1] = x[1];
    }
    if (!select_status(st)) mask = 0u;
  }
#pragma unroll
  for (int j = 0; j < S; ++j) {
    const int64_t i = m * S + j;
    const bool game = (mask >> j) & 1u;
    keys[i] = game ? (uint32_t)r[j] : (uint32_t)P;
    vals[i] = (uint32_t)i;
    if (game) {
      uint32_t ev[kCareerEventWords];
      career_event<K>(r, j, st, ms[j], ms[S + j], quality, score, ev);
      v2u x;
      x[0] = ev[0];
      x[1] = ev[1];
      events[i] = x;
    }
  }
}

struct CareerOps {
  static __device__ __forceinline__ CareerRun combine(const CareerRun& a, const CareerRun& b) {
    return career_combine(a, b);
  }
  static __device__ __forceinline__ CareerRun identity() { return career_empty(); }
};
// on return from step a lane's run covers its key from the key's first element of this workgroup
typedef SegScan<kCareerThreads, CareerRun, CareerOps> CareerScan;

__device__ __forceinline__ void row_add(int32_t* __restrict__ table, uint32_t p, const CareerRun& run) {
  v4i* q = reinterpret_cast<v4i*>(table + (int64_t)p * kCareerWords);
  int32_t row[kCareerWords];
#pragma unroll
  for (int c = 0; c < kCareerWords / 4; ++c) {
    const v4i x = q[c];
#pragma unroll
    for (int d = 0; d < 4; ++d) row[4 * c + d] = x[d];
  }
  career_row_add(row, run);
#pragma unroll
  for (int c = 0; c < kCareerWords / 4; ++c) {
    v4i x;
#pragma unroll
    for (int d = 0; d < 4; ++d) x[d] = row[4 * c + d];
    q[c] = x;
  }
}

__device__ __forceinline__ void edge_store(int32_t* __restrict__ edges, int64_t e, uint32_t key, const CareerRun& run) {
  int32_t* w = edges + e * kEdgeWords;
  w[0] = (int32_t)key;
  state_store(reinterpret_cast<CareerRun*>(w + 2), run);
}

__global__ void __launch_bounds__(kCareerThreads) career_fold_kernel(
    const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, const v2u* __restrict__ events, int64_t n,
    uint32_t S, int64_t base, uint32_t P, int32_t* __restrict__ table, int32_t* __restrict__ edges) {
  __shared__ CareerScan::Lds lds;
  const int t = threadIdx.x;
  const int64_t lo = (int64_t)blockIdx.x * kCareerTile;
  const int64_t hi = lo + kCareerTile < n ? lo + kCareerTile : n;
  const uint32_t head = keys[lo];
  if (head >= P) {  // sorted: nothing but slots that are no game from here on
    if (t < 2) edges[(2 * (int64_t)blockIdx.x + t) * kEdgeWords] = (int32_t)kNoKey;
    return;
  }
  CareerScan::init(lds);
  for (int it = 0; it < kCareerIters; ++it) {
    const int64_t i = lo + (int64_t)it * kCareerThreads + t;
    if (lo + (int64_t)it * kCareerThreads >= hi) break;  // uniform over the workgroup
    const bool valid = i < hi;
    const uint32_t key = valid ? keys[i] : kNoKey;
    const uint32_t next = valid && i + 1 < n ? keys[i + 1] : kNoKey;
    CareerRun run = career_empty();
    if (valid && key < P) {
      const uint32_t v = vals[i];
      if ((int64_t)v < n) {  // always: the values are a permutation of the slots
        const v2u ev = events[v];
        run = career_game(ev[0], ev[1], base + (int64_t)(v / S));
      }
    }
    CareerScan::step(lds, it, key, run);
    const bool tail = i + 1 == hi;
    if (valid && (tail || next != key)) {  // the last element of its key in this tile
      if (key == head) {
        edge_store(edges, 2 * (int64_t)blockIdx.x, key, run);
        if (tail) edge_store(edges, 2 * (int64_t)blockIdx.x + 1, key, career_empty());
      } else if (tail) {
        edge_store(edges, 2 * (int64_t)blockIdx.x + 1, key, run);
      } else if (key < P) {
        row_add(table, key, run);
      }
    }
  }
}

// one workgroup over the edges [E] in tile order
__global__ void __launch_bounds__(kCareerThreads) career_stitch_kernel(const int32_t* __restrict__ edges, int64_t E,
                                                                       uint32_t P, int32_t* __restrict__ table) {
  __shared__ CareerScan::Lds lds;
  const int t = threadIdx.x;
  CareerScan::init(lds);
  const int iters = (int)((E + kCareerThreads - 1) / kCareerThreads);
  // the edge of the next iteration is loaded ahead of this one's scan: the loop is one
  // workgroup's latency chain
  uint32_t key_n, next_n;
  CareerRun run_n;
  const auto load = [&](int it) {
    const int64_t e = (int64_t)it * kCareerThreads + t;
    key_n = e < E ? (uint32_t)edges[e * kEdgeWords] : kNoKey;
    next_n = e + 1 < E ? (uint32_t)edges[(e + 1) * kEdgeWords] : kNoKey;
    run_n = career_empty();
    if (key_n < P) run_n = state_load(reinterpret_cast<const CareerRun*>(edges + e * kEdgeWords + 2));
  };
  load(0);
  for (int it = 0; it < iters; ++it) {
    const uint32_t key = key_n, next = next_n;
    CareerRun run = run_n;
    if (it + 1 < iters) load(it + 1);
    CareerScan::step(lds, it, key, run);
    if (key < P && next != key) row_add(table, key, run);
  }
}

}  // namespace

static int64_t career_tiles(int64_t n) { return (n + kCareerTile - 1) / kCareerTile; }
size_t career_edge_bytes(int64_t n) { return (size_t)(2 * career_tiles(n) * kEdgeWords) * 4; }

int launch_career_keys(int K, const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t P, int track,
                       int score, uint32_t modes, uint32_t* keys, uint32_t* vals, uint32_t* events, hipStream_t s) {
  if (K < 1 || K > kMaxTeamSize || W < 5 * 2 * K + 2 || M < 0 || P < 0 || P > 0x7fffffffll ||
      M * 2 * K > kMaxSlots || (track != kCareerShared && track != kCareerMode) ||
      (score != kLadderConservative && score != kLadderMu) || (modes & ~kCareerAllModes))
    return (int)hipErrorInvalidValue;
  if (M == 0) return 0;
  const unsigned blocks = (unsigned)((M + kCareerThreads - 1) / kCareerThreads);
  with_team_size(K, [&](auto k) {
    hipLaunchKernelGGL(career_keys_kernel<decltype(k)::value>, dim3(blocks), dim3(kCareerThreads), 0, s, rec,
                       reinterpret_cast<const uint32_t*>(rows), W, M, P, (int32_t)track, (int32_t)score, modes, keys,
                       vals, reinterpret_cast<v2u*>(events));
  });
  return (int)hipGetLastError();
}

int launch_career_fold(const uint32_t* keys, const uint32_t* vals, const uint32_t* events, int64_t n, int K,
                       int64_t base, int64_t P, int32_t* table, void* edges, hipStream_t s) {
  if (K < 1 || K > kMaxTeamSize || n < 0 || n > kMaxSlots || n % (2 * K) || base < 0 || P < 0 || P > 0x7fffffffll)
    return (int)hipErrorInvalidValue;
  if (n == 0 || P == 0) return 0;
  const int64_t tiles = career_tiles(n);
  int32_t* e = static_cast<int32_t*>(edges);
  hipLaunchKernelGGL(career_fold_kernel, dim3((unsigned)tiles), dim3(kCareerThreads), 0, s, keys, vals,
                     reinterpret_cast<const v2u*>(events), n, (uint32_t)(2 * K), base, (uint32_t)P, table, e);
  hipLaunchKernelGGL(career_stitch_kernel, dim3(1), dim3(kCareerThreads), 0, s, e, 2 * tiles, (uint32_t)P, table);
  return (int)hipGetLastError();
}

}  // namespace ana
