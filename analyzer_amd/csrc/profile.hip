// K17 profiles: every player's stat totals and the baselines per (mode, skill bracket, result)
// (profile_core.h), folded from one window of the match stream rec [M][2K+2] joined with its
// packed output rows [M][W] and its telemetry stat vectors stats [M][2K][8].
//
// The player table [P][kProfileWords] and the baseline table are updated in place, window by
// window.  Every sum is an integer, so both are the same bits for any grid, tile size or
// launch order.  A player row has one writer per launch; the baseline table is integer
// atomics.  Four steps on one stream, ordered by the stream alone:
//
//   keys    one lane per match (the vector record loads of select.hip): per slot the sort key
//           -- the player id of a game, else P -- and the value slot | won << 31.  For each
//           game the lane reads the slot's 32 B of stats as two 16-B loads and adds
//           (1, terms[8]) to the game's cell of a copy of the baseline table in LDS; after a
//           barrier the workgroup adds its non-zero words to the global table, once per word.
//           The two counters travel the same way.  The row words and the stats of a match's
//           candidate slots (career_mask) are asked for together, ahead of the status: one
//           wait per match instead of three (1.74 -> 1.08 ms per 10M 3v3 matches), and what
//           a match that turns out not rated brought in is dropped.  Stats of a slot that is
//           no candidate are never loaded, and only a game's stats reach a sum.
//   sort    launch_radix_sort_pairs on bit_length(P) bits; the slots that are no game sort last.
//   fold    one workgroup per tile of kProfileTile sorted elements, one lane per element per
//           iteration: the lane gathers its slot's stats, forms the terms, and the segmented
//           inclusive scan of scan_dev.h under profile_combine leaves a player's whole run in
//           the lane of its last element.  A run strictly inside the tile is added to its row
//           by that lane.  The runs of the tile's first and last key go to
//           edges[2 * tile + 0 / 1]: they may go on in a neighbour tile.
//   stitch  one workgroup: the same scan over the 2 * tiles edge runs in tile order; the last
//           edge of each player adds the stitched run to its row.
//
// Built with -ffp-contract=off: the score is the one IEEE subtraction the host mirror does.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "common.h"
#include "kernels.h"
#include "profile_core.h"
#include "record_dev.h"
#include "scan_dev.h"

namespace ana {

namespace {

constexpr int kProfileThreads = 256;
constexpr int kProfileIters = kProfileTile / kProfileThreads;
static_assert(kProfileTile % kProfileThreads == 0, "a tile is a whole number of iterations");
// an edge: [key, -, ProfileRun]
constexpr int kEdgeWords = 20;
static_assert(sizeof(ProfileRun) == 4 * (kEdgeWords - 2), "an edge holds a key and a run");
static_assert(kProfileWords % 4 == 0, "a row is whole 16-B pieces");

typedef unsigned int v2u __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));

// the 8 stat values of one slot, two 16-B loads
__device__ __forceinline__ void load_stats(const v4f* __restrict__ stats, int64_t slot, float* x) {
  const v4f a = stats[2 * slot], b = stats[2 * slot + 1];
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    x[d] = a[d];
    x[4 + d] = b[d];
  }
}

template <int K>
__global__ void __launch_bounds__(kProfileThreads) profile_keys_kernel(
    const int32_t* __restrict__ rec, const uint32_t* __restrict__ rows, int64_t W, const v4f* __restrict__ stats,
    int64_t M, int64_t P, int32_t track, int32_t score, uint32_t modes, ProfileEdges edges,
    uint32_t* __restrict__ keys, uint32_t* __restrict__ vals, unsigned long long* __restrict__ cells) {
  constexpr int S = 2 * K;
  __shared__ unsigned long long part[kProfileMaxTableWords];
  const int words = profile_table_words(edges.n + 1);
  for (int c = threadIdx.x; c < words; c += kProfileThreads) part[c] = 0ull;
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * kProfileThreads;
  for (int64_t m = (int64_t)blockIdx.x * kProfileThreads + threadIdx.x; m < M; m += stride) {
    int32_t r[S + 2];
    load_record<K>(rec, m, r);
    uint32_t mask = career_mask<K>(r, P, modes);
    // Behind a candidate slot everything the lane needs is asked for at once, so one wait
    // covers it: of the row the status and the track's (mu, sigma) fields [2S], and the 32 B of
    // stats of every candidate slot.  What a match that is not rated brought in is dropped.
    uint32_t ms[2 * S];
    float x[S][kProfileStats];
    if (mask) {
      const uint32_t* row = rows + m * W;
      const v2u tail = *reinterpret_cast<const v2u*>(row + 5 * S);
      const v2u* src = reinterpret_cast<const v2u*>(row + career_field(track) * S);
#pragma unroll
      for (int c = 0; c < S; ++c) {
        const v2u f = src[c];
        ms[2 * c] = f[0];
        ms[2 * c + 1] = f[1];
      }
#pragma unroll
      for (int j = 0; j < S; ++j)
        if ((mask >> j) & 1u) load_stats(stats, m * S + j, x[j]);
      if ((tail[1] & 0xffu) != kRated) mask = 0u;
    }
    const int mode = meta_mode((uint32_t)r[S]);
#pragma unroll
    for (int j = 0; j < S; ++j) {
      const int64_t i = m * S + j;
      const bool game = (mask >> j) & 1u;
      const bool won = game && profile_won<K>(r, j);
      keys[i] = game ? (uint32_t)r[j] : (uint32_t)P;
      vals[i] = (uint32_t)i | (won ? kProfileWonBit : 0u);
      if (game) {
        int32_t bad = 0;
        const ProfileRun g = profile_game(x[j], won, bad);
        const float s = ladder_score(ladder_float(ms[j]), ladder_float(ms[S + j]), score);
        profile_cell_add(edges, mode, s, g, bad,
                         [&](int c, int64_t v) { atomicAdd(&part[c], (unsigned long long)v); });
      }
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < words; c += kProfileThreads)
    if (part[c] != 0ull) atomicAdd(&cells[c], part[c]);
}

struct ProfileOps {
  static __device__ __forceinline__ ProfileRun combine(const ProfileRun& a, const ProfileRun& b) {
    return profile_combine(a, b);
  }
  static __device__ __forceinline__ ProfileRun identity() { return profile_empty(); }
};
// on return from step a lane's run covers its key from the key's first element of this workgroup
typedef SegScan<kProfileThreads, ProfileRun, ProfileOps> ProfileScan;

__device__ __forceinline__ void row_add(int32_t* __restrict__ table, uint32_t p, const ProfileRun& run) {
  v4i* q = reinterpret_cast<v4i*>(table + (int64_t)p * kProfileWords);
  int32_t row[kProfileWords];
#pragma unroll
  for (int c = 0; c < kProfileWords / 4; ++c) {
    const v4i x = q[c];
#pragma unroll
    for (int d = 0; d < 4; ++d) row[4 * c + d] = x[d];
  }
  profile_row_add(row, run);
#pragma unroll
  for (int c = 0; c < kProfileWords / 4; ++c) {
    v4i x;
#pragma unroll
    for (int d = 0; d < 4; ++d) x[d] = row[4 * c + d];
    q[c] = x;
  }
}

__device__ __forceinline__ void edge_store(int32_t* __restrict__ edges, int64_t e, uint32_t key,
                                           const ProfileRun& run) {
  int32_t* w = edges + e * kEdgeWords;
  w[0] = (int32_t)key;
  state_store(reinterpret_cast<ProfileRun*>(w + 2), run);
}

__global__ void __launch_bounds__(kProfileThreads) profile_fold_kernel(
    const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, const v4f* __restrict__ stats, int64_t n,
    uint32_t P, int32_t* __restrict__ table, int32_t* __restrict__ edges) {
  __shared__ ProfileScan::Lds lds;
  const int t = threadIdx.x;
  const int64_t lo = (int64_t)blockIdx.x * kProfileTile;
  const int64_t hi = lo + kProfileTile < n ? lo + kProfileTile : n;
  const uint32_t head = keys[lo];
  if (head >= P) {  // sorted: nothing but slots that are no game from here on
    if (t < 2) edges[(2 * (int64_t)blockIdx.x + t) * kEdgeWords] = (int32_t)kNoKey;
    return;
  }
  ProfileScan::init(lds);
  for (int it = 0; it < kProfileIters; ++it) {
    const int64_t i = lo + (int64_t)it * kProfileThreads + t;
    if (lo + (int64_t)it * kProfileThreads >= hi) break;  // uniform over the workgroup
    const bool valid = i < hi;
    const uint32_t key = valid ? keys[i] : kNoKey;
    const uint32_t next = valid && i + 1 < n ? keys[i + 1] : kNoKey;
    ProfileRun run = profile_empty();
    if (valid && key < P) {
      const uint32_t v = vals[i];
      const int64_t slot = (int64_t)(v & kProfileSlotMask);
      if (slot < n) {  // always: the slot indices are a permutation of the slots
        float x[kProfileStats];
        load_stats(stats, slot, x);
        int32_t bad = 0;  // counted by the keys kernel
        run = profile_game(x, (v & kProfileWonBit) != 0u, bad);
      }
    }
    ProfileScan::step(lds, it, key, run);
    const bool tail = i + 1 == hi;
    if (valid && (tail || next != key)) {  // the last element of its key in this tile
      if (key == head) {
        edge_store(edges, 2 * (int64_t)blockIdx.x, key, run);
        if (tail) edge_store(edges, 2 * (int64_t)blockIdx.x + 1, key, profile_empty());
      } else if (tail) {
        edge_store(edges, 2 * (int64_t)blockIdx.x + 1, key, run);
      } else if (key < P) {
        row_add(table, key, run);
      }
    }
  }
}

// one workgroup over the edges [E] in tile order
__global__ void __launch_bounds__(kProfileThreads) profile_stitch_kernel(const int32_t* __restrict__ edges, int64_t E,
                                                                         uint32_t P, int32_t* __restrict__ table) {
  __shared__ ProfileScan::Lds lds;
  const int t = threadIdx.x;
  ProfileScan::init(lds);
  const int iters = (int)((E + kProfileThreads - 1) / kProfileThreads);
  // the edge of the next iteration is loaded ahead of this one's scan: the loop is one
  // workgroup's latency chain
  uint32_t key_n, next_n;
  ProfileRun run_n;
  const auto load = [&](int it) {
    const int64_t e = (int64_t)it * kProfileThreads + t;
    key_n = e < E ? (uint32_t)edges[e * kEdgeWords] : kNoKey;
    next_n = e + 1 < E ? (uint32_t)edges[(e + 1) * kEdgeWords] : kNoKey;
    run_n = profile_empty();
    if (key_n < P) run_n = state_load(reinterpret_cast<const ProfileRun*>(edges + e * kEdgeWords + 2));
  };
  load(0);
  for (int it = 0; it < iters; ++it) {
    const uint32_t key = key_n, next = next_n;
    ProfileRun run = run_n;
    if (it + 1 < iters) load(it + 1);
    ProfileScan::step(lds, it, key, run);
    if (key < P && next != key) row_add(table, key, run);
  }
}

}  // namespace

static int64_t profile_tiles(int64_t n) { return (n + kProfileTile - 1) / kProfileTile; }
size_t profile_edge_bytes(int64_t n) { return (size_t)(2 * profile_tiles(n) * kEdgeWords) * 4; }

static bool profile_edges_ok(const float* edges, int n_edges) {
  if (n_edges < 0 || n_edges > kProfileMaxEdges || (n_edges > 0 && edges == nullptr)) return false;
  for (int i = 0; i < n_edges; ++i)
    if (!(edges[i] - edges[i] == 0.0f) || (i > 0 && !(edges[i - 1] < edges[i]))) return false;
  return true;
}

int launch_profile_keys(int K, const int32_t* rec, const float* rows, int64_t W, const float* stats, int64_t M,
                        int64_t P, int track, int score, uint32_t modes, const float* edges, int n_edges,
                        uint32_t* keys, uint32_t* vals, int64_t* cells, hipStream_t s) {
  if (K < 1 || K > kMaxTeamSize || W < 5 * 2 * K + 2 || M < 0 || P < 0 || P > 0x7fffffffll ||
      M * 2 * K > kMaxSlots || (track != kCareerShared && track != kCareerMode) ||
      (score != kLadderConservative && score != kLadderMu) || (modes & ~kCareerAllModes) ||
      !profile_edges_ok(edges, n_edges) || cells == nullptr || reinterpret_cast<uintptr_t>(stats) % 16 != 0)
    return (int)hipErrorInvalidValue;
  if (M == 0) return 0;
  ProfileEdges pe;
  pe.n = n_edges;
  for (int i = 0; i < kProfileMaxEdges; ++i) pe.e[i] = i < n_edges ? edges[i] : 0.0f;
  const int64_t want = (M + kProfileThreads - 1) / kProfileThreads;
  // the LDS table lets 5 workgroups share a CU: one wave of them over the chip, then a grid stride
  const unsigned blocks = (unsigned)(want < 1280 ? want : 1280);
  with_team_size(K, [&](auto k) {
    hipLaunchKernelGGL(profile_keys_kernel<decltype(k)::value>, dim3(blocks), dim3(kProfileThreads), 0, s, rec,
                       reinterpret_cast<const uint32_t*>(rows), W, reinterpret_cast<const v4f*>(stats), M, P,
                       (int32_t)track, (int32_t)score, modes, pe, keys, vals,
                       reinterpret_cast<unsigned long long*>(cells));
  });
  return (int)hipGetLastError();
}

int launch_profile_fold(const uint32_t* keys, const uint32_t* vals, const float* stats, int64_t n, int K, int64_t P,
                        int32_t* table, void* edges, hipStream_t s) {
  if (K < 1 || K > kMaxTeamSize || n < 0 || n > kMaxSlots || n % (2 * K) || P < 0 || P > 0x7fffffffll ||
      reinterpret_cast<uintptr_t>(stats) % 16 != 0 || reinterpret_cast<uintptr_t>(table) % 16 != 0 ||
      reinterpret_cast<uintptr_t>(edges) % 16 != 0)
    return (int)hipErrorInvalidValue;
  if (n == 0 || P == 0) return 0;
  const int64_t tiles = profile_tiles(n);
  int32_t* e = static_cast<int32_t*>(edges);
  hipLaunchKernelGGL(profile_fold_kernel, dim3((unsigned)tiles), dim3(kProfileThreads), 0, s, keys, vals,
                     reinterpret_cast<const v4f*>(stats), n, (uint32_t)P, table, e);
  hipLaunchKernelGGL(profile_stitch_kernel, dim3(1), dim3(kProfileThreads), 0, s, e, 2 * tiles, (uint32_t)P, table);
  return (int)hipGetLastError();
}

}  // namespace ana
