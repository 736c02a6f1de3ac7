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
//   fold    the run fold of fold_dev.h over tiles of kProfileTile sorted elements under
//   stitch  profile_combine and profile_row_add: a lane gathers its slot's 32 B of stats and
//           forms the terms of a run of one game (profile_game).
//
// Built with -ffp-contract=off: the score is the one IEEE subtraction the host mirror does.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "common.h"
#include "fold_dev.h"
#include "kernels.h"
#include "profile_core.h"
#include "record_dev.h"

namespace ana {

namespace {

constexpr int kProfileThreads = 256;

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

struct ProfileFeature {
  typedef ProfileRun Run;
  static constexpr int kWords = kProfileWords;
  static __device__ __forceinline__ ProfileRun empty() { return profile_empty(); }
  static __device__ __forceinline__ ProfileRun combine(const ProfileRun& a, const ProfileRun& b) {
    return profile_combine(a, b);
  }
  static __device__ __forceinline__ void row_add(int32_t* row, const ProfileRun& run) { profile_row_add(row, run); }
};
typedef RunFold<ProfileFeature, kProfileThreads, kProfileTile> ProfileFold;

__global__ void __launch_bounds__(kProfileThreads) profile_fold_kernel(
    const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, const v4f* __restrict__ stats, int64_t n,
    uint32_t P, int32_t* __restrict__ table, int32_t* __restrict__ edges) {
  // a lane gathers its slot's 32 B of stats and forms the terms; the won bit rides in the value
  ProfileFold::fold(keys, vals, n, P, table, edges, [&](uint32_t v) {
    const int64_t slot = (int64_t)(v & kProfileSlotMask);
    if (slot >= n) return profile_empty();  // never: the slot indices are a permutation of the slots
    float x[kProfileStats];
    load_stats(stats, slot, x);
    int32_t bad = 0;  // counted by the keys kernel
    return profile_game(x, (v & kProfileWonBit) != 0u, bad);
  });
}

__global__ void __launch_bounds__(kProfileThreads) profile_stitch_kernel(const int32_t* __restrict__ edges, int64_t E,
                                                                         uint32_t P, int32_t* __restrict__ table) {
  ProfileFold::stitch(edges, E, P, table);
}

}  // namespace

size_t profile_edge_bytes(int64_t n) { return ProfileFold::edge_bytes(n); }

static bool profile_edges_ok(const float* edges, int n_edges) {
  if (n_edges < 0 || n_edges > kProfileMaxEdges || (n_edges > 0 && edges == nullptr)) return false;
  for (int i = 0; i < n_edges; ++i)
    if (!(edges[i] - edges[i] == 0.0f) || (i > 0 && !(edges[i - 1] < edges[i]))) return false;
  return true;
}

int launch_profile_keys(int K, const int32_t* rec, const float* rows, int64_t W, const float* stats, int64_t M,
                        int64_t P, int track, int score, uint32_t modes, const float* edges, int n_edges,
                        uint32_t* keys, uint32_t* vals, int64_t* cells, hipStream_t s) {
  if (!window_slots_ok(K, W, M, P) || !career_options_ok(track, score, modes) || !profile_edges_ok(edges, n_edges) || cells == nullptr || reinterpret_cast<uintptr_t>(stats) % 16 != 0)
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
  if (!sorted_slots_ok(K, n, P) || reinterpret_cast<uintptr_t>(stats) % 16 != 0 || reinterpret_cast<uintptr_t>(table) % 16 != 0 ||
      reinterpret_cast<uintptr_t>(edges) % 16 != 0)
    return (int)hipErrorInvalidValue;
  if (n == 0 || P == 0) return 0;
  const int64_t tiles = ProfileFold::tiles(n);
  int32_t* e = static_cast<int32_t*>(edges);
  hipLaunchKernelGGL(profile_fold_kernel, dim3((unsigned)tiles), dim3(kProfileThreads), 0, s, keys, vals,
                     reinterpret_cast<const v4f*>(stats), n, (uint32_t)P, table, e);
  hipLaunchKernelGGL(profile_stitch_kernel, dim3(1), dim3(kProfileThreads), 0, s, e, 2 * tiles, (uint32_t)P, table);
  return (int)hipGetLastError();
}

}  // namespace ana
