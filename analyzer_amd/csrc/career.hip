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
//   fold    the run fold of fold_dev.h over tiles of kCareerTile sorted elements under
//   stitch  career_combine and career_row_add: a lane gathers its game's 8-B event and makes
//           it a run of one (career_game).  Cost per element is the same for every key
//           distribution.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "career_core.h"
#include "common.h"
#include "fold_dev.h"
#include "kernels.h"
#include "record_dev.h"

namespace ana {

namespace {

constexpr int kCareerThreads = 256;

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

struct CareerFeature {
  typedef CareerRun Run;
  static constexpr int kWords = kCareerWords;
  static __device__ __forceinline__ CareerRun empty() { return career_empty(); }
  static __device__ __forceinline__ CareerRun combine(const CareerRun& a, const CareerRun& b) {
    return career_combine(a, b);
  }
  static __device__ __forceinline__ void row_add(int32_t* row, const CareerRun& run) { career_row_add(row, run); }
};
typedef RunFold<CareerFeature, kCareerThreads, kCareerTile> CareerFold;

__global__ void __launch_bounds__(kCareerThreads) career_fold_kernel(
    const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, const v2u* __restrict__ events, int64_t n,
    uint32_t S, int64_t base, uint32_t P, int32_t* __restrict__ table, int32_t* __restrict__ edges) {
  // a lane gathers its game's 8-B event; the value is the slot, so slot / 2K is the match
  CareerFold::fold(keys, vals, n, P, table, edges, [&](uint32_t v) {
    if ((int64_t)v >= n) return career_empty();  // never: the values are a permutation of the slots
    const v2u ev = events[v];
    return career_game(ev[0], ev[1], base + (int64_t)(v / S));
  });
}

__global__ void __launch_bounds__(kCareerThreads) career_stitch_kernel(const int32_t* __restrict__ edges, int64_t E,
                                                                       uint32_t P, int32_t* __restrict__ table) {
  CareerFold::stitch(edges, E, P, table);
}

}  // namespace

size_t career_edge_bytes(int64_t n) { return CareerFold::edge_bytes(n); }

int launch_career_keys(int K, const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t P, int track,
                       int score, uint32_t modes, uint32_t* keys, uint32_t* vals, uint32_t* events, hipStream_t s) {
  if (!window_slots_ok(K, W, M, P) || !career_options_ok(track, score, modes)) return (int)hipErrorInvalidValue;
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
  if (!sorted_slots_ok(K, n, P) || base < 0) return (int)hipErrorInvalidValue;
  if (n == 0 || P == 0) return 0;
  const int64_t tiles = CareerFold::tiles(n);
  int32_t* e = static_cast<int32_t*>(edges);
  hipLaunchKernelGGL(career_fold_kernel, dim3((unsigned)tiles), dim3(kCareerThreads), 0, s, keys, vals,
                     reinterpret_cast<const v2u*>(events), n, (uint32_t)(2 * K), base, (uint32_t)P, table, e);
  hipLaunchKernelGGL(career_stitch_kernel, dim3(1), dim3(kCareerThreads), 0, s, e, 2 * tiles, (uint32_t)P, table);
  return (int)hipGetLastError();
}

}  // namespace ana
