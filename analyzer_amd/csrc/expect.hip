// K19 expectations: every player's predicted against actual results (expect_core.h), folded from
// one window of the match stream rec [M][2K+2] joined with the raw priors [M][4][2K] and the pred
// rows [M][kPredWords] K14 made of it.
//
// The player table [P][kExpectWords] is updated in place, window by window.  Every sum is an
// integer, so it is the same bits for any grid, tile size or launch order.  A player row has one
// writer per launch.  Four steps on one stream, ordered by the stream alone:
//
//   keys    one lane per match (the vector record loads of select.hip) and one 16-B load of its
//           pred row.  Behind a scored row the lane loads the 2K (track mode: 4K) prior mu words
//           with 16-B and 8-B loads, forms the two roster sums once and writes per slot the sort
//           key -- the player id of a game, else P --, the value slot | won << 31 and, for a game,
//           its 32-B term record as two 16-B stores.  The priors of a match that is not scored are
//           never loaded, a slot that is no game writes no term, and bad own values are counted
//           with one integer atomicAdd per workgroup that has any.
//   sort    launch_radix_sort_pairs on bit_length(P) bits; the slots that are no game sort last.
//   fold    the run fold of fold_dev.h over tiles of kExpectTile sorted elements under
//   stitch  expect_combine and expect_row_add: a lane gathers its slot's 32-B term record.
//
// Built with -ffp-contract=off: rint(p * 2^24) and rint(mu * 256) are the products the host forms.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "common.h"
#include "expect_core.h"
#include "fold_dev.h"
#include "kernels.h"
#include "record_dev.h"

namespace ana {

namespace {

constexpr int kExpectThreads = 256;

typedef unsigned int v2u __attribute__((ext_vector_type(2)));
typedef unsigned int v4u __attribute__((ext_vector_type(4)));

// N consecutive words from a 16-B aligned address: 16-B loads and, for N % 4 == 2, one 8-B load
template <int N>
__device__ __forceinline__ void load_words(const uint32_t* __restrict__ p, uint32_t* w) {
  static_assert(N % 2 == 0, "a field of a match's priors is 2K words");
#pragma unroll
  for (int q = 0; q < N / 4; ++q) {
    const v4u x = reinterpret_cast<const v4u*>(p)[q];
#pragma unroll
    for (int c = 0; c < 4; ++c) w[4 * q + c] = x[c];
  }
  if constexpr (N % 4 == 2) {
    const v2u x = *reinterpret_cast<const v2u*>(p + N - 2);
    w[N - 2] = x[0];
    w[N - 1] = x[1];
  }
}

template <int K>
__global__ void __launch_bounds__(kExpectThreads) expect_keys_kernel(
    const int32_t* __restrict__ rec, const uint32_t* __restrict__ priors, const v4i* __restrict__ pred, int64_t M,
    int64_t P, int32_t track, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals, v4i* __restrict__ terms,
    unsigned long long* __restrict__ bad) {
  constexpr int S = 2 * K;
  __shared__ int32_t wg_bad;
  if (threadIdx.x == 0) wg_bad = 0;
  __syncthreads();
  const int64_t m = (int64_t)blockIdx.x * kExpectThreads + threadIdx.x;
  int32_t my_bad = 0;
  if (m < M) {
    int32_t r[S + 2];
    load_record<K>(rec, m, r);
    const v4i pr = pred[m];
    const uint32_t mask = expect_game_mask<K>(r, P, (uint32_t)pr[0], (uint32_t)pr[1]);
    uint32_t mu[S];
#pragma unroll
    for (int j = 0; j < S; ++j) mu[j] = kPriorNull;
    if (mask) {
      const uint32_t* src = priors + m * (4 * S);  // 32K bytes per match: every field pair is 16-B aligned
      load_words<S>(src, mu);
      if (track == kScoreMode) {
        uint32_t mm[S];
        load_words<S>(src + 2 * S, mm);
#pragma unroll
        for (int j = 0; j < S; ++j) mu[j] = expect_raw(track, mu[j], mm[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < S; ++j) {
      const int64_t i = m * S + j;
      const bool game = (mask >> j) & 1u;
      const bool won = game && profile_won<K>(r, j);
      keys[i] = game ? (uint32_t)r[j] : (uint32_t)P;
      vals[i] = (uint32_t)i | (won ? kExpectWonBit : 0u);
    }
    if (mask) {
      my_bad = expect_terms<K>(mask, (uint32_t)pr[1], (uint32_t)pr[2], mu, [&](int j, const int32_t* t) {
        v4i a, b;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          a[d] = t[d];
          b[d] = t[4 + d];
        }
        v4i* dst = terms + 2 * (m * S + j);
        dst[0] = a;
        dst[1] = b;
      });
    }
  }
  if (my_bad) atomicAdd(&wg_bad, my_bad);
  __syncthreads();
  if (threadIdx.x == 0 && wg_bad) atomicAdd(bad, (unsigned long long)wg_bad);
}

struct ExpectFeature {
  typedef ExpectRun Run;
  static constexpr int kWords = kExpectWords;
  static __device__ __forceinline__ ExpectRun empty() { return expect_empty(); }
  static __device__ __forceinline__ ExpectRun combine(const ExpectRun& a, const ExpectRun& b) {
    return expect_combine(a, b);
  }
  static __device__ __forceinline__ void row_add(int32_t* row, const ExpectRun& run) { expect_row_add(row, run); }
};
typedef RunFold<ExpectFeature, kExpectThreads, kExpectTile> ExpectFold;

__global__ void __launch_bounds__(kExpectThreads) expect_fold_kernel(
    const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, const v4i* __restrict__ terms, int64_t n,
    uint32_t P, int32_t* __restrict__ table, int32_t* __restrict__ edges) {
  // a lane gathers its slot's 32-B term record; the won bit rides in the value
  ExpectFold::fold(keys, vals, n, P, table, edges, [&](uint32_t v) {
    const int64_t slot = (int64_t)(v & kExpectSlotMask);
    if (slot >= n) return expect_empty();  // never: the slot indices are a permutation of the slots
    const v4i a = terms[2 * slot], b = terms[2 * slot + 1];
    int32_t t[kExpectTermWords];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      t[d] = a[d];
      t[4 + d] = b[d];
    }
    return expect_game(t, (v & kExpectWonBit) != 0u);
  });
}

__global__ void __launch_bounds__(kExpectThreads) expect_stitch_kernel(const int32_t* __restrict__ edges, int64_t E,
                                                                       uint32_t P, int32_t* __restrict__ table) {
  ExpectFold::stitch(edges, E, P, table);
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

size_t expect_edge_bytes(int64_t n) { return ExpectFold::edge_bytes(n); }

int launch_expect_keys(int K, const int32_t* rec, const float* priors, const int32_t* pred, int64_t M, int64_t P,
                       int track, uint32_t* keys, uint32_t* vals, int32_t* terms, int64_t* bad, hipStream_t s) {
  // the window carries no output rows: the narrowest row the shared check takes stands in
  if (!window_slots_ok(K, 5 * 2 * K + 2, M, P) || (track != kScoreShared && track != kScoreMode) || bad == nullptr ||
      !aligned16(priors) || !aligned16(pred) || !aligned16(terms) ||
      reinterpret_cast<uintptr_t>(rec) % (K % 2 == 0 ? 8 : 16) != 0)
    return (int)hipErrorInvalidValue;
  if (M == 0) return 0;
  const unsigned blocks = (unsigned)((M + kExpectThreads - 1) / kExpectThreads);
  with_team_size(K, [&](auto k) {
    hipLaunchKernelGGL(expect_keys_kernel<decltype(k)::value>, dim3(blocks), dim3(kExpectThreads), 0, s, rec,
                       reinterpret_cast<const uint32_t*>(priors), reinterpret_cast<const v4i*>(pred), M, P,
                       (int32_t)track, keys, vals, reinterpret_cast<v4i*>(terms),
                       reinterpret_cast<unsigned long long*>(bad));
  });
  return (int)hipGetLastError();
}

int launch_expect_fold(const uint32_t* keys, const uint32_t* vals, const int32_t* terms, int64_t n, int K, int64_t P,
                       int32_t* table, void* edges, hipStream_t s) {
  if (!sorted_slots_ok(K, n, P) || !aligned16(terms) || !aligned16(table) || !aligned16(edges))
    return (int)hipErrorInvalidValue;
  if (n == 0 || P == 0) return 0;
  const int64_t tiles = ExpectFold::tiles(n);
  int32_t* e = static_cast<int32_t*>(edges);
  hipLaunchKernelGGL(expect_fold_kernel, dim3((unsigned)tiles), dim3(kExpectThreads), 0, s, keys, vals,
                     reinterpret_cast<const v4i*>(terms), n, (uint32_t)P, table, e);
  hipLaunchKernelGGL(expect_stitch_kernel, dim3(1), dim3(kExpectThreads), 0, s, e, 2 * tiles, (uint32_t)P, table);
  return (int)hipGetLastError();
}

}  // namespace ana
