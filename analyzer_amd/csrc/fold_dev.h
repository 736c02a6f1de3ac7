// The run fold of the per-player tables (K13 careers, K17 profiles, K19 expectations): the fold and stitch
// kernels behind "sort a window's slots by player, fold each player's run into its row".
// docs/ARCHITECTURE.md ("The shared scans", the run fold) says what it guarantees.
//
// A feature type F supplies
//   F::Run                        the summary of a stretch of one player's games
//   F::kWords                     the row width in int32 words, whole 16-B pieces
//   F::empty()                    the identity of combine
//   F::combine(a, b)              a earlier; associative
//   F::row_add(int32_t* row, r)   row = row then r, on a row held in registers
// and each of its two kernels is one call: RunFold<F, kThreads, kTile>::fold with a gather
// callable (sort value -> the run of that one game) and ::stitch.
//
// K14 and K16 (score.hip prior_tile_kernel<*>, prior_stitch_kernel; hindsight.hip likewise) do
// not belong here but in chain_dev.h: their scan is seeded from the row it ends in, over three
// kernels, and who owns a row differs -- here a row is only ever added to.
#pragma once

#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include "record_dev.h"
#include "scan_dev.h"

namespace ana {

template <class F, int kThreads, int kTile>
struct RunFold {
  typedef typename F::Run Run;
  struct Ops {
    static __device__ __forceinline__ Run combine(const Run& a, const Run& b) { return F::combine(a, b); }
    static __device__ __forceinline__ Run identity() { return F::empty(); }
  };
  // on return from step a lane's run covers its key from the key's first element of this workgroup
  typedef SegScan<kThreads, Run, Ops> Scan;

  static constexpr int kIters = kTile / kThreads;
  static_assert(kTile % kThreads == 0, "a tile is a whole number of iterations");
  // an edge: [key, -, Run]
  static constexpr int kEdgeWords = 2 + (int)(sizeof(Run) / 4);
  static_assert(sizeof(Run) % 4 == 0 && kEdgeWords % 4 == 0, "an edge is whole 16-B pieces");
  static_assert(F::kWords % 4 == 0, "a row is whole 16-B pieces");

  // host: two edges per tile of the n sorted elements
  static int64_t tiles(int64_t n) { return (n + kTile - 1) / kTile; }
  static size_t edge_bytes(int64_t n) { return (size_t)(2 * tiles(n) * kEdgeWords) * 4; }

  static __device__ __forceinline__ void row_add(int32_t* __restrict__ table, uint32_t p, const Run& run) {
    v4i* q = reinterpret_cast<v4i*>(table + (int64_t)p * F::kWords);
    int32_t row[F::kWords];
#pragma unroll
    for (int c = 0; c < F::kWords / 4; ++c) {
      const v4i x = q[c];
#pragma unroll
      for (int d = 0; d < 4; ++d) row[4 * c + d] = x[d];
    }
    F::row_add(row, run);
#pragma unroll
    for (int c = 0; c < F::kWords / 4; ++c) {
      v4i x;
#pragma unroll
      for (int d = 0; d < 4; ++d) x[d] = row[4 * c + d];
      q[c] = x;
    }
  }

  static __device__ __forceinline__ void edge_store(int32_t* __restrict__ edges, int64_t e, uint32_t key,
                                                    const Run& run) {
    int32_t* w = edges + e * kEdgeWords;
    w[0] = (int32_t)key;
    state_store(reinterpret_cast<Run*>(w + 2), run);
  }

  // One workgroup per tile of the sorted (keys, vals) [n]; keys >= P are no game and sort last.
  // gather(val) is the run of one game and is called only for an element with key < P.  A run
  // strictly inside the tile is folded into its row by the lane of its last element; the runs
  // of the tile's first and last key go to edges[2 * tile + 0 / 1], as they may go on in a
  // neighbour tile (a tile of one key: the run and an empty one).
  template <class Gather>
  static __device__ __forceinline__ void fold(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                              int64_t n, uint32_t P, int32_t* __restrict__ table,
                                              int32_t* __restrict__ edges, Gather&& gather) {
    __shared__ typename Scan::Lds lds;
    const int t = threadIdx.x;
    const int64_t lo = (int64_t)blockIdx.x * kTile;
    const int64_t hi = lo + kTile < n ? lo + kTile : n;
    const uint32_t head = keys[lo];
    if (head >= P) {  // sorted: nothing but slots that are no game from here on
      if (t < 2) edges[(2 * (int64_t)blockIdx.x + t) * kEdgeWords] = (int32_t)kNoKey;
      return;  // before init: no lane of this workgroup enters the scan
    }
    Scan::init(lds);
    for (int it = 0; it < kIters; ++it) {
      const int64_t i = lo + (int64_t)it * kThreads + t;
      if (lo + (int64_t)it * kThreads >= hi) break;  // uniform over the workgroup
      const bool valid = i < hi;
      const uint32_t key = valid ? keys[i] : kNoKey;
      const uint32_t next = valid && i + 1 < n ? keys[i + 1] : kNoKey;
      Run run = F::empty();
      if (valid && key < P) run = gather(vals[i]);
      Scan::step(lds, it, key, run);
      const bool tail = i + 1 == hi;
      if (valid && (tail || next != key)) {  // the last element of its key in this tile
        if (key == head) {
          edge_store(edges, 2 * (int64_t)blockIdx.x, key, run);
          if (tail) edge_store(edges, 2 * (int64_t)blockIdx.x + 1, key, F::empty());
        } else if (tail) {
          edge_store(edges, 2 * (int64_t)blockIdx.x + 1, key, run);
        } else if (key < P) {
          row_add(table, key, run);
        }
      }
    }
  }

  // One workgroup over the edges [E] in tile order: the last edge of each player folds the
  // stitched run into its row.  A player cut by a tile edge is folded here and only here.
  static __device__ __forceinline__ void stitch(const int32_t* __restrict__ edges, int64_t E, uint32_t P,
                                                int32_t* __restrict__ table) {
    __shared__ typename Scan::Lds lds;
    const int t = threadIdx.x;
    Scan::init(lds);
    const int iters = (int)((E + kThreads - 1) / kThreads);
    // the edge of the next iteration is loaded ahead of this one's scan: the loop is one
    // workgroup's latency chain
    uint32_t key_n, next_n;
    Run run_n;
    const auto load = [&](int it) {
      const int64_t e = (int64_t)it * kThreads + t;
      key_n = e < E ? (uint32_t)edges[e * kEdgeWords] : kNoKey;
      next_n = e + 1 < E ? (uint32_t)edges[(e + 1) * kEdgeWords] : kNoKey;
      run_n = F::empty();
      if (key_n < P) run_n = state_load(reinterpret_cast<const Run*>(edges + e * kEdgeWords + 2));
    };
    load(0);
    for (int it = 0; it < iters; ++it) {
      const uint32_t key = key_n, next = next_n;
      Run run = run_n;
      if (it + 1 < iters) load(it + 1);
      Scan::step(lds, it, key, run);
      if (key < P && next != key) row_add(table, key, run);
    }
  }
};

}  // namespace ana
