// The chained scan of the per-player tables that are read and written in place (K14 scorecard
// priors, K16 hindsight): the summaries, stitch and apply kernels behind "sort a window's slots
// by player, scan each player's run seeded from its row, leave the run's end in the row".
// docs/ARCHITECTURE.md ("The shared scans", the chained scan) says what it guarantees.
//
// The input is the sorted pairs (keys, vals) [n] of a window's slots; keys >= P are no element
// and sort last.  Three stream-ordered launches, no atomics, no workgroup waits on another:
//   summaries  tile<false>, one workgroup per tile: the segmented scan of the elements' terms
//              without any seed.  The runs of the tile's first and last key, the only ones that
//              can go on in a neighbour tile, leave their totals in edges[2 * tile + 0 / 1] (a
//              tile of one key: the total and the identity; no key < P there: kNoKey).
//   stitch     one workgroup: the same scan over the 2 * tiles edges in tile order.  The first
//              edge of a key contributes the seed of the key's row, every other edge the total
//              of the edge before it, so seeds[e] is the state in front of edge e's stretch,
//              the row included; the last edge of a key stores the row.
//   apply      tile<true>: the summaries scan again, the first element of a key in the tile
//              seeded from seeds[2 * tile] (the tile's first key), seeds[2 * tile + 1] (its last
//              key) or, for a run strictly inside the tile, from the key's row.  Every element
//              is emitted; the last element of an inner run stores the row.
//
// The table in place, without a race.  Summaries only reads rows (F::open), and every later
// launch starts after it has finished.  From then on a key's row has one reader, the step that
// seeds the globally first element of the key, and one writer, the step that holds the globally
// last, and the written value depends on the read one through the scan.  A run inside one tile
// that is neither the tile's first nor last key is read and written by that tile's apply
// workgroup alone: the first element's lane loads the row, the scan (shuffles, LDS, barriers)
// carries it to the last element's lane, which stores; no other workgroup sees the key.  Every
// other run -- across tiles or touching a tile's end -- is in the edges, and its row is read
// and written by the stitch workgroup alone, first edge to last edge through the same scan;
// apply never touches that row and takes what lies in front from seeds, which stitch filled
// before it overwrote the row.  The code below holds every F::seed and F::row_store there is:
// two of each, under `!edge_run` in apply and under first / last in stitch.
//
// A feature type F supplies F::State, F::identity() and the associative F::combine(a, b) (a
// earlier in the scan); F::seed(table, key), the row of a key as the state in front of its run,
// and F::row_store(table, key, s), the row from the state at the run's end; and, on an object f
// with whatever else its kernels take, what an element with a key < P and the sort value v means:
//   f.next(prev, v)                 its term behind an element (sort value prev) of its key in the tile
//   f.first(v, seed)                its term as the first of its key in the tile, under apply
//   f.open(v, key, newest, table)   the same under summaries, where the seed is not known yet; newest: it
//                                   is the key's first of the whole window; the table may only be read
//   f.total(v, s)                   the run's total through it, from its scanned state s
//   f.emit(v, s)                    its output under apply
#pragma once

#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include "scan_dev.h"

namespace ana {

template <class F, int kThreads, int kTile>
struct ChainScan {
  typedef typename F::State State;
  // on return from step a lane's state covers the terms of its key from the first one this
  // workgroup saw up to the lane's
  typedef SegScan<kThreads, State, F> Scan;
  static constexpr int kIters = kTile / kThreads;
  static_assert(kTile % kThreads == 0, "a tile is a whole number of iterations");
  // an edge or a seed: its key and a state, at the offset the state's alignment asks for
  struct Edge {
    uint32_t key;
    State s;
  };
  static_assert(offsetof(Edge, s) == (alignof(State) > 4 ? alignof(State) : 4), "no padding but the state's own");

  // host: edges and seeds, 2 * tiles entries each, of the n sorted elements
  static int64_t tiles(int64_t n) { return (n + kTile - 1) / kTile; }
  static size_t edge_bytes(int64_t n) { return (size_t)(2 * 2 * tiles(n)) * sizeof(Edge); }

  static __device__ __forceinline__ void edge_store(Edge* edges, int64_t e, uint32_t key, const State& s) {
    edges[e].key = key;
    state_store(&edges[e].s, s);
  }

  // summaries (APPLY = false) and apply (APPLY = true) over one tile of the sorted keys [n]
  template <bool APPLY, class Cell>
  static __device__ __forceinline__ void tile(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                              int64_t n, uint32_t P, Cell* __restrict__ table, Edge* __restrict__ edges,
                                              const Edge* __restrict__ seeds, const F& f) {
    __shared__ typename Scan::Lds lds;
    const int t = threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int64_t lo = tile * kTile;
    const int64_t hi = lo + kTile < n ? lo + kTile : n;
    const uint32_t head = keys[lo], tailkey = keys[hi - 1];
    if (head >= P) {  // sorted: nothing but slots that are no element from here on
      if (!APPLY && t < 2) edges[2 * tile + t].key = kNoKey;
      return;  // before init: no lane of this workgroup enters the scan
    }
    Scan::init(lds);
    for (int it = 0; it < kIters; ++it) {
      const int64_t i = lo + (int64_t)it * kThreads + t;
      if (lo + (int64_t)it * kThreads >= hi) break;  // uniform over the workgroup
      const bool valid = i < hi;
      const uint32_t key = valid ? keys[i] : kNoKey;
      const bool has = valid && key < P;
      const bool first = !(valid && i > lo && keys[i - 1] == key);  // of its key in this tile
      const bool last = valid && (i + 1 == hi || keys[i + 1] != key);
      const uint32_t v = has ? vals[i] : 0u;
      State s = F::identity();
      if (has) {
        if (!first) {
          s = f.next(vals[i - 1], v);
        } else if (APPLY) {
          s = f.first(v, key == head      ? state_load(&seeds[2 * tile].s)
                         : key == tailkey ? state_load(&seeds[2 * tile + 1].s)
                                          : F::seed(table, key));
        } else {
          // the key's first element of the window, unless its run began in the tile before
          s = f.open(v, key, i == 0 || keys[i - 1] != key, table);
        }
      }
      Scan::step(lds, it, key, s);
      if (APPLY) {
        const bool edge_run = key == head || key == tailkey;  // its row is the stitch's
        if (has) f.emit(v, s);
        if (has && last && !edge_run) F::row_store(table, key, f.total(v, s));
      } else if (valid && (i + 1 == hi || (last && key == head))) {
        // the last element of the first key, and the tile's last element
        const State total = has ? f.total(v, s) : F::identity();
        if (key == head) {
          edge_store(edges, 2 * tile, key, total);
          if (i + 1 == hi) edge_store(edges, 2 * tile + 1, key, F::identity());
        } else {
          edge_store(edges, 2 * tile + 1, has ? key : kNoKey, total);
        }
      }
    }
  }

  // one workgroup over the edges [E] in tile order
  template <class Cell>
  static __device__ __forceinline__ void stitch(const Edge* __restrict__ edges, int64_t E, uint32_t P,
                                                Cell* __restrict__ table, Edge* __restrict__ seeds) {
    __shared__ typename Scan::Lds lds;
    const int t = threadIdx.x;
    Scan::init(lds);
    const int iters = (int)((E + kThreads - 1) / kThreads);
    for (int it = 0; it < iters; ++it) {
      const int64_t e = (int64_t)it * kThreads + t;
      const uint32_t key = e < E ? edges[e].key : kNoKey;
      const bool has = key < P;
      const bool first = !(e > 0 && e < E && edges[e - 1].key == key);
      const bool last = !(e + 1 < E && edges[e + 1].key == key);
      State s = F::identity();
      if (has) s = first ? F::seed(table, key) : state_load(&edges[e - 1].s);
      Scan::step(lds, it, key, s);  // the state in front of edge e's stretch
      if (has) {
        state_store(&seeds[e].s, s);
        if (last) F::row_store(table, key, F::combine(s, state_load(&edges[e].s)));
      }
    }
  }
};

}  // namespace ana
