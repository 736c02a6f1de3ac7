// K16 hindsight: the smoothed (mu, sigma) of every element of a window, from the match stream
// rec [M][2K+2] joined with its packed output rows [M][W] (hindsight_core.h: the model, the
// maps, the order of the scan and the error budget).
//
// Windows are added NEWEST FIRST.  carry [P][2] fp64 holds per player (mh, Ph) of its oldest
// element added so far -- what lies behind the next, older window -- and NaN while the player
// has none.  It is updated in place.  No float atomics, and no workgroup waits on another:
// five stream-ordered steps.
//
//   keys       one lane per match: per slot i = m * 2K + j, written at the mirrored position
//              n - 1 - i, the sort key -- the player of an element, else P -- and the value i;
//              at events[i] the 8-B (mu, sigma) bits of an element, so the later passes never
//              touch the 128-B row line.  A slot that is not an element gets its (NaN, NaN)
//              at out[i] here, and sorts last; a bad one adds 1 to *bad (an integer atomicAdd,
//              one per workgroup that has any).
//   sort       launch_radix_sort_pairs on bit_length(P) bits: stable, so each player's elements
//              come out newest first.
//   summaries  one workgroup per tile of kHindsightTile sorted elements: the inclusive SegScan
//              of the elements' maps.  The newest element of a player in the window whose
//              carry row is NaN is the chain's newest, a constant; every other element is its
//              map.  The runs of the tile's first and last key, the only ones that can go on
//              in a neighbour tile, leave their totals (without anything behind them) in
//              edges[2 * tile + 0 / 1].
//   stitch     one workgroup: the same scan over the 2 * tiles edges in tile order.  The first
//              edge of a key, its newest stretch, contributes the key's carry row as a seed
//              (the identity for a NaN row), every other edge the total of the edge before
//              it, so seeds[e] is what lies behind edge e's stretch; the last edge of a key
//              stores the new carry row.
//   apply      the summaries scan again, now seeded: the first element of a key in the tile
//              takes seeds[2 * tile] (the tile's first key), seeds[2 * tile + 1] (its last
//              key) or, for a run strictly inside the tile, the key's carry row.  Every
//              element stores its 8-B (mh, sqrt(Ph)) as fp32 at out[slot], slot-major
//              [M][2K][2], which is the public layout; the last (oldest) element of an inner
//              run stores its carry row.
//
// The table in place, without a race.  summaries only reads carry rows, and every later step
// starts after it has finished.  From then on a key's row has one reader, the step that seeds
// the key's newest element in the window, and one writer, the step that holds its oldest, and
// the written value depends on the read one through the scan.  A run inside one tile that is
// neither the tile's first nor last key is read and written by that tile's apply workgroup
// alone: the newest element's lane loads the row, the scan (shuffles, LDS, barriers) carries it
// to the oldest element's lane, which stores; no other workgroup sees the key.  Every other run
// -- across tiles or touching a tile's end -- is in the edges, and its row is read and written
// by the stitch workgroup alone, first edge to last edge through the same scan; apply never
// touches that row and takes what lies behind from seeds, which stitch filled before it
// overwrote the row.  Whether a seed is "nothing" survives the overwrite as the identity in
// seeds (hindsight_core.h: B == 1 against the B == 0 of every constant).
//
// Built with -ffp-contract=off: every fp64 operation is the one written.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "common.h"
#include "hindsight_core.h"
#include "kernels.h"
#include "record_dev.h"
#include "scan_dev.h"

namespace ana {

namespace {

constexpr int kHsThreads = 256;
constexpr int kHsIters = kHindsightTile / kHsThreads;
static_assert(kHindsightTile % kHsThreads == 0, "a tile is a whole number of iterations");

typedef unsigned int v2u __attribute__((ext_vector_type(2)));

// an edge or a seed: its key and a map, 32 B
struct HsEdge {
  uint32_t key, pad;
  HsMap s;
};
static_assert(sizeof(HsEdge) == 32 && alignof(HsEdge) == 8, "an edge is four 8-B pieces");

template <int K>
__global__ void __launch_bounds__(kHsThreads) hindsight_keys_kernel(
    const int32_t* __restrict__ rec, const uint32_t* __restrict__ rows, int64_t W, int64_t M, int64_t P,
    int32_t track, int32_t mode, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
    v2u* __restrict__ events, v2u* __restrict__ out, int32_t* __restrict__ bad) {
  constexpr int S = 2 * K;
  __shared__ int32_t wg_bad;
  if (threadIdx.x == 0) wg_bad = 0;
  __syncthreads();
  const int64_t m = (int64_t)blockIdx.x * kHsThreads + threadIdx.x;
  int32_t my_bad = 0;
  if (m < M) {
    const int64_t n = M * S;
    int32_t r[S + 2];
    load_record<K>(rec, m, r);
    const uint32_t live = prior_live_mask<K>(r, P);
    uint32_t elems = 0u;
    uint32_t ms[2 * S];  // (mu[S], sigma[S]) of the track, as 8-B loads
    if (live) {
      const uint32_t* row = rows + m * W;
      const v2u tail = *reinterpret_cast<const v2u*>(row + 5 * S);
      elems = hs_element_mask<K>(r, live, tail[1] & 0xffu, track, mode);
      if (elems) {
        const v2u* a = reinterpret_cast<const v2u*>(row + (track == kHsMode ? 3 * S : 0));
#pragma unroll
        for (int c = 0; c < S; ++c) {
          const v2u x = a[c];
          ms[2 * c] = x[0];
          ms[2 * c + 1] = x[1];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < S; ++j) {
      const int64_t i = m * S + j;
      bool el = (elems >> j) & 1u;
      v2u e;
      e[0] = e[1] = kHsNull;
      if (el) {
        e[0] = ms[j];
        e[1] = ms[S + j];
        if (!hs_value_ok(__uint_as_float(e[0]), __uint_as_float(e[1]))) {
          el = false;
          ++my_bad;
        }
      }
      keys[n - 1 - i] = el ? (uint32_t)r[j] : (uint32_t)P;
      vals[n - 1 - i] = (uint32_t)i;
      if (el) {
        events[i] = e;
      } else {
        v2u none;
        none[0] = none[1] = kHsNull;
        out[i] = none;
      }
    }
  }
  if (my_bad) atomicAdd(&wg_bad, my_bad);
  __syncthreads();
  if (threadIdx.x == 0 && wg_bad) atomicAdd(bad, wg_bad);
}

struct HsOps {
  static __device__ __forceinline__ HsMap combine(const HsMap& x, const HsMap& y) { return hs_scan_combine(x, y); }
  static __device__ __forceinline__ HsMap identity() { return hs_identity(); }
};
// on return from step a lane's state is the composition of the maps of its key from the lane's
// element to the newest one this workgroup saw
typedef SegScan<kHsThreads, HsMap, HsOps> HsScan;

__device__ __forceinline__ HsMap carry_seed(const double* __restrict__ carry, uint32_t key) {
  const double* row = carry + (int64_t)key * 2;
  return hs_seed_of_row(row[0], row[1]);
}

// s ends in a constant: the smoothed (mh, Ph) of its oldest element
__device__ __forceinline__ void carry_store(double* __restrict__ carry, uint32_t key, const HsMap& s) {
  double* row = carry + (int64_t)key * 2;
  row[0] = s.A;
  row[1] = s.C;
}

__device__ __forceinline__ void edge_store(HsEdge* __restrict__ edges, int64_t e, uint32_t key, const HsMap& s) {
  edges[e].key = key;
  state_store(&edges[e].s, s);
}

// summaries (APPLY = false) and apply (APPLY = true) over one tile of the sorted pairs
template <bool APPLY>
__global__ void __launch_bounds__(kHsThreads) hindsight_tile_kernel(
    const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, const v2u* __restrict__ events, int64_t n,
    uint32_t P, double tau2, double* __restrict__ carry, HsEdge* __restrict__ edges,
    const HsEdge* __restrict__ seeds, v2u* __restrict__ out) {
  __shared__ HsScan::Lds lds;
  const int t = threadIdx.x;
  const int64_t tile = blockIdx.x;
  const int64_t lo = tile * kHindsightTile;
  const int64_t hi = lo + kHindsightTile < n ? lo + kHindsightTile : n;
  const uint32_t head = keys[lo], tailkey = keys[hi - 1];
  if (head >= P) {  // sorted: nothing but slots that are no elements from here on
    if (!APPLY && t < 2) edges[2 * tile + t].key = kNoKey;
    return;
  }
  HsScan::init(lds);
  for (int it = 0; it < kHsIters; ++it) {
    const int64_t i = lo + (int64_t)it * kHsThreads + t;
    if (lo + (int64_t)it * kHsThreads >= hi) break;  // uniform over the workgroup
    const bool valid = i < hi;
    const uint32_t key = valid ? keys[i] : kNoKey;
    const bool first = !(valid && i > lo && keys[i - 1] == key);  // of its key in this tile
    const bool last = valid && (i + 1 == hi || keys[i + 1] != key);
    const bool edge_run = key == head || key == tailkey;
    const uint32_t slot = valid ? vals[i] : 0u;
    const bool has = valid && key < P && (int64_t)slot < n;  // slot < n always: a permutation
    HsMap s = hs_identity();
    if (has) {
      const v2u e = events[slot];
      const float mu = __uint_as_float(e[0]), sigma = __uint_as_float(e[1]);
      if (!first) {
        s = hs_element(mu, sigma, tau2);
      } else if (APPLY) {
        const HsMap seed = key == head      ? state_load(&seeds[2 * tile].s)
                           : key == tailkey ? state_load(&seeds[2 * tile + 1].s)
                                            : carry_seed(carry, key);
        s = hs_seeded(mu, sigma, tau2, seed);
      } else {
        // The key's newest element in the window, unless its run began in the tile before.
        // With a NaN carry row nothing lies behind it: it is the chain's newest, a constant.
        // A row that is set is applied by stitch or apply, not here.
        const bool newest = i == 0 || keys[i - 1] != key;
        const double behind = carry[(int64_t)key * 2];
        s = newest && behind != behind ? hs_newest(mu, sigma) : hs_element(mu, sigma, tau2);
      }
    }
    HsScan::step(lds, it, key, s);  // the element and everything newer of its key in the tile
    if (APPLY) {
      if (has) {
        v2u x;
        x[0] = __float_as_uint((float)s.A);
        x[1] = __float_as_uint((float)sqrt(s.C));
        out[slot] = x;
        if (last && !edge_run) carry_store(carry, key, s);
      }
    } else if (valid && (i + 1 == hi || (last && key == head))) {
      // the last element of the first key, and the tile's last element
      if (key == head) {
        edge_store(edges, 2 * tile, key, s);
        if (i + 1 == hi) edge_store(edges, 2 * tile + 1, key, hs_identity());
      } else {
        edge_store(edges, 2 * tile + 1, has ? key : kNoKey, s);
      }
    }
  }
}

// one workgroup over the edges [E] in tile order
__global__ void __launch_bounds__(kHsThreads) hindsight_stitch_kernel(const HsEdge* __restrict__ edges, int64_t E,
                                                                      uint32_t P, double* __restrict__ carry,
                                                                      HsEdge* __restrict__ seeds) {
  __shared__ HsScan::Lds lds;
  const int t = threadIdx.x;
  HsScan::init(lds);
  const int iters = (int)((E + kHsThreads - 1) / kHsThreads);
  for (int it = 0; it < iters; ++it) {
    const int64_t e = (int64_t)it * kHsThreads + t;
    const uint32_t key = e < E ? edges[e].key : kNoKey;
    const bool has = key < P;
    const bool first = !(e > 0 && e < E && edges[e - 1].key == key);
    const bool last = !(e + 1 < E && edges[e + 1].key == key);
    HsMap s = hs_identity();
    if (has) s = first ? carry_seed(carry, key) : state_load(&edges[e - 1].s);
    HsScan::step(lds, it, key, s);  // what lies behind edge e's stretch
    if (has) {
      state_store(&seeds[e].s, s);
      // a run always ends in a constant: its newest element, or the carry row behind it
      if (last) carry_store(carry, key, hs_scan_combine(s, state_load(&edges[e].s)));
    }
  }
}

}  // namespace

static int64_t hindsight_tiles(int64_t n) { return (n + kHindsightTile - 1) / kHindsightTile; }
// edges and seeds, 2 * tiles entries each
size_t hindsight_edge_bytes(int64_t n) { return (size_t)(2 * 2 * hindsight_tiles(n)) * sizeof(HsEdge); }

int launch_hindsight_keys(int K, const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t P, int track,
                          int mode, uint32_t* keys, uint32_t* vals, uint32_t* events, float* out, int32_t* bad,
                          hipStream_t s) {
  if (!window_slots_ok(K, W, M, P) || (track != kHsShared && track != kHsMode) ||
      (track == kHsMode && (mode < 0 || mode >= kModes)) || bad == nullptr ||
      reinterpret_cast<uintptr_t>(events) % 8 != 0 || reinterpret_cast<uintptr_t>(out) % 8 != 0)
    return (int)hipErrorInvalidValue;
  if (M == 0) return 0;
  const unsigned blocks = (unsigned)((M + kHsThreads - 1) / kHsThreads);
  with_team_size(K, [&](auto k) {
    hipLaunchKernelGGL(hindsight_keys_kernel<decltype(k)::value>, dim3(blocks), dim3(kHsThreads), 0, s, rec,
                       reinterpret_cast<const uint32_t*>(rows), W, M, P, (int32_t)track, (int32_t)mode, keys, vals,
                       reinterpret_cast<v2u*>(events), reinterpret_cast<v2u*>(out), bad);
  });
  return (int)hipGetLastError();
}

int launch_hindsight_scan(const uint32_t* keys, const uint32_t* vals, const uint32_t* events, int64_t n, int K,
                          int64_t P, double tau2, double* carry, void* edges, float* out, hipStream_t s) {
  if (!sorted_slots_ok(K, n, P) || !(tau2 >= 0.0) || !isfinite(tau2) || reinterpret_cast<uintptr_t>(events) % 8 != 0 ||
      reinterpret_cast<uintptr_t>(out) % 8 != 0 || reinterpret_cast<uintptr_t>(edges) % 8 != 0)
    return (int)hipErrorInvalidValue;
  if (n == 0 || P == 0) return 0;
  const int64_t tiles = hindsight_tiles(n);
  HsEdge* e = static_cast<HsEdge*>(edges);
  HsEdge* seeds = e + 2 * tiles;
  const v2u* ev = reinterpret_cast<const v2u*>(events);
  v2u* o = reinterpret_cast<v2u*>(out);
  hipLaunchKernelGGL(hindsight_tile_kernel<false>, dim3((unsigned)tiles), dim3(kHsThreads), 0, s, keys, vals, ev, n,
                     (uint32_t)P, tau2, carry, e, seeds, o);
  hipLaunchKernelGGL(hindsight_stitch_kernel, dim3(1), dim3(kHsThreads), 0, s, e, 2 * tiles, (uint32_t)P, carry,
                     seeds);
  hipLaunchKernelGGL(hindsight_tile_kernel<true>, dim3((unsigned)tiles), dim3(kHsThreads), 0, s, keys, vals, ev, n,
                     (uint32_t)P, tau2, carry, e, seeds, o);
  return (int)hipGetLastError();
}

}  // namespace ana
