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
//   summaries  one workgroup per tile of kHindsightTile sorted elements: the inclusive scan of
//              the elements' maps.  The newest element of a player in the window whose carry
//              row is NaN is the chain's newest, a constant; every other element is its map.
//              The totals of the tile's first and last key (without anything behind them) go
//              to edges[2 * tile + 0 / 1].
//   stitch     one workgroup over the 2 * tiles edges, seeded from the carry rows (the identity
//              for a NaN row): seeds[e] is what lies behind edge e's stretch; a key's last
//              edge stores its new carry row.
//   apply      the summaries scan again, seeded from seeds or, for a run strictly inside the
//              tile, from the carry row, which the run's last (oldest) element stores.  Every
//              element stores its 8-B (mh, sqrt(Ph)) as fp32 at out[slot], slot-major
//              [M][2K][2], which is the public layout.
//
// The last three are the chained scan of chain_dev.h over HsChain below; its header argues why
// the carry rows are updated in place without a race (its "first" is a player's newest element,
// its "last" the oldest).  That a seed is "nothing" survives in seeds as the identity (B == 1).
//
// Built with -ffp-contract=off: every fp64 operation is the one written.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "chain_dev.h"
#include "common.h"
#include "hindsight_core.h"
#include "kernels.h"
#include "record_dev.h"

namespace ana {

namespace {

constexpr int kHsThreads = 256;

typedef unsigned int v2u __attribute__((ext_vector_type(2)));

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

// The feature of the chained scan (chain_dev.h), newest first: a lane's scanned state is the
// composition of the maps of its key from its element to the newest, behind it the seed.  A run
// ends in a constant, so its total is the smoothed (mh, Ph) of its oldest element.
struct HsChain {
  typedef HsMap State;
  const v2u* __restrict__ events;
  int64_t n;
  double tau2;
  v2u* __restrict__ out;

  static __device__ __forceinline__ HsMap identity() { return hs_identity(); }
  static __device__ __forceinline__ HsMap combine(const HsMap& x, const HsMap& y) { return hs_scan_combine(x, y); }
  static __device__ __forceinline__ HsMap seed(const double* __restrict__ carry, uint32_t key) {
    return hs_seed_of_row(carry[(int64_t)key * 2], carry[(int64_t)key * 2 + 1]);
  }
  static __device__ __forceinline__ void row_store(double* __restrict__ carry, uint32_t key, const HsMap& s) {
    carry[(int64_t)key * 2] = s.A;
    carry[(int64_t)key * 2 + 1] = s.C;
  }

  // make(mu, sigma) of the filtered values of the element in slot
  template <class Make>
  __device__ __forceinline__ HsMap term(uint32_t slot, Make&& make) const {
    if ((int64_t)slot >= n) return hs_identity();  // slot < n always: a permutation
    const v2u e = events[slot];
    return make(__uint_as_float(e[0]), __uint_as_float(e[1]));
  }
  __device__ __forceinline__ HsMap next(uint32_t, uint32_t slot) const {
    return term(slot, [&](float mu, float sigma) { return hs_element(mu, sigma, tau2); });
  }
  __device__ __forceinline__ HsMap first(uint32_t slot, const HsMap& seed) const {
    return term(slot, [&](float mu, float sigma) { return hs_seeded(mu, sigma, tau2, seed); });
  }
  // With a NaN carry row nothing lies behind the key's newest element of the window: it is the
  // chain's newest, a constant.  A row that is set is applied by stitch or apply, not here.
  __device__ __forceinline__ HsMap open(uint32_t slot, uint32_t key, bool newest, const double* carry) const {
    const double behind = carry[(int64_t)key * 2];
    return term(slot, [&](float mu, float sigma) {
      return newest && behind != behind ? hs_newest(mu, sigma) : hs_element(mu, sigma, tau2);
    });
  }
  __device__ __forceinline__ HsMap total(uint32_t, const HsMap& s) const { return s; }
  __device__ __forceinline__ void emit(uint32_t slot, const HsMap& s) const {
    if ((int64_t)slot >= n) return;
    v2u x;
    x[0] = __float_as_uint((float)s.A);
    x[1] = __float_as_uint((float)sqrt(s.C));
    out[slot] = x;
  }
};
typedef ChainScan<HsChain, kHsThreads, kHindsightTile> HsScan;
typedef HsScan::Edge HsEdge;
static_assert(sizeof(HsEdge) == 32 && offsetof(HsEdge, s) == 8, "an edge or a seed: [key, -, map], four 8-B pieces");

template <bool APPLY>  // summaries (false) and apply (true)
__global__ void __launch_bounds__(kHsThreads) hindsight_tile_kernel(
    const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, const v2u* __restrict__ events, int64_t n,
    uint32_t P, double tau2, double* __restrict__ carry, HsEdge* __restrict__ edges,
    const HsEdge* __restrict__ seeds, v2u* __restrict__ out) {
  HsScan::tile<APPLY>(keys, vals, n, P, carry, edges, seeds, HsChain{events, n, tau2, out});
}

__global__ void __launch_bounds__(kHsThreads) hindsight_stitch_kernel(const HsEdge* __restrict__ edges, int64_t E,
                                                                      uint32_t P, double* __restrict__ carry,
                                                                      HsEdge* __restrict__ seeds) {
  HsScan::stitch(edges, E, P, carry, seeds);
}

}  // namespace

size_t hindsight_edge_bytes(int64_t n) { return HsScan::edge_bytes(n); }

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
  const int64_t tiles = HsScan::tiles(n);
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
