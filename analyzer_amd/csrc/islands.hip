// K18 islands: the connected components of the match graph as a concurrent union-find over the
// roster table (island_core.h has the state, the invariants and why the result is order-free).
//
//   hook     one lane per match: the record and, for a match with a live slot, the row's status
//            word.  A rated match adds 1 to slots[p] of every live slot and 1 to credit of the
//            first live slot's player, and unites every further live slot's player with it.
//            The lanes of a wave that count the same player in the same slot add once together.
//   edges    the same unions for an explicit edge list, one lane per edge: a self loop unites
//            nothing, an endpoint outside [0, P) drops the edge and counts it in ctrl[1]; with
//            ``mark`` both endpoints get kIslandSeenBit.
//   flatten  a later launch: parent[i] = root(i) for every player.
//   census   over flattened parents: players, matches (credit) and player_games (slots) of every
//            seen player added to its root's words of census [3][P] int64.  A wave first sums the
//            lanes that share a root (the giant island, regions dealt over consecutive ids) for
//            up to kCensusRounds roots, so those add once per wave.
//
// find follows parent to a root and halves the path on the way (parent[x] = min(parent[x],
// grandparent)); a hook is a compare-and-swap on the larger root's own word, and a failed one
// goes on from the value it returned.  parent is read with relaxed agent-scope loads and written
// with agent-scope atomics only, inside every kernel here: the per-XCD L2s are not coherent and a
// CU's L1 is never refreshed by another CU's stores, and an older value of a word is harmless
// where a torn or L1-cached one would not be.  Nothing spins: both loops are capped at P and set
// ctrl[0] when they hit the cap or read a word above its own index.  Counters are integer atomics.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "common.h"
#include "island_core.h"
#include "kernels.h"
#include "record_dev.h"
#include "select_core.h"

namespace ana {

namespace {

constexpr int kIslandThreads = 256;
constexpr int kCensusRounds = 8;  // groups of one root that a wave of the census sums before it adds lane by lane

// Experiment builds only (python -m analyzer_amd.build_ext --variant NAME --define ANA_ISLAND_HOOK_PART=1 or 2;
// scripts/islands_bench.py --timing-only): the hook with its counters alone (1) or its unions alone (2), which
// is how the split of its time was measured.  Such a library computes no islands.
#ifndef ANA_ISLAND_HOOK_PART
#define ANA_ISLAND_HOOK_PART 0
#endif
constexpr bool kHookCounts = ANA_ISLAND_HOOK_PART != 2, kHookUnites = ANA_ISLAND_HOOK_PART != 1;

__device__ __forceinline__ int32_t island_load(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void island_fail(int64_t* ctrl, int64_t bits) {
  atomicOr(reinterpret_cast<unsigned long long*>(ctrl), (unsigned long long)bits);
}

// the root of x as this lane sees it; ok = false after an error (the walk stopped where it was)
__device__ __forceinline__ int32_t island_find(int32_t* parent, int32_t x, int64_t cap, int64_t* ctrl, bool& ok) {
  int64_t why = kIslandErrSteps;  // more than P steps, which strictly decreasing words cannot take
  for (int64_t step = 0; step <= cap; ++step) {
    const int32_t p = island_load(parent + x);
    if (p == x) return x;
    const bool p_ok = island_word_ok(p, x);
    const int32_t g = p_ok ? island_load(parent + p) : 0;
    if (p_ok && g == p) return p;
    if (!p_ok || !island_word_ok(g, p)) {  // a word outside [0, its index]: it is not followed
      why = kIslandErrParent;
      break;
    }
    __hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // g < p <= the word
    x = g;
  }
  island_fail(ctrl, why);
  ok = false;
  return x;
}

// unites the islands of a and b; returns a player of the united island near its root
__device__ __forceinline__ int32_t island_unite(int32_t* parent, int32_t a, int32_t b, int64_t cap, int64_t* ctrl) {
  bool ok = true;
  for (int64_t round = 0; round <= cap; ++round) {
    a = island_find(parent, a, cap, ctrl, ok);
    if (!ok) return a;
    b = island_find(parent, b, cap, ctrl, ok);
    if (!ok) return a;
    if (a == b) return a;
    const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
    const int32_t old = atomicCAS(parent + hi, hi, lo);  // device scope, on hi's own word
    if (old == hi) return lo;
    if (!island_word_ok(old, hi)) {
      island_fail(ctrl, kIslandErrParent);
      return lo;
    }
    a = old;  // hi was hooked meanwhile: old < hi is of its island
    b = lo;
  }
  island_fail(ctrl, kIslandErrSteps);  // max(a, b) fell every round: more than P rounds cannot be
  return a;
}

// counter[p] += 1 for every lane with ``active``, called by the whole wave: the lanes that share
// the first active lane's p add once together, so a player who stands in one slot of every match
// costs one atomic per wave there, not 64 on one address
__device__ __forceinline__ void island_count(int32_t* counter, int32_t p, bool active) {
  const unsigned long long bal = __ballot(active);
  if (bal == 0ull) return;  // uniform over the wave
  const int lane = threadIdx.x & 63, leader = __ffsll((long long)bal) - 1;
  const int32_t p0 = __shfl(p, leader, 64);
  const bool shared = active && p == p0;
  const int n = __popcll(__ballot(shared));
  if (lane == leader) atomicAdd(counter + p0, n);
  else if (active && !shared) atomicAdd(counter + p, 1);
}

template <int K>
__global__ void __launch_bounds__(kIslandThreads) island_hook_kernel(
    const int32_t* __restrict__ rec, const uint32_t* __restrict__ rows, int64_t W, int64_t M, int64_t P,
    uint32_t modes, int32_t* parent, int32_t* slots, int32_t* credit, int64_t* ctrl) {
  constexpr int S = 2 * K;
  const int64_t m = (int64_t)blockIdx.x * kIslandThreads + threadIdx.x;
  int32_t r[S + 2];
  uint32_t live = 0u;  // no lane leaves before the counting: it is wave-wide
  if (m < M) {
    load_record<K>(rec, m, r);
    live = island_live_mask<K>(r, P, modes);
    if (live != 0u && select_row_status<K>(rows + m * W) != kRated) live = 0u;
  }
  int32_t first = 0;  // the first live slot's player
#pragma unroll
  for (int j = S - 1; j >= 0; --j) {
    const bool on = (live >> j) & 1u;
    const int32_t p = on ? r[j] : 0;  // in [0, P): the slot is live
    if constexpr (kHookCounts) island_count(slots, p, on);
    if (on) first = p;
  }
  if constexpr (kHookCounts) island_count(credit, first, live != 0u);
  if (live == 0u || !kHookUnites) return;
  int32_t at = first;  // where the island is held by now
#pragma unroll
  for (int j = 0; j < S; ++j) {
    if (!((live >> j) & 1u) || r[j] == first) continue;
    at = island_unite(parent, at, r[j], P, ctrl);
  }
}

__global__ void __launch_bounds__(kIslandThreads) island_edges_kernel(
    const int32_t* __restrict__ ea, const int32_t* __restrict__ eb, int64_t n, int64_t P, int mark, int32_t* parent,
    int32_t* slots, int64_t* ctrl) {
  const int64_t i = (int64_t)blockIdx.x * kIslandThreads + threadIdx.x;
  if (i >= n) return;
  const int32_t a = ea[i], b = eb[i];
  if (a < 0 || (int64_t)a >= P || b < 0 || (int64_t)b >= P) {
    atomicAdd(reinterpret_cast<unsigned long long*>(ctrl + 1), 1ull);
    return;
  }
  if (mark) {
    atomicOr(reinterpret_cast<uint32_t*>(slots + a), kIslandSeenBit);
    if (b != a) atomicOr(reinterpret_cast<uint32_t*>(slots + b), kIslandSeenBit);
  }
  if (a != b) island_unite(parent, a, b, P, ctrl);
}

__global__ void __launch_bounds__(kIslandThreads) island_flatten_kernel(int32_t* parent, int64_t P, int64_t* ctrl) {
  const int64_t i = (int64_t)blockIdx.x * kIslandThreads + threadIdx.x;
  if (i >= P) return;
  bool ok = true;
  const int32_t root = island_find(parent, (int32_t)i, P, ctrl, ok);
  if (ok) __hip_atomic_fetch_min(parent + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ void __launch_bounds__(kIslandThreads) island_census_kernel(
    const int32_t* __restrict__ parent, const int32_t* __restrict__ slots, const int32_t* __restrict__ credit,
    int64_t P, int64_t* census, int64_t* ctrl) {
  const int64_t i = (int64_t)blockIdx.x * kIslandThreads + threadIdx.x;  // no lane leaves before the shuffles
  const uint32_t sw = i < P ? (uint32_t)slots[i] : 0u;
  bool seen = sw != 0u;
  int32_t root = 0;
  if (seen) {
    root = parent[i];
    if (!island_word_ok(root, (int32_t)i)) {  // never with a table this file wrote
      island_fail(ctrl, kIslandErrParent);
      seen = false;
    }
  }
  long long games = seen ? (long long)(sw & kIslandSlotMask) : 0ll;
  long long matches = seen ? (long long)credit[i] : 0ll;
  long long players = seen ? 1ll : 0ll;
  // up to kCensusRounds times the lanes that share the first pending lane's root add up inside the
  // wave and leave as one: the giant island, or a few islands dealt over consecutive ids (regions),
  // cost a few atomics per wave instead of 64 on a handful of addresses.  What is still pending
  // after the rounds adds lane by lane.
  const int lane = threadIdx.x & 63;
  bool pending = seen, holds = false;  // not summed into a leader yet; a leader with its group's sums
#pragma unroll 1
  for (int round = 0; round < kCensusRounds; ++round) {
    const unsigned long long bal = __ballot(pending);
    if (bal == 0ull) break;  // uniform over the wave
    const int leader = __ffsll((long long)bal) - 1;
    const bool mine = pending && root == __shfl(root, leader, 64);
    const long long p = wave_sum(mine ? players : 0ll), m = wave_sum(mine ? matches : 0ll),
                    g = wave_sum(mine ? games : 0ll);
    if (lane == leader) {
      players = p;
      matches = m;
      games = g;
      holds = true;
    }
    if (mine) pending = false;
  }
  if (!holds && !pending) return;
  unsigned long long* out = reinterpret_cast<unsigned long long*>(census) + root;
  atomicAdd(out, (unsigned long long)players);
  if (matches) atomicAdd(out + P, (unsigned long long)matches);
  if (games) atomicAdd(out + 2 * P, (unsigned long long)games);
}

bool aligned(const void* p, uintptr_t to) { return p != nullptr && reinterpret_cast<uintptr_t>(p) % to == 0; }

unsigned blocks_of(int64_t n) { return (unsigned)((n + kIslandThreads - 1) / kIslandThreads); }

}  // namespace

int launch_island_hook(int K, const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t P, uint32_t modes,
                       int32_t* parent, int32_t* slots, int32_t* credit, int64_t* ctrl, hipStream_t s) {
  if (!window_slots_ok(K, W, M, P) || (modes & ~kIslandAllModes)) return (int)hipErrorInvalidValue;
  if (M == 0 || P == 0) return 0;
  if (!aligned(rec, K % 2 == 0 ? 8 : 16) || !aligned(rows, 4) || !aligned(parent, 4) || !aligned(slots, 4) ||
      !aligned(credit, 4) || !aligned(ctrl, 8))
    return (int)hipErrorInvalidValue;
  const uint32_t* rw = reinterpret_cast<const uint32_t*>(rows);
  with_team_size(K, [&](auto k) {
    hipLaunchKernelGGL((island_hook_kernel<decltype(k)::value>), dim3(blocks_of(M)), dim3(kIslandThreads), 0, s, rec,
                       rw, W, M, P, modes, parent, slots, credit, ctrl);
  });
  return (int)hipGetLastError();
}

int launch_island_edges(const int32_t* a, const int32_t* b, int64_t n, int64_t P, int mark, int32_t* parent,
                        int32_t* slots, int64_t* ctrl, hipStream_t s) {
  if (n < 0 || n > 0x7fffffffll * kIslandThreads || P < 0 || P > 0x7fffffffll) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  if (!aligned(a, 4) || !aligned(b, 4) || !aligned(ctrl, 8) || (P > 0 && (!aligned(parent, 4) || !aligned(slots, 4))))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(island_edges_kernel, dim3(blocks_of(n)), dim3(kIslandThreads), 0, s, a, b, n, P, mark, parent,
                     slots, ctrl);
  return (int)hipGetLastError();
}

int launch_island_flatten(int32_t* parent, int64_t P, int64_t* ctrl, hipStream_t s) {
  if (P < 0 || P > 0x7fffffffll) return (int)hipErrorInvalidValue;
  if (P == 0) return 0;
  if (!aligned(parent, 4) || !aligned(ctrl, 8)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(island_flatten_kernel, dim3(blocks_of(P)), dim3(kIslandThreads), 0, s, parent, P, ctrl);
  return (int)hipGetLastError();
}

int launch_island_census(const int32_t* parent, const int32_t* slots, const int32_t* credit, int64_t P,
                         int64_t* census, int64_t* ctrl, hipStream_t s) {
  if (P < 0 || P > 0x7fffffffll) return (int)hipErrorInvalidValue;
  if (P == 0) return 0;
  if (!aligned(parent, 4) || !aligned(slots, 4) || !aligned(credit, 4) || !aligned(census, 8) || !aligned(ctrl, 8))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(island_census_kernel, dim3(blocks_of(P)), dim3(kIslandThreads), 0, s, parent, slots, credit, P,
                     census, ctrl);
  return (int)hipGetLastError();
}

}  // namespace ana
