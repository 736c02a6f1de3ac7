// K15 pairs: who plays with and against whom.  One window of the match stream rec [M][2K+2]
// joined with its packed output rows [M][W] becomes the pair table of pair_core.h: the distinct
// (a, b) in ascending order of a << 32 | b, each with [with_games, with_wins, vs_games, vs_wins].
// The same sort and reduce compact several tables into one.  Every step is stream-ordered and
// only reads rec and rows; the counters are integer sums, so the result is the same bits for
// any grid, tile size or order of the additions.
//
//   keys    one lane per entry i = m * E_K + q (E_K = 2K(2K - 1)), so the output streams are
//           coalesced; the record words of a match are shared by E_K consecutive lanes and
//           come from cache, and the row's status word is the only row word read, and only
//           for an entry whose slots and filter bit allow it.  Writes ka[i] (a, or P for a
//           dead entry, which therefore sorts last), the sort key kb[i] = b, the same b into
//           an array that survives the sort, and vals[i] = i | flags.  Under a player filter
//           nearly every entry is dead and would only be carried through six sort passes, so
//           there the kernel writes the live entries alone, packed from 0: a wave reserves its
//           places with one atomicAdd on a counter the host then reads.  The places come out
//           in any order, which the sort and the integer sums make invisible.
//   split   the compaction's keys: ka / kb / b from the int64 keys of the concatenated
//           tables, vals[i] = i.
//   sort    two runs of launch_radix_sort_pairs: on b, then -- after gather has fetched
//           ka[vals[i] & mask] into the order of the first run -- on a.  Stable, so the
//           result is ordered by (a, b).  A second gather lays b out in the sorted order.
//   count   one workgroup per tile of kPairTile sorted entries: the run heads of the tile.
//           A head is a live entry whose a OR b differs from its predecessor's.
//   scan    launch_tile_offsets: exclusive scan of the tile counts, the total U last; the host
//           reads U once to size the table.
//   emit    the same tile walk.  A head writes its row's key.  The counters of an entry are
//           decoded from its value's flags (a window) or loaded as the 16-B row at its
//           value's index (compaction), summed over the run inside the wave by a segmented
//           shuffle scan, and leave the wave once per run: a run that begins and ends inside
//           one wave is one 16-B store, a run cut by a wave or tile edge is finished by
//           integer atomicAdd onto the zeroed counters (no edge + stitch pass: integer sums
//           do not depend on the order).  Tiles whose first key is dead return at once.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "common.h"
#include "kernels.h"
#include "pair_core.h"
#include "record_dev.h"
#include "scan_dev.h"
#include "select_core.h"

namespace ana {

namespace {

constexpr int kPairThreads = 256;
constexpr int kPairIters = kPairTile / kPairThreads;
static_assert(kPairTile % kPairThreads == 0, "a tile is a whole number of iterations");

// kCompact: only the live entries are written, packed from 0 in any order (``live`` counts them)
template <int K, bool kCompact>
__global__ void __launch_bounds__(kPairThreads) pair_keys_kernel(
    const int32_t* __restrict__ rec, const uint32_t* __restrict__ rows, int64_t W, int64_t n, int64_t P,
    uint32_t modes, const uint32_t* __restrict__ bitmap, uint32_t* __restrict__ ka, uint32_t* __restrict__ kb,
    uint32_t* __restrict__ bkeep, uint32_t* __restrict__ vals, uint32_t* __restrict__ live_count) {
  constexpr int S = 2 * K, E = pair_entries(K);
  const int64_t i = (int64_t)blockIdx.x * kPairThreads + threadIdx.x;
  bool live = i < n;
  int32_t a = 0, b = 0;
  uint32_t flags = 0u;
  if (live) {
    const int64_t m = i / E;
    const int q = (int)(i - m * E);
    int ja, jb;
    pair_slots<K>(q, ja, jb);
    const int32_t* r = rec + m * (S + 2);
    const uint32_t m0 = (uint32_t)r[S];
    a = r[ja];
    b = r[jb];
    flags = pair_flags<K>((uint32_t)r[S + 1], ja, jb);
    live = pair_mode_selected(m0, modes) && pair_slot_live<K>(m0, ja, a, P) && pair_slot_live<K>(m0, jb, b, P) &&
           a != b;
    if (live) live = pair_filtered(bitmap, a);  // behind the range check
    if (live) live = select_row_status<K>(rows + m * W) == kRated;
  }
  if constexpr (kCompact) {
    // one atomicAdd per wave reserves its live entries' places; the order of the places does not
    // matter: the sort orders the entries and the reduce adds integers
    const unsigned long long bal = __ballot(live);
    if (bal == 0ull) return;  // uniform over the wave
    const int lane = threadIdx.x & 63, first = __ffsll((long long)bal) - 1;
    uint32_t base = 0u;
    if (lane == first) base = atomicAdd(live_count, (uint32_t)__popcll(bal));
    base = __shfl(base, first, 64);
    const int64_t pos = (int64_t)base + __popcll(bal & ((1ull << lane) - 1ull));
    if (live && pos < n) {  // always: at most n entries are live
      ka[pos] = (uint32_t)a;
      kb[pos] = (uint32_t)b;
      bkeep[pos] = (uint32_t)b;
      vals[pos] = (uint32_t)pos | flags;
    }
  } else {
    if (i >= n) return;
    ka[i] = live ? (uint32_t)a : (uint32_t)P;
    const uint32_t bb = live ? (uint32_t)b : 0u;
    kb[i] = bb;
    bkeep[i] = bb;
    vals[i] = (uint32_t)i | flags;
  }
}

__global__ void __launch_bounds__(kPairThreads) pair_split_kernel(const int64_t* __restrict__ keys, int64_t n,
                                                                  uint32_t* __restrict__ ka, uint32_t* __restrict__ kb,
                                                                  uint32_t* __restrict__ bkeep,
                                                                  uint32_t* __restrict__ vals) {
  const int64_t i = (int64_t)blockIdx.x * kPairThreads + threadIdx.x;
  if (i >= n) return;
  const uint64_t k = (uint64_t)keys[i];
  const uint32_t b = (uint32_t)(k & 0xffffffffull);
  ka[i] = (uint32_t)(k >> 32);
  kb[i] = b;
  bkeep[i] = b;
  vals[i] = (uint32_t)i;
}

// out[i] = src[vals[i] & mask]
__global__ void __launch_bounds__(kPairThreads) pair_gather_kernel(const uint32_t* __restrict__ src,
                                                                   const uint32_t* __restrict__ vals, uint32_t mask,
                                                                   int64_t n, uint32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kPairThreads + threadIdx.x;
  if (i >= n) return;
  const uint32_t v = vals[i] & mask;
  out[i] = (int64_t)v < n ? src[v] : 0u;  // always: the values index the n entries
}

// live entry i of the sorted (a, b) begins a run; a_i = a[i] < dead
__device__ __forceinline__ bool pair_head(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, int64_t i,
                                          uint32_t a_i, uint32_t b_i) {
  return i == 0 || a[i - 1] != a_i || b[i - 1] != b_i;
}

__global__ void __launch_bounds__(kPairThreads) pair_count_kernel(const uint32_t* __restrict__ a,
                                                                  const uint32_t* __restrict__ b, int64_t n,
                                                                  uint32_t dead, uint32_t* __restrict__ counts) {
  const int t = threadIdx.x;
  const int64_t lo = (int64_t)blockIdx.x * kPairTile;
  uint32_t heads = 0u;
  if (a[lo] < dead) {  // sorted: else nothing but dead entries from here on (uniform)
#pragma unroll
    for (int it = 0; it < kPairIters; ++it) {
      const int64_t i = lo + (int64_t)it * kPairThreads + t;
      if (i >= n) continue;
      const uint32_t a_i = a[i];
      if (a_i < dead && pair_head(a, b, i, a_i, b[i])) ++heads;
    }
  }
  block_sum_store<kPairThreads>(heads, counts + blockIdx.x);
}

// kGather: the counters of an entry are the row src[value] (compaction), else its value's flags
template <bool kGather>
__global__ void __launch_bounds__(kPairThreads) pair_emit_kernel(
    const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, const uint32_t* __restrict__ vals, int64_t n,
    uint32_t dead, const v4i* __restrict__ src, const int64_t* __restrict__ offsets, int64_t U,
    int64_t* __restrict__ keys, int32_t* __restrict__ counts) {
  const int t = threadIdx.x, lane = t & 63;
  const int64_t lo = (int64_t)blockIdx.x * kPairTile;
  if (a[lo] >= dead) return;  // uniform over the workgroup
  int64_t run = offsets[blockIdx.x];  // run heads before this tile
  for (int it = 0; it < kPairIters; ++it) {
    const int64_t i0 = lo + (int64_t)it * kPairThreads;
    if (i0 >= n) break;  // uniform over the workgroup
    const int64_t i = i0 + t;
    const uint32_t a_i = i < n ? a[i] : dead;
    const bool valid = a_i < dead;  // a prefix of the lanes: dead entries sort last
    const uint32_t b_i = valid ? b[i] : 0u;
    const bool head = valid && pair_head(a, b, i, a_i, b_i);
    const unsigned long long bal = __ballot(head);
    const int incl = __popcll(bal & (~0ull >> (63 - lane)));  // heads of this wave up to this lane
    int total;
    const int before = block_offset<kPairThreads>(it, incl, total);
    const int64_t row = run + before + incl - 1;  // a run without a head here goes on from an earlier wave or tile
    run += total;
    int32_t c[kPairWords] = {0, 0, 0, 0};
    if (valid) {
      const uint32_t v = vals[i];
      if constexpr (kGather) {
        if ((int64_t)v < n) {  // always: the values are a permutation of the rows
          const v4i x = src[v];
#pragma unroll
          for (int d = 0; d < kPairWords; ++d) c[d] = x[d];
        }
      } else {
        pair_counters(v, c);
      }
    }
    // segmented inclusive sum inside the wave: the live lanes of one run share ``incl``
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int oi = __shfl_up(incl, o, 64);
      int32_t oc[kPairWords];
#pragma unroll
      for (int d = 0; d < kPairWords; ++d) oc[d] = __shfl_up(c[d], o, 64);
      if (lane >= o && oi == incl) {
#pragma unroll
        for (int d = 0; d < kPairWords; ++d) c[d] += oc[d];
      }
    }
    if (!valid || row < 0 || row >= U) continue;  // (a live entry always has a row: the counts come from the same walk)
    if (head) keys[row] = pair_key(a_i, b_i);
    const bool ends = i + 1 >= n || a[i + 1] != a_i || b[i + 1] != b_i;  // a dead successor differs in a
    if (!ends && lane != 63) continue;  // the run goes on inside this wave
    int32_t* dst = counts + row * kPairWords;
    if (ends && incl >= 1) {  // the whole run lies in this wave: its only writer
      v4i x;
#pragma unroll
      for (int d = 0; d < kPairWords; ++d) x[d] = c[d];
      *reinterpret_cast<v4i*>(dst) = x;
    } else {
#pragma unroll
      for (int d = 0; d < kPairWords; ++d)
        if (c[d]) atomicAdd(dst + d, c[d]);
    }
  }
}

bool aligned(const void* p, uintptr_t to) { return p != nullptr && reinterpret_cast<uintptr_t>(p) % to == 0; }

unsigned blocks_of(int64_t n) { return (unsigned)((n + kPairThreads - 1) / kPairThreads); }

}  // namespace

int64_t pair_tiles(int64_t n) { return (n + kPairTile - 1) / kPairTile; }

int launch_pair_keys(int K, const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t P, uint32_t modes,
                     const uint32_t* bitmap, uint32_t* ka, uint32_t* kb, uint32_t* bkeep, uint32_t* vals,
                     uint32_t* live_count, hipStream_t s) {
  if (!window_ok(K, W, M, P) || M > kMaxSlots / pair_entries(K) || (modes & ~kPairAllModes))
    return (int)hipErrorInvalidValue;
  if (M == 0) return 0;
  if (!aligned(rec, 4) || !aligned(rows, 4) || !aligned(ka, 4) || !aligned(kb, 4) || !aligned(bkeep, 4) ||
      !aligned(vals, 4) || (bitmap != nullptr && !aligned(bitmap, 4)) ||
      (live_count != nullptr && !aligned(live_count, 4)))
    return (int)hipErrorInvalidValue;
  const int64_t n = M * pair_entries(K);
  const uint32_t* rw = reinterpret_cast<const uint32_t*>(rows);
  with_team_size(K, [&](auto k) {
    constexpr int kK = decltype(k)::value;
    if (live_count != nullptr)
      hipLaunchKernelGGL((pair_keys_kernel<kK, true>), dim3(blocks_of(n)), dim3(kPairThreads), 0, s, rec, rw, W, n, P,
                         modes, bitmap, ka, kb, bkeep, vals, live_count);
    else
      hipLaunchKernelGGL((pair_keys_kernel<kK, false>), dim3(blocks_of(n)), dim3(kPairThreads), 0, s, rec, rw, W, n, P,
                         modes, bitmap, ka, kb, bkeep, vals, live_count);
  });
  return (int)hipGetLastError();
}

int launch_pair_split(const int64_t* keys, int64_t n, uint32_t* ka, uint32_t* kb, uint32_t* bkeep, uint32_t* vals,
                      hipStream_t s) {
  if (n < 0 || n > 0x7fffffffll) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  if (!aligned(keys, 8) || !aligned(ka, 4) || !aligned(kb, 4) || !aligned(bkeep, 4) || !aligned(vals, 4))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(pair_split_kernel, dim3(blocks_of(n)), dim3(kPairThreads), 0, s, keys, n, ka, kb, bkeep, vals);
  return (int)hipGetLastError();
}

int launch_pair_gather(const uint32_t* src, const uint32_t* vals, uint32_t mask, int64_t n, uint32_t* out,
                       hipStream_t s) {
  if (n < 0 || n > 0x7fffffffll) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  if (!aligned(src, 4) || !aligned(vals, 4) || !aligned(out, 4) || src == out) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(pair_gather_kernel, dim3(blocks_of(n)), dim3(kPairThreads), 0, s, src, vals, mask, n, out);
  return (int)hipGetLastError();
}

int launch_pair_count(const uint32_t* a, const uint32_t* b, int64_t n, uint32_t dead, uint32_t* counts,
                      int64_t* offsets, hipStream_t s) {
  if (n < 0 || n > 0x7fffffffll) return (int)hipErrorInvalidValue;
  if (!aligned(offsets, 8) || (n > 0 && (!aligned(a, 4) || !aligned(b, 4) || !aligned(counts, 4))))
    return (int)hipErrorInvalidValue;
  const int64_t tiles = pair_tiles(n);
  if (tiles > 0)
    hipLaunchKernelGGL(pair_count_kernel, dim3((unsigned)tiles), dim3(kPairThreads), 0, s, a, b, n, dead, counts);
  return launch_tile_offsets(counts, tiles, offsets, s);
}

int launch_pair_emit(const uint32_t* a, const uint32_t* b, const uint32_t* vals, int64_t n, uint32_t dead,
                     const int32_t* src, const int64_t* offsets, int64_t U, int64_t* keys, int32_t* counts,
                     hipStream_t s) {
  if (n < 0 || n > 0x7fffffffll || U < 0 || U > n || (src == nullptr && n > kMaxSlots))
    return (int)hipErrorInvalidValue;
  if (n == 0 || U == 0) return 0;
  if (!aligned(a, 4) || !aligned(b, 4) || !aligned(vals, 4) || !aligned(offsets, 8) || !aligned(keys, 8) ||
      !aligned(counts, 16) || (src != nullptr && !aligned(src, 16)))
    return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)pair_tiles(n)), block(kPairThreads);
  if (src != nullptr)
    hipLaunchKernelGGL(pair_emit_kernel<true>, grid, block, 0, s, a, b, vals, n, dead,
                       reinterpret_cast<const v4i*>(src), offsets, U, keys, counts);
  else
    hipLaunchKernelGGL(pair_emit_kernel<false>, grid, block, 0, s, a, b, vals, n, dead,
                       static_cast<const v4i*>(nullptr), offsets, U, keys, counts);
  return (int)hipGetLastError();
}

}  // namespace ana
