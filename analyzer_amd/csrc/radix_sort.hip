// K5 building block: stable LSD radix sort of (u32 key, u32 value) pairs for
// gfx950, written to CO-RUN with the persistent dataflow executor.
//
// hipCUB's onesweep sort chains its tiles through a decoupled look-back: tile
// t spins until tile t-1 has published its prefix.  Next to the rating
// kernel (which keeps the memory system busy with latency-bound sc1 traffic)
// every link of that chain waits microseconds and one 60M-slot pass stretches
// from 0.4 ms to 9.5 ms (rocprofv3 trace, profiles/).  This sort is
// reduce-then-scan instead: every pass is three launches whose workgroups
// never wait on each other --
//   upsweep   per-tile digit histograms (LDS atomics, one row per digit),
//   rowscan   one workgroup per digit: exclusive scan of its row over tiles,
//   downsweep per tile: stable rank in wave order (8 ballots -> peer mask),
//             wave prefixes in LDS, local scatter into an LDS-sorted tile,
//             then coalesced runs to the global digit offsets.
// 8192-element tiles (512 threads x 16) and 8-bit digits: the per-(tile, digit) runs the
// downsweeps write average 32 elements, whole 128-B lines.  Measured and not taken:
//   4096-element tiles (256 threads): 0.03-0.04 ms slower per 10M 3v3 prepass
//     (profiles/r3/sort_tile_8192.log);
//   10-bit digits for the schedule (two passes for <= 2^20 players): 3.11 against 1.76 ms per
//     prepass -- 1024 runs of ~4 elements per tile scatter the writes, 56 KB of LDS halve the
//     link pass's occupancy, the fix-up has four times the runs
//     (profiles/r3/prepass_rb8_vs_rb10.txt);
//   non-temporal stores: see ld32.
//
// The schedule prepass (launch_sched_sort) fuses both ends: pass 0 computes its
// keys from the match records, and the last pass writes each slot's link from
// its LDS neighbours instead of the sorted pairs (only run-boundary pairs go out,
// for the fix-up).  For 10M 3v3 matches that drops a 480-MB key/value write, the
// re-reads of it and a separate 720-MB link pass.  The fix-up of a last pass over at most
// 32 digits (1M players: bits 16..19) works from a [tile][digit] table of run ends, which
// needs no upsweep / rowscan in front of that pass (1.63 against 1.78 ms per prepass,
// profiles/r3/sched_run_table.log); a last pass over more digits (10M players) scatters
// its boundary pairs to their digit offsets for sched_fixup.
//
// Rosters of <= 2^20 players need only the first of those passes: one stable
// partition by the key bits above the low 12, then sched_chain -- one workgroup per bucket
// sorts its tiles in LDS and chains each player's slots through a last-occurrence table
// (4 launches and ~1.84 GB per 10M 3v3 window instead of 9 and ~3.0 GB; 1.22-1.25 ms alone
// against 1.60-1.64, the config 2 step 0.10-0.12 ms shorter, profiles/r7/sched_chain_ab.log).
// Larger rosters, and windows whose buckets would be long (launch_sched_sort), take the
// three LSD passes; ANA_SCHED_CHAIN=1 / 0 forces either, which is how small tests reach both.
//
// Beside the executor the links of the chain path leave as whole lines (a prepass with nothing
// beside it keeps the direct stores, see sched_sort_k).  Direct, sched_chain writes link[slot]:
// 60M random 4-B stores per window, one fabric write request each, beside an executor whose time
// is the latency of its own requests.  The whole-lines variant writes each link at the slot's
// position in its bucket, in place over the bucket's keys and one tile late through an LDS buffer,
// so that a link resolved by the next tile still leaves inside a coalesced run; 6.2 % of the links
// (deferred past the next tile, or to the final flush) remain single stores.  sched_unpartition, one
// workgroup per input tile, then reads the tile's 256 runs back through the partition's own
// offset table and writes link[] in slot order with 16-B stores.  5 launches and ~2.56 GB per
// window, but 10.3M write requests from the two kernels instead of 58.8M: alone the prepass is
// slower (1.54-1.57 against 1.22-1.26 ms), beside the executor the config 2 step is 0.27-0.37 ms
// shorter (profiles/r8/links_whole_lines_ab.log).
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "common.h"
#include "kernels.h"
#include "record_dev.h"

namespace ana {

namespace {

constexpr int kThreads = 512;  // threads per tile (x 16 items = 8192 elements)
constexpr int kWaves = kThreads / 64;
constexpr int kItems = 16;
constexpr int kTile = kThreads * kItems;
constexpr int kRadixBits = 8;
constexpr int kRadix = 1 << kRadixBits;  // digits per pass: at most one per thread in the scans
static_assert(kRadix <= kThreads, "one digit per thread");

// Tile of this workgroup.  Workgroups go round-robin over the 8 XCDs; giving
// each XCD a contiguous range of tiles puts the digit runs that consecutive
// tiles write next to each other into one L2, which merges them into full
// lines before they leave for HBM.
__device__ __forceinline__ int64_t xcd_tile(int64_t tiles) {
  const int64_t i = blockIdx.x, q = tiles >> 3, r = tiles & 7, x = i & 7;
  return x * q + (x < r ? x : r) + (i >> 3);
}

// NT: streaming (non-temporal) loads of the sort's key / value / link input, so a prepass
// that co-runs with the dataflow executor evicts less of the roster the executor keeps in
// the Infinity Cache (each pass reads its input once).  Stores stay plain: the digit runs
// need L2 write combining -- non-temporal stores as well measured 4.35 against 1.75 ms per
// prepass and 9.2 against 8.1 ms per bench step (re-checked: config 3 17.0 against 14.9 ms,
// config 5 14.1 against 10.9, profiles/r6/tail_points.log).
template <bool NT>
__device__ __forceinline__ uint32_t ld32(const uint32_t* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}

// exclusive scan of one value per thread over a 256-thread block
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t x, uint32_t* wsum,
                                                         uint32_t* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t inc = x;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t y = __shfl_up(inc, off);
    if (lane >= off) inc += y;
  }
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    if (w < wv) before += wsum[w];
    all += wsum[w];
  }
  if (total) *total = all;
  __syncthreads();  // wsum may be reused by the caller
  return before + inc - x;
}

// The schedule's first pass sorts the slots of the match stream straight from
// the records: key = the slot's player (kend if the match touches no state or
// the slot is empty), value = the slot index.  A workgroup decodes each match
// of its tile once (one thread per match, one 16-B-vector record load) into an
// LDS key array, instead of every slot re-decoding its whole match.
template <int KS>
__device__ __forceinline__ void decode_tile_keys(const int32_t* __restrict__ rec, uint32_t kend,
                                                 int64_t base, int64_t n, uint32_t* lk, uint32_t knone) {
  constexpr int S = 2 * KS, R = S + 2;
  const uint32_t lo = (uint32_t)base;  // slots < kMaxSlots
  const uint32_t hi = (uint32_t)(base + kTile < n ? base + kTile : n);
  const uint32_t m_lo = lo / S, m_hi = (hi + S - 1) / S;
  for (uint32_t m = m_lo + threadIdx.x; m < m_hi; m += kThreads) {
    uint32_t key[S];
    sched_slot_keys<KS>(rec + (int64_t)m * R, (int64_t)kend, knone, key);
#pragma unroll
    for (int j = 0; j < S; ++j) {
      const uint32_t slot = m * S + j;
      if (slot >= lo && slot < hi) lk[slot - lo] = key[j];
    }
  }
}

// What the schedule's first kernel also does, so the prepass needs no fill
// dispatches of its own: zero the window's completion counters (each tile its
// matches), the control words, and bump the device launch epoch (graph replays).
struct SchedInit {
  int32_t* deps = nullptr;       // [M] completion counters
  uint32_t* ctrl = nullptr;      // ctrl[0..nz) zeroed by block 0
  int nz = 0;
  int32_t* epoch_bump = nullptr; // += 1 by block 0
};

// KS > 0: keys from the match stream (decode_tile_keys), and the SchedInit duties.
template <int KS, bool NT = false>
__global__ void __launch_bounds__(kThreads)
radix_upsweep(const uint32_t* __restrict__ keys, const int32_t* __restrict__ rec, uint32_t kend,
              int64_t n, int shift, uint32_t* __restrict__ counts, int64_t tiles, SchedInit init = {},
              uint32_t knone = 0u) {
  __shared__ uint32_t hist[kWaves][kRadix];
  __shared__ uint32_t lkeys[KS > 0 ? kTile : 1];
  const int tid = threadIdx.x, wv = tid >> 6;
  for (int i = tid; i < kWaves * kRadix; i += kThreads) (&hist[0][0])[i] = 0u;
  const int64_t tile = xcd_tile(tiles);
  const int64_t base = tile * kTile;
  if constexpr (KS > 0) {
    if (init.deps) {  // the matches whose slots start in this tile (every match has its first slot in one)
      constexpr int S = 2 * KS;
      const int64_t hi = base + kTile < n ? base + kTile : n;
      for (int64_t m = (base + S - 1) / S + tid; m < (hi + S - 1) / S; m += kThreads) init.deps[m] = 0;
    }
    if (blockIdx.x == 0) {
      if (tid < init.nz) init.ctrl[tid] = 0u;
      if (tid == 0 && init.epoch_bump) init.epoch_bump[0] += 1;
    }
  }
  if constexpr (KS > 0) decode_tile_keys<KS>(rec, kend, base, n, lkeys, knone ? knone : kend);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    const int64_t idx = base + k * kThreads + tid;
    if (idx < n) {
      const uint32_t key = KS > 0 ? lkeys[k * kThreads + tid] : ld32<NT>(keys + idx);
      atomicAdd(&hist[wv][(key >> shift) & (kRadix - 1)], 1u);
    }
  }
  __syncthreads();
#pragma unroll
  for (int d = tid; d < kRadix; d += kThreads) {
    uint32_t c = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) c += hist[w][d];
    counts[(int64_t)d * tiles + tile] = c;
  }
}

// One workgroup per digit: counts[d][*] <- exclusive prefix over tiles; totals[d] <- row sum.
__global__ void __launch_bounds__(kThreads)
radix_rowscan(uint32_t* __restrict__ counts, int64_t tiles, uint32_t* __restrict__ totals) {
  __shared__ uint32_t wsum[kWaves];
  constexpr int kPer = 4;
  uint32_t* row = counts + (int64_t)blockIdx.x * tiles;
  uint32_t carry = 0;
  for (int64_t start = 0; start < tiles; start += kThreads * kPer) {
    uint32_t v[kPer], s = 0;
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      const int64_t t = start + (int64_t)threadIdx.x * kPer + q;
      v[q] = t < tiles ? row[t] : 0u;
      s += v[q];
    }
    uint32_t all;
    uint32_t ex = carry + block_exclusive_scan(s, wsum, &all);
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      const int64_t t = start + (int64_t)threadIdx.x * kPer + q;
      if (t < tiles) row[t] = ex;
      ex += v[q];
    }
    carry += all;
  }
  if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// The two ends of one (tile, digit) run of the schedule's last pass (first and last
// key / value; kf = kRunEmpty: the tile has no element of that digit).
struct RunEnds {
  uint32_t kf, vf, kl, vl;
};
constexpr uint32_t kRunEmpty = 0xffffffffu;

// KS > 0: elements come from the match stream (decode_tile_keys).  LINK (the schedule's
// last pass): instead of writing the sorted pairs, write every slot's link from
// its neighbours in the LDS-sorted tile -- within a (tile, digit) run they are
// its global neighbours -- and only the run-boundary pairs, whose outer
// neighbour lives in another tile (sched_fixup completes those links).
// bnd (LINK, last pass with nd <= kRunsMaxDigits digits): the boundary pairs go to a
// [tile][nd] RunEnds table instead of their global sorted positions, so this pass
// needs no digit offsets -- no upsweep / rowscan in front of it -- and sched_runs_fixup
// links each run to the nearest non-empty run of its digit in an earlier tile.
template <int KS, bool LINK, bool NT = false>
__global__ void __launch_bounds__(kThreads)
radix_downsweep(const uint32_t* __restrict__ kin, const uint32_t* __restrict__ vin,
                const int32_t* __restrict__ rec, uint32_t kend,
                uint32_t* __restrict__ kout, uint32_t* __restrict__ vout, int64_t n, int shift,
                const uint32_t* __restrict__ counts, const uint32_t* __restrict__ totals,
                int64_t tiles, int slots_per_match, uint32_t* __restrict__ link,
                uint32_t vlo = 0u, uint32_t vhi = 0xffffffffu, int bounds = 1,
                RunEnds* __restrict__ bnd = nullptr, int nd = 0, uint32_t knone = 0u) {
  __shared__ uint32_t skey[kTile];
  __shared__ uint32_t sval[kTile];
  __shared__ uint32_t wcnt[kWaves][kRadix];
  __shared__ uint32_t tstart[kRadix];
  __shared__ uint32_t gstart[kRadix];
  __shared__ uint32_t wsum[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t tile = xcd_tile(tiles);
  const int64_t base = tile * kTile;
  for (int i = tid; i < kWaves * kRadix; i += kThreads) (&wcnt[0][0])[i] = 0u;
  const bool local_ends = LINK && bnd != nullptr;  // uniform: no global digit offsets needed
  if (!local_ends) {  // global start of each digit for this tile
    const uint32_t below = block_exclusive_scan(tid < kRadix ? totals[tid] : 0u, wsum, nullptr);
    if (tid < kRadix) gstart[tid] = below + counts[(int64_t)tid * tiles + tile];
  }
  if constexpr (KS > 0)  // sval: scratch until the scatter
    decode_tile_keys<KS>(rec, kend, base, n, sval, knone ? knone : kend);
  __syncthreads();

  // wave wv owns tile elements [wv*kItems*64, (wv+1)*kItems*64) in (item, lane) order,
  // so (wave, item, lane) order is tile order and the ranks below are stable
  const uint64_t lt_mask = (1ull << lane) - 1ull;
  uint32_t key[kItems], val[kItems], rank[kItems];
#pragma unroll
  for (int it = 0; it < kItems; ++it) {
    const int64_t idx = base + (int64_t)(wv * kItems + it) * 64 + lane;
    const bool valid = idx < n;
    // pads sort last: digit 255, after every real key
    if constexpr (KS > 0) key[it] = valid ? sval[(wv * kItems + it) * 64 + lane] : 0xffffffffu;
    else key[it] = valid ? ld32<NT>(kin + idx) : 0xffffffffu;
    if constexpr (KS == 0) val[it] = valid ? ld32<NT>(vin + idx) : 0u;
    else val[it] = (uint32_t)idx;
  }
#pragma unroll
  for (int it = 0; it < kItems; ++it) {
    const uint32_t d = (key[it] >> shift) & (kRadix - 1);
    uint64_t peers = ~0ull;
#pragma unroll
    for (int b = 0; b < kRadixBits; ++b) {
      const uint64_t bal = __ballot((d >> b) & 1u);
      peers &= ((d >> b) & 1u) ? bal : ~bal;
    }
    const uint32_t before = (uint32_t)__popcll(peers & lt_mask);
    const uint32_t run = wcnt[wv][d];
    rank[it] = run + before;
    if (before == (uint32_t)__popcll(peers) - 1u) wcnt[wv][d] = run + (uint32_t)__popcll(peers);
  }
  __syncthreads();
  {  // per-digit prefix over waves, then tile-local digit starts
    uint32_t s = 0;
    if (tid < kRadix) {  // (threads past kRadix own no digit: they add 0 to the scan)
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        const uint32_t c = wcnt[w][tid];
        wcnt[w][tid] = s;
        s += c;
      }
    }
    const uint32_t ts = block_exclusive_scan(s, wsum, nullptr);
    if (tid < kRadix) tstart[tid] = ts;
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < kItems; ++it) {
    const uint32_t d = (key[it] >> shift) & (kRadix - 1);
    const uint32_t pos = tstart[d] + wcnt[wv][d] + rank[it];
    skey[pos] = key[it];
    sval[pos] = val[it];
  }
  __syncthreads();
  const int64_t nvalid = n - base < kTile ? n - base : kTile;
  if constexpr (LINK) {
    if (local_ends && bounds && tid < nd) {  // digits without an element in this tile
      const uint32_t e = tid + 1 < kRadix ? tstart[tid + 1] : (uint32_t)kTile;
      if (tstart[tid] == e) bnd[tile * nd + tid].kf = kRunEmpty;
    }
  }
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    const int i = k * kThreads + tid;
    if (i < nvalid) {
      const uint32_t kk = skey[i];
      const uint32_t d = (kk >> shift) & (kRadix - 1);
      const int64_t o = local_ends ? 0 : (int64_t)gstart[d] + (i - (int64_t)tstart[d]);
      if constexpr (!LINK) {
        kout[o] = kk;
        vout[o] = sval[i];
      } else {
        const int hi = d + 1 < (uint32_t)kRadix ? (int)tstart[d + 1] : kTile;
        const bool first = i == (int)tstart[d];
        const bool last = i + 1 == hi || i + 1 >= nvalid;
        const uint32_t v = sval[i];
        if (bounds && (first || last)) {  // the fix-up reads the boundary pairs of every run
          if (local_ends) {
            if ((int)d < nd) {  // (pads sort to digit kRadix - 1, past the schedule's digits)
              RunEnds* r = bnd + tile * nd + d;
              if (first) { r->kf = kk; r->vf = v; }
              if (last) { r->kl = kk; r->vl = v; }
            }
          } else {
            kout[o] = kk;
            vout[o] = v;
          }
        }
        if (kk < kend && v >= vlo && v < vhi) {  // this part's slot range (link_parts)
          uint32_t w = (!last && skey[i + 1] == kk) ? sval[i + 1] / (uint32_t)slots_per_match
                                                     : kNoMatch;
          if (!first && skey[i - 1] == kk) w |= kLinkHasPred;
          // (plain: non-temporal link stores alone measured 3.6 against 1.6 ms per prepass, L2
          // write combining of these random 4-B stores matters, profiles/r3/ab_link_nt.log)
          link[v] = w;
        }
      }
    }
  }
}

// The LINK pass in parts by slot range.  Its link stores are random 4-B writes,
// each its own fabric request (PMC: one TCC_EA0_WRREQ per store), and they stay
// cheap only while the link array they land in fits the 256-MB Infinity Cache:
// 60M 3v3 slots (240 MB) take 0.85 ms, 96M (config 5, 384 MB) 2.61 ms and 125M
// 5v5 slots (500 MB) 3.35 ms.  A larger array is written in ceil(bytes / 256 MB)
// passes over the sorted pairs, each storing only the links of its slot range
// (the LDS sort is repeated; the boundary pairs go out once): config 5 in two
// parts 2 x 0.91 ms, its step 13.40 -> 12.56 ms.  Splitting config 2's 240 MB
// as well costs more than it saves (8.13 -> 8.46 ms).  ANA_LINK_PARTS overrides
// the count (1 = one pass).
static int link_parts(int64_t n) {
  if (const char* e = getenv("ANA_LINK_PARTS")) {  // per launch: tests switch it at run time
    const int v = atoi(e);
    if (v >= 1) return v > 16 ? 16 : v;
  }
  const int64_t bytes = n * 4, part = 256ll << 20;
  return (int)((bytes + part - 1) / part);
}

// Completes the links of the run-boundary slots of the LINK pass: one thread per
// (tile, digit) run; its first pair's predecessor and its last pair's successor
// are the last / first pairs of the neighbouring runs, which that pass wrote.
// Grid: (tile groups of 256, digits); blocks of empty digits exit at once.
__global__ void __launch_bounds__(kThreads)
sched_fixup(const uint32_t* __restrict__ kout, const uint32_t* __restrict__ vout, int64_t n,
            uint32_t kend, const uint32_t* __restrict__ counts, const uint32_t* __restrict__ totals,
            int64_t tiles, int slots_per_match, uint32_t* __restrict__ link) {
  __shared__ uint32_t wsum[kWaves];
  const int d = blockIdx.y;
  const uint32_t tot = totals[d];
  if (tot == 0) return;
  uint32_t below = 0;
#pragma unroll
  for (int j = threadIdx.x; j < kRadix; j += kThreads) below += j < d ? totals[j] : 0u;
  uint32_t all = 0;
  const uint32_t before = block_exclusive_scan(below, wsum, &all);
  (void)before;
  const uint32_t dstart = all;  // sum of the totals of the digits below d
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= tiles) return;
  const uint32_t* row = counts + (int64_t)d * tiles;
  const uint32_t c0 = row[t];
  const uint32_t c1 = t + 1 < tiles ? row[t + 1] : tot;
  if (c1 == c0) return;
  const int64_t of = (int64_t)dstart + c0, ol = (int64_t)dstart + c1 - 1;
  const uint32_t kf = kout[of], kl = kout[ol];
  const bool pred = kf < kend && of > 0 && kout[of - 1] == kf;
  const bool succ = kl < kend && ol + 1 < n && kout[ol + 1] == kl;
  const uint32_t nxt = succ ? vout[ol + 1] / (uint32_t)slots_per_match : kNoMatch;
  if (of == ol) {
    if (kf < kend) link[vout[of]] = nxt | (pred ? kLinkHasPred : 0u);
    return;
  }
  if (pred) {
    const uint32_t v = vout[of];
    link[v] |= kLinkHasPred;
  }
  if (succ) {
    const uint32_t v = vout[ol];
    link[v] = (link[v] & ~kMatchMask) | nxt;
  }
}

// The last pass's run table -> links across tiles (sched_runs_fixup): the
// predecessor of the first pair of run (t, d) is the last pair of the nearest
// non-empty run (t' < t, d).  Segments of kThreads tiles: sched_runs_last finds each
// segment's last non-empty tile per digit, sched_runs_fixup takes the nearest one
// before its segment as the carry and a block max-scan of the non-empty tiles inside
// it.  Grids (segments, nd); nd <= kRunsMaxDigits keeps the table small.
constexpr int kRunsMaxDigits = 32;

__global__ void __launch_bounds__(kThreads)
sched_runs_last(const RunEnds* __restrict__ bnd, int64_t tiles, int nd, int32_t* __restrict__ seglast) {
  __shared__ int32_t wmax[kWaves];
  const int d = blockIdx.y;
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  int32_t x = (t < tiles && bnd[t * nd + d].kf != kRunEmpty) ? (int32_t)t : -1;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x = max(x, __shfl_xor(x, off));
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t m = wmax[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) m = max(m, wmax[w]);
    seglast[(int64_t)d * gridDim.x + blockIdx.x] = m;
  }
}

__global__ void __launch_bounds__(kThreads)
sched_runs_fixup(const RunEnds* __restrict__ bnd, int64_t tiles, int nd, const int32_t* __restrict__ seglast,
                 uint32_t kend, int slots_per_match, uint32_t* __restrict__ link) {
  __shared__ int32_t wmax[kWaves];
  __shared__ int32_t carry_s;
  const int d = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t seg = blockIdx.x;
  // carry: the last non-empty tile of digit d before this segment (seglast grows with the segment)
  if (wv == 0) {
    int32_t c = -1;
    for (int64_t q = lane; q < seg; q += 64) c = max(c, seglast[(int64_t)d * gridDim.x + q]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) c = max(c, __shfl_xor(c, off));
    if (lane == 0) carry_s = c;
  }
  const int64_t t = seg * kThreads + threadIdx.x;
  RunEnds me = {kRunEmpty, 0u, kRunEmpty, 0u};
  if (t < tiles) me = bnd[t * nd + d];
  const bool full = me.kf != kRunEmpty;
  // inclusive max-scan of the non-empty tiles: wave, then across the block's waves
  int32_t x = full ? (int32_t)t : -1;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int32_t y = __shfl_up(x, off);
    if (lane >= off) x = max(x, y);
  }
  if (lane == 63) wmax[wv] = x;
  __syncthreads();
  int32_t before = carry_s;
  for (int w = 0; w < wv; ++w) before = max(before, wmax[w]);
  int32_t ex = __shfl_up(x, 1);  // exclusive within the wave
  ex = lane == 0 ? -1 : ex;
  const int32_t pred = max(before, ex);
  if (!full || pred < 0 || me.kf >= kend) return;
  const RunEnds pr = bnd[(int64_t)pred * nd + d];
  if (pr.kl != me.kf) return;  // the key starts here: no earlier occurrence
  // the two boundary links: each word gets its bits from one thread each (atomics on
  // disjoint fields, so a one-pair run that is both a first and a last is safe)
  atomicOr(&link[me.vf], kLinkHasPred);
  atomicAnd(&link[pr.vl], ~kMatchMask | (me.vf / (uint32_t)slots_per_match));
}

// The chain pass (sched_sort_k, rosters of <= 2^20 players).  The links need less than a
// sorted array: per slot the match of the same player's next slot and a has-earlier
// bit.  After ONE stable partition by the key bits above `low` (<= 12) every bucket holds
// at most 2^low players in slot (time) order, and one workgroup per bucket chains them:
// it walks its bucket tile by tile, sorts each tile stably by the low key bits in LDS
// (two 6-bit rounds of the downsweep's ballot ranking, no global traffic) and keeps a
// last-occurrence table T[2^low] in LDS -- per player the last slot seen and its
// has-earlier bit (slots < 2^28: one word).  In the sorted tile
//   an element with a successor in the tile  writes link[slot] = succ match | has_pred,
//   the first of a player's run              writes the link T deferred for that player,
//   the last of a run                        goes into T, its link deferred,
// and after the last tile T is flushed with kNoMatch links.  Every link is written once,
// with plain stores (L2 write combining, see radix_downsweep); no workgroup waits on
// another.  KS > 0: no partition in front (top = 0, <= 4096 players): the one workgroup
// decodes its keys from the records, does the SchedInit duties and writes link[slot] itself
// (its windows are small).  LINES: the links of a bucket in bucket order instead, see below.
constexpr int kChainLowBits = 12;
constexpr int kChainRB = 6;
constexpr uint32_t kChainEmpty = 0xffffffffu;
constexpr bool kChainDefault = true;  // ANA_SCHED_CHAIN overrides (launch_sched_sort)

// one stable ranking round of the tile held in registers ((wave, item, lane) order = tile
// order) by kChainRB key bits at `shift`, scattered into skey / sval (VALS = false: keys only)
template <bool VALS = true>
__device__ __forceinline__ void chain_sort_round(const uint32_t (&key)[kItems], const uint32_t (&val)[kItems],
                                                 int shift, uint32_t* skey, uint32_t* sval,
                                                 uint32_t (*wcnt)[1 << kChainRB], uint32_t* tstart,
                                                 uint32_t* wsum) {
  constexpr int kR = 1 << kChainRB;
  static_assert(kR <= kThreads, "one digit per thread in the scan");
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint64_t lt_mask = (1ull << lane) - 1ull;
  for (int i = tid; i < kWaves * kR; i += kThreads) (&wcnt[0][0])[i] = 0u;
  __syncthreads();
  uint32_t rank[kItems];
#pragma unroll
  for (int it = 0; it < kItems; ++it) {
    const uint32_t d = (key[it] >> shift) & (kR - 1);
    uint64_t peers = ~0ull;
#pragma unroll
    for (int b = 0; b < kChainRB; ++b) {
      const uint64_t bal = __ballot((d >> b) & 1u);
      peers &= ((d >> b) & 1u) ? bal : ~bal;
    }
    const uint32_t before = (uint32_t)__popcll(peers & lt_mask);
    const uint32_t run = wcnt[wv][d];
    rank[it] = run + before;
    if (before == (uint32_t)__popcll(peers) - 1u) wcnt[wv][d] = run + (uint32_t)__popcll(peers);
  }
  __syncthreads();
  {  // per-digit prefix over waves, then tile-local digit starts
    uint32_t s = 0;
    if (tid < kR) {
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        const uint32_t c = wcnt[w][tid];
        wcnt[w][tid] = s;
        s += c;
      }
    }
    const uint32_t ts = block_exclusive_scan(s, wsum, nullptr);
    if (tid < kR) tstart[tid] = ts;
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < kItems; ++it) {
    const uint32_t d = (key[it] >> shift) & (kR - 1);
    const uint32_t pos = tstart[d] + wcnt[wv][d] + rank[it];
    skey[pos] = key[it];
    if constexpr (VALS) sval[pos] = val[it];
  }
  __syncthreads();
}

// LINES (a bucket of the partition, KS == 0): the links leave as whole lines.  A slot's link is written
// at the slot's POSITION in the partitioned arrays, in place over the bucket's keys (a tile's
// keys are dead once it is in registers, and only this workgroup reads its bucket), and
// sched_unpartition below carries it to link[slot].  The sort key of an element is its low key
// bits | its position in the tile << low (inside a bucket only the low bits differ), so a sorted
// element knows where it sat.  The links of a tile go through lbuf, indexed by that position,
// and leave one tile late: while tile i is linked, a deferred link of tile i - 1 is resolved in
// lbuf, one of an older tile with a plain store at its bucket position (T holds bucket positions);
// then lbuf is written out in position order, minus the positions still deferred (kLinkDeferred:
// masked, not written, so every link word has exactly one writer), and takes the links of tile i.
// Slots without state that share a chained bucket with players (256 buckets) get kLinkSkip.
constexpr uint32_t kLinkDeferred = 0xfffffffeu;  // lbuf only
constexpr uint32_t kLinkSkip = 0xffffffffu;      // no link for this slot: sched_unpartition leaves link[slot] alone

// (LINES: 116 KB of LDS, else 84 KB: one workgroup per CU, two waves per SIMD.  The link
// loops are unrolled by 2 only: fully unrolled the compiler takes 236 VGPRs, and two such waves
// no longer fit on a SIMD beside a wave of the executor)
template <int KS, bool NT, bool LINES>
__global__ void __launch_bounds__(kThreads)
sched_chain(uint32_t* kio, const uint32_t* __restrict__ vin,
            const int32_t* __restrict__ rec, uint32_t kend, int64_t n, int low,
            const uint32_t* __restrict__ totals, int slots_per_match, uint32_t* __restrict__ link,
            uint32_t vlo, uint32_t vhi, int64_t matches, SchedInit init) {
  constexpr int kR = 1 << kChainRB;
  static_assert(!LINES || KS == 0, "bucket positions need the partition");
  __shared__ uint32_t skey[kTile];
  __shared__ uint32_t sval[kTile];
  __shared__ uint32_t lbuf[LINES ? kTile : 1];        // links of the previous tile, by position
  __shared__ uint32_t last_seen[1 << kChainLowBits];  // T: slot (LINES: bucket position) | kLinkHasPred, kChainEmpty
  __shared__ uint32_t wcnt[kWaves][kR];
  __shared__ uint32_t tstart[kR];
  __shared__ uint32_t wsum[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t lmask = (1u << low) - 1u;
  for (int e = tid; e <= (int)lmask; e += kThreads) last_seen[e] = kChainEmpty;
  // this workgroup's bucket: [start, start + cnt) of the partitioned pairs
  int64_t start = 0, cnt = n;
  if constexpr (KS > 0) {
    if (init.deps)
      for (int64_t m = tid; m < matches; m += kThreads) init.deps[m] = 0;
    if (tid < init.nz) init.ctrl[tid] = 0u;
    if (tid == 0 && init.epoch_bump) init.epoch_bump[0] += 1;
  } else {
    uint32_t below = 0;
    const uint32_t x = tid < (int)blockIdx.x ? totals[tid] : 0u;  // <= 256 buckets <= kThreads
    block_exclusive_scan(x, wsum, &below);
    start = below;
    cnt = totals[blockIdx.x];
  }
  const uint32_t kbase = LINES ? (uint32_t)blockIdx.x << low : 0u;  // the bucket's key bits above `low`
  for (int64_t base = 0; base < cnt; base += kTile) {
    const int64_t nvalid = cnt - base < kTile ? cnt - base : kTile;
    uint32_t key[kItems], val[kItems];
    if constexpr (KS > 0) {
      decode_tile_keys<KS>(rec, kend, base, n, sval, kend);  // sval: scratch until the scatter
      __syncthreads();
    }
    // (loading the next tile's pairs ahead, over this tile's link stores, measured slower
    // beside the executor: 6.31-6.35 against 6.09-6.10 ms per config 2 step)
#pragma unroll
    for (int it = 0; it < kItems; ++it) {
      const int p = (wv * kItems + it) * 64 + lane;
      const bool valid = p < nvalid;
      const int64_t idx = start + base + p;
      // pads sort last: both digits 63, after every real key of the tile (stable)
      if constexpr (KS > 0) {
        key[it] = valid ? sval[p] : 0xffffffffu;
        val[it] = (uint32_t)idx;
      } else if constexpr (!LINES) {
        key[it] = valid ? ld32<NT>(kio + idx) : 0xffffffffu;
        val[it] = valid ? ld32<NT>(vin + idx) : 0u;
      } else {
        // the slots stay in tile order (sval[p]); only the keys are sorted, and each carries its p
        key[it] = valid ? (ld32<NT>(kio + idx) & lmask) | (uint32_t)p << low : 0xffffffffu;
        if (valid) sval[p] = ld32<NT>(vin + idx);
      }
    }
    chain_sort_round<!LINES>(key, val, 0, skey, sval, wcnt, tstart, wsum);
    if (low > kChainRB) {  // (uniform)
#pragma unroll
      for (int it = 0; it < kItems; ++it) {
        const int p = (wv * kItems + it) * 64 + lane;
        key[it] = skey[p];
        if constexpr (!LINES) val[it] = sval[p];
      }
      chain_sort_round<!LINES>(key, val, kChainRB, skey, sval, wcnt, tstart, wsum);
    }
    // the tile is sorted by player, each player's slots in time order
    uint32_t is_last = 0u, has = 0u;  // bit k: element k of this thread ends a run / has a predecessor
    if constexpr (!LINES) {
#pragma unroll 2
      for (int k = 0; k < kItems; ++k) {
        const int i = k * kThreads + tid;
        if (i < nvalid) {
          const uint32_t kk = skey[i];
          if (kk < kend) {
            const uint32_t v = sval[i];
            const bool next = i + 1 < nvalid && skey[i + 1] == kk;
            bool pred = i > 0 && skey[i - 1] == kk;
            if (!pred) {  // first of its run: the player's last slot of an earlier tile links here
              const uint32_t t = last_seen[kk & lmask];
              if (t != kChainEmpty) {
                pred = true;
                const uint32_t ts = t & kMatchMask;
                if (ts >= vlo && ts < vhi) link[ts] = v / (uint32_t)slots_per_match | (t & kLinkHasPred);
              }
            }
            if (next) {
              if (v >= vlo && v < vhi)  // this part's slot range (link_parts)
                link[v] = sval[i + 1] / (uint32_t)slots_per_match | (pred ? kLinkHasPred : 0u);
            } else {
              is_last |= 1u << k;
            }
            if (pred) has |= 1u << k;
          }
        }
      }
      __syncthreads();  // every first has read T before the lasts replace its entries
#pragma unroll 2
      for (int k = 0; k < kItems; ++k) {
        const int i = k * kThreads + tid;
        if (is_last >> k & 1u) last_seen[skey[i] & lmask] = sval[i] | (has >> k & 1u ? kLinkHasPred : 0u);
      }
    } else {
      const int64_t prev = base - kTile;  // bucket position of lbuf[0]: the previous tile
#pragma unroll 2
      for (int k = 0; k < kItems; ++k) {
        const int i = k * kThreads + tid;
        if (i < nvalid) {
          const uint32_t kl = skey[i] & lmask;
          if ((kbase | kl) < kend) {
            const bool next = i + 1 < nvalid && (skey[i + 1] & lmask) == kl;
            bool pred = i > 0 && (skey[i - 1] & lmask) == kl;
            if (!pred) {  // first of its run: the link T deferred for this player
              const uint32_t t = last_seen[kl];
              if (t != kChainEmpty) {
                pred = true;
                const int64_t tp = t & kMatchMask;
                const uint32_t w = sval[skey[i] >> low] / (uint32_t)slots_per_match | (t & kLinkHasPred);
                if (tp >= prev) lbuf[tp - prev] = w;  // still in LDS: leaves with its tile's lines
                else kio[start + tp] = w;            // an older tile: the one random store left
              }
            }
            if (!next) is_last |= 1u << k;
            if (pred) has |= 1u << k;
          }
        }
      }
      __syncthreads();  // lbuf holds every link of the previous tile that this tile resolves
      // (the address as kio + start, then + prev + j: written kio[start + prev + j] the compiler
      // schedules this kernel differently, 0.01-0.02 ms per prepass, profiles/r10/sched_variants_ab.log)
      if (base > 0) {   // (a previous tile is a full tile)
#pragma unroll 2
        for (int k = 0; k < kItems; ++k) {
          const int j = k * kThreads + tid;
          const uint32_t w = lbuf[j];
          if (w != kLinkDeferred) *(kio + start + prev + j) = w;
        }
      }
#pragma unroll 2
      for (int k = 0; k < kItems; ++k) {
        const int i = k * kThreads + tid;
        if (is_last >> k & 1u) {
          const uint32_t kk = skey[i];
          last_seen[kk & lmask] = (uint32_t)(base + (kk >> low)) | (has >> k & 1u ? kLinkHasPred : 0u);
        }
      }
      __syncthreads();  // lbuf is written out
#pragma unroll 2
      for (int k = 0; k < kItems; ++k) {
        const int i = k * kThreads + tid;
        if (i < nvalid) {
          const uint32_t kk = skey[i];
          uint32_t w = kLinkSkip;
          if ((kbase | (kk & lmask)) < kend)
            w = is_last >> k & 1u ? kLinkDeferred
                                  : sval[skey[i + 1] >> low] / (uint32_t)slots_per_match |
                                        (has >> k & 1u ? kLinkHasPred : 0u);
          lbuf[kk >> low] = w;
        }
      }
    }
    __syncthreads();  // skey / sval are rewritten by the next tile
  }
  __syncthreads();
  if constexpr (!LINES) {
    for (int e = tid; e <= (int)lmask; e += kThreads) {  // the last slot of every player seen
      const uint32_t t = last_seen[e];
      if (t != kChainEmpty) {
        const uint32_t ts = t & kMatchMask;
        if (ts >= vlo && ts < vhi) link[ts] = kNoMatch | (t & kLinkHasPred);
      }
    }
  } else {
    // the last slot of every player seen; those of the last tile leave with its lines
    const int64_t lastb = cnt > 0 ? (cnt - 1) / kTile * kTile : 0;
    for (int e = tid; e <= (int)lmask; e += kThreads) {
      const uint32_t t = last_seen[e];
      if (t != kChainEmpty) {
        const int64_t tp = t & kMatchMask;
        const uint32_t w = kNoMatch | (t & kLinkHasPred);
        if (tp >= lastb) lbuf[tp - lastb] = w;
        else kio[start + tp] = w;
      }
    }
    __syncthreads();
    for (int64_t j = tid; j < cnt - lastb; j += kThreads) *(kio + start + lastb + j) = lbuf[j];
  }
}

// Links from bucket order to slot order (after sched_chain<0>): one workgroup per INPUT tile of
// the partition.  The partition is stable, so the pairs a tile sent to one bucket are one run
// of that bucket, in slot order, at the offset radix_downsweep stored them to: this kernel is
// its store loop turned into loads.  It reads the tile's runs of slots (vo) and of links (lk:
// what sched_chain left in place of the keys), places each link in LDS at slot - tile start
// and writes link[tile] as whole lines.  Slots that get no link -- the buckets nobody chains
// (d >= nb) and kLinkSkip -- are left alone.
template <bool NT>
__global__ void __launch_bounds__(kThreads)
sched_unpartition(const uint32_t* __restrict__ lk, const uint32_t* __restrict__ vo, int64_t n,
                  const uint32_t* __restrict__ counts, const uint32_t* __restrict__ totals,
                  int64_t tiles, int nb, uint32_t* __restrict__ link) {
  __shared__ uint32_t out[kTile];
  __shared__ uint32_t tstart[kRadix];  // start of each digit's run in the (sorted) tile
  __shared__ uint32_t gstart[kRadix];  // ... and in the partitioned arrays
  __shared__ uint32_t wsum[kWaves];
  const int tid = threadIdx.x;
  const int64_t tile = xcd_tile(tiles);
  const int64_t base = tile * kTile;
  const int64_t nvalid = n - base < kTile ? n - base : kTile;
  uint32_t c0 = 0u, len = 0u;
  if (tid < nb) {
    c0 = counts[(int64_t)tid * tiles + tile];
    len = (tile + 1 < tiles ? counts[(int64_t)tid * tiles + tile + 1] : totals[tid]) - c0;
  }
  uint32_t nchain = 0u;
  const uint32_t g = block_exclusive_scan(tid < kRadix ? totals[tid] : 0u, wsum, nullptr);
  const uint32_t ts = block_exclusive_scan(len, wsum, &nchain);
  if (tid < kRadix) {
    gstart[tid] = g + c0;
    tstart[tid] = ts;  // (digits >= nb: nchain, past every element)
  }
#pragma unroll
  for (int k = 0; k < kItems; ++k) out[k * kThreads + tid] = kLinkSkip;
  __syncthreads();
#pragma unroll 4
  for (int k = 0; k < kItems; ++k) {
    const uint32_t i = k * kThreads + tid;
    if (i < nchain) {
      uint32_t d = 0u;  // the last digit whose run starts at or before i (the runs before it may be empty)
#pragma unroll
      for (uint32_t step = kRadix >> 1; step > 0u; step >>= 1)
        if (tstart[d + step] <= i) d += step;
      const int64_t o = (int64_t)gstart[d] + (i - tstart[d]);
      if (o < n) {
        const uint32_t at = ld32<NT>(vo + o) - (uint32_t)base;
        if (at < (uint32_t)kTile) out[at] = ld32<NT>(lk + o);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kItems / 4; ++k) {
    const int j = (k * kThreads + tid) * 4;
    const uint4 w = *reinterpret_cast<const uint4*>(out + j);
    const bool all = w.x != kLinkSkip && w.y != kLinkSkip && w.z != kLinkSkip && w.w != kLinkSkip;
    if (j + 4 <= nvalid && all && (reinterpret_cast<uintptr_t>(link + base + j) & 15u) == 0u) {
      *reinterpret_cast<uint4*>(link + base + j) = w;
    } else {
      if (j < nvalid && w.x != kLinkSkip) link[base + j] = w.x;
      if (j + 1 < nvalid && w.y != kLinkSkip) link[base + j + 1] = w.y;
      if (j + 2 < nvalid && w.z != kLinkSkip) link[base + j + 2] = w.z;
      if (j + 3 < nvalid && w.w != kLinkSkip) link[base + j + 3] = w.w;
    }
  }
}

}  // namespace

size_t radix_sort_workspace_bytes(int64_t n) {
  const int64_t tiles = (n + kTile - 1) / kTile;
  return (size_t)(tiles * kRadix + kRadix) * 4;  // counts[kRadix][tiles], totals[kRadix]
}

int launch_radix_sort_pairs(uint32_t* keys, uint32_t* vals, uint32_t* keys_alt, uint32_t* vals_alt,
                            int64_t n, int bits, void* ws, int* result_in_alt, hipStream_t s) {
  *result_in_alt = 0;
  if (n <= 0) return 0;
  if (n > 0x7fffffffLL || bits < 1 || bits > 32) return (int)hipErrorInvalidValue;
  const int64_t tiles = (n + kTile - 1) / kTile;
  uint32_t* counts = static_cast<uint32_t*>(ws);
  uint32_t* totals = counts + tiles * kRadix;
  uint32_t *ki = keys, *vi = vals, *ko = keys_alt, *vo = vals_alt;
  for (int shift = 0; shift < bits; shift += 8) {
    hipLaunchKernelGGL(radix_upsweep<0>, dim3((unsigned)tiles), dim3(kThreads), 0, s, ki, nullptr,
                       0u, n, shift, counts, tiles);
    hipLaunchKernelGGL(radix_rowscan, dim3(kRadix), dim3(kThreads), 0, s, counts, tiles, totals);
    hipLaunchKernelGGL((radix_downsweep<0, false>), dim3((unsigned)tiles), dim3(kThreads), 0, s, ki,
                       vi, nullptr, 0u, ko, vo, n, shift, counts, totals, tiles, 1, nullptr);
    std::swap(ki, ko);
    std::swap(vi, vo);
    *result_in_alt ^= 1;
  }
  return (int)hipGetLastError();
}

// The schedule's sort (K5): the slots of the stream by player, stable, fused at
// both ends -- the first pass reads the records (no key array is written), the
// last pass writes links instead of sorted pairs, then a fix-up of the run boundaries.
// NT: the passes stream their input with non-temporal loads (ld32).
template <int K, bool NT>
static void sched_sort_k(const int32_t* rec, int64_t n, uint32_t kend, int bits, uint32_t* ka,
                         uint32_t* va, uint32_t* kb, uint32_t* vb, uint32_t* counts,
                         int64_t tiles, uint32_t* link, const SchedInit& init, bool chain,
                         hipStream_t s) {
  constexpr int S = 2 * K;
  uint32_t* totals = counts + tiles * kRadix;
  const dim3 grid((unsigned)tiles), block(kThreads);
  const uint32_t *ki = nullptr, *vi = nullptr;
  uint32_t *ko = kb, *vo = vb;
  if (chain) {  // one partition by the bits above `low`, then one workgroup per bucket (sched_chain)
    const int low = bits < kChainLowBits ? bits : kChainLowBits, top = bits - low;
    if (top > 0) {
      // Players fill the buckets below nb.  The slots without state (key kend: 2 % of the
      // matches of the bench stream, five buckets' worth) would all land in kend's bucket and
      // make its workgroup the long pole, so the partition keys them with the first key of
      // bucket nb instead, which no workgroup chains (when nb is a digit of its own, < 256).
      const uint32_t nb = ((kend - 1u) >> low) + 1u;
      const uint32_t knone = nb < (uint32_t)kRadix ? nb << low : kend;
      hipLaunchKernelGGL((radix_upsweep<K, NT>), grid, block, 0, s, nullptr, rec, kend, n, low, counts, tiles,
                         init, knone);
      hipLaunchKernelGGL(radix_rowscan, dim3(kRadix), block, 0, s, counts, tiles, totals);
      hipLaunchKernelGGL((radix_downsweep<K, false, NT>), grid, block, 0, s, nullptr, nullptr, rec, kend, ko,
                         vo, n, low, counts, totals, tiles, S, nullptr, 0u, 0xffffffffu, 1, nullptr, 0, knone);
      // A prepass beside the executor (its caller streams the sort's input with non-temporal
      // loads: sort_nt / ANA_SORT_NT = 2) writes the links as whole lines: the executor pays
      // for the prepass's write requests, and the step is 0.27-0.37 ms shorter.  A prepass with
      // nothing beside it keeps the direct stores: alone they are 0.32 ms faster per window
      // (config 2 with ANA_PREPASS_SERIAL=1: 6.32-6.37 against 6.69-6.72 ms with whole lines).
      if constexpr (NT) {
        // once, whatever ANA_LINK_PARTS says: there is no randomly written link array to keep
        // inside the Infinity Cache
        hipLaunchKernelGGL((sched_chain<0, NT, true>), dim3(nb), block, 0, s, ko, vo, nullptr, kend, n, low,
                           totals, S, nullptr, 0u, 0xffffffffu, n / S, SchedInit{});
        hipLaunchKernelGGL(sched_unpartition<NT>, grid, block, 0, s, ko, vo, n, counts, totals, tiles,
                           (int)nb, link);
      } else {
        const int parts = link_parts(n);
        for (int q = 0; q < parts; ++q)
          hipLaunchKernelGGL((sched_chain<0, NT, false>), dim3(nb), block, 0, s, ko, vo, nullptr, kend, n, low,
                             totals, S, link, (uint32_t)(n * q / parts), (uint32_t)(n * (q + 1) / parts),
                             n / S, SchedInit{});
      }
    } else {
      const int parts = link_parts(n);
      for (int q = 0; q < parts; ++q)
        hipLaunchKernelGGL((sched_chain<K, NT, false>), dim3(1), block, 0, s, nullptr, nullptr, rec, kend, n, low,
                           nullptr, S, link, (uint32_t)(n * q / parts), (uint32_t)(n * (q + 1) / parts),
                           n / S, q == 0 ? init : SchedInit{});
    }
    return;
  }
  for (int shift = 0; shift < bits; shift += kRadixBits) {
    const bool first = shift == 0, last = shift + kRadixBits >= bits;
    // the last pass of a multi-pass sort over few digits (1M players: bits 16..19, 16
    // digits): run ends in a table, no digit offsets (radix_downsweep bnd).  A last pass over
    // more digits (config 5, 10M players: 256) takes the digit offsets and sched_fixup below.
    const int nd = bits - shift < kRadixBits ? 1 << (bits - shift) : kRadix;
    if (last && !first && nd <= kRunsMaxDigits) {
      // The table lives in the counts region, whose pass counts are consumed by now: that
      // region is kRadix * 4 = 1024 B per tile (+ 1024 B of totals); bnd takes nd * 16 <= 512 B
      // per tile (nd <= kRunsMaxDigits = 32) and seglast nd * 4 <= 128 B per segment of
      // kThreads tiles, i.e. under 1 B per tile + 128 B.
      RunEnds* bnd = reinterpret_cast<RunEnds*>(counts);
      const int64_t nseg = (tiles + kThreads - 1) / kThreads;
      int32_t* seglast = reinterpret_cast<int32_t*>(bnd + tiles * nd);
      const int parts = link_parts(n);
      for (int q = 0; q < parts; ++q)
        hipLaunchKernelGGL((radix_downsweep<0, true, NT>), grid, block, 0, s, ki, vi, nullptr, kend, ko, vo,
                           n, shift, counts, totals, tiles, S, link, (uint32_t)(n * q / parts),
                           (uint32_t)(n * (q + 1) / parts), q == 0 ? 1 : 0, bnd, nd);
      const dim3 sgrid((unsigned)nseg, (unsigned)nd);
      hipLaunchKernelGGL(sched_runs_last, sgrid, block, 0, s, bnd, tiles, nd, seglast);
      hipLaunchKernelGGL(sched_runs_fixup, sgrid, block, 0, s, bnd, tiles, nd, seglast, kend, S, link);
      break;
    }
    if (first)
      hipLaunchKernelGGL((radix_upsweep<K, NT>), grid, block, 0, s, nullptr, rec, kend, n, shift, counts, tiles,
                         init);
    else
      hipLaunchKernelGGL((radix_upsweep<0, NT>), grid, block, 0, s, ki, nullptr, kend, n, shift, counts, tiles);
    hipLaunchKernelGGL(radix_rowscan, dim3(kRadix), block, 0, s, counts, tiles, totals);
    const int parts = last ? link_parts(n) : 1;
    if (first && last)
      for (int q = 0; q < parts; ++q)
        hipLaunchKernelGGL((radix_downsweep<K, true, NT>), grid, block, 0, s, nullptr, nullptr, rec, kend, ko,
                           vo, n, shift, counts, totals, tiles, S, link, (uint32_t)(n * q / parts),
                           (uint32_t)(n * (q + 1) / parts), q == 0 ? 1 : 0);
    else if (first)
      hipLaunchKernelGGL((radix_downsweep<K, false, NT>), grid, block, 0, s, nullptr, nullptr, rec, kend, ko,
                         vo, n, shift, counts, totals, tiles, S, nullptr);
    else if (last)
      for (int q = 0; q < parts; ++q)
        hipLaunchKernelGGL((radix_downsweep<0, true, NT>), grid, block, 0, s, ki, vi, nullptr, kend, ko, vo,
                           n, shift, counts, totals, tiles, S, link, (uint32_t)(n * q / parts),
                           (uint32_t)(n * (q + 1) / parts), q == 0 ? 1 : 0);
    else
      hipLaunchKernelGGL((radix_downsweep<0, false, NT>), grid, block, 0, s, ki, vi, nullptr, kend, ko, vo, n,
                         shift, counts, totals, tiles, S, nullptr);
    if (last)
      hipLaunchKernelGGL(sched_fixup, dim3((unsigned)((tiles + kThreads - 1) / kThreads), kRadix), block,
                         0, s, ko, vo, n, kend, counts, totals, tiles, S, link);
    ki = ko;
    vi = vo;
    ko = ko == kb ? ka : kb;
    vo = vo == vb ? va : vb;
  }
}

int launch_sched_sort(int K, const int32_t* rec, int64_t M, uint32_t num_players, uint32_t* ka,
                      uint32_t* va, uint32_t* kb, uint32_t* vb, void* ws, uint32_t* link,
                      hipStream_t s, int32_t* deps, uint32_t* ctrl, int nz, int32_t* epoch_bump,
                      int sort_nt) {
  const int64_t n = M * 2 * K;
  if (n <= 0) return 0;
  if (n > kMaxSlots) return (int)hipErrorInvalidValue;
  int bits = 1;  // keys run up to num_players (= "no state")
  while (bits < 32 && (1ull << bits) <= (uint64_t)num_players) ++bits;
  const int64_t tiles = (n + kTile - 1) / kTile;
  uint32_t* counts = static_cast<uint32_t*>(ws);
  SchedInit init;
  init.deps = deps;
  init.ctrl = ctrl;
  init.nz = ctrl ? nz : 0;
  init.epoch_bump = epoch_bump;
  // Non-temporal loads: 0 (none) or 2 (every pass streams its input).  sort_nt >= 0 is the
  // caller's choice (WindowPipeline: 2 for a prepass beside the executor); ANA_SORT_NT wins,
  // read per schedule like ANA_SCHED_CHAIN / ANA_LINK_PARTS, so that tests reach the
  // whole-lines path through BatchRater.rate.  Any other value is refused before a launch.
  const char* nt_e = getenv("ANA_SORT_NT");
  const int nt = nt_e ? atoi(nt_e) : sort_nt >= 0 ? sort_nt : 0;
  if (nt != 0 && nt != 2) return (int)hipErrorInvalidValue;
  // The chain pass (sched_chain) for rosters of <= 2^20 players; above that (config 5) the
  // three LSD passes stay.  ANA_SCHED_CHAIN=1 / 0 forces it / the LSD passes.
  // Unforced, the chain pass runs where its one workgroup per bucket is not the long pole.
  // A workgroup chains a tile in ~26 us (0.79 ms for the 30 tiles of a config 2 bucket),
  // the LSD passes take ~27 ps per slot (1.6 ms for 60M) on top of ~40 us of launches:
  // the chain pass wins while a bucket averages under 2 tiles + n / 128 slots, i.e. with
  // >= 128 buckets at any window size, or in small windows.  (The small-window end of this
  // rule is reasoned from those two rates, not measured.)
  const char* chain_e = getenv("ANA_SCHED_CHAIN");
  const int top = bits > kChainLowBits ? bits - kChainLowBits : 0;
  const bool chain_pays = (n >> top) <= 2 * kTile + n / 128;
  const bool chain = (chain_e ? atoi(chain_e) != 0 : kChainDefault && chain_pays) && bits <= 20;
  const bool known = with_team_size(K, [&](auto k) {
    constexpr int kK = decltype(k)::value;
    if (nt == 2) sched_sort_k<kK, true>(rec, n, num_players, bits, ka, va, kb, vb, counts, tiles, link, init, chain, s);
    else sched_sort_k<kK, false>(rec, n, num_players, bits, ka, va, kb, vb, counts, tiles, link, init, chain, s);
  });
  return known ? (int)hipGetLastError() : (int)hipErrorInvalidValue;
}

}  // namespace ana
