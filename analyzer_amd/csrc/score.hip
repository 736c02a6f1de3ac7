// K14 scorecard: the belief before every match of a window, reconstructed from the match
// stream rec [M][2K+2] joined with its packed output rows [M][W], and the score of the
// prediction that belief makes (score_core.h).
//
// Priors.  chain [P][kBaseFloats] is updated in place, window by window; every value is a
// copied bit pattern and prior_combine is associative, so priors and chain are the same bits
// for any grid, tile size or cut of the history into calls.  No atomics, and no workgroup
// waits on another: six stream-ordered steps.
//
//   keys       one lane per match: per slot the sort key -- the player of a live slot, else
//              P --, the value (slot index | mode << 28 | write flag << 31) and, for a slot
//              that writes, its 16-B event (s_mu, s_sig, m_mu, m_sig), so the later passes
//              never touch the 128-B row line.  Slots that are not live get their NaN priors
//              here (slot-major, 16 B per slot), and sort last.
//   sort       launch_radix_sort_pairs on bit_length(P) bits: stable, so each player's slots
//              come out in (match, slot) order.
//   summaries  one workgroup per tile of kPriorTile sorted elements.  The exclusive scan is
//              run as the inclusive scan over shifted terms: element i contributes the write of
//              element i - 1 of the same key, so the scanned value is the state before i and
//              one 16-B gather per element feeds it.  The totals of the tile's first and last
//              key (without any starting state) go to edges[2 * tile + 0 / 1].
//   stitch     one workgroup over the 2 * tiles edges, seeded from the chain rows: carry[e] is
//              the state before edge e's stretch; a key's last edge stores its chain row.
//   apply      the summaries scan again, seeded from carry or, for a run strictly inside the
//              tile, from the chain row, which the run's last element stores.  Every live
//              element stores the four prior words of its mode as one 16-B slot-major entry.
//   fields     one lane per match: the slot-major entries [M][2K][4] to the field-major
//              priors [M][4][2K], 16-B loads and stores (four scattered 4-B stores per slot
//              in apply instead cost more than this pass and its buffer).
//
// summaries, stitch and apply are the chained scan of chain_dev.h over PriorChain below; its
// header has the argument why the chain rows are read and written in place without a race.
//
// Score.  One lane per match over rec, priors, the row's status byte and (behind a NULL
// shared track only) attrs: player_prior per slot, then d and sum sigma^2 in preview_kernel's
// operation order (matchmake.hip; the butterfly as butterfly_sum), p_win0 and p_outcome.  The
// table is integer sums only: each workgroup adds into a copy in LDS and then once per
// non-zero cell into the global table, so any order gives the same bits.
//
// Built with -ffp-contract=off: every fp32 operation is the one written.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "chain_dev.h"
#include "common.h"
#include "kernels.h"
#include "record_dev.h"
#include "score_core.h"

namespace ana {

namespace {

constexpr int kPriorThreads = 256;
constexpr int kScoreThreads = 256;

typedef unsigned int v2u __attribute__((ext_vector_type(2)));
typedef unsigned int v4u __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));

template <int K>
__global__ void __launch_bounds__(kPriorThreads) prior_keys_kernel(
    const int32_t* __restrict__ rec, const uint32_t* __restrict__ rows, int64_t W, int64_t M, int64_t P,
    uint32_t* __restrict__ keys, uint32_t* __restrict__ vals, v4u* __restrict__ events,
    v4u* __restrict__ slot_priors) {
  constexpr int S = 2 * K;
  const int64_t m = (int64_t)blockIdx.x * kPriorThreads + threadIdx.x;
  if (m >= M) return;
  int32_t r[S + 2];
  load_record<K>(rec, m, r);
  const uint32_t live = prior_live_mask<K>(r, P);
  const uint32_t mode = (uint32_t)meta_mode((uint32_t)r[S]);
  uint32_t writes = 0u;
  uint32_t sh[2 * S], md[2 * S];  // the fields (s_mu, s_sig) and (m_mu, m_sig), as 8-B loads
  if (live) {
    const uint32_t* row = rows + m * W;
    const v2u tail = *reinterpret_cast<const v2u*>(row + 5 * S);
    if ((tail[1] & 0xffu) == kRated) {
      writes = prior_last_mask<K>(r, live);
      const v2u* a = reinterpret_cast<const v2u*>(row);
      const v2u* b = reinterpret_cast<const v2u*>(row + 3 * S);
#pragma unroll
      for (int c = 0; c < S; ++c) {
        const v2u x = a[c], y = b[c];
        sh[2 * c] = x[0];
        sh[2 * c + 1] = x[1];
        md[2 * c] = y[0];
        md[2 * c + 1] = y[1];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < S; ++j) {
    const int64_t i = m * S + j;
    const bool lv = (live >> j) & 1u, wr = (writes >> j) & 1u;
    keys[i] = lv ? (uint32_t)r[j] : (uint32_t)P;
    vals[i] = (uint32_t)i | (lv ? mode << kPriorModeShift : 0u) | (wr ? kPriorWriteBit : 0u);
    if (wr) {
      v4u e;
      e[0] = sh[j];
      e[1] = sh[S + j];
      e[2] = md[j];
      e[3] = md[S + j];
      events[i] = e;
    }
    if (!lv) {
      v4u none;
      none[0] = none[1] = none[2] = none[3] = kPriorNull;
      slot_priors[i] = none;
    }
  }
}

// The feature of the chained scan (chain_dev.h): an exclusive scan under "the later write
// wins", run as the inclusive one over shifted terms.  An element contributes the write of the
// one before it, so its scanned state is the one before it; a run's total adds its own write.
struct PriorChain {
  typedef PriorState State;
  const v4u* __restrict__ events;
  int64_t n;
  v4u* __restrict__ slot_priors;

  static __device__ __forceinline__ PriorState identity() { return prior_none(); }
  static __device__ __forceinline__ State combine(const State& a, const State& b) { return prior_combine(a, b); }
  static __device__ __forceinline__ PriorState seed(const uint32_t* __restrict__ chain, uint32_t key) {
    return prior_from_chain(chain + (int64_t)key * kBaseFloats);
  }
  static __device__ __forceinline__ void row_store(uint32_t* __restrict__ chain, uint32_t key, const PriorState& s) {
    uint32_t* row = chain + (int64_t)key * kBaseFloats;
#pragma unroll
    for (int i = 0; i < 2 * kTracks; ++i) row[i] = s.w[i];
  }

  // the write of the slot with sort value v (prior_none() when it does not write)
  __device__ __forceinline__ PriorState write(uint32_t v) const {
    const uint32_t slot = v & kPriorSlotMask;
    if (!(v & kPriorWriteBit) || (int64_t)slot >= n) return prior_none();  // slot < n always: a permutation
    const v4u e = events[slot];
    return prior_write((int)((v >> kPriorModeShift) & 7u), e[0], e[1], e[2], e[3]);
  }
  __device__ __forceinline__ PriorState next(uint32_t prev, uint32_t) const { return write(prev); }
  __device__ __forceinline__ PriorState first(uint32_t, const PriorState& seed) const { return seed; }
  __device__ __forceinline__ PriorState open(uint32_t, uint32_t, bool, const uint32_t*) const { return prior_none(); }
  __device__ __forceinline__ State total(uint32_t v, const State& s) const { return prior_combine(s, write(v)); }
  // the four prior words of the element's mode from the state before it, as one 16-B store
  __device__ __forceinline__ void emit(uint32_t v, const PriorState& s) const {
    const uint32_t slot = v & kPriorSlotMask;
    if ((int64_t)slot >= n) return;
    uint32_t w[4];
    prior_pick(s, (int)((v >> kPriorModeShift) & 7u), w);
    v4u x;
#pragma unroll
    for (int f = 0; f < 4; ++f) x[f] = w[f];
    slot_priors[slot] = x;
  }
};
typedef ChainScan<PriorChain, kPriorThreads, kPriorTile> PriorScan;
static_assert(sizeof(PriorScan::Edge) == 64 && offsetof(PriorScan::Edge, s) == 4, "an edge: [key, mask, w[14]]");

template <bool APPLY>  // summaries (false) and apply (true)
__global__ void __launch_bounds__(kPriorThreads) prior_tile_kernel(
    const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, const v4u* __restrict__ events, int64_t n,
    uint32_t P, uint32_t* __restrict__ chain, PriorScan::Edge* __restrict__ edges,
    const PriorScan::Edge* __restrict__ carry, v4u* __restrict__ slot_priors) {
  PriorScan::tile<APPLY>(keys, vals, n, P, chain, edges, carry, PriorChain{events, n, slot_priors});
}

// slot-major prior words [M][2K][4] to the field-major priors [M][4][2K]: one lane per match,
// 16-B loads and stores
template <int K>
__global__ void __launch_bounds__(kPriorThreads) prior_fields_kernel(const v4u* __restrict__ slot_priors, int64_t M,
                                                                     v4u* __restrict__ priors) {
  constexpr int S = 2 * K;
  const int64_t m = (int64_t)blockIdx.x * kPriorThreads + threadIdx.x;
  if (m >= M) return;
  uint32_t w[4 * S];
#pragma unroll
  for (int j = 0; j < S; ++j) {
    const v4u x = slot_priors[m * S + j];
#pragma unroll
    for (int f = 0; f < 4; ++f) w[f * S + j] = x[f];
  }
#pragma unroll
  for (int c = 0; c < S; ++c) {
    v4u x;
#pragma unroll
    for (int d = 0; d < 4; ++d) x[d] = w[4 * c + d];
    priors[m * S + c] = x;
  }
}

__global__ void __launch_bounds__(kPriorThreads) prior_stitch_kernel(const PriorScan::Edge* __restrict__ edges,
                                                                     int64_t E, uint32_t P,
                                                                     uint32_t* __restrict__ chain,
                                                                     PriorScan::Edge* __restrict__ carry) {
  PriorScan::stitch(edges, E, P, chain, carry);
}

// What the priors pr [4][2K] of one record resolve to, as preview_kernel (matchmake.hip) sees
// the same record against a roster: the status, and on kRated p_win0 and p_outcome.
template <int K>
__device__ __forceinline__ void predict(const int32_t* r, const float* pr, const v4f* __restrict__ attrs,
                                        const float* __restrict__ vst, int64_t P, float beta2, float us,
                                        bool mode_track, uint8_t& gst, float& pw, float& po) {
  constexpr int S = 2 * K, G = split_group_lanes(K);
  const uint32_t meta0 = (uint32_t)r[S], meta1 = (uint32_t)r[S + 1];
  const int n0 = meta_n0(meta0), n1 = meta_n1(meta0);
  const uint8_t est = early_status<K>(r, P);
  int32_t id[S];
  bool inr[S];
#pragma unroll
  for (int j = 0; j < S; ++j) {
    inr[j] = (j < K ? j : j - K) < (j < K ? n0 : n1);
    id[j] = inr[j] && r[j] >= 0 && (int64_t)r[j] < P ? r[j] : -1;
  }
  float ms[S], ss[S], mm[S], sm[S];
  gst = est;
  bool failed = false;
#pragma unroll
  for (int j = 0; j < S; ++j) {
    int first = j;  // first slot carrying the same player
#pragma unroll
    for (int i = j - 1; i >= 0; --i)
      if (id[j] >= 0 && id[i] == id[j]) first = i;
    ms[j] = ss[j] = mm[j] = sm[j] = NAN;
    if (first != j) {  // a repeated player takes the priors of its first slot
#pragma unroll
      for (int i = 0; i < j; ++i) {
        if (first == i) {
          ms[j] = ms[i];
          ss[j] = ss[i];
          mm[j] = mm[i];
          sm[j] = sm[i];
        }
      }
    } else if (est == kRated && id[j] >= 0) {
      float attr[4] = {NAN, NAN, NAN, 0.f};
      if (pr[j] != pr[j] && attrs != nullptr) {  // seeding only: a NULL shared track
        const v4f a = attrs[id[j]];
        attr[0] = a[0];
        attr[1] = a[1];
        attr[2] = a[2];
      }
      uint32_t flags;
      float a = NAN, b = NAN, c = NAN, d = NAN;
      const uint8_t st = player_prior<float>(pr[j], pr[S + j], pr[2 * S + j], pr[3 * S + j], attr, us, vst, a, b, c, d,
                                             flags);
      if (st == kRated) {
        ms[j] = a;
        ss[j] = b;
        mm[j] = c;
        sm[j] = d;
      } else if (!failed) {  // the first failing slot decides
        failed = true;
        gst = st;
      }
    }
  }
  if (gst == kRated && (n0 == 0 || n1 == 0)) gst = kErrEmptyRoster;
  // d in slot order, sum sigma^2 as the butterfly: on the mode track for the quality, which
  // decides kErrNumeric as in preview, and on the chosen track for the prediction
  float d = 0.f, v[G];
  bool nonfinite = false;
#pragma unroll
  for (int i = 0; i < G; ++i) v[i] = 0.f;
#pragma unroll
  for (int i = 0; i < S; ++i) {
    if (i < K && i < n0) d += mm[i];
    if (i >= K && i - K < n1) d -= mm[i];
    if (inr[i] && id[i] >= 0) {
      v[i] = sm[i] * sm[i];
      nonfinite = nonfinite || !prior_finite<float>(ms[i], ss[i], mm[i], sm[i]);
    }
  }
  float s2 = butterfly_sum<G>(v);
  const int n = n0 + n1;
  const float q = quality_from_sums<float>(n, s2, d, beta2);
  if (!mode_track) {
    d = 0.f;
#pragma unroll
    for (int i = 0; i < G; ++i) v[i] = 0.f;
#pragma unroll
    for (int i = 0; i < S; ++i) {
      if (i < K && i < n0) d += ms[i];
      if (i >= K && i - K < n1) d -= ms[i];
      if (inr[i] && id[i] >= 0) v[i] = ss[i] * ss[i];
    }
    s2 = butterfly_sum<G>(v);
  }
  const float den = (float)n * beta2 + s2;
  pw = win_probability<float>(d, den);
  if (gst == kRated && (nonfinite || !isfinite(q) || !isfinite(pw))) gst = kErrNumeric;
  const bool w0 = meta_winner0(meta1), w1 = meta_winner1(meta1);
  po = gst == kRated && w0 != w1 ? win_probability<float>(w0 ? d : -d, den) : NAN;
  if (gst != kRated) pw = NAN;
}

template <int K>
__global__ void __launch_bounds__(kScoreThreads) score_kernel(
    const int32_t* __restrict__ rec, const float* __restrict__ priors, const uint32_t* __restrict__ rows, int64_t W,
    int64_t M, const v4f* __restrict__ attrs, const float* __restrict__ vst, int64_t P, float beta2, float us,
    int32_t track, uint32_t modes, unsigned long long* __restrict__ table, int32_t* __restrict__ pred) {
  constexpr int S = 2 * K;
  __shared__ unsigned long long part[kScoreTableWords];
  for (int c = threadIdx.x; c < kScoreTableWords; c += kScoreThreads) part[c] = 0ull;
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * kScoreThreads;
  for (int64_t m = (int64_t)blockIdx.x * kScoreThreads + threadIdx.x; m < M; m += stride) {
    int32_t r[S + 2];
    load_record<K>(rec, m, r);
    float pr[4 * S];
    const v4f* src = reinterpret_cast<const v4f*>(priors + m * (4 * S));
#pragma unroll
    for (int c = 0; c < S; ++c) {
      const v4f x = src[c];
#pragma unroll
      for (int d = 0; d < 4; ++d) pr[4 * c + d] = x[d];
    }
    const uint32_t st = rows[m * W + 5 * S + 1] & 0xffu;
    uint8_t gst;
    float pw, po;
    predict<K>(r, pr, attrs, vst, P, beta2, us, track == kScoreMode, gst, pw, po);
    const uint32_t word = score_match(st, (uint32_t)r[S], (uint32_t)r[S + 1], modes, gst, pw, po,
                                      [&](int c, int64_t x) { atomicAdd(&part[c], (unsigned long long)x); });
    if (pred != nullptr) {
      v4u o;
      o[0] = word;
      o[1] = __float_as_uint(pw);
      o[2] = __float_as_uint(po);
      o[3] = 0u;
      reinterpret_cast<v4u*>(pred)[m] = o;
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < kScoreTableWords; c += kScoreThreads)
    if (part[c] != 0ull) atomicAdd(&table[c], part[c]);
}

__global__ void __launch_bounds__(kScoreThreads) nlog2_kernel(const uint32_t* __restrict__ bits, int64_t n,
                                                               int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kScoreThreads + threadIdx.x;
  if (i < n) out[i] = nlog2_q20(bits[i]);
}

}  // namespace

int launch_nlog2_q20(const uint32_t* bits, int64_t n, int64_t* out, hipStream_t s) {
  if (n < 0 || n > 0x7fffffffll * kScoreThreads) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  hipLaunchKernelGGL(nlog2_kernel, dim3((unsigned)((n + kScoreThreads - 1) / kScoreThreads)), dim3(kScoreThreads), 0, s,
                     bits, n, out);
  return (int)hipGetLastError();
}

size_t prior_edge_bytes(int64_t n) { return PriorScan::edge_bytes(n); }

int launch_prior_keys(int K, const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t P, uint32_t* keys,
                      uint32_t* vals, uint32_t* events, uint32_t* slot_priors, hipStream_t s) {
  if (!window_slots_ok(K, W, M, P)) return (int)hipErrorInvalidValue;
  if (M == 0) return 0;
  const unsigned blocks = (unsigned)((M + kPriorThreads - 1) / kPriorThreads);
  with_team_size(K, [&](auto k) {
    hipLaunchKernelGGL(prior_keys_kernel<decltype(k)::value>, dim3(blocks), dim3(kPriorThreads), 0, s, rec,
                       reinterpret_cast<const uint32_t*>(rows), W, M, P, keys, vals, reinterpret_cast<v4u*>(events),
                       reinterpret_cast<v4u*>(slot_priors));
  });
  return (int)hipGetLastError();
}

int launch_prior_scan(const uint32_t* keys, const uint32_t* vals, const uint32_t* events, int64_t n, int K, int64_t P,
                      float* chain, void* edges, uint32_t* slot_priors, float* priors, hipStream_t s) {
  if (!sorted_slots_ok(K, n, P) || reinterpret_cast<uintptr_t>(slot_priors) % 16 != 0 ||
      reinterpret_cast<uintptr_t>(priors) % 16 != 0)
    return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  v4u* sp = reinterpret_cast<v4u*>(slot_priors);
  if (P > 0) {
    const int64_t tiles = PriorScan::tiles(n);
    PriorScan::Edge* e = static_cast<PriorScan::Edge*>(edges);
    PriorScan::Edge* carry = e + 2 * tiles;
    uint32_t* ch = reinterpret_cast<uint32_t*>(chain);
    const v4u* ev = reinterpret_cast<const v4u*>(events);
    hipLaunchKernelGGL(prior_tile_kernel<false>, dim3((unsigned)tiles), dim3(kPriorThreads), 0, s, keys, vals, ev, n,
                       (uint32_t)P, ch, e, carry, sp);
    hipLaunchKernelGGL(prior_stitch_kernel, dim3(1), dim3(kPriorThreads), 0, s, e, 2 * tiles, (uint32_t)P, ch, carry);
    hipLaunchKernelGGL(prior_tile_kernel<true>, dim3((unsigned)tiles), dim3(kPriorThreads), 0, s, keys, vals, ev, n,
                       (uint32_t)P, ch, e, carry, sp);
  }
  const int64_t M = n / (2 * K);
  const unsigned blocks = (unsigned)((M + kPriorThreads - 1) / kPriorThreads);
  with_team_size(K, [&](auto k) {
    hipLaunchKernelGGL(prior_fields_kernel<decltype(k)::value>, dim3(blocks), dim3(kPriorThreads), 0, s, sp, M,
                       reinterpret_cast<v4u*>(priors));
  });
  return (int)hipGetLastError();
}

int launch_score(int K, const int32_t* rec, const float* priors, const float* rows, int64_t W, int64_t M,
                 const float* attrs, const float* vst, int64_t P, float beta2, float unknown_sigma, int track,
                 uint32_t modes, int64_t* table, int32_t* pred, hipStream_t s) {
  if (!window_ok(K, W, M, P) || vst == nullptr ||
      table == nullptr || (track != kScoreShared && track != kScoreMode) || (modes & ~kScoreAllModes) ||
      reinterpret_cast<uintptr_t>(attrs) % 16 != 0 || reinterpret_cast<uintptr_t>(priors) % 16 != 0 ||
      reinterpret_cast<uintptr_t>(pred) % 16 != 0)
    return (int)hipErrorInvalidValue;
  if (M == 0) return 0;
  const int64_t want = (M + kScoreThreads - 1) / kScoreThreads;
  const unsigned blocks = (unsigned)(want < 2048 ? want : 2048);  // 8 workgroups per CU, then a grid stride
  with_team_size(K, [&](auto k) {
    hipLaunchKernelGGL(score_kernel<decltype(k)::value>, dim3(blocks), dim3(kScoreThreads), 0, s, rec, priors,
                       reinterpret_cast<const uint32_t*>(rows), W, M, reinterpret_cast<const v4f*>(attrs), vst, P,
                       beta2, unknown_sigma, (int32_t)track, modes, reinterpret_cast<unsigned long long*>(table),
                       pred);
  });
  return (int)hipGetLastError();
}

}  // namespace ana
