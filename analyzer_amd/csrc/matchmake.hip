// K12 matchmaking: questions about the match not yet played, answered from the roster alone
// (read-only; tag words are never looked at).
//
//   preview   per stream record: the status and quality `rate` would write, and team 0's win
//             probability
//   balance   per lobby of 2K players: the split into two teams of K with the smallest |d|
//             (matchmake_core.h), as a ready-to-rate stream record
//   queue_keys  per queue entry the sort key of its mode-track prior mu; launch_radix_sort_pairs
//             then orders the queue best first
//
// preview and balance give a match to a group of G = split_group_lanes(K) lanes (8 for
// K <= 3, 16 for K = 4, 5): lane j holds slot j.  Its id comes from one coalesced load of the
// record, its priors from two 16-B loads of the player's 128-B roster line (shared granule
// and mode granule; the attrs float4 only behind a NULL shared track), and the output
// record leaves as one word per lane.  The 2K mode-track mus are then broadcast to every lane
// of the group; lane l evaluates the splits [l * SPL, (l + 1) * SPL) from masks it loaded once
// (a 16-B row of a constant table), and the (|d| bits, index) argmin is log2(G) exchange steps
// inside the group.  Errors are collected with wave ballots masked to the group, so an error
// lobby changes nothing for its neighbours.  No LDS, no atomics, plain vector stores.  The
// file is built with -ffp-contract=off: every fp32 operation is the one written, which is
// what makes the split choice equal the host mirror's.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "common.h"
#include "kernels.h"
#include "matchmake_core.h"

namespace ana {

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef uint32_t v4u __attribute__((ext_vector_type(4)));

// lane-major split masks: row [K - 1][lane] = the lane's split_per_lane(K) masks, 0 = none
struct LaneMasks {
  uint16_t m[kSplitMaxK][16][8];
};

template <int K>
constexpr void fill_lane_masks(LaneMasks& t) {
  constexpr int G = split_group_lanes(K), SPL = split_per_lane(K), C = split_count(K);
  static_assert(SPL <= 8 && G <= 16 && G >= 2 * K + 2 && G * SPL >= C, "a lane's masks fit one 16-B row");
  for (int l = 0; l < G; ++l)
    for (int s = 0; s < SPL; ++s)
      if (l * SPL + s < C) t.m[K - 1][l][s] = kSplits<K>.mask[l * SPL + s];
}

constexpr LaneMasks make_lane_masks() {
  LaneMasks t{};
  fill_lane_masks<1>(t);
  fill_lane_masks<2>(t);
  fill_lane_masks<3>(t);
  fill_lane_masks<4>(t);
  fill_lane_masks<5>(t);
  return t;
}

__constant__ __attribute__((aligned(16))) LaneMasks kLaneMasks = make_lane_masks();

struct Prior {
  float ms, ss, mm, sm;
  uint8_t st;
};

// player_prior (rate_core.h) of one player from its roster line; own = false loads nothing
__device__ __forceinline__ Prior load_prior(const v4f* __restrict__ state, const v4f* __restrict__ attrs,
                                            const float* __restrict__ vst, float us, int32_t id, bool own,
                                            int mode) {
  Prior p{NAN, NAN, NAN, NAN, (uint8_t)kRated};
  if (own) {
    const v4f gs = state[(int64_t)id * kGranules];
    const v4f gm = state[(int64_t)id * kGranules + 1 + mode];
    float attr[4] = {NAN, NAN, NAN, 0.f};
    if (gs[0] != gs[0] && attrs != nullptr) {  // seeding only: a NULL shared track
      const v4f a = attrs[id];
      attr[0] = a[0];
      attr[1] = a[1];
      attr[2] = a[2];
    }
    uint32_t flags;
    float ms = NAN, ss = NAN, mm = NAN, sm = NAN;
    p.st = player_prior<float>(gs[0], gs[2], gm[0], gm[2], attr, us, vst, ms, ss, mm, sm, flags);
    if (p.st == kRated) {
      p.ms = ms;
      p.ss = ss;
      p.mm = mm;
      p.sm = sm;
    }
  }
  return p;
}

template <int G>
__device__ __forceinline__ uint64_t group_mask(int gbase) {
  return ((1ull << G) - 1ull) << gbase;
}

template <int K>
__global__ void __launch_bounds__(kMatchmakeThreads) preview_kernel(
    const int32_t* __restrict__ rec, int64_t M, const v4f* __restrict__ state, const v4f* __restrict__ attrs,
    const float* __restrict__ vst, int64_t P, float beta2, float us, int32_t* __restrict__ out) {
  constexpr int S = 2 * K, G = split_group_lanes(K), LPW = 64 / G;
  const int lane = threadIdx.x & 63, j = lane & (G - 1), gbase = lane - j;
  const uint64_t gmask = group_mask<G>(gbase);
  const int64_t wave = ((int64_t)blockIdx.x * kMatchmakeThreads + threadIdx.x) >> 6;
  const int64_t nwaves = (int64_t)gridDim.x * (kMatchmakeThreads / 64);
  for (int64_t m0 = wave * LPW; m0 < M; m0 += nwaves * LPW) {  // wave-uniform trip count
    const int64_t m = m0 + gbase / G;
    const bool act = m < M;
    const int32_t word = act && j < S + 2 ? rec[m * (S + 2) + j] : 0;
    const uint32_t meta0 = (uint32_t)__shfl(word, gbase + S), meta1 = (uint32_t)__shfl(word, gbase + S + 1);
    const int mode = meta_mode(meta0), n0 = meta_n0(meta0), n1 = meta_n1(meta0);
    // decode_record's precedence (rate_core.h)
    const bool inr = act && j < S && (j < K ? j : j - K) < (j < K ? n0 : n1);
    const bool idok = word >= 0 && (int64_t)word < P;
    const bool bad = (__ballot(inr && !idok) & gmask) != 0ull || n0 > K || n1 > K;
    const uint8_t est = mode >= kModes ? kUnsupportedMode
                        : bad ? kErrBadRecord
                        : meta_nrosters(meta0) != 2 ? kInvalidRosters
                        : meta_afk(meta1) ? kAfk : kRated;
    const int32_t id = inr && idok ? word : -1;
    int first = j;  // first slot carrying the same player
#pragma unroll
    for (int i = 0; i < S; ++i) {
      const int32_t o = __shfl(id, gbase + i);
      if (i < j && id >= 0 && o == id && first == j) first = i;
    }
    const Prior p = load_prior(state, attrs, vst, us, id, est == kRated && id >= 0 && first == j, mode);
    // the first failing slot decides, as the sequential prior loop of rate does
    const uint64_t eb = __ballot(p.st != kRated) & gmask;
    uint8_t gst = est;
    const int bad_lane = eb ? (int)__builtin_ctzll(eb) : gbase;
    const uint8_t first_bad = (uint8_t)__shfl((int)p.st, bad_lane);
    if (est == kRated && eb) gst = first_bad;
    // a repeated player takes the priors of its first slot (copy_dup_priors)
    const float ms = __shfl(p.ms, gbase + first), ss = __shfl(p.ss, gbase + first);
    const float mm = __shfl(p.mm, gbase + first), sm = __shfl(p.sm, gbase + first);
    if (gst == kRated && (n0 == 0 || n1 == 0)) gst = kErrEmptyRoster;
    // match_quality's sums on the mode track: d in slot order, sum sigma^2 as a butterfly
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < S; ++i) {
      const float mu = __shfl(mm, gbase + i);
      if (i < K && i < n0) d += mu;
      if (i >= K && i - K < n1) d -= mu;
    }
    float s2 = inr && id >= 0 ? sm * sm : 0.f;
#pragma unroll
    for (int o = 1; o < G; o <<= 1) s2 += __shfl_xor(s2, o);
    const bool nonfinite = inr && id >= 0 && !prior_finite<float>(ms, ss, mm, sm);
    const bool gnonfinite = (__ballot(nonfinite) & gmask) != 0ull;
    const int n = n0 + n1;
    const float q = quality_from_sums<float>(n, s2, d, beta2);
    const float pw = win_probability<float>(d, (float)n * beta2 + s2);
    if (gst == kRated && (gnonfinite || !isfinite(q) || !isfinite(pw))) gst = kErrNumeric;
    const float qo = gst == kRated ? q : (gst == kAfk || gst == kInvalidRosters) ? 0.f : NAN;
    const float po = gst == kRated ? pw : NAN;
    const uint32_t w = j == 0 ? (uint32_t)gst : j == 1 ? __float_as_uint(qo) : j == 2 ? __float_as_uint(po) : 0u;
    if (act && j < kPreviewWords) out[m * kPreviewWords + j] = (int32_t)w;
  }
}

template <int K>
__global__ void __launch_bounds__(kMatchmakeThreads) balance_kernel(
    const int32_t* __restrict__ lobbies, int64_t L, const v4f* __restrict__ state,
    const v4f* __restrict__ attrs, const float* __restrict__ vst, int64_t P, int mode, float beta2, float us,
    int32_t* __restrict__ out, int32_t* __restrict__ records) {
  constexpr int S = 2 * K, G = split_group_lanes(K), SPL = split_per_lane(K), LPW = 64 / G;
  const int lane = threadIdx.x & 63, j = lane & (G - 1), gbase = lane - j;
  const uint64_t gmask = group_mask<G>(gbase);
  // this lane's splits, for every lobby it sees
  const v4u row = *reinterpret_cast<const v4u*>(&kLaneMasks.m[K - 1][j][0]);
  uint32_t msk[SPL];
#pragma unroll
  for (int s = 0; s < SPL; ++s) msk[s] = (row[s / 2] >> (16 * (s & 1))) & 0xffffu;
  const uint32_t meta0 = pack_meta0(mode, K, K, 2);
  const int64_t wave = ((int64_t)blockIdx.x * kMatchmakeThreads + threadIdx.x) >> 6;
  const int64_t nwaves = (int64_t)gridDim.x * (kMatchmakeThreads / 64);
  for (int64_t l0 = wave * LPW; l0 < L; l0 += nwaves * LPW) {  // wave-uniform trip count
    const int64_t l = l0 + gbase / G;
    const bool inr = l < L && j < S;
    const int32_t id = inr ? lobbies[l * S + j] : -1;
    bool badl = inr && (id < 0 || (int64_t)id >= P);
#pragma unroll
    for (int i = 0; i < S; ++i) {
      const int32_t o = __shfl(id, gbase + i);
      if (i < j && inr && o == id) badl = true;  // a player in two slots
    }
    const bool gbad = (__ballot(badl) & gmask) != 0ull;
    const Prior p = load_prior(state, attrs, vst, us, id, inr && !gbad, mode);
    const bool e_seed = (__ballot(p.st == kErrSeed) & gmask) != 0ull;
    const bool e_sigma = (__ballot(p.st == kErrSigma) & gmask) != 0ull;
    const bool nonfinite = inr && !prior_finite<float>(p.ms, p.ss, p.mm, p.sm);
    float mu[S];
#pragma unroll
    for (int i = 0; i < S; ++i) mu[i] = __shfl(p.mm, gbase + i);
    float s2 = inr ? p.sm * p.sm : 0.f;
#pragma unroll
    for (int o = 1; o < G; o <<= 1) s2 += __shfl_xor(s2, o);
    // the lane's best (|d| bits, index << 16 | mask): ascending index, strict <
    uint32_t bb = 0xffffffffu, bp = 0xffffffffu;
    bool dbad = false;
#pragma unroll
    for (int s = 0; s < SPL; ++s) {
      // opaque to the optimiser: the 2K - 1 sign words of a mask are recomputed per lobby (two
      // integer operations each) instead of living in 8 x 9 registers across the loop
      uint32_t mk = msk[s];
      asm volatile("" : "+v"(mk));
      const float d = split_d<K>(mu, mk);
      const uint32_t bits = mk ? split_abs_bits(d) : 0xffffffffu;
      const uint32_t pay = mk ? ((uint32_t)(j * SPL + s) << 16) | mk : 0xffffffffu;
      dbad = dbad || (mk && !isfinite(d));
      if (bits < bb) {
        bb = bits;
        bp = pay;
      }
    }
#pragma unroll
    for (int o = 1; o < G; o <<= 1) {
      const uint32_t ob = (uint32_t)__shfl_xor((int)bb, o), op = (uint32_t)__shfl_xor((int)bp, o);
      if (split_better(ob, op, bb, bp)) {
        bb = ob;
        bp = op;
      }
    }
    const bool e_num = (__ballot(nonfinite || dbad) & gmask) != 0ull;
    const uint32_t mask = bp & 0xffffu, idx = bp >> 16;
    const float den = (float)S * beta2 + s2;
    const float db = split_d<K>(mu, mask), dg = split_d<K>(mu, (1u << K) - 1u);
    const float q = quality_from_sums<float>(S, s2, db, beta2), qg = quality_from_sums<float>(S, s2, dg, beta2);
    const float pw = win_probability<float>(db, den);
    const uint8_t st = gbad ? kErrBadRecord
                       : e_seed ? kErrSeed
                       : e_sigma ? kErrSigma
                       : (e_num || !isfinite(q) || !isfinite(qg) || !isfinite(pw)) ? kErrNumeric : kRated;
    const bool ok = st == kRated;
    const uint32_t w = j == 0 ? (uint32_t)st
                       : j == 1 ? (ok ? idx : 0xffffffffu)
                       : j == 2 ? (ok ? mask : 0u)
                       : j == 3 ? __float_as_uint(ok ? q : NAN)
                       : j == 4 ? __float_as_uint(ok ? pw : NAN)
                       : j == 5 ? __float_as_uint(ok ? qg : NAN) : 0u;
    if (l < L && j < kBalanceWords) out[l * kBalanceWords + j] = (int32_t)w;
    if (l < L && j < S + 2) {
      const int pos = j < S ? (ok ? split_position(mask, j, K) : j) : j;
      records[l * (S + 2) + pos] = j < S ? id : j == S ? (int32_t)meta0 : 0;
    }
  }
}

__global__ void __launch_bounds__(kMatchmakeThreads) queue_keys_kernel(
    const int32_t* __restrict__ queue, int64_t Q, const v4f* __restrict__ state, const v4f* __restrict__ attrs,
    const float* __restrict__ vst, int64_t P, int mode, float us, uint32_t* __restrict__ keys,
    uint32_t* __restrict__ vals) {
  const int64_t i = (int64_t)blockIdx.x * kMatchmakeThreads + threadIdx.x;
  if (i >= Q) return;
  const int32_t id = queue[i];
  const bool idok = id >= 0 && (int64_t)id < P;
  const Prior p = load_prior(state, attrs, vst, us, id, idok, mode);
  keys[i] = idok ? queue_key(p.st, p.mm) : kLadderUnranked;
  vals[i] = (uint32_t)i;
}

bool bad_roster_args(const float* state, const float* attrs, const float* vst, int64_t P) {
  return P < 0 || P > 0x7fffffffll || vst == nullptr || (P > 0 && state == nullptr) ||
         reinterpret_cast<uintptr_t>(state) % 16 != 0 || reinterpret_cast<uintptr_t>(attrs) % 16 != 0;
}

unsigned grid_for(int64_t items, int per_block) {
  const int64_t blocks = (items + per_block - 1) / per_block;
  return (unsigned)(blocks < 2048 ? blocks : 2048);  // 8 workgroups per CU, then a grid stride
}

template <int K>
int preview_k(const int32_t* rec, int64_t M, const float* state, const float* attrs, const float* vst, int64_t P,
              float beta2, float us, int32_t* out, hipStream_t s) {
  hipLaunchKernelGGL(preview_kernel<K>, dim3(grid_for(M, kMatchmakeThreads / split_group_lanes(K))),
                     dim3(kMatchmakeThreads), 0, s, rec, M, reinterpret_cast<const v4f*>(state),
                     reinterpret_cast<const v4f*>(attrs), vst, P, beta2, us, out);
  return (int)hipGetLastError();
}

template <int K>
int balance_k(const int32_t* lobbies, int64_t L, const float* state, const float* attrs, const float* vst,
              int64_t P, int mode, float beta2, float us, int32_t* out, int32_t* records, hipStream_t s) {
  hipLaunchKernelGGL(balance_kernel<K>, dim3(grid_for(L, kMatchmakeThreads / split_group_lanes(K))),
                     dim3(kMatchmakeThreads), 0, s, lobbies, L, reinterpret_cast<const v4f*>(state),
                     reinterpret_cast<const v4f*>(attrs), vst, P, mode, beta2, us, out, records);
  return (int)hipGetLastError();
}

}  // namespace

int launch_preview(int K, const int32_t* rec, int64_t M, const float* state, const float* attrs, const float* vst,
                   int64_t P, float beta2, float unknown_sigma, int32_t* out, hipStream_t s) {
  if (K < 1 || K > kSplitMaxK || M < 0 || bad_roster_args(state, attrs, vst, P) || (M > 0 && (!rec || !out)))
    return (int)hipErrorInvalidValue;
  if (M == 0) return 0;
  int rc = (int)hipErrorInvalidValue;
  with_team_size(K, [&](auto k) {
    rc = preview_k<decltype(k)::value>(rec, M, state, attrs, vst, P, beta2, unknown_sigma, out, s);
  });
  return rc;
}

int launch_balance(int K, const int32_t* lobbies, int64_t L, const float* state, const float* attrs,
                   const float* vst, int64_t P, int mode, float beta2, float unknown_sigma, int32_t* out,
                   int32_t* records, hipStream_t s) {
  if (K < 1 || K > kSplitMaxK || L < 0 || mode < 0 || mode >= kModes || bad_roster_args(state, attrs, vst, P) ||
      (L > 0 && (!lobbies || !out || !records)))
    return (int)hipErrorInvalidValue;
  if (L == 0) return 0;
  int rc = (int)hipErrorInvalidValue;
  with_team_size(K, [&](auto k) {
    rc = balance_k<decltype(k)::value>(lobbies, L, state, attrs, vst, P, mode, beta2, unknown_sigma, out, records, s);
  });
  return rc;
}

int launch_queue_keys(const int32_t* queue, int64_t Q, const float* state, const float* attrs, const float* vst,
                      int64_t P, int mode, float unknown_sigma, uint32_t* keys, uint32_t* vals, hipStream_t s) {
  if (Q < 0 || Q > 0x7fffffffll || mode < 0 || mode >= kModes || bad_roster_args(state, attrs, vst, P) ||
      (Q > 0 && (!queue || !keys || !vals)))
    return (int)hipErrorInvalidValue;
  if (Q == 0) return 0;
  const int64_t blocks = (Q + kMatchmakeThreads - 1) / kMatchmakeThreads;
  hipLaunchKernelGGL(queue_keys_kernel, dim3((unsigned)blocks), dim3(kMatchmakeThreads), 0, s, queue, Q,
                     reinterpret_cast<const v4f*>(state), reinterpret_cast<const v4f*>(attrs), vst, P, mode,
                     unknown_sigma, keys, vals);
  return (int)hipGetLastError();
}

}  // namespace ana
