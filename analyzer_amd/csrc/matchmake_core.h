// K12 matchmaking: the split enumeration of a lobby, the balance criterion, the win
// probability and the queue key, shared by the device kernels (matchmake.hip) and the host
// mirror (host.cpp) so both choose the same split, bit for bit.
//
// A lobby has S = 2K slots (K = 1..5).  A split is a K-subset T of the slots that contains
// slot 0 (T is team 0), written as a bit mask (bit j = slot j is in team 0); splits are
// ordered by ascending mask value and there are C(2K-1, K-1) of them: 1, 3, 10, 35, 126.
// Index 0 is (1 << K) - 1: the lobby as given, first K slots against the last K.
//
// Every split of one lobby has the same n and the same sum of sigma^2, so the quality
// (rate_core.h quality_from_sums) is strictly decreasing in |d| and the best split is the one
// with the smallest |d|.  d is the fp32 sum over the slots in ascending slot order of
// (in T ? mu_j : -mu_j), starting from the slot-0 term: additions and exact sign flips only,
// nothing an FMA could absorb.  The comparison is on the bits of |d| with strict <, so a tie
// (+d and -d tie) keeps the lower index: the choice is a pure function of the inputs.
//
// p_win0 = Phi(d / sqrt(n beta^2 + sum sigma_j^2)) on the mode track, sigma without tau:
// the (d, den) of match_quality, so quality and p_win0 describe the same belief.
#pragma once

#include <math.h>
#include <stdint.h>

#include "common.h"
#include "ladder_core.h"
#include "rate_core.h"

namespace ana {

constexpr int kSplitMaxK = kMaxTeamSize;
constexpr int kPreviewWords = 4;  // packed preview row: status, quality, p_win0, 0
constexpr int kBalanceWords = 8;  // packed balance row: status, split, team0, quality, p_win0, quality_given, 0, 0

// C(2K-1, K-1)
constexpr int split_count(int K) {
  int c = 1;
  for (int i = 1; i < K; ++i) c = c * (K + i) / i;
  return c;
}

constexpr int split_popcount(uint32_t m) {
  int n = 0;
  for (; m; m &= m - 1u) ++n;
  return n;
}

template <int K>
struct SplitTable {
  static constexpr int C = split_count(K);
  uint16_t mask[C];
};

template <int K>
constexpr SplitTable<K> make_split_table() {
  SplitTable<K> t{};
  int n = 0;
  for (uint32_t m = 1u; m < (1u << (2 * K)); m += 2u)  // odd masks: slot 0 is in team 0
    if (split_popcount(m) == K) t.mask[n++] = (uint16_t)m;
  return t;
}

template <int K>
inline constexpr SplitTable<K> kSplits = make_split_table<K>();

static_assert(split_count(1) == 1 && split_count(2) == 3 && split_count(3) == 10 && split_count(4) == 35 &&
                  split_count(5) == 126, "C(2K-1, K-1)");
static_assert(kSplits<1>.mask[0] == 1 && kSplits<2>.mask[0] == 3 && kSplits<3>.mask[0] == 7 &&
                  kSplits<4>.mask[0] == 15 && kSplits<5>.mask[0] == 31, "split 0 is the lobby as given");
static_assert(kSplits<2>.mask[2] == 9 && kSplits<5>.mask[125] == 0x3c1, "ascending mask order");

// Device geometry: the lanes that share one lobby (a power of two >= 2K + 2, so that a lane
// per word loads a stream record and stores the output record) and the splits each of them
// evaluates; lane l owns the indices [l * split_per_lane, (l + 1) * split_per_lane).
constexpr int split_group_lanes(int K) { return K <= 3 ? 8 : 16; }
constexpr int split_per_lane(int K) { return (split_count(K) + split_group_lanes(K) - 1) / split_group_lanes(K); }
constexpr int kMatchmakeThreads = 256;  // lanes per workgroup

template <int K>
ANA_HD float split_d(const float (&mu)[2 * K], uint32_t mask) {
  // -mu_j as a flip of the sign bit: integer operations instead of a select per term
  const uint32_t out = ~mask;
  float d = mu[0];
#pragma unroll
  for (int j = 1; j < 2 * K; ++j) d += ladder_float(ladder_bits(mu[j]) ^ ((out << (31 - j)) & 0x80000000u));
  return d;
}

ANA_HD uint32_t split_abs_bits(float d) { return ladder_bits(d) & 0x7fffffffu; }

// (|d| bits, index) of a candidate against the best so far
ANA_HD bool split_better(uint32_t bits, uint32_t idx, uint32_t best_bits, uint32_t best_idx) {
  return bits < best_bits || (bits == best_bits && idx < best_idx);
}

// position of slot j in the output record: team 0's players in ascending slot order, then team 1's
ANA_HD int split_position(uint32_t mask, int j, int K) {
  const uint32_t below = (1u << j) - 1u;
  return ((mask >> j) & 1u) ? __builtin_popcount(mask & below) : K + __builtin_popcount(~mask & below);
}

template <typename T>
ANA_HD T win_probability(T d, T den) {
  const T t = d / sqrt(den);
  return (T)0.5 * erfc(-t * (T)0.70710678118654752);
}

// queue order: descending mode-track prior mu (-0 read as +0), failed players last
ANA_HD uint32_t queue_key(uint8_t st, float mm) {
  const float s = mm + 0.0f;
  return st == kRated && s == s ? ladder_score_key(s) : kLadderUnranked;
}

template <typename T>
ANA_HD bool prior_finite(T ms, T ss, T mm, T sm) {
  return isfinite(ms) && isfinite(ss) && isfinite(mm) && isfinite(sm);
}

}  // namespace ana
