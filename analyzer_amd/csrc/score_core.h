// K14 scorecard: the pre-match priors of a window, the prediction they give and the integer
// score of that prediction, shared by the device kernels (score.hip) and the host mirror
// (host.cpp) so both produce the same bits.
//
// Priors.  The chain table chain [P][kBaseFloats] holds (mu, sigma) per granule (the base-row
// layout of sweep_core.h; NaN mu = NULL).  A slot j of a match is *live* when it is occupied
// (its position within its team < n0 / n1), its id lies in [0, P) and the match's mode is
// < kModes.  A live slot *writes* when the row's status byte is kRated and the same player
// occupies no later slot of the record (later writes win): the shared granule becomes the
// slot's (s_mu, s_sig), the mode granule its (m_mu, m_sig), copied bit for bit.  The prior of
// a live slot is the chain state of its player before its match -- every slot of one match,
// twins included, sees the state before that match -- as four raw words: shared (mu, sigma),
// mode track (mu, sigma).  No seeding, no fallback; a slot that is not live gets four NaNs.
//
// PriorState is what a stretch of one player's slots leaves behind: per track the last write,
// if any.  prior_combine(a, b) (a earlier) takes b's track where b has it, else a's: it is
// associative with prior_none() as its identity and copies bits, so a chain is the same bits
// however the slots are cut into stretches.
//
// Scorecard.  table [kModes][kScoreBins + 1][4] int64, every word an integer sum:
//   bin row b (b = min(kScoreBins - 1, (int)(p_win0 * kScoreBins))) of the match's mode:
//     [n, team0_wins, sum rint(p_win0 * 2^24), spare]
//   the spare word of bin row kSpareInconsistent counts the mode's inconsistent matches, that
//   of bin row kSpareCoin its scored matches with p_outcome == 0.5; the other spares stay 0
//   last row: [sum rint((p_win0 - y)^2 * 2^24), sum nlog2_q20(p_outcome), favourite_won, ties]
// with y = 1 when roster 0 won.  A match counts when its row status is kRated and its mode has
// its bit in the modes mask.  Of those, a match whose priors do not resolve to kRated with a
// finite prediction is *inconsistent* (the chain did not start from the roster the history
// started from); a match without a winner bit is a tie; a match with exactly one winner bit
// is *scored*.  The squared error is formed in fp64 from the fp32 p_win0: e = (double)p - y,
// rint(e * e * 2^24), each operation IEEE, so a host of any kind reproduces it.
//
// nlog2_q20(bits) = -log2(p) * 2^20 for an fp32 p in (0, 1], integer operations only: the
// exponent field gives the integer part, and 20 steps of square-and-compare on the mantissa
// x in [1, 2), held with 31 fraction bits, give the 20 fraction bits N of log2(x), so the
// result is (127 - E) * 2^20 - N.  Every step truncates x downwards by a relative error
// below 2^-31, which after 20 doublings is below 2^-11 / ln 2 units of 2^-20, so against the
// real number T = -log2(p) * 2^20 the result R satisfies 0 <= R - T < 1 + 2^-10 (the analytic
// bound, 1.00098); over 4,096 random patterns in (0, 1] the largest R - T measured against a
// 50-digit -log2 is 1.00015 units and the smallest 0.00077 (tests/test_scorecard.py).  p = 0 and
// denormals give kNlog2Cap; p >= 1 gives 0.
#pragma once

#include <math.h>
#include <stdint.h>

#include "common.h"
#include "ladder_core.h"
#include "matchmake_core.h"
#include "rate_core.h"

namespace ana {

constexpr int kScoreBins = 32;
constexpr int kScoreRowWords = 4;
constexpr int kScoreModeWords = (kScoreBins + 1) * kScoreRowWords;
constexpr int kScoreTableWords = kModes * kScoreModeWords;
constexpr int kSpareInconsistent = 0;  // bin row whose spare word counts inconsistent matches
constexpr int kSpareCoin = 1;          // bin row whose spare word counts p_outcome == 0.5
constexpr uint32_t kScoreAllModes = (1u << kModes) - 1u;
constexpr int64_t kNlog2Cap = (int64_t)150 << 20;  // above -log2 of every normal fp32

enum ScoreTrack : int32_t {
  kScoreShared = 0,  // d and sum sigma^2 on the shared track
  kScoreMode = 1,    // on the match's mode track, as quality and preview_matches
};

// pred row [kPredWords] int32: flags word, p_win0 bits, p_outcome bits, 0.
// flags word: resolved status | mode << 8 | bin << 16 | flag bits << 24
constexpr int kPredWords = 4;
constexpr uint32_t kPredScored = 1u << 24;
constexpr uint32_t kPredTie = 1u << 25;
constexpr uint32_t kPredInconsistent = 1u << 26;
constexpr uint32_t kPredCoin = 1u << 27;
constexpr uint32_t kPredTeam0Won = 1u << 28;

// sort value of a slot: the slot index, its match's mode and the write flag
constexpr int kPriorModeShift = kSlotBits;
constexpr uint32_t kPriorWriteBit = 1u << 31;
constexpr uint32_t kPriorSlotMask = (1u << kSlotBits) - 1u;
constexpr int kPriorEventWords = 4;  // (s_mu, s_sig, m_mu, m_sig) bits of a writing slot
constexpr uint32_t kPriorNull = 0x7fc00000u;
static_assert(kModes <= 8 && kSlotBits + 4 == 32, "mode and write flag ride above the slot index");

// bit j set: slot j of the record is live
template <int K>
ANA_HD uint32_t prior_live_mask(const int32_t* r, int64_t P) {
  constexpr int S = 2 * K;
  const uint32_t m0 = (uint32_t)r[S];
  if (meta_mode(m0) >= kModes) return 0u;
  const int n0 = meta_n0(m0), n1 = meta_n1(m0);
  uint32_t mask = 0u;
#pragma unroll
  for (int j = 0; j < S; ++j) {
    const int pos = j < K ? j : j - K;
    const int32_t p = r[j];
    if (pos < (j < K ? n0 : n1) && p >= 0 && (int64_t)p < P) mask |= 1u << j;
  }
  return mask;
}

// of the live slots, those whose write is seen: no later live slot carries the same player
template <int K>
ANA_HD uint32_t prior_last_mask(const int32_t* r, uint32_t live) {
  constexpr int S = 2 * K;
  uint32_t last = live;
#pragma unroll
  for (int j = 1; j < S; ++j) {
#pragma unroll
    for (int i = 0; i < j; ++i)
      if (((live >> j) & 1u) && ((live >> i) & 1u) && r[i] == r[j]) last &= ~(1u << i);
  }
  return last;
}

struct PriorState {
  uint32_t mask;             // bit t: track t was written
  uint32_t w[2 * kTracks];   // (mu, sigma) bits per track
};

ANA_HD PriorState prior_none() {
  PriorState s;
  s.mask = 0u;
#pragma unroll
  for (int i = 0; i < 2 * kTracks; ++i) s.w[i] = kPriorNull;
  return s;
}

// a then b
ANA_HD PriorState prior_combine(const PriorState& a, const PriorState& b) {
  PriorState c;
  c.mask = a.mask | b.mask;
#pragma unroll
  for (int t = 0; t < kTracks; ++t) {
    const bool hb = (b.mask >> t) & 1u;
    c.w[2 * t] = hb ? b.w[2 * t] : a.w[2 * t];
    c.w[2 * t + 1] = hb ? b.w[2 * t + 1] : a.w[2 * t + 1];
  }
  return c;
}

// the write of a slot on mode 0..5 with event (s_mu, s_sig, m_mu, m_sig)
ANA_HD PriorState prior_write(int mode, uint32_t e0, uint32_t e1, uint32_t e2, uint32_t e3) {
  PriorState s = prior_none();
  s.mask = 1u | (2u << mode);
  s.w[0] = e0;
  s.w[1] = e1;
#pragma unroll
  for (int t = 1; t < kTracks; ++t) {  // compile-time indices only
    if (t == 1 + mode) {
      s.w[2 * t] = e2;
      s.w[2 * t + 1] = e3;
    }
  }
  return s;
}

// a player's chain row as a state with every track present
ANA_HD PriorState prior_from_chain(const uint32_t* row) {
  PriorState s;
  s.mask = (1u << kTracks) - 1u;
#pragma unroll
  for (int i = 0; i < 2 * kTracks; ++i) s.w[i] = row[i];
  return s;
}

// the four prior words of a slot on mode 0..5 from the state before its match
ANA_HD void prior_pick(const PriorState& s, int mode, uint32_t* out) {
  out[0] = s.w[0];
  out[1] = s.w[1];
  out[2] = out[3] = kPriorNull;
#pragma unroll
  for (int t = 1; t < kTracks; ++t) {
    if (t == 1 + mode) {
      out[2] = s.w[2 * t];
      out[3] = s.w[2 * t + 1];
    }
  }
}

ANA_HD int64_t nlog2_q20(uint32_t bits) {
  const uint32_t e = bits >> 23;
  if (bits >= 0x3f800000u) return 0;  // p >= 1 (and what is no probability)
  if (e == 0u) return kNlog2Cap;      // 0 and denormals
  uint64_t x = (uint64_t)(0x800000u | (bits & 0x7fffffu)) << 8;  // [2^31, 2^32)
  uint32_t n = 0u;
#pragma unroll
  for (int k = 0; k < 20; ++k) {
    const uint64_t y = x * x;  // [2^62, 2^64)
    const bool two = (y >> 63) != 0ull;
    n = (n << 1) | (two ? 1u : 0u);
    x = two ? y >> 32 : y >> 31;
  }
  return (((int64_t)127 - (int64_t)e) << 20) - (int64_t)n;
}

ANA_HD int score_bin(float p) {
  const int b = (int)(p * (float)kScoreBins);
  return b < kScoreBins - 1 ? b : kScoreBins - 1;
}

// rint(p * 2^24): the product is exact
ANA_HD int64_t score_p_term(float p) { return (int64_t)rintf(p * 16777216.0f); }

ANA_HD int64_t score_brier_term(float p, bool team0_won) {
  const double e = (double)p - (team0_won ? 1.0 : 0.0);
  return (int64_t)rint(e * e * 16777216.0);
}

// What one match adds to its mode's part of the table.  st: the row's status byte; gst, pw,
// po: the status, p_win0 and p_outcome its priors resolve to.  Returns the pred flags word
// and calls add(word index within the table, amount) for every sum that moves.
template <class Add>
ANA_HD uint32_t score_match(uint32_t st, uint32_t meta0, uint32_t meta1, uint32_t modes, uint8_t gst, float pw,
                            float po, Add&& add) {
  const int mode = meta_mode(meta0);
  uint32_t word = (uint32_t)gst | ((uint32_t)(mode & 0xff) << 8);
  const bool ok = gst == kRated && isfinite(pw);  // po is a NaN without a single winner
  int bin = 0;
  if (ok) {
    bin = score_bin(pw);
    word |= (uint32_t)bin << 16;
  }
  const bool w0 = meta_winner0(meta1), w1 = meta_winner1(meta1);
  if (w0 && !w1) word |= kPredTeam0Won;
  if (st != kRated || mode >= kModes || !((modes >> mode) & 1u)) return word;
  const int base = mode * kScoreModeWords, tail = base + kScoreBins * kScoreRowWords;
  if (!ok) {
    add(base + kSpareInconsistent * kScoreRowWords + 3, (int64_t)1);
    return word | kPredInconsistent;
  }
  if (!w0 && !w1) {
    add(tail + 3, (int64_t)1);
    return word | kPredTie;
  }
  if (w0 && w1) return word;
  const int row = base + bin * kScoreRowWords;
  add(row + 0, (int64_t)1);
  if (w0) add(row + 1, (int64_t)1);
  add(row + 2, score_p_term(pw));
  add(tail + 0, score_brier_term(pw, w0));
  add(tail + 1, nlog2_q20(ladder_bits(po)));
  if (po > 0.5f) add(tail + 2, (int64_t)1);
  word |= kPredScored;
  if (po == 0.5f) {
    add(base + kSpareCoin * kScoreRowWords + 3, (int64_t)1);
    word |= kPredCoin;
  }
  return word;
}

// the sum the lanes of a preview group form with an xor butterfly over G lanes, in one lane:
// ((v0 + v1) + (v2 + v3)) + ...; fp32 addition commutes, so every lane of the butterfly holds
// these bits
template <int G>
ANA_HD float butterfly_sum(float (&v)[G]) {
#pragma unroll
  for (int o = 1; o < G; o <<= 1) {
#pragma unroll
    for (int i = 0; i < G; i += 2 * o) v[i] = v[i] + v[i + o];
  }
  return v[0];
}

}  // namespace ana
