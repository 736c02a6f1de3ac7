// K19 expectations: every player's predicted against actual results -- what a game is, the
// per-game terms, the player row and the run summary -- shared by the device kernels
// (expect.hip) and the host mirror (host.cpp) so both produce the same bits.
//
// The inputs of a window are rec [M][2K+2], the raw priors [M][4][2K] of K14 (field-major:
// shared mu, sigma, mode mu, sigma) and the pred rows [M][kPredWords] of score_add: flags word,
// p_win0 bits, p_outcome bits.  Everything here is an integer function of those words; nothing
// is recomputed from a roster.
//
// Game.  A slot j of match m is a game when pred[m].flags has kPredScored (the row is rated, its
// mode is in the card's mask, exactly one roster won, the priors resolved), p_win0 lies in
// [0, 1] (score_add writes no other p_win0 into a scored row; a row made by hand with one
// holds no game) and the slot is live by prior_live_mask.  Twins are two games: everything goes
// slot by slot.  A game is won when its own roster carries its winner bit (profile_won).
//
// Terms of a game.  P24 = score_p_term(p_win0) = rint(p * 2^24); q24 = P24 for a slot of
// roster 0, 2^24 - P24 for one of roster 1 (an integer complement).
//   exp += q24                          var += (q24 * (2^24 - q24)) >> 16      (2^-32 wins^2)
//   surprise += nlog2_q20(p_outcome)    fav: q24 > 2^23    dog: q24 < 2^23     (+ _wins when won)
//
// Strength.  The raw value of a slot is prior word 0 (track shared) or word 2, and word 0 where
// word 2 is a NaN (track mode), as bits.  A NaN has no strength; +-inf or |mu| > 2^20 has none
// either and counts as bad, once per game whose own value it is; otherwise the strength is
// t = (int32) rintf(mu * 256) (the product is exact, ties to even).  A game adds its own t (and
// own_known), the t of the other live slots of its roster that have one (mates, mate_slots) and
// those of the other roster (opp, opp_slots).
//
// term record, kExpectTermWords int32 (32 B), one per game slot:
//   [q24, var, surprise, own t, mates, opp, own_known | mate_slots << 1 | opp_slots << 4, 0]
// every field fits: var <= 2^30, surprise <= kNlog2Cap, |t| <= 2^28, |mates| <= 4 * 2^28,
// |opp| <= 5 * 2^28.
//
// player row, kExpectWords int32 (96 B):
//   [games, wins, fav, fav_wins, dog, dog_wins, own_known, 0,
//    exp, var, surprise, own, mates, mate_slots, opp, opp_slots as (lo, hi) each]
//
// Every operation is an integer add, so the table is the same bits on every run, on device and
// host, in any window order and however a window is cut.
#pragma once

#include <math.h>
#include <stdint.h>

#include "career_core.h"
#include "common.h"
#include "ladder_core.h"
#include "profile_core.h"
#include "score_core.h"

namespace ana {

constexpr int kExpectCounters = 7;
constexpr int kExpectSums = 8;
constexpr int kExpectWords = 8 + 2 * kExpectSums;
constexpr int kExpectTermWords = 8;
constexpr int32_t kExpectOne = 1 << 24;   // q24 of a certain win
constexpr int32_t kExpectHalf = 1 << 23;
constexpr float kExpectMuMax = 1048576.0f;  // 2^20
constexpr uint32_t kExpectWonBit = 1u << 31;  // of a sort value, above the slot index
constexpr uint32_t kExpectSlotMask = (1u << kSlotBits) - 1u;

// the live slots of record r when its pred row (flags word, p_win0 bits) makes them games, else 0
template <int K>
ANA_HD uint32_t expect_game_mask(const int32_t* r, int64_t P, uint32_t flags, uint32_t pbits) {
  if (!(flags & kPredScored)) return 0u;
  const float p = ladder_float(pbits);
  if (!(p >= 0.0f && p <= 1.0f)) return 0u;
  return prior_live_mask<K>(r, P);
}

// the raw strength bits of a slot from its prior words 0 and 2
ANA_HD uint32_t expect_raw(int32_t track, uint32_t w0, uint32_t w2) {
  const float m = ladder_float(w2);
  return track == kScoreMode && m == m ? w2 : w0;
}

// 1: t is the strength; 0: none (a NaN); -1: none, and bad
ANA_HD int expect_strength(uint32_t bits, int32_t& t) {
  const float mu = ladder_float(bits);
  t = 0;
  if (mu != mu) return 0;
  if (!(fabsf(mu) <= kExpectMuMax)) return -1;
  t = (int32_t)rintf(mu * 256.0f);
  return 1;
}

// The term records of the games of one match: mask from expect_game_mask (not 0), pbits / pobits
// the pred row's p_win0 and p_outcome, mu[j] the raw strength bits of every slot of mask.  Calls
// emit(j, term) for every game slot, ascending, and returns the number of bad own values.
template <int K, class Emit>
ANA_HD int32_t expect_terms(uint32_t mask, uint32_t pbits, uint32_t pobits, const uint32_t* mu, Emit&& emit) {
  constexpr int S = 2 * K;
  const int32_t p24 = (int32_t)score_p_term(ladder_float(pbits));
  const int32_t surprise = (int32_t)nlog2_q20(pobits);
  int32_t t[S], sum[2] = {0, 0}, cnt[2] = {0, 0}, bad = 0;
  uint32_t known = 0u;
#pragma unroll
  for (int j = 0; j < S; ++j) {
    t[j] = 0;
    if (!((mask >> j) & 1u)) continue;
    const int st = expect_strength(mu[j], t[j]);
    if (st > 0) {
      known |= 1u << j;
      sum[j < K ? 0 : 1] += t[j];
      cnt[j < K ? 0 : 1] += 1;
    } else if (st < 0) {
      ++bad;
    }
  }
#pragma unroll
  for (int j = 0; j < S; ++j) {
    if (!((mask >> j) & 1u)) continue;
    const int me = j < K ? 0 : 1;
    const int32_t q = me == 0 ? p24 : kExpectOne - p24;
    const int32_t own = (int32_t)((known >> j) & 1u);
    int32_t term[kExpectTermWords];
    term[0] = q;
    term[1] = (int32_t)(((int64_t)q * (int64_t)(kExpectOne - q)) >> 16);
    term[2] = surprise;
    term[3] = t[j];
    term[4] = sum[me] - t[j];
    term[5] = sum[1 - me];
    term[6] = own | ((cnt[me] - own) << 1) | (cnt[1 - me] << 4);
    term[7] = 0;
    emit(j, term);
  }
  return bad;
}

struct ExpectRun {
  int32_t games, wins, fav, fav_wins, dog, dog_wins, own_known;
  int32_t pad[3];  // an edge of the run fold is 4n + 2 words
  int64_t exp, var, surprise, own, mates, mate_slots, opp, opp_slots;
};

ANA_HD ExpectRun expect_empty() {
  ExpectRun c;
  c.games = c.wins = c.fav = c.fav_wins = c.dog = c.dog_wins = c.own_known = 0;
  c.pad[0] = c.pad[1] = c.pad[2] = 0;
  c.exp = c.var = c.surprise = c.own = c.mates = c.mate_slots = c.opp = c.opp_slots = 0;
  return c;
}

// the run of one game from its term record
ANA_HD ExpectRun expect_game(const int32_t* term, bool won) {
  ExpectRun c = expect_empty();
  const int32_t q = term[0], w = won ? 1 : 0, packed = term[6];
  c.games = 1;
  c.wins = w;
  c.fav = q > kExpectHalf ? 1 : 0;
  c.fav_wins = c.fav & w;
  c.dog = q < kExpectHalf ? 1 : 0;
  c.dog_wins = c.dog & w;
  c.own_known = packed & 1;
  c.exp = q;
  c.var = term[1];
  c.surprise = term[2];
  c.own = term[3];
  c.mates = term[4];
  c.mate_slots = (packed >> 1) & 7;
  c.opp = term[5];
  c.opp_slots = (packed >> 4) & 7;
  return c;
}

ANA_HD ExpectRun expect_combine(const ExpectRun& a, const ExpectRun& b) {
  ExpectRun c;
  c.games = a.games + b.games;
  c.wins = a.wins + b.wins;
  c.fav = a.fav + b.fav;
  c.fav_wins = a.fav_wins + b.fav_wins;
  c.dog = a.dog + b.dog;
  c.dog_wins = a.dog_wins + b.dog_wins;
  c.own_known = a.own_known + b.own_known;
  c.pad[0] = c.pad[1] = c.pad[2] = 0;
  c.exp = a.exp + b.exp;
  c.var = a.var + b.var;
  c.surprise = a.surprise + b.surprise;
  c.own = a.own + b.own;
  c.mates = a.mates + b.mates;
  c.mate_slots = a.mate_slots + b.mate_slots;
  c.opp = a.opp + b.opp;
  c.opp_slots = a.opp_slots + b.opp_slots;
  return c;
}

ANA_HD void expect_row_add(int32_t* row, const ExpectRun& b) {
  row[0] += b.games;
  row[1] += b.wins;
  row[2] += b.fav;
  row[3] += b.fav_wins;
  row[4] += b.dog;
  row[5] += b.dog_wins;
  row[6] += b.own_known;
  const int64_t s[kExpectSums] = {b.exp, b.var, b.surprise, b.own, b.mates, b.mate_slots, b.opp, b.opp_slots};
#pragma unroll
  for (int k = 0; k < kExpectSums; ++k) career_put64(row + 8 + 2 * k, career_get64(row + 8 + 2 * k) + s[k]);
}

}  // namespace ana
