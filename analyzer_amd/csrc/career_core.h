// K13 careers: what a game is, the career row, and the run summary with its combines,
// shared by the device kernels (career.hip) and the host mirror (host.cpp) so both produce
// the same bits.
//
// A game of player p is an occupied slot j of a match (select_core.h: its position within
// its team < n0 / n1) with rec[j] == p in [0, P), in a match whose mode has its bit in the
// modes mask and whose status byte is rated, AFK or invalid rosters.  The id range is
// checked before anything indexed by the id is touched.  A player's games are ordered by
// ascending (match, slot).
//
// Only rated games have a score, a result and a quality.  The score is ladder_score
// (ladder_core.h) of the slot's (s_mu, s_sig) -- track shared -- or (m_mu, m_sig) -- track
// mode; a NaN score counts as a game but not for peak and trough, which compare through
// ladder_score_key.  A game is won when its own roster's winner bit is set in meta1.  The
// quality adds rint(q * 2^24) (ties to even; 0 for a NaN or a q outside [0, 1]).
//
// career row, kCareerWords int32:
//   [games, wins, afk, invalid, first lo, hi, last lo, hi, peak bits, peak_match lo, hi,
//    trough bits, streak, best_win, quality_sum lo, hi]
// games / wins count rated games; first / last / peak_match are global match indices (-1:
// none); peak / trough are fp32 bit patterns (kCareerNone: none); streak is +n for a career
// that ends in n wins, -n for n losses.
//
// A CareerRun summarises a stretch of one player's games: the row's fields plus the leading
// win run and the trailing win and loss runs, which is what a streak needs across a cut.
// career_combine(a, b) (a earlier) and career_row_add(row, b) are exact integer operations
// and career_combine is associative with career_empty() as its identity, so a career is the
// same bits however the games are cut into runs.
#pragma once

#include <math.h>
#include <stdint.h>

#include "common.h"
#include "ladder_core.h"
#include "select_core.h"

namespace ana {

constexpr int kCareerWords = 16;
constexpr uint32_t kCareerNone = 0x7fc00000u;
constexpr uint32_t kCareerAllModes = (1u << kModes) - 1u;

enum CareerTrack : int32_t {
  kCareerShared = 0,  // (s_mu, s_sig)
  kCareerMode = 1,    // (m_mu, m_sig)
};

// host side: the options of a K13 / K17 table as the launchers and host mirrors check them
inline bool career_options_ok(int track, int score, uint32_t modes) {
  return (track == kCareerShared || track == kCareerMode) && (score == kLadderConservative || score == kLadderMu) &&
         !(modes & ~kCareerAllModes);
}

// a game's event, 8 B: word 0 the score bits, word 1 the quality term | win | status
constexpr int kCareerEventWords = 2;
constexpr uint32_t kCareerQualityMask = (1u << 25) - 1u;  // terms are 0..2^24
constexpr uint32_t kCareerWinBit = 1u << 25;
constexpr int kCareerStatusShift = 26;

// bit j set: slot j of the record is a candidate game (occupied, id in range, mode selected)
template <int K>
ANA_HD uint32_t career_mask(const int32_t* r, int64_t P, uint32_t modes) {
  constexpr int S = 2 * K;
  const uint32_t m0 = (uint32_t)r[S];
  const int mode = meta_mode(m0);
  if (mode >= kModes || !((modes >> mode) & 1u)) return 0u;
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

ANA_HD uint32_t career_quality_term(float q) {
  return q >= 0.0f && q <= 1.0f ? (uint32_t)rintf(q * 16777216.0f) : 0u;
}

// the first of the two row fields (mu, sigma) a track's score is made of
ANA_HD int career_field(int32_t track) { return track == kCareerMode ? 3 : 0; }

// the event of slot j of a match with status st (select_status holds) from the slot's mu and
// sigma words (row[f * 2K + j], row[(f + 1) * 2K + j], f = career_field) and the quality word
template <int K>
ANA_HD void career_event(const int32_t* r, int j, uint32_t st, uint32_t mu, uint32_t sigma, uint32_t quality,
                         int32_t score, uint32_t* ev) {
  constexpr int S = 2 * K;
  uint32_t bits = kCareerNone, w = st << kCareerStatusShift;
  if (st == kRated) {
    bits = ladder_bits(ladder_score(ladder_float(mu), ladder_float(sigma), score));
    w |= career_quality_term(ladder_float(quality));
    const uint32_t m1 = (uint32_t)r[S + 1];
    if (j < K ? meta_winner0(m1) : meta_winner1(m1)) w |= kCareerWinBit;
  }
  ev[0] = bits;
  ev[1] = w;
}

struct CareerRun {
  int32_t games, wins, afk, invalid;  // games: the rated ones
  int64_t first, last, peak_match, quality_sum;
  uint32_t peak, trough;
  int32_t lead_win, trail_win, trail_loss, best_win;
};

ANA_HD CareerRun career_empty() {
  CareerRun c;
  c.games = c.wins = c.afk = c.invalid = 0;
  c.first = c.last = c.peak_match = -1;
  c.quality_sum = 0;
  c.peak = c.trough = kCareerNone;
  c.lead_win = c.trail_win = c.trail_loss = c.best_win = 0;
  return c;
}

// the run of one game: its event at global match g
ANA_HD CareerRun career_game(uint32_t bits, uint32_t w, int64_t g) {
  CareerRun c = career_empty();
  const uint32_t st = w >> kCareerStatusShift;
  if (st == kAfk) c.afk = 1;
  if (st == kInvalidRosters) c.invalid = 1;
  if (st != kRated) return c;
  const int32_t win = (w & kCareerWinBit) ? 1 : 0;
  c.games = 1;
  c.wins = win;
  c.first = c.last = g;
  c.quality_sum = (int64_t)(w & kCareerQualityMask);
  const float s = ladder_float(bits);
  if (s == s) {
    c.peak = c.trough = bits;
    c.peak_match = g;
  }
  c.lead_win = c.trail_win = c.best_win = win;
  c.trail_loss = 1 - win;
  return c;
}

// is score bits b above (below) score bits a; neither is a NaN
ANA_HD bool career_above(uint32_t b, uint32_t a) {
  return ladder_score_key(ladder_float(b)) < ladder_score_key(ladder_float(a));
}
ANA_HD bool career_below(uint32_t b, uint32_t a) {
  return ladder_score_key(ladder_float(b)) > ladder_score_key(ladder_float(a));
}

ANA_HD int32_t career_max(int32_t a, int32_t b) { return a > b ? a : b; }

// a then b
ANA_HD CareerRun career_combine(const CareerRun& a, const CareerRun& b) {
  CareerRun c;
  c.games = a.games + b.games;
  c.wins = a.wins + b.wins;
  c.afk = a.afk + b.afk;
  c.invalid = a.invalid + b.invalid;
  c.quality_sum = a.quality_sum + b.quality_sum;
  c.first = a.first >= 0 ? a.first : b.first;
  c.last = b.last >= 0 ? b.last : a.last;
  const bool has_a = a.peak_match >= 0, has_b = b.peak_match >= 0;
  const bool up = has_b && (!has_a || career_above(b.peak, a.peak));  // a tie keeps the earlier match
  c.peak = up ? b.peak : a.peak;
  c.peak_match = up ? b.peak_match : a.peak_match;
  c.trough = has_b && (!has_a || career_below(b.trough, a.trough)) ? b.trough : a.trough;
  c.lead_win = a.lead_win == a.games ? a.games + b.lead_win : a.lead_win;
  c.trail_win = b.trail_win == b.games ? a.trail_win + b.games : b.trail_win;
  c.trail_loss = b.trail_loss == b.games ? a.trail_loss + b.games : b.trail_loss;
  c.best_win = career_max(career_max(a.best_win, b.best_win), a.trail_win + b.lead_win);
  return c;
}

ANA_HD int64_t career_get64(const int32_t* w) {
  return (int64_t)((uint64_t)(uint32_t)w[0] | ((uint64_t)(uint32_t)w[1] << 32));
}
ANA_HD void career_put64(int32_t* w, int64_t v) {
  w[0] = (int32_t)(uint32_t)((uint64_t)v & 0xffffffffull);
  w[1] = (int32_t)(uint32_t)((uint64_t)v >> 32);
}

ANA_HD void career_row_empty(int32_t* row) {
#pragma unroll
  for (int i = 0; i < kCareerWords; ++i) row[i] = 0;
  career_put64(row + 4, -1);
  career_put64(row + 6, -1);
  career_put64(row + 9, -1);
  row[8] = row[11] = (int32_t)kCareerNone;
}

// row = row then b
ANA_HD void career_row_add(int32_t* row, const CareerRun& b) {
  row[0] += b.games;
  row[1] += b.wins;
  row[2] += b.afk;
  row[3] += b.invalid;
  if (b.games == 0) return;  // nothing else moves without a rated game
  career_put64(row + 14, career_get64(row + 14) + b.quality_sum);
  if (career_get64(row + 4) < 0) career_put64(row + 4, b.first);
  career_put64(row + 6, b.last);
  if (b.peak_match >= 0) {
    const bool has = career_get64(row + 9) >= 0;
    if (!has || career_above(b.peak, (uint32_t)row[8])) {  // a tie keeps the earlier match
      row[8] = (int32_t)b.peak;
      career_put64(row + 9, b.peak_match);
    }
    if (!has || career_below(b.trough, (uint32_t)row[11])) row[11] = (int32_t)b.trough;
  }
  const int32_t tw = row[12] > 0 ? row[12] : 0, tl = row[12] < 0 ? -row[12] : 0;
  row[13] = career_max(career_max(row[13], b.best_win), tw + b.lead_win);
  const int32_t ntw = b.trail_win == b.games ? tw + b.games : b.trail_win;
  const int32_t ntl = b.trail_loss == b.games ? tl + b.games : b.trail_loss;
  row[12] = ntw > 0 ? ntw : -ntl;
}

}  // namespace ana
