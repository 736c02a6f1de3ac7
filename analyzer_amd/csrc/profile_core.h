// K17 profiles: what a game is, the stat term, the bracket of a score, the player row and
// the baseline table, shared by the device kernels (profile.hip) and the host mirror
// (host.cpp) so both produce the same bits.
//
// A game of player p is a slot j of a match whose bit career_mask (career_core.h) sets --
// occupied, rec[j] == p in [0, P), the mode in the modes mask -- in a match whose status byte
// is kRated.  AFK, invalid and unsupported matches are no games here: their stats mean nothing.
// A game is won when its own roster's winner bit is set in meta1.
//
// Stat term.  A stat value x (fp32) that is finite with 0 <= x <= 2^30 adds the integer
// rint(x * 256) (x * 256 is exact, ties to even); any other value adds 0 and counts as bad.
//
// Bracket.  The score is ladder_score (ladder_core.h) of the slot's (mu, sigma) on the chosen
// track.  ProfileEdges holds up to kProfileMaxEdges finite, strictly ascending fp32 edges; the
// bracket of a score is the number of edges <= it (plain fp32 compares), 0 .. B - 1 with
// B = n + 1.  A NaN score has no bracket (-1): the game counts for its player, not for the
// baselines, and bumps the unbracketed counter.
//
// player row, kProfileWords int32 (80 B): [games, wins, 0, 0, sum[0] lo, hi, ..., sum[7] lo, hi]
// baseline table, int64: [kModes][B][2 (lost, won)][kProfileCellWords] = games and the 8 sums,
// then [bad, unbracketed]: profile_table_words(B) words.
//
// Every operation is an integer add, so both tables are the same bits on every run, on device
// and host, in any window order and however a window is cut.
#pragma once

#include <math.h>
#include <stdint.h>

#include "career_core.h"
#include "common.h"
#include "ladder_core.h"

namespace ana {

constexpr int kProfileStats = 8;
constexpr int kProfileWords = 4 + 2 * kProfileStats;
constexpr int kProfileMaxEdges = 31;
constexpr int kProfileMaxBrackets = kProfileMaxEdges + 1;
constexpr int kProfileCellWords = 1 + kProfileStats;
constexpr int kProfileCounters = 2;  // bad, unbracketed
constexpr int kProfileMaxTableWords = kModes * kProfileMaxBrackets * 2 * kProfileCellWords + kProfileCounters;
constexpr uint32_t kProfileWonBit = 1u << 31;  // of a sort value, above the slot index
constexpr uint32_t kProfileSlotMask = (1u << kSlotBits) - 1u;
constexpr float kProfileStatMax = 1073741824.0f;  // 2^30

struct ProfileEdges {
  int32_t n;
  float e[kProfileMaxEdges];
};

ANA_HD int profile_table_words(int B) { return kModes * B * 2 * kProfileCellWords + kProfileCounters; }

// the first word of the cell (mode, bracket, won) of a table with B brackets
ANA_HD int profile_cell(int B, int mode, int bracket, bool won) {
  return ((mode * B + bracket) * 2 + (won ? 1 : 0)) * kProfileCellWords;
}

// the term of one stat value; an offending value adds 0 and bumps bad
ANA_HD int64_t profile_term(float x, int32_t& bad) {
  if (x >= 0.0f && x <= kProfileStatMax) return (int64_t)rintf(x * 256.0f);
  ++bad;
  return 0;
}

// the number of edges <= s, or -1 for a NaN
ANA_HD int profile_bracket(const ProfileEdges& edges, float s) {
  if (s != s) return -1;
  int b = 0;
#pragma unroll
  for (int i = 0; i < kProfileMaxEdges; ++i)
    if (i < edges.n && edges.e[i] <= s) ++b;
  return b;
}

// does slot j of record r carry its own roster's winner bit
template <int K>
ANA_HD bool profile_won(const int32_t* r, int j) {
  const uint32_t m1 = (uint32_t)r[2 * K + 1];
  return j < K ? meta_winner0(m1) : meta_winner1(m1);
}

struct ProfileRun {
  int32_t games, wins;
  int64_t sum[kProfileStats];
};

ANA_HD ProfileRun profile_empty() {
  ProfileRun c;
  c.games = c.wins = 0;
#pragma unroll
  for (int k = 0; k < kProfileStats; ++k) c.sum[k] = 0;
  return c;
}

// the run of one game from its 8 stat values; the bad values are counted where the cells are
ANA_HD ProfileRun profile_game(const float* x, bool won, int32_t& bad) {
  ProfileRun c;
  c.games = 1;
  c.wins = won ? 1 : 0;
#pragma unroll
  for (int k = 0; k < kProfileStats; ++k) c.sum[k] = profile_term(x[k], bad);
  return c;
}

ANA_HD ProfileRun profile_combine(const ProfileRun& a, const ProfileRun& b) {
  ProfileRun c;
  c.games = a.games + b.games;
  c.wins = a.wins + b.wins;
#pragma unroll
  for (int k = 0; k < kProfileStats; ++k) c.sum[k] = a.sum[k] + b.sum[k];
  return c;
}

ANA_HD void profile_row_add(int32_t* row, const ProfileRun& b) {
  row[0] += b.games;
  row[1] += b.wins;
#pragma unroll
  for (int k = 0; k < kProfileStats; ++k)
    career_put64(row + 4 + 2 * k, career_get64(row + 4 + 2 * k) + b.sum[k]);
}

// What one game adds to the baseline table of B = edges.n + 1 brackets: add(word, amount) for
// every word that moves.  score: the game's score; bad: the offending values profile_game
// counted for it.
template <class Add>
ANA_HD void profile_cell_add(const ProfileEdges& edges, int mode, float score, const ProfileRun& g, int32_t bad,
                             Add&& add) {
  const int B = edges.n + 1, counters = profile_table_words(B) - kProfileCounters;
  if (bad) add(counters, (int64_t)bad);
  const int b = profile_bracket(edges, score);
  if (b < 0) {
    add(counters + 1, (int64_t)1);
    return;
  }
  const int c = profile_cell(B, mode, b, g.wins != 0);
  add(c, (int64_t)1);
#pragma unroll
  for (int k = 0; k < kProfileStats; ++k)
    if (g.sum[k] != 0) add(c + 1 + k, g.sum[k]);
}

}  // namespace ana
