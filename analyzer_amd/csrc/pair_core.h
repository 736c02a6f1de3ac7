// K15 pairs: what an entry of the pair table is, how the entries of a match are numbered and
// how an entry rides in a sort value, shared by the device kernels (pairs.hip) and the host
// mirror (host.cpp) so both produce the same bits.
//
// A slot j of a match is *live* when it is occupied (its position within its team < n0 / n1),
// its id lies in [0, P), the match's mode has its bit in the modes mask (career_core.h calls
// this a candidate game) and the row's status byte is kRated: AFK and invalid-roster matches
// have no result.  An *entry* is an ordered pair of two different live slots (ja, jb) with
// a = rec[ja] != b = rec[jb]; a 2K-slot match has at most 2K(2K - 1) of them.  A player aliased
// into two slots makes no entry with itself, and each of its slots makes entries with the
// others.  The entry's relation is *with* when both slots are on one roster, else *against*;
// its win bit is the winner bit of a's roster in meta1, taken as it stands.  With a player
// filter (a bitmap over [0, P), probed only after the id range check) an entry also needs
// a's bit.
//
// The pair table is the set of distinct (a, b) in ascending order of key = a << 32 | b, each
// with kPairWords int32 counters [with_games, with_wins, vs_games, vs_wins] from a's side.
// Every counter is an integer sum, so a table is the same bits however the entries are cut,
// ordered or grouped.
#pragma once

#include <stdint.h>

#include "common.h"

namespace ana {

constexpr int kPairWords = 4;
constexpr uint32_t kPairAllModes = (1u << kModes) - 1u;

// entries of a match of team size K
constexpr int pair_entries(int K) { return 2 * K * (2 * K - 1); }

// sort value of an entry: its index in the window and, above it, the relation and the win bit
constexpr uint32_t kPairIndexMask = (1u << kSlotBits) - 1u;
constexpr uint32_t kPairVsBit = 1u << kSlotBits;
constexpr uint32_t kPairWinBit = 1u << (kSlotBits + 1);
static_assert(kSlotBits + 2 <= 32, "relation and win bit ride above the entry index");

// entry q of a match, 0 <= q < 2K(2K - 1): slot ja with its q % (2K - 1)-th other slot
template <int K>
ANA_HD void pair_slots(int q, int& ja, int& jb) {
  constexpr int S = 2 * K;
  ja = q / (S - 1);
  const int t = q - ja * (S - 1);
  jb = t + (t >= ja ? 1 : 0);
}

ANA_HD bool pair_mode_selected(uint32_t m0, uint32_t modes) {
  const int mode = meta_mode(m0);
  return mode < kModes && ((modes >> mode) & 1u);
}

// slot j holding id p is occupied by a player of [0, P)
template <int K>
ANA_HD bool pair_slot_live(uint32_t m0, int j, int32_t p, int64_t P) {
  const int pos = j < K ? j : j - K;
  return pos < (j < K ? meta_n0(m0) : meta_n1(m0)) && p >= 0 && (int64_t)p < P;
}

// the id range is checked by the caller
ANA_HD bool pair_filtered(const uint32_t* bitmap, int32_t a) {
  return bitmap == nullptr || ((bitmap[a >> 5] >> (a & 31)) & 1u);
}

template <int K>
ANA_HD bool pair_with(int ja, int jb) { return (ja < K) == (jb < K); }

template <int K>
ANA_HD bool pair_win(uint32_t m1, int ja) { return ja < K ? meta_winner0(m1) : meta_winner1(m1); }

template <int K>
ANA_HD uint32_t pair_flags(uint32_t m1, int ja, int jb) {
  return (pair_with<K>(ja, jb) ? 0u : kPairVsBit) | (pair_win<K>(m1, ja) ? kPairWinBit : 0u);
}

// the counters of one entry from its flags
ANA_HD void pair_counters(uint32_t flags, int32_t* c) {
  const int o = (flags & kPairVsBit) ? 2 : 0;
  c[0] = c[1] = c[2] = c[3] = 0;
  c[o] = 1;
  c[o + 1] = (flags & kPairWinBit) ? 1 : 0;
}

ANA_HD int64_t pair_key(uint32_t a, uint32_t b) { return (int64_t)(((uint64_t)a << 32) | (uint64_t)b); }

}  // namespace ana
