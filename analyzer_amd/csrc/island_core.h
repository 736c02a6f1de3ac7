// K18 islands: the connected components of the match graph, shared by the device kernels
// (islands.hip) and the host mirror (host.cpp) so both produce the same bits.
//
// The vertices are the players [0, P); an edge joins any two live slots of one match, live as
// pair_core.h has it: the slot is occupied, its id lies in [0, P), the match's mode is in the
// modes mask and the row's status byte is kRated.  A match with live slots j0 < j1 < ... is the
// star that joins rec[j1], rec[j2], ... to rec[j0]; a player aliased into two slots makes no edge
// with itself and is still seen.
//
// State per player:
//   parent  int32, initially parent[i] = i: the union-find forest
//   slots   int32: the live slots of the player so far in the low 31 bits; kIslandSeenBit marks a
//           player that an explicit edge named.  A player is *seen* when the word is not 0
//   credit  int32: the rated matches whose first live slot holds the player.  The credit depends
//           on the match alone, so an island's matches are an integer sum that does not depend on
//           how the history is cut or ordered
//
// Invariants of parent, kept by every writer on the device and on the host:
//   (1) parent[x] <= x, always; a root is a word with parent[x] == x
//   (2) a word only ever decreases
//   (3) a word only ever points to a player of its own island
//   (4) only roots are hooked: a hook is a compare-and-swap of parent[hi] from hi to lo < hi
// By (1) every walk x, parent[x], parent[parent[x]], ... strictly decreases until it stops at a
// root, so a find takes at most P steps and no cycle can form.  By (3) and (4) two players share a
// root after the unions exactly when they are connected, and since a union always hooks the larger
// root under the smaller, the one root left in an island is the smallest of all roots it ever had:
// the smallest id of the island, whatever the order or interleaving of the unions.  Shortening a
// path (parent[x] = an ancestor of x) keeps all four.  So parent after a flatten, and with it every
// sum grouped by it, is the same bits on the device, in the host mirror and for any order, cut or
// repetition of the history.
//
// Concurrency (device): a lane reads parent words with relaxed agent-scope loads and writes them
// only with agent-scope atomics.  A stale read returns an older value of the word, which by (2)
// and (3) is an ancestor-or-self in the same island that may no longer be a root; the
// compare-and-swap of a hook then fails and returns the word's current value, from which the lane
// goes on.  No lane waits for another: every loop iteration either ends the loop or has seen a
// word below the value it last saw there, so a union of a and b takes at most P rounds (max(a, b)
// strictly decreases) of finds of at most P steps each.  Both loops are capped at P; a lane that
// hits the cap, or reads a word that breaks (1), stops and sets the sticky error word.
#pragma once

#include <stdint.h>

#include "common.h"
#include "pair_core.h"

namespace ana {

constexpr uint32_t kIslandSeenBit = 0x80000000u;  // of a slots word: named by an explicit edge
constexpr uint32_t kIslandSlotMask = 0x7fffffffu;
constexpr int kIslandCtrlWords = 2;  // int64 ctrl: [0] sticky error, [1] edges dropped as bad
constexpr int kIslandCensusRows = 3;  // census [3][P] int64: players, matches, player_games
constexpr uint32_t kIslandAllModes = kPairAllModes;

// sticky error bits
constexpr int64_t kIslandErrSteps = 1;   // a find or a union ran into its cap
constexpr int64_t kIslandErrParent = 2;  // a parent word outside [0, x]

// the live slots of record r (rows' status not yet looked at): bit j of the result
template <int K>
ANA_HD uint32_t island_live_mask(const int32_t* r, int64_t P, uint32_t modes) {
  constexpr int S = 2 * K;
  const uint32_t m0 = (uint32_t)r[S];
  if (!pair_mode_selected(m0, modes)) return 0u;
  uint32_t live = 0u;
#pragma unroll
  for (int j = 0; j < S; ++j)
    if (pair_slot_live<K>(m0, j, r[j], P)) live |= 1u << j;
  return live;
}

// a parent word p read at x keeps invariant (1)
ANA_HD bool island_word_ok(int32_t p, int32_t x) { return (uint32_t)p <= (uint32_t)x; }

}  // namespace ana
