// K10 records_select: what a hit is and how it is laid out, shared by the device
// kernels (select.hip) and the host mirror (host.cpp) so both produce the same bits.
//
// A hit is an occupied slot j of a match (its position within its team < n0 / n1, as
// early_status decodes them) whose player id lies in [0, P) and has its bit set in the
// query bitmap, in a match whose status byte is rated, AFK or invalid rosters.  The id
// range is checked before the bitmap is probed, and the bitmap before the match's output
// row is touched (the status byte sits in the row).
//
// hits [n][kHitWords] int32, 48 B per hit:
//   [match_lo, match_hi, player, slot | status << 8,
//    s_mu, s_sig, delta, m_mu, m_sig, quality (fp32 bit patterns: a NaN stays a NaN),
//    meta0, meta1]
#pragma once

#include <stdint.h>

#include "common.h"

namespace ana {

constexpr int kHitWords = 12;

// bit j set: slot j of the record is occupied by a queried player
template <int K>
ANA_HD uint32_t select_mask(const int32_t* r, int64_t P, const uint32_t* bitmap) {
  constexpr int S = 2 * K;
  const uint32_t m0 = (uint32_t)r[S];
  const int n0 = meta_n0(m0), n1 = meta_n1(m0);
  uint32_t mask = 0u;
#pragma unroll
  for (int j = 0; j < S; ++j) {
    const int pos = j < K ? j : j - K;
    const int32_t p = r[j];
    if (pos < (j < K ? n0 : n1) && p >= 0 && (int64_t)p < P && ((bitmap[p >> 5] >> (p & 31)) & 1u))
      mask |= 1u << j;
  }
  return mask;
}

// matches with records: unsupported, error and not-processed matches produce no hits
ANA_HD bool select_status(uint32_t st) { return st == kRated || st == kAfk || st == kInvalidRosters; }

// status byte of a packed output row (csrc/common.h RateOut), row as 32-bit words
template <int K>
ANA_HD uint32_t select_row_status(const uint32_t* row) {
  return row[5 * 2 * K + 1] & 0xffu;
}

// the hit of slot j (a compile-time constant at every call site) of global match g
template <int K>
ANA_HD void select_hit(const int32_t* r, const uint32_t* row, int64_t g, int j, uint32_t st, int32_t* h) {
  constexpr int S = 2 * K;
  h[0] = (int32_t)(uint32_t)((uint64_t)g & 0xffffffffull);
  h[1] = (int32_t)(uint32_t)((uint64_t)g >> 32);
  h[2] = r[j];
  h[3] = (int32_t)((uint32_t)j | (st << 8));
#pragma unroll
  for (int f = 0; f < 5; ++f) h[4 + f] = (int32_t)row[f * S + j];
  h[9] = (int32_t)row[5 * S];
  h[10] = r[S];
  h[11] = r[S + 1];
}

}  // namespace ana
