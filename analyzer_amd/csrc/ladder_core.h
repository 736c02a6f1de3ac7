// K11 ladder: what a player's score on a track is, who is ranked, and the sort key,
// shared by the device kernels (ladder.hip) and the host mirror (host.cpp) so both
// produce the same bits.
//
// A track is granule 0..6 of a roster row, (mu, tag, sigma, tag); the tag words belong
// to the executor and are never looked at.  The score is computed in fp32: mu - sigma
// (conservative, one IEEE subtraction) or mu, with -0 canonicalised to +0 by adding
// 0.0f.  A player is ranked iff the score is not NaN and sigma <= max_sigma (a NaN
// sigma fails the comparison; NULL tracks have a NaN mu and inf - inf is NaN, so both
// drop out).  The order is descending score, ties by ascending player id.
//
// The key maps the score's bits u to asc = (u >> 31) ? ~u : (u | 0x80000000), whose
// unsigned order is the scores' ascending order, and key = ~asc, so ascending unsigned
// keys are descending scores; a stable sort of pairs that start in id order gives the
// tie rule.  The largest key of a ranked player is 0xFF800000 (-inf); unranked players
// get kLadderUnranked and sort last.  ladder_key_score inverts the key exactly.
#pragma once

#include <stdint.h>

#include "common.h"

namespace ana {

constexpr uint32_t kLadderUnranked = 0xffffffffu;
constexpr uint32_t kLadderTrackMask = (1u << kTracks) - 1u;  // valid bits of a track set

enum LadderScore : int32_t {
  kLadderConservative = 0,  // mu - sigma
  kLadderMu = 1,
};

ANA_HD uint32_t ladder_bits(float x) {
  uint32_t u;
  __builtin_memcpy(&u, &x, 4);
  return u;
}
ANA_HD float ladder_float(uint32_t u) {
  float x;
  __builtin_memcpy(&x, &u, 4);
  return x;
}

ANA_HD float ladder_score(float mu, float sigma, int32_t score) {
  const float s = score == kLadderMu ? mu : mu - sigma;
  return s + 0.0f;
}

ANA_HD bool ladder_ranked(float s, float sigma, float max_sigma) { return s == s && sigma <= max_sigma; }

ANA_HD uint32_t ladder_score_key(float s) {
  const uint32_t u = ladder_bits(s);
  const uint32_t asc = (u >> 31) ? ~u : (u | 0x80000000u);
  return ~asc;
}

ANA_HD float ladder_key_score(uint32_t key) {
  const uint32_t asc = ~key;
  return ladder_float((asc >> 31) ? (asc & 0x7fffffffu) : ~asc);
}

// the key of one granule's (mu, sigma)
ANA_HD uint32_t ladder_key(float mu, float sigma, int32_t score, float max_sigma) {
  const float s = ladder_score(mu, sigma, score);
  return ladder_ranked(s, sigma, max_sigma) ? ladder_score_key(s) : kLadderUnranked;
}

}  // namespace ana
