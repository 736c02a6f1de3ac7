// K16 hindsight: every player's skill curve smoothed backwards over its own history, shared by
// the device kernels (hindsight.hip) and the host mirror (host.cpp).
//
// The model.  On one track a player's *chain* is its elements (below) in chronological order.
// Element t holds the filtered posterior (m_t, sigma_t) of the packed output row, read as fp32.
// The engine's own model of a track between two rated matches is a random walk with variance
// tau^2, so with P_t = sigma_t^2 and G_t = P_t / (P_t + tau^2) (G_t = 0 when P_t + tau^2 = 0)
// the Rauch-Tung-Striebel smoother of the chain is, walking backwards from the newest element,
// which is its own smoothed value:
//
//   mh_t = m_t + G_t (mh_{t+1} - m_t)
//   Ph_t = P_t + G_t^2 (Ph_{t+1} - P_t - tau^2)
//
// It conditions on the filtered posteriors; it does not run the match factors again, so it is
// not TrueSkill-Through-Time: what a later match says about a player reaches an earlier one
// only through that player's own chain, never through the team mates and opponents.  K20
// (ttt_core.h) is that; it shares the elements below and with zero sweeps computes the same.
//
// Elements.  A slot is an element when it is live (score_core.h prior_live_mask), its row's
// status is kRated, no later slot of the record carries the same player (prior_last_mask) and,
// on a mode track, the match is of that mode -- the shared track takes every mode, because
// tau^2 is added at every rated match.  Such a slot whose (mu, sigma) is not finite or whose
// sigma < 0 is not an element and counts as *bad*.  Every slot that is not an element gets
// (NaN, NaN).
//
// As maps.  With G(P_t + tau^2) = P_t the recursion reads mh_t = a_t + G_t mh_{t+1} and
// Ph_t = c_t + G_t^2 Ph_{t+1}, a_t = (1 - G_t) m_t, c_t = G_t tau^2 >= 0: element t is the pair
// of affine maps x -> a_t + G_t x, y -> c_t + G_t^2 y, held as HsMap (A, B, C) = (a_t, G_t, c_t).
// hs_combine(a, b), a EARLIER IN TIME, is a applied after b:
//
//   A = a.A + a.B b.A     B = a.B b.B     C = a.C + a.B^2 b.C
//
// associative, identity (0, 1, 0).  What lies behind a stretch of the chain -- the chain's
// newest element, or the carry of the windows added before (they are LATER in time: windows are
// added newest first) -- is the constant map (mh, 0, Ph); a state that ends in one has B == 0
// exactly, a state that does not has B == 1 only as the identity (B is a product of G's; no
// seed is ever anything else than a constant or the identity).
//
// Order, in one place.  The smoothed value of element t needs the composition of the maps of
// t, t + 1, ... up to the newest: a suffix in time.  SegScan (scan_dev.h) scans prefixes.  So
// the keys kernel writes slot i of an n-slot call to position n - 1 - i; the stable sort by
// player then leaves each player's slots NEWEST FIRST, and an inclusive scan in that order
// covers the element and everything later in time.  The scan's combine(x, y), x earlier IN THE
// SCAN, is therefore hs_combine(y, x): y is the older one.  hs_scan_combine below is the only
// place where the two orders meet.
//
// Arithmetic.  (G, a, c), the combine and the mirror's loop are fp64, every operation the IEEE
// one written (hindsight.hip is built with -ffp-contract=off).  sigma^2 of an fp32 is exact in
// fp64 and so is its square root.  The output is (mh, sqrt(Ph)) rounded once to fp32.
//
// Error budget (u = 2^-53, n the length of the chain, M = max |m_t| over it, E the exact value
// of the recursion on the fp32 inputs and the real tau^2):
//
//   |mh - E|        <= ulp32(E) / 2 + c n u M
//   |sqrt(Ph) - E|  <= ulp32(E) / 2 + (c n / 2 + 1) u E                    with c = kHsBudgetC = 20.
//
// Derivation.  mh_t = sum_s w_s m_s is a convex combination of m_t .. m_T, |partial sums| <= M.
//  (1) G_t carries a relative error <= 4u: tau^2 rounded once, the sum, the quotient, and one of
//      the roundings of the products of B's, of which a chain of k elements has k - 1 however it
//      is bracketed.  d mh / d G_j = (prod of G's before j) (mh_{j+1} - m_j), at most 2M in
//      size, so a relative error of 4u in G_j moves mh by at most 8uM.
//  (2) 1 - G_t has an absolute error <= 4u + u and is multiplied by m_t with one rounding more:
//      a_t is off by at most 5uM + uM, and the factors in front of it are <= 1.
//  (3) A combine rounds A twice (product, sum), each by <= uM, and later factors B <= 1 do not
//      grow it.  The expression tree of one output has one combine per element and at most one
//      more per element for the carries between windows (which are fp64 and round nothing
//      themselves): <= 4uM per element.  Combining with the identity is exact.
//      Together <= (8 + 6 + 4) n u M <= 20 n u M.
//  Ph_t = sum of the positive terms (prod G^2) c_s and (prod G^2) P_T, so relative errors add
//  without cancellation: c_s <= 5u (G, tau^2, the product); prod G^2 <= 8u per factor; a
//  combine rounds C three times (square, product, sum), twice per element with the carries:
//  <= 6u.  Together <= 19 n u <= 20 n u relative on Ph, half of it on the root, plus u for
//  the root's own rounding.
//  The mirror's loop rounds each step a bounded number of times on values of size <= M (mean)
//  and stays inside the same budget on the chains a filter produces; on the variance it forms
//  Ph_{t+1} - P_t - tau^2, which cancels, so its error is relative to P_t + tau^2, not to
//  Ph_t: the tests hold it to the budget on chains whose sigma stay within a factor of four.
//
// Exact, bit for bit: a chain's newest element is its filtered (mu, sigma); with tau = 0 every
// G is 1 (or 0 at sigma = 0), every map the identity (or a constant), so every element equals
// the next newer one; non-elements are NaN; bad is an integer count.
#pragma once

#include <math.h>
#include <stdint.h>

#include "common.h"
#include "score_core.h"

namespace ana {

constexpr int kHsBudgetC = 20;
constexpr uint32_t kHsNull = 0x7fc00000u;

enum HsTrack : int32_t {
  kHsShared = 0,  // (s_mu, s_sig) of every mode
  kHsMode = 1,    // (m_mu, m_sig) of the matches of one mode
};

struct HsMap {
  double A, B, C;
};

ANA_HD HsMap hs_identity() { return HsMap{0.0, 1.0, 0.0}; }
ANA_HD HsMap hs_const(double m, double Pv) { return HsMap{m, 0.0, Pv}; }

// a earlier in time: a after b
ANA_HD HsMap hs_combine(const HsMap& a, const HsMap& b) {
  return HsMap{a.A + a.B * b.A, a.B * b.B, a.C + (a.B * a.B) * b.C};
}

// x earlier in the scan, which runs newest first: x is the newer one
ANA_HD HsMap hs_scan_combine(const HsMap& x, const HsMap& y) { return hs_combine(y, x); }

ANA_HD double hs_gain(double Pv, double tau2) {
  const double d = Pv + tau2;
  return d == 0.0 ? 0.0 : Pv / d;
}

// the map of an element with something later in time behind it
ANA_HD HsMap hs_element(float mu, float sigma, double tau2) {
  const double m = (double)mu, s = (double)sigma;
  const double g = hs_gain(s * s, tau2);
  return HsMap{(1.0 - g) * m, g, g * tau2};
}

// the newest element of a chain: its own smoothed value
ANA_HD HsMap hs_newest(float mu, float sigma) {
  const double s = (double)sigma;
  return hs_const((double)mu, s * s);
}

// The scan's term of the first element a workgroup sees of a key.  seed: what lies behind it,
// a constant, or the identity when nothing does -- then the element is the chain's newest.
ANA_HD HsMap hs_seeded(float mu, float sigma, double tau2, const HsMap& seed) {
  return seed.B != 0.0 ? hs_newest(mu, sigma) : hs_combine(hs_element(mu, sigma, tau2), seed);
}

// a carry row (mh, Ph) as a seed: NaN = no later match
ANA_HD HsMap hs_seed_of_row(double m, double Pv) { return m != m ? hs_identity() : hs_const(m, Pv); }

ANA_HD bool hs_value_ok(float mu, float sigma) { return isfinite(mu) && isfinite(sigma) && !(sigma < 0.0f); }

// bit j set: slot j of record r, whose row has the status byte st, is an element on the track
// (before the check of its values).  mode: the mode of a kHsMode track.
template <int K>
ANA_HD uint32_t hs_element_mask(const int32_t* r, uint32_t live, uint32_t st, int track, int mode) {
  if (!live || st != kRated) return 0u;
  if (track == kHsMode && meta_mode((uint32_t)r[2 * K]) != mode) return 0u;
  return prior_last_mask<K>(r, live);
}

}  // namespace ana
