// K20 through time: a history re-estimated jointly -- TrueSkill-Through-Time, expectation
// propagation over every player's chain and every match factor -- shared by the device kernels
// (ttt.hip) and the host mirror (host.cpp host_ttt_fit).
//
// Elements are K16's (hindsight_core.h): live, the row rated, the player's last slot of the
// record, on a mode track the match of that mode, the filtered (mu, sigma) finite with sigma >= 0
// (else *bad*).  A match that would have elements but whose K14 priors do not resolve through
// player_prior (fp32, as the scorecard resolves them) has none and counts as *inconsistent*.  A
// match one of whose slots is bad keeps the initial messages of its other elements for good: its
// factor cannot be formed without that slot's cavity, so it is never run (it is *frozen*).
//
// Chain.  s_0 ~ N(m0, P0), s_t = s_{t-1} + N(0, q), q = tau^2, the walk before every element;
// (m0, P0) the resolved prior of the chain's first element.  Every element holds a likelihood
// message l_t = (h, pi) in natural parameters, pi >= 0.
//   forward   f_1 = N(m0, P0 + q), f_{t+1} = walk(f_t l_t)
//   backward  b_n flat, b_t = walk(b_{t+1} l_{t+1}); in information form walk is (h, pi) / (1 + q pi)
//   cavity    c_t = f_t b_t            marginal  f_t l_t b_t
//
// Match factor.  Every live slot takes the cavity (mu_c, s2) of its player's element (a twin's
// earlier slot too; it gets no message).  d = sum mu_c | roster 0 - sum mu_c | roster 1,
// c2 = n beta^2 + sum s2 (no tau^2: it is in the chain), (a, wf) = update_coef(d, c2), g = wf / c2:
//   pi_l = g / (1 - s2 g)        h_l = (a + mu_c g) / (1 - s2 g)
// which is the closed-form posterior (rate_core.h apply_coef) divided by the cavity, without the
// cancellation of forming that quotient.  A message that comes out non-finite or negative keeps
// the old one.  Damping: l <- (1 - theta) l + theta l_new, theta == 1 stores l_new itself.
//
// Initial messages: the filter's own, pi = 1 / s'^2 - 1 / (s_pre^2 + q), h = mu' / s'^2 -
// mu_pre / (s_pre^2 + q); pi < 0 or anything non-finite gives (0, 0) and counts as *flat*.
//
// The scan element (device only; the mirror runs the recursions above as loops) is the 1-D
// element of the parallel Kalman smoother (Sarkka & Garcia-Fernandez 2021), TttEl (A, b, C, eta,
// J): "N(x_out; A x_in + b, C) exp(eta x_in - J x_in^2 / 2)".  Element t is (1, 0, q, h_t, pi_t):
// observe l_t, then walk.  ttt_combine(i, j), i EARLIER IN TIME, with d = 1 + C_i J_j:
//   A = A_j A_i / d                      b = A_j (b_i + C_i eta_j) / d + b_j
//   C = A_j^2 C_i / d + C_j              eta = A_i (eta_j - J_j b_i) / d + eta_i
//   J = A_i^2 J_j / d + J_i
// associative, identity (1, 0, 0, 0, 0), exact against the identity on either side.  Behind the
// seed (0, m0, P0 + q, 0, 0) the composite of elements 1 .. t-1 holds f_t as (b, C), and A == 0
// exactly -- a state without a seed has A > 0, which is how "nothing lies in front" is told from
// a seed.  The composite of t+1 .. n holds b_t as (eta, J) / (1 + q J).  Both scans are
// exclusive, run as the inclusive scan over shifted terms (an element contributes the element
// before it, as K14's priors); the backward one runs on K16's mirrored order, newest first,
// where ttt_scan_combine_back is the only place the two orders meet.  Every entry stays bounded:
// A decays, C <= C_j + C_i, J <= J_i + 1 / C_i.
//
// Arithmetic is fp64, every operation the IEEE one written (ttt.hip is built with
// -ffp-contract=off); outputs are rounded once to fp32.  The tolerance the tests hold both paths
// to is measured against a 50-digit oracle (tests/through_time_cases.py E64).
#pragma once

#include <math.h>
#include <stdint.h>

#include "common.h"
#include "hindsight_core.h"
#include "rate_core.h"
#include "score_core.h"

namespace ana {

constexpr uint32_t kTttActive = 1u << 31;  // match word: its factor runs (elements, none bad)
constexpr int kTttCounters = 3;            // bad, flat, inconsistent

struct TttEl {
  double A, b, C, eta, J;
};

ANA_HD TttEl ttt_identity() { return TttEl{1.0, 0.0, 0.0, 0.0, 0.0}; }
ANA_HD TttEl ttt_element(double h, double pi, double q) { return TttEl{1.0, 0.0, q, h, pi}; }
ANA_HD TttEl ttt_seed(double m, double v) { return TttEl{0.0, m, v, 0.0, 0.0}; }

// i earlier in time
ANA_HD TttEl ttt_combine(const TttEl& i, const TttEl& j) {
  const double d = 1.0 + i.C * j.J;
  TttEl o;
  o.A = j.A * i.A / d;
  o.b = j.A * (i.b + i.C * j.eta) / d + j.b;
  o.C = (j.A * j.A) * i.C / d + j.C;
  o.eta = i.A * (j.eta - j.J * i.b) / d + i.eta;
  o.J = (i.A * i.A) * j.J / d + i.J;
  return o;
}

// x earlier in the backward scan, which runs newest first: x is the later one in time
ANA_HD TttEl ttt_scan_combine_back(const TttEl& x, const TttEl& y) { return ttt_combine(y, x); }

// the filter's own message of an element: posterior (mu', s') over the walked prior (mu_pre, v_pre)
ANA_HD bool ttt_initial_message(float mu, float sigma, double mu_pre, double v_pre, double& h, double& pi) {
  const double m = (double)mu, s = (double)sigma, p = s * s;
  pi = 1.0 / p - 1.0 / v_pre;
  h = m / p - mu_pre / v_pre;
  if (isfinite(pi) && isfinite(h) && pi >= 0.0) return true;
  h = pi = 0.0;
  return false;
}

// b_t from the composite of the elements after t
ANA_HD void ttt_backward_of(const TttEl& s, double q, double& h, double& pi) {
  const double w = 1.0 + q * s.J;
  h = s.eta / w;
  pi = s.J / w;
}

// cavity (mu_c, s2) = f b and the marginal (mu, var) = f l b, f as (mean, variance)
ANA_HD void ttt_beliefs(double fm, double fv, double hb, double pib, double hl, double pil, double& mu_c, double& s2,
                        double& mu, double& var) {
  const double pc = 1.0 / fv + pib, hc = fm / fv + hb;
  mu_c = hc / pc;
  s2 = 1.0 / pc;
  const double pm = pc + pil;
  mu = (hc + hl) / pm;
  var = 1.0 / pm;
}

// the message of an element with cavity (mu_c, s2) and roster coefficient a; false: keep the old one
ANA_HD bool ttt_factor_message(double a, double g, double mu_c, double s2, double& h, double& pi) {
  const double den = 1.0 - s2 * g;
  pi = g / den;
  h = (a + mu_c * g) / den;
  return isfinite(pi) && isfinite(h) && pi >= 0.0;
}

ANA_HD double ttt_damp(double old, double fresh, double theta) {
  return theta == 1.0 ? fresh : (1.0 - theta) * old + theta * fresh;
}

// One match at the start of a fit.  r: its record; st: its row's status byte; pr [4][2K]: its K14
// priors, field-major; mu, sg [2K]: the filtered values of the track; attrs [P][4] (may be null).
// Calls element(j, h, pi, m_pre, v_pre) for every element slot j: its initial message and its
// walked prior.  Returns the match word: the element mask | kTttActive; adds to cnt [bad, flat,
// inconsistent].
template <int K, class Element>
ANA_HD uint32_t ttt_setup_match(const int32_t* r, int64_t P, uint32_t st, const float* pr, const float* mu,
                                const float* sg, const float* attrs, const float* vst, float us, int track, int mode,
                                double q, int32_t* cnt, Element&& element) {
  constexpr int S = 2 * K;
  const uint32_t live = prior_live_mask<K>(r, P);
  uint32_t elems = hs_element_mask<K>(r, live, st, track, mode);
  if (!elems) return 0u;
  float pm[S], ps[S];  // the resolved prior of the track
  bool resolved = true;
#pragma unroll
  for (int j = 0; j < S; ++j) {
    pm[j] = ps[j] = NAN;
    if (!((live >> j) & 1u)) continue;
    float attr[4] = {NAN, NAN, NAN, 0.f};
    if (pr[j] != pr[j] && attrs != nullptr) {  // seeding only: a NULL shared track
      const float* a = attrs + (int64_t)r[j] * 4;
      attr[0] = a[0];
      attr[1] = a[1];
      attr[2] = a[2];
    }
    uint32_t flags;
    float ms = NAN, ss = NAN, mm = NAN, sm = NAN;
    if (player_prior<float>(pr[j], pr[S + j], pr[2 * S + j], pr[3 * S + j], attr, us, vst, ms, ss, mm, sm, flags) !=
        kRated)
      resolved = false;
    pm[j] = track == kHsMode ? mm : ms;
    ps[j] = track == kHsMode ? sm : ss;
  }
  if (!resolved) {
    ++cnt[2];
    return 0u;
  }
  uint32_t word = kTttActive;
#pragma unroll
  for (int j = 0; j < S; ++j) {
    if (!((elems >> j) & 1u)) continue;
    if (!hs_value_ok(mu[j], sg[j])) {
      elems &= ~(1u << j);
      word = 0u;
      ++cnt[0];
      continue;
    }
    const double m_pre = (double)pm[j], s_pre = (double)ps[j], v_pre = s_pre * s_pre + q;
    double h, pi;
    if (!ttt_initial_message(mu[j], sg[j], m_pre, v_pre, h, pi)) ++cnt[1];
    element(j, h, pi, m_pre, v_pre);
  }
  return elems ? word | elems : 0u;
}

// The factor of one active match.  r: its record; elems: its element mask; cavity(j, mu_c, s2)
// loads the cavity of element slot j; message(j, h, pi) takes the new message of element slot j
// (only called when it is to be stored).
template <int K, class Cavity, class Message>
ANA_HD void ttt_match_factor(const int32_t* r, int64_t P, uint32_t elems, double beta2, Cavity&& cavity,
                             Message&& message) {
  constexpr int S = 2 * K;
  const uint32_t live = prior_live_mask<K>(r, P);
  const uint32_t m1 = (uint32_t)r[S + 1];
  double mc[S], s2[S];
#pragma unroll
  for (int j = 0; j < S; ++j) {
    mc[j] = s2[j] = 0.0;
    if ((elems >> j) & 1u) cavity(j, mc[j], s2[j]);
  }
  // a twin's earlier slot: the cavity of the player's element, its last slot
#pragma unroll
  for (int i = 0; i < S - 1; ++i) {
#pragma unroll
    for (int j = i + 1; j < S; ++j) {
      if (((live >> i) & 1u) && ((elems >> j) & 1u) && r[i] == r[j]) {
        mc[i] = mc[j];
        s2[i] = s2[j];
      }
    }
  }
  double d = 0.0, sum = 0.0;
  int n = 0;
#pragma unroll
  for (int j = 0; j < S; ++j) {
    if (!((live >> j) & 1u)) continue;
    ++n;
    sum += s2[j];
    d += j < K ? mc[j] : -mc[j];
  }
  const UpdCoef<double> k =
      update_coef<double>(d, (double)n * beta2 + sum, meta_winner0(m1) ? 0 : 1, meta_winner1(m1) ? 0 : 1);
  const double g = k.wf / k.c2;
#pragma unroll
  for (int j = 0; j < S; ++j) {
    if (!((elems >> j) & 1u)) continue;
    double h, pi;
    if (ttt_factor_message(j < K ? k.a0 : k.a1, g, mc[j], s2[j], h, pi)) message(j, h, pi);
  }
}

}  // namespace ana
