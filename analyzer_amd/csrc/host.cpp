// Host (CPU) mirror of the engine: the same per-match core as the MI355X
// kernels, run sequentially in stream order.  It is the exact-semantics oracle
// for the device dataflow executor (fp64 by default) and the CPU path for the
// plumbing configuration (BASELINE config 1).  It is not a fallback for GPU
// tensors: device tensors always go to the HIP kernels.  Every mirror takes raw
// pointers, so the sanitized stand-alone self-test (tests/native) reaches all of them.
#include "host.h"

#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "career_core.h"
#include "expect_core.h"
#include "gen_core.h"
#include "hindsight_core.h"
#include "island_core.h"
#include "ladder_core.h"
#include "matchmake_core.h"
#include "pair_core.h"
#include "profile_core.h"
#include "rate_core.h"
#include "score_core.h"
#include "select_core.h"
#include "ttt_core.h"

namespace ana {

void host_gen_roster(const GenRosterParams& g, float* state, float* attrs) {
  for (int64_t p = 0; p < g.num_players; ++p) gen_player(g, p, state + p * kRowFloats, attrs + p * 4);
}

template <int K>
static void gen_stream_k(const GenStreamParams& g, int32_t* rec, int64_t M) {
  for (int64_t m = 0; m < M; ++m) gen_match<K>(g, m, rec + m * (2 * K + 2));
}

int host_gen_stream(int K, const GenStreamParams& g, int32_t* rec, int64_t M) {
  return with_team_size(K, [&](auto k) { gen_stream_k<decltype(k)::value>(g, rec, M); }) ? 0 : -1;
}

// Same outputs as the device schedule (common.h kLinkWords): link[slot] =
// next match of the player | has-earlier flag; deps[m].  Slots of matches that
// rate nothing are left unwritten.
template <int K>
static void schedule_k(const int32_t* rec, int64_t M, int64_t P, uint32_t* link, int32_t* deps) {
  constexpr int S = 2 * K;
  std::vector<uint32_t> last((size_t)P, kNone);
  for (int64_t m = 0; m < M; ++m) {
    MatchWork<float, K> w;
    decode_record<float, K>(rec + m * (S + 2), P, w);
    deps[m] = 0;
    if (w.status != kRated) continue;
    for (int j = 0; j < S; ++j) {
      if (w.id[j] < 0) continue;
      const uint32_t slot = (uint32_t)(m * S + j);
      const size_t p = (size_t)w.id[j];
      link[slot] = kNoMatch;
      if (last[p] != kNone) {
        link[last[p]] = (link[last[p]] & ~kMatchMask) | (uint32_t)m;
        link[slot] |= kLinkHasPred;
        if (w.first[j] == j) ++deps[m];
      }
      last[p] = slot;
    }
  }
}

void host_gen_event_counts(const GenEventParams& g, int64_t base, int64_t M, int64_t* counts) {
  for (int64_t m = 0; m < M; ++m) counts[m] = gen_event_count(g, (uint64_t)(base + m));
}

int host_gen_events(int K, const GenEventParams& g, int64_t base, const int32_t* rec,
                    const int64_t* evoff, int64_t M, int32_t* events) {
  if (K < 1 || K > kMaxTeamSize) return -1;
  const int S = 2 * K;
  for (int64_t m = 0; m < M; ++m) {
    const uint32_t m0 = (uint32_t)rec[m * (S + 2) + S];
    const int n0 = meta_n0(m0) < K ? meta_n0(m0) : K, n1 = meta_n1(m0) < K ? meta_n1(m0) : K;
    for (int64_t e = evoff[m]; e < evoff[m + 1]; ++e) {
      int32_t* ev = events + e * 2;
      gen_event(g, (uint64_t)(base + m), e - evoff[m], (int32_t)m, n0 + n1, ev);
      const int r = event_slot(ev[0]);
      ev[0] = (ev[0] & ~0xff) | (r < n0 ? r : K + (r - n0));
    }
  }
  return 0;
}

int64_t host_telemetry(int K, const TelemetryParams& tp) {
  const int S = 2 * K;
  const int64_t M = tp.num_matches;
  int64_t bad = 0;
  for (int64_t i = 0; i < M * S * kStatFeatures; ++i) tp.stats[i] = 0.f;
  for (int64_t m = 0; m < M; ++m)
    for (int64_t e = tp.evoff[m]; e < tp.evoff[m + 1]; ++e) {
      const int32_t* ev = tp.events + e * 2;
      const int slot = event_slot(ev[0]);
      if (event_tag(ev[0]) != (uint32_t)(m & 0xffff) || slot >= S) {  // strict attribution
        ++bad;
        continue;
      }
      float value, add;
      memcpy(&value, ev + 1, 4);
      const int f = event_feature(event_type(ev[0]), value, add);
      float* row = tp.stats + ((int64_t)m * S + slot) * kStatFeatures;
      if (f >= 0) row[f] += add;
      row[kStatEvents] += 1.f;
    }
  return bad;
}

template <int K>
static int64_t levels_k(const int32_t* rec, int64_t M, int64_t P, int32_t* level) {
  constexpr int S = 2 * K;
  std::vector<int32_t> last((size_t)P, 0);
  int64_t depth = 0;
  for (int64_t m = 0; m < M; ++m) {
    MatchWork<float, K> w;
    decode_record<float, K>(rec + m * (S + 2), P, w);
    level[m] = 0;
    if (w.status != kRated) continue;
    int32_t l = 0;
    for (int j = 0; j < S; ++j)
      if (w.id[j] >= 0 && last[(size_t)w.id[j]] > l) l = last[(size_t)w.id[j]];
    ++l;
    for (int j = 0; j < S; ++j)
      if (w.id[j] >= 0) last[(size_t)w.id[j]] = l;
    level[m] = l;
    if (l > depth) depth = l;
  }
  return depth;
}

int64_t host_levels(int K, const int32_t* rec, int64_t M, int64_t P, int32_t* level) {
  int64_t depth = -1;
  with_team_size(K, [&](auto k) { depth = levels_k<decltype(k)::value>(rec, M, P, level); });
  return depth;
}

int host_schedule(int K, const int32_t* rec, int64_t M, int64_t P, uint32_t* link, int32_t* deps) {
  return with_team_size(K, [&](auto k) { schedule_k<decltype(k)::value>(rec, M, P, link, deps); }) ? 0 : -1;
}

template <typename T, int K>
static void rate_k(const int32_t* rec, float* state, const float* attrs, float* first_prior,
                   const RateOut& out, const RateParams& prm) {
  constexpr int S = 2 * K;
  const T beta2 = (T)prm.beta2, tau2 = (T)prm.tau2, us = (T)prm.unknown_sigma;
  for (int64_t m = 0; m < prm.num_matches; ++m) {
    MatchWork<T, K> w;
    decode_record<T, K>(rec + m * (S + 2), prm.num_players, w);
    uint32_t nulls = 0;
    if (w.status == kRated) {
      uint8_t st = kRated;
      for (int j = 0; j < S && st == kRated; ++j) {
        if (w.first[j] != j) continue;
        const float* row = state + (int64_t)w.id[j] * kRowFloats;
        const float* gm = row + 4 * (1 + w.mode);
        st = make_prior<T, K>(w, j, (T)row[0], (T)row[2], (T)gm[0], (T)gm[2],
                              attrs + (int64_t)w.id[j] * 4, us, prm.vst, nulls);
      }
      w.status = st;
      if (st == kRated) {
        copy_dup_priors<T, K>(w);
        rate_priors<T, K>(w, beta2, tau2);
      }
    }
    const bool rated = w.status == kRated;
    if (rated) {
      for (int j = 0; j < S; ++j) {
        if (w.id[j] < 0) continue;
        float* row = state + (int64_t)w.id[j] * kRowFloats;
        float* gm = row + 4 * (1 + w.mode);
        if ((w.last >> j) & 1u) {  // host mirror writes tag 0 (never a live device tag)
          row[0] = (float)w.ns_mu[j];
          row[2] = (float)w.ns_sig[j];
          gm[0] = (float)w.nm_mu[j];
          gm[2] = (float)w.nm_sig[j];
          row[1] = row[3] = gm[1] = gm[3] = 0.f;
        }
        if (prm.record_first_prior && first_prior && w.first[j] == j) {
          float* fp = first_prior + (int64_t)w.id[j] * kRowFloats;
          if ((nulls >> (2 * j)) & 1u) { fp[0] = (float)w.ms[j]; fp[2] = (float)w.ss[j]; }
          if ((nulls >> (2 * j + 1)) & 1u) {
            fp[4 * (1 + w.mode)] = (float)w.mm[j];
            fp[4 * (1 + w.mode) + 2] = (float)w.sm[j];
          }
        }
      }
    }
    const bool afkish = w.status == kAfk || w.status == kInvalidRosters;
    out.quality[m * out.qrow] = rated ? (float)w.quality : (afkish ? 0.f : NAN);
    out.status[m * out.srow] = w.status;
    for (int j = 0; j < S; ++j) {
      const bool on = rated && w.id[j] >= 0;
      out.s_mu[m * out.row + j] = on ? (float)w.ns_mu[j] : NAN;
      out.s_sig[m * out.row + j] = on ? (float)w.ns_sig[j] : NAN;
      out.delta[m * out.row + j] = on ? (float)w.delta[j] : NAN;
      out.m_mu[m * out.row + j] = on ? (float)w.nm_mu[j] : NAN;
      out.m_sig[m * out.row + j] = on ? (float)w.nm_sig[j] : NAN;
    }
  }
}

template <typename T>
static int rate_t(int K, const int32_t* rec, float* state, const float* attrs, float* first_prior,
                  const RateOut& out, const RateParams& prm) {
  const bool known =
      with_team_size(K, [&](auto k) { rate_k<T, decltype(k)::value>(rec, state, attrs, first_prior, out, prm); });
  return known ? 0 : -1;
}

int host_rate(int K, bool fp64, const int32_t* rec, float* state, const float* attrs,
              float* first_prior, const RateOut& out, const RateParams& prm) {
  return fp64 ? rate_t<double>(K, rec, state, attrs, first_prior, out, prm)
              : rate_t<float>(K, rec, state, attrs, first_prior, out, prm);
}

}  // namespace ana

#include "sweep_core.h"

namespace ana {

// s0, a, s2: base rows [P][kBaseFloats] (sweep_core.h); s: roster rows [P][32]
void host_sweep_delta(const float* s0, const float* a, const float* s, const float* attrs,
                      const float* vst, float unknown_sigma, bool scaled, float* buf, int64_t P) {
  for (int64_t p = 0; p < P; ++p)
    sweep_delta_player(s0 + p * kBaseFloats, a + p * kBaseFloats, s + p * kRowFloats, attrs + p * 4,
                       vst, unknown_sigma, scaled, buf + p * 16);
}

void host_sweep_apply(const float* s0, const float* buf, const float* attrs, float* s, float* s2,
                      bool scaled, const float* vst, float unknown_sigma, int64_t P, uint32_t* clamps) {
  for (int64_t p = 0; p < P; ++p) {
    float ob[kBaseFloats];
    sweep_apply_player(s0 + p * kBaseFloats, buf + p * 16, attrs + p * 4, vst, unknown_sigma, scaled,
                       s + p * kRowFloats, ob, clamps);
    if (s2)
      for (int k = 0; k < kBaseFloats; ++k) s2[p * kBaseFloats + k] = ob[k];
  }
}

void host_correct_records(int K, const int32_t* rec, int64_t M, float* rows, int64_t orow, const float* delta,
                          int64_t P) {
  const int S = 2 * K;
  for (int64_t m = 0; m < M; ++m) {
    float* row = rows + m * orow;
    if (reinterpret_cast<const uint8_t*>(row + 5 * S + 1)[0] != kRated) continue;
    const int32_t* r = rec + m * (S + 2);
    const uint32_t m0 = (uint32_t)r[S];
    const int t = 1 + meta_mode(m0);
    for (int j = 0; j < S; ++j) {
      if ((j < K ? j : j - K) >= (j < K ? meta_n0(m0) : meta_n1(m0))) continue;
      const int32_t p = r[j];
      if (p < 0 || p >= P) continue;
      const float* d = delta + (int64_t)p * 16;
      correct_record_track(d[0], d[1], row[j], row[S + j]);
      correct_record_track(d[2 * t], d[2 * t + 1], row[3 * S + j], row[4 * S + j]);
    }
  }
}

void host_prefix_delta(const float* s0, const float* prefix, const float* attrs, const float* vst,
                       float unknown_sigma, float* delta, int64_t P) {
  for (int64_t p = 0; p < P; ++p)
    prefix_delta_player(s0 + p * kBaseFloats, prefix + p * 14, attrs + p * 4, vst, unknown_sigma, delta + p * 16);
}

// C2 exchange (sweep.hip pack_rows / unpack_rows / check_round): entries of 33 words, the
// roster row of a rated match's slot and its player id (-1: no row)
int host_pack_rows(const int32_t* rec, int K, int64_t m, const uint8_t* status, int64_t sstride, const float* state,
                   int64_t P, float* out, int64_t cap) {
  if (K < 1 || K > kMaxTeamSize) return -1;
  const int S = 2 * K;
  for (int64_t e = 0; e < cap; ++e) {
    int32_t id = -1;
    if (e < m * S) {
      const int64_t i = e / S;
      const int j = (int)(e % S);
      const uint32_t m0 = (uint32_t)rec[i * (S + 2) + S];
      const int n = j < K ? meta_n0(m0) : meta_n1(m0);
      const int32_t v = rec[i * (S + 2) + j];
      if (status[i * sstride] == kRated && (j < K ? j : j - K) < n && v >= 0 && v < P) id = v;
    }
    float* o = out + e * 33;
    if (id >= 0) memcpy(o, state + (int64_t)id * kRowFloats, kRowFloats * sizeof(float));
    memcpy(o + kRowFloats, &id, 4);
  }
  return 0;
}

// rows of the entries with an id in 0..P-1 into the roster, tags zeroed
void host_unpack_rows(const float* buf, int64_t n, float* state, int64_t P) {
  for (int64_t e = 0; e < n; ++e) {
    const float* b = buf + e * 33;
    int32_t id;
    memcpy(&id, b + kRowFloats, 4);
    if (id < 0 || id >= P) continue;
    for (int k = 0; k < kRowFloats; ++k) state[(int64_t)id * kRowFloats + k] = (k & 1) ? 0.f : b[k];
  }
}

// owner[p] = (round + 1) << 32 | (match + 1) of the first match of the round that holds p
int host_check_round(const int32_t* rec, int K, const int64_t* idx, int64_t m, int64_t P, uint32_t round,
                     uint64_t* owner, int32_t* flag) {
  if (K < 1 || K > kMaxTeamSize) return -1;
  const int S = 2 * K;
  const uint64_t tag = (uint64_t)round + 1;
  for (int64_t i = 0; i < m; ++i) {
    const int32_t* r = rec + idx[i] * (S + 2);
    if (early_status_k(r, S, P) != kRated) continue;
    const uint32_t m0 = (uint32_t)r[S];
    const uint64_t mine = (tag << 32) | (uint64_t)(idx[i] + 1);
    for (int j = 0; j < S; ++j) {
      const int n = j < K ? meta_n0(m0) : meta_n1(m0);
      const int32_t p = r[j];
      if ((j < K ? j : j - K) >= n || p < 0 || p >= P) continue;
      if (owner[p] >> 32 == tag) {
        if (owner[p] != mine) flag[0] |= 1;
      } else {
        owner[p] = mine;
      }
    }
  }
  return 0;
}

void host_reset_tags(float* state, int64_t P) {
  for (int64_t i = 0; i < P * kRowFloats; i += 2) state[i + 1] = 0.f;
}

// K10: the device's three launches as one sequential walk (the order is the walk's)
template <int K>
static int64_t records_select_k(const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t base, int64_t P,
                                const uint32_t* bitmap, int32_t* hits) {
  constexpr int S = 2 * K;
  int64_t n = 0;
  for (int64_t m = 0; m < M; ++m) {
    const int32_t* r = rec + m * (S + 2);
    const uint32_t mask = select_mask<K>(r, P, bitmap);
    if (!mask) continue;  // the row is only read behind a bitmap hit
    uint32_t row[5 * S + 2];
    memcpy(row, rows + m * W, sizeof(row));
    const uint32_t st = select_row_status<K>(row);
    if (!select_status(st)) continue;
    for (int j = 0; j < S; ++j) {
      if (!((mask >> j) & 1u)) continue;
      if (hits != nullptr) select_hit<K>(r, row, base + m, j, st, hits + n * kHitWords);
      ++n;
    }
  }
  return n;
}

int64_t records_select_host(int K, const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t base,
                            int64_t P, const uint32_t* bitmap, int32_t* hits) {
  int64_t n = -1;
  with_team_size(K, [&](auto k) { n = records_select_k<decltype(k)::value>(rec, rows, W, M, base, P, bitmap, hits); });
  return n;
}

// K13: the games in (match, slot) order, each folded into its player's row as a run of one
template <int K>
static void careers_add_k(const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t base, int64_t P,
                          int32_t track, int32_t score, uint32_t modes, int32_t* table) {
  constexpr int S = 2 * K;
  for (int64_t m = 0; m < M; ++m) {
    const int32_t* r = rec + m * (S + 2);
    const uint32_t mask = career_mask<K>(r, P, modes);
    if (!mask) continue;  // the row is only read for a candidate
    uint32_t row[5 * S + 2];
    memcpy(row, rows + m * W, sizeof(row));
    const uint32_t st = select_row_status<K>(row);
    if (!select_status(st)) continue;
    const int f = career_field(track);
    for (int j = 0; j < S; ++j) {
      if (!((mask >> j) & 1u)) continue;
      uint32_t ev[kCareerEventWords];
      career_event<K>(r, j, st, row[f * S + j], row[(f + 1) * S + j], row[5 * S], score, ev);
      career_row_add(table + (int64_t)r[j] * kCareerWords, career_game(ev[0], ev[1], base + m));
    }
  }
}

int host_careers_add(int K, const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t base, int64_t P,
                     int track, int score, uint32_t modes, int32_t* table) {
  if (!window_ok(K, W, M, P) || base < 0 || !career_options_ok(track, score, modes)) return -1;
  return with_team_size(K, [&](auto k) {
    careers_add_k<decltype(k)::value>(rec, rows, W, M, base, P, track, score, modes, table);
  }) ? 0 : -1;
}

// K17: every game in (match, slot) order, added to its player's row and to its cell
template <int K>
static void profiles_add_k(const int32_t* rec, const float* rows, int64_t W, const float* stats, int64_t M, int64_t P,
                           int32_t track, int32_t score, uint32_t modes, const ProfileEdges& edges, int32_t* table,
                           int64_t* cells) {
  constexpr int S = 2 * K;
  for (int64_t m = 0; m < M; ++m) {
    const int32_t* r = rec + m * (S + 2);
    const uint32_t mask = career_mask<K>(r, P, modes);
    if (!mask) continue;  // the row is only read for a candidate
    uint32_t row[5 * S + 2];
    memcpy(row, rows + m * W, sizeof(row));
    if (select_row_status<K>(row) != kRated) continue;
    const int f = career_field(track), mode = meta_mode((uint32_t)r[S]);
    for (int j = 0; j < S; ++j) {
      if (!((mask >> j) & 1u)) continue;
      int32_t bad = 0;
      const ProfileRun g = profile_game(stats + (m * S + j) * kProfileStats, profile_won<K>(r, j), bad);
      profile_row_add(table + (int64_t)r[j] * kProfileWords, g);
      const float s = ladder_score(ladder_float(row[f * S + j]), ladder_float(row[(f + 1) * S + j]), score);
      profile_cell_add(edges, mode, s, g, bad, [&](int c, int64_t v) { cells[c] += v; });
    }
  }
}

int host_profiles_add(int K, const int32_t* rec, const float* rows, int64_t W, const float* stats, int64_t M,
                      int64_t P, int track, int score, uint32_t modes, const float* edges, int n_edges,
                      int32_t* table, int64_t* cells) {
  if (!window_ok(K, W, M, P) || !career_options_ok(track, score, modes) || n_edges < 0 || n_edges > kProfileMaxEdges)
    return -1;
  ProfileEdges pe;
  pe.n = n_edges;
  for (int i = 0; i < kProfileMaxEdges; ++i) pe.e[i] = i < n_edges ? edges[i] : 0.0f;
  for (int i = 0; i < n_edges; ++i)
    if (!isfinite(pe.e[i]) || (i > 0 && !(pe.e[i - 1] < pe.e[i]))) return -1;
  return with_team_size(K, [&](auto k) {
    profiles_add_k<decltype(k)::value>(rec, rows, W, stats, M, P, track, score, modes, pe, table, cells);
  }) ? 0 : -1;
}

// K15: every entry of every match, in (match, entry) order, added to its row of the ordered map
template <int K>
static void pairs_add_k(const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t P, uint32_t modes,
                        const uint32_t* bitmap, PairMap& table) {
  constexpr int S = 2 * K, E = pair_entries(K);
  for (int64_t m = 0; m < M; ++m) {
    const int32_t* r = rec + m * (S + 2);
    const uint32_t m0 = (uint32_t)r[S], m1 = (uint32_t)r[S + 1];
    if (!pair_mode_selected(m0, modes)) continue;
    bool rated = false, read = false;  // the row is only read for an entry that is live otherwise
    for (int q = 0; q < E; ++q) {
      int ja, jb;
      pair_slots<K>(q, ja, jb);
      const int32_t a = r[ja], b = r[jb];
      if (!pair_slot_live<K>(m0, ja, a, P) || !pair_slot_live<K>(m0, jb, b, P) || a == b) continue;
      if (!pair_filtered(bitmap, a)) continue;
      if (!read) {
        uint32_t st;
        memcpy(&st, rows + m * W + 5 * S + 1, sizeof(st));
        rated = (st & 0xffu) == kRated;
        read = true;
      }
      if (!rated) break;
      int32_t c[kPairWords];
      pair_counters(pair_flags<K>(m1, ja, jb), c);
      auto& row = table[pair_key((uint32_t)a, (uint32_t)b)];  // a new row is zeroed
      for (int d = 0; d < kPairWords; ++d) row[d] += c[d];
    }
  }
}

int host_pairs_add(int K, const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t P, uint32_t modes,
                   const uint32_t* bitmap, PairMap& table) {
  if (!window_ok(K, W, M, P) || (modes & ~kPairAllModes)) return -1;
  return with_team_size(K, [&](auto k) {
    pairs_add_k<decltype(k)::value>(rec, rows, W, M, P, modes, bitmap, table);
  }) ? 0 : -1;
}

void host_pairs_merge(const int64_t* keys, const int32_t* counts, int64_t n, PairMap& table) {
  for (int64_t i = 0; i < n; ++i) {
    auto& row = table[keys[i]];
    for (int d = 0; d < kPairWords; ++d) row[d] += counts[i * kPairWords + d];
  }
}

// K18: the sequential union-find.  -1 from find: a word outside [0, its index]
static int32_t island_find_host(int32_t* parent, int32_t x) {
  for (;;) {
    const int32_t p = parent[x];
    if (p == x) return x;
    if (!island_word_ok(p, x)) return -1;
    const int32_t g = parent[p];
    if (!island_word_ok(g, p)) return -1;
    parent[x] = g;  // path halving
    x = g;
  }
}

static bool island_unite_host(int32_t* parent, int32_t a, int32_t b) {
  a = island_find_host(parent, a);
  b = island_find_host(parent, b);
  if (a < 0 || b < 0) return false;
  if (a != b) parent[a > b ? a : b] = a > b ? b : a;
  return true;
}

template <int K>
static bool islands_add_k(const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t P, uint32_t modes,
                          int32_t* parent, int32_t* slots, int32_t* credit) {
  constexpr int S = 2 * K;
  for (int64_t m = 0; m < M; ++m) {
    const int32_t* r = rec + m * (S + 2);
    const uint32_t live = island_live_mask<K>(r, P, modes);
    if (live == 0u) continue;
    uint32_t st;
    memcpy(&st, rows + m * W + 5 * S + 1, sizeof(st));
    if ((st & 0xffu) != kRated) continue;
    int32_t first = -1;
    for (int j = 0; j < S; ++j) {
      if (!((live >> j) & 1u)) continue;
      const int32_t p = r[j];
      slots[p] += 1;
      if (first < 0) {
        first = p;
        credit[p] += 1;
      } else if (p != first && !island_unite_host(parent, first, p)) {
        return false;
      }
    }
  }
  return true;
}

int host_islands_add(int K, const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t P, uint32_t modes,
                     int32_t* parent, int32_t* slots, int32_t* credit) {
  if (!window_ok(K, W, M, P) || (modes & ~kIslandAllModes)) return -1;
  bool ok = true;
  const bool known = with_team_size(K, [&](auto k) {
    ok = islands_add_k<decltype(k)::value>(rec, rows, W, M, P, modes, parent, slots, credit);
  });
  return known && ok ? 0 : -1;
}

int host_islands_edges(const int32_t* a, const int32_t* b, int64_t n, int64_t P, int mark, int32_t* parent,
                       int32_t* slots, int64_t* ctrl) {
  if (n < 0 || P < 0 || P > 0x7fffffffll) return -1;
  for (int64_t i = 0; i < n; ++i) {
    if (a[i] < 0 || (int64_t)a[i] >= P || b[i] < 0 || (int64_t)b[i] >= P) {
      ctrl[1] += 1;
      continue;
    }
    if (mark) {
      slots[a[i]] = (int32_t)((uint32_t)slots[a[i]] | kIslandSeenBit);
      slots[b[i]] = (int32_t)((uint32_t)slots[b[i]] | kIslandSeenBit);
    }
    if (a[i] != b[i] && !island_unite_host(parent, a[i], b[i])) return -1;
  }
  return 0;
}

int host_islands_flatten(int32_t* parent, int64_t P) {
  if (P < 0 || P > 0x7fffffffll) return -1;
  for (int64_t i = 0; i < P; ++i) {  // ascending: parent[i] <= i is flat already when i is reached
    const int32_t p = parent[i];
    if (!island_word_ok(p, (int32_t)i)) return -1;
    parent[i] = parent[p];
  }
  return 0;
}

int host_islands_census(const int32_t* parent, const int32_t* slots, const int32_t* credit, int64_t P,
                        int64_t* census) {
  if (P < 0 || P > 0x7fffffffll) return -1;
  for (int64_t i = 0; i < P; ++i) {
    const uint32_t sw = (uint32_t)slots[i];
    if (sw == 0u) continue;
    const int32_t root = parent[i];
    if (!island_word_ok(root, (int32_t)i)) return -1;
    census[root] += 1;
    census[P + root] += credit[i];
    census[2 * P + root] += (int64_t)(sw & kIslandSlotMask);
  }
  return 0;
}

// K11: the device's three stages on one track -- keys in id order, a stable sort of the
// ids by key, ranks from the sorted positions (ladder_core.h)
int64_t host_ladder(const float* state, int64_t P, int track, int score, float max_sigma, int32_t* order,
                    float* score_out, int32_t* rank) {
  if (track < 0 || track >= kTracks || P < 0 || P > 0x7fffffffll ||
      (score != kLadderConservative && score != kLadderMu))
    return -1;
  std::vector<uint32_t> keys((size_t)P);
  std::vector<int32_t> ids((size_t)P);
  int64_t R = 0;
  for (int64_t p = 0; p < P; ++p) {
    const float* g = state + p * kRowFloats + 4 * track;
    keys[p] = ladder_key(g[0], g[2], score, max_sigma);
    ids[p] = (int32_t)p;
    R += keys[p] != kLadderUnranked;
  }
  std::stable_sort(ids.begin(), ids.end(), [&](int32_t a, int32_t b) { return keys[a] < keys[b]; });
  for (int64_t i = 0; i < P; ++i) {
    const int32_t id = ids[i];
    rank[id] = i < R ? (int32_t)i : -1;
    if (i < R) {
      order[i] = id;
      score_out[i] = ladder_key_score(keys[id]);
    }
  }
  return R;
}

// K12 / K14: what `rate` would make of one record against stored (mu, sigma) pairs, on
// rate_k's own code path (decode_record, the prior loop in slot order, copy_dup_priors,
// match_quality) in fp64, so status and quality are the bits host_rate writes.  raw(j, x) gives
// slot j's stored shared (mu, sigma) and mode-track (mu, sigma).  d and den are the sums
// p_win0 = win_probability(d, den) is made of, on the mode track or (shared) the shared one.
template <int K, class Raw>
static void preview_match(const int32_t* r, int64_t P, Raw&& raw, const float* attrs, const float* vst, double beta2,
                          double us, bool shared, MatchWork<double, K>& w, double& q, double& d, double& den) {
  constexpr int S = 2 * K;
  const float no_attr[4] = {NAN, NAN, NAN, 0.f};
  decode_record<double, K>(r, P, w);
  q = d = den = 0;
  if (w.status != kRated) return;
  uint8_t st = kRated;
  uint32_t nulls = 0;
  for (int j = 0; j < S && st == kRated; ++j) {
    if (w.first[j] != j) continue;
    double x[4];
    raw(j, x);
    st = make_prior<double, K>(w, j, x[0], x[1], x[2], x[3], attrs ? attrs + (int64_t)w.id[j] * 4 : no_attr, us, vst,
                               nulls);
  }
  w.status = st;
  if (st != kRated) return;
  copy_dup_priors<double, K>(w);
  if (w.n0 == 0 || w.n1 == 0) {
    w.status = kErrEmptyRoster;
    return;
  }
  q = match_quality<double, K>(w.mm, w.sm, w.n0, w.n1, beta2);
  double s2 = 0;
  bool finite = true;
  for (int j = 0; j < S; ++j) {
    const bool in0 = j < K && j < w.n0, in1 = j >= K && j - K < w.n1;
    if (!(in0 || in1)) continue;
    const double mu = shared ? w.ms[j] : w.mm[j], sg = shared ? w.ss[j] : w.sm[j];
    s2 += sg * sg;
    d += in0 ? mu : -mu;
    finite = finite && prior_finite<double>(w.ms[j], w.ss[j], w.mm[j], w.sm[j]);
  }
  den = (double)(w.n0 + w.n1) * beta2 + s2;
  if (!finite || !isfinite(q) || !isfinite(win_probability<double>(d, den))) w.status = kErrNumeric;
}

template <int K>
static void preview_k(const int32_t* rec, int64_t M, const float* state, const float* attrs, const float* vst,
                      int64_t P, double beta2, double us, int32_t* out) {
  constexpr int S = 2 * K;
  for (int64_t m = 0; m < M; ++m) {
    MatchWork<double, K> w;
    double q, d, den;
    preview_match<K>(
        rec + m * (S + 2), P,
        [&](int j, double* x) {
          const float* row = state + (int64_t)w.id[j] * kRowFloats;
          const float* gm = row + 4 * (1 + w.mode);
          x[0] = row[0], x[1] = row[2], x[2] = gm[0], x[3] = gm[2];
        },
        attrs, vst, beta2, us, false, w, q, d, den);
    const bool rated = w.status == kRated, afkish = w.status == kAfk || w.status == kInvalidRosters;
    const float qo = rated ? (float)q : afkish ? 0.f : NAN;
    const float po = rated ? (float)win_probability<double>(d, den) : NAN;
    int32_t* o = out + m * kPreviewWords;
    o[0] = (int32_t)w.status;
    o[1] = (int32_t)ladder_bits(qo);
    o[2] = (int32_t)ladder_bits(po);
    o[3] = 0;
  }
}

int host_preview(int K, const int32_t* rec, int64_t M, const float* state, const float* attrs, const float* vst,
                 int64_t P, float beta2, float unknown_sigma, int32_t* out) {
  if (M < 0 || P < 0 || P > 0x7fffffffll) return -1;
  const bool known = with_team_size(
      K, [&](auto k) { preview_k<decltype(k)::value>(rec, M, state, attrs, vst, P, beta2, unknown_sigma, out); });
  return known ? 0 : -1;
}

// K14: the chain walked in match order; every slot of a match reads before any of them writes
template <int K>
static void priors_add_k(const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t P, float* chain,
                         float* priors) {
  constexpr int S = 2 * K;
  uint32_t* ch = reinterpret_cast<uint32_t*>(chain);
  uint32_t* out = reinterpret_cast<uint32_t*>(priors);
  for (int64_t m = 0; m < M; ++m) {
    const int32_t* r = rec + m * (S + 2);
    const uint32_t live = prior_live_mask<K>(r, P);
    const int mode = meta_mode((uint32_t)r[S]);
    uint32_t* pr = out + m * (4 * S);
    for (int j = 0; j < S; ++j) {
      uint32_t w[4] = {kPriorNull, kPriorNull, kPriorNull, kPriorNull};
      if ((live >> j) & 1u) prior_pick(prior_from_chain(ch + (int64_t)r[j] * kBaseFloats), mode, w);
      for (int f = 0; f < 4; ++f) pr[f * S + j] = w[f];
    }
    if (!live) continue;  // the row is only read for a live slot
    uint32_t row[5 * S + 2];
    memcpy(row, rows + m * W, sizeof(row));
    if (select_row_status<K>(row) != kRated) continue;
    const uint32_t writes = prior_last_mask<K>(r, live);
    for (int j = 0; j < S; ++j) {
      if (!((writes >> j) & 1u)) continue;
      uint32_t* c = ch + (int64_t)r[j] * kBaseFloats;
      const PriorState s = prior_combine(prior_from_chain(c),
                                         prior_write(mode, row[j], row[S + j], row[3 * S + j], row[4 * S + j]));
      for (int i = 0; i < 2 * kTracks; ++i) c[i] = s.w[i];
    }
  }
}

int host_priors_add(int K, const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t P, float* chain,
                    float* priors) {
  if (!window_ok(K, W, M, P)) return -1;
  return with_team_size(K, [&](auto k) { priors_add_k<decltype(k)::value>(rec, rows, W, M, P, chain, priors); })
             ? 0 : -1;
}

// K16: the smoother's recursion, newest match first; the carry row of a player is the
// smoothed state of the element after the one at hand
template <int K>
static void hindsight_add_k(const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t P, double tau2,
                            int track, int mode, double* carry, float* out, int64_t* bad) {
  constexpr int S = 2 * K;
  for (int64_t m = M - 1; m >= 0; --m) {
    const int32_t* r = rec + m * (S + 2);
    float* o = out + m * (2 * S);
    for (int j = 0; j < 2 * S; ++j) o[j] = NAN;
    const uint32_t live = prior_live_mask<K>(r, P);
    if (!live) continue;  // the row is only read for a live slot
    uint32_t row[5 * S + 2];
    memcpy(row, rows + m * W, sizeof(row));
    const uint32_t elems = hs_element_mask<K>(r, live, select_row_status<K>(row), track, mode);
    const uint32_t* mu = row + (track == kHsMode ? 3 * S : 0);
    for (int j = 0; j < S; ++j) {
      if (!((elems >> j) & 1u)) continue;
      float m_t, s_t;
      memcpy(&m_t, mu + j, 4);
      memcpy(&s_t, mu + S + j, 4);
      if (!hs_value_ok(m_t, s_t)) {
        ++*bad;
        continue;
      }
      double* c = carry + (int64_t)r[j] * 2;
      double mh = (double)m_t, ph = (double)s_t * (double)s_t;
      if (c[0] == c[0]) {
        const double p_t = ph, g = hs_gain(p_t, tau2);
        mh = (double)m_t + g * (c[0] - (double)m_t);
        ph = p_t + (g * g) * (c[1] - p_t - tau2);
      }
      c[0] = mh;
      c[1] = ph;
      o[2 * j] = (float)mh;
      o[2 * j + 1] = (float)sqrt(ph);
    }
  }
}

int host_hindsight_add(int K, const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t P, double tau2,
                       int track, int mode, double* carry, float* out, int64_t* bad) {
  if (!window_ok(K, W, M, P) || !(tau2 >= 0.0) || !std::isfinite(tau2) || (track != kHsShared && track != kHsMode) ||
      (track == kHsMode && (mode < 0 || mode >= kModes)))
    return -1;
  return with_team_size(K, [&](auto k) {
    hindsight_add_k<decltype(k)::value>(rec, rows, W, M, P, tau2, track, mode, carry, out, bad);
  }) ? 0 : -1;
}

// K20: the schedule of ttt.hip as loops.  A chain is walked forwards and backwards by the
// recursions of ttt_core.h themselves; the device composes scan elements instead.
template <int K>
static int64_t ttt_fit_k(const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t P, const float* priors,
                         const float* attrs, const float* vst, float us, double beta2, double q, int track, int mode,
                         int64_t sweeps, double tol, double theta, float* out, double* cav, double* msg,
                         double* resid, int64_t* counters) {
  constexpr int S = 2 * K;
  const int64_t n = M * S;
  std::vector<uint32_t> mword((size_t)M);
  std::vector<double> prior((size_t)(2 * n)), fwd((size_t)(2 * n)), mu64((size_t)n);
  std::vector<int64_t> start((size_t)P + 2, 0);
  int32_t cnt[kTttCounters] = {0, 0, 0};
  for (int64_t i = 0; i < 2 * n; ++i) {
    out[i] = NAN;
    cav[i] = msg[i] = 0.0;
  }
  for (int64_t m = 0; m < M; ++m) {
    const int32_t* r = rec + m * (S + 2);
    uint32_t row[5 * S + 2];
    memcpy(row, rows + m * W, sizeof(row));
    float mu[S], sg[S];
    memcpy(mu, row + (track == kHsMode ? 3 * S : 0), sizeof(mu));
    memcpy(sg, row + (track == kHsMode ? 4 * S : S), sizeof(sg));
    mword[m] = ttt_setup_match<K>(r, P, select_row_status<K>(row), priors + m * (4 * S), mu, sg, attrs, vst, us, track,
                                  mode, q, cnt, [&](int j, double h, double pi, double m_pre, double v_pre) {
                                    const int64_t i = m * S + j;
                                    msg[2 * i] = h;
                                    msg[2 * i + 1] = pi;
                                    prior[2 * i] = m_pre;
                                    prior[2 * i + 1] = v_pre;
                                    ++start[(size_t)r[j] + 2];
                                  });
  }
  for (int c = 0; c < kTttCounters; ++c) counters[c] += cnt[c];
  // every player's elements in chronological order: order[start[p + 1] ...) once filled
  for (int64_t p = 0; p < P; ++p) start[(size_t)p + 2] += start[(size_t)p + 1];
  std::vector<int64_t> order((size_t)start[(size_t)P + 1]);
  for (int64_t m = 0; m < M; ++m)
    for (int j = 0; j < S; ++j)
      if ((mword[m] >> j) & 1u) order[(size_t)start[(size_t)rec[m * (S + 2) + j] + 1]++] = m * S + j;
  // now start[p + 1] is the end of p's chain and start[p] its begin
  auto chain_pass = [&](bool have_before) {
    double worst = 0.0;
    for (int64_t p = 0; p < P; ++p) {
      const int64_t a = start[(size_t)p], b = start[(size_t)p + 1];
      if (a == b) continue;
      double fm = prior[2 * order[a]], fv = prior[2 * order[a] + 1];
      for (int64_t t = a; t < b; ++t) {
        const int64_t i = order[t];
        fwd[2 * i] = fm;
        fwd[2 * i + 1] = fv;
        const double pi = 1.0 / fv + msg[2 * i + 1], h = fm / fv + msg[2 * i];
        fm = h / pi;
        fv = 1.0 / pi + q;
      }
      double hb = 0.0, pib = 0.0;
      for (int64_t t = b - 1; t >= a; --t) {
        const int64_t i = order[t];
        double mu, var;
        ttt_beliefs(fwd[2 * i], fwd[2 * i + 1], hb, pib, msg[2 * i], msg[2 * i + 1], cav[2 * i], cav[2 * i + 1], mu,
                    var);
        out[2 * i] = (float)mu;
        out[2 * i + 1] = (float)sqrt(var);
        if (have_before) worst = fmax(worst, fabs(mu - mu64[i]));
        mu64[i] = mu;
        const double hs = hb + msg[2 * i], ps = pib + msg[2 * i + 1], w = 1.0 + q * ps;
        hb = hs / w;
        pib = ps / w;
      }
    }
    return worst;
  };
  // Jacobi: a factor reads the cavities of the chain pass before and, to damp, its own old messages
  int64_t run = 0;
  for (int64_t k = 0;; ++k) {
    const double r = chain_pass(k > 0);
    if (k > 0) resid[k - 1] = r;
    if (k == sweeps || (k > 0 && tol >= 0.0 && r < tol)) break;
    for (int64_t m = 0; m < M; ++m) {
      if (!(mword[m] & kTttActive)) continue;
      ttt_match_factor<K>(
          rec + m * (S + 2), P, mword[m] & ~kTttActive, beta2,
          [&](int j, double& mu_c, double& s2) {
            mu_c = cav[2 * (m * S + j)];
            s2 = cav[2 * (m * S + j) + 1];
          },
          [&](int j, double h, double pi) {
            const int64_t i = m * S + j;
            msg[2 * i] = ttt_damp(msg[2 * i], h, theta);
            msg[2 * i + 1] = ttt_damp(msg[2 * i + 1], pi, theta);
          });
    }
    ++run;
  }
  return run;
}

int64_t host_ttt_fit(int K, const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t P,
                     const float* priors, const float* attrs, const float* vst, float unknown_sigma, double beta2,
                     double tau2, int track, int mode, int64_t sweeps, double tol, double theta, float* out,
                     double* cav, double* msg, double* resid, int64_t* counters) {
  if (!window_slots_ok(K, W, M, P) || !(tau2 >= 0.0) || !std::isfinite(tau2) || !(beta2 >= 0.0) ||
      !std::isfinite(beta2) || (track != kHsShared && track != kHsMode) ||
      (track == kHsMode && (mode < 0 || mode >= kModes)) || sweeps < 0 || !(theta > 0.0 && theta <= 1.0) ||
      vst == nullptr)
    return -1;
  int64_t run = -1;
  with_team_size(K, [&](auto k) {
    run = ttt_fit_k<decltype(k)::value>(rec, rows, W, M, P, priors, attrs, vst, unknown_sigma, beta2, tau2, track,
                                        mode, sweeps, tol, theta, out, cav, msg, resid, counters);
  });
  return run;
}

// K14: the prediction of every match from its priors, on preview's fp64 path, and its score
template <int K>
static void score_add_k(const int32_t* rec, const float* priors, const float* rows, int64_t W, int64_t M,
                        const float* attrs, const float* vst, int64_t P, double beta2, double us, int track,
                        uint32_t modes, int64_t* table, int32_t* pred) {
  constexpr int S = 2 * K;
  for (int64_t m = 0; m < M; ++m) {
    const int32_t* r = rec + m * (S + 2);
    const float* pr = priors + m * (4 * S);
    MatchWork<double, K> w;
    double q, d, den;
    preview_match<K>(
        r, P, [&](int j, double* x) { x[0] = pr[j], x[1] = pr[S + j], x[2] = pr[2 * S + j], x[3] = pr[3 * S + j]; },
        attrs, vst, beta2, us, track == kScoreShared, w, q, d, den);
    const uint32_t meta1 = (uint32_t)r[S + 1];
    const bool rated = w.status == kRated, w0 = meta_winner0(meta1), w1 = meta_winner1(meta1);
    const float pw = rated ? (float)win_probability<double>(d, den) : NAN;
    const float po = rated && w0 != w1 ? (float)win_probability<double>(w0 ? d : -d, den) : NAN;
    uint32_t row[5 * S + 2];
    memcpy(row, rows + m * W, sizeof(row));
    const uint32_t word = score_match(select_row_status<K>(row), (uint32_t)r[S], meta1, modes, w.status, pw, po,
                                      [&](int c, int64_t x) { table[c] += x; });
    if (pred != nullptr) {
      int32_t* o = pred + m * kPredWords;
      o[0] = (int32_t)word;
      o[1] = (int32_t)ladder_bits(pw);
      o[2] = (int32_t)ladder_bits(po);
      o[3] = 0;
    }
  }
}

int host_score_add(int K, const int32_t* rec, const float* priors, const float* rows, int64_t W, int64_t M,
                   const float* attrs, const float* vst, int64_t P, float beta2, float unknown_sigma, int track,
                   uint32_t modes, int64_t* table, int32_t* pred) {
  if (!window_ok(K, W, M, P) || (track != kScoreShared && track != kScoreMode) ||
      (modes & ~kScoreAllModes))
    return -1;
  return with_team_size(K, [&](auto k) {
    score_add_k<decltype(k)::value>(rec, priors, rows, W, M, attrs, vst, P, beta2, unknown_sigma, track, modes, table,
                                    pred);
  }) ? 0 : -1;
}

// K19: every game in (match, slot) order, its term record added to its player's row
template <int K>
static void expect_add_k(const int32_t* rec, const float* priors, const int32_t* pred, int64_t M, int64_t P,
                         int32_t track, int32_t* table, int64_t* bad) {
  constexpr int S = 2 * K;
  const uint32_t* pri = reinterpret_cast<const uint32_t*>(priors);
  for (int64_t m = 0; m < M; ++m) {
    const int32_t* r = rec + m * (S + 2);
    const int32_t* pr = pred + m * kPredWords;
    const uint32_t mask = expect_game_mask<K>(r, P, (uint32_t)pr[0], (uint32_t)pr[1]);
    if (!mask) continue;  // the priors are only read for a scored match
    const uint32_t* src = pri + m * (4 * S);
    uint32_t mu[S];
    for (int j = 0; j < S; ++j) mu[j] = expect_raw(track, src[j], src[2 * S + j]);
    *bad += expect_terms<K>(mask, (uint32_t)pr[1], (uint32_t)pr[2], mu, [&](int j, const int32_t* t) {
      expect_row_add(table + (int64_t)r[j] * kExpectWords, expect_game(t, profile_won<K>(r, j)));
    });
  }
}

int host_expect_add(int K, const int32_t* rec, const float* priors, const int32_t* pred, int64_t M, int64_t P,
                    int track, int32_t* table, int64_t* bad) {
  if (!window_ok(K, 5 * 2 * K + 2, M, P) || (track != kScoreShared && track != kScoreMode) || bad == nullptr)
    return -1;
  return with_team_size(K, [&](auto k) {
    expect_add_k<decltype(k)::value>(rec, priors, pred, M, P, track, table, bad);
  }) ? 0 : -1;
}

// fp32 player_prior of one player, as the device's load_prior
static uint8_t host_prior(const float* state, const float* attrs, const float* vst, float us, int32_t id, int mode,
                          float& ms, float& ss, float& mm, float& sm) {
  const float no_attr[4] = {NAN, NAN, NAN, 0.f};
  const float* row = state + (int64_t)id * kRowFloats;
  const float* gm = row + 4 * (1 + mode);
  uint32_t flags;
  ms = ss = mm = sm = NAN;
  float a, b, c, d;
  const uint8_t st = player_prior<float>(row[0], row[2], gm[0], gm[2], attrs ? attrs + (int64_t)id * 4 : no_attr, us,
                                         vst, a, b, c, d, flags);
  if (st == kRated) {
    ms = a;
    ss = b;
    mm = c;
    sm = d;
  }
  return st;
}

// the split choice in fp32 (matchmake_core.h: the device's bits); quality and p_win0 in fp64
template <int K>
static void balance_k(const int32_t* lobbies, int64_t L, const float* state, const float* attrs, const float* vst,
                      int64_t P, int mode, double beta2, float us, int32_t* out, int32_t* records) {
  constexpr int S = 2 * K, C = split_count(K);
  const int32_t meta0 = (int32_t)pack_meta0(mode, K, K, 2);
  for (int64_t l = 0; l < L; ++l) {
    const int32_t* ids = lobbies + l * S;
    bool bad = false, e_seed = false, e_sigma = false, e_num = false;
    for (int j = 0; j < S; ++j) {
      if (ids[j] < 0 || (int64_t)ids[j] >= P) bad = true;
      for (int i = 0; i < j; ++i)
        if (ids[i] == ids[j]) bad = true;
    }
    float mu[S] = {};
    double s2 = 0;
    for (int j = 0; j < S && !bad; ++j) {
      float ms, ss, mm, sm;
      const uint8_t st = host_prior(state, attrs, vst, us, ids[j], mode, ms, ss, mm, sm);
      e_seed = e_seed || st == kErrSeed;
      e_sigma = e_sigma || st == kErrSigma;
      e_num = e_num || !prior_finite<float>(ms, ss, mm, sm);
      mu[j] = mm;
      s2 += (double)sm * (double)sm;
    }
    uint32_t bb = 0xffffffffu, bi = 0;
    for (int c = 0; c < C; ++c) {
      const float d = split_d<K>(mu, kSplits<K>.mask[c]);
      e_num = e_num || !isfinite(d);
      if (split_abs_bits(d) < bb) {
        bb = split_abs_bits(d);
        bi = (uint32_t)c;
      }
    }
    const uint32_t mask = kSplits<K>.mask[bi];
    double db = 0, dg = 0;  // exact sums of the fp32 mus
    for (int j = 0; j < S; ++j) {
      db += ((mask >> j) & 1u) ? (double)mu[j] : -(double)mu[j];
      dg += j < K ? (double)mu[j] : -(double)mu[j];
    }
    const double den = (double)S * beta2 + s2;
    const double q = quality_from_sums<double>(S, s2, db, beta2), qg = quality_from_sums<double>(S, s2, dg, beta2);
    const double pw = win_probability<double>(db, den);
    const uint8_t st = bad ? kErrBadRecord
                       : e_seed ? kErrSeed
                       : e_sigma ? kErrSigma
                       : (e_num || !isfinite((float)q) || !isfinite((float)qg) || !isfinite((float)pw)) ? kErrNumeric
                                                                                                       : kRated;
    const bool ok = st == kRated;
    int32_t* o = out + l * kBalanceWords;
    o[0] = (int32_t)st;
    o[1] = ok ? (int32_t)bi : -1;
    o[2] = ok ? (int32_t)mask : 0;
    o[3] = (int32_t)ladder_bits(ok ? (float)q : NAN);
    o[4] = (int32_t)ladder_bits(ok ? (float)pw : NAN);
    o[5] = (int32_t)ladder_bits(ok ? (float)qg : NAN);
    o[6] = o[7] = 0;
    int32_t* r = records + l * (S + 2);
    for (int j = 0; j < S; ++j) r[ok ? split_position(mask, j, K) : j] = ids[j];
    r[S] = meta0;
    r[S + 1] = 0;
  }
}

int host_balance(int K, const int32_t* lobbies, int64_t L, const float* state, const float* attrs, const float* vst,
                 int64_t P, int mode, float beta2, float unknown_sigma, int32_t* out, int32_t* records) {
  if (L < 0 || P < 0 || P > 0x7fffffffll || mode < 0 || mode >= kModes) return -1;
  const bool known = with_team_size(K, [&](auto k) {
    balance_k<decltype(k)::value>(lobbies, L, state, attrs, vst, P, mode, beta2, unknown_sigma, out, records);
  });
  return known ? 0 : -1;
}

int host_queue_keys(const int32_t* queue, int64_t Q, const float* state, const float* attrs, const float* vst,
                    int64_t P, int mode, float unknown_sigma, uint32_t* keys, uint32_t* vals) {
  if (Q < 0 || Q > 0x7fffffffll || P < 0 || P > 0x7fffffffll || mode < 0 || mode >= kModes) return -1;
  for (int64_t i = 0; i < Q; ++i) {
    const int32_t id = queue[i];
    keys[i] = kLadderUnranked;
    vals[i] = (uint32_t)i;
    if (id < 0 || (int64_t)id >= P) continue;
    float ms, ss, mm, sm;
    const uint8_t st = host_prior(state, attrs, vst, unknown_sigma, id, mode, ms, ss, mm, sm);
    keys[i] = queue_key(st, mm);
  }
  return 0;
}

}  // namespace ana
