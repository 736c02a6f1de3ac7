// Host (CPU) mirror of the engine kernels; see host.cpp.
#pragma once

#include <stdint.h>

#include <array>
#include <map>

#include "common.h"
#include "gen_core.h"
#include "telemetry_core.h"

namespace ana {

void host_gen_roster(const GenRosterParams& g, float* state, float* attrs);
int host_gen_stream(int K, const GenStreamParams& g, int32_t* rec, int64_t M);
int host_schedule(int K, const int32_t* rec, int64_t M, int64_t P, uint32_t* link, int32_t* deps);
// K5 levelizer: level[m] = 1 + max level of the previous matches of m's players
// (1 for a player's first match), 0 for matches that touch no state.  Returns
// the number of levels (conflict-free rounds).
// K8 host mirror: generation (counts per match, then events given the CSR
// offsets) and aggregation into stats [M][2K][kStatFeatures].
void host_gen_event_counts(const GenEventParams& g, int64_t base, int64_t M, int64_t* counts);
int host_gen_events(int K, const GenEventParams& g, int64_t base, const int32_t* rec,
                    const int64_t* evoff, int64_t M, int32_t* events);
int64_t host_telemetry(int K, const TelemetryParams& tp);
int64_t host_levels(int K, const int32_t* rec, int64_t M, int64_t P, int32_t* level);
int host_rate(int K, bool fp64, const int32_t* rec, float* state, const float* attrs,
              float* first_prior, const RateOut& out, const RateParams& prm);

}  // namespace ana

namespace ana {
void host_sweep_delta(const float* s0, const float* a, const float* s, const float* attrs,
                      const float* vst, float unknown_sigma, bool scaled, float* buf, int64_t P);
// clamps (nullable): += decoded tracks whose merged precision hit the floor (sweep_core.h)
void host_sweep_apply(const float* s0, const float* buf, const float* attrs, float* s, float* s2,
                      bool scaled, const float* vst, float unknown_sigma, int64_t P, uint32_t* clamps = nullptr);
// causal record correction: rows [M][orow] += delta [P][16] (raw natural-parameter
// increments per track) of each slot's player; the delta table of a scaled prefix
// [P][14] (fp32) against the window start s0 [P][16]
void host_correct_records(int K, const int32_t* rec, int64_t M, float* rows, int64_t orow, const float* delta,
                          int64_t P);
void host_prefix_delta(const float* s0, const float* prefix, const float* attrs, const float* vst,
                       float unknown_sigma, float* delta, int64_t P);
// C2 exchange host mirrors (kernels.h launch_pack_rows / launch_unpack_rows / launch_check_round):
// out / buf are [cap][33] entries = a roster row + the player id (-1: none); state is [P][32].
// pack and check_round return -1 for a K out of range.
int host_pack_rows(const int32_t* rec, int K, int64_t m, const uint8_t* status, int64_t sstride, const float* state,
                   int64_t P, float* out, int64_t cap);
void host_unpack_rows(const float* buf, int64_t n, float* state, int64_t P);
int host_check_round(const int32_t* rec, int K, const int64_t* idx, int64_t m, int64_t P, uint32_t round,
                     uint64_t* owner, int32_t* flag);
// zero the dataflow tags of state [P][32]
void host_reset_tags(float* state, int64_t P);
// K10 host mirror (select_core.h): the hits of the bitmap's players in rec [M][2K+2] joined
// with rows [M][W], ascending (match, slot), bit-identical to the device.  Returns their
// number (-1: K out of range); hits == nullptr only counts.
int64_t records_select_host(int K, const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t base,
                            int64_t P, const uint32_t* bitmap, int32_t* hits);
// K11 host mirror (ladder_core.h): the ladder of one track (granule 0..6) of state [P][32]:
// order / score_out (the first R of [P] entries are written) and rank [P] (-1: unranked),
// bit-identical to the device.  Returns R, the number of ranked players (-1: bad arguments).
int64_t host_ladder(const float* state, int64_t P, int track, int score, float max_sigma, int32_t* order,
                    float* score_out, int32_t* rank);
// K13 host mirror (career_core.h): the games of rec [M][2K+2] joined with rows [M][W], in
// (match, slot) order, folded into table [P][kCareerWords], bit-identical to the device.
// -1: bad arguments.
int host_careers_add(int K, const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t base, int64_t P,
                     int track, int score, uint32_t modes, int32_t* table);
// K14 host mirror (score_core.h).  priors_add: the priors [M][4 * 2K] of rec [M][2K+2] joined with
// rows [M][W], walking chain [P][kBaseFloats] in match order and leaving it after the window,
// bit-identical to the device.  score_add: the prediction of every match from its priors on
// preview's fp64 path (so status and p_win0 are host_preview's bits) added into table
// [kModes][kScoreBins + 1][4]; pred (nullable) [M][kPredWords]; attrs may be null.  -1: bad arguments.
int host_priors_add(int K, const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t P, float* chain,
                    float* priors);
int host_score_add(int K, const int32_t* rec, const float* priors, const float* rows, int64_t W, int64_t M,
                   const float* attrs, const float* vst, int64_t P, float beta2, float unknown_sigma, int track,
                   uint32_t modes, int64_t* table, int32_t* pred);
// K15 host mirror (pair_core.h): a plain loop over matches and slot pairs into an ordered map
// from a << 32 | b to the four counters.  pairs_add adds the entries of rec [M][2K+2] joined with
// rows [M][W] (bitmap nullable), pairs_merge the rows of a table (keys [n], counts [n][4]); the
// map's rows in order are the device's (keys, counts), bit for bit.  -1: bad arguments.
using PairMap = std::map<int64_t, std::array<int32_t, 4>>;
int host_pairs_add(int K, const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t P, uint32_t modes,
                   const uint32_t* bitmap, PairMap& table);
void host_pairs_merge(const int64_t* keys, const int32_t* counts, int64_t n, PairMap& table);
// K16 host mirror (hindsight_core.h): the recursion itself, walked backwards over rec [M][2K+2]
// joined with rows [M][W] in fp64 -- not the composition of maps the device scans -- against
// carry [P][2] (mh, Ph; NaN: no later match), which is left at every player's oldest element.
// out [M][2K][2] fp32 (NaN where no element); *bad is incremented.  -1: bad arguments.
int host_hindsight_add(int K, const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t P, double tau2,
                       int track, int mode, double* carry, float* out, int64_t* bad);
// K20 host mirror (ttt_core.h): the same schedule as plain loops -- per chain the forward and
// backward recursions themselves, not the composition of scan elements the device runs -- over
// rec [M][2K+2] joined with rows [M][W] and the K14 priors [M][4][2K].  Runs at most `sweeps`
// sweeps (a chain pass, then the match factors) and a final chain pass; stops early after the
// chain pass whose residual is < tol (tol < 0: never).  out [M][2K][2] fp32 (NaN where no
// element), cav and msg [M * 2K][2] fp64 (the cavities of the last chain pass and the messages it
// ran on), resid [sweeps], counters [3] (bad, flat, inconsistent).  Returns the sweeps run, -1:
// bad arguments.
int64_t host_ttt_fit(int K, const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t P,
                     const float* priors, const float* attrs, const float* vst, float unknown_sigma, double beta2,
                     double tau2, int track, int mode, int64_t sweeps, double tol, double theta, float* out,
                     double* cav, double* msg, double* resid, int64_t* counters);
// K17 host mirror (profile_core.h): the games of rec [M][2K+2] joined with rows [M][W] and stats
// [M][2K][8], each added to its row of table [P][kProfileWords] and its cell of cells
// [profile_table_words(n_edges + 1)], bit-identical to the device.  -1: bad arguments.
int host_profiles_add(int K, const int32_t* rec, const float* rows, int64_t W, const float* stats, int64_t M,
                      int64_t P, int track, int score, uint32_t modes, const float* edges, int n_edges,
                      int32_t* table, int64_t* cells);
// K19 host mirror (expect_core.h): a plain loop over the matches of rec [M][2K+2] joined with the
// raw priors [M][4 * 2K] and the pred rows [M][kPredWords]; every game's term record is added to
// its row of table [P][kExpectWords] and the bad own values to *bad, bit-identical to the device.
// -1: bad arguments.
int host_expect_add(int K, const int32_t* rec, const float* priors, const int32_t* pred, int64_t M, int64_t P,
                    int track, int32_t* table, int64_t* bad);
// K18 host mirror (island_core.h): the plain sequential union-find -- find with path halving,
// the larger root hooked under the smaller -- over parent / slots / credit [P] and ctrl
// [kIslandCtrlWords], with the device's liveness rules and counters.  After host_islands_flatten
// parent is the device's, bit for bit; census [kIslandCensusRows][P] is added to.  -1: bad
// arguments, or a parent word outside [0, its index].
int host_islands_add(int K, const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t P, uint32_t modes,
                     int32_t* parent, int32_t* slots, int32_t* credit);
int host_islands_edges(const int32_t* a, const int32_t* b, int64_t n, int64_t P, int mark, int32_t* parent,
                       int32_t* slots, int64_t* ctrl);
int host_islands_flatten(int32_t* parent, int64_t P);
int host_islands_census(const int32_t* parent, const int32_t* slots, const int32_t* credit, int64_t P,
                        int64_t* census);
// K12 host mirror (matchmake_core.h); out / records as launch_preview / launch_balance /
// launch_queue_keys (kernels.h) lay them out; attrs may be null.  preview runs rate's own
// fp64 path (status and quality are the bits host_rate writes); balance chooses the split in
// fp32, bit-identical to the device, and computes quality and p_win0 in fp64.  -1: bad arguments.
int host_preview(int K, const int32_t* rec, int64_t M, const float* state, const float* attrs, const float* vst,
                 int64_t P, float beta2, float unknown_sigma, int32_t* out);
int host_balance(int K, const int32_t* lobbies, int64_t L, const float* state, const float* attrs, const float* vst,
                 int64_t P, int mode, float beta2, float unknown_sigma, int32_t* out, int32_t* records);
int host_queue_keys(const int32_t* queue, int64_t Q, const float* state, const float* attrs, const float* vst,
                    int64_t P, int mode, float unknown_sigma, uint32_t* keys, uint32_t* vals);
}  // namespace ana
