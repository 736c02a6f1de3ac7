// Host-callable launchers of the MI355X kernels (implemented in kernels.hip).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime_api.h>

#include "common.h"
#include "gen_core.h"
#include "telemetry_core.h"

namespace ana {

int launch_gen_roster(const GenRosterParams& g, float* state, float* attrs, hipStream_t s);
int launch_gen_stream(int K, const GenStreamParams& g, int32_t* rec, int64_t M, hipStream_t s);

int launch_reset_tags(float* state, int64_t P, hipStream_t s);
// read every roster row once (Infinity Cache warm-up in front of a rating launch);
// sink: >= 256 words, written only under a condition that is never true in practice
int launch_warm_rows(const float* state, int64_t P, uint32_t* sink, hipStream_t s);
// e[0] += 1 on the stream (the device epoch of graph replays, RateParams::epoch_ptr)
int launch_epoch_bump(int32_t* e, hipStream_t s);
// DP pricing on one GPU: an all-reduce stand-in over `bytes` of `buf` (unchanged) on
// `channels` workgroups, `passes` streams of the buffer, held at least `us` microseconds
int launch_emulate_allreduce(void* buf, int64_t bytes, int channels, int passes, double us, hipStream_t s);

size_t schedule_workspace_bytes(int64_t nslots, int64_t num_players);

// Deterministic per-window digest of the packed output rows [M, W] (digest.hip):
// out[3 + 10K] fp64 = matches with records, participant records, the NaN-skipping
// column sums of s_mu / s_sig / delta / m_mu / m_sig per slot, the quality sum.
// scratch: records_digest_scratch_doubles(K) doubles.  hist (nullable) int64[256]:
// the window's status counts are ADDED to it (the run's running status histogram).
size_t records_digest_scratch_doubles(int K);
int launch_records_digest(int K, const float* rows, int64_t M, int64_t W, double* scratch, double* out,
                          int64_t* hist, hipStream_t s);

// Tile offsets (scan.hip): offsets [tiles + 1] (8-B aligned) = the exclusive scan of counts
// [tiles] read as unsigned, in 64 bits, the total last; one workgroup.  tiles == 0 writes
// offsets[0] = 0.  K10 and K15 run it between their count and emit launches.
int launch_tile_offsets(const uint32_t* counts, int64_t tiles, int64_t* offsets, hipStream_t s);

// K10 records_select (select.hip, select_core.h): the hits [n][kHitWords] int32 of the players
// of ``bitmap`` (uint32 [ceil(P / 32)]) in a window's records rec [M][2K+2] joined with its
// packed output rows [M][W], in ascending (match, slot) order; base: global index of match 0.
// rec and rows 16-B aligned (rec 8-B for K = 2, 4).  Two calls with one host read between them:
// count fills counts [tiles] and offsets [tiles + 1] (exclusive scan; the total last), emit
// writes hits [nhits] with nhits = offsets[tiles].
constexpr int kSelectTile = 2048;  // matches per workgroup
int64_t records_select_tiles(int64_t M);
int launch_records_select_count(int K, const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t P,
                                const uint32_t* bitmap, uint32_t* counts, int64_t* offsets, hipStream_t s);
int launch_records_select_emit(int K, const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t base,
                               int64_t P, const uint32_t* bitmap, const int64_t* offsets, int32_t* hits,
                               int64_t nhits, hipStream_t s);

// K11 ladder (ladder.hip, ladder_core.h).  ladder_keys: one pass over state [P][32] for the
// tracks of ``mask`` (bit t = granule t, 0..6); track slot j (the j-th set bit) gets its
// sort keys in keys[j * stride ..) and the identity permutation in ids[j * stride ..)
// (stride >= P, a multiple of 4 words; state, keys, ids 16-B aligned), and counts[j] its
// number of ranked players (counts: kTracks words, zeroed by the launch).  The pairs are
// sorted with launch_radix_sort_pairs (32 bits); ladder_ranks then turns one track's sorted
// (keys, ids) [P] and its count R into order [R], score [R] and rank [P].
constexpr int kLadderTile = 1024;  // players per workgroup
int launch_ladder_keys(const float* state, int64_t P, uint32_t mask, int score, float max_sigma, uint32_t* keys,
                       uint32_t* ids, int64_t stride, uint32_t* counts, hipStream_t s);
int launch_ladder_ranks(const uint32_t* keys, const uint32_t* ids, int64_t P, int64_t R, int32_t* order, float* score,
                        int32_t* rank, hipStream_t s);

// K12 matchmaking (matchmake.hip, matchmake_core.h); the roster is only read.  state [P][32]
// and attrs [P][4] 16-B aligned; attrs may be null ("no attributes": a NULL shared track is
// then kErrSeed); vst: kVstTiers floats.
// preview: per record of rec [M][2K+2] the packed row out [M][kPreviewWords] = status, quality
// and p_win0 (fp32 bits), 0: what `rate` would write for the record against the stored state
// (winner bits ignored), and team 0's win probability (NaN unless kRated).
int launch_preview(int K, const int32_t* rec, int64_t M, const float* state, const float* attrs, const float* vst,
                   int64_t P, float beta2, float unknown_sigma, int32_t* out, hipStream_t s);
// balance: per lobby of lobbies [L][2K] (all slots filled) on mode 0..5 the packed row out
// [L][kBalanceWords] = status, split index (-1 on error), team-0 mask (0), quality, p_win0,
// quality_given (fp32 bits, NaN on error), 0, 0, and the stream record records [L][2K+2] of
// the chosen split (on error: the ids as given).
int launch_balance(int K, const int32_t* lobbies, int64_t L, const float* state, const float* attrs,
                   const float* vst, int64_t P, int mode, float beta2, float unknown_sigma, int32_t* out,
                   int32_t* records, hipStream_t s);
// queue_keys: keys[i] = the descending-mu sort key of queue[i]'s mode-track prior
// (kLadderUnranked: the prior fails or the id is outside [0, P)), vals[i] = i; sort the pairs
// with launch_radix_sort_pairs (32 bits, stable: ties keep queue order)
int launch_queue_keys(const int32_t* queue, int64_t Q, const float* state, const float* attrs, const float* vst,
                      int64_t P, int mode, float unknown_sigma, uint32_t* keys, uint32_t* vals, hipStream_t s);

// K13 careers (career.hip, career_core.h): one window rec [M][2K+2] joined with its packed rows
// [M][W] (alignment as for K10), M * 2K <= kMaxSlots, folded into table [P][kCareerWords] (16-B
// aligned).  career_keys writes per slot i = m * 2K + j the sort key (the player of a game, else
// P), vals[i] = i and the game's event (events: 2 words per slot, 8-B aligned); the pairs are
// sorted with launch_radix_sort_pairs on bit_length(P) bits; career_fold takes the sorted pairs
// [n = M * 2K] and adds every player's run to its row (edges: career_edge_bytes(n) bytes, 16-B
// aligned).  base: global index of match 0; track: CareerTrack; score: LadderScore; modes: bit
// per mode.  Everything is stream-ordered and only reads rec and rows.
constexpr int kCareerTile = 4096;  // sorted elements per workgroup of the fold
size_t career_edge_bytes(int64_t n);
int launch_career_keys(int K, const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t P, int track,
                       int score, uint32_t modes, uint32_t* keys, uint32_t* vals, uint32_t* events, hipStream_t s);
int launch_career_fold(const uint32_t* keys, const uint32_t* vals, const uint32_t* events, int64_t n, int K,
                       int64_t base, int64_t P, int32_t* table, void* edges, hipStream_t s);

// K14 scorecard (score.hip, score_core.h).  Priors: one window rec [M][2K+2] joined with its
// packed rows [M][W] (alignment as for K10), M * 2K <= kMaxSlots; chain [P][kBaseFloats] is read
// and advanced in place; priors [M][4 * 2K] (field-major: shared mu, sigma, mode mu, sigma; 16-B
// aligned).  prior_keys writes per slot i = m * 2K + j the sort key (the player of a live slot,
// else P), the value (i | mode << 28 | write flag << 31), the 16-B event of a writing slot
// (events: 4 words per slot, 16-B aligned) and, into slot_priors (4 words per slot, 16-B
// aligned), the NaN priors of the slots that are not live; the pairs are sorted with
// launch_radix_sort_pairs on bit_length(P) bits; prior_scan takes the sorted pairs [n = M * 2K]
// (P = 0: unsorted will do), adds the prior words of the live slots to slot_priors, lays all of
// them out by field in priors and leaves chain after the window (edges: prior_edge_bytes(n)
// bytes, 16-B aligned).  Everything is stream-ordered.
constexpr int kPriorTile = 4096;  // sorted elements per workgroup of the scan
size_t prior_edge_bytes(int64_t n);
int launch_prior_keys(int K, const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t P, uint32_t* keys,
                      uint32_t* vals, uint32_t* events, uint32_t* slot_priors, hipStream_t s);
int launch_prior_scan(const uint32_t* keys, const uint32_t* vals, const uint32_t* events, int64_t n, int K, int64_t P,
                      float* chain, void* edges, uint32_t* slot_priors, float* priors, hipStream_t s);
// score: per match the prediction its priors make (attrs [P][4] 16-B aligned or null, vst:
// kVstTiers floats; track: ScoreTrack; modes: bit per mode) added into table
// [kModes][kScoreBins + 1][4] int64; pred (nullable, 16-B aligned): [M][kPredWords] int32
int launch_score(int K, const int32_t* rec, const float* priors, const float* rows, int64_t W, int64_t M,
                 const float* attrs, const float* vst, int64_t P, float beta2, float unknown_sigma, int track,
                 uint32_t modes, int64_t* table, int32_t* pred, hipStream_t s);
// out[i] = nlog2_q20(bits[i]) (score_core.h), i < n
int launch_nlog2_q20(const uint32_t* bits, int64_t n, int64_t* out, hipStream_t s);

// K15 pairs (pairs.hip, pair_core.h): the pair table of one window rec [M][2K+2] joined with its
// packed rows [M][W], or of several tables compacted into one.  n entries everywhere; every
// array is n words unless said otherwise.  Everything is stream-ordered and only reads rec, rows
// and the source tables; bad sizes or pointers return hipErrorInvalidValue without a launch.
//   pair_keys   n = M * pair_entries(K) <= kMaxSlots, K in 1..5, P fits int32; bitmap (nullable)
//               uint32 [ceil(P / 32)]: per entry i = m * E_K + q the key ka[i] (a, or P for a dead
//               entry), kb[i] = bkeep[i] = b and vals[i] = i | flags.  live_count (nullable; one
//               zeroed word): only the live entries are written instead, packed from 0 in any
//               order as vals[pos] = pos | flags, and counted there
//   pair_split  the same four arrays from int64 keys [n] (a << 32 | b), vals[i] = i
//   the pairs (kb, vals) are sorted with launch_radix_sort_pairs, pair_gather fetches
//   out[i] = src[vals[i] & mask] (ka into the sorted order, later b from bkeep), a second sort on
//   a leaves the entries ordered by (a, b)
//   pair_count  counts [pair_tiles(n)] = the run heads per tile of the sorted (a, b) (dead: keys
//               >= dead end the live entries) and offsets [tiles + 1] (8-B aligned) = their
//               exclusive scan, the number of rows U last: one host read
//   pair_emit   keys [U] int64 and counts [U][kPairWords] int32 (16-B aligned, zeroed by the
//               caller); src == nullptr: the counters of an entry are decoded from its value's
//               flags (n <= kMaxSlots), else they are the 16-B row src[value] (src [n][4])
constexpr int kPairTile = 2048;  // sorted entries per workgroup of count and emit
int64_t pair_tiles(int64_t n);
int launch_pair_keys(int K, const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t P, uint32_t modes,
                     const uint32_t* bitmap, uint32_t* ka, uint32_t* kb, uint32_t* bkeep, uint32_t* vals,
                     uint32_t* live_count, hipStream_t s);
int launch_pair_split(const int64_t* keys, int64_t n, uint32_t* ka, uint32_t* kb, uint32_t* bkeep, uint32_t* vals,
                      hipStream_t s);
int launch_pair_gather(const uint32_t* src, const uint32_t* vals, uint32_t mask, int64_t n, uint32_t* out,
                       hipStream_t s);
int launch_pair_count(const uint32_t* a, const uint32_t* b, int64_t n, uint32_t dead, uint32_t* counts,
                      int64_t* offsets, hipStream_t s);
int launch_pair_emit(const uint32_t* a, const uint32_t* b, const uint32_t* vals, int64_t n, uint32_t dead,
                     const int32_t* src, const int64_t* offsets, int64_t U, int64_t* keys, int32_t* counts,
                     hipStream_t s);

// K16 hindsight (hindsight.hip, hindsight_core.h): the smoothed (mu, sigma) of one window rec
// [M][2K+2] joined with its packed rows [M][W] (alignment as for K10), M * 2K <= kMaxSlots;
// windows come newest first.  track: HsTrack; mode: the mode 0..5 of a kHsMode track.
// hindsight_keys writes per slot i = m * 2K + j, at the mirrored position n - 1 - i, the sort key
// (the player of an element, else P) and the value i, at events[i] (2 words per slot, 8-B
// aligned) the (mu, sigma) bits of an element and at out[i] (out [M][2K][2] fp32, 8-B aligned)
// the (NaN, NaN) of a slot that is none, and adds the bad slots to *bad; the pairs are sorted with
// launch_radix_sort_pairs on bit_length(P) bits; hindsight_scan takes the sorted pairs [n = M *
// 2K], stores the smoothed pair of every element in out and advances carry [P][2] fp64 (mh, Ph;
// NaN: no later match) in place (tau2 finite and >= 0; edges: hindsight_edge_bytes(n) bytes, 8-B
// aligned).  Everything is stream-ordered.
constexpr int kHindsightTile = 4096;  // sorted elements per workgroup of the scan
size_t hindsight_edge_bytes(int64_t n);
int launch_hindsight_keys(int K, const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t P, int track,
                          int mode, uint32_t* keys, uint32_t* vals, uint32_t* events, float* out, int32_t* bad,
                          hipStream_t s);
int launch_hindsight_scan(const uint32_t* keys, const uint32_t* vals, const uint32_t* events, int64_t n, int K,
                          int64_t P, double tau2, double* carry, void* edges, float* out, hipStream_t s);

// K20 through time (ttt.hip, ttt_core.h): the joint re-estimate of one history rec [M][2K+2]
// joined with its packed rows [M][W] (alignment as for K10) and its K14 priors [M][4][2K] fp32
// (16-B aligned), M * 2K = n <= kMaxSlots.  track, mode as K16.  Per slot buffers, [n] each: msg,
// prior, fwd, cav (2 fp64, 16-B aligned), mu64 (fp64), out (2 fp32, 8-B aligned); mword [M];
// counters [kTttCounters] int32 (bad, flat, inconsistent; added to).  ttt_setup fills the sort
// pairs of the forward scan (keys_f, vals_f: slot i at i) and of the backward scan (keys_b,
// vals_b: slot i at n - 1 - i), msg, prior, mword, the NaNs of out and the counters; both pair
// sets are sorted with launch_radix_sort_pairs on bit_length(P) bits.  ttt_chain is one chain
// pass over the sorted pairs: it fills fwd, cav, out and mu64 and, when have_before, folds the
// largest |mu - mu64 of the pass before| into *resid (the bits of a non-negative fp64, integer
// max; 8-B aligned; edges: ttt_edge_bytes(n) bytes, 8-B aligned).  ttt_match runs the match
// factors: it reads cav and writes msg, damped by theta in (0, 1].  Everything is stream-ordered.
constexpr int kTttTile = 4096;  // sorted elements per workgroup of the scans
size_t ttt_edge_bytes(int64_t n);
int launch_ttt_setup(int K, const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t P,
                     const float* priors, const float* attrs, const float* vst, float unknown_sigma, int track,
                     int mode, double tau2, uint32_t* keys_f, uint32_t* vals_f, uint32_t* keys_b, uint32_t* vals_b,
                     double* msg, double* prior, float* out, uint32_t* mword, int32_t* counters, hipStream_t s);
int launch_ttt_chain(const uint32_t* keys_f, const uint32_t* vals_f, const uint32_t* keys_b, const uint32_t* vals_b,
                     int64_t n, int K, int64_t P, double tau2, const double* msg, const double* prior, double* fwd,
                     double* cav, double* mu64, float* out, void* edges, int have_before, uint64_t* resid,
                     hipStream_t s);
int launch_ttt_match(int K, const int32_t* rec, int64_t M, int64_t P, const uint32_t* mword, const double* cav,
                     double* msg, double beta2, double theta, hipStream_t s);

// K17 profiles (profile.hip, profile_core.h): one window rec [M][2K+2] joined with its packed rows
// [M][W] (alignment as for K10) and its stat vectors stats [M][2K][8] fp32 (16-B aligned), M * 2K
// <= kMaxSlots.  profile_keys writes per slot i = m * 2K + j the sort key (the player of a game,
// else P) and vals[i] = i | won << 31, and adds every game to its cell of the baseline table cells
// [profile_table_words(n_edges + 1)] int64 (edges: n_edges <= kProfileMaxEdges finite ascending
// host floats); the pairs are sorted with launch_radix_sort_pairs on bit_length(P) bits;
// profile_fold takes the sorted pairs [n = M * 2K] and adds every player's run to its row of table
// [P][kProfileWords] (16-B aligned; edges: profile_edge_bytes(n) bytes, 16-B aligned).  track:
// CareerTrack; score: LadderScore; modes: bit per mode.  Everything is stream-ordered and only
// reads rec, rows and stats.
constexpr int kProfileTile = 4096;  // sorted elements per workgroup of the fold
size_t profile_edge_bytes(int64_t n);
int launch_profile_keys(int K, const int32_t* rec, const float* rows, int64_t W, const float* stats, int64_t M,
                        int64_t P, int track, int score, uint32_t modes, const float* edges, int n_edges,
                        uint32_t* keys, uint32_t* vals, int64_t* cells, hipStream_t s);
int launch_profile_fold(const uint32_t* keys, const uint32_t* vals, const float* stats, int64_t n, int K, int64_t P,
                        int32_t* table, void* edges, hipStream_t s);

// K18 islands (islands.hip, island_core.h): the connected components of the match graph as a
// union-find over parent / slots / credit int32 [P], updated in place; ctrl: kIslandCtrlWords
// int64 ([0] sticky error bits, [1] edges dropped as bad).  island_hook takes one window rec
// [M][2K+2] joined with its packed rows [M][W] (alignment as for K10), M * 2K <= kMaxSlots;
// island_edges the edges (a[i], b[i]), i < n, and marks their endpoints seen when mark != 0;
// island_flatten, a launch after the last of those, leaves parent[i] = the smallest id of i's
// island; island_census then adds the seen players of flattened parents to census
// [kIslandCensusRows][P] int64 (zeroed by the caller): players, matches, player_games at the
// root's index.  Everything is stream-ordered; no lane waits for another.
int launch_island_hook(int K, const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t P, uint32_t modes,
                       int32_t* parent, int32_t* slots, int32_t* credit, int64_t* ctrl, hipStream_t s);
int launch_island_edges(const int32_t* a, const int32_t* b, int64_t n, int64_t P, int mark, int32_t* parent,
                        int32_t* slots, int64_t* ctrl, hipStream_t s);
int launch_island_flatten(int32_t* parent, int64_t P, int64_t* ctrl, hipStream_t s);
int launch_island_census(const int32_t* parent, const int32_t* slots, const int32_t* credit, int64_t P,
                         int64_t* census, int64_t* ctrl, hipStream_t s);

// K19 expectations (expect.hip, expect_core.h): one window rec [M][2K+2] (alignment as for K10)
// joined with the raw priors [M][4 * 2K] of K14 (field-major, 16-B aligned) and the pred rows
// [M][kPredWords] of launch_score (16-B aligned), M * 2K <= kMaxSlots.  expect_keys writes per
// slot i = m * 2K + j the sort key (the player of a game, else P), vals[i] = i | won << 31 and, for
// a game, its term record at terms[i] (terms [M * 2K][kExpectTermWords] int32, 16-B aligned), and
// adds the bad own values to *bad; the pairs are sorted with launch_radix_sort_pairs on
// bit_length(P) bits; expect_fold takes the sorted pairs [n = M * 2K] and adds every player's run
// to its row of table [P][kExpectWords] (16-B aligned; edges: expect_edge_bytes(n) bytes, 16-B
// aligned).  track: ScoreTrack.  Everything is stream-ordered and only reads rec, priors and pred.
constexpr int kExpectTile = 4096;  // sorted elements per workgroup of the fold
size_t expect_edge_bytes(int64_t n);
int launch_expect_keys(int K, const int32_t* rec, const float* priors, const int32_t* pred, int64_t M, int64_t P,
                       int track, uint32_t* keys, uint32_t* vals, int32_t* terms, int64_t* bad, hipStream_t s);
int launch_expect_fold(const uint32_t* keys, const uint32_t* vals, const int32_t* terms, int64_t n, int K, int64_t P,
                       int32_t* table, void* edges, hipStream_t s);

// Stable LSD radix sort of (key, value) pairs on the low ``bits`` key bits
// (radix_sort.hip).  Ping-pongs between the two buffer pairs; *result_in_alt
// says which holds the result.  ws: radix_sort_workspace_bytes(n) bytes (256 counts per
// 8192-element tile and the 256 digit totals; the schedule's run table reuses them).
size_t radix_sort_workspace_bytes(int64_t n);
int launch_radix_sort_pairs(uint32_t* keys, uint32_t* vals, uint32_t* keys_alt, uint32_t* vals_alt,
                            int64_t n, int bits, void* ws, int* result_in_alt, hipStream_t s);
// The schedule's sort (radix_sort.hip): link[slot] for every slot of a
// stateful match (next match of its player | kLinkHasPred), from a stable sort
// of the stream's slots by player fused with the record decode and the links.
// ws: radix_sort_workspace_bytes(M * 2K) bytes; ka..vb: M * 2K words each.
// deps [M] (zeroed by the first kernel), ctrl[0..nz) (zeroed), epoch_bump (+1): the
// schedule's fill work, folded into that kernel (null / 0: skipped).  sort_nt (ANA_SORT_NT wins):
// non-temporal loads of the sort, 0 none, 2 every pass's input (-1: ANA_SORT_NT or none) -- 2 is
// what a caller asks for whose prepass runs beside the executor, so with it the chain path also
// writes its links as whole lines (sched_unpartition), which costs the executor less and the
// prepass itself more.  Any other value: hipErrorInvalidValue, nothing launched.
int launch_sched_sort(int K, const int32_t* rec, int64_t M, uint32_t num_players, uint32_t* ka,
                      uint32_t* va, uint32_t* kb, uint32_t* vb, void* ws, uint32_t* link,
                      hipStream_t s, int32_t* deps = nullptr, uint32_t* ctrl = nullptr, int nz = 0,
                      int32_t* epoch_bump = nullptr, int sort_nt = -1);
// Device levelizer (levels.hip): level[m] = 0 for a match without state, else
// 1 + the largest level of its players' previous matches -- the exact-DP rounds --
// as a dataflow over a fresh schedule (link, deps zeroed; deps are consumed).
// pushed: int32 [M] zeroed scratch; ctrl: uint32 [4] zeroed ([2] depth, [3] error).
int launch_levels(int K, const int32_t* rec, const uint32_t* link, int32_t* deps, int32_t* pushed,
                  int32_t* level, int64_t M, int64_t P, uint32_t* ctrl, hipStream_t s);
// link: uint32 [M][2K] = next match of the player (kNoMatch: none) | kLinkHasPred
//       if the player has an earlier occurrence in the window
// deps: int32 [M] zeroed: the completion counters the executor counts up (a
//       match is ready when its counter reaches the number of its players with
//       kLinkHasPred, which the executor reads from the links)
// overflow: zeroed (reserved for schedule error reporting)
// Up to 8192 slots one workgroup links the batch through LDS hash lists (sched_hash_kernel);
// larger windows take launch_sched_sort, which sort_nt is for.
int launch_schedule(int K, const int32_t* rec, int64_t M, int64_t P, uint32_t* link,
                    int32_t* deps, void* ws, size_t ws_bytes, uint32_t* overflow, hipStream_t s,
                    bool zero_ctrl = false, int32_t* epoch_bump = nullptr, int sort_nt = -1);

// out must be the packed layout (one row per match: [s_mu | s_sig | delta |
// m_mu | m_sig][2K], quality, status byte), else hipErrorInvalidValue.
// tp.evoff == nullptr: no telemetry; otherwise idle waves aggregate telemetry
// tiles (K8 fused streaming mode).  ctrl[12] = telemetry tile ticket,
// ctrl[13] = malformed events.
int launch_rate(int K, const int32_t* rec, const uint32_t* link, int32_t* deps, float* state,
                const float* attrs, float* first_prior, const RateOut& out, uint32_t* ctrl,
                const RateParams& prm, const TelemetryParams& tp, int blocks, hipStream_t s);


// K8 (telemetry.hip)
int launch_gen_event_counts(const GenEventParams& g, int64_t base, int64_t M, int64_t* counts,
                            hipStream_t s);
int launch_gen_events(int K, const GenEventParams& g, int64_t base, const int32_t* rec,
                      const int64_t* evoff, int64_t M, int32_t* events, hipStream_t s);
// K8 implementation: 1 = one-hot MFMA (default), 0 = LDS float atomics (ANA_TELE_IMPL)
int tele_impl();
int launch_telemetry(int K, const TelemetryParams& tp, uint32_t* bad, hipStream_t s);

}  // namespace ana

namespace ana {
// s0: common window start, a: the rank's prior of this sweep (may be s0), s: posterior
int launch_sweep_delta(const float* s0, const float* a, const float* s, const float* attrs,
                       const float* vst, float unknown_sigma, int scaled, float* buf, int64_t P,
                       hipStream_t st);
// decoded rows to s and (s2 != nullptr) s2; clamps (nullable): += decoded tracks whose
// merged precision hit the floor (sweep_core.h sweep_apply_track), here and below
int launch_sweep_apply(const float* s0, const float* buf, const float* attrs, float* s, float* s2,
                       const float* vst, float unknown_sigma, int scaled, int64_t P, uint32_t* clamps,
                       hipStream_t st);
// compressed merges: msg [P][14] bf16 (bf16 != 0) or fp16 + cnt [P] int32 (touch fields lo | hi << 16);
// mstride / cstride: row strides in 32-bit words (7 / 1 for separate tensors, 8 / 8 for the
// split collective's [P][8]-word operand rows with the touch word last)
int launch_sweep_delta_packed(const float* s0, const float* a, const float* s, const float* attrs,
                              const float* vst, float unknown_sigma, int bf16, void* msg, int32_t* cnt,
                              int64_t P, hipStream_t st, int64_t mstride = 7, int64_t cstride = 1);
// split collective (parallel/comm.py): recv [N][blk][8] words -> total [blk][8] (+ the exclusive
// prefixes pref [N][blk][7] when non-null)
int launch_sweep_block_reduce(const int32_t* recv, int N, int64_t blk, int bf16, int32_t* total, int32_t* pref,
                              hipStream_t st);
// prefix (nullable): the scaled exclusive prefix of the messages (same type as msg) ->
// delta [P][16] fp32, the record correction's increments (sweep_core.h prefix_delta_track)
int launch_sweep_apply_packed(const float* s0, const void* msg, const int32_t* cnt, int bf16,
                              const float* attrs, float* s, float* s2, const float* vst, float unknown_sigma,
                              int64_t P, uint32_t* clamps, const void* prefix, float* delta, hipStream_t st,
                              int64_t mstride = 7, int64_t cstride = 1);
int launch_prefix_delta(const float* s0, const void* prefix, int bf16, const float* attrs, const float* vst,
                        float unknown_sigma, float* delta, int64_t P, hipStream_t st);
// causal record correction: rows = RateResult's packed rows [M][orow] += delta [P][16]
// fp32 (raw natural-parameter increments per track) of each slot's player
int launch_correct_records(int K, const int32_t* rec, int64_t M, float* rows, int64_t orow, const float* delta,
                           int64_t P, hipStream_t st);
// C2 exact-DP exchange (sweep.hip): fixed-capacity [cap][33] entries of changed rows
int launch_pack_rows(const int32_t* rec, int K, int64_t m, const uint8_t* status, int64_t sstride,
                     const float* state, float* out, int64_t cap, hipStream_t st);
int launch_unpack_rows(const float* buf, int64_t n, float* state, hipStream_t st);
// exact-DP race detector: matches idx[0..m) of round ``round`` share no player
// (owner: P 64-bit claims, zeroed once; *flag |= 1 on a conflict)
int launch_check_round(const int32_t* rec, int K, const int64_t* idx, int64_t m, int64_t P, uint32_t round,
                       unsigned long long* owner, uint32_t* flag, hipStream_t st);
}  // namespace ana
