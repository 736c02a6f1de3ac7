// PyTorch bindings of the engine.  Device (ROCm) tensors run the gfx950
// kernels (kernels.h) on the current HIP stream; CPU tensors run the host
// mirror of host.cpp.  Every shape/dtype/device assumption a kernel makes is
// checked here, on the host, before anything is launched, by the shared
// operand checks below; an entry point is those and the device / host branch.
#include <torch/extension.h>

#include <cstdlib>
#include <ATen/hip/HIPContext.h>

#include <algorithm>
#include <numeric>
#include <string>
#include <tuple>
#include <vector>

#include "career_core.h"
#include "common.h"
#include "expect_core.h"
#include "gen_core.h"
#include "hindsight_core.h"
#include "host.h"
#include "ingest.h"
#include "island_core.h"
#include "kernels.h"
#include "ladder_core.h"
#include "matchmake_core.h"
#include "pair_core.h"
#include "profile_core.h"
#include "score_core.h"
#include "select_core.h"
#include "ttt_core.h"

namespace {

using torch::Tensor;

void check_hip(int err, const char* what) {
  TORCH_CHECK(err == 0, what, " failed: ", hipGetErrorString((hipError_t)err), " (", err, ")");
}

void check(const Tensor& t, const char* name, torch::ScalarType dt, const torch::Device& dev) {
  TORCH_CHECK(t.defined(), name, " is undefined");
  TORCH_CHECK(t.scalar_type() == dt, name, " must be ", c10::toString(dt), ", got ",
              c10::toString(t.scalar_type()));
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.device() == dev, name, " is on ", t.device(), " but expected ", dev);
}

// strided output views: rows of `inner` contiguous elements, any row stride
int64_t check_rows_view(const Tensor& t, const char* name, torch::ScalarType dt,
                        const torch::Device& dev, int64_t rows, int64_t inner) {
  TORCH_CHECK(t.defined(), name, " is undefined");
  TORCH_CHECK(t.scalar_type() == dt, name, " must be ", c10::toString(dt));
  TORCH_CHECK(t.device() == dev, name, " is on ", t.device(), " but expected ", dev);
  if (inner == 1) {
    TORCH_CHECK(t.dim() == 1 && t.size(0) == rows, name, " must have ", rows, " entries");
    return rows > 1 ? t.stride(0) : 1;
  }
  TORCH_CHECK(t.dim() == 2 && t.size(0) == rows && t.size(1) == inner, name, " must be [", rows,
              ", ", inner, "]");
  TORCH_CHECK(t.stride(1) == 1 && (rows <= 1 || t.stride(0) >= inner), name,
              " rows must be contiguous and non-overlapping");
  return rows > 1 ? t.stride(0) : inner;
}

// the device's vector loads and stores need their operands aligned
bool aligned(const Tensor& t, int bytes) { return reinterpret_cast<uintptr_t>(t.data_ptr()) % bytes == 0; }

hipStream_t stream_of(const Tensor& t) {
  return at::hip::getCurrentHIPStream(t.device().index()).stream();
}

uint32_t u32(int64_t v, const char* name) {
  TORCH_CHECK(v >= 0 && v <= 0xffffffffLL, name, " must fit in uint32");
  return (uint32_t)v;
}

// ---- operand checks shared by the entry points (common.h data layout); ``what`` names the
// entry point in the message, and each returns what its caller needs next
// match stream rec [M, 2K+2] int32 -> M
int64_t check_rec(const Tensor& rec, int64_t K, const torch::Device& dev, const char* what) {
  check(rec, "rec", torch::kInt32, dev);
  TORCH_CHECK(K >= 1 && K <= ana::kMaxTeamSize, what, ": K (players per roster) must be 1..5");
  TORCH_CHECK(rec.dim() == 2 && rec.size(1) == 2 * K + 2, what, ": rec must be [M, 2K+2]");
  return rec.size(0);
}

// the team size K of a match stream rec [M, 2K+2], from its width (check_rec holds K to 1..5)
int64_t team_size_of(const Tensor& rec, const char* what) {
  TORCH_CHECK(rec.dim() == 2 && rec.size(1) >= 4 && rec.size(1) % 2 == 0, what, ": rec must be [M, 2K+2]");
  return (rec.size(1) - 2) / 2;
}

// one window as K10, K13, K14 and K15 take it: rec [M, 2K+2] and its packed output rows [M, W]
// on dev, aligned for the device's vector loads -> M
int64_t check_window(const Tensor& rec, const Tensor& rows, int64_t K, const torch::Device& dev, const char* what) {
  const int64_t M = check_rec(rec, K, dev, what);
  check(rows, "rows", torch::kFloat32, dev);
  TORCH_CHECK(rows.dim() == 2 && rows.size(0) == M && rows.size(1) >= 10 * K + 2 && rows.size(1) % 4 == 0, what,
              ": rows must be the packed [M, W] output rows of rec's matches");
  if (dev.is_cuda())
    TORCH_CHECK(aligned(rec, K % 2 == 0 ? 8 : 16) && aligned(rows, 16), what, ": rec and rows must be 16-B aligned");
  return M;
}

// the slots of a window are sort values (K13, K14)
void check_slots(int64_t M, int64_t K, const char* what) {
  TORCH_CHECK(M * 2 * K <= ana::kMaxSlots, what, ": a window holds at most ", ana::kMaxSlots, " slots");
}

// the key bits of a sort by player: P itself, the key of a slot without one, sorts last
int bit_length(int64_t v) {
  int bits = 1;
  while ((v >> bits) != 0) ++bits;
  return bits;
}

// roster state [P, 32] fp32 -> P
int64_t check_state(const Tensor& state, const torch::Device& dev, const char* what) {
  check(state, "state", torch::kFloat32, dev);
  TORCH_CHECK(state.dim() == 2 && state.size(1) == ana::kRowFloats, what, ": state must be [P, 32]");
  return state.size(0);
}

// player attributes [P, 4] fp32 -> their pointer
const float* check_attrs(const Tensor& attrs, int64_t P, const torch::Device& dev, const char* what) {
  check(attrs, "attrs", torch::kFloat32, dev);
  TORCH_CHECK(attrs.dim() == 2 && attrs.size(0) == P && attrs.size(1) == 4, what, ": attrs must be [P, 4]");
  return attrs.data_ptr<float>();
}

// the tier seed table, indexed by tier + 1 -> its pointer
const float* check_vst(const Tensor& vst, const torch::Device& dev, const char* what) {
  check(vst, "vst", torch::kFloat32, dev);
  TORCH_CHECK(vst.numel() == ana::kVstTiers, what, ": vst must have 31 entries (tiers -1..29)");
  return vst.data_ptr<float>();
}

// the schedule of rec: link [M, 2K] and deps [M], int32
void check_schedule(const Tensor& link, const Tensor& deps, int64_t M, int64_t K, const torch::Device& dev) {
  check(link, "link", torch::kInt32, dev);
  check(deps, "deps", torch::kInt32, dev);
  TORCH_CHECK(link.dim() == 2 && link.size(0) == M && link.size(1) == 2 * K, "link must be [M, 2K]");
  TORCH_CHECK(deps.numel() == M, "deps must have M entries");
}

// the words of an int32 tensor as the kernels take them
uint32_t* u32p(const Tensor& t) { return reinterpret_cast<uint32_t*>(t.data_ptr<int32_t>()); }

bool present(const c10::optional<Tensor>& t) { return t.has_value() && t->defined() && t->numel() > 0; }

int is_bf16(const Tensor& t) { return t.scalar_type() == torch::kBFloat16 ? 1 : 0; }

// Stable sort of n uint32 (key, value) pairs by the low ``bits`` key bits (radix_sort.hip), in
// place or into scratch buffers: returns the tensors that hold the result, {keys, vals}.
std::vector<Tensor> sort_pairs_on_stream(Tensor keys, Tensor vals, int64_t n, int bits, hipStream_t s) {
  Tensor kalt = torch::empty({n}, keys.options()), valt = torch::empty({n}, vals.options());
  Tensor ws = torch::empty({(int64_t)ana::radix_sort_workspace_bytes(n)}, keys.options().dtype(torch::kUInt8));
  int in_alt = 0;
  check_hip(ana::launch_radix_sort_pairs(u32p(keys), u32p(vals), u32p(kalt), u32p(valt), n, bits,
                                         ws.data_ptr<uint8_t>(), &in_alt, s),
            "radix sort");
  return in_alt ? std::vector<Tensor>{kalt, valt} : std::vector<Tensor>{keys, vals};
}

// What the per-player tables (K13, K14, K16, K17, K19) do with a window's n = M * 2K slots before
// their scan: run_keys(keys, vals) fills the sort pairs, the stable sort by player follows on the
// same stream (P == 0: no player, nothing to sort), and the scan's edge buffer is allocated.
struct SortedSlots { Tensor keys, vals, edges; };
template <class RunKeys>
SortedSlots sort_by_player(int64_t n, int64_t P, size_t edge_bytes, const torch::Device& dev, hipStream_t s,
                           RunKeys&& run_keys) {
  const auto i32 = torch::TensorOptions().dtype(torch::kInt32).device(dev);
  Tensor keys = torch::empty({n}, i32), vals = torch::empty({n}, i32);
  run_keys(u32p(keys), u32p(vals));
  const auto sorted = P > 0 ? sort_pairs_on_stream(keys, vals, n, bit_length(P), s) : std::vector<Tensor>{keys, vals};
  return {sorted[0], sorted[1], torch::empty({(int64_t)edge_bytes}, i32.dtype(torch::kUInt8))};
}

// --------------------------------------------------------------------- K7
void gen_roster(Tensor state, Tensor attrs, int64_t seed, int64_t p_tier_null, int64_t p_tier_bad,
                int64_t p_rp_ranked, int64_t p_rp_blitz, int64_t p_rated, int64_t p_mode_rated,
                double mu_lo, double mu_span, double sig_lo, double sig_span) {
  const auto dev = state.device();
  ana::GenRosterParams g{};
  g.seed = (uint64_t)seed;
  g.num_players = check_state(state, dev, "gen_roster");
  check_attrs(attrs, g.num_players, dev, "gen_roster");
  g.p_tier_null = u32(p_tier_null, "p_tier_null");
  g.p_tier_bad = u32(p_tier_bad, "p_tier_bad");
  g.p_rp_ranked = u32(p_rp_ranked, "p_rp_ranked");
  g.p_rp_blitz = u32(p_rp_blitz, "p_rp_blitz");
  g.p_rated = u32(p_rated, "p_rated");
  g.p_mode_rated = u32(p_mode_rated, "p_mode_rated");
  g.mu_lo = (float)mu_lo;
  g.mu_span = (float)mu_span;
  g.sig_lo = (float)sig_lo;
  g.sig_span = (float)sig_span;
  if (dev.is_cuda()) {
    check_hip(ana::launch_gen_roster(g, state.data_ptr<float>(), attrs.data_ptr<float>(),
                                     stream_of(state)), "gen_roster");
  } else {
    ana::host_gen_roster(g, state.data_ptr<float>(), attrs.data_ptr<float>());
  }
}

void gen_stream(Tensor rec, int64_t K, int64_t seed, int64_t base, int64_t num_players,
                int64_t team_size, std::vector<int64_t> mode_cdf, int64_t p_uneven,
                int64_t p_bad_rosters, int64_t p_tie, int64_t p_afk, int64_t p_hot,
                int64_t hot_players, int64_t skew) {
  const auto dev = rec.device();
  const int64_t M = check_rec(rec, K, dev, "gen_stream");
  TORCH_CHECK(team_size >= 1 && team_size <= K, "team_size must be in 1..K");
  TORCH_CHECK(num_players >= 1 && num_players < 0x7fffffffLL, "num_players out of range");
  TORCH_CHECK(hot_players >= 1 && hot_players <= num_players, "hot_players must be 1..num_players");
  TORCH_CHECK(mode_cdf.size() == 7, "mode_cdf must have 7 thresholds");
  TORCH_CHECK(skew >= 1 && skew <= 8, "skew must be 1..8");
  ana::GenStreamParams g{};
  g.seed = (uint64_t)seed;
  g.base = base;
  g.num_players = num_players;
  g.team_size = (int32_t)team_size;
  g.skew = (int32_t)skew;
  for (int k = 0; k < 7; ++k) g.mode_cdf[k] = u32(mode_cdf[k], "mode_cdf");
  g.p_uneven = u32(p_uneven, "p_uneven");
  g.p_bad_rosters = u32(p_bad_rosters, "p_bad_rosters");
  g.p_tie = u32(p_tie, "p_tie");
  g.p_afk = u32(p_afk, "p_afk");
  g.p_hot = u32(p_hot, "p_hot");
  g.hot_players = u32(hot_players, "hot_players");
  if (dev.is_cuda()) {
    check_hip(ana::launch_gen_stream((int)K, g, rec.data_ptr<int32_t>(), M, stream_of(rec)),
              "gen_stream");
  } else {
    TORCH_CHECK(ana::host_gen_stream((int)K, g, rec.data_ptr<int32_t>(), M) == 0, "bad K");
  }
}

// --------------------------------------------------------------------- K5
int64_t schedule_workspace_bytes(int64_t nslots, int64_t num_players) {
  return (int64_t)ana::schedule_workspace_bytes(nslots, num_players);
}

// Stable sort of int32 (key, value) pairs by the low ``bits`` key bits on the
// device (the K5 radix sort, exposed for tests and tools).  Returns new tensors.
std::vector<Tensor> sort_pairs(Tensor keys, Tensor vals, int64_t bits) {
  const auto dev = keys.device();
  TORCH_CHECK(dev.is_cuda(), "sort_pairs runs on the device");
  check(keys, "keys", torch::kInt32, dev);
  check(vals, "vals", torch::kInt32, dev);
  const int64_t n = keys.numel();
  TORCH_CHECK(vals.numel() == n, "keys and vals must have the same length");
  TORCH_CHECK(bits >= 1 && bits <= 32, "bits must be 1..32");
  return sort_pairs_on_stream(keys.clone(), vals.clone(), n, (int)bits, stream_of(keys));
}

// K5 host levelizer (conflict-free rounds for the exact DP mode).
std::tuple<Tensor, int64_t> levels(Tensor rec, int64_t K, int64_t num_players) {
  TORCH_CHECK(!rec.is_cuda(), "levels runs on the host (pass a CPU stream)");
  const int64_t M = check_rec(rec, K, rec.device(), "levels");
  auto level = torch::empty({M}, rec.options());
  const int64_t depth = ana::host_levels((int)K, rec.data_ptr<int32_t>(), M, num_players, level.data_ptr<int32_t>());
  return {level, depth};
}

// K5 device levelizer over a fresh schedule (its deps are consumed): (level [M], depth).
std::tuple<Tensor, int64_t> levels_device(Tensor rec, int64_t K, int64_t num_players, Tensor link,
                                          Tensor deps) {
  const auto dev = rec.device();
  TORCH_CHECK(dev.is_cuda(), "levels_device runs on the device (host: levels)");
  const int64_t M = check_rec(rec, K, dev, "levels_device");
  check_schedule(link, deps, M, K, dev);
  TORCH_CHECK(M * 2 * K <= ana::kMaxSlots, "more than 2^28 slots in one window (split the stream)");
  TORCH_CHECK(num_players >= 1 && num_players < 0x7fffffffLL, "num_players out of range");
  auto level = torch::empty({M}, rec.options());
  auto pushed = torch::zeros({M}, rec.options());
  auto ctrl = torch::zeros({4}, rec.options());
  check_hip(ana::launch_levels((int)K, rec.data_ptr<int32_t>(), u32p(link), deps.data_ptr<int32_t>(),
                               pushed.data_ptr<int32_t>(), level.data_ptr<int32_t>(), M, num_players, u32p(ctrl),
                               stream_of(rec)),
            "levels");
  const auto c = ctrl.cpu();
  TORCH_CHECK(c[3].item<int32_t>() == 0,
              "device levelizer made no progress for 5 s (schedule and stream disagree)");
  return {level, (int64_t)c[2].item<int32_t>()};
}

void schedule(Tensor rec, int64_t K, int64_t num_players, Tensor link, Tensor deps,
              Tensor workspace, Tensor ctrl, bool zero_ctrl, int64_t epoch_bump_ptr, int64_t sort_nt) {
  const auto dev = rec.device();
  const int64_t M = check_rec(rec, K, dev, "schedule");
  check_schedule(link, deps, M, K, dev);
  TORCH_CHECK(num_players >= 1 && num_players < 0x7fffffffLL, "num_players out of range");
  TORCH_CHECK(M * 2 * K <= ana::kMaxSlots, "more than 2^28 slots in one window (split the stream)");
  TORCH_CHECK(sort_nt == -1 || sort_nt == 0 || sort_nt == 2,
              "sort_nt must be 0 (plain loads), 2 (non-temporal loads) or -1 (ANA_SORT_NT or plain), got ", sort_nt);
  if (dev.is_cuda()) {
    check(workspace, "workspace", torch::kUInt8, dev);
    check(ctrl, "ctrl", torch::kInt32, dev);
    TORCH_CHECK(ctrl.numel() >= 52, "ctrl must have 52 entries");
    const size_t need = ana::schedule_workspace_bytes(M * 2 * K, num_players);
    TORCH_CHECK((size_t)workspace.numel() >= need, "workspace too small: need ", need, " bytes");
    check_hip(ana::launch_schedule((int)K, rec.data_ptr<int32_t>(), M, num_players, u32p(link),
                                   deps.data_ptr<int32_t>(), workspace.data_ptr<uint8_t>(),
                                   (size_t)workspace.numel(), u32p(ctrl), stream_of(rec), zero_ctrl,
                                   reinterpret_cast<int32_t*>((intptr_t)epoch_bump_ptr), (int)sort_nt),
              "schedule");
  } else {
    TORCH_CHECK(ana::host_schedule((int)K, rec.data_ptr<int32_t>(), M, num_players, u32p(link),
                                   deps.data_ptr<int32_t>()) == 0,
                "bad K");
  }
}

// knobs (EngineConfig, config.py): [rate_idle, rate_local, rate_diag, rate_tight,
// tele_fused_tail, tele_role] -- executor / fused-telemetry tuning, per BatchRater
constexpr size_t kKnobs = 6;

static ana::TelemetryParams telemetry_params(const Tensor& evoff, const Tensor& events,
                                             const Tensor& stats, int64_t M, int64_t K,
                                             const torch::Device& dev, const std::vector<int64_t>& knobs) {
  ana::TelemetryParams tp{nullptr, nullptr, nullptr, M};
  if (evoff.numel() == 0) return tp;
  check(evoff, "evoff", torch::kInt64, dev);
  check(events, "events", torch::kInt32, dev);
  check(stats, "stats", torch::kFloat32, dev);
  TORCH_CHECK(evoff.numel() == M + 1, "evoff must have M + 1 entries");
  TORCH_CHECK(events.dim() == 2 && events.size(1) == 2, "events must be [E, 2] (8-B events, telemetry_core.h)");
  TORCH_CHECK(stats.numel() == M * 2 * K * ana::kStatFeatures, "stats must be [M, 2K, 8]");
  tp.evoff = evoff.data_ptr<int64_t>();
  tp.events = events.data_ptr<int32_t>();
  tp.stats = stats.data_ptr<float>();
  if (dev.is_cuda()) tp.impl = ana::tele_impl();
  tp.fused_tail = (int32_t)knobs[4];
  // fused: < 0 inline in the rating groups (default, 11.4 ms per config 4 step); N > 0 one wave
  // in N aggregates tiles first (N = 2: 14.4 -> 11.4-11.7 ms, profiles/r2/tele_role_split.log)
  tp.role_stride = (int32_t)knobs[5];
  return tp;
}

// ------------------------------------------------------------ K1-K4, K6
void rate(Tensor rec, int64_t K, Tensor link, Tensor deps, Tensor state, Tensor attrs,
          Tensor first_prior, Tensor quality, Tensor status, Tensor s_mu, Tensor s_sig,
          Tensor delta, Tensor m_mu, Tensor m_sig, Tensor ctrl, Tensor vst, double beta2,
          double tau2, double unknown_sigma, bool record_first_prior, int64_t blocks,
          int64_t epoch, bool host_fp64, Tensor tele_evoff, Tensor tele_events, Tensor tele_stats,
          int64_t progress, int64_t progress_value, int64_t progress_at, int64_t epoch_ptr,
          int64_t chunk_len, bool ctrl_ready, std::vector<int64_t> knobs) {
  const auto dev = rec.device();
  TORCH_CHECK(knobs.size() == kKnobs, "knobs must be [idle, local, diag, tight, tele_fused_tail, tele_role]");
  const int64_t M = check_rec(rec, K, dev, "rate");
  const int64_t S = 2 * K;
  const int64_t P = check_state(state, dev, "rate");
  TORCH_CHECK(P >= 1 && P * ana::kRowFloats * 4 < 0x7fffffffLL,
              "roster size out of range (<= 16.7M players per device roster)");
  check_attrs(attrs, P, dev, "rate");
  const int64_t qrow = check_rows_view(quality, "quality", torch::kFloat32, dev, M, 1);
  const int64_t srow = check_rows_view(status, "status", torch::kUInt8, dev, M, 1);
  const int64_t row = check_rows_view(s_mu, "s_mu", torch::kFloat32, dev, M, S);
  for (const Tensor* t : {&s_sig, &delta, &m_mu, &m_sig})
    TORCH_CHECK(check_rows_view(*t, "per-slot output", torch::kFloat32, dev, M, S) == row,
                "per-slot outputs must share one row stride");
  float* fp = nullptr;
  if (record_first_prior) {
    check(first_prior, "first_prior", torch::kFloat32, dev);
    TORCH_CHECK(first_prior.sizes() == state.sizes(), "first_prior must match state");
    fp = first_prior.data_ptr<float>();
  }
  ana::RateOut out{quality.data_ptr<float>(), status.data_ptr<uint8_t>(), s_mu.data_ptr<float>(),
                   s_sig.data_ptr<float>(), delta.data_ptr<float>(), m_mu.data_ptr<float>(),
                   m_sig.data_ptr<float>(), row, qrow, srow};
  ana::RateParams prm{};
  prm.beta2 = (float)beta2;
  prm.tau2 = (float)tau2;
  prm.unknown_sigma = (float)unknown_sigma;
  prm.num_players = (int32_t)P;
  prm.num_matches = M;
  prm.record_first_prior = record_first_prior ? 1 : 0;
  prm.epoch_ptr = reinterpret_cast<const int32_t*>((intptr_t)epoch_ptr);
  TORCH_CHECK(prm.epoch_ptr ? dev.is_cuda() : (epoch >= 1 && epoch <= 255), "epoch must be 1..255");
  prm.epoch = (int32_t)epoch;
  prm.vst = check_vst(vst, dev, "rate");
  prm.idle_spins = (int32_t)knobs[0];
  prm.local_handoff = (int32_t)knobs[1];
  prm.diag = (int32_t)knobs[2];
  prm.tight_groups = (int32_t)knobs[3];
  prm.progress = reinterpret_cast<uint64_t*>((intptr_t)progress);
  prm.progress_value = (uint64_t)progress_value;
  prm.progress_at = progress_at;
  TORCH_CHECK(chunk_len >= 1 && chunk_len <= 64, "chunk_len must be 1..64");
  prm.chunk_len = (int32_t)chunk_len;
  prm.ctrl_ready = ctrl_ready ? 1 : 0;
  const ana::TelemetryParams tp = telemetry_params(tele_evoff, tele_events, tele_stats, M, K, dev, knobs);
  if (dev.is_cuda()) {
    check(link, "link", torch::kInt32, dev);
    check(deps, "deps", torch::kInt32, dev);
    check(ctrl, "ctrl", torch::kInt32, dev);
    // (by word count, not check_schedule's [M, 2K]: any view of the schedule's link words is taken)
    TORCH_CHECK(link.numel() == M * S * ana::kLinkWords, "link must be [M, 2K]");
    TORCH_CHECK(deps.numel() == M, "deps must have M entries");
    TORCH_CHECK(ctrl.numel() >= 52, "ctrl must have 52 entries");
    TORCH_CHECK(blocks >= 1 && blocks <= 65535, "blocks must be 1..65535");
    // the executor writes packed rows; other layouts go through a packed buffer
    const bool packed = out.s_sig == out.s_mu + S && out.delta == out.s_mu + 2 * S &&
                        out.m_mu == out.s_mu + 3 * S && out.m_sig == out.s_mu + 4 * S &&
                        out.quality == out.s_mu + 5 * S && qrow == row &&
                        (void*)out.status == (void*)(out.s_mu + 5 * S + 1) && srow == row * 4;
    Tensor staged;
    if (!packed) {
      const int64_t W = (5 * S + 2 + 31) / 32 * 32;
      staged = torch::empty({M, W}, state.options());
      float* b = staged.data_ptr<float>();
      out = ana::RateOut{b + 5 * S, reinterpret_cast<uint8_t*>(b + 5 * S + 1), b, b + S, b + 2 * S,
                         b + 3 * S, b + 4 * S, W, W, W * 4};
    }
    const int rc = ana::launch_rate((int)K, rec.data_ptr<int32_t>(), u32p(link), deps.data_ptr<int32_t>(),
                                    state.data_ptr<float>(), attrs.data_ptr<float>(), fp, out, u32p(ctrl), prm, tp,
                                    (int)blocks, stream_of(rec));
    check_hip(rc, "rate");
    if (!packed) {
      using torch::indexing::Slice;
      s_mu.copy_(staged.index({Slice(), Slice(0, S)}));
      s_sig.copy_(staged.index({Slice(), Slice(S, 2 * S)}));
      delta.copy_(staged.index({Slice(), Slice(2 * S, 3 * S)}));
      m_mu.copy_(staged.index({Slice(), Slice(3 * S, 4 * S)}));
      m_sig.copy_(staged.index({Slice(), Slice(4 * S, 5 * S)}));
      quality.copy_(staged.index({Slice(), 5 * S}));
      status.copy_(staged.view(torch::kUInt8).index({Slice(), 4 * (5 * S + 1)}));
    }
    if (prm.progress)  // releases the waiter even if the launch ended without firing
      check_hip((int)hipStreamWriteValue64(stream_of(rec), prm.progress, prm.progress_value, 0),
                "hipStreamWriteValue64");
  } else {
    TORCH_CHECK(ana::host_rate((int)K, host_fp64, rec.data_ptr<int32_t>(), state.data_ptr<float>(),
                               attrs.data_ptr<float>(), fp, out, prm) == 0, "bad K");
    if (tp.evoff) ana::host_telemetry((int)K, tp);
  }
}

// ------------------------------------------------------------------ K8
Tensor gen_event_counts(int64_t M, int64_t seed, int64_t min_events, int64_t max_events,
                        int64_t base, torch::Device device) {
  TORCH_CHECK(min_events >= 0 && max_events >= min_events, "need 0 <= min_events <= max_events");
  ana::GenEventParams g{(uint64_t)seed, (int32_t)min_events, (int32_t)max_events};
  auto counts = torch::empty({M}, torch::TensorOptions().dtype(torch::kInt64).device(device));
  if (device.is_cuda())
    check_hip(ana::launch_gen_event_counts(g, base, M, counts.data_ptr<int64_t>(),
                                           at::hip::getCurrentHIPStream(device.index()).stream()),
              "gen_event_counts");
  else
    ana::host_gen_event_counts(g, base, M, counts.data_ptr<int64_t>());
  return counts;
}

void gen_events(Tensor rec, int64_t K, Tensor evoff, int64_t seed, int64_t min_events,
                int64_t max_events, int64_t base, Tensor events) {
  const auto dev = rec.device();
  const int64_t M = check_rec(rec, K, dev, "gen_events");
  check(evoff, "evoff", torch::kInt64, dev);
  check(events, "events", torch::kInt32, dev);
  TORCH_CHECK(evoff.numel() == M + 1, "evoff must have M + 1 entries");
  TORCH_CHECK(events.dim() == 2 && events.size(1) == 2, "events must be [E, 2] (8-B events, telemetry_core.h)");
  ana::GenEventParams g{(uint64_t)seed, (int32_t)min_events, (int32_t)max_events};
  if (dev.is_cuda())
    check_hip(ana::launch_gen_events((int)K, g, base, rec.data_ptr<int32_t>(),
                                     evoff.data_ptr<int64_t>(), M, events.data_ptr<int32_t>(),
                                     stream_of(rec)), "gen_events");
  else
    TORCH_CHECK(ana::host_gen_events((int)K, g, base, rec.data_ptr<int32_t>(),
                                     evoff.data_ptr<int64_t>(), M, events.data_ptr<int32_t>()) == 0,
                "bad K");
}

// standalone aggregation; bad (device: int32[>=1] counter, host: ignored) counts malformed events
int64_t telemetry(Tensor evoff, Tensor events, int64_t K, Tensor stats, Tensor bad) {
  const auto dev = events.device();
  TORCH_CHECK(K >= 1 && K <= ana::kMaxTeamSize, "telemetry: K must be 1..5");
  const int64_t M = evoff.numel() - 1;
  TORCH_CHECK(M >= 0, "evoff must have M + 1 entries");
  // standalone: the fused-executor knobs do not apply
  const ana::TelemetryParams tp = telemetry_params(evoff, events, stats, M, K, dev, {0, 1, 0, -1, 0, 2});
  if (!tp.evoff) return 0;
  if (dev.is_cuda()) {
    check(bad, "bad", torch::kInt32, dev);
    TORCH_CHECK(bad.numel() >= 1, "bad must have an entry");
    const int rc = ana::launch_telemetry((int)K, tp, u32p(bad), stream_of(events));
    TORCH_CHECK(rc != (int)hipErrorNotSupported,
                "ANA_TELE_DEBUG / ANA_TELE_SPAN select diagnostic telemetry variants, which only the "
                "diagnostic library has: python -m analyzer_amd.build_ext --diag, then "
                "ANA_NATIVE_LIB=<path of analyzer_amd/_C_diag*.so>");
    check_hip(rc, "telemetry");
    return -1;
  }
  return ana::host_telemetry((int)K, tp);
}

// ------------------------------------------------------------- K9 / C1
void check_rows(const Tensor& t, const char* name, int64_t P, int64_t cols, const torch::Device& dev,
                torch::ScalarType ty = torch::kFloat32) {
  check(t, name, ty, dev);
  TORCH_CHECK(t.dim() == 2 && t.size(0) == P && t.size(1) == cols, name, " must be [P, ", cols, "]");
}

// the operands every K9 merge entry point takes: the window start s0 (base rows), the player
// attributes and the tier seed table, for a roster of P players on dev -> vst's pointer
const float* check_sweep(const Tensor& s0, const Tensor& attrs, const Tensor& vst, int64_t P,
                         const torch::Device& dev, const char* what) {
  check_rows(s0, "s0 (base rows)", P, ana::kBaseFloats, dev);
  check_attrs(attrs, P, dev, what);
  return check_vst(vst, dev, what);
}

// s0: common window start, prior: this rank's prior of the sweep (s0 itself in
// the first sweep), s: the posterior after the local shard
// K9 merge: s0 / prior / s2 are base rows [P, 16] = (mu, sigma) of the 8 granules
// (sweep_core.h kBaseFloats); s is the roster [P, 32]
void sweep_delta(Tensor s0, Tensor prior, Tensor s, Tensor attrs, Tensor vst, double unknown_sigma,
                 bool scaled, Tensor buf) {
  const auto dev = s.device();
  const int64_t P = s.size(0);
  const float* vp = check_sweep(s0, attrs, vst, P, dev, "sweep_delta");
  check_rows(prior, "prior (base rows)", P, ana::kBaseFloats, dev);
  check_rows(s, "state", P, ana::kRowFloats, dev);
  check_rows(buf, "buf", P, 16, dev);
  if (dev.is_cuda()) {
    check_hip(ana::launch_sweep_delta(s0.data_ptr<float>(), prior.data_ptr<float>(),
                                      s.data_ptr<float>(), attrs.data_ptr<float>(), vp,
                                      (float)unknown_sigma, scaled ? 1 : 0,
                                      buf.data_ptr<float>(), P, stream_of(s)), "sweep_delta");
  } else {
    ana::host_sweep_delta(s0.data_ptr<float>(), prior.data_ptr<float>(), s.data_ptr<float>(),
                          attrs.data_ptr<float>(), vp, (float)unknown_sigma, scaled, buf.data_ptr<float>(), P);
  }
}

// clamps: int32 [1] (empty: not counted) += the decoded tracks whose merged precision
// hit the floor (sweep_core.h sweep_apply_track); the merger raises on it
static uint32_t* clamp_ptr(const c10::optional<Tensor>& c, const torch::Device& dev) {
  if (!present(c)) return nullptr;
  check(*c, "clamps", torch::kInt32, dev);
  return u32p(*c);
}

// decoded rows to s and, if s2 is non-empty, base rows [P, 16] (sweep_core.h) to s2
void sweep_apply(Tensor s0, Tensor buf, Tensor attrs, Tensor s, Tensor s2, Tensor vst,
                 double unknown_sigma, bool scaled, const c10::optional<Tensor>& clamps) {
  const auto dev = s.device();
  uint32_t* cl = clamp_ptr(clamps, dev);
  const int64_t P = s.size(0);
  const float* vp = check_sweep(s0, attrs, vst, P, dev, "sweep_apply");
  check_rows(buf, "buf", P, 16, dev);
  check_rows(s, "state", P, ana::kRowFloats, dev);
  float* p2 = nullptr;
  if (s2.numel()) {
    check_rows(s2, "s2 (base rows)", P, ana::kBaseFloats, dev);
    p2 = s2.data_ptr<float>();
  }
  if (dev.is_cuda()) {
    check_hip(ana::launch_sweep_apply(s0.data_ptr<float>(), buf.data_ptr<float>(),
                                      attrs.data_ptr<float>(), s.data_ptr<float>(), p2, vp,
                                      (float)unknown_sigma, scaled ? 1 : 0, P, cl, stream_of(s)), "sweep_apply");
  } else {
    ana::host_sweep_apply(s0.data_ptr<float>(), buf.data_ptr<float>(), attrs.data_ptr<float>(),
                          s.data_ptr<float>(), p2, scaled, vp, (float)unknown_sigma, P, cl);
  }
}

// compressed merge operands: msg [P, 14] bf16/fp16, cnt [P, 1] int32 = the two base-16 touch
// fields packed as lo | hi << 16 (4 + 3 nibbles; sweep.hip); the CPU path goes through the
// fp32 host mirror and torch's conversions
// msg: [P, 14] rows with unit column stride and an even row stride (a separate [P, 14]
// tensor, or columns 0..13 of the split collective's [P, 16] operand rows); cnt: [P, 1] int32
// with any row stride (its own tensor, or word 7 of those rows)
static void check_operands(const Tensor& msg, const Tensor& cnt, int64_t P, const torch::Device& dev) {
  TORCH_CHECK(msg.device() == dev && msg.dim() == 2 && msg.size(0) == P && msg.size(1) == 14 &&
                  msg.stride(1) == 1 && msg.stride(0) % 2 == 0 &&
                  (msg.scalar_type() == torch::kBFloat16 || msg.scalar_type() == torch::kHalf),
              "msg must be [P, 14] bf16/fp16 rows (unit column stride, even row stride) on the state's device");
  TORCH_CHECK(cnt.device() == dev && cnt.scalar_type() == torch::kInt32 && cnt.dim() == 2 && cnt.size(0) == P &&
                  cnt.size(1) == 1,
              "cnt must be [P, 1] int32 on the state's device");
  TORCH_CHECK(aligned(msg, 4), "msg rows must be 4-B aligned");
}

static Tensor pack_touch(const Tensor& lohi) {  // [P, 2] float fields -> [P, 1] int32
  const Tensor x = lohi.to(torch::kInt32);
  return x.slice(1, 0, 1).bitwise_or(x.slice(1, 1, 2).bitwise_left_shift(16));
}
static Tensor unpack_touch(const Tensor& cnt) {  // [P, 1] int32 -> [P, 2] (lo, hi)
  return torch::cat({cnt.bitwise_and(0xffff), cnt.bitwise_right_shift(16)}, 1);
}
void sweep_delta_packed(Tensor s0, Tensor prior, Tensor s, Tensor attrs, Tensor vst, double unknown_sigma,
                        Tensor msg, Tensor cnt) {
  const auto dev = s.device();
  const int64_t P = s.size(0);
  const float* vp = check_sweep(s0, attrs, vst, P, dev, "sweep_delta_packed");
  check_rows(prior, "prior (base rows)", P, ana::kBaseFloats, dev);
  check_rows(s, "state", P, ana::kRowFloats, dev);
  check_operands(msg, cnt, P, dev);
  if (dev.is_cuda()) {
    check_hip(ana::launch_sweep_delta_packed(s0.data_ptr<float>(), prior.data_ptr<float>(), s.data_ptr<float>(),
                                             attrs.data_ptr<float>(), vp, (float)unknown_sigma, is_bf16(msg),
                                             msg.data_ptr(), cnt.data_ptr<int32_t>(), P, stream_of(s),
                                             msg.stride(0) / 2, cnt.stride(0)),
              "sweep_delta_packed");
    return;
  }
  Tensor buf = torch::empty({P, 16}, s.options());
  ana::host_sweep_delta(s0.data_ptr<float>(), prior.data_ptr<float>(), s.data_ptr<float>(),
                        attrs.data_ptr<float>(), vp, (float)unknown_sigma, true, buf.data_ptr<float>(), P);
  msg.copy_(buf.slice(1, 0, 14));
  cnt.copy_(pack_touch(buf.slice(1, 14, 16)));
}

void prefix_delta(Tensor s0, Tensor prefix, Tensor attrs, Tensor vst, double unknown_sigma, Tensor delta);

void sweep_apply_packed(Tensor s0, Tensor msg, Tensor cnt, Tensor attrs, Tensor s, Tensor s2, Tensor vst,
                        double unknown_sigma, const c10::optional<Tensor>& clamps,
                        const c10::optional<Tensor>& prefix, const c10::optional<Tensor>& delta) {
  const auto dev = s.device();
  uint32_t* cl = clamp_ptr(clamps, dev);
  const int64_t P = s.size(0);
  const float* vp = check_sweep(s0, attrs, vst, P, dev, "sweep_apply_packed");
  check_operands(msg, cnt, P, dev);
  check_rows(s, "state", P, ana::kRowFloats, dev);
  float* p2 = nullptr;
  if (s2.numel()) {
    check_rows(s2, "s2 (base rows)", P, ana::kBaseFloats, dev);
    p2 = s2.data_ptr<float>();
  }
  const bool with_prefix = present(prefix);
  if (with_prefix) {
    TORCH_CHECK(delta.has_value() && delta->defined(), "a prefix needs a delta table");
    TORCH_CHECK(prefix->scalar_type() == msg.scalar_type() && prefix->is_contiguous() && prefix->device() == dev &&
                    prefix->sizes() == msg.sizes(),
                "prefix must be a contiguous [P, 14] tensor of msg's type");
    check_rows(*delta, "delta", P, 16, dev);
  }
  if (dev.is_cuda()) {
    check_hip(ana::launch_sweep_apply_packed(s0.data_ptr<float>(), msg.data_ptr(), cnt.data_ptr<int32_t>(),
                                             is_bf16(msg), attrs.data_ptr<float>(), s.data_ptr<float>(), p2, vp,
                                             (float)unknown_sigma, P, cl,
                                             with_prefix ? prefix->data_ptr() : nullptr,
                                             with_prefix ? delta->data_ptr<float>() : nullptr, stream_of(s),
                                             msg.stride(0) / 2, cnt.stride(0)),
              "sweep_apply_packed");
    return;
  }
  if (with_prefix)  // (before the host decode: it overwrites the window start through s2)
    prefix_delta(s0, *prefix, attrs, vst, unknown_sigma, *delta);
  Tensor buf = torch::empty({P, 16}, s.options());
  buf.slice(1, 0, 14).copy_(msg);
  buf.slice(1, 14, 16).copy_(unpack_touch(cnt));
  ana::host_sweep_apply(s0.data_ptr<float>(), buf.data_ptr<float>(), attrs.data_ptr<float>(),
                        s.data_ptr<float>(), p2, true, vp, (float)unknown_sigma, P, cl);
}

// the split collective's owner reduce (sweep.hip): recv [N * blk, 8] int32 words of
// bf16 / fp16 halves + the touch word -> total [blk, 8] and, when given, the exclusive
// prefixes pref [N * blk, 7] (device tensors; the CPU path is parallel/comm.py)
void sweep_block_reduce(Tensor recv, int64_t N, bool bf16, Tensor total, const c10::optional<Tensor>& pref) {
  const auto dev = recv.device();
  TORCH_CHECK(dev.is_cuda(), "sweep_block_reduce: device tensors (the host path is parallel/comm.py)");
  check(recv, "recv", torch::kInt32, dev);
  check(total, "total", torch::kInt32, dev);
  TORCH_CHECK(N >= 1 && recv.dim() == 2 && recv.size(1) == 8 && recv.size(0) % N == 0, "recv must be [N * blk, 8]");
  const int64_t blk = recv.size(0) / N;
  TORCH_CHECK(total.dim() == 2 && total.size(0) == blk && total.size(1) == 8, "total must be [blk, 8]");
  int32_t* pp = nullptr;
  if (present(pref)) {
    check(*pref, "pref", torch::kInt32, dev);
    TORCH_CHECK(pref->dim() == 2 && pref->size(0) == N * blk && pref->size(1) == 7, "pref must be [N * blk, 7]");
    pp = pref->data_ptr<int32_t>();
  }
  check_hip(ana::launch_sweep_block_reduce(recv.data_ptr<int32_t>(), (int)N, blk, bf16 ? 1 : 0,
                                           total.data_ptr<int32_t>(), pp, stream_of(recv)),
            "sweep_block_reduce");
}

// causal record correction of a window's records (parallel/sweep.py): rows = RateResult
// packed [M, row] += delta [P, 16] fp32 (raw natural-parameter increments per track)
void correct_records(Tensor rec, int64_t K, Tensor rows, Tensor delta) {
  const auto dev = rows.device();
  const int64_t M = check_rec(rec, K, dev, "correct_records");
  TORCH_CHECK(rows.dim() == 2 && rows.size(0) == M && rows.scalar_type() == torch::kFloat32 && rows.stride(1) == 1 &&
                  rows.size(1) >= 5 * 2 * K + 2,
              "rows must be RateResult.packed [M, row] fp32");
  const int64_t P = delta.size(0);
  check_rows(delta, "delta", P, 16, dev);
  if (dev.is_cuda()) {
    check_hip(ana::launch_correct_records((int)K, rec.data_ptr<int32_t>(), M, rows.data_ptr<float>(), rows.stride(0),
                                          delta.data_ptr<float>(), P, stream_of(rows)),
              "correct_records");
    return;
  }
  ana::host_correct_records((int)K, rec.data_ptr<int32_t>(), M, rows.data_ptr<float>(), rows.stride(0),
                            delta.data_ptr<float>(), P);
}

// the record correction's delta table [P, 16] of a scaled (bf16 / fp16) prefix [P, 14]
// against the window start s0 [P, 16] (the fused decode computes it in production)
void prefix_delta(Tensor s0, Tensor prefix, Tensor attrs, Tensor vst, double unknown_sigma, Tensor delta) {
  const auto dev = s0.device();
  const int64_t P = s0.size(0);
  const float* vp = check_sweep(s0, attrs, vst, P, dev, "prefix_delta");
  check_rows(delta, "delta", P, 16, dev);
  TORCH_CHECK(prefix.device() == dev && prefix.is_contiguous() && prefix.dim() == 2 && prefix.size(0) == P &&
                  prefix.size(1) == 14 &&
                  (prefix.scalar_type() == torch::kBFloat16 || prefix.scalar_type() == torch::kHalf),
              "prefix must be a contiguous bf16 / fp16 [P, 14]");
  if (dev.is_cuda()) {
    check_hip(ana::launch_prefix_delta(s0.data_ptr<float>(), prefix.data_ptr(), is_bf16(prefix),
                                       attrs.data_ptr<float>(), vp, (float)unknown_sigma, delta.data_ptr<float>(), P,
                                       stream_of(s0)),
              "prefix_delta");
    return;
  }
  Tensor pf = prefix.to(torch::kFloat32).contiguous();
  ana::host_prefix_delta(s0.data_ptr<float>(), pf.data_ptr<float>(), attrs.data_ptr<float>(), vp,
                         (float)unknown_sigma, delta.data_ptr<float>(), P);
}

// ------------------------------------------------------------- C2 exchange
// rec: the rank's slice of one round [m, 2K+2]; status: its per-match status
// (any row stride); out: [cap, 33] float entries, cap >= m * 2K
void pack_rows(Tensor rec, int64_t K, Tensor status, Tensor state, Tensor out) {
  const auto dev = state.device();
  const int64_t m = check_rec(rec, K, dev, "pack_rows");
  const int64_t P = check_state(state, dev, "pack_rows");
  check(out, "out", torch::kFloat32, dev);
  TORCH_CHECK(out.dim() == 2 && out.size(1) == 33 && out.size(0) >= m * 2 * K, "out must be [cap >= m*2K, 33]");
  const int64_t sstride = check_rows_view(status, "status", torch::kUInt8, dev, m, 1);
  if (dev.is_cuda()) {
    check_hip(ana::launch_pack_rows(rec.data_ptr<int32_t>(), (int)K, m, status.data_ptr<uint8_t>(), sstride,
                                    state.data_ptr<float>(), out.data_ptr<float>(), out.size(0),
                                    stream_of(state)), "pack_rows");
    return;
  }
  TORCH_CHECK(ana::host_pack_rows(rec.data_ptr<int32_t>(), (int)K, m, status.data_ptr<uint8_t>(), sstride,
                                  state.data_ptr<float>(), P, out.data_ptr<float>(), out.size(0)) == 0, "bad K");
}

// C2 race detector: rec [M, 2K+2] (the window), idx int64 [m] (one round's matches),
// owner int64 [P] (zeroed once per window), flag int32 [1]
void check_round(Tensor rec, int64_t K, Tensor idx, int64_t round, Tensor owner, Tensor flag) {
  const auto dev = rec.device();
  check_rec(rec, K, dev, "check_round");
  check(idx, "idx", torch::kInt64, dev);
  check(owner, "owner", torch::kInt64, dev);
  check(flag, "flag", torch::kInt32, dev);
  TORCH_CHECK(round >= 0 && round < 0xffffffffLL, "round out of range");
  const int64_t m = idx.numel(), P = owner.numel();
  if (dev.is_cuda()) {
    check_hip(ana::launch_check_round(rec.data_ptr<int32_t>(), (int)K, idx.data_ptr<int64_t>(), m, P,
                                      (uint32_t)round,
                                      reinterpret_cast<unsigned long long*>(owner.data_ptr<int64_t>()),
                                      u32p(flag), stream_of(rec)),
              "check_round");
    return;
  }
  TORCH_CHECK(ana::host_check_round(rec.data_ptr<int32_t>(), (int)K, idx.data_ptr<int64_t>(), m, P, (uint32_t)round,
                                    reinterpret_cast<uint64_t*>(owner.data_ptr<int64_t>()),
                                    flag.data_ptr<int32_t>()) == 0, "bad K");
}

void unpack_rows(Tensor buf, Tensor state) {
  const auto dev = state.device();
  check(buf, "buf", torch::kFloat32, dev);
  TORCH_CHECK(buf.dim() == 2 && buf.size(1) == 33, "buf must be [n, 33]");
  const int64_t n = buf.size(0), P = check_state(state, dev, "unpack_rows");
  if (dev.is_cuda()) {
    check_hip(ana::launch_unpack_rows(buf.data_ptr<float>(), n, state.data_ptr<float>(), stream_of(state)),
              "unpack_rows");
    return;
  }
  ana::host_unpack_rows(buf.data_ptr<float>(), n, state.data_ptr<float>(), P);
}

// A HIP stream restricted to ``num_cus`` compute units, spread evenly over the
// device's CUs (and so over its XCDs).  Used for the schedule prepass so its
// bandwidth-bound kernels trickle alongside the latency-bound executor instead
// of bursting.  Returns the raw handle for torch.cuda.ExternalStream; the
// stream lives until process exit (one per pipeline).
int64_t cu_masked_stream(int64_t device, int64_t num_cus, bool invert) {
  hipDeviceProp_t prop;
  check_hip((int)hipGetDeviceProperties(&prop, (int)device), "hipGetDeviceProperties");
  const int total = prop.multiProcessorCount;
  TORCH_CHECK(num_cus >= 1 && num_cus <= total, "num_cus must be 1..", total);
  std::vector<uint32_t> mask((total + 31) / 32, 0u);
  for (int64_t i = 0; i < num_cus; ++i) {
    const int cu = (int)(i * total / num_cus);
    mask[cu / 32] |= 1u << (cu % 32);
  }
  if (invert) {  // every CU but those N (the complement of the same call without invert)
    for (int c = 0; c < total; ++c) mask[c / 32] ^= 1u << (c % 32);
    TORCH_CHECK(num_cus < total, "an inverted mask needs num_cus < ", total);
  }
  int prev = 0;
  check_hip((int)hipGetDevice(&prev), "hipGetDevice");
  check_hip((int)hipSetDevice((int)device), "hipSetDevice");
  hipStream_t st = nullptr;
  const hipError_t e = hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data());
  check_hip((int)hipSetDevice(prev), "hipSetDevice");
  check_hip((int)e, "hipExtStreamCreateWithCUMask");
  return (int64_t)reinterpret_cast<intptr_t>(st);
}

// Tail overlap (runtime/engine.py): an 8-B word in signal memory that the
// executor stores its launch number to when the launch reaches its tail, and a
// stream wait on it.  The handle is the device address (lives until exit).
int64_t progress_signal(int64_t device) {
  int prev = 0;
  check_hip((int)hipGetDevice(&prev), "hipGetDevice");
  check_hip((int)hipSetDevice((int)device), "hipSetDevice");
  void* p = nullptr;
  hipError_t e = hipExtMallocWithFlags(&p, 8, hipMallocSignalMemory);
  if (e == hipSuccess) e = hipMemset(p, 0, 8);
  check_hip((int)hipSetDevice(prev), "hipSetDevice");
  check_hip((int)e, "hipExtMallocWithFlags(hipMallocSignalMemory)");
  return (int64_t)reinterpret_cast<intptr_t>(p);
}

void stream_wait_value64(int64_t stream, int64_t ptr, int64_t value) {
  check_hip((int)hipStreamWaitValue64(reinterpret_cast<hipStream_t>((intptr_t)stream),
                                      reinterpret_cast<void*>((intptr_t)ptr), (uint64_t)value,
                                      hipStreamWaitValueGte),
            "hipStreamWaitValue64");
}

// the host side of a tail gate: write ``value`` to the signal word in stream order (releases
// waiters whose launch will not come, runtime/engine.py)
void stream_write_value64(int64_t stream, int64_t ptr, int64_t value) {
  check_hip((int)hipStreamWriteValue64(reinterpret_cast<hipStream_t>((intptr_t)stream),
                                       reinterpret_cast<void*>((intptr_t)ptr), (uint64_t)value, 0),
            "hipStreamWriteValue64");
}

bool can_wait_value(int64_t device) {
  int v = 0;
  return hipDeviceGetAttribute(&v, hipDeviceAttributeCanUseStreamWaitValue, (int)device) ==
             hipSuccess && v != 0;
}

// ------------------------------------------------------------------ ingest (P3)
void write_record_file(const std::string& path, Tensor rec, int64_t K) {
  const int64_t M = check_rec(rec, K, torch::Device(torch::kCPU), "write_record_file");
  ana::write_record_file(path, rec.data_ptr<int32_t>(), M, (int)K);
}

static py::object reader_acquire(ana::RecordReader& r) {
  int slot = 0;
  int64_t base = 0, n = 0;
  bool ok;
  {
    py::gil_scoped_release nogil;  // the producer thread may still be reading
    ok = r.acquire(&slot, &base, &n);
  }
  if (!ok) return py::none();
  auto t = torch::from_blob(r.slot_data(slot), {n, 2 * (int64_t)r.K() + 2},
                            torch::TensorOptions().dtype(torch::kInt32));
  return py::make_tuple(slot, base, t);
}

void epoch_bump(Tensor e) {
  TORCH_CHECK(e.is_cuda() && e.scalar_type() == torch::kInt32 && e.numel() >= 1, "epoch must be a device int32 tensor");
  check_hip(ana::launch_epoch_bump(e.data_ptr<int32_t>(), stream_of(e)), "epoch_bump");
}

// the all-reduce stand-in of one-GPU DP pricing (kernels.hip emulate_allreduce_kernel)
void emulate_allreduce(Tensor buf, int64_t channels, int64_t passes, double us) {
  TORCH_CHECK(buf.is_cuda() && buf.is_contiguous(), "emulate_allreduce: a contiguous device tensor");
  check_hip(ana::launch_emulate_allreduce(buf.data_ptr(), (int64_t)(buf.numel() * buf.element_size()), (int)channels,
                                          (int)passes, us, stream_of(buf)),
            "emulate_allreduce");
}

void warm_rows(Tensor state, Tensor sink) {
  const auto dev = state.device();
  const int64_t P = check_state(state, dev, "warm_rows");
  check(sink, "sink", torch::kInt32, dev);
  TORCH_CHECK(sink.numel() >= 256, "sink needs 256 words");
  if (!dev.is_cuda()) return;  // nothing to warm on the host
  check_hip(ana::launch_warm_rows(state.data_ptr<float>(), P, u32p(sink), stream_of(state)), "warm_rows");
}

// runtime/rerate.py window digest of the packed output rows (digest.hip); out [3 + 10K] fp64
void records_digest(Tensor rows, int64_t K, Tensor scratch, Tensor out, const c10::optional<Tensor>& hist) {
  const auto dev = rows.device();
  check(rows, "rows", torch::kFloat32, dev);
  check(scratch, "scratch", torch::kFloat64, dev);
  check(out, "out", torch::kFloat64, dev);
  TORCH_CHECK(K >= 1 && K <= ana::kMaxTeamSize, "records_digest: K must be 1..5");
  TORCH_CHECK(rows.dim() == 2 && rows.size(1) >= 10 * K + 2 && rows.size(1) % 4 == 0 &&
                  256 % (rows.size(1) / 4) == 0,
              "records_digest: rows must be the packed [M, W] output rows (W / 4 a divisor of 256)");
  TORCH_CHECK(out.numel() == 3 + 10 * K, "records_digest: out needs 3 + 10K doubles");
  TORCH_CHECK(aligned(rows, 16), "records_digest: rows must be 16-B aligned");
  TORCH_CHECK(dev.is_cuda(), "records_digest: device rows (the host path is runtime/rerate.py window_digest)");
  TORCH_CHECK((size_t)scratch.numel() >= ana::records_digest_scratch_doubles((int)K), "records_digest: scratch too small");
  int64_t* h = nullptr;
  if (hist.has_value()) {
    check(*hist, "hist", torch::kInt64, dev);
    TORCH_CHECK(hist->numel() == 256, "records_digest: hist must be int64[256]");
    h = hist->data_ptr<int64_t>();
  }
  check_hip(ana::launch_records_digest((int)K, rows.data_ptr<float>(), rows.size(0), rows.size(1),
                                       scratch.data_ptr<double>(), out.data_ptr<double>(), h, stream_of(rows)),
            "records_digest");
}

int64_t records_digest_scratch(int64_t K) { return (int64_t)ana::records_digest_scratch_doubles((int)K); }

// K10 (select.hip; host mirror host.cpp records_select_host): hits [n, 12] int32 of the bitmap's
// players in a window's records joined with its packed output rows, ascending (match, slot).
// Dispatches on the tensors' device; the device path synchronises once to size hits exactly.
Tensor records_select(Tensor rec, Tensor rows, int64_t base, int64_t P, Tensor bitmap) {
  const auto dev = rec.device();
  TORCH_CHECK(rec.dim() == 2, "records_select: rec must be [M, 2K+2] with K in 1..5");
  const int64_t K = (rec.size(1) - 2) / 2;
  const int64_t M = check_window(rec, rows, K, dev, "records_select");  // K outside 1..5 and odd widths included
  check(bitmap, "bitmap", torch::kInt32, dev);
  TORCH_CHECK(P >= 0 && P <= 0x7fffffffLL, "records_select: P must fit in int32");
  TORCH_CHECK(base >= 0, "records_select: base must be >= 0");
  TORCH_CHECK(bitmap.dim() == 1 && bitmap.numel() >= (P + 31) / 32, "records_select: bitmap needs ceil(P / 32) words");
  const uint32_t* bm = u32p(bitmap);
  const auto i32 = torch::TensorOptions().dtype(torch::kInt32).device(dev);
  if (!dev.is_cuda()) {
    const int64_t n = ana::records_select_host((int)K, rec.data_ptr<int32_t>(), rows.data_ptr<float>(), rows.size(1),
                                               M, base, P, bm, nullptr);
    Tensor hits = torch::empty({n, (int64_t)ana::kHitWords}, i32);
    ana::records_select_host((int)K, rec.data_ptr<int32_t>(), rows.data_ptr<float>(), rows.size(1), M, base, P, bm,
                             hits.data_ptr<int32_t>());
    return hits;
  }
  const int64_t tiles = ana::records_select_tiles(M);
  Tensor counts = torch::empty({tiles}, i32);
  Tensor offsets = torch::empty({tiles + 1}, i32.dtype(torch::kInt64));
  check_hip(ana::launch_records_select_count((int)K, rec.data_ptr<int32_t>(), rows.data_ptr<float>(), rows.size(1), M,
                                             P, bm, u32p(counts), offsets.data_ptr<int64_t>(), stream_of(rec)),
            "records_select (count)");
  const int64_t n = offsets[tiles].item<int64_t>();  // the one synchronisation of a call
  TORCH_CHECK(n >= 0 && n <= M * 2 * K, "records_select: impossible hit count ", n);
  Tensor hits = torch::empty({n, (int64_t)ana::kHitWords}, i32);
  check_hip(ana::launch_records_select_emit((int)K, rec.data_ptr<int32_t>(), rows.data_ptr<float>(), rows.size(1), M,
                                            base, P, bm, offsets.data_ptr<int64_t>(), hits.data_ptr<int32_t>(), n,
                                            stream_of(rec)),
            "records_select (emit)");
  return hits;
}

// the scan between the count and emit launches of K10 and K15 on its own, for the tests
Tensor tile_offsets(Tensor counts) {
  TORCH_CHECK(counts.is_cuda(), "tile_offsets: counts must be on the device");
  check(counts, "counts", torch::kInt32, counts.device());
  TORCH_CHECK(counts.dim() == 1, "tile_offsets: counts must be [T]");
  Tensor offsets = torch::empty({counts.numel() + 1}, counts.options().dtype(torch::kInt64));
  check_hip(ana::launch_tile_offsets(u32p(counts), counts.numel(), offsets.data_ptr<int64_t>(), stream_of(counts)),
            "tile_offsets");
  return offsets;
}

// The leading checks of careers_add and profiles_add: the window, its slots, P, the table
// [P, words] int32 and the options -> (K, M)
std::pair<int64_t, int64_t> check_fold_args(const Tensor& table, int64_t words, const Tensor& rec, const Tensor& rows,
                                            int64_t P, int64_t track, int64_t score, int64_t modes, const char* what) {
  const auto dev = table.device();
  const int64_t K = team_size_of(rec, what);
  const int64_t M = check_window(rec, rows, K, dev, what);
  check_slots(M, K, what);
  TORCH_CHECK(P >= 0 && P <= 0x7fffffffLL, what, ": P must fit in int32");
  check_rows(table, "table", P, words, dev, torch::kInt32);
  TORCH_CHECK(track == ana::kCareerShared || track == ana::kCareerMode, what, ": unknown track ", track);
  TORCH_CHECK(score == ana::kLadderConservative || score == ana::kLadderMu, what, ": unknown score ", score);
  TORCH_CHECK(modes >= 0 && (modes & ~(int64_t)ana::kCareerAllModes) == 0, what,
              ": the modes mask must name modes 0..5");
  return {K, M};
}

// K13 (career.hip; host mirror host.cpp host_careers_add): folds the games of one window -- rec
// [M, 2K+2] joined with its packed output rows [M, W], base the global index of match 0 -- into
// the career table [P, 16] int32 in place (career_core.h).  Dispatches on the tensors' device;
// the device path is four stream-ordered steps (keys, sort, fold, stitch) without a host read.
void careers_add(Tensor table, Tensor rec, Tensor rows, int64_t base, int64_t P, int64_t track, int64_t score,
                 int64_t modes) {
  const auto dev = table.device();
  const auto [K, M] = check_fold_args(table, ana::kCareerWords, rec, rows, P, track, score, modes, "careers_add");
  TORCH_CHECK(base >= 0, "careers_add: base must be >= 0");
  if (M == 0 || P == 0) return;
  if (!dev.is_cuda()) {
    TORCH_CHECK(ana::host_careers_add((int)K, rec.data_ptr<int32_t>(), rows.data_ptr<float>(), rows.size(1), M, base,
                                      P, (int)track, (int)score, (uint32_t)modes, table.data_ptr<int32_t>()) == 0,
                "careers_add: bad arguments");
    return;
  }
  TORCH_CHECK(aligned(table, 16), "careers_add: table must be 16-B aligned");
  const hipStream_t s = stream_of(table);
  const int64_t n = M * 2 * K;
  Tensor events = torch::empty({n, (int64_t)ana::kCareerEventWords}, rec.options());
  const auto sorted = sort_by_player(n, P, ana::career_edge_bytes(n), dev, s, [&](uint32_t* keys, uint32_t* vals) {
    check_hip(ana::launch_career_keys((int)K, rec.data_ptr<int32_t>(), rows.data_ptr<float>(), rows.size(1), M, P,
                                      (int)track, (int)score, (uint32_t)modes, keys, vals, u32p(events), s),
              "career_keys");
  });
  check_hip(ana::launch_career_fold(u32p(sorted.keys), u32p(sorted.vals), u32p(events), n, (int)K, base, P,
                                    table.data_ptr<int32_t>(), sorted.edges.data_ptr<uint8_t>(), s),
            "career_fold");
}

// K17 (profile.hip; host mirror host.cpp host_profiles_add): folds the games of one window -- rec
// [M, 2K+2] joined with its packed output rows [M, W] and its stat vectors stats [M, 2K, 8] --
// into the player table [P, 20] int32 and the baseline table cells [6 * B * 2 * 9 + 2] int64 in
// place (profile_core.h); edges: the B - 1 bracket edges, fp32 on the CPU.  Dispatches on the
// tensors' device; the device path is four stream-ordered steps (keys, sort, fold, stitch).
void profiles_add(Tensor table, Tensor cells, Tensor rec, Tensor rows, Tensor stats, int64_t P, int64_t track,
                  int64_t score, int64_t modes, Tensor edges) {
  const auto dev = table.device();
  const auto [K, M] = check_fold_args(table, ana::kProfileWords, rec, rows, P, track, score, modes, "profiles_add");
  check(stats, "stats", torch::kFloat32, dev);
  TORCH_CHECK(stats.dim() == 3 && stats.size(0) == M && stats.size(1) == 2 * K && stats.size(2) == ana::kProfileStats,
              "profiles_add: stats must be [M, 2K, 8]");
  check(edges, "edges", torch::kFloat32, torch::Device(torch::kCPU));
  TORCH_CHECK(edges.dim() == 1 && edges.numel() <= ana::kProfileMaxEdges, "profiles_add: at most ",
              ana::kProfileMaxEdges, " edges");
  const int n_edges = (int)edges.numel();
  const float* ep = edges.data_ptr<float>();
  for (int i = 0; i < n_edges; ++i)
    TORCH_CHECK(std::isfinite(ep[i]) && (i == 0 || ep[i - 1] < ep[i]),
                "profiles_add: edges must be finite and strictly ascending");
  check(cells, "cells", torch::kInt64, dev);
  TORCH_CHECK(cells.numel() == ana::profile_table_words(n_edges + 1), "profiles_add: cells must hold ",
              ana::profile_table_words(n_edges + 1), " words");
  if (M == 0 || P == 0) return;
  if (!dev.is_cuda()) {
    TORCH_CHECK(ana::host_profiles_add((int)K, rec.data_ptr<int32_t>(), rows.data_ptr<float>(), rows.size(1),
                                       stats.data_ptr<float>(), M, P, (int)track, (int)score, (uint32_t)modes, ep,
                                       n_edges, table.data_ptr<int32_t>(), cells.data_ptr<int64_t>()) == 0,
                "profiles_add: bad arguments");
    return;
  }
  TORCH_CHECK(aligned(table, 16) && aligned(stats, 16), "profiles_add: table and stats must be 16-B aligned");
  const hipStream_t s = stream_of(table);
  const int64_t n = M * 2 * K;
  const auto sorted = sort_by_player(n, P, ana::profile_edge_bytes(n), dev, s, [&](uint32_t* keys, uint32_t* vals) {
    check_hip(ana::launch_profile_keys((int)K, rec.data_ptr<int32_t>(), rows.data_ptr<float>(), rows.size(1),
                                       stats.data_ptr<float>(), M, P, (int)track, (int)score, (uint32_t)modes, ep,
                                       n_edges, keys, vals, cells.data_ptr<int64_t>(), s),
              "profile_keys");
  });
  check_hip(ana::launch_profile_fold(u32p(sorted.keys), u32p(sorted.vals), stats.data_ptr<float>(), n, (int)K, P,
                                     table.data_ptr<int32_t>(), sorted.edges.data_ptr<uint8_t>(), s),
            "profile_fold");
}

// K19 (expect.hip; host mirror host.cpp host_expect_add): folds the games of one window -- rec
// [M, 2K+2] joined with the raw priors [M, 4, 2K] (or [M, 8K]) of priors_add and the pred rows
// [M, 4] of score_add(keep=True) -- into the player table [P, 24] int32 and the counter bad int64
// [1] in place (expect_core.h).  Dispatches on the tensors' device; the device path is four
// stream-ordered steps (keys, sort, fold, stitch) without a host read.
void expect_add(Tensor table, Tensor bad, Tensor rec, Tensor priors, Tensor pred, int64_t P, int64_t track) {
  const auto dev = table.device();
  const int64_t K = team_size_of(rec, "expect_add");
  const int64_t M = check_rec(rec, K, dev, "expect_add");
  check_slots(M, K, "expect_add");
  TORCH_CHECK(P >= 0 && P <= 0x7fffffffLL, "expect_add: P must fit in int32");
  check_rows(table, "table", P, ana::kExpectWords, dev, torch::kInt32);
  check(bad, "bad", torch::kInt64, dev);
  TORCH_CHECK(bad.numel() == 1, "expect_add: bad must hold one word");
  check(priors, "priors", torch::kFloat32, dev);
  TORCH_CHECK((priors.dim() == 2 && priors.size(0) == M && priors.size(1) == 8 * K) ||
                  (priors.dim() == 3 && priors.size(0) == M && priors.size(1) == 4 && priors.size(2) == 2 * K),
              "expect_add: priors must be [M, 4, 2K] of rec's matches");
  check_rows(pred, "pred", M, ana::kPredWords, dev, torch::kInt32);
  TORCH_CHECK(track == ana::kScoreShared || track == ana::kScoreMode, "expect_add: unknown track ", track);
  if (M == 0 || P == 0) return;
  if (!dev.is_cuda()) {
    TORCH_CHECK(ana::host_expect_add((int)K, rec.data_ptr<int32_t>(), priors.data_ptr<float>(),
                                     pred.data_ptr<int32_t>(), M, P, (int)track, table.data_ptr<int32_t>(),
                                     bad.data_ptr<int64_t>()) == 0,
                "expect_add: bad arguments");
    return;
  }
  TORCH_CHECK(aligned(rec, K % 2 == 0 ? 8 : 16) && aligned(table, 16) && aligned(priors, 16) && aligned(pred, 16),
              "expect_add: rec, table, priors and pred must be 16-B aligned");
  const hipStream_t s = stream_of(table);
  const int64_t n = M * 2 * K;
  Tensor terms = torch::empty({n, (int64_t)ana::kExpectTermWords}, rec.options());
  const auto sorted = sort_by_player(n, P, ana::expect_edge_bytes(n), dev, s, [&](uint32_t* keys, uint32_t* vals) {
    check_hip(ana::launch_expect_keys((int)K, rec.data_ptr<int32_t>(), priors.data_ptr<float>(),
                                      pred.data_ptr<int32_t>(), M, P, (int)track, keys, vals, terms.data_ptr<int32_t>(),
                                      bad.data_ptr<int64_t>(), s),
              "expect_keys");
  });
  check_hip(ana::launch_expect_fold(u32p(sorted.keys), u32p(sorted.vals), terms.data_ptr<int32_t>(), n, (int)K, P,
                                    table.data_ptr<int32_t>(), sorted.edges.data_ptr<uint8_t>(), s),
            "expect_fold");
}

// K18 (islands.hip; host mirror host.cpp host_islands_*; island_core.h): the state of an island
// forest -- parent, slots, credit int32 [P] and ctrl int64 [2] on one device -> that device
torch::Device check_island_state(const Tensor& parent, const Tensor* slots, const Tensor* credit, const Tensor* ctrl,
                                 int64_t P, const char* what) {
  const auto dev = parent.device();
  TORCH_CHECK(P >= 0 && P <= 0x7fffffffLL, what, ": P must fit in int32");
  check(parent, "parent", torch::kInt32, dev);
  TORCH_CHECK(parent.dim() == 1 && parent.numel() == P, what, ": parent must be [P]");
  if (slots != nullptr) {
    check(*slots, "slots", torch::kInt32, dev);
    TORCH_CHECK(slots->dim() == 1 && slots->numel() == P, what, ": slots must be [P]");
  }
  if (credit != nullptr) {
    check(*credit, "credit", torch::kInt32, dev);
    TORCH_CHECK(credit->dim() == 1 && credit->numel() == P, what, ": credit must be [P]");
  }
  if (ctrl != nullptr) {
    check(*ctrl, "ctrl", torch::kInt64, dev);
    TORCH_CHECK(ctrl->numel() == ana::kIslandCtrlWords, what, ": ctrl must hold ", ana::kIslandCtrlWords, " words");
  }
  return dev;
}

// unites the live slots of every rated match of one window -- rec [M, 2K+2] joined with its
// packed output rows [M, W] -- and counts them, in place
void islands_add(Tensor parent, Tensor slots, Tensor credit, Tensor ctrl, Tensor rec, Tensor rows, int64_t P,
                 int64_t modes) {
  const auto dev = check_island_state(parent, &slots, &credit, &ctrl, P, "islands_add");
  const int64_t K = team_size_of(rec, "islands_add");
  const int64_t M = check_window(rec, rows, K, dev, "islands_add");
  check_slots(M, K, "islands_add");
  TORCH_CHECK(modes >= 0 && (modes & ~(int64_t)ana::kIslandAllModes) == 0,
              "islands_add: the modes mask must name modes 0..5");
  if (M == 0 || P == 0) return;
  if (!dev.is_cuda()) {
    TORCH_CHECK(ana::host_islands_add((int)K, rec.data_ptr<int32_t>(), rows.data_ptr<float>(), rows.size(1), M, P,
                                      (uint32_t)modes, parent.data_ptr<int32_t>(), slots.data_ptr<int32_t>(),
                                      credit.data_ptr<int32_t>()) == 0,
                "islands_add: bad arguments or a parent word outside [0, its index]");
    return;
  }
  check_hip(ana::launch_island_hook((int)K, rec.data_ptr<int32_t>(), rows.data_ptr<float>(), rows.size(1), M, P,
                                    (uint32_t)modes, parent.data_ptr<int32_t>(), slots.data_ptr<int32_t>(),
                                    credit.data_ptr<int32_t>(), ctrl.data_ptr<int64_t>(), stream_of(parent)),
            "island_hook");
}

// the same unions for the edges (a[i], b[i]); mark: the endpoints become seen
void islands_edges(Tensor parent, Tensor slots, Tensor ctrl, Tensor a, Tensor b, int64_t P, bool mark) {
  const auto dev = check_island_state(parent, &slots, nullptr, &ctrl, P, "islands_edges");
  check(a, "a", torch::kInt32, dev);
  check(b, "b", torch::kInt32, dev);
  TORCH_CHECK(a.dim() == 1 && b.dim() == 1 && a.numel() == b.numel(), "islands_edges: a and b must be [n]");
  const int64_t n = a.numel();
  if (n == 0) return;
  if (!dev.is_cuda()) {
    TORCH_CHECK(ana::host_islands_edges(a.data_ptr<int32_t>(), b.data_ptr<int32_t>(), n, P, mark ? 1 : 0,
                                        parent.data_ptr<int32_t>(), slots.data_ptr<int32_t>(),
                                        ctrl.data_ptr<int64_t>()) == 0,
                "islands_edges: bad arguments or a parent word outside [0, its index]");
    return;
  }
  check_hip(ana::launch_island_edges(a.data_ptr<int32_t>(), b.data_ptr<int32_t>(), n, P, mark ? 1 : 0,
                                     parent.data_ptr<int32_t>(), slots.data_ptr<int32_t>(), ctrl.data_ptr<int64_t>(),
                                     stream_of(parent)),
            "island_edges");
}

// parent[i] = the smallest id of i's island
void islands_flatten(Tensor parent, Tensor ctrl, int64_t P) {
  const auto dev = check_island_state(parent, nullptr, nullptr, &ctrl, P, "islands_flatten");
  if (P == 0) return;
  if (!dev.is_cuda()) {
    TORCH_CHECK(ana::host_islands_flatten(parent.data_ptr<int32_t>(), P) == 0,
                "islands_flatten: a parent word outside [0, its index]");
    return;
  }
  check_hip(ana::launch_island_flatten(parent.data_ptr<int32_t>(), P, ctrl.data_ptr<int64_t>(), stream_of(parent)),
            "island_flatten");
}

// census [3, P] int64 of flattened parents: players, matches, player_games at each root's index
Tensor islands_census(Tensor parent, Tensor slots, Tensor credit, Tensor ctrl, int64_t P) {
  const auto dev = check_island_state(parent, &slots, &credit, &ctrl, P, "islands_census");
  Tensor census = torch::zeros({(int64_t)ana::kIslandCensusRows, P}, parent.options().dtype(torch::kInt64));
  if (P == 0) return census;
  if (!dev.is_cuda()) {
    TORCH_CHECK(ana::host_islands_census(parent.data_ptr<int32_t>(), slots.data_ptr<int32_t>(),
                                         credit.data_ptr<int32_t>(), P, census.data_ptr<int64_t>()) == 0,
                "islands_census: a parent word outside [0, its index]");
    return census;
  }
  check_hip(ana::launch_island_census(parent.data_ptr<int32_t>(), slots.data_ptr<int32_t>(),
                                      credit.data_ptr<int32_t>(), P, census.data_ptr<int64_t>(),
                                      ctrl.data_ptr<int64_t>(), stream_of(parent)),
            "island_census");
  return census;
}

// priors [M, 4 * 2K] fp32 (field-major: shared mu, sigma, mode mu, sigma) of one window against
// the chain table [P, 16] (mu, sigma per granule), which is advanced in place to the state
// after the window (score_core.h).  The device path is six stream-ordered steps (keys, sort,
// summaries, stitch, apply, fields) without a host read.
Tensor priors_add(Tensor chain, Tensor rec, Tensor rows) {
  const auto dev = chain.device();
  const int64_t K = team_size_of(rec, "priors_add");
  const int64_t M = check_window(rec, rows, K, dev, "priors_add");
  check_slots(M, K, "priors_add");
  TORCH_CHECK(chain.dim() == 2, "priors_add: chain must be [P, 16]");
  const int64_t P = chain.size(0);
  TORCH_CHECK(P <= 0x7fffffffLL, "priors_add: P must fit in int32");
  check_rows(chain, "chain", P, ana::kBaseFloats, dev);
  Tensor priors = torch::empty({M, 8 * K}, chain.options());
  if (M == 0) return priors;
  if (!dev.is_cuda()) {
    TORCH_CHECK(ana::host_priors_add((int)K, rec.data_ptr<int32_t>(), rows.data_ptr<float>(), rows.size(1), M, P,
                                     chain.data_ptr<float>(), priors.data_ptr<float>()) == 0,
                "priors_add: bad arguments");
    return priors;
  }
  const hipStream_t s = stream_of(chain);
  const int64_t n = M * 2 * K;
  Tensor events = torch::empty({n, (int64_t)ana::kPriorEventWords}, rec.options());
  Tensor slot_priors = torch::empty({n, 4}, rec.options());  // the prior words slot-major, 16 B per slot
  const auto sorted = sort_by_player(n, P, ana::prior_edge_bytes(n), dev, s, [&](uint32_t* keys, uint32_t* vals) {
    check_hip(ana::launch_prior_keys((int)K, rec.data_ptr<int32_t>(), rows.data_ptr<float>(), rows.size(1), M, P, keys,
                                     vals, u32p(events), u32p(slot_priors), s),
              "prior_keys");
  });
  check_hip(ana::launch_prior_scan(u32p(sorted.keys), u32p(sorted.vals), u32p(events), n, (int)K, P,
                                   chain.data_ptr<float>(), sorted.edges.data_ptr<uint8_t>(), u32p(slot_priors),
                                   priors.data_ptr<float>(), s),
            "prior_scan");
  return priors;
}

// K16 (hindsight.hip; host mirror host.cpp host_hindsight_add): [out, bad] of one window -- out
// [M, 2K, 2] fp32, the smoothed (mu, sigma) of every element and NaN elsewhere; bad int64 [1], the
// slots skipped for their values -- against the carry table [P, 2] fp64, advanced in place to
// every player's oldest element (hindsight_core.h).  Windows come newest first.  The device path
// is five stream-ordered steps (keys, sort, summaries, stitch, apply) without a host read.
std::vector<Tensor> hindsight_add(Tensor carry, Tensor rec, Tensor rows, double tau, int64_t track, int64_t mode) {
  const auto dev = carry.device();
  const int64_t K = team_size_of(rec, "hindsight_add");
  const int64_t M = check_window(rec, rows, K, dev, "hindsight_add");
  check_slots(M, K, "hindsight_add");
  TORCH_CHECK(carry.dim() == 2, "hindsight_add: carry must be [P, 2]");
  const int64_t P = carry.size(0);
  TORCH_CHECK(P <= 0x7fffffffLL, "hindsight_add: P must fit in int32");
  check_rows(carry, "carry", P, 2, dev, torch::kFloat64);
  TORCH_CHECK(std::isfinite(tau) && tau >= 0.0, "hindsight_add: tau must be finite and >= 0, got ", tau);
  TORCH_CHECK(track == ana::kHsShared || track == ana::kHsMode, "hindsight_add: unknown track ", track);
  TORCH_CHECK(track != ana::kHsMode || (mode >= 0 && mode < ana::kModes), "hindsight_add: a mode track needs a mode "
              "0..5, got ", mode);
  const double tau2 = tau * tau;
  Tensor out = torch::empty({M, 2 * K, 2}, rows.options());
  if (!dev.is_cuda()) {
    Tensor bad = torch::zeros({1}, torch::TensorOptions().dtype(torch::kInt64));
    TORCH_CHECK(ana::host_hindsight_add((int)K, rec.data_ptr<int32_t>(), rows.data_ptr<float>(), rows.size(1), M, P,
                                        tau2, (int)track, (int)mode, carry.data_ptr<double>(), out.data_ptr<float>(),
                                        bad.data_ptr<int64_t>()) == 0,
                "hindsight_add: bad arguments");
    return {out, bad};
  }
  const auto i32 = torch::TensorOptions().dtype(torch::kInt32).device(dev);
  Tensor bad = torch::zeros({1}, i32);
  if (M == 0) return {out, bad.to(torch::kInt64)};
  const hipStream_t s = stream_of(carry);
  const int64_t n = M * 2 * K;
  Tensor events = torch::empty({n, 2}, i32);
  const auto sorted = sort_by_player(n, P, ana::hindsight_edge_bytes(n), dev, s, [&](uint32_t* keys, uint32_t* vals) {
    check_hip(ana::launch_hindsight_keys((int)K, rec.data_ptr<int32_t>(), rows.data_ptr<float>(), rows.size(1), M, P,
                                         (int)track, (int)mode, keys, vals, u32p(events), out.data_ptr<float>(),
                                         bad.data_ptr<int32_t>(), s),
              "hindsight_keys");
  });
  check_hip(ana::launch_hindsight_scan(u32p(sorted.keys), u32p(sorted.vals), u32p(events), n, (int)K, P, tau2,
                                       carry.data_ptr<double>(), sorted.edges.data_ptr<uint8_t>(),
                                       out.data_ptr<float>(), s),
            "hindsight_scan");
  return {out, bad.to(torch::kInt64)};
}

// K20 (ttt.hip; host mirror host.cpp host_ttt_fit; ttt_core.h): the joint re-estimate of one
// history -- rec [M, 2K+2] joined with its packed rows [M, W] and its K14 priors [M, 4, 2K] (or
// [M, 8K]) -- after at most `sweeps` sweeps and a final chain pass; tol >= 0 stops after the chain
// pass whose residual is below it (one host read per sweep then, none otherwise).  Returns [out
// [M, 2K, 2] fp32 (NaN: no element), residual fp64 [sweeps run], cav [M * 2K, 2] fp64 (the
// cavities of the last chain pass), msg [M * 2K, 2] fp64 (the messages it ran on), counters int64
// [3] (bad, flat, inconsistent)].  Dispatches on rec's device.
std::vector<Tensor> ttt_fit(Tensor rec, Tensor rows, Tensor priors, c10::optional<Tensor> attrs, Tensor vst, int64_t P,
                            double beta2, double tau, double unknown_sigma, int64_t track, int64_t mode,
                            int64_t sweeps, double tol, double damping) {
  const auto dev = rec.device();
  const int64_t K = team_size_of(rec, "ttt_fit");
  const int64_t M = check_window(rec, rows, K, dev, "ttt_fit");
  check_slots(M, K, "ttt_fit");
  TORCH_CHECK(P >= 0 && P <= 0x7fffffffLL, "ttt_fit: P must fit in int32");
  check(priors, "priors", torch::kFloat32, dev);
  TORCH_CHECK((priors.dim() == 2 && priors.size(0) == M && priors.size(1) == 8 * K) ||
                  (priors.dim() == 3 && priors.size(0) == M && priors.size(1) == 4 && priors.size(2) == 2 * K),
              "ttt_fit: priors must be [M, 4, 2K] of rec's matches");
  check_vst(vst, dev, "ttt_fit");
  const float* at = nullptr;
  if (attrs.has_value() && attrs->defined()) at = check_attrs(*attrs, P, dev, "ttt_fit");
  TORCH_CHECK(std::isfinite(tau) && tau >= 0.0, "ttt_fit: tau must be finite and >= 0, got ", tau);
  TORCH_CHECK(std::isfinite(beta2) && beta2 >= 0.0, "ttt_fit: beta2 must be finite and >= 0, got ", beta2);
  TORCH_CHECK(track == ana::kHsShared || track == ana::kHsMode, "ttt_fit: unknown track ", track);
  TORCH_CHECK(track != ana::kHsMode || (mode >= 0 && mode < ana::kModes), "ttt_fit: a mode track needs a mode 0..5, "
              "got ", mode);
  TORCH_CHECK(sweeps >= 0 && sweeps <= (1 << 20), "ttt_fit: sweeps must be 0..2^20, got ", sweeps);
  TORCH_CHECK(damping > 0.0 && damping <= 1.0, "ttt_fit: damping must lie in (0, 1], got ", damping);
  TORCH_CHECK(!(tol != tol), "ttt_fit: tol is a NaN");
  const double tau2 = tau * tau;
  const int64_t n = M * 2 * K;
  const auto f64 = torch::TensorOptions().dtype(torch::kFloat64).device(dev);
  Tensor out = torch::empty({M, 2 * K, 2}, rows.options());
  Tensor cav = torch::empty({n, 2}, f64), msg = torch::empty({n, 2}, f64);
  if (!dev.is_cuda()) {
    Tensor resid = torch::zeros({sweeps}, f64), counters = torch::zeros({(int64_t)ana::kTttCounters}, torch::kInt64);
    const int64_t run = ana::host_ttt_fit(
        (int)K, rec.data_ptr<int32_t>(), rows.data_ptr<float>(), rows.size(1), M, P, priors.data_ptr<float>(), at,
        vst.data_ptr<float>(), (float)unknown_sigma, beta2, tau2, (int)track, (int)mode, sweeps, tol, damping,
        out.data_ptr<float>(), cav.data_ptr<double>(), msg.data_ptr<double>(), resid.data_ptr<double>(),
        counters.data_ptr<int64_t>());
    TORCH_CHECK(run >= 0, "ttt_fit: bad arguments");
    return {out, resid.narrow(0, 0, run), cav, msg, counters};
  }
  TORCH_CHECK(aligned(priors, 16) && (at == nullptr || aligned(*attrs, 16)), "ttt_fit: priors and attrs must be 16-B "
              "aligned");
  const hipStream_t s = stream_of(rec);
  const auto i32 = torch::TensorOptions().dtype(torch::kInt32).device(dev);
  cav.zero_();
  msg.zero_();
  Tensor prior = torch::empty({n, 2}, f64), fwd = torch::empty({n, 2}, f64), mu64 = torch::empty({n}, f64);
  Tensor mword = torch::empty({M}, i32), counters = torch::zeros({(int64_t)ana::kTttCounters}, i32);
  Tensor bits = torch::zeros({sweeps + 1}, i32.dtype(torch::kInt64));  // bits[k]: the residual of chain pass k
  Tensor kf = torch::empty({n}, i32), vf = torch::empty({n}, i32), kb = torch::empty({n}, i32),
         vb = torch::empty({n}, i32);
  check_hip(ana::launch_ttt_setup((int)K, rec.data_ptr<int32_t>(), rows.data_ptr<float>(), rows.size(1), M, P,
                                  priors.data_ptr<float>(), at, vst.data_ptr<float>(), (float)unknown_sigma, (int)track,
                                  (int)mode, tau2, u32p(kf), u32p(vf), u32p(kb), u32p(vb), msg.data_ptr<double>(),
                                  prior.data_ptr<double>(), out.data_ptr<float>(), u32p(mword),
                                  counters.data_ptr<int32_t>(), s),
            "ttt_setup");
  std::vector<Tensor> fs = {kf, vf}, bs = {kb, vb};
  if (P > 0 && n > 0) {
    fs = sort_pairs_on_stream(kf, vf, n, bit_length(P), s);
    bs = sort_pairs_on_stream(kb, vb, n, bit_length(P), s);
  }
  Tensor edges = torch::empty({(int64_t)ana::ttt_edge_bytes(n)}, i32.dtype(torch::kUInt8));
  int64_t run = 0;
  for (int64_t k = 0;; ++k) {
    check_hip(ana::launch_ttt_chain(u32p(fs[0]), u32p(fs[1]), u32p(bs[0]), u32p(bs[1]), n, (int)K, P, tau2,
                                    msg.data_ptr<double>(), prior.data_ptr<double>(), fwd.data_ptr<double>(),
                                    cav.data_ptr<double>(), mu64.data_ptr<double>(), out.data_ptr<float>(),
                                    edges.data_ptr<uint8_t>(), k > 0 ? 1 : 0,
                                    reinterpret_cast<uint64_t*>(bits.data_ptr<int64_t>()) + k, s),
              "ttt_chain");
    if (k == sweeps) break;
    if (k > 0 && tol >= 0.0 && bits[k].view(torch::kFloat64).item<double>() < tol) break;
    check_hip(ana::launch_ttt_match((int)K, rec.data_ptr<int32_t>(), M, P, u32p(mword), cav.data_ptr<double>(),
                                    msg.data_ptr<double>(), beta2, damping, s),
              "ttt_match");
    ++run;
  }
  return {out, bits.narrow(0, 1, run).view(torch::kFloat64), cav, msg, counters.to(torch::kInt64)};
}

// adds the predictions of one window's priors to the scorecard table [6, 33, 4] int64 in
// place; returns the pred rows [M, 4] int32 (flags word, p_win0 bits, p_outcome bits, 0) when
// ``keep``, else an empty tensor
Tensor score_add(Tensor table, Tensor rec, Tensor priors, Tensor rows, c10::optional<Tensor> attrs, Tensor vst,
                 int64_t P, double beta2, double unknown_sigma, int64_t track, int64_t modes, bool keep) {
  const auto dev = table.device();
  const int64_t K = team_size_of(rec, "score_add");
  const int64_t M = check_window(rec, rows, K, dev, "score_add");
  check_slots(M, K, "score_add");
  check(table, "table", torch::kInt64, dev);
  TORCH_CHECK(table.numel() == ana::kScoreTableWords, "score_add: table must be [6, 33, 4]");
  check_rows(priors, "priors", M, 8 * K, dev);
  check_vst(vst, dev, "score_add");
  TORCH_CHECK(P >= 0 && P <= 0x7fffffffLL, "score_add: P must fit in int32");
  const float* at = nullptr;
  if (attrs.has_value() && attrs->defined()) at = check_attrs(*attrs, P, dev, "score_add");
  TORCH_CHECK(track == ana::kScoreShared || track == ana::kScoreMode, "score_add: unknown track ", track);
  TORCH_CHECK(modes >= 0 && (modes & ~(int64_t)ana::kScoreAllModes) == 0,
              "score_add: the modes mask must name modes 0..5");
  Tensor pred = torch::empty({keep ? M : 0, (int64_t)ana::kPredWords}, rec.options());
  if (M == 0) return pred;
  int32_t* pp = keep ? pred.data_ptr<int32_t>() : nullptr;
  if (!dev.is_cuda()) {
    TORCH_CHECK(ana::host_score_add((int)K, rec.data_ptr<int32_t>(), priors.data_ptr<float>(), rows.data_ptr<float>(),
                                    rows.size(1), M, at, vst.data_ptr<float>(), P, (float)beta2, (float)unknown_sigma,
                                    (int)track, (uint32_t)modes, table.data_ptr<int64_t>(), pp) == 0,
                "score_add: bad arguments");
    return pred;
  }
  check_hip(ana::launch_score((int)K, rec.data_ptr<int32_t>(), priors.data_ptr<float>(), rows.data_ptr<float>(),
                              rows.size(1), M, at, vst.data_ptr<float>(), P, (float)beta2, (float)unknown_sigma,
                              (int)track, (uint32_t)modes, table.data_ptr<int64_t>(), pp, stream_of(table)),
            "score");
  return pred;
}

// nlog2_q20 (score_core.h) of fp32 bit patterns [n] int32 -> [n] int64, computed where the
// tensor lives: the one function, compiled for the host and for the device
Tensor nlog2_q20(Tensor bits) {
  const auto dev = bits.device();
  check(bits, "bits", torch::kInt32, dev);
  const int64_t n = bits.numel();
  Tensor out = torch::empty({n}, bits.options().dtype(torch::kInt64));
  if (n == 0) return out;
  if (dev.is_cuda()) {
    check_hip(ana::launch_nlog2_q20(u32p(bits), n, out.data_ptr<int64_t>(), stream_of(bits)), "nlog2_q20");
  } else {
    const int32_t* b = bits.data_ptr<int32_t>();
    for (int64_t i = 0; i < n; ++i) out.data_ptr<int64_t>()[i] = ana::nlog2_q20((uint32_t)b[i]);
  }
  return out;
}

// K15 (pairs.hip; host mirror host.cpp): the rows of an ordered pair map as (keys [U] int64
// ascending, counts [U, 4] int32)
std::tuple<Tensor, Tensor> pair_table_of(const ana::PairMap& map) {
  const int64_t U = (int64_t)map.size();
  Tensor keys = torch::empty({U}, torch::kInt64), counts = torch::empty({U, (int64_t)ana::kPairWords}, torch::kInt32);
  int64_t* k = keys.data_ptr<int64_t>();
  int32_t* c = counts.data_ptr<int32_t>();
  for (const auto& row : map) {
    *k++ = row.first;
    for (int d = 0; d < ana::kPairWords; ++d) *c++ = row.second[d];
  }
  return {keys, counts};
}

// the device steps both pair entry points share: n entries with keys ka (a; >= dead: no entry),
// kb = bkeep (b) and values vals, stably sorted by (a, b) -- on b, then, with a gathered into that
// order, on a -- and reduced to the table of their distinct (a, b).  The sorts ping-pong between
// (kb, vals) and two scratch arrays and clobber them, hence bkeep.  src: the counters of an entry
// are the row src[value] [n, 4], undefined: they are decoded from the value's flags.  One host
// read, of the number of rows.
std::tuple<Tensor, Tensor> pair_sort_reduce(Tensor ka, Tensor kb, Tensor bkeep, Tensor vals, int64_t n, int bits,
                                            uint32_t mask, uint32_t dead, const Tensor& src, hipStream_t s) {
  const auto i32 = ka.options();
  Tensor kalt = torch::empty({n}, i32), valt = torch::empty({n}, i32);
  Tensor ws = torch::empty({(int64_t)ana::radix_sort_workspace_bytes(n)}, i32.dtype(torch::kUInt8));
  int in_alt = 0;
  check_hip(ana::launch_radix_sort_pairs(u32p(kb), u32p(vals), u32p(kalt), u32p(valt), n, bits, ws.data_ptr<uint8_t>(),
                                         &in_alt, s),
            "pairs: radix sort on b");
  Tensor k1 = in_alt ? kalt : kb, v1 = in_alt ? valt : vals, k2 = in_alt ? kb : kalt, v2 = in_alt ? vals : valt;
  // the sorted b keys are no longer needed: a goes where they are
  check_hip(ana::launch_pair_gather(u32p(ka), u32p(v1), mask, n, u32p(k1), s), "pair_gather (a)");
  check_hip(ana::launch_radix_sort_pairs(u32p(k1), u32p(v1), u32p(k2), u32p(v2), n, bits, ws.data_ptr<uint8_t>(),
                                         &in_alt, s),
            "pairs: radix sort on a");
  Tensor a = in_alt ? k2 : k1, v = in_alt ? v2 : v1, b = in_alt ? k1 : k2;
  check_hip(ana::launch_pair_gather(u32p(bkeep), u32p(v), mask, n, u32p(b), s), "pair_gather (b)");
  const int64_t tiles = ana::pair_tiles(n);
  Tensor tcounts = torch::empty({tiles}, i32), offsets = torch::empty({tiles + 1}, i32.dtype(torch::kInt64));
  check_hip(ana::launch_pair_count(u32p(a), u32p(b), n, dead, u32p(tcounts), offsets.data_ptr<int64_t>(), s),
            "pair_count");
  const int64_t U = offsets[tiles].item<int64_t>();  // the one synchronisation of a call
  TORCH_CHECK(U >= 0 && U <= n, "pairs: impossible row count ", U);
  Tensor keys = torch::empty({U}, i32.dtype(torch::kInt64));
  Tensor counts = torch::zeros({U, (int64_t)ana::kPairWords}, i32);  // runs cut by an edge are added atomically
  check_hip(ana::launch_pair_emit(u32p(a), u32p(b), u32p(v), n, dead, src.defined() ? src.data_ptr<int32_t>() : nullptr,
                                  offsets.data_ptr<int64_t>(), U, keys.data_ptr<int64_t>(), counts.data_ptr<int32_t>(),
                                  s),
            "pair_emit");
  return {keys, counts};
}

// the pair table (pair_core.h) of one window -- rec [M, 2K+2] joined with its packed output rows
// [M, W] -- among P players on the modes of the mask, of the players of ``bitmap`` (int32
// [ceil(P / 32)]; none: of everybody): (keys [U] int64 = a << 32 | b ascending, counts [U, 4] int32
// = with_games, with_wins, vs_games, vs_wins from a's side).  Dispatches on the tensors' device.
std::tuple<Tensor, Tensor> pairs_window(Tensor rec, Tensor rows, int64_t P, int64_t modes,
                                        const c10::optional<Tensor>& bitmap) {
  const auto dev = rec.device();
  const int64_t K = team_size_of(rec, "pairs_window");
  const int64_t M = check_window(rec, rows, K, dev, "pairs_window");
  TORCH_CHECK(P >= 0 && P <= 0x7fffffffLL, "pairs_window: P must fit in int32");
  TORCH_CHECK(modes >= 0 && (modes & ~(int64_t)ana::kPairAllModes) == 0,
              "pairs_window: the modes mask must name modes 0..5");
  const int64_t E = ana::pair_entries((int)K);
  TORCH_CHECK(M <= ana::kMaxSlots / E, "pairs_window: a window holds at most ", ana::kMaxSlots, " entries (", E,
              " per match)");
  const uint32_t* bm = nullptr;
  if (bitmap.has_value() && bitmap->defined()) {
    check(*bitmap, "bitmap", torch::kInt32, dev);
    TORCH_CHECK(bitmap->dim() == 1 && bitmap->numel() >= (P + 31) / 32, "pairs_window: bitmap needs ceil(P / 32) words");
    bm = u32p(*bitmap);
  }
  const auto i32 = torch::TensorOptions().dtype(torch::kInt32).device(dev);
  if (!dev.is_cuda()) {
    ana::PairMap map;
    TORCH_CHECK(ana::host_pairs_add((int)K, rec.data_ptr<int32_t>(), rows.data_ptr<float>(), rows.size(1), M, P,
                                    (uint32_t)modes, bm, map) == 0,
                "pairs_window: bad arguments");
    return pair_table_of(map);
  }
  const int64_t n = M * E;
  if (n == 0 || P < 2)  // two different players make an entry
    return {torch::empty({0}, i32.dtype(torch::kInt64)), torch::empty({0, (int64_t)ana::kPairWords}, i32)};
  const hipStream_t s = stream_of(rec);
  Tensor ka = torch::empty({n}, i32), kb = torch::empty({n}, i32), bkeep = torch::empty({n}, i32),
         vals = torch::empty({n}, i32);
  // under a filter nearly every entry is dead: only the live ones are written, packed, and sorted
  Tensor live = bm != nullptr ? torch::zeros({1}, i32) : Tensor();
  check_hip(ana::launch_pair_keys((int)K, rec.data_ptr<int32_t>(), rows.data_ptr<float>(), rows.size(1), M, P,
                                  (uint32_t)modes, bm, u32p(ka), u32p(kb), u32p(bkeep), u32p(vals),
                                  live.defined() ? u32p(live) : nullptr, s),
            "pair_keys");
  int64_t nl = n;
  if (live.defined()) {
    nl = live.item<int32_t>();  // a second synchronisation, which saves the sorts of the dead entries
    TORCH_CHECK(nl >= 0 && nl <= n, "pairs_window: impossible entry count ", nl);
    if (nl == 0) return {torch::empty({0}, i32.dtype(torch::kInt64)), torch::empty({0, (int64_t)ana::kPairWords}, i32)};
  }
  // bit_length(P): the key P of a dead entry sorts last
  return pair_sort_reduce(ka.narrow(0, 0, nl), kb.narrow(0, 0, nl), bkeep.narrow(0, 0, nl), vals.narrow(0, 0, nl), nl,
                          bit_length(P), ana::kPairIndexMask, (uint32_t)P, Tensor(), s);
}

// the compaction: the tables (keys [n_i] int64, counts [n_i, 4] int32) of one device added into
// one table.  The rows are concatenated, sorted by key with their indices as values (up to
// 2^31 - 1 rows) and reduced with the counters gathered at those indices.  P: every id of the
// keys is below it (it bounds the sort's key bits; 2^31 - 1 is always right).
std::tuple<Tensor, Tensor> pairs_merge(std::vector<Tensor> keys_list, std::vector<Tensor> counts_list, int64_t P) {
  TORCH_CHECK(!keys_list.empty() && keys_list.size() == counts_list.size(),
              "pairs_merge: as many key tensors as count tensors, at least one");
  TORCH_CHECK(P >= 1 && P <= 0x7fffffffLL, "pairs_merge: P must lie in [1, 2^31)");
  const auto dev = keys_list[0].device();
  int64_t n = 0;
  for (size_t i = 0; i < keys_list.size(); ++i) {
    check(keys_list[i], "keys", torch::kInt64, dev);
    check(counts_list[i], "counts", torch::kInt32, dev);
    TORCH_CHECK(keys_list[i].dim() == 1 && counts_list[i].dim() == 2 &&
                    counts_list[i].size(0) == keys_list[i].size(0) && counts_list[i].size(1) == ana::kPairWords,
                "pairs_merge: keys must be [n] and counts [n, 4]");
    n += keys_list[i].size(0);
  }
  TORCH_CHECK(n <= 0x7fffffffLL, "pairs_merge: at most 2^31 - 1 rows");
  Tensor keys = torch::cat(keys_list), counts = torch::cat(counts_list);
  if (!dev.is_cuda()) {
    ana::PairMap map;
    ana::host_pairs_merge(keys.data_ptr<int64_t>(), counts.data_ptr<int32_t>(), n, map);
    return pair_table_of(map);
  }
  if (n == 0) return {keys, counts};
  const hipStream_t s = stream_of(keys);
  const auto i32 = counts.options();
  Tensor ka = torch::empty({n}, i32), kb = torch::empty({n}, i32), bkeep = torch::empty({n}, i32),
         vals = torch::empty({n}, i32);
  check_hip(ana::launch_pair_split(keys.data_ptr<int64_t>(), n, u32p(ka), u32p(kb), u32p(bkeep), u32p(vals), s),
            "pair_split");
  // every a is below 2^31: nothing is dead
  return pair_sort_reduce(ka, kb, bkeep, vals, n, bit_length(P), 0xffffffffu, 0x80000000u, counts, s);
}

// K11 (ladder.hip; host mirror host.cpp host_ladder): the ladders of the tracks of ``mask``
// (bit t = granule t) of a roster's state [P, 32], as [order, score, rank] per track in
// ascending track order: order int32 [R] (best first), score fp32 [R], rank int32 [P]
// (-1 = unranked).  Dispatches on the tensor's device; the device path reads the roster
// once for all tracks and synchronises once, for the ranked counts that size the outputs.
std::vector<Tensor> ladder(Tensor state, int64_t mask, int64_t score, double max_sigma) {
  const auto dev = state.device();
  const int64_t P = check_state(state, dev, "ladder");
  TORCH_CHECK(mask > 0 && (mask & ~(int64_t)ana::kLadderTrackMask) == 0,
              "ladder: the track mask must name some of tracks 0..6");
  TORCH_CHECK(score == ana::kLadderConservative || score == ana::kLadderMu, "ladder: unknown score ", score);
  TORCH_CHECK(P <= 0x7fffffffLL, "ladder: P must be below 2^31");
  const float bound = (float)max_sigma;
  const auto i32 = torch::TensorOptions().dtype(torch::kInt32).device(dev);
  const auto f32 = i32.dtype(torch::kFloat32);
  std::vector<int> tracks;
  for (int t = 0; t < ana::kTracks; ++t)
    if ((mask >> t) & 1) tracks.push_back(t);
  const int64_t T = (int64_t)tracks.size();
  std::vector<Tensor> out;
  if (P == 0) {
    for (int64_t j = 0; j < T; ++j) {
      out.push_back(torch::empty({0}, i32));
      out.push_back(torch::empty({0}, f32));
      out.push_back(torch::empty({0}, i32));
    }
    return out;
  }
  if (!dev.is_cuda()) {
    for (int64_t j = 0; j < T; ++j) {
      Tensor order = torch::empty({P}, i32), sc = torch::empty({P}, f32), rank = torch::empty({P}, i32);
      const int64_t R = ana::host_ladder(state.data_ptr<float>(), P, tracks[j], (int)score, bound,
                                         order.data_ptr<int32_t>(), sc.data_ptr<float>(), rank.data_ptr<int32_t>());
      TORCH_CHECK(R >= 0 && R <= P, "ladder: bad arguments");
      out.push_back(R == P ? order : order.narrow(0, 0, R).clone());
      out.push_back(R == P ? sc : sc.narrow(0, 0, R).clone());
      out.push_back(rank);
    }
    return out;
  }
  TORCH_CHECK(aligned(state, 16), "ladder: state must be 16-B aligned");
  const hipStream_t s = stream_of(state);
  const int64_t stride = (P + 31) / 32 * 32;  // every track's keys start on a 128-B line
  Tensor keys = torch::empty({T, stride}, i32), ids = torch::empty({T, stride}, i32);
  Tensor counts = torch::empty({(int64_t)ana::kTracks}, i32);
  check_hip(ana::launch_ladder_keys(state.data_ptr<float>(), P, (uint32_t)mask, (int)score, bound, u32p(keys),
                                    u32p(ids), stride, u32p(counts), s),
            "ladder_keys");
  const Tensor host_counts = counts.cpu();  // the one synchronisation of a build
  for (int64_t j = 0; j < T; ++j) {
    const int64_t R = host_counts.data_ptr<int32_t>()[j];
    TORCH_CHECK(R >= 0 && R <= P, "ladder: impossible ranked count ", R);
    const auto sorted = sort_pairs_on_stream(keys[j].narrow(0, 0, P), ids[j].narrow(0, 0, P), P, 32, s);
    Tensor order = torch::empty({R}, i32), sc = torch::empty({R}, f32), rank = torch::empty({P}, i32);
    check_hip(ana::launch_ladder_ranks(u32p(sorted[0]), u32p(sorted[1]), P, R, order.data_ptr<int32_t>(),
                                       sc.data_ptr<float>(), rank.data_ptr<int32_t>(), s),
              "ladder_ranks");
    out.push_back(order);
    out.push_back(sc);
    out.push_back(rank);
  }
  return out;
}

// K12 (matchmake.hip; host mirror host.cpp): the roster operands every matchmaking call takes.
// attrs may be absent ("no attributes"); returns its pointer or null.
const float* matchmake_roster(const Tensor& state, const c10::optional<Tensor>& attrs, const Tensor& vst,
                              const torch::Device& dev, const char* what) {
  const int64_t P = check_state(state, dev, what);
  check_vst(vst, dev, what);
  TORCH_CHECK(P <= 0x7fffffffLL, what, ": P must be below 2^31");
  TORCH_CHECK(aligned(state, 16), what, ": state must be 16-B aligned");
  if (!attrs.has_value() || !attrs->defined()) return nullptr;
  const float* at = check_attrs(*attrs, P, dev, what);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(at) % 16 == 0, what, ": attrs must be 16-B aligned");
  return at;
}

// packed rows [M, 4] int32: status, quality bits, p_win0 bits, 0 (ops/matchmake.py views them)
Tensor preview(Tensor rec, int64_t K, Tensor state, c10::optional<Tensor> attrs, Tensor vst, double beta2,
               double unknown_sigma) {
  const auto dev = rec.device();
  const int64_t M = check_rec(rec, K, dev, "preview");
  const float* at = matchmake_roster(state, attrs, vst, dev, "preview");
  const int64_t P = state.size(0);
  Tensor out = torch::empty({M, (int64_t)ana::kPreviewWords}, rec.options());
  if (M == 0) return out;
  if (dev.is_cuda()) {
    check_hip(ana::launch_preview((int)K, rec.data_ptr<int32_t>(), M, state.data_ptr<float>(), at,
                                  vst.data_ptr<float>(), P, (float)beta2, (float)unknown_sigma,
                                  out.data_ptr<int32_t>(), stream_of(rec)),
              "preview");
  } else {
    TORCH_CHECK(ana::host_preview((int)K, rec.data_ptr<int32_t>(), M, state.data_ptr<float>(), at,
                                  vst.data_ptr<float>(), P, (float)beta2, (float)unknown_sigma,
                                  out.data_ptr<int32_t>()) == 0, "preview: bad arguments");
  }
  return out;
}

// [packed rows [L, 8] int32 (status, split, team0, quality, p_win0, quality_given bits, 0, 0),
//  records [L, 2K+2] int32]
std::vector<Tensor> balance(Tensor lobbies, int64_t K, Tensor state, c10::optional<Tensor> attrs, Tensor vst,
                            int64_t mode, double beta2, double unknown_sigma) {
  const auto dev = lobbies.device();
  check(lobbies, "lobbies", torch::kInt32, dev);
  TORCH_CHECK(K >= 1 && K <= ana::kMaxTeamSize, "balance: K must be 1..5");
  TORCH_CHECK(lobbies.dim() == 2 && lobbies.size(1) == 2 * K, "balance: lobbies must be [L, 2K]");
  TORCH_CHECK(mode >= 0 && mode < ana::kModes, "balance: mode must be 0..5");
  const float* at = matchmake_roster(state, attrs, vst, dev, "balance");
  const int64_t L = lobbies.size(0), P = state.size(0);
  Tensor out = torch::empty({L, (int64_t)ana::kBalanceWords}, lobbies.options());
  Tensor records = torch::empty({L, 2 * K + 2}, lobbies.options());
  if (L == 0) return {out, records};
  if (dev.is_cuda()) {
    check_hip(ana::launch_balance((int)K, lobbies.data_ptr<int32_t>(), L, state.data_ptr<float>(), at,
                                  vst.data_ptr<float>(), P, (int)mode, (float)beta2, (float)unknown_sigma,
                                  out.data_ptr<int32_t>(), records.data_ptr<int32_t>(), stream_of(lobbies)),
              "balance");
  } else {
    TORCH_CHECK(ana::host_balance((int)K, lobbies.data_ptr<int32_t>(), L, state.data_ptr<float>(), at,
                                  vst.data_ptr<float>(), P, (int)mode, (float)beta2, (float)unknown_sigma,
                                  out.data_ptr<int32_t>(), records.data_ptr<int32_t>()) == 0,
                "balance: bad arguments");
  }
  return {out, records};
}

// [keys, positions] int32 [Q]: the queue's sort keys in ascending order (descending prior mu,
// kLadderUnranked = -1 last) and the queue positions in that order; stable
std::vector<Tensor> queue_order(Tensor queue, Tensor state, c10::optional<Tensor> attrs, Tensor vst, int64_t mode,
                                double unknown_sigma) {
  const auto dev = queue.device();
  check(queue, "queue", torch::kInt32, dev);
  TORCH_CHECK(queue.dim() == 1 && queue.size(0) <= 0x7fffffffLL, "queue_order: queue must be [Q], Q < 2^31");
  TORCH_CHECK(mode >= 0 && mode < ana::kModes, "queue_order: mode must be 0..5");
  const float* at = matchmake_roster(state, attrs, vst, dev, "queue_order");
  const int64_t Q = queue.size(0), P = state.size(0);
  Tensor keys = torch::empty({Q}, queue.options()), vals = torch::empty({Q}, queue.options());
  if (Q == 0) return {keys, vals};
  if (!dev.is_cuda()) {
    TORCH_CHECK(ana::host_queue_keys(queue.data_ptr<int32_t>(), Q, state.data_ptr<float>(), at,
                                     vst.data_ptr<float>(), P, (int)mode, (float)unknown_sigma, u32p(keys),
                                     u32p(vals)) == 0, "queue_order: bad arguments");
    Tensor sk = torch::empty({Q}, queue.options()), sv = torch::empty({Q}, queue.options());
    const uint32_t* k = u32p(keys);
    uint32_t* order = u32p(sv);
    std::iota(order, order + Q, 0u);
    std::stable_sort(order, order + Q, [&](uint32_t a, uint32_t b) { return k[a] < k[b]; });
    for (int64_t i = 0; i < Q; ++i) u32p(sk)[i] = k[order[i]];
    return {sk, sv};
  }
  const hipStream_t s = stream_of(queue);
  check_hip(ana::launch_queue_keys(queue.data_ptr<int32_t>(), Q, state.data_ptr<float>(), at, vst.data_ptr<float>(),
                                   P, (int)mode, (float)unknown_sigma, u32p(keys), u32p(vals), s),
            "queue_keys");
  return sort_pairs_on_stream(keys, vals, Q, 32, s);
}

// (lanes of a lane group, lobbies per wave, lobbies per workgroup) of preview / balance at team size K
std::tuple<int64_t, int64_t, int64_t> matchmake_geometry(int64_t K) {
  TORCH_CHECK(K >= 1 && K <= ana::kMaxTeamSize, "matchmake_geometry: K must be 1..5");
  const int G = ana::split_group_lanes((int)K);
  return {G, 64 / G, ana::kMatchmakeThreads / G};
}

std::vector<int64_t> split_masks(int64_t K) {
  TORCH_CHECK(K >= 1 && K <= ana::kMaxTeamSize, "split_masks: K must be 1..5");
  std::vector<int64_t> out;
  ana::with_team_size((int)K, [&](auto k) {
    for (uint16_t m : ana::kSplits<decltype(k)::value>.mask) out.push_back(m);
  });
  return out;
}

void reset_tags(Tensor state) {
  const auto dev = state.device();
  const int64_t P = check_state(state, dev, "reset_tags");
  if (dev.is_cuda()) check_hip(ana::launch_reset_tags(state.data_ptr<float>(), P, stream_of(state)), "reset_tags");
  else ana::host_reset_tags(state.data_ptr<float>(), P);
}

}  // namespace

void register_batch_host(pybind11::module& m);      // batch_host.cpp
void register_telemetry_file(pybind11::module& m);  // telemetry_file.cpp

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  register_batch_host(m);
  register_telemetry_file(m);
  m.doc() = "analyzer_amd native engine: gfx950 HIP kernels + C++ host mirror";
  m.def("gen_roster", &gen_roster, "K7: synthetic roster (state [P,16], attrs [P,4])");
  m.def("gen_stream", &gen_stream, "K7: synthetic match stream rec [M, 2K+2]");
  m.def("schedule_workspace_bytes", &schedule_workspace_bytes);
  m.def("levels_device", &levels_device);
  m.def("sort_pairs", &sort_pairs, "stable LSD radix sort of int32 (key, value) pairs (device)");
  m.def("levels", &levels, "K5 host levelizer: per-match conflict-free round (0 = stateless)");
  m.def("schedule", &schedule, "K5: per-slot occurrence index (chronological order per player)");
  m.def("rate", &rate, "K1-K4/K6: exact dataflow rating of a stream");
  m.def("gen_event_counts", &gen_event_counts, "K8/K7: synthetic telemetry events per match");
  m.def("gen_events", &gen_events, "K8/K7: synthetic telemetry events (CSR by match)");
  m.def("telemetry", &telemetry, "K8: per-participant telemetry aggregation [M, 2K, 8]");
  m.attr("STAT_FEATURES") = ana::kStatFeatures;
  m.def("sweep_delta", &sweep_delta, "K9: per-rank natural-parameter messages for the DP merge");
  m.def("sweep_apply", &sweep_apply, "K9: decode summed messages against the common start (-> s, s2)",
        py::arg("s0"), py::arg("buf"), py::arg("attrs"), py::arg("s"), py::arg("s2"), py::arg("vst"),
        py::arg("unknown_sigma"), py::arg("scaled"), py::arg("clamps") = py::none());
  m.def("sweep_delta_packed", &sweep_delta_packed, "K9: messages straight into bf16/fp16 + int32 all-reduce operands");
  m.def("sweep_apply_packed", &sweep_apply_packed,
        "K9: decode bf16/fp16 + int32 summed messages (-> s, s2); with a prefix also the record-correction delta table",
        py::arg("s0"), py::arg("msg"), py::arg("cnt"), py::arg("attrs"), py::arg("s"), py::arg("s2"), py::arg("vst"),
        py::arg("unknown_sigma"), py::arg("clamps") = py::none(), py::arg("prefix") = py::none(),
        py::arg("delta") = py::none());
  m.def("correct_records", &correct_records,
        "K9: causal correction of a window's records: += the delta table of the earlier ranks' messages");
  m.def("sweep_block_reduce", &sweep_block_reduce, "K9: owner block sum (+ exclusive prefixes) of the split collective",
        py::arg("recv"), py::arg("N"), py::arg("bf16"), py::arg("total"), py::arg("pref") = py::none());
  m.def("prefix_delta", &prefix_delta, "K9: the record correction's delta table of a scaled message prefix");
  m.def("pack_rows", &pack_rows, "C2: changed rows of a round slice -> fixed-capacity [cap, 33] entries");
  m.def("check_round", &check_round, "C2 race detector: one round's matches share no player (flag |= 1)");
  m.def("unpack_rows", &unpack_rows, "C2: write gathered entries (id >= 0) into the roster, tags zeroed");
  m.def("write_record_file", &write_record_file, "P3: write a match-record file (ANAREC01)");
  py::class_<ana::RecordReader>(m, "RecordReader")
      .def(py::init<const std::string&, int64_t, int, bool>(), py::arg("path"), py::arg("window"),
           py::arg("slots") = 3, py::arg("pinned") = true)
      .def_property_readonly("K", &ana::RecordReader::K)
      .def_property_readonly("num_matches", &ana::RecordReader::num_matches)
      .def_property_readonly("window", &ana::RecordReader::window)
      .def_property_readonly("num_windows", &ana::RecordReader::num_windows)
      .def_property_readonly("pinned", &ana::RecordReader::pinned)
      .def("acquire", &reader_acquire,
           "next filled window as (slot, base, tensor view of pinned memory) or None at EOF")
      .def("release", &ana::RecordReader::release, "return the oldest acquired slot");
  m.def("cu_masked_stream", &cu_masked_stream, "HIP stream limited to N CUs (spread over XCDs), or to the others",
        py::arg("device"), py::arg("num_cus"), py::arg("invert") = false);
  m.def("progress_signal", &progress_signal, "8-B signal-memory word for the executor's tail signal");
  m.def("stream_wait_value64", &stream_wait_value64, "hipStreamWaitValue64(stream, ptr, >= value)");
  m.def("stream_write_value64", &stream_write_value64, "hipStreamWriteValue64(stream, ptr, value)");
  m.def("can_wait_value", &can_wait_value, "hipDeviceAttributeCanUseStreamWaitValue");
  m.def("reset_tags", &reset_tags, "zero the dataflow tags of a roster");
  m.def("records_digest", &records_digest, "deterministic fp64 digest of a window's packed output rows "
        "(+ its status counts added to hist)", py::arg("rows"), py::arg("K"), py::arg("scratch"),
        py::arg("out"), py::arg("hist") = py::none());
  m.def("records_digest_scratch", &records_digest_scratch, "scratch doubles of records_digest");
  m.def("records_select", &records_select, "K10: hits [n, 12] int32 of the bitmap's players in a window's records "
        "joined with its packed output rows, ascending (match, slot)", py::arg("rec"), py::arg("rows"),
        py::arg("base"), py::arg("P"), py::arg("bitmap"));
  m.def("tile_offsets", &tile_offsets, "offsets [T + 1] int64 = exclusive scan of counts [T] int32 read as unsigned, "
        "the total last (the scan between K10's and K15's count and emit; device only)", py::arg("counts"));
  m.def("ladder", &ladder, "K11: [order, score, rank] per track of the mask (bit t = granule t) of a roster's state: "
        "descending score, ties by ascending id, rank -1 = unranked", py::arg("state"), py::arg("mask"),
        py::arg("score"), py::arg("max_sigma"));
  m.def("preview", &preview, "K12: packed [M, 4] int32 rows (status, quality, p_win0 bits, 0) of a stream's records "
        "against the stored roster: what rate would write, read-only", py::arg("rec"), py::arg("K"), py::arg("state"),
        py::arg("attrs"), py::arg("vst"), py::arg("beta2"), py::arg("unknown_sigma"));
  m.def("balance", &balance, "K12: [packed [L, 8] int32 rows (status, split, team0, quality, p_win0, quality_given), "
        "records [L, 2K+2]] of the best split of each lobby", py::arg("lobbies"), py::arg("K"), py::arg("state"),
        py::arg("attrs"), py::arg("vst"), py::arg("mode"), py::arg("beta2"), py::arg("unknown_sigma"));
  m.def("queue_order", &queue_order, "K12: [sorted keys, queue positions] of a queue by descending mode-track prior mu "
        "(stable; failed players last with key -1)", py::arg("queue"), py::arg("state"), py::arg("attrs"),
        py::arg("vst"), py::arg("mode"), py::arg("unknown_sigma"));
  m.def("matchmake_geometry", &matchmake_geometry, "K12: (lanes per lobby, lobbies per wave, lobbies per workgroup)");
  m.def("split_masks", &split_masks, "K12: the team-0 masks of the splits of a 2K lobby, in index order");
  m.def("careers_add", &careers_add, "K13: fold one window (rec [M, 2K+2] joined with its packed rows [M, W]) into the "
        "career table [P, 16] int32 in place: careers_add(table, rec, rows, base, P, track, score, modes)");
  m.attr("CAREER_WORDS") = ana::kCareerWords;
  m.attr("CAREER_TILE") = ana::kCareerTile;
  m.def("profiles_add", &profiles_add, "K17: fold one window (rec [M, 2K+2] joined with its packed rows [M, W] and "
        "its stat vectors stats [M, 2K, 8]) into the player table [P, 20] int32 and the baseline table int64 in "
        "place: profiles_add(table, cells, rec, rows, stats, P, track, score, modes, edges)");
  m.attr("PROFILE_WORDS") = ana::kProfileWords;
  m.attr("PROFILE_TILE") = ana::kProfileTile;
  m.def("expect_add", &expect_add, "K19: fold one window (rec [M, 2K+2] joined with its raw priors [M, 4, 2K] and its "
        "pred rows [M, 4]) into the player table [P, 24] int32 and the counter bad int64 [1] in place: "
        "expect_add(table, bad, rec, priors, pred, P, track)");
  m.attr("EXPECT_WORDS") = ana::kExpectWords;
  m.attr("EXPECT_TILE") = ana::kExpectTile;
  m.def("priors_add", &priors_add, "K14: the pre-match priors [M, 4 * 2K] fp32 of one window (rec [M, 2K+2] joined with "
        "its packed rows [M, W]) against the chain table [P, 16], advanced in place: priors_add(chain, rec, rows)");
  m.def("hindsight_add", &hindsight_add, "K16: [out [M, 2K, 2] fp32, bad int64 [1]] -- the smoothed (mu, sigma) of one "
        "window (rec [M, 2K+2] joined with its packed rows [M, W]; windows newest first) against the carry table "
        "[P, 2] fp64, advanced in place: hindsight_add(carry, rec, rows, tau, track, mode)",
        py::arg("carry"), py::arg("rec"), py::arg("rows"), py::arg("tau"), py::arg("track"), py::arg("mode"));
  m.attr("HINDSIGHT_TILE") = ana::kHindsightTile;
  m.attr("HINDSIGHT_BUDGET_C") = ana::kHsBudgetC;
  m.def("ttt_fit", &ttt_fit, "K20: [out [M, 2K, 2] fp32, residual fp64 [sweeps run], cav [M * 2K, 2] fp64, msg [M * 2K, 2] "
        "fp64, counters int64 [3] (bad, flat, inconsistent)] -- one history (rec [M, 2K+2] joined with its packed rows "
        "[M, W] and its K14 priors [M, 4, 2K]) re-estimated jointly by expectation propagation: ttt_fit(rec, rows, "
        "priors, attrs, vst, P, beta2, tau, unknown_sigma, track, mode, sweeps, tol, damping); tol < 0: no early stop",
        py::arg("rec"), py::arg("rows"), py::arg("priors"), py::arg("attrs"), py::arg("vst"), py::arg("P"),
        py::arg("beta2"), py::arg("tau"), py::arg("unknown_sigma"), py::arg("track"), py::arg("mode"),
        py::arg("sweeps"), py::arg("tol"), py::arg("damping"));
  m.attr("TTT_TILE") = ana::kTttTile;
  m.def("score_add", &score_add, "K14: add the predictions of a window's priors to the scorecard table [6, 33, 4] int64 "
        "in place; returns the pred rows [M, 4] int32 when keep: score_add(table, rec, priors, rows, attrs, vst, P, "
        "beta2, unknown_sigma, track, modes, keep)",
        py::arg("table"), py::arg("rec"), py::arg("priors"), py::arg("rows"), py::arg("attrs"), py::arg("vst"),
        py::arg("P"), py::arg("beta2"), py::arg("unknown_sigma"), py::arg("track"), py::arg("modes"), py::arg("keep"));
  m.def("nlog2_q20", &nlog2_q20, "K14: -log2(p) * 2^20 of fp32 bit patterns [n] int32 -> [n] int64, integer operations only");
  m.def("pairs_window", &pairs_window, "K15: the pair table (keys [U] int64 = a << 32 | b ascending, counts [U, 4] int32 = "
        "with_games, with_wins, vs_games, vs_wins) of one window (rec [M, 2K+2] joined with its packed rows [M, W])",
        py::arg("rec"), py::arg("rows"), py::arg("P"), py::arg("modes"), py::arg("bitmap") = py::none());
  m.def("pairs_merge", &pairs_merge, "K15: several pair tables added into one (keys, counts); P: a bound above every id",
        py::arg("keys_list"), py::arg("counts_list"), py::arg("P") = (int64_t)0x7fffffffLL);
  m.attr("PAIR_TILE") = ana::kPairTile;
  m.attr("PAIR_WORDS") = ana::kPairWords;
  m.def("PAIR_ENTRIES", [](int64_t K) {
    TORCH_CHECK(K >= 1 && K <= ana::kMaxTeamSize, "PAIR_ENTRIES: K must be 1..5");
    return (int64_t)ana::pair_entries((int)K);
  }, "K15: entries of a match of team size K, 2K(2K - 1)");
  m.def("islands_add", &islands_add, "K18: unite the live slots of every rated match of one window (rec [M, 2K+2] joined "
        "with its packed rows [M, W]) in the island forest, in place: islands_add(parent, slots, credit, ctrl, rec, rows, "
        "P, modes)");
  m.def("islands_edges", &islands_edges, "K18: the same unions for the edges (a[i], b[i]); bad edges are counted in ctrl[1]: "
        "islands_edges(parent, slots, ctrl, a, b, P, mark)");
  m.def("islands_flatten", &islands_flatten, "K18: parent[i] = the smallest id of i's island: islands_flatten(parent, ctrl, P)");
  m.def("islands_census", &islands_census, "K18: [3, P] int64 (players, matches, player_games at each root) of flattened "
        "parents: islands_census(parent, slots, credit, ctrl, P)");
  m.attr("ISLAND_SEEN_BIT") = (int64_t)ana::kIslandSeenBit;
  m.attr("ISLAND_ERR_STEPS") = (int64_t)ana::kIslandErrSteps;
  m.attr("ISLAND_ERR_PARENT") = (int64_t)ana::kIslandErrParent;
  m.attr("SCORE_BINS") = ana::kScoreBins;
  m.attr("PRIOR_TILE") = ana::kPriorTile;
  m.attr("NLOG2_CAP") = (int64_t)ana::kNlog2Cap;
  m.attr("MAX_SLOTS") = (int64_t)ana::kMaxSlots;
  m.attr("LADDER_CONSERVATIVE") = (int)ana::kLadderConservative;
  m.attr("LADDER_MU") = (int)ana::kLadderMu;
  m.attr("HIT_WORDS") = ana::kHitWords;
  m.attr("SELECT_TILE") = ana::kSelectTile;
  m.def("emulate_allreduce", &emulate_allreduce,
        "DP pricing on one GPU: an all-reduce stand-in (buffer unchanged) on N CUs for >= us microseconds");
  m.def("warm_rows", &warm_rows, "read every roster row once (cache warm-up before a rating launch)");
  m.def("epoch_bump", &epoch_bump, "device launch epoch += 1 (graph replays)");
  m.attr("ROW_FLOATS") = ana::kRowFloats;
  m.attr("N_TRACKS") = ana::kTracks;
  m.attr("VST_TIERS") = ana::kVstTiers;
}
