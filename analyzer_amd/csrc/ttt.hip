// K20 through time: the joint re-estimate of one history -- rec [M][2K+2], its packed output rows
// [M][W] and its K14 priors [M][4][2K] -- by expectation propagation (ttt_core.h: the model, the
// messages, the scan element).  No float atomics, and no workgroup waits on another.
//
// Once per fit:
//   setup      one lane per match (ttt_setup_match): per slot i = m * 2K + j the sort key -- the
//              player of an element, else P -- with the value i, at position i for the forward
//              scan (oldest first) and at K16's mirrored position n - 1 - i for the backward one
//              (newest first); per element its initial message msg[i] = (h, pi) and its walked
//              prior prior[i] = (m_pre, s_pre^2 + q), fp64; (NaN, NaN) at out[i] of every slot
//              that is no element; the match word (element mask | active); the counters bad,
//              flat, inconsistent (integer atomicAdd, one per workgroup and counter that moved).
//   sorts      launch_radix_sort_pairs twice, stable: a player's elements oldest / newest first.
// Per chain pass, the chained scan of chain_dev.h twice (summaries, stitch, apply each); both
// scans are exclusive, run over shifted terms, and neither keeps a per-player row:
//   forward    the state in front of an element is the seed of its chain's first element's
//              prior and the elements before it; apply stores f_t = (mean, variance) at fwd[i].
//   backward   the state in front of an element is the composite of the elements after it;
//              apply has f, b and l in hand: it stores the cavity cav[i] = (mu_c, s2) fp64, the
//              marginal out[i] = (mu, sigma) fp32 and its fp64 mean mu64[i], and folds
//              |mu - mu64[i]| of the pass before into *resid: a max per lane, per wave by
//              shuffles, then one integer max per wave on the bits of the non-negative double.
// The match pass: one lane per match (ttt_match_factor) reads the cavities of its slots and
// writes msg, damped.  Every message is computed from the cavities of the chain pass before it
// (Jacobi), and the passes are stream-ordered, so no pass reads what it writes.
//
// Built with -ffp-contract=off: every fp64 operation is the one written.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "chain_dev.h"
#include "common.h"
#include "kernels.h"
#include "record_dev.h"
#include "ttt_core.h"

namespace ana {

namespace {

constexpr int kTttThreads = 256;

typedef unsigned int v2u __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));

template <int K>
__global__ void __launch_bounds__(kTttThreads) ttt_setup_kernel(
    const int32_t* __restrict__ rec, const uint32_t* __restrict__ rows, int64_t W, int64_t M, int64_t P,
    const float* __restrict__ priors, const float* __restrict__ attrs, const float* __restrict__ vst, float us,
    int32_t track, int32_t mode, double q, uint32_t* __restrict__ keys_f, uint32_t* __restrict__ vals_f,
    uint32_t* __restrict__ keys_b, uint32_t* __restrict__ vals_b, v2d* __restrict__ msg, v2d* __restrict__ prior,
    v2u* __restrict__ out, uint32_t* __restrict__ mword, int32_t* __restrict__ counters) {
  constexpr int S = 2 * K;
  __shared__ int32_t wg_cnt[kTttCounters];
  if (threadIdx.x < kTttCounters) wg_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t m = (int64_t)blockIdx.x * kTttThreads + threadIdx.x;
  int32_t cnt[kTttCounters] = {0, 0, 0};
  if (m < M) {
    const int64_t n = M * S;
    int32_t r[S + 2];
    load_record<K>(rec, m, r);
    const uint32_t* row = rows + m * W;
    const v2u tail = *reinterpret_cast<const v2u*>(row + 5 * S);
    float mu[S], sg[S], pr[4 * S];
    const v2u* a = reinterpret_cast<const v2u*>(row + (track == kHsMode ? 3 * S : 0));
#pragma unroll
    for (int c = 0; c < S; ++c) {
      const v2u x = a[c];
      if (2 * c < S) {
        mu[2 * c] = __uint_as_float(x[0]);
        mu[2 * c + 1] = __uint_as_float(x[1]);
      } else {
        sg[2 * c - S] = __uint_as_float(x[0]);
        sg[2 * c + 1 - S] = __uint_as_float(x[1]);
      }
    }
    const v4f* src = reinterpret_cast<const v4f*>(priors + m * (4 * S));
#pragma unroll
    for (int c = 0; c < S; ++c) {
      const v4f x = src[c];
#pragma unroll
      for (int d = 0; d < 4; ++d) pr[4 * c + d] = x[d];
    }
    const uint32_t word = ttt_setup_match<K>(
        r, P, tail[1] & 0xffu, pr, mu, sg, attrs, vst, us, track, mode, q, cnt,
        [&](int j, double h, double pi, double m_pre, double v_pre) {
          v2d x, y;
          x[0] = h;
          x[1] = pi;
          y[0] = m_pre;
          y[1] = v_pre;
          msg[m * S + j] = x;
          prior[m * S + j] = y;
        });
    mword[m] = word;
#pragma unroll
    for (int j = 0; j < S; ++j) {
      const int64_t i = m * S + j;
      const bool el = (word >> j) & 1u;
      const uint32_t key = el ? (uint32_t)r[j] : (uint32_t)P;
      keys_f[i] = key;
      vals_f[i] = (uint32_t)i;
      keys_b[n - 1 - i] = key;
      vals_b[n - 1 - i] = (uint32_t)i;
      if (!el) {
        v2u none;
        none[0] = none[1] = kHsNull;
        out[i] = none;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < kTttCounters; ++c)
    if (cnt[c]) atomicAdd(&wg_cnt[c], cnt[c]);
  __syncthreads();
  if (threadIdx.x < kTttCounters && wg_cnt[threadIdx.x]) atomicAdd(&counters[threadIdx.x], wg_cnt[threadIdx.x]);
}

// What both scans share: the element of a slot from its message, and no per-player row.
struct TttChain {
  typedef TttEl State;
  const v2d* __restrict__ msg;
  int64_t n;
  double q;

  static __device__ __forceinline__ TttEl identity() { return ttt_identity(); }
  static __device__ __forceinline__ TttEl seed(const double*, uint32_t) { return ttt_identity(); }
  static __device__ __forceinline__ void row_store(double*, uint32_t, const TttEl&) {}
  // the element of slot v (slot < n always: a permutation)
  __device__ __forceinline__ TttEl write(uint32_t v) const {
    if ((int64_t)v >= n) return ttt_identity();
    const v2d l = msg[v];
    return ttt_element(l[0], l[1], q);
  }
  __device__ __forceinline__ TttEl next(uint32_t prev, uint32_t) const { return write(prev); }
};

// Forward, oldest first: the state in front of an element is f_t behind the seed of its chain.
// A seed that holds the chain's seed has A == 0; the identity (A == 1) means the element is its
// chain's first.
struct TttForward : TttChain {
  const v2d* __restrict__ prior;
  v2d* __restrict__ fwd;

  static __device__ __forceinline__ TttEl combine(const TttEl& x, const TttEl& y) { return ttt_combine(x, y); }
  __device__ __forceinline__ TttEl chain_seed(uint32_t v) const {
    if ((int64_t)v >= n) return ttt_identity();
    const v2d p = prior[v];
    return ttt_seed(p[0], p[1]);
  }
  __device__ __forceinline__ TttEl first(uint32_t v, const TttEl& seed) const {
    return seed.A != 0.0 ? chain_seed(v) : seed;
  }
  __device__ __forceinline__ TttEl open(uint32_t v, uint32_t, bool oldest, const double*) const {
    return oldest ? chain_seed(v) : ttt_identity();
  }
  __device__ __forceinline__ TttEl total(uint32_t v, const TttEl& s) const { return ttt_combine(s, write(v)); }
  __device__ __forceinline__ void emit(uint32_t v, const TttEl& s) const {
    if ((int64_t)v >= n) return;
    v2d x;
    x[0] = s.b;
    x[1] = s.C;
    fwd[v] = x;
  }
};

// Backward, newest first: the state in front of an element is the composite of the later ones.
struct TttBackward : TttChain {
  const v2d* __restrict__ fwd;
  v2d* __restrict__ cav;
  double* __restrict__ mu64;
  v2u* __restrict__ out;
  bool have_before;      // mu64 holds the pass before: fold the residual
  mutable double rmax;   // the lane's largest |mu - mu of the pass before|

  static __device__ __forceinline__ TttEl combine(const TttEl& x, const TttEl& y) {
    return ttt_scan_combine_back(x, y);
  }
  __device__ __forceinline__ TttEl first(uint32_t, const TttEl& seed) const { return seed; }
  __device__ __forceinline__ TttEl open(uint32_t, uint32_t, bool, const double*) const { return ttt_identity(); }
  __device__ __forceinline__ TttEl total(uint32_t v, const TttEl& s) const {
    return ttt_scan_combine_back(s, write(v));
  }
  __device__ __forceinline__ void emit(uint32_t v, const TttEl& s) const {
    if ((int64_t)v >= n) return;
    const v2d f = fwd[v], l = msg[v];
    double hb, pib, mu_c, s2, mu, var;
    ttt_backward_of(s, q, hb, pib);
    ttt_beliefs(f[0], f[1], hb, pib, l[0], l[1], mu_c, s2, mu, var);
    v2d c;
    c[0] = mu_c;
    c[1] = s2;
    cav[v] = c;
    v2u x;
    x[0] = __float_as_uint((float)mu);
    x[1] = __float_as_uint((float)sqrt(var));
    out[v] = x;
    if (have_before) rmax = fmax(rmax, fabs(mu - mu64[v]));
    mu64[v] = mu;
  }
};

typedef ChainScan<TttForward, kTttThreads, kTttTile> TttFwdScan;
typedef ChainScan<TttBackward, kTttThreads, kTttTile> TttBwdScan;
typedef TttFwdScan::Edge TttEdge;
static_assert(sizeof(TttEdge) == 48 && offsetof(TttEdge, s) == 8, "an edge or a seed: [key, -, element]");
static_assert(sizeof(TttBwdScan::Edge) == sizeof(TttEdge), "both scans share the edge buffer");

template <bool APPLY>
__global__ void __launch_bounds__(kTttThreads) ttt_forward_kernel(
    const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, int64_t n, uint32_t P, double q,
    const v2d* __restrict__ msg, const v2d* __restrict__ prior, v2d* __restrict__ fwd, TttEdge* __restrict__ edges,
    const TttEdge* __restrict__ seeds) {
  TttForward f;
  f.msg = msg;
  f.n = n;
  f.q = q;
  f.prior = prior;
  f.fwd = fwd;
  TttFwdScan::tile<APPLY>(keys, vals, n, P, (double*)nullptr, edges, seeds, f);
}

template <bool APPLY>
__global__ void __launch_bounds__(kTttThreads) ttt_backward_kernel(
    const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, int64_t n, uint32_t P, double q,
    const v2d* __restrict__ msg, const v2d* __restrict__ fwd, v2d* __restrict__ cav, double* __restrict__ mu64,
    v2u* __restrict__ out, TttBwdScan::Edge* __restrict__ edges, const TttBwdScan::Edge* __restrict__ seeds,
    int32_t have_before, unsigned long long* __restrict__ resid) {
  TttBackward f;
  f.msg = msg;
  f.n = n;
  f.q = q;
  f.fwd = fwd;
  f.cav = cav;
  f.mu64 = mu64;
  f.out = out;
  f.have_before = have_before != 0;
  f.rmax = 0.0;
  TttBwdScan::tile<APPLY>(keys, vals, n, P, (double*)nullptr, edges, seeds, f);
  if (APPLY && have_before) {
    double r = f.rmax;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) r = fmax(r, __shfl_xor(r, o, 64));
    // r >= 0 and no NaN (fmax drops one): the order of the bits is the order of the values
    if ((threadIdx.x & 63) == 0 && r > 0.0) atomicMax(resid, (unsigned long long)__double_as_longlong(r));
  }
}

template <bool BACK>
__global__ void __launch_bounds__(kTttThreads) ttt_stitch_kernel(const TttEdge* __restrict__ edges, int64_t E,
                                                                 uint32_t P, TttEdge* __restrict__ seeds) {
  if (BACK) {
    TttBwdScan::stitch(reinterpret_cast<const TttBwdScan::Edge*>(edges), E, P, (double*)nullptr,
                       reinterpret_cast<TttBwdScan::Edge*>(seeds));
  } else {
    TttFwdScan::stitch(edges, E, P, (double*)nullptr, seeds);
  }
}

template <int K>
__global__ void __launch_bounds__(kTttThreads) ttt_match_kernel(const int32_t* __restrict__ rec, int64_t M, int64_t P,
                                                                const uint32_t* __restrict__ mword,
                                                                const v2d* __restrict__ cav, v2d* __restrict__ msg,
                                                                double beta2, double theta) {
  constexpr int S = 2 * K;
  const int64_t m = (int64_t)blockIdx.x * kTttThreads + threadIdx.x;
  if (m >= M) return;
  const uint32_t word = mword[m];
  if (!(word & kTttActive)) return;
  int32_t r[S + 2];
  load_record<K>(rec, m, r);
  ttt_match_factor<K>(
      r, P, word & ~kTttActive, beta2,
      [&](int j, double& mu_c, double& s2) {
        const v2d c = cav[m * S + j];
        mu_c = c[0];
        s2 = c[1];
      },
      [&](int j, double h, double pi) {
        v2d x;
        if (theta == 1.0) {
          x[0] = h;
          x[1] = pi;
        } else {
          const v2d old = msg[m * S + j];
          x[0] = ttt_damp(old[0], h, theta);
          x[1] = ttt_damp(old[1], pi, theta);
        }
        msg[m * S + j] = x;
      });
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

size_t ttt_edge_bytes(int64_t n) { return TttFwdScan::edge_bytes(n); }

int launch_ttt_setup(int K, const int32_t* rec, const float* rows, int64_t W, int64_t M, int64_t P,
                     const float* priors, const float* attrs, const float* vst, float unknown_sigma, int track,
                     int mode, double tau2, uint32_t* keys_f, uint32_t* vals_f, uint32_t* keys_b, uint32_t* vals_b,
                     double* msg, double* prior, float* out, uint32_t* mword, int32_t* counters, hipStream_t s) {
  if (!window_slots_ok(K, W, M, P) || (track != kHsShared && track != kHsMode) ||
      (track == kHsMode && (mode < 0 || mode >= kModes)) || !(tau2 >= 0.0) || !isfinite(tau2) || vst == nullptr ||
      counters == nullptr || !aligned16(priors) || !aligned16(msg) || !aligned16(prior) ||
      reinterpret_cast<uintptr_t>(out) % 8 != 0)
    return (int)hipErrorInvalidValue;
  if (M == 0) return 0;
  const unsigned blocks = (unsigned)((M + kTttThreads - 1) / kTttThreads);
  with_team_size(K, [&](auto k) {
    hipLaunchKernelGGL(ttt_setup_kernel<decltype(k)::value>, dim3(blocks), dim3(kTttThreads), 0, s, rec,
                       reinterpret_cast<const uint32_t*>(rows), W, M, P, priors, attrs, vst, unknown_sigma,
                       (int32_t)track, (int32_t)mode, tau2, keys_f, vals_f, keys_b, vals_b,
                       reinterpret_cast<v2d*>(msg), reinterpret_cast<v2d*>(prior), reinterpret_cast<v2u*>(out), mword,
                       counters);
  });
  return (int)hipGetLastError();
}

int launch_ttt_chain(const uint32_t* keys_f, const uint32_t* vals_f, const uint32_t* keys_b, const uint32_t* vals_b,
                     int64_t n, int K, int64_t P, double tau2, const double* msg, const double* prior, double* fwd,
                     double* cav, double* mu64, float* out, void* edges, int have_before, uint64_t* resid,
                     hipStream_t s) {
  if (!sorted_slots_ok(K, n, P) || !(tau2 >= 0.0) || !isfinite(tau2) || !aligned16(msg) || !aligned16(prior) ||
      !aligned16(fwd) || !aligned16(cav) || reinterpret_cast<uintptr_t>(mu64) % 8 != 0 ||
      reinterpret_cast<uintptr_t>(out) % 8 != 0 || reinterpret_cast<uintptr_t>(edges) % 8 != 0 ||
      reinterpret_cast<uintptr_t>(resid) % 8 != 0 || resid == nullptr)
    return (int)hipErrorInvalidValue;
  if (n == 0 || P == 0) return 0;
  const int64_t tiles = TttFwdScan::tiles(n);
  TttEdge* e = static_cast<TttEdge*>(edges);
  TttEdge* seeds = e + 2 * tiles;
  TttBwdScan::Edge* eb = static_cast<TttBwdScan::Edge*>(edges);
  TttBwdScan::Edge* seeds_b = eb + 2 * tiles;
  const v2d* l = reinterpret_cast<const v2d*>(msg);
  const v2d* pr = reinterpret_cast<const v2d*>(prior);
  v2d* f = reinterpret_cast<v2d*>(fwd);
  v2d* c = reinterpret_cast<v2d*>(cav);
  v2u* o = reinterpret_cast<v2u*>(out);
  unsigned long long* rw = reinterpret_cast<unsigned long long*>(resid);
  const dim3 grid((unsigned)tiles), one(1), wg(kTttThreads);
  hipLaunchKernelGGL(ttt_forward_kernel<false>, grid, wg, 0, s, keys_f, vals_f, n, (uint32_t)P, tau2, l, pr, f, e,
                     seeds);
  hipLaunchKernelGGL(ttt_stitch_kernel<false>, one, wg, 0, s, e, 2 * tiles, (uint32_t)P, seeds);
  hipLaunchKernelGGL(ttt_forward_kernel<true>, grid, wg, 0, s, keys_f, vals_f, n, (uint32_t)P, tau2, l, pr, f, e,
                     seeds);
  hipLaunchKernelGGL(ttt_backward_kernel<false>, grid, wg, 0, s, keys_b, vals_b, n, (uint32_t)P, tau2, l, f, c, mu64,
                     o, eb, seeds_b, (int32_t)have_before, rw);
  hipLaunchKernelGGL(ttt_stitch_kernel<true>, one, wg, 0, s, e, 2 * tiles, (uint32_t)P, seeds);
  hipLaunchKernelGGL(ttt_backward_kernel<true>, grid, wg, 0, s, keys_b, vals_b, n, (uint32_t)P, tau2, l, f, c, mu64, o,
                     eb, seeds_b, (int32_t)have_before, rw);
  return (int)hipGetLastError();
}

int launch_ttt_match(int K, const int32_t* rec, int64_t M, int64_t P, const uint32_t* mword, const double* cav,
                     double* msg, double beta2, double theta, hipStream_t s) {
  if (K < 1 || K > kMaxTeamSize || M < 0 || M * 2 * K > kMaxSlots || P < 0 || P > 0x7fffffffll ||
      !(theta > 0.0 && theta <= 1.0) || !(beta2 >= 0.0) || !isfinite(beta2) || !aligned16(cav) || !aligned16(msg))
    return (int)hipErrorInvalidValue;
  if (M == 0) return 0;
  const unsigned blocks = (unsigned)((M + kTttThreads - 1) / kTttThreads);
  with_team_size(K, [&](auto k) {
    hipLaunchKernelGGL(ttt_match_kernel<decltype(k)::value>, dim3(blocks), dim3(kTttThreads), 0, s, rec, M, P, mword,
                       reinterpret_cast<const v2d*>(cav), reinterpret_cast<v2d*>(msg), beta2, theta);
  });
  return (int)hipGetLastError();
}

}  // namespace ana
