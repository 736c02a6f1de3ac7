// Workgroup scans of the analytics kernels (K10 select, K13 careers, K14 scorecard, K15 pairs,
// K16 hindsight, K17 profiles, K19 expectations),
// device only: the segmented scan by key behind the fold / tile / stitch kernels, and the
// block sum and block offset behind the count / emit kernels.  docs/ARCHITECTURE.md ("The
// shared scans") says what they guarantee and how a new feature plugs in.  On the segmented
// scan sit fold_dev.h (K13, K17, K19: fold and stitch) and chain_dev.h (K14, K16: tile and stitch).
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include <type_traits>

namespace ana {

constexpr uint32_t kNoKey = 0xffffffffu;  // above every sort key (keys are <= P < 2^31)

// A state in 8-B pieces where its alignment allows them, else in words, so it stays in
// registers on either side of a shuffle, an LDS entry or an edge in global memory.
template <typename T>
struct StatePieces {
  static_assert(std::is_trivially_copyable<T>::value && sizeof(T) % 4 == 0, "a state is whole words");
  typedef typename std::conditional<alignof(T) % 8 == 0 && sizeof(T) % 8 == 0, uint64_t, uint32_t>::type Piece;
  typedef Piece __attribute__((may_alias)) Alias;
  static constexpr int kCount = sizeof(T) / sizeof(Piece);
  Piece p[kCount];
};

template <typename T>
__device__ __forceinline__ void state_store(T* dst, const T& a) {
  typedef StatePieces<T> Pieces;
  const Pieces x = __builtin_bit_cast(Pieces, a);
  typename Pieces::Alias* d = reinterpret_cast<typename Pieces::Alias*>(dst);
#pragma unroll
  for (int i = 0; i < Pieces::kCount; ++i) d[i] = x.p[i];
}

template <typename T>
__device__ __forceinline__ T state_load(const T* src) {
  typedef StatePieces<T> Pieces;
  const typename Pieces::Alias* s = reinterpret_cast<const typename Pieces::Alias*>(src);
  Pieces x;
#pragma unroll
  for (int i = 0; i < Pieces::kCount; ++i) x.p[i] = s[i];
  return __builtin_bit_cast(T, x);
}

template <typename T>
__device__ __forceinline__ T state_shfl_up(const T& a, int o) {
  typedef StatePieces<T> Pieces;
  Pieces x = __builtin_bit_cast(Pieces, a);
#pragma unroll
  for (int i = 0; i < Pieces::kCount; ++i) x.p[i] = __shfl_up(x.p[i], o, 64);
  return __builtin_bit_cast(T, x);
}

// Segmented inclusive scan by key over one workgroup of kThreads lanes, one element per lane
// per iteration.  Ops::combine(a, b) (a earlier) is associative with Ops::identity().
template <int kThreads, typename State, typename Ops>
struct SegScan {
  static constexpr int kWaves = kThreads / 64;
  static_assert(kThreads % 64 == 0, "whole waves");

  // double-buffered over the iterations (one barrier each): entry 0 is the carry of the
  // earlier iterations, entry 1 + w the total of wave w
  struct Lds {
    uint32_t key[2][kWaves + 1];
    State st[2][kWaves + 1];
  };

  static __device__ __forceinline__ void init(Lds& lds) {
    if (threadIdx.x == 0) lds.key[0][0] = kNoKey;
  }

  // Iteration ``it`` (0, 1, ... after init, by every lane of the workgroup) over elements in
  // ascending key order: on return ``s`` covers the lane's key from its first element this
  // workgroup saw up to the lane.  Lanes past the end pass kNoKey.
  static __device__ __forceinline__ void step(Lds& lds, int it, uint32_t key, State& s) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, b = it & 1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t ok = __shfl_up(key, o, 64);
      const State os = state_shfl_up(s, o);
      if (lane >= o && ok == key) s = Ops::combine(os, s);
    }
    if (lane == 63) {
      lds.key[b][1 + wave] = key;
      state_store(&lds.st[b][1 + wave], s);
    }
    __syncthreads();
    // keys ascend, so the entries that match are the last ones before this wave
    State before = Ops::identity();
#pragma unroll
    for (int e = 0; e < kWaves; ++e)
      if (e <= wave && lds.key[b][e] == key) before = Ops::combine(before, state_load(&lds.st[b][e]));
    s = Ops::combine(before, s);
    // The carry goes to the other buffer: written after this iteration's barrier, read after
    // the next one's.  Other waves may still be reading this buffer; it is written again only
    // behind the next barrier (the carry of iteration it + 1, the wave totals of it + 2), which
    // no wave passes before every wave has finished these reads.
    if (t == kThreads - 1) {
      lds.key[b ^ 1][0] = key;
      state_store(&lds.st[b ^ 1][0], s);
    }
  }
};

// The sum of ``n`` over the workgroup, stored to *dst by thread 0.  One barrier.
template <int kThreads>
__device__ __forceinline__ void block_sum_store(uint32_t n, uint32_t* dst) {
  constexpr int kWaves = kThreads / 64;
  const int t = threadIdx.x;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) n += __shfl_xor(n, o, 64);
  __shared__ uint32_t wsum[kWaves];
  if ((t & 63) == 0) wsum[t >> 6] = n;
  __syncthreads();
  if (t == 0) {
    uint32_t s = 0u;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s += wsum[w];
    *dst = s;
  }
}

// Iteration ``it`` of a per-iteration block offset: ``incl`` is the lane's inclusive count
// within its wave; returns the total of the earlier waves and sets ``total`` to the workgroup's.
// The per-wave sums are double-buffered over the iterations: one barrier per iteration.
template <int kThreads>
__device__ __forceinline__ int block_offset(int it, int incl, int& total) {
  constexpr int kWaves = kThreads / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ int wsum[2][kWaves];
  if (lane == 63) wsum[it & 1][wave] = incl;
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const int s = wsum[it & 1][w];
    before += w < wave ? s : 0;
    total += s;
  }
  return before;
}

}  // namespace ana
