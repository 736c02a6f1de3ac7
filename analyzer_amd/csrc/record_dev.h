// One stream record rec[m] ([2K+2] int32) into registers, shared by the kernels that walk
// a window with one lane per match (select.hip, career.hip), and the schedule's slot keys.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "common.h"

namespace ana {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v2i __attribute__((ext_vector_type(2)));

// record m into registers: 16-B loads where the record size is a multiple of 16 B, else 8-B
template <int K>
__device__ __forceinline__ void load_record(const int32_t* __restrict__ rec, int64_t m, int32_t* r) {
  constexpr int NW = 2 * K + 2;
  const int32_t* p = rec + m * NW;
  if constexpr (NW % 4 == 0) {
#pragma unroll
    for (int q = 0; q < NW / 4; ++q) {
      const v4i x = reinterpret_cast<const v4i*>(p)[q];
#pragma unroll
      for (int c = 0; c < 4; ++c) r[4 * q + c] = x[c];
    }
  } else {
#pragma unroll
    for (int q = 0; q < NW / 2; ++q) {
      const v2i x = reinterpret_cast<const v2i*>(p)[q];
      r[2 * q] = x[0];
      r[2 * q + 1] = x[1];
    }
  }
}

// The schedule's key of every slot of the record at src (K5: the radix prepass and the
// micro-batch kernel): the slot's player where the match is to be rated and the slot lies
// inside its roster, else `none` -- such a slot touches no state and gets no link.  16-B loads
// where the record size is a multiple of 16 B, else single words (not load_record's 8-B
// loads: these are the prepass's hot kernels, and their loads stay what they were tuned with).
template <int K>
__device__ __forceinline__ void sched_slot_keys(const int32_t* src, int64_t P, uint32_t none,
                                                uint32_t (&key)[2 * K]) {
  constexpr int S = 2 * K, R = S + 2;
  int32_t r[R];
  if constexpr (R % 4 == 0) {
#pragma unroll
    for (int k = 0; k < R / 4; ++k) {
      const int4 v = reinterpret_cast<const int4*>(src)[k];
      r[4 * k] = v.x; r[4 * k + 1] = v.y; r[4 * k + 2] = v.z; r[4 * k + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < R; ++k) r[k] = src[k];
  }
  const bool rates = early_status<K>(r, P) == kRated;
  const uint32_t m0 = (uint32_t)r[S];
#pragma unroll
  for (int j = 0; j < S; ++j) {
    const int pos = j < K ? j : j - K;
    const bool in_roster = pos < (j < K ? meta_n0(m0) : meta_n1(m0));
    key[j] = rates && in_roster ? (uint32_t)r[j] : none;
  }
}

}  // namespace ana
