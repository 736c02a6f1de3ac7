// One stream record rec[m] ([2K+2] int32) into registers, shared by the kernels that walk
// a window with one lane per match (select.hip, career.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

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

}  // namespace ana
