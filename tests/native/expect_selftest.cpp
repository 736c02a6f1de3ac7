// Stand-alone self-test of the K19 host mirror (csrc/host.cpp host_expect_add), built with
// -fsanitize=address,undefined by tests/test_expectations.py: every word pattern a pred row or
// a prior can hold goes through the integer conversions, and the table and the inputs are
// allocated to their exact sizes, so an access outside them or an undefined conversion aborts.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "expect_core.h"
#include "host.h"

using namespace ana;

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
  g_state = mix64(g_state);
  return (uint32_t)(g_state >> 32);
}

// bit patterns at the edges of every conversion: NaNs, infinities, denormals, +-2^20, 0.5 and
// its neighbours, values far outside [0, 1]
static const uint32_t kEdge[] = {0x00000000u, 0x80000000u, 0x00000001u, 0x007fffffu, 0x00800000u, 0x3f000000u,
                                 0x3effffffu, 0x3f000001u, 0x3f800000u, 0x3f800001u, 0x49800000u, 0xc9800000u,
                                 0x49800001u, 0x7f7fffffu, 0xff7fffffu, 0x7f800000u, 0xff800000u, 0x7fc00000u,
                                 0xffc00000u, 0x7f800001u, 0x4f000000u, 0xcf000000u, 0x5f000000u, 0xbf800000u};

static uint32_t word() {
  const uint32_t r = rnd();
  return (r & 3u) == 0u ? kEdge[(r >> 8) % (sizeof(kEdge) / sizeof(kEdge[0]))] : rnd();
}

template <int K>
static int run(int64_t M, int64_t P, int track) {
  constexpr int S = 2 * K;
  std::vector<int32_t> rec((size_t)M * (S + 2)), pred((size_t)M * kPredWords);
  std::vector<float> priors((size_t)M * 4 * S);
  std::vector<int32_t> table((size_t)P * kExpectWords, 0);
  int64_t bad = 0;
  for (int64_t m = 0; m < M; ++m) {
    int32_t* r = rec.data() + m * (S + 2);
    for (int j = 0; j < S; ++j) {
      const uint32_t x = rnd();
      r[j] = (x & 15u) == 0u ? (int32_t)rnd() : (int32_t)(x % (uint32_t)(P + 2)) - 1;  // -1 and P among them
    }
    const uint32_t x = rnd();
    const int mode = (x & 7u) == 7u ? 255 : (int)(x & 7u);
    r[S] = (int32_t)pack_meta0(mode, (int)((x >> 8) % (K + 2)), (int)((x >> 12) % (K + 2)), 2);
    r[S + 1] = (int32_t)(rnd() & 7u);
    int32_t* p = pred.data() + m * kPredWords;
    p[0] = (int32_t)((rnd() & 3u) ? (kPredScored | rnd()) : (rnd() & ~kPredScored));
    p[1] = (int32_t)word();
    p[2] = (int32_t)word();
    p[3] = 0;
    for (int i = 0; i < 4 * S; ++i) {
      const uint32_t w = word();
      memcpy(&priors[(size_t)m * 4 * S + i], &w, 4);
    }
  }
  if (host_expect_add(K, rec.data(), priors.data(), pred.data(), M, P, track, table.data(), &bad) != 0) return 1;
  int64_t games = 0, own_known = 0;
  for (int64_t p = 0; p < P; ++p) {
    const int32_t* row = table.data() + p * kExpectWords;
    if (row[0] < 0 || row[1] > row[0] || row[2] + row[4] > row[0] || row[6] > row[0] || row[7] != 0) return 2;
    if (career_get64(row + 8) < 0 || career_get64(row + 8) > (int64_t)row[0] * kExpectOne) return 3;
    games += row[0];
    own_known += row[6];
  }
  if (bad < 0 || bad + own_known > games) return 4;
  return 0;
}

int main() {
  for (int track = 0; track < 2; ++track) {
    int rc = run<1>(3000, 7, track);
    rc = rc ? rc : run<2>(2000, 1, track);
    rc = rc ? rc : run<3>(2000, 50, track);
    rc = rc ? rc : run<4>(1000, 3, track);
    rc = rc ? rc : run<5>(1000, 11, track);
    rc = rc ? rc : run<3>(0, 5, track);
    if (rc) {
      printf("expect selftest FAILED: %d (track %d)\n", rc, track);
      return 1;
    }
  }
  int64_t bad = 0;
  int32_t row[kExpectWords] = {0};
  if (host_expect_add(6, nullptr, nullptr, nullptr, 0, 1, 0, row, &bad) == 0 ||
      host_expect_add(3, nullptr, nullptr, nullptr, 0, 1, 2, row, &bad) == 0 ||
      host_expect_add(3, nullptr, nullptr, nullptr, 0, 1, 0, row, nullptr) == 0) {
    printf("expect selftest FAILED: bad arguments were taken\n");
    return 1;
  }
  printf("expect selftest ok\n");
  return 0;
}
