// predict_scale_exhaustive.cpp -- the PredictScale threshold table
// (csrc/projbuild_internal.h) against the host's logf over
// every positive finite float: the number of thresholds a ratio reaches must
// be the level of MapPoint::PredictScale's sequence (logf, divide, ceil,
// truncate, clamp), and that level must never step down as the ratio grows.
//   predict_scale_exhaustive <log_scale_factor as hex float bits> <nlevels> [stride]
// With stride > 1 only every stride-th float and the 64 floats to either side
// of each threshold are tried.  Stand-alone, at most 16 threads, no GPU.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

#include "projbuild_internal.h"

using namespace orbx;

static float from_bits(uint32_t b) {
  float f;
  memcpy(&f, &b, 4);
  return f;
}

static uint32_t to_bits(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  return b;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s <lsf bits, hex> <nlevels> [stride]\n", argv[0]);
    return 2;
  }
  const float lsf = from_bits((uint32_t)strtoul(argv[1], nullptr, 16));
  const int nlevels = atoi(argv[2]);
  const uint32_t stride = argc > 3 ? (uint32_t)std::max(1, atoi(argv[3])) : 1u;
  if (!predict_scale_args_ok(lsf, nlevels)) {
    fprintf(stderr, "rejected arguments\n");
    return 2;
  }
  float thr[ORBX_PROJ_MAX_LEVELS] = {};
  predict_scale_thresholds_host(lsf, nlevels, thr);
  for (int L = 0; L + 1 < nlevels; ++L) printf("thr[%d] = 0x%08x (%.9g)\n", L, to_bits(thr[L]), thr[L]);
  const auto count_of = [&](float r) {
    int c = 0;
    for (int L = 0; L + 1 < nlevels; ++L) c += r >= thr[L] ? 1 : 0;
    return c;
  };
  const uint32_t first = 1u, last = 0x7F7FFFFFu;  // every positive finite float
  const unsigned hw = std::thread::hardware_concurrency();
  const unsigned nt = std::max(1u, std::min(16u, hw ? hw : 1u));
  std::atomic<uint64_t> checked(0), mismatches(0), steps_down(0);
  std::vector<std::thread> pool;
  const uint64_t span = (uint64_t)last - first + 1;
  for (unsigned t = 0; t < nt; ++t)
    pool.emplace_back([&, t] {
      const uint32_t b0 = first + (uint32_t)(span * t / nt), b1 = first + (uint32_t)(span * (t + 1) / nt);
      uint64_t n = 0, bad = 0, down = 0;
      // the float before the chunk, so that a step down across chunks is seen
      int prev = b0 > first ? predict_scale_level_host(from_bits(b0 - 1), lsf, nlevels) : 0;
      for (uint64_t b = b0; b < b1; b += stride) {
        const float r = from_bits((uint32_t)b);
        const int lv = predict_scale_level_host(r, lsf, nlevels);
        bad += lv != count_of(r);
        down += lv < prev;
        prev = lv;
        ++n;
      }
      checked += n;
      mismatches += bad;
      steps_down += down;
    });
  for (auto& th : pool) th.join();
  if (stride > 1)
    for (int L = 0; L + 1 < nlevels; ++L) {
      const uint32_t c = to_bits(thr[L]);
      if (c > last) continue;
      const uint32_t lo = c > first + 64 ? c - 64 : first, hi = std::min(last, c + 64);
      int prev = predict_scale_level_host(from_bits(lo), lsf, nlevels);
      for (uint32_t b = lo; b <= hi; ++b) {
        const float r = from_bits(b);
        const int lv = predict_scale_level_host(r, lsf, nlevels);
        mismatches += lv != count_of(r);
        steps_down += lv < prev;
        prev = lv;
        ++checked;
      }
    }
  printf("checked %llu ratios: %llu mismatches, %llu non-monotone steps (%u threads, stride %u)\n",
         (unsigned long long)checked.load(), (unsigned long long)mismatches.load(),
         (unsigned long long)steps_down.load(), nt, stride);
  return mismatches.load() || steps_down.load() ? 1 : 0;
}
