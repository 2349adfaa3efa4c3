// Exhaustive host check of k_pyramid's word-aligned fixed point
// (csrc/pyr_arith.h) against OpenCV's INTER_LINEAR formula.
//   part 1: every s0, s1 in 0..255 and every a0 in 0..2048 (a1 = 2048 - a0):
//           the new dot product is 4096*D, fits 32 bits, and its high word is
//           D >> 4
//   part 2: every pair (D0 >> 4, D1 >> 4) from {0, 127, 254, ..., 32639, 32640}
//           (stride 127 = 32639 / 257, plus the upper end 255*2048 >> 4) with
//           every b0 in 0..2048 (b1 = 2048 - b0): the multiplies stay exact in
//           24 bits, the packed rounding carries nothing across its halves,
//           and the result bytes equal the reference pixel
// Prints the case counts; exit status 0 iff nothing differs.
#include <stdint.h>
#include <stdio.h>

#include "pyr_arith.h"

using namespace orbx::pyr_arith;

static int fail(const char* what, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  fprintf(stderr, "FAIL %s: %u %u %u %u\n", what, a, b, c, d);
  return 2;
}

int main() {
  unsigned long long n1 = 0, n2 = 0;
  uint64_t xmax = 0;
  for (uint32_t a0 = 0; a0 <= 2048; ++a0) {
    const uint32_t a1 = 2048 - a0;
    for (uint32_t s0 = 0; s0 <= 255; ++s0)
      for (uint32_t s1 = 0; s1 <= 255; ++s1) {
        const uint32_t D = ref_hdot(s0, s1, a0, a1);
        const uint64_t X = word_hdot(s0, s1, a0, a1);
        if (X > 0xFFFFFFFFull) return fail("dot product exceeds 32 bits", s0, s1, a0, a1);
        if (X != 4096ull * D) return fail("dot product is not 4096*D", s0, s1, a0, a1);
        if (word1((uint32_t)X) != D >> 4) return fail("high word is not D >> 4", s0, s1, a0, a1);
        if (X > xmax) xmax = X;
        ++n1;
      }
  }
  if (xmax != 255ull * 2048 * 4096) return fail("largest dot product", (uint32_t)xmax, 0, 0, 0);

  const uint32_t QMAX = 255 * 2048 >> 4;  // 32640
  static uint32_t q[260];
  int nq = 0;
  for (uint32_t v = 0; v < QMAX; v += 127) q[nq++] = v;
  q[nq++] = QMAX;
  uint32_t tmax = 0, vmax = 0;
  for (uint32_t b0 = 0; b0 <= 2048; ++b0) {
    const uint32_t b1 = 2048 - b0, by = b0 | b1 << 16;
    for (int i = 0; i < nq; ++i)
      for (int j = 0; j < nq; ++j) {
        // the rows' dot products: D >> 4 in the high word; the low word
        // ((D & 15) << 12 in the kernel) must not matter, so all of it is set
        const uint32_t x0 = q[i] << 16 | 0xFFFFu, x1 = q[j] << 16 | 0xFFFFu;
        const uint32_t d0 = q[i] << 4 | 15u, d1 = q[j] << 4 | 15u;
        const uint64_t t0 = (uint64_t)b0 * q[i], t1 = (uint64_t)b1 * q[j];
        if (b0 >> 24 || b1 >> 24 || q[i] >> 24 || q[j] >> 24 || t0 >> 32 || t1 >> 32)
          return fail("24-bit multiply not exact", b0, q[i], q[j], 0);
        if (t0 > tmax) tmax = (uint32_t)t0;
        if (t1 > tmax) tmax = (uint32_t)t1;
        // this column as the pair's even half, the mirrored column (rows
        // swapped) as its odd half
        const uint32_t ve = word_vsum(x0, x1, by), vo = word_vsum(x1, x0, by);
        if (ve + 2 >= 1024 || vo + 2 >= 1024) return fail("sum + 2 reaches 1024", b0, q[i], q[j], ve);
        if (ve > vmax) vmax = ve;
        const uint32_t p = word_round_pair(ve, vo);
        const uint32_t re = ref_pixel(d0, d1, b0, b1), ro = ref_pixel(d1, d0, b0, b1);
        if (re > 255 || ro > 255) return fail("reference exceeds a byte", b0, q[i], q[j], re);
        if ((p & 0xFFu) != re || (p >> 16 & 0xFFu) != ro) return fail("pixel", b0, q[i], q[j], p);
        ++n2;
      }
  }
  if (tmax != 2048u * QMAX) return fail("largest product", tmax, 0, 0, 0);
  printf("ok: %llu horizontal cases (max X %llu), %llu vertical cases (%d values of D >> 4, max product %u, max sum %u)\n",
         n1, (unsigned long long)xmax, n2, nq, tmax, vmax);
  return 0;
}
