/* sincos_core_cmp.c -- orbx_sincos_core (csrc/orbx_sincos.h) against the
 * form it replaced: the floor written as (double)(int64_t)v plus a fix-up
 * and the quadrant as a switch on doubles, kept here verbatim.  Compares the
 * sin and cos bits over the inputs where a floor or a quadrant step can go
 * wrong and prints "checked N differences D" (exit 1 when D > 0).
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../orb-slam-system_amd/csrc/orbx_sincos.h"

static double old_floor_d(double v) {
  /* exact floor without a library call (|v| < 2^52 here) */
  double t = (double)(int64_t)v;
  return (t > v) ? t - 1.0 : t;
}

static void old_sincos_core(float x, float* s, float* c) {
  double xd = (double)x;
  double kd = old_floor_d(xd * ORBX_INVPIO2 + 0.5);
  int k = (int)kd;
  double r = (xd - kd * ORBX_PIO2_1) - kd * ORBX_PIO2_1T;
  double sr = orbx_ksin(r), cr = orbx_kcos(r);
  double sv, cv;
  switch (k & 3) {
    case 0: sv = sr; cv = cr; break;
    case 1: sv = cr; cv = -sr; break;
    case 2: sv = -sr; cv = -cr; break;
    default: sv = -cr; cv = sr; break;
  }
  *s = (float)sv;
  *c = (float)cv;
}

static uint64_t nchecked, ndiff;

static void check(uint32_t b) {
  float x = orbx_u2f(b), s0, c0, s1, c1;
  old_sincos_core(x, &s0, &c0);
  orbx_sincos_core(x, &s1, &c1);
  ++nchecked;
  if (orbx_f2u(s0) != orbx_f2u(s1) || orbx_f2u(c0) != orbx_f2u(c1)) {
    if (ndiff < 10)
      printf("x %08x: old %08x %08x new %08x %08x\n", b, orbx_f2u(s0), orbx_f2u(c0), orbx_f2u(s1), orbx_f2u(c1));
    ++ndiff;
  }
}

int main(void) {
  const uint32_t xmax = 0x40c90fdbu; /* f32(360 * factorPI), the largest reachable angle */
  /* every float within 64 ulp of each multiple of pi/4 up to 2 pi: the floor's
   * steps (odd multiples) and the polynomials' zeros (even ones) */
  for (int m = 0; m <= 8; ++m) {
    const uint32_t b = orbx_f2u((float)(m * 0.78539816339744830962));
    for (int d = -64; d <= 64; ++d) {
      const int64_t v = (int64_t)b + d;
      if (v >= 0 && v <= (int64_t)xmax + 64) check((uint32_t)v);
    }
  }
  check(0u);
  check(xmax);
  /* denormals: both ends and a stride through them */
  for (uint32_t b = 1; b < 0x00800000u; b += 0x1001u) check(b);
  check(0x007fffffu);
  check(0x00800000u);
  /* 2^20 bit patterns, evenly strided over [0, xmax] */
  for (uint32_t i = 0; i < (1u << 20); ++i) check((uint32_t)(((uint64_t)i * xmax) >> 20));
  printf("checked %llu differences %llu\n", (unsigned long long)nchecked, (unsigned long long)ndiff);
  return ndiff ? 1 : 0;
}
