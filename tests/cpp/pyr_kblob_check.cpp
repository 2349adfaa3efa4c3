// The planner writes k_pyramid's LUT blobs in two forms (geometry.cpp
// build_blobs): Plan::pyr_blob, which tests/cpp/pyramid_emu.cpp replays
// against the oracle, and Plan::pyr_kblob, which the kernel reads.  This
// checks that the kernel's form says the same thing, entry by entry: row
// entries and column 0's source entry are equal; a column selector applied as
// v_perm to an 8-byte window puts the same two source bytes in the high bytes
// of the u16 halves, with zero below; a column coefficient pair is 16x the
// plain one, sums to 16*2048 and fits its halves.
// usage: pyr_kblob_check W H nfeatures nlevels scale
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "geometry.h"

using namespace orbx;

static int fail(const char* m, long long a, long long b) {
  fprintf(stderr, "FAIL %s %lld %lld\n", m, a, b);
  exit(2);
}

// v_perm_b32 for selector bytes 0..7 (a byte of {hi, lo}) and 0x0C (zero)
static uint32_t v_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
  const uint64_t w = (uint64_t)hi << 32 | lo;
  uint32_t r = 0;
  for (int i = 0; i < 4; ++i) {
    const uint32_t s = sel >> (8 * i) & 0xFF;
    if (s == 0x0C) continue;
    if (s > 7) fail("selector byte", s, i);
    r |= (uint32_t)(w >> (8 * s) & 0xFF) << (8 * i);
  }
  return r;
}

int main(int argc, char** argv) {
  if (argc < 6) return 1;
  orbx_params prm = {atoi(argv[3]), (float)atof(argv[5]), atoi(argv[4]), 20, 7, 1};
  Plan P;
  const int rc = plan_geometry(prm, atoi(argv[1]), atoi(argv[2]), P);
  if (rc) { printf("rc %d\n", rc); return 3; }
  if (P.pyr_kblob.size() != P.pyr_blob.size()) fail("sizes", P.pyr_kblob.size(), P.pyr_blob.size());
  const uint32_t lo = 0x13121110u, hi = 0x17161514u;  // window byte i holds 0x10 + i
  long long nx = 0, ny = 0;
  for (const PyrSeg& g : P.segs) {
    if (g.area) continue;
    for (int t = 0; t < g.nty; ++t)
      for (int i = 2 * P.pyr_bo[g.ybo_off + t]; i < 2 * P.pyr_bo[g.ybo_off + t + 1]; ++i, ++ny)
        if (P.pyr_kblob[i] != P.pyr_blob[i]) fail("row entry", t, i);
    for (int t = 0; t < g.ntx; ++t) {
      const int e0 = P.pyr_bo[g.xbo_off + t], e1 = P.pyr_bo[g.xbo_off + t + 1];
      for (int e = e0; e < e1; ++e, ++nx) {
        const uint32_t px = P.pyr_blob[2 * e], pc = P.pyr_blob[2 * e + 1];
        const uint32_t kx = P.pyr_kblob[2 * e], kc = P.pyr_kblob[2 * e + 1];
        if (((e - e0) & 3) == 0) {  // group column 0 (blobs start on a group: level entries are multiples of 4)
          if (kx != px) fail("column 0 entry", t, e);
          // the selector k_pyramid builds from it (bytes 0 and sx1 - s0 of the
          // window, placed high) against the plain one (bytes 0 / 2)
          const uint32_t ksel = ((kx << 8) & 0xFF000000u) | 0x000C000Cu;
          const uint32_t psel = (px & 0xFFFF0000u) | 0x0C000C00u;
          if (v_perm(hi, lo, ksel) != v_perm(hi, lo, psel) << 8) fail("column 0 selector", t, e);
        } else if (px | pc) {  // (a blob's 16-B pad entry is zero in both forms)
          const uint32_t want = v_perm(hi, lo, px) << 8;  // plain form: bytes 0 / 2
          if (v_perm(hi, lo, kx) != want || (want & 0x00FF00FFu)) fail("column selector", t, e);
        } else if (kx | kc) fail("pad entry", t, e);
        if (px | pc) {
          const uint32_t a0 = pc & 0xFFFF, a1 = pc >> 16;
          if (a0 + a1 != 2048) fail("coefficient sum", a0, a1);
          if ((kc & 0xFFFF) != 16 * a0 || kc >> 16 != 16 * a1) fail("column coefficients", t, e);
        }
      }
    }
  }
  printf("ok: %lld column entries, %lld row words\n", nx, ny);
  return 0;
}
