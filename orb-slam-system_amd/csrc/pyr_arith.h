/* k_pyramid's fixed-point arithmetic as plain host C++: OpenCV's INTER_LINEAR
 * formula and the word-aligned sequence the kernel's row loop issues
 * (kernels_extract.hip), instruction by instruction.  The kernel does not
 * include this header; tests/cpp/pyr_arith_exhaustive.cpp checks the two
 * against each other over the whole operand range.
 *
 * Operands: source bytes s <= 255; column coefficients a0 + a1 == 2048 and
 * row coefficients b0 + b1 == 2048, each in [0, 2048] (the planner refuses
 * anything else, geometry.cpp build_blobs). */
#pragma once
#include <stdint.h>

namespace orbx {
namespace pyr_arith {

/* horizontal pass, reference: D = S[sx]*a0 + S[sx1]*a1 (<= 255*2048) */
inline uint32_t ref_hdot(uint32_t s0, uint32_t s1, uint32_t a0, uint32_t a1) {
  return s0 * a0 + s1 * a1;
}

/* vertical pass, reference (resize.cpp VResizeLinear<uchar>) */
inline uint32_t ref_pixel(uint32_t d0, uint32_t d1, uint32_t b0, uint32_t b1) {
  return (((b0 * (d0 >> 4)) >> 16) + ((b1 * (d1 >> 4)) >> 16) + 2) >> 2;
}

inline uint32_t word0(uint32_t v) { return v & 0xFFFFu; }
inline uint32_t word1(uint32_t v) { return v >> 16; }

/* v_perm with the source bytes placed high, then v_dot2_u32_u16 against the
 * blob's (16*a0 | 16*a1 << 16): X = (s0 << 8)*16*a0 + (s1 << 8)*16*a1 =
 * 4096*D.  Computed in 64 bits so that the caller can see that nothing wraps
 * (X <= 255*2048*4096 = 2139095040 < 2^32). */
inline uint64_t word_hdot(uint32_t s0, uint32_t s1, uint32_t a0, uint32_t a1) {
  const uint32_t pix = (s0 << 8) | (s1 << 8) << 16;    /* v_perm: bytes 1 / 3 */
  const uint32_t coef = (16u * a0) | (16u * a1) << 16; /* blob .y, both halves <= 32768 */
  return (uint64_t)word0(pix) * word0(coef) + (uint64_t)word1(pix) * word1(coef);
}

/* v_mul_u32_u24: the product of the operands' low 24 bits, low 32 bits */
inline uint32_t mul_u24(uint32_t a, uint32_t b) {
  return (uint32_t)((uint64_t)(a & 0xFFFFFFu) * (b & 0xFFFFFFu));
}

/* vertical pass of one column from the two rows' X (x0, x1) and the row
 * entry's by = b0 | b1 << 16:
 *   t0 = v_mul_u32_u24_sdwa(by WORD_0, x0 WORD_1)    b0 * (D0 >> 4)
 *   t1 = v_mul_u32_u24_sdwa(by WORD_1, x1 WORD_1)    b1 * (D1 >> 4)
 *   v  = v_add_u32_sdwa(t0 WORD_1, t1 WORD_1)        (t0 >> 16) + (t1 >> 16) */
inline uint32_t word_vsum(uint32_t x0, uint32_t x1, uint32_t by) {
  const uint32_t t0 = mul_u24(word0(by), word1(x0));
  const uint32_t t1 = mul_u24(word1(by), word1(x1));
  return word1(t0) + word1(t1);
}

/* two columns' sums packed (v_lshl_or_b32), rounded and shifted as one dword;
 * the result bytes are bytes 0 and 2 (the kernel's final v_perm picks them) */
inline uint32_t word_round_pair(uint32_t v_even, uint32_t v_odd) {
  return (((v_odd << 16) | v_even) + 0x00020002u) >> 2;
}

}  // namespace pyr_arith
}  // namespace orbx
