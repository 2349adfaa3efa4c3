// match_fold_hash.h -- the hash k_match_select folds identical descriptors
// of a selected list with (kernels_match.hip; host tests include it too).
//
// A list's entries claim slots of a table of 2^hbits entries by their
// descriptor's hash; entries of one slot are compared byte by byte with the
// slot's claimant, so the hash decides only how many identical descriptors
// are found, never whether two descriptors count as identical.  An entry that
// loses its slot to a different descriptor is not folded (ORBM_FOLD_ROUNDS 1;
// `round` 1 is a second, independent hash that host tests use).
#ifndef ORBX_MATCH_FOLD_HASH_H
#define ORBX_MATCH_FOLD_HASH_H

#include <stdint.h>

#define ORBM_FOLD_ROUNDS 1
#define ORBM_FOLD_MIN_HBITS 6
#define ORBM_FOLD_MAX_HBITS 13 /* a table of 2^13 dwords: 32 KB of LDS */

#if defined(__HIPCC__)
#define ORBM_FOLD_FN __host__ __device__ static inline
#else
#define ORBM_FOLD_FN static inline
#endif

/* table size for lists of up to topn entries: at least four slots per entry */
ORBM_FOLD_FN int orbm_fold_hbits(int topn) {
  int b = ORBM_FOLD_MIN_HBITS;
  while (b < ORBM_FOLD_MAX_HBITS && (1 << b) < 4 * topn) ++b;
  return b;
}

/* slot of the descriptor w[0..7] in round `round` (0 or 1) */
ORBM_FOLD_FN uint32_t orbm_fold_slot(const uint32_t* w, int round, int hbits) {
  uint32_t h = round ? 0xC2B2AE35u : 0x85EBCA6Bu;
  for (int i = 0; i < 8; ++i) {
    h = (h ^ w[i]) * 0x9E3779B1u;
    h ^= h >> 15;
  }
  return h >> (32 - hbits);
}

#endif
