/* The matcher's fold hash (csrc/match_fold_hash.h) for host tests: built as a
 * shared object by tests/test_match_fold.py. */
#include "../../orb-slam-system_amd/csrc/match_fold_hash.h"

int fold_rounds(void) { return ORBM_FOLD_ROUNDS; }
int fold_hbits(int topn) { return orbm_fold_hbits(topn); }

/* slot of each of n descriptors (8 dwords each) */
void fold_slots(const uint32_t* w, int n, int round, int hbits, uint32_t* out) {
  for (int i = 0; i < n; ++i) out[i] = orbm_fold_slot(w + 8 * (long)i, round, hbits);
}
