// Host-side ASan/UBSan run of the batched query's host pieces
// (csrc/bowdb_internal.h): the CSR / word validation on good and bad inputs
// held in exactly-sized heap arrays (so that ASan sees a read past a query),
// the word gate on every count up to the longest query against an integer
// statement of it, and the packing of the result's offsets.  Plain host C++,
// nothing of the library.  Built by `make sanitize`.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "bowdb_internal.h"
#include "expect.h"

using namespace orbx;

enum { OK = 0, ERR_ARG = -1, ERR_UNSUPPORTED = -6 };
static const uint32_t NWORDS = 10000;

// queries as lists of words -> bowdb_check_batch over exactly-sized arrays;
// off: other offsets than the lists give (the arrays still hold the lists)
static int check(const std::vector<std::vector<uint32_t> >& qs, const std::vector<uint32_t>* off = nullptr,
                 bool null_words = false) {
  size_t total = 0;
  for (const auto& q : qs) total += q.size();
  uint32_t* o = static_cast<uint32_t*>(malloc((qs.size() + 1) * sizeof(uint32_t)));
  uint32_t* w = static_cast<uint32_t*>(malloc((total ? total : 1) * sizeof(uint32_t)));
  double* v = static_cast<double*>(malloc((total ? total : 1) * sizeof(double)));
  size_t at = 0;
  o[0] = 0;
  for (size_t i = 0; i < qs.size(); ++i) {
    for (uint32_t x : qs[i]) {
      w[at] = x;
      v[at++] = 0.5;
    }
    o[i + 1] = (uint32_t)at;
  }
  if (off) memcpy(o, off->data(), (qs.size() + 1) * sizeof(uint32_t));
  const int rc = bowdb_check_batch((int)qs.size(), o, null_words ? nullptr : w, null_words ? nullptr : v, NWORDS);
  free(o);
  free(w);
  free(v);
  return rc;
}

static std::vector<uint32_t> run(uint32_t from, uint32_t n) {
  std::vector<uint32_t> q(n);
  for (uint32_t i = 0; i < n; ++i) q[i] = from + i;
  return q;
}

int main() {
  // ------------------------------------------------------------ validation
  const std::vector<uint32_t> good = {3, 9, 500}, empty;
  EXPECT(check({good}) == OK);
  EXPECT(check({good, empty, {7}, good}) == OK);
  EXPECT(check({empty, empty}) == OK);
  EXPECT(check({{NWORDS - 1}}) == OK);
  EXPECT(check({run(0, BOWDB_MAX_WORDS)}) == OK);  // the limit itself
  EXPECT(check({run(1000, BOWDB_MAX_WORDS), good}) == OK);
  EXPECT(bowdb_check_batch(0, nullptr, nullptr, nullptr, NWORDS) == OK);  // nq == 0 reads nothing
  EXPECT(bowdb_check_batch(-1, nullptr, nullptr, nullptr, NWORDS) == ERR_ARG);
  EXPECT(bowdb_check_batch(2, nullptr, nullptr, nullptr, NWORDS) == ERR_ARG);
  EXPECT(check({empty, empty}, nullptr, true) == OK);  // no words are due
  EXPECT(check({empty, good}, nullptr, true) == ERR_ARG);
  EXPECT(check({{3, 500, 9}}) == ERR_ARG);             // descending words
  EXPECT(check({good, {3, 3, 9}}) == ERR_ARG);         // a repeat
  EXPECT(check({good, {3, 9, NWORDS}}) == ERR_ARG);    // a word past the vocabulary
  EXPECT(check({{3, 9, NWORDS}, good}) == ERR_ARG);
  EXPECT(check({good, {9}, {9, 3}}) == ERR_ARG);       // the last query's last word
  // ascending across queries is not asked for: each query on its own
  EXPECT(check({{500, 600}, {3, 9}}) == OK);
  std::vector<uint32_t> off = {1, 3, 6};
  EXPECT(check({good, good}, &off) == ERR_ARG);  // q_off[0] != 0
  off = {0, 4, 3};
  EXPECT(check({good, good}, &off) == ERR_ARG);  // descending offsets
  off = {0, 0, 6};                               // other cuts of the same words: {} and {3, 9, 500, 3, 9, 500}
  EXPECT(check({good, good}, &off) == ERR_ARG);
  off = {0, 2, 6};                               // {3, 9} and {500, 3, 9, 500}
  EXPECT(check({good, good}, &off) == ERR_ARG);
  off = {0, 3, 3};                               // {3, 9, 500} and {}: fine, the tail is never read
  EXPECT(check({good, good}, &off) == OK);
  EXPECT(check({run(0, BOWDB_MAX_WORDS + 1)}) == ERR_UNSUPPORTED);
  EXPECT(check({good, run(0, BOWDB_MAX_WORDS + 1)}) == ERR_UNSUPPORTED);
  // the first offending query decides
  EXPECT(check({{9, 3}, run(0, BOWDB_MAX_WORDS + 1)}) == ERR_ARG);
  EXPECT(check({run(0, BOWDB_MAX_WORDS + 1), {9, 3}}) == ERR_UNSUPPORTED);

  // ------------------------------------------------------------------ gate
  // (int)(m * 0.8f) against integers: floor(4m / 5), except that the float
  // product may round up to the next whole number only where 4m / 5 is whole
  // already -- so the two agree on 0 .. 8192, which the loop asserts
  for (int m = 0; m <= BOWDB_MAX_WORDS; ++m) {
    const int g = bowdb_gate(m);
    EXPECT(g == (4 * m) / 5);
    EXPECT(g >= 0 && (m == 0 || g < m));  // the largest count itself always passes
  }
  EXPECT(bowdb_gate(5) == 4 && bowdb_gate(10) == 8 && bowdb_gate(1) == 0 && bowdb_gate(8192) == 6553);
  static_assert(bowdb_gate(5) == 4, "usable in constant expressions");

  // --------------------------------------------------------------- packing
  {
    const int cnt[6] = {2, 0, 3, 0, 0, 7};
    uint32_t* out = static_cast<uint32_t*>(malloc(7 * sizeof(uint32_t)));
    EXPECT(bowdb_pack_offsets(cnt, 6, out) == 12);
    const uint32_t want[7] = {0, 2, 2, 5, 5, 5, 12};
    EXPECT(memcmp(out, want, sizeof(want)) == 0);
    EXPECT(bowdb_pack_offsets(cnt, 0, out) == 0 && out[0] == 0);
    EXPECT(bowdb_pack_offsets(cnt, 1, out) == 2 && out[1] == 2);
    free(out);
    // a total close to the 2^31 the entry point allows: no wrap on the way
    std::vector<int> big(4096, 524287);
    std::vector<uint32_t> o(big.size() + 1);
    const uint64_t total = bowdb_pack_offsets(big.data(), (int)big.size(), o.data());
    EXPECT(total == 4096ull * 524287ull && total < 0x80000000ull && o.back() == (uint32_t)total);
    for (size_t i = 0; i < big.size(); ++i) EXPECT(o[i + 1] - o[i] == 524287u);
  }

  printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
