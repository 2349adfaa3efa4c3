// Host-side ASan/UBSan run of the keyframe database's slot bookkeeping
// (csrc/bowdb_internal.h): the table drives malloc-backed word / value stores
// the way api_bowdb.hip drives the device arrays -- growth from a capacity of
// one word, appends at the tail, tombstones, compaction into fresh arrays by
// the planned runs, clear -- through add, erase, re-add and absent-id erases,
// and after every step the slot table and the stores are checked against a
// plain std::map model (id -> words, values, sequence).  ASan sees every copy
// a plan asks for.  Built by `make sanitize`.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <random>
#include <vector>

#include "bowdb_internal.h"
#include "expect.h"

using namespace orbx;

struct Model {
  std::vector<uint32_t> word;
  std::vector<double> value;
  uint64_t seq;
};

struct Store {  // exactly `cap` elements each, so that ASan catches a word past the capacity
  uint32_t* w = nullptr;
  double* v = nullptr;
  size_t cap = 0;
  void alloc(size_t c) {
    w = static_cast<uint32_t*>(malloc((c ? c : 1) * sizeof(uint32_t)));
    v = static_cast<double*>(malloc((c ? c : 1) * sizeof(double)));
    cap = c;
  }
  void release() {
    free(w);
    free(v);
    w = nullptr;
    v = nullptr;
  }
};

static int ngrow = 0, ncompact = 0;

// new arrays of `cap` words holding the runs of the old ones (api_bowdb.hip: restore)
static void restore(Store& s, size_t cap, const std::vector<BowdbMove>& moves) {
  Store n;
  n.alloc(cap);
  size_t at = 0;
  for (const BowdbMove& m : moves) {
    EXPECT(m.dst == at && m.len > 0 && m.src >= m.dst && m.src + m.len <= s.cap && m.dst + m.len <= cap);
    memcpy(n.w + m.dst, s.w + m.src, m.len * sizeof(uint32_t));
    memcpy(n.v + m.dst, s.v + m.src, m.len * sizeof(double));
    at = m.dst + m.len;
  }
  s.release();
  s = n;
}

static void add(BowdbTable& t, Store& s, std::map<uint64_t, Model>& model, uint64_t id, std::mt19937& rng) {
  const uint32_t n = rng() % 9;  // 0 .. 8 words
  Model m;
  uint32_t w = rng() % 5;
  for (uint32_t i = 0; i < n; ++i, w += 1 + rng() % 7) {
    m.word.push_back(w);
    m.value.push_back((double)(rng() % 1000) / 999.0);
  }
  EXPECT(bowdb_check_words(m.word.data(), (int)n, 1000) == 0);
  EXPECT(!t.contains(id));
  const size_t cap = t.capacity_for(n);
  EXPECT(cap >= t.used() + n && (cap == t.capacity() || cap >= 2 * t.capacity()));
  if (cap > t.capacity()) {
    std::vector<BowdbMove> whole;
    if (t.used()) whole.push_back({0, 0, t.used()});
    restore(s, cap, whole);
    t.set_capacity(cap);
    ++ngrow;
  }
  const size_t at = t.used();
  if (n) {
    memcpy(s.w + at, m.word.data(), n * sizeof(uint32_t));
    memcpy(s.v + at, m.value.data(), n * sizeof(double));
  }
  m.seq = t.next_seq();
  const int slot = t.add(id, n);
  EXPECT(slot == (int)t.slots().size() - 1 && t.slot_of(id) == slot);
  model[id] = m;
}

static void erase(BowdbTable& t, Store& s, std::map<uint64_t, Model>& model, uint64_t id) {
  const bool had = model.count(id) != 0;
  EXPECT(t.erase(id) == had);
  model.erase(id);
  if (had && t.wants_compaction()) {
    BowdbTable next = t;
    const std::vector<BowdbMove> moves = next.compact();
    restore(s, next.capacity(), moves);
    t = std::move(next);
    EXPECT(t.dead_words() == 0 && t.slots().size() == model.size());
    ++ncompact;
  }
}

// the table and the stores say what the model says
static void check(const BowdbTable& t, const Store& s, const std::map<uint64_t, Model>& model) {
  EXPECT(t.nkf() == (int)model.size());
  EXPECT(s.cap == t.capacity() && t.used() <= t.capacity());
  size_t live = 0, end = 0, nalive = 0;
  uint64_t last_seq = 0;
  for (size_t j = 0; j < t.slots().size(); ++j) {
    const BowdbSlot& sl = t.slots()[j];
    EXPECT(sl.off == end);  // slots tile [0, used) in order
    end = sl.off + sl.len;
    EXPECT(j == 0 || sl.seq > last_seq);  // add order
    last_seq = sl.seq;
    if (!sl.alive) {
      EXPECT(t.slot_of(sl.id) != (int)j);
      continue;
    }
    ++nalive;
    live += sl.len;
    auto it = model.find(sl.id);
    EXPECT(it != model.end() && t.slot_of(sl.id) == (int)j);
    if (it == model.end()) continue;
    EXPECT(it->second.seq == sl.seq && it->second.word.size() == sl.len);
    EXPECT(end <= s.cap);
    if (it->second.word.size() == sl.len && end <= s.cap && sl.len) {
      EXPECT(memcmp(s.w + sl.off, it->second.word.data(), sl.len * sizeof(uint32_t)) == 0);
      EXPECT(memcmp(s.v + sl.off, it->second.value.data(), sl.len * sizeof(double)) == 0);
    }
  }
  EXPECT(end == t.used() && live == t.live_words() && nalive == model.size());
  EXPECT(t.dead_words() == t.used() - live);
}

int main() {
  std::mt19937 rng(12345);
  BowdbTable t(1);  // reserve_words = 1
  Store s;
  s.alloc(t.capacity());
  std::map<uint64_t, Model> model;
  EXPECT(t.capacity() == 1 && BowdbTable().capacity() == BOWDB_DEFAULT_RESERVE);

  {  // argument checks of the word arrays
    const uint32_t up[3] = {1, 5, 9}, flat[3] = {1, 5, 5}, down[3] = {1, 5, 4};
    EXPECT(bowdb_check_words(up, 3, 10) == 0 && bowdb_check_words(up, 3, 9) != 0);
    EXPECT(bowdb_check_words(flat, 3, 10) != 0 && bowdb_check_words(down, 3, 10) != 0);
    EXPECT(bowdb_check_words(nullptr, 0, 0) == 0);
  }

  for (uint64_t id = 0; id < 300; ++id) {  // growth from one word
    add(t, s, model, id, rng);
    if (id % 16 == 0) check(t, s, model);
  }
  check(t, s, model);
  EXPECT(ngrow >= 8);
  erase(t, s, model, 100000);  // an absent id
  check(t, s, model);
  for (uint64_t id = 0; id < 300; ++id)  // two thirds, compacting on the way
    if (id % 3 != 1) {
      erase(t, s, model, id);
      check(t, s, model);
    }
  EXPECT(ncompact >= 1 && model.size() == 100);
  const int compact_before = ncompact;
  for (uint64_t id = 0; id < 300; id += 3) {  // re-add erased ids: they go to the back
    const uint64_t before = t.next_seq();
    add(t, s, model, id, rng);
    EXPECT(t.slots().back().id == id && t.slots().back().seq == before);
  }
  check(t, s, model);
  erase(t, s, model, 1);
  erase(t, s, model, 1);  // twice: the second is absent
  check(t, s, model);
  for (int step = 0; step < 3000; ++step) {  // a random history over 64 ids
    const uint64_t id = 1000 + rng() % 64;
    if (model.count(id) && rng() % 2) erase(t, s, model, id);
    else if (!model.count(id)) add(t, s, model, id, rng);
    if (step % 8 == 0) check(t, s, model);
  }
  check(t, s, model);
  EXPECT(ncompact > compact_before);
  while (!model.empty()) erase(t, s, model, model.begin()->first);  // down to nothing
  check(t, s, model);
  EXPECT(t.slots().empty() && t.used() == 0);
  const uint64_t seq = t.next_seq();
  add(t, s, model, 7, rng);
  add(t, s, model, 8, rng);
  t.clear();
  model.clear();
  check(t, s, model);
  EXPECT(t.next_seq() == seq + 2 && t.slots().empty());
  add(t, s, model, 7, rng);  // usable after clear
  check(t, s, model);
  s.release();

  printf("bowdb: %d grows, %d compactions, %d failures\n", ngrow, ncompact, fails);
  return fails ? 1 : 0;
}
