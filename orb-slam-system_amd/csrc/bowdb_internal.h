// bowdb_internal.h -- the slot bookkeeping of the keyframe database
// (api_bowdb.hip), with no HIP calls so that it runs on the host alone
// (tests/cpp/bowdb_main.cpp): id -> slot, add sequence numbers, the tombstone
// count, the compaction plan and the growth policy.  The device arrays mirror
// what is kept here: words / values hold `used` elements, slot j's vector at
// [off, off + len); the slot table is uploaded when `dirty`.
#ifndef ORBX_BOWDB_INTERNAL_H
#define ORBX_BOWDB_INTERNAL_H

#include <stddef.h>
#include <stdint.h>

#include <unordered_map>
#include <vector>

namespace orbx {

#define BOWDB_MAX_WORDS 8192          /* orbv_transform's own limit */
#define BOWDB_DEFAULT_RESERVE 65536   /* words (768 KB of device memory) */

// one stored keyframe, as the kernel reads it (32 bytes)
struct BowdbSlot {
  uint64_t id, seq;
  uint32_t off, len, alive, pad;
};

// what the kernel writes per slot (32 bytes); ncommon == 0: not sharing / dead.
// Record j belongs to slot j, and slots are in add order, so the host orders
// records by (first, j); seq travels with the record for a consumer that has
// only the records
struct BowdbRec {
  uint64_t id, seq;
  double score;
  int32_t ncommon;
  uint32_t first;  // smallest common word
};

// what the batched query kernel writes per (query, slot) (16 bytes), record
// q * nslots + j; ncommon == 0: not sharing / dead.  rank: the position in the
// query of the smallest common word, below the query's length.  The rank is
// monotone in the word, so (rank, j) orders as (first, j) does
struct BowdbBatchRec {
  double score;
  int32_t ncommon;
  uint32_t rank;
};

#define BOWDB_ORDER_TILE 256  /* slots per step of the order kernel's placement = its workgroup */

// a run of the word store that compaction moves: [src, src + len) -> dst
struct BowdbMove {
  size_t src, dst, len;
};

class BowdbTable {
 public:
  explicit BowdbTable(size_t reserve_words = 0) : cap_(reserve_words ? reserve_words : BOWDB_DEFAULT_RESERVE) {}

  const std::vector<BowdbSlot>& slots() const { return slots_; }
  size_t capacity() const { return cap_; }  // words the device arrays hold
  size_t used() const { return used_; }     // words appended since the last compaction
  size_t live_words() const { return live_; }
  size_t dead_words() const { return used_ - live_; }
  int nkf() const { return (int)by_id_.size(); }
  uint64_t next_seq() const { return seq_; }
  bool contains(uint64_t id) const { return by_id_.count(id) != 0; }
  int slot_of(uint64_t id) const {
    auto it = by_id_.find(id);
    return it == by_id_.end() ? -1 : (int)it->second;
  }

  // growth policy: the capacity that holds n more words, doubling from the
  // current one (the current one when they fit)
  size_t capacity_for(size_t n) const {
    size_t c = cap_ ? cap_ : 1;
    while (c < used_ + n) c *= 2;
    return c;
  }
  void set_capacity(size_t c) { cap_ = c; }

  // appends a keyframe of n words at the tail (the caller has made room and
  // checked !contains(id)); returns its slot
  int add(uint64_t id, uint32_t n) {
    BowdbSlot s = {id, seq_++, (uint32_t)used_, n, 1u, 0u};
    by_id_[id] = (uint32_t)slots_.size();
    slots_.push_back(s);
    used_ += n;
    live_ += n;
    return (int)slots_.size() - 1;
  }
  // tombstones id's slot; false for an absent id
  bool erase(uint64_t id) {
    auto it = by_id_.find(id);
    if (it == by_id_.end()) return false;
    BowdbSlot& s = slots_[it->second];
    s.alive = 0;
    live_ -= s.len;
    by_id_.erase(it);
    return true;
  }
  void clear() {
    slots_.clear();
    by_id_.clear();
    used_ = live_ = 0;  // sequence numbers go on: nothing refers to the old ones
  }

  // dead words outnumber live ones (or only tombstones are left)
  bool wants_compaction() const { return dead_words() > live_ || (live_ == 0 && !slots_.empty()); }

  // Drops the tombstones: live slots keep their order, ids and sequence
  // numbers and move down to a gapless store.  Returns the runs to copy from
  // the old arrays into new ones (adjacent slots merged), ascending and
  // disjoint on both sides.
  std::vector<BowdbMove> compact() {
    std::vector<BowdbMove> moves;
    std::vector<BowdbSlot> kept;
    kept.reserve(by_id_.size());
    size_t at = 0;
    for (const BowdbSlot& s : slots_) {
      if (!s.alive) continue;
      if (s.len) {
        if (!moves.empty() && moves.back().src + moves.back().len == s.off)
          moves.back().len += s.len;
        else
          moves.push_back({(size_t)s.off, at, (size_t)s.len});
      }
      BowdbSlot k = s;
      k.off = (uint32_t)at;
      at += s.len;
      by_id_[k.id] = (uint32_t)kept.size();
      kept.push_back(k);
    }
    slots_.swap(kept);
    used_ = live_ = at;
    return moves;
  }

 private:
  std::vector<BowdbSlot> slots_;
  std::unordered_map<uint64_t, uint32_t> by_id_;
  uint64_t seq_ = 0;
  size_t used_ = 0, live_ = 0, cap_;
};

// strictly ascending words below nwords: ORBX_OK (0) or ORBX_ERR_ARG (-1)
inline int bowdb_check_words(const uint32_t* word, int n, uint32_t nwords) {
  for (int i = 0; i < n; ++i)
    if (word[i] >= nwords || (i > 0 && word[i] <= word[i - 1])) return -1;
  return 0;
}

// The queries of a batched call in CSR form: query q is
// q_word / q_value[q_off[q], q_off[q + 1]), q_off[0] == 0 and never descending,
// every query's words as bowdb_check_words wants them.  ORBX_OK (0),
// ORBX_ERR_ARG (-1), or ORBX_ERR_UNSUPPORTED (-6) for a query of more than
// BOWDB_MAX_WORDS words; the first offending query decides
inline int bowdb_check_batch(int nq, const uint32_t* q_off, const uint32_t* q_word, const double* q_value,
                             uint32_t nwords) {
  if (nq < 0) return -1;
  if (nq == 0) return 0;
  if (!q_off || q_off[0] != 0) return -1;
  for (int q = 0; q < nq; ++q) {
    if (q_off[q + 1] < q_off[q]) return -1;
    const uint32_t len = q_off[q + 1] - q_off[q];
    if (len > BOWDB_MAX_WORDS) return -6;
    if (len > 0 && (!q_word || !q_value)) return -1;
    if (len > 0 && bowdb_check_words(q_word + q_off[q], (int)len, nwords)) return -1;
  }
  return 0;
}

// minCommonWords of KeyFrameDatabase.cc:207-214 from the largest count: an
// entry stays when its count is above it.  constexpr: the order kernel calls it
constexpr int bowdb_gate(int max_common) { return (int)(max_common * 0.8f); }

// the packed result's offsets from the per-query counts: out_off[0] = 0,
// out_off[q + 1] = out_off[q] + cnt[q]; returns the total
inline uint64_t bowdb_pack_offsets(const int* cnt, int nq, uint32_t* out_off) {
  uint64_t at = 0;
  out_off[0] = 0;
  for (int q = 0; q < nq; ++q) {
    at += (uint64_t)(cnt[q] > 0 ? cnt[q] : 0);
    out_off[q + 1] = (uint32_t)at;
  }
  return at;
}

}  // namespace orbx

#endif
