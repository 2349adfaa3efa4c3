// api_bowdb.hip -- C ABI of the DBoW2 score and of the keyframe database on
// the device: TemplatedVocabulary::score (TemplatedVocabulary.h:1199-1203,
// ScoringObject.cpp) and KeyFrameDatabase's add / erase / clear and the word
// walk of its two Detect*Candidates (src/KeyFrameDatabase.cc).  The store's
// bookkeeping is bowdb_internal.h; the kernel is kernels_bowdb.hip.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "../../include/orbx.h"
#include "api_common.h"
#include "bowdb_internal.h"
#include "call_arena.h"

namespace orbx {
__global__ void k_bowdb_query(const uint32_t*, const double*, int, const BowdbSlot*, int, const uint32_t*,
                              const double*, int, BowdbRec*);
__global__ void k_bowdb_query_batch(const uint32_t*, const int*, int, const uint32_t*, const double*, int,
                                    const BowdbSlot*, int, const uint32_t*, const double*, int, BowdbBatchRec*);
__global__ void k_bowdb_order(const BowdbBatchRec*, const BowdbSlot*, int, int, const uint32_t*, const int*, int, int,
                              int, int, int*, uint64_t*, int32_t*, double*, int*);
int vocab_device(const orbv_vocab* v);  // api_bow.hip
}  // namespace orbx

using namespace orbx;

struct orbv_db {
  int device = 0, scoring = 0;
  uint32_t nwords = 0;
  BowdbTable table;
  DevBuf<uint32_t> d_words;
  DevBuf<double> d_values;
  DevBuf<BowdbSlot> d_slots;
  size_t slot_cap = 0;
  bool dirty = false;  // the host's slot table is ahead of d_slots
  Stream stream;       // growth, compaction and the slot table's upload
  // the batched queries' scratch, acquired at the first batched call: one
  // record per (query, slot), grown by doubling; and the event recorded behind
  // the device form's last kernel, which reads the store and this scratch
  DevBuf<BowdbBatchRec> d_rec;
  size_t rec_cap = 0;
  Event done;
  bool inflight = false;  // `done` was recorded and not waited for on the host
  explicit orbv_db(size_t reserve) : table(reserve) {}
  ~orbv_db() {
    hipSetDevice(device);
    if (inflight) (void)hipEventSynchronize(done);
  }
};

namespace {

bool supported(int scoring) { return scoring == 0 || scoring == 1 || scoring == 2 || scoring == 5; }

// L2Scoring's closing step (ScoringObject.cpp:114-117), one scalar per pair on
// the host: glibc's sqrt is the reference's own
double close_score(int scoring, double s) {
  if (scoring != 1) return s;
  return s >= 1 ? 1.0 : 1.0 - sqrt(1.0 - s);
}

void launch_query(hipStream_t s, const uint32_t* qw, const double* qv, int nq, const BowdbSlot* slots, int nslots,
                  const uint32_t* words, const double* values, int scoring, BowdbRec* out) {
  const int blocks = std::min((nslots + 3) / 4, 2048);
  hipLaunchKernelGGL(k_bowdb_query, dim3(blocks), dim3(256), (size_t)nq * sizeof(uint32_t), s, qw, qv, nq, slots,
                     nslots, words, values, scoring, out);
}

// new word / value arrays of `cap` words holding the runs `moves` of the old
// ones; the old ones are released once the copies are done
int restore(orbv_db* db, size_t cap, const std::vector<BowdbMove>& moves) {
  DevBuf<uint32_t> w;
  DevBuf<double> v;
  if (w.alloc(cap) || v.alloc(cap)) return ORBX_ERR_HIP;
  for (const BowdbMove& m : moves) {
    ORBX_TRY(hipMemcpyAsync(w + m.dst, db->d_words + m.src, m.len * sizeof(uint32_t), hipMemcpyDeviceToDevice,
                            db->stream));
    ORBX_TRY(hipMemcpyAsync(v + m.dst, db->d_values + m.src, m.len * sizeof(double), hipMemcpyDeviceToDevice,
                            db->stream));
  }
  ORBX_TRY(hipStreamSynchronize(db->stream));
  db->d_words = std::move(w);
  db->d_values = std::move(v);
  return ORBX_OK;
}

int upload_slots(orbv_db* db) {
  const std::vector<BowdbSlot>& sl = db->table.slots();
  if (sl.size() > db->slot_cap) {
    size_t c = db->slot_cap ? db->slot_cap : 64;
    while (c < sl.size()) c *= 2;
    db->slot_cap = 0;
    if (db->d_slots.alloc(c)) return ORBX_ERR_HIP;
    db->slot_cap = c;
  }
  if (!sl.empty()) {
    ORBX_TRY(hipMemcpyAsync(db->d_slots, sl.data(), sl.size() * sizeof(BowdbSlot), hipMemcpyHostToDevice,
                            db->stream));
    ORBX_TRY(hipStreamSynchronize(db->stream));
  }
  db->dirty = false;
  return ORBX_OK;
}

// the host's wait for the device form's work in flight, before anything it
// reads is touched or released
int wait_inflight(orbv_db* db) {
  if (!db->inflight) return ORBX_OK;
  ORBX_TRY(hipSetDevice(db->device));
  ORBX_TRY(hipEventSynchronize(db->done));
  db->inflight = false;
  return ORBX_OK;
}

// the batched calls' scratch: the event, and room for `nrec` records
int ensure_batch_scratch(orbv_db* db, size_t nrec) {
  if (!db->done && db->done.create(hipEventDisableTiming)) return ORBX_ERR_HIP;
  if (nrec <= db->rec_cap && db->d_rec) return ORBX_OK;
  const int rc = wait_inflight(db);  // the old scratch may be in use
  if (rc) return rc;
  size_t c = db->rec_cap ? db->rec_cap : 4096;
  while (c < nrec) c *= 2;
  db->rec_cap = 0;
  if (db->d_rec.alloc(c)) return ORBX_ERR_HIP;
  db->rec_cap = c;
  return ORBX_OK;
}

// the two kernels of a batched call on stream s.  Query layout: see
// kernels_bowdb.hip.  lds_words: the longest query the layout allows
void launch_query_batch(hipStream_t s, const orbv_db* db, int nq, int nslots, const uint32_t* q_off, const int* d_n,
                        int qstride, const uint32_t* qw, const double* qv, int lds_words) {
  if (nslots == 0) return;
  // about 2048 workgroups in all: few queries spread over the slots as the
  // single query does, many queries stage each query's words a few times only
  const int bx = std::min((nslots + 3) / 4, std::max(1, (2048 + nq - 1) / nq));
  hipLaunchKernelGGL(k_bowdb_query_batch, dim3(bx, std::min(nq, 65535)), dim3(256),
                     (size_t)lds_words * sizeof(uint32_t), s, q_off, d_n, qstride, qw, qv, nq, db->d_slots, nslots,
                     db->d_words, db->d_values, db->scoring, db->d_rec);
}

void launch_order(hipStream_t s, const orbv_db* db, int nq, int nslots, const uint32_t* q_off, const int* d_n,
                  int qstride, int lds_words, int flags, int mode, int cap, int* cnt, uint64_t* kf_id,
                  int32_t* ncommon, double* score, int* nsharing) {
  hipLaunchKernelGGL(k_bowdb_order, dim3(std::min(nq, 65535)), dim3(BOWDB_ORDER_TILE),
                     (size_t)lds_words * sizeof(uint32_t), s, db->d_rec, db->d_slots, nslots, nq, q_off, d_n, qstride,
                     (flags & ORBV_QUERY_GATED) ? 1 : 0, mode, cap, cnt, kf_id, ncommon, score, nsharing);
}

}  // namespace

extern "C" int orbv_score(const orbv_vocab* v, const uint32_t* a_word, const double* a_value, int na,
                          const uint32_t* b_off, const uint32_t* b_word, const double* b_value, int nvec,
                          double* score) {
  if (!v || na < 0 || nvec < 0 || (na > 0 && (!a_word || !a_value))) return ORBX_ERR_ARG;
  int scoring = 0, nwords = 0;
  if (orbv_vocab_info(v, nullptr, nullptr, &scoring, nullptr, nullptr, &nwords)) return ORBX_ERR_ARG;
  if (!supported(scoring)) return ORBX_ERR_UNSUPPORTED;  // KL, Bhattacharyya: log / sqrt per term
  if (nvec == 0) return ORBX_OK;
  if (!b_off || !score || b_off[0] != 0) return ORBX_ERR_ARG;
  if (na > BOWDB_MAX_WORDS) return ORBX_ERR_UNSUPPORTED;
  if (bowdb_check_words(a_word, na, (uint32_t)nwords)) return ORBX_ERR_ARG;
  for (int j = 0; j < nvec; ++j) {
    if (b_off[j + 1] < b_off[j]) return ORBX_ERR_ARG;
    const uint32_t len = b_off[j + 1] - b_off[j];
    if (len > 0 && (!b_word || !b_value)) return ORBX_ERR_ARG;
    if (len > BOWDB_MAX_WORDS) return ORBX_ERR_UNSUPPORTED;
    if (bowdb_check_words(b_word + b_off[j], (int)len, (uint32_t)nwords)) return ORBX_ERR_ARG;
  }
  const size_t nb = b_off[nvec];
  const int device = vocab_device(v);
  ORBX_TRY(hipSetDevice(device));
  CallArena A(device);
  if (!A.ok()) return ORBX_ERR_HIP;
  auto qw = A.in(a_word, (size_t)na);
  auto qv = A.in(a_value, (size_t)na);
  auto sl = A.in<BowdbSlot>((size_t)nvec);
  auto bw = A.in(b_word, nb);
  auto bv = A.in(b_value, nb);
  auto rec = A.out<BowdbRec>(nullptr, (size_t)nvec);
  if (A.commit()) return ORBX_ERR_HIP;
  BowdbSlot* hs = A.h(sl);
  for (int j = 0; j < nvec; ++j) hs[j] = {(uint64_t)j, (uint64_t)j, b_off[j], b_off[j + 1] - b_off[j], 1u, 0u};
  if (A.upload()) return ORBX_ERR_HIP;
  launch_query(A.stream(), A.d(qw), A.d(qv), na, A.d(sl), nvec, A.d(bw), A.d(bv), scoring, A.d(rec));
  const int rc = A.finish();
  if (rc) return rc;
  const BowdbRec* hr = A.h(rec);
  for (int j = 0; j < nvec; ++j) score[j] = close_score(scoring, hr[j].score);
  return ORBX_OK;
}

extern "C" int orbv_db_create(const orbv_vocab* v, size_t reserve_words, int device, orbv_db** out) {
  if (!out) return ORBX_ERR_ARG;
  *out = nullptr;
  if (!v) return ORBX_ERR_ARG;
  int scoring = 0, nwords = 0;
  if (orbv_vocab_info(v, nullptr, nullptr, &scoring, nullptr, nullptr, &nwords)) return ORBX_ERR_ARG;
  if (!supported(scoring)) return ORBX_ERR_UNSUPPORTED;
  if (reserve_words > 0xFFFFFFFFull) return ORBX_ERR_ARG;
  if (check_device(device)) return ORBX_ERR_NO_DEVICE;
  std::unique_ptr<orbv_db> db(new orbv_db(reserve_words));
  db->device = device;
  db->scoring = scoring;
  db->nwords = (uint32_t)nwords;
  db->slot_cap = 64;
  if (hipSetDevice(device) != hipSuccess || db->d_words.alloc(db->table.capacity()) ||
      db->d_values.alloc(db->table.capacity()) || db->d_slots.alloc(db->slot_cap) || db->stream.create())
    return ORBX_ERR_HIP;
  *out = db.release();
  return ORBX_OK;
}

extern "C" int orbv_db_destroy(orbv_db* db) {
  delete db;
  return ORBX_OK;
}

extern "C" int orbv_db_add(orbv_db* db, uint64_t kf_id, const uint32_t* word, const double* value, int n) {
  if (!db || n < 0 || (n > 0 && (!word || !value))) return ORBX_ERR_ARG;
  if (n > BOWDB_MAX_WORDS) return ORBX_ERR_UNSUPPORTED;
  if (bowdb_check_words(word, n, db->nwords) || db->table.contains(kf_id)) return ORBX_ERR_ARG;
  if (db->table.used() + (size_t)n > 0xFFFFFFFFull) return ORBX_ERR_UNSUPPORTED;  // 32-bit offsets
  ORBX_TRY(hipSetDevice(db->device));
  if (wait_inflight(db)) return ORBX_ERR_HIP;
  const size_t cap = db->table.capacity_for((size_t)n);
  if (cap > db->table.capacity()) {
    std::vector<BowdbMove> whole;
    if (db->table.used()) whole.push_back({0, 0, db->table.used()});
    const int rc = restore(db, cap, whole);
    if (rc) return rc;
    db->table.set_capacity(cap);
  }
  if (n > 0) {
    CallArena A(db->device);
    if (!A.ok()) return ORBX_ERR_HIP;
    auto w = A.in(word, (size_t)n);
    auto v = A.in(value, (size_t)n);
    if (A.commit() || A.upload()) return ORBX_ERR_HIP;
    const size_t at = db->table.used();
    ORBX_TRY(hipMemcpyAsync(db->d_words + at, A.d(w), (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice,
                            A.stream()));
    ORBX_TRY(hipMemcpyAsync(db->d_values + at, A.d(v), (size_t)n * sizeof(double), hipMemcpyDeviceToDevice,
                            A.stream()));
    const int rc = A.finish();
    if (rc) return rc;
  }
  db->table.add(kf_id, (uint32_t)n);
  db->dirty = true;
  return ORBX_OK;
}

extern "C" int orbv_db_erase(orbv_db* db, uint64_t kf_id) {
  if (!db) return ORBX_ERR_ARG;
  if (wait_inflight(db)) return ORBX_ERR_HIP;
  if (!db->table.erase(kf_id)) return ORBX_OK;  // as list::erase never reached
  db->dirty = true;
  if (db->table.wants_compaction()) {
    ORBX_TRY(hipSetDevice(db->device));
    /* the plan is applied to the host table at once: on a failed copy the
     * store would be lost, so take the plan from a copy first */
    BowdbTable next = db->table;
    const std::vector<BowdbMove> moves = next.compact();
    const int rc = restore(db, next.capacity(), moves);
    if (rc) return rc;
    db->table = std::move(next);
  }
  return ORBX_OK;
}

extern "C" int orbv_db_clear(orbv_db* db) {
  if (!db) return ORBX_ERR_ARG;
  if (wait_inflight(db)) return ORBX_ERR_HIP;
  db->table.clear();
  db->dirty = true;
  return ORBX_OK;
}

extern "C" int orbv_db_size(const orbv_db* db, int* nkf) {
  if (!db || !nkf) return ORBX_ERR_ARG;
  *nkf = db->table.nkf();
  return ORBX_OK;
}

extern "C" int orbv_db_query(orbv_db* db, const uint32_t* word, const double* value, int n, int cap,
                             uint64_t* kf_id, int32_t* ncommon, double* score, int* nsharing) {
  if (!db || !nsharing || n < 0 || cap < 0 || (n > 0 && (!word || !value))) return ORBX_ERR_ARG;
  *nsharing = 0;
  if (n > BOWDB_MAX_WORDS) return ORBX_ERR_UNSUPPORTED;
  if (bowdb_check_words(word, n, db->nwords)) return ORBX_ERR_ARG;
  if (n == 0 || db->table.nkf() == 0) return ORBX_OK;
  ORBX_TRY(hipSetDevice(db->device));
  if (wait_inflight(db)) return ORBX_ERR_HIP;
  if (db->dirty) {
    const int rc = upload_slots(db);
    if (rc) return rc;
  }
  const int nslots = (int)db->table.slots().size();
  CallArena A(db->device);
  if (!A.ok()) return ORBX_ERR_HIP;
  auto qw = A.in(word, (size_t)n);
  auto qv = A.in(value, (size_t)n);
  auto rec = A.out<BowdbRec>(nullptr, (size_t)nslots);
  if (A.commit() || A.upload()) return ORBX_ERR_HIP;
  launch_query(A.stream(), A.d(qw), A.d(qv), n, db->d_slots, nslots, db->d_words, db->d_values, db->scoring,
               A.d(rec));
  const int rc = A.finish();
  if (rc) return rc;
  const BowdbRec* hr = A.h(rec);
  /* lKFsSharingWords' order: a keyframe enters at its smallest common word,
   * and within a word in the inverted list's order, which is add order.
   * Slots are in add order (compaction keeps it), so the slot index stands
   * for the sequence number: one 64-bit key per sharing keyframe */
  std::vector<uint64_t> key;
  key.reserve((size_t)nslots);
  for (int j = 0; j < nslots; ++j)
    if (hr[j].ncommon > 0) key.push_back((uint64_t)hr[j].first << 32 | (uint32_t)j);
  std::sort(key.begin(), key.end());
  *nsharing = (int)key.size();
  if ((int)key.size() > cap) return ORBX_ERR_CAPACITY;
  if (!key.empty() && (!kf_id || !ncommon || !score)) return ORBX_ERR_ARG;
  for (size_t i = 0; i < key.size(); ++i) {
    const BowdbRec& r = hr[(uint32_t)key[i]];
    kf_id[i] = r.id;
    ncommon[i] = r.ncommon;
    score[i] = close_score(db->scoring, r.score);
  }
  return ORBX_OK;
}

extern "C" int orbv_db_query_batch(orbv_db* db, int nq, const uint32_t* q_off, const uint32_t* q_word,
                                   const double* q_value, int flags, int cap, uint32_t* out_off, uint64_t* kf_id,
                                   int32_t* ncommon, double* score) {
  if (!db || nq < 0 || cap < 0 || (flags & ~ORBV_QUERY_GATED) || !out_off) return ORBX_ERR_ARG;
  const int ok = bowdb_check_batch(nq, q_off, q_word, q_value, db->nwords);
  if (ok) return ok;
  const int nslots = (int)db->table.slots().size();
  if ((uint64_t)nq * (uint64_t)nslots >= 0x80000000ull) return ORBX_ERR_UNSUPPORTED;
  for (int q = 0; q <= nq; ++q) out_off[q] = 0;
  if (nq == 0 || q_off[nq] == 0 || db->table.nkf() == 0) return ORBX_OK;
  ORBX_TRY(hipSetDevice(db->device));
  if (wait_inflight(db)) return ORBX_ERR_HIP;
  if (db->dirty) {
    const int rc = upload_slots(db);
    if (rc) return rc;
  }
  int rc = ensure_batch_scratch(db, (size_t)nq * (size_t)nslots);
  if (rc) return rc;
  int longest = 0;
  for (int q = 0; q < nq; ++q) longest = std::max(longest, (int)(q_off[q + 1] - q_off[q]));
  // the queries up, the counts down
  CallArena A(db->device);
  if (!A.ok()) return ORBX_ERR_HIP;
  auto qo = A.in(q_off, (size_t)nq + 1);
  auto qw = A.in(q_word, (size_t)q_off[nq]);
  auto qv = A.in(q_value, (size_t)q_off[nq]);
  auto cnt = A.out<int>(nullptr, (size_t)nq);
  if (A.commit() || A.upload()) return ORBX_ERR_HIP;
  launch_query_batch(A.stream(), db, nq, nslots, A.d(qo), nullptr, 0, A.d(qw), A.d(qv), longest);
  launch_order(A.stream(), db, nq, nslots, A.d(qo), nullptr, 0, longest, flags, 0, 0, A.d(cnt), nullptr, nullptr,
               nullptr, nullptr);
  rc = A.finish();
  if (rc) return rc;
  const uint64_t total = bowdb_pack_offsets(A.h(cnt), nq, out_off);
  if (total > (uint64_t)cap) return ORBX_ERR_CAPACITY;
  if (total == 0) return ORBX_OK;
  if (!kf_id || !ncommon || !score) return ORBX_ERR_ARG;
  // the entries in use down: placed by a second pass of the order kernel, which
  // reads the counts and the offsets where the first arena still holds them
  CallArena B(db->device);
  if (!B.ok()) return ORBX_ERR_HIP;
  auto oid = B.out(kf_id, (size_t)total);
  auto onc = B.out(ncommon, (size_t)total);
  auto osc = B.out<double>(nullptr, (size_t)total);
  if (B.commit()) return ORBX_ERR_HIP;
  launch_order(B.stream(), db, nq, nslots, A.d(qo), nullptr, 0, longest, flags, 1, 0, A.d(cnt), B.d(oid), B.d(onc),
               B.d(osc), nullptr);
  rc = B.finish();
  if (rc) return rc;
  const double* hs = B.h(osc);
  for (uint64_t i = 0; i < total; ++i) score[i] = close_score(db->scoring, hs[i]);
  return ORBX_OK;
}

extern "C" int orbv_db_query_batch_device(orbv_db* db, int nq, const uint32_t* d_word, const double* d_value,
                                          const int* d_n, int qstride, int flags, int cap, uint64_t* d_kf_id,
                                          int32_t* d_ncommon, double* d_score, int* d_nsharing, void* stream) {
  if (!db || nq < 0 || cap < 0 || qstride < 0 || (flags & ~ORBV_QUERY_GATED)) return ORBX_ERR_ARG;
  if (qstride > BOWDB_MAX_WORDS) return ORBX_ERR_UNSUPPORTED;
  const int nslots = (int)db->table.slots().size();
  if ((uint64_t)nq * (uint64_t)nslots >= 0x80000000ull) return ORBX_ERR_UNSUPPORTED;
  if (nq == 0) return ORBX_OK;
  if (!d_n || !d_nsharing || (qstride > 0 && (!d_word || !d_value)) ||
      (cap > 0 && (!d_kf_id || !d_ncommon || !d_score)))
    return ORBX_ERR_ARG;
  ORBX_TRY(hipSetDevice(db->device));
  if (db->dirty) {  // the slot table changes under whatever is in flight
    if (wait_inflight(db)) return ORBX_ERR_HIP;
    const int rc = upload_slots(db);
    if (rc) return rc;
  }
  const int rc = ensure_batch_scratch(db, (size_t)nq * (size_t)nslots);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  // an earlier call's kernels, on whichever stream, are done with the scratch first
  if (db->inflight) ORBX_TRY(hipStreamWaitEvent(s, db->done, 0));
  launch_query_batch(s, db, nq, nslots, nullptr, d_n, qstride, d_word, d_value, qstride);
  launch_order(s, db, nq, nslots, nullptr, d_n, qstride, qstride, flags, 2, cap, nullptr, d_kf_id, d_ncommon, d_score,
               d_nsharing);
  ORBX_TRY(hipGetLastError());
  ORBX_TRY(hipEventRecord(db->done, s));
  db->inflight = true;
  return ORBX_OK;
}
