// Host-side ASan/UBSan run of the drop-in calls' typed arena (csrc/call_arena.h)
// over a CallWs whose "pinned" and "device" buffers are two ordinary host
// allocations with their capacity preset, so reserve() allocates nothing and
// no GPU is touched: slot layout (256-byte alignment, no overlap, in_end /
// out_end), zero-length and absent slots, and a round trip of every element
// size and count through gather -> "upload" -> "kernel" -> "download" ->
// scatter.  Built by `make sanitize`.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "call_arena.h"
#include "expect.h"

using orbx::CallArena;
using orbx::CallWs;
using orbx::Slot;

static const size_t kCounts[] = {0, 1, 7, 300};
enum { NC = 4 };

struct Range {
  size_t off, bytes;
};
static std::vector<Range> g_ranges;  // every present slot, in declaration order

template <class T>
static void note(const Slot<T>& s) {
  EXPECT(s.present);
  EXPECT(s.off % 256 == 0);
  g_ranges.push_back({s.off, s.bytes()});
}

static unsigned char pattern(size_t elem, size_t count, size_t byte) {
  return (unsigned char)(elem * 131 + count * 17 + byte * 7 + 3);
}

// the sources, destinations and slots of one element type, one per count
template <class T>
struct Cases {
  std::vector<T> src[NC], dst[NC];
  Slot<T> in[NC], out[NC];

  Cases() {
    for (int c = 0; c < NC; ++c) {
      src[c].resize(kCounts[c]);
      dst[c].resize(kCounts[c]);
      unsigned char* b = reinterpret_cast<unsigned char*>(src[c].data());
      for (size_t i = 0; i < kCounts[c] * sizeof(T); ++i) b[i] = pattern(sizeof(T), kCounts[c], i);
      if (kCounts[c]) memset(dst[c].data(), 0xEE, kCounts[c] * sizeof(T));
    }
  }
  void declare_in(CallArena& A) {
    for (int c = 0; c < NC; ++c) note(in[c] = A.in(static_cast<const T*>(src[c].data()), kCounts[c]));
  }
  void declare_out(CallArena& A) {
    for (int c = 0; c < NC; ++c) note(out[c] = A.out(dst[c].data(), kCounts[c]));
  }
  // the "kernel": every output is its input with all bits flipped
  void device_side(const CallArena& A) const {
    for (int c = 0; c < NC; ++c) {
      const unsigned char* a = reinterpret_cast<const unsigned char*>(A.d(in[c]));
      unsigned char* o = reinterpret_cast<unsigned char*>(A.d(out[c]));
      EXPECT(a != nullptr && o != nullptr);  // a zero-length slot still has an address
      for (size_t i = 0; i < kCounts[c] * sizeof(T); ++i) o[i] = (unsigned char)~a[i];
    }
  }
  void check() const {
    for (int c = 0; c < NC; ++c) {
      const unsigned char* b = reinterpret_cast<const unsigned char*>(dst[c].data());
      size_t bad = 0;
      for (size_t i = 0; i < kCounts[c] * sizeof(T); ++i)
        bad += b[i] != (unsigned char)~pattern(sizeof(T), kCounts[c], i);
      EXPECT(bad == 0);
    }
  }
};

int main() {
  static_assert(sizeof(orbx_keypoint) == 28, "the fourth element size");
  const size_t cap = 1 << 20;
  CallWs w;
  w.h = static_cast<uint8_t*>(malloc(cap));
  w.d = static_cast<uint8_t*>(malloc(cap));
  w.hcap = w.dcap = cap;
  uint8_t* const h0 = w.h;
  uint8_t* const d0 = w.d;
  memset(w.h, 0xAA, cap);
  memset(w.d, 0xBB, cap);
  {
    CallArena A(&w);
    EXPECT(A.ok());
    Cases<uint8_t> c1;
    Cases<uint32_t> c4;
    Cases<uint64_t> c8;
    Cases<orbx_keypoint> c28;
    c1.declare_in(A);
    c4.declare_in(A);
    const uint8_t* none = nullptr;
    const Slot<uint8_t> absent = A.in_opt(none, 300);  // takes no space
    c8.declare_in(A);
    c28.declare_in(A);
    const Slot<int> table = A.in<int>(5);  // built in place
    note(table);
    const size_t want_in_end = g_ranges.back().off + 256;
    c1.declare_out(A);
    c4.declare_out(A);
    c8.declare_out(A);
    c28.declare_out(A);
    const size_t want_out_end = g_ranges.back().off + ((g_ranges.back().bytes + 255) & ~(size_t)255);
    const Slot<int> unused;  // scratch only another path of the call would use
    const Slot<double> scr = A.scratch<double>(33);
    note(scr);
    EXPECT(A.commit() == ORBX_OK);
    EXPECT(w.h == h0 && w.d == d0 && w.hcap == cap && w.dcap == cap);  // nothing reallocated

    // layout: declaration order, 256-byte steps, nothing overlaps
    size_t end = 0;
    for (const Range& r : g_ranges) {
      EXPECT(r.off == end);
      end = r.off + ((r.bytes + 255) & ~(size_t)255);
    }
    EXPECT(A.total() == end && end <= cap);
    EXPECT(A.in_end() == want_in_end);
    EXPECT(A.out_end() == want_out_end);
    EXPECT(A.in_end() % 256 == 0 && A.out_end() % 256 == 0);
    EXPECT(scr.off == A.out_end());
    EXPECT(!absent.present && A.d(absent) == nullptr && A.h(absent) == nullptr);
    EXPECT(!unused.present && A.d(unused) == nullptr);
    EXPECT(A.h(table) == reinterpret_cast<int*>(w.h + table.off));
    EXPECT(A.d(scr) == reinterpret_cast<double*>(w.d + scr.off));

    // round trip
    for (int i = 0; i < 5; ++i) A.h(table)[i] = 100 + i;
    A.gather();
    memcpy(w.d, w.h, A.in_end());                               // stage_in
    for (int i = 0; i < 5; ++i) EXPECT(A.d(table)[i] == 100 + i);
    c1.device_side(A);
    c4.device_side(A);
    c8.device_side(A);
    c28.device_side(A);
    for (int i = 0; i < 33; ++i) A.d(scr)[i] = i;               // scratch is writable on the device side
    memcpy(w.h + A.in_end(), w.d + A.in_end(), A.out_end() - A.in_end());  // finish_call
    A.scatter();
    c1.check();
    c4.check();
    c8.check();
    c28.check();
  }
  free(w.h);
  free(w.d);
  printf("arena: %zu slots, %d failures\n", g_ranges.size(), fails);
  return fails ? 1 : 0;
}
