// Host-side ASan/UBSan run of the handles' resource owners (csrc/owned.h):
// the owner template over malloc'd blocks and a counting free function, so no
// GPU is touched.  An empty owner destroys nothing; the destructor frees
// exactly once; moves empty their source and free what they overwrite;
// reset() twice is safe; alloc on a filled owner frees the old block; a vector
// of owners frees every one; an injected failure (orbx_debug_fail_acquire)
// leaves the owner empty; a plan's table (csrc/plan_table.h) over two such
// owners holds both halves or neither, whichever acquisition fails;
// acquisitions equal releases at exit, on the owners' own counter
// (orbx_debug_live_resources) as well.  Built by `make sanitize`.
#include <stdio.h>
#include <stdlib.h>

#include <utility>
#include <vector>

#include "owned.h"
#include "plan_table.h"
#include "expect.h"

static int g_made = 0, g_freed = 0;
static void counting_free(char* p) {
  ++g_freed;
  free(p);  // ASan reports a block freed twice, or never written through
}

// counted with the device buffers: nothing else here touches that counter
struct HostBuf : orbx::Owned<char*, counting_free, orbx::OWN_DEVICE> {
  int alloc(size_t n) {
    return acquire([n](char** p) {
      *p = static_cast<char*>(malloc(n ? n : 16));
      if (*p) ++g_made;
      return *p != nullptr;
    });
  }
};

static int live() {
  int c[4] = {-1, -1, -1, -1};
  EXPECT(orbx_debug_live_resources(c) == ORBX_OK);
  EXPECT(c[1] == 0 && c[2] == 0 && c[3] == 0);
  return c[0];
}

int main() {
  EXPECT(live() == 0);
  {  // empty: nothing to destroy, reset() is a no-op
    HostBuf e;
    EXPECT(static_cast<char*>(e) == nullptr && !e);
    e.reset();
  }
  EXPECT(g_made == 0 && g_freed == 0);

  {  // the destructor frees exactly once
    HostBuf a;
    EXPECT(a.alloc(100) == ORBX_OK);
    char* p = a;
    EXPECT(p != nullptr);
    p[0] = 1;
    p[99] = 2;
    EXPECT(a[99] == 2 && *(a + 0) == 1);  // used like the raw pointer
    EXPECT(live() == 1);
  }
  EXPECT(g_made == 1 && g_freed == 1 && live() == 0);

  {  // move construction: the source is empty, one block, one free
    HostBuf a;
    EXPECT(a.alloc(8) == ORBX_OK);
    char* const p = a;
    HostBuf b(std::move(a));
    EXPECT(static_cast<char*>(a) == nullptr && static_cast<char*>(b) == p);
    EXPECT(g_freed == 1);
  }
  EXPECT(g_made == 2 && g_freed == 2);

  {  // move assignment: the overwritten target is freed once, at the assignment
    HostBuf a, b;
    EXPECT(a.alloc(8) == ORBX_OK && b.alloc(8) == ORBX_OK);
    char* const pa = a;
    b = std::move(a);
    EXPECT(g_freed == 3);
    EXPECT(static_cast<char*>(a) == nullptr && static_cast<char*>(b) == pa);
    HostBuf& self = b;
    b = std::move(self);  // self-assignment keeps the block
    EXPECT(static_cast<char*>(b) == pa && g_freed == 3);
    b = HostBuf();  // assigning an empty owner releases
    EXPECT(static_cast<char*>(b) == nullptr && g_freed == 4);
  }
  EXPECT(g_made == 4 && g_freed == 4);

  {  // reset() twice; alloc() on a filled owner frees the old block
    HostBuf a;
    EXPECT(a.alloc(0) == ORBX_OK);  // a zero-length request still holds a block
    EXPECT(static_cast<char*>(a) != nullptr);
    a.reset();
    EXPECT(g_freed == 5 && !a);
    a.reset();
    EXPECT(g_freed == 5);
    EXPECT(a.alloc(32) == ORBX_OK);
    EXPECT(a.alloc(64) == ORBX_OK);
    EXPECT(g_made == 7 && g_freed == 6 && live() == 1);
    a[63] = 3;
  }
  EXPECT(g_made == 7 && g_freed == 7);

  {  // a vector of owners (reallocating as it grows) frees all of them
    std::vector<HostBuf> v;
    for (int i = 0; i < 37; ++i) {
      HostBuf b;
      EXPECT(b.alloc(i) == ORBX_OK);
      v.push_back(std::move(b));
    }
    EXPECT(g_made == 44 && g_freed == 7 && live() == 37);
    v.erase(v.begin() + 5);
    EXPECT(g_freed == 8);
  }
  EXPECT(g_made == 44 && g_freed == 44);

  {  // the nth acquisition from now fails without making anything; then disarmed
    HostBuf a, b, c;
    EXPECT(orbx_debug_fail_acquire(2) == ORBX_OK);
    EXPECT(a.alloc(8) == ORBX_OK);
    EXPECT(b.alloc(8) == ORBX_ERR_HIP && !b);
    EXPECT(c.alloc(8) == ORBX_OK);
    EXPECT(g_made == 46 && live() == 2);
    EXPECT(orbx_debug_fail_acquire(1) == ORBX_OK);
    EXPECT(a.alloc(8) == ORBX_ERR_HIP && !a);  // a filled owner gave its block back first
    EXPECT(g_freed == 45 && live() == 1);
    EXPECT(orbx_debug_fail_acquire(1) == ORBX_OK && orbx_debug_fail_acquire(0) == ORBX_OK);
    EXPECT(a.alloc(8) == ORBX_OK);
  }
  EXPECT(g_made == 47 && g_freed == 47 && live() == 0);

  {  // a plan's table over two such owners: both halves or neither
    orbx::PlanTable<char, HostBuf, HostBuf> t;
    EXPECT(!t);
    for (int nth = 1; nth <= 2; ++nth) {  // the device half fails, then the staging half
      EXPECT(orbx_debug_fail_acquire(nth) == ORBX_OK);
      EXPECT(t.alloc(8) == ORBX_ERR_HIP && !t);
      EXPECT(t.host() == nullptr && t.dev() == nullptr);
      EXPECT(g_made == 46 + nth && g_freed == g_made && live() == 0);
    }
    EXPECT(t.alloc(8) == ORBX_OK && t);  // unarmed
    t[0] = 1;
    t.host()[7] = 2;
    EXPECT(t[7] == 2 && t.host()[0] == 1 && t.dev() != nullptr);
    EXPECT(g_made == 50 && g_freed == 48 && live() == 2);
    EXPECT(t.alloc(16) == ORBX_OK && t);  // a filled table frees the old pair
    EXPECT(g_made == 52 && g_freed == 50 && live() == 2);
    t[15] = 3;
    EXPECT(orbx_debug_fail_acquire(2) == ORBX_OK);
    EXPECT(t.alloc(8) == ORBX_ERR_HIP && !t);  // and keeps neither old half when the new staging fails
    EXPECT(g_made == 53 && g_freed == 53 && live() == 0);
  }
  EXPECT(orbx_debug_live_resources(nullptr) == ORBX_ERR_ARG);

  printf("owned: %d acquired, %d released, %d failures\n", g_made, g_freed, fails);
  return fails || g_made != g_freed ? 1 : 0;
}
