// CPU check of DevBuf (cdae_amd/csrc/cdae_dev_buf.h): the memory seam is defined over malloc / free with a live-block counter, a switch
// that fails the next acquire and one that makes the next release report an error (after freeing).  Built with the address and
// undefined-behaviour sanitizers and run by tests/test_dev_buf_cpu.py; exit 0 = every property below holds.
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "../../cdae_amd/csrc/cdae_dev_buf.h"

namespace {
long g_live = 0, g_acquires = 0, g_releases = 0;
size_t g_last_bytes = 0;
bool g_fail_acquire = false, g_fail_release = false;
int g_failed = 0;
}  // namespace

namespace cdae { namespace mem {
int acquire(void** p, size_t bytes) {
  if (g_fail_acquire) { g_fail_acquire = false; return 1; }
  void* q = std::malloc(bytes);
  if (!q) return 1;
  *p = q; ++g_live; ++g_acquires; g_last_bytes = bytes;
  return 0;
}
int release(void* p) {
  std::free(p); --g_live; ++g_releases;
  if (g_fail_release) { g_fail_release = false; return 1; }
  return 0;
}
} }  // namespace cdae::mem

#define EXPECT(cond)                                                               \
  do {                                                                             \
    if (!(cond)) { std::printf("%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); ++g_failed; } \
  } while (0)

static_assert(!std::is_copy_constructible<DevBuf<float>>::value, "an owner must not be copied");
static_assert(!std::is_copy_assignable<DevBuf<float>>::value, "an owner must not be copied");
static_assert(std::is_nothrow_move_constructible<DevBuf<float>>::value && std::is_nothrow_move_assignable<DevBuf<float>>::value, "move-only");

int main() {
  {   // ensure: grow-only, in units of `per` elements
    DevBuf<float> b;
    EXPECT(b.p == nullptr && b.cap == 0 && !b);
    EXPECT(b.ensure(10, 3) == 0 && b.p && b.cap == 10 && g_live == 1 && g_last_bytes == 30 * sizeof(float));
    float* const first = b.p;
    const long acq = g_acquires;
    b.p[29] = 1.f;
    EXPECT(b.ensure(10, 3) == 0 && b.ensure(4, 3) == 0 && b.p == first && b.cap == 10 && g_acquires == acq);   // cap >= n: nothing
    const long rel = g_releases;
    EXPECT(b.ensure(11, 3) == 0 && b.cap == 11 && g_acquires == acq + 1 && g_releases == rel + 1 && g_live == 1);   // above: old block released first
    b.p[32] = 2.f;
    EXPECT((float*)b == b.p);
    // a failed acquire in ensure: empty, nothing live
    g_fail_acquire = true;
    EXPECT(b.ensure(100) != 0 && b.p == nullptr && b.cap == 0 && g_live == 0);
    EXPECT(b.ensure(1) == 0 && b.cap == 1 && g_live == 1);
  }
  EXPECT(g_live == 0);   // destruction releases
  {   // alloc: exact size, at least one element, old block released first
    DevBuf<double> b;
    EXPECT(b.alloc(0) == 0 && b.p != nullptr && b.cap == 0 && g_live == 1 && g_last_bytes == sizeof(double));
    b.p[0] = 1.0;
    const long rel = g_releases;
    EXPECT(b.alloc(7) == 0 && b.cap == 7 && g_releases == rel + 1 && g_live == 1 && g_last_bytes == 7 * sizeof(double));
    b.p[6] = 1.0;
    EXPECT(b.alloc(3) == 0 && b.cap == 3 && g_releases == rel + 2 && g_live == 1);   // (not grow-only: a smaller request reallocates)
    g_fail_acquire = true;
    EXPECT(b.alloc(5) != 0 && b.p == nullptr && b.cap == 0 && g_live == 0);
    // drop clears both members even when release reports an error, and returns the error
    EXPECT(b.alloc(2) == 0 && g_live == 1);
    g_fail_release = true;
    EXPECT(b.drop() != 0 && b.p == nullptr && b.cap == 0 && g_live == 0);
    EXPECT(b.drop() == 0);                                                            // empty: no release call
    // ... and so do ensure and alloc when the drop inside them fails: the error is returned, nothing is acquired
    EXPECT(b.alloc(2) == 0);
    g_fail_release = true;
    EXPECT(b.alloc(4) != 0 && b.p == nullptr && b.cap == 0 && g_live == 0);
    EXPECT(b.ensure(2) == 0);
    g_fail_release = true;
    EXPECT(b.ensure(4) != 0 && b.p == nullptr && b.cap == 0 && g_live == 0);
  }
  EXPECT(g_live == 0);
  {   // moves
    DevBuf<float> a;
    EXPECT(a.alloc(5) == 0);
    float* const pa = a.p;
    DevBuf<float> b(std::move(a));
    EXPECT(a.p == nullptr && a.cap == 0 && b.p == pa && b.cap == 5 && g_live == 1);
    DevBuf<float> c;
    EXPECT(c.alloc(9) == 0 && g_live == 2);
    c = std::move(b);                                                                 // the target's own block is released
    EXPECT(b.p == nullptr && b.cap == 0 && c.p == pa && c.cap == 5 && g_live == 1);
    DevBuf<float>& same = c;
    c = std::move(same);                                                              // self-assignment keeps the block
    EXPECT(c.p == pa && c.cap == 5 && g_live == 1);
    // std::swap of two arrays (install_staged)
    DevBuf<float> x[4], y[4];
    for (int i = 0; i < 4; ++i) EXPECT(x[i].ensure(i + 1, 2) == 0);
    EXPECT(y[2].alloc(50) == 0);
    float* px[4]; for (int i = 0; i < 4; ++i) px[i] = x[i].p;
    float* const py2 = y[2].p;
    const long live = g_live, acq = g_acquires, rel = g_releases;
    std::swap(x, y);
    EXPECT(g_live == live && g_acquires == acq && g_releases == rel);               // ownership moved: no copy, no release
    for (int i = 0; i < 4; ++i) EXPECT(y[i].p == px[i] && y[i].cap == (size_t)i + 1);
    EXPECT(x[2].p == py2 && x[2].cap == 50 && x[0].p == nullptr && x[1].p == nullptr && x[3].p == nullptr && x[0].cap == 0);
    EXPECT(g_live == 6);
  }
  EXPECT(g_live == 0);
  EXPECT(g_acquires == g_releases);
  if (g_failed) { std::printf("dev_buf check: %d expectation(s) failed\n", g_failed); return 1; }
  std::printf("dev_buf check OK\n");
  return 0;
}
