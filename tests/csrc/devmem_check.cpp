// The ownership rules of csrc/rs_devmem.h (DevBuf, dev_alloc_all) against a HIP runtime of this file's own: hipMalloc and its kin are
// malloc underneath, with a count of the live blocks and a switch that fails the k-th allocation from now.  Stand-alone: built by
// tests/test_devmem.py with g++ -fsanitize=address,undefined and without the HIP runtime, run with leak detection on.  Exits 0 when
// every rule holds, 1 with the line of the first that does not.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../../radiosaber_amd/csrc/rs_devmem.h"

static int g_live = 0, g_frees = 0;
static int g_fail_in = -1;  // fail the allocation that comes after this many more successful ones; -1: none

extern "C" hipError_t hipMalloc(void** p, size_t bytes) {
  if (g_fail_in == 0) { g_fail_in = -1; *p = nullptr; return hipErrorOutOfMemory; }
  if (g_fail_in > 0) g_fail_in--;
  *p = malloc(bytes);
  g_live++;
  return hipSuccess;
}
extern "C" hipError_t hipFree(void* p) {
  if (p) { g_live--; g_frees++; }
  free(p);
  return hipSuccess;
}
extern "C" hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {
  memcpy(dst, src, bytes);
  return hipSuccess;
}
extern "C" hipError_t hipMemset(void* dst, int value, size_t bytes) {
  memset(dst, value, bytes);
  return hipSuccess;
}

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      fprintf(stderr, "devmem_check.cpp:%d: %s\n", __LINE__, #cond);     \
      return 1;                                                          \
    }                                                                    \
  } while (0)

static int single_buffer() {
  DevBuf<int> a;
  CHECK(!a && a.get() == nullptr && a.count() == 0 && a.bytes() == 0);
  // a first allocation sets the size
  CHECK(a.alloc(5) == hipSuccess);
  CHECK(a && a.count() == 5 && a.bytes() == 20 && g_live == 1);
  const int five[5] = {1, 2, 3, 4, 5};
  int back[5] = {0, 0, 0, 0, 0};
  CHECK(a.upload(five) == hipSuccess && a.download(back) == hipSuccess && memcmp(five, back, sizeof five) == 0);
  int* const as_pointer = a;  // (what every launch block and launcher call reads)
  CHECK(as_pointer == a.get() && a + 2 == a.get() + 2 && a[4] == 5);
  // a replacing allocation frees the old block exactly once
  const int frees0 = g_frees;
  CHECK(a.alloc(3) == hipSuccess);
  CHECK(a.count() == 3 && g_live == 1 && g_frees == frees0 + 1);
  CHECK(a.zero() == hipSuccess && a[0] == 0 && a[2] == 0);
  // a failed replacing allocation keeps the old pointer, size and contents
  CHECK(a.upload(five) == hipSuccess);
  int* const kept = a;
  g_fail_in = 0;
  CHECK(a.alloc(100) == hipErrorOutOfMemory);
  CHECK(a.get() == kept && a.count() == 3 && g_live == 1 && g_frees == frees0 + 1 && a[0] == 1 && a[2] == 3);
  // assign = alloc + upload; a block of no elements is set and empty
  CHECK(a.assign(five, 4) == hipSuccess && a.count() == 4 && a[3] == 4 && g_live == 1);
  CHECK(a.alloc_zeroed(3) == hipSuccess && a.count() == 3 && a[0] == 0 && a[1] == 0 && a[2] == 0 && g_live == 1);
  CHECK(a.alloc(0) == hipSuccess && a && a.count() == 0 && a.bytes() == 0 && g_live == 1);
  CHECK(a.upload(nullptr) == hipSuccess && a.zero() == hipSuccess && a.download(nullptr) == hipSuccess);
  // release() twice is harmless
  a.release();
  CHECK(!a && a.count() == 0 && g_live == 0);
  const int frees1 = g_frees;
  a.release();
  CHECK(g_live == 0 && g_frees == frees1);
  // a move empties its source
  CHECK(a.alloc(7) == hipSuccess);
  int* const block = a;
  DevBuf<int> b(std::move(a));
  CHECK(!a && a.count() == 0 && b.get() == block && b.count() == 7 && g_live == 1);
  DevBuf<int> c;
  CHECK(c.alloc(2) == hipSuccess && g_live == 2);
  c = std::move(b);  // (the target's own block goes)
  CHECK(!b && b.count() == 0 && c.get() == block && c.count() == 7 && g_live == 1);
  return 0;  // (c frees itself here)
}

// a family of four, of three element types; `full`: the members hold blocks already
static int family(bool full) {
  const int n = 4;
  for (int k = 0; k <= n; k++) {  // k == n: no failure
    DevBuf<double> w;
    DevBuf<int> e, p;
    DevBuf<unsigned char> u;
    if (full) {
      CHECK(dev_alloc_all(w, 2, e, 3, p, 4, u, 5) == hipSuccess);
      CHECK(w.zero() == hipSuccess && u.zero() == hipSuccess);
      w[1] = 2.5;
      u[4] = 9;
    }
    const int live0 = g_live, frees0 = g_frees;
    CHECK(live0 == (full ? n : 0));
    void* const was[n] = {w.get(), e.get(), p.get(), u.get()};
    const size_t had[n] = {w.count(), e.count(), p.count(), u.count()};
    g_fail_in = k < n ? k : -1;
    const hipError_t rc = dev_alloc_all(w, 20, e, 30, p, 40, u, 50);
    void* const is[n] = {w.get(), e.get(), p.get(), u.get()};
    const size_t has[n] = {w.count(), e.count(), p.count(), u.count()};
    if (k < n) {
      // failing the k-th allocation leaves every member as it was, and the live count unchanged
      CHECK(rc == hipErrorOutOfMemory && g_live == live0 && g_frees == frees0 + k);
      for (int i = 0; i < n; i++) CHECK(is[i] == was[i] && has[i] == had[i]);
      if (full) CHECK(w[1] == 2.5 && u[4] == 9);
    } else {
      CHECK(rc == hipSuccess && g_live == n && g_frees == frees0 + (full ? n : 0));
      const size_t want[n] = {20, 30, 40, 50};
      for (int i = 0; i < n; i++) CHECK(is[i] != nullptr && (!full || is[i] != was[i]) && has[i] == want[i]);
    }
    CHECK(g_fail_in == -1);  // (the switch was reached)
  }
  return 0;
}

int main() {
  if (single_buffer() || family(false) || family(true)) return 1;
  // the live count is 0 at exit
  CHECK(g_live == 0);
  printf("devmem_check: ok (%d blocks freed)\n", g_frees);
  return 0;
}
