// Stand-alone host program over the owning device buffer (admp_amd/csrc/dev_buf.h), compiled against the counting stand-in
// for the HIP runtime next to it (tests/test_dev_buf_cpu.py compiles and runs it, once more under the address and
// undefined-behaviour sanitizers).  Prints one line per property, "ok <name>" or "FAIL <name>"; exits non-zero on any FAIL.
#include <cstdio>
#include <stdexcept>
#include <type_traits>

#include "dev_buf.h"

using admp::DevBuf;
using admp::Err;

static_assert(!std::is_copy_constructible<DevBuf>::value, "a copied DevBuf would free its allocation twice");
static_assert(!std::is_copy_assignable<DevBuf>::value, "a copied DevBuf would free its allocation twice");

static int failures = 0;
static void check(const char* name, bool ok) {
  std::printf("%s %s\n", ok ? "ok" : "FAIL", name);
  if (!ok) ++failures;
}

struct TwoBuffers { DevBuf ints, reals; };      // the shape of a plan slot of the MD driver

int main() {
  StubHeap& h = stub_heap();
  {
    DevBuf b;
    check("starts empty", b.p == nullptr && b.bytes == 0 && h.live.empty());
    b.need(100);
    void* first = b.p;
    check("need allocates", first && b.bytes == 100 && h.live.size() == 1 && h.bytes == 100 && h.mallocs == 1);
    b.need(40);
    b.need(100);
    check("a smaller or equal request keeps the allocation", b.p == first && b.bytes == 100 && h.mallocs == 1 && h.frees == 0);
    b.need(101);
    check("a larger request grows", b.bytes == 101 && h.live.size() == 1 && h.bytes == 101 && h.mallocs == 2 && h.frees == 1);
    check("as<U> is the pointer", b.as<int>() == static_cast<int*>(b.p));
    h.fail = true;
    bool threw = false;
    try { b.need(1000); } catch (const Err& e) { threw = e.code == ADMP_E_HIP && e.msg.find("out of memory") != std::string::npos; }
    h.fail = false;
    check("a failed hipMalloc throws and leaves {nullptr, 0}", threw && b.p == nullptr && b.bytes == 0 && h.live.empty());
    b.need(8);
    b.release();
    b.release();
    check("release twice is harmless", b.p == nullptr && b.bytes == 0 && h.live.empty() && h.bad_frees == 0);
    b.need(16);
    check("a released buffer can be used again", b.bytes == 16 && h.live.size() == 1);
  }
  check("scope exit frees", h.live.empty() && h.bytes == 0);
  try {      // admp_set_pairs: a staging buffer, then a call that throws before the end of the scope
    DevBuf staged;
    staged.need(64);
    throw Err{ADMP_E_HIP, "a later call failed"};
  } catch (const Err&) {
  }
  check("an exception between need and the end of scope frees", h.live.empty() && h.bytes == 0);
  {
    TwoBuffers slot;
    slot.ints.need(12);
    slot.reals.need(24);
    check("a struct holds two allocations", h.live.size() == 2 && h.bytes == 36);
  }
  check("a struct of two buffers frees both", h.live.empty() && h.bytes == 0);
  check("nothing live at exit, every free was of a live allocation", h.live.empty() && h.mallocs == h.frees && h.bad_frees == 0);
  return failures ? 1 : 0;
}
