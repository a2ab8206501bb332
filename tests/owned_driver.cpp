// Host driver of csrc/owned.hpp (tests/test_owned_driver_host.py compiles it as plain C++ under the address and undefined-
// behaviour sanitizers and runs it): the block type over a malloc-backed memory policy that counts live allocations, records the
// order of quiesce / release / alloc calls and fails the k-th allocation on request; the handle type over a counting kind; the
// carve cursor against the running sum of sizes rounded up to 256.  The failure paths of Block::ensure are checked here and
// nowhere else: on a GPU they would take a device starved of memory.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../taiwan_tongues_asr_ce_amd/csrc/owned.hpp"

using namespace ttasr_detail;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
  } while (0)

struct Ctx { std::string err; int code = 0; };

struct FakeMem {
  static int live, allocs, fail_at /*the allocs-th allocation from now fails; 0: none*/, quiesce_rc;
  static std::string log;   // 'q' quiesce, 'f' release, 'a' allocation, 'x' failed allocation
  static std::set<void*> held;   // what alloc gave out and release has not taken back: every release names one of these
  static int releases;
  static const char* alloc(void** p, size_t bytes) {
    if (fail_at && --fail_at == 0) { log += 'x'; return "out of fake memory"; }
    *p = malloc(bytes);   // exactly `bytes`: the sanitizer sees a touch of byte `bytes`
    CHECK(*p && held.insert(*p).second);
    ++live; ++allocs; log += 'a';
    return nullptr;
  }
  static void release(void* p) {
    CHECK(held.erase(p) == 1);   // given out, and not released before
    free(p);
    --live; ++releases; log += 'f';
  }
  static int quiesce(Ctx* c) { log += 'q'; if (quiesce_rc) c->code = quiesce_rc; return quiesce_rc; }
  static int nomem(Ctx* c, const char* what, size_t bytes, const char* err) {
    c->err = std::string(what) + " (" + std::to_string(bytes) + " bytes): " + err;
    return c->code = -3;
  }
  static void clear() { CHECK(held.empty()); log.clear(); }
};
int FakeMem::live = 0, FakeMem::allocs = 0, FakeMem::fail_at = 0, FakeMem::quiesce_rc = 0;
std::string FakeMem::log;
std::set<void*> FakeMem::held;
int FakeMem::releases = 0;

struct FakeKind {
  using type = int*;
  static int destroyed;
  static void destroy(int* h) { ++destroyed; delete h; }
};
int FakeKind::destroyed = 0;

using Blk = Block<FakeMem, uint8_t>;

static void touch(Blk& b) { for (size_t i = 0; i < b.size(); ++i) b[i] = (uint8_t)i; }

static void test_ensure() {
  Ctx c;
  {
    Blk b;
    CHECK(!b && b.get() == nullptr && b.size() == 0);
    CHECK(b.ensure(&c, 0, "nothing") == 0 && !b && FakeMem::log.empty());   // 0 bytes of an empty block: nothing to hold
    CHECK(b.ensure(&c, 1000, "block") == 0);
    CHECK(b && b.size() == 1000 && FakeMem::log == "a" && FakeMem::live == 1);   // exactly the request, no wait on first use
    touch(b);
    uint8_t* const first = b;
    CHECK(b.ensure(&c, 1000, "block") == 0 && b.ensure(&c, 1, "block") == 0 && b.ensure(&c, 0, "block") == 0);
    CHECK(b.get() == first && b.size() == 1000 && FakeMem::log == "a");          // equal or smaller: same pointer, no wait
    CHECK(b.ensure(&c, 1001, "block") == 0);
    CHECK(b.size() == 1001 && FakeMem::log == "aqfa" && FakeMem::live == 1);     // larger: quiesce, release, allocate
    touch(b);
  }
  CHECK(FakeMem::live == 0 && FakeMem::log == "aqfaf");   // the destructor released the second allocation
  FakeMem::clear();
}

static void test_failures() {
  Ctx c;
  {
    Blk b;
    FakeMem::fail_at = 1;   // failure on first use
    CHECK(b.ensure(&c, 64, "first block") == -3);
    CHECK(!b && b.size() == 0 && FakeMem::live == 0 && FakeMem::log == "x");
    CHECK(c.err == "first block (64 bytes): out of fake memory");
    CHECK(b.ensure(&c, 64, "first block") == 0 && b.size() == 64 && FakeMem::log == "xa");   // the next call allocates
    touch(b);
    FakeMem::fail_at = 1;   // failure on regrow: the old block is gone (it was released to make room), the block is empty
    CHECK(b.ensure(&c, 128, "grown block") == -3);
    CHECK(!b && b.size() == 0 && FakeMem::live == 0 && FakeMem::log == "xaqfx");
    CHECK(c.err == "grown block (128 bytes): out of fake memory");
    CHECK(b.ensure(&c, 32, "grown block") == 0 && b.size() == 32 && FakeMem::log == "xaqfxa");   // no wait: nothing was held
    touch(b);
    FakeMem::quiesce_rc = -2;   // a wait that fails keeps the block in service: nothing may be released under enqueued work
    uint8_t* const kept = b;
    CHECK(b.ensure(&c, 4096, "grown block") == -2 && b.get() == kept && b.size() == 32 && FakeMem::log == "xaqfxaq");
    FakeMem::quiesce_rc = 0;
    b.reset();
    CHECK(!b && b.size() == 0 && FakeMem::live == 0);
    b.reset();   // of an empty block: nothing
    CHECK(FakeMem::log == "xaqfxaqf");
  }
  CHECK(FakeMem::live == 0 && FakeMem::log == "xaqfxaqf");
  FakeMem::clear();
}

static void test_moves() {
  Ctx c;
  const int before = FakeMem::allocs, freed = FakeMem::releases;
  {
    Blk a;
    CHECK(a.ensure(&c, 300, "a") == 0);
    uint8_t* const p = a;
    Blk b(std::move(a));
    CHECK(!a && a.size() == 0 && b.get() == p && b.size() == 300);   // the source is empty
    CHECK(a.ensure(&c, 10, "a") == 0 && a.size() == 10);             // ... and an empty block like any other
    Blk d;
    CHECK(d.ensure(&c, 20, "d") == 0);
    d = std::move(b);                                                // releases what d held
    CHECK(!b && b.size() == 0 && d.get() == p && d.size() == 300 && FakeMem::live == 2);
    touch(d);
    std::vector<Blk> v;
    for (int i = 0; i < 9; ++i) { v.emplace_back(); CHECK(v.back().ensure(&c, 16 + i, "v") == 0); }   // reallocation moves them
    for (int i = 0; i < 9; ++i) { CHECK(v[i].size() == (size_t)(16 + i)); touch(v[i]); }
    CHECK(FakeMem::live == 11);
  }
  CHECK(FakeMem::live == 0 && FakeMem::allocs - before == 12 && FakeMem::releases - freed == 12);   // each released exactly once
  FakeMem::clear();
}

static void test_handles() {
  {
    Handle<FakeKind> e, f;
    CHECK(!e);
    e.h = new int(7);
    Handle<FakeKind> g(std::move(e));
    CHECK(!e && g && *g.h == 7);
    f.h = new int(8);
    f = std::move(g);   // destroys what f held
    CHECK(!g && *f.h == 7 && FakeKind::destroyed == 1);
    f.reset(); f.reset();
    CHECK(!f && FakeKind::destroyed == 2);
    e.h = new int(9);
  }
  CHECK(FakeKind::destroyed == 3);   // e's; the empty ones destroy nothing
}

static void test_carve() {
  const size_t sizes[] = {0, 1, 255, 256, 257, 0, 1000000007, 512, 3};
  Carve cv;
  size_t sum = 0;
  for (size_t b : sizes) {
    CHECK(cv.take(b) == sum && sum % 256 == 0);
    sum += (b + 255) / 256 * 256;
    CHECK(cv.used == sum);
  }
  Carve one;
  CHECK(one.take(0) == 0 && one.take(1) == 0 && one.take(255) == 256 && one.take(256) == 512 && one.take(257) == 768 && one.used == 1280);
}

int main() {
  test_ensure();
  test_failures();
  test_moves();
  test_handles();
  test_carve();
  CHECK(FakeMem::live == 0 && FakeMem::held.empty() && FakeMem::releases == FakeMem::allocs);
  printf("owned driver ok: %d allocations, 0 live\n", FakeMem::allocs);
  return 0;
}
