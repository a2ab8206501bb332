// libttasr host side: the owners of everything a context holds beside its arenas - side blocks of device or pinned memory,
// events, a session's second stream - and the cursor that carves a block into regions.  The rule: a resource dies with its holder.
// Plain C++, no HIP: what allocates, releases and waits comes in as a policy (the production ones stand next to HIPCHK in
// engine_ctx.hpp; tests/owned_driver.cpp brings a malloc-backed one that counts and can fail).
#pragma once
#include <cstddef>

namespace ttasr_detail {

// One allocation of M's memory, read as T*.  Starts empty, grows only, is released by its destructor.  M brings
//   const char* alloc(void** p, size_t bytes)   nullptr, or the error's text with *p untouched and no error left pending
//   void release(void* p)
//   int quiesce(C* c)                           0 once nothing enqueued can read the block any more
//   int nomem(C* c, const char* what, size_t bytes, const char* error_text)   records the failure, returns its code
template <class M, class T = char>
class Block {
 public:
  Block() = default;
  Block(Block&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  Block& operator=(Block&& o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
    return *this;
  }
  Block(const Block&) = delete;
  Block& operator=(const Block&) = delete;
  ~Block() { reset(); }

  // At least `bytes`: nothing happens if the block holds them; an empty block allocates exactly `bytes`; a smaller one waits until
  // no enqueued work can read it, is released and allocated anew.  A request that cannot be allocated leaves the block empty (the
  // next call allocates again) and the context otherwise as it was.
  template <class C>
  int ensure(C* c, size_t bytes, const char* what) {
    if (bytes <= n_) return 0;
    if (p_) {
      if (const int rc = M::quiesce(c)) return rc;
      reset();
    }
    void* q = nullptr;
    if (const char* err = M::alloc(&q, bytes)) return M::nomem(c, what, bytes, err);
    p_ = q; n_ = bytes;
    return 0;
  }
  void reset() {
    if (p_) M::release(p_);
    p_ = nullptr; n_ = 0;
  }
  T* get() const { return (T*)p_; }
  operator T*() const { return (T*)p_; }
  size_t size() const { return n_; }

 private:
  void* p_ = nullptr;
  size_t n_ = 0;
};

// One handle of K::type (an event, a stream), destroyed with its holder by K::destroy.  Whoever creates the handle writes it to h.
template <class K>
struct Handle {
  typename K::type h{};
  Handle() = default;
  Handle(Handle&& o) noexcept : h(o.h) { o.h = typename K::type{}; }
  Handle& operator=(Handle&& o) noexcept {
    if (this != &o) { reset(); h = o.h; o.h = typename K::type{}; }
    return *this;
  }
  Handle(const Handle&) = delete;
  Handle& operator=(const Handle&) = delete;
  ~Handle() { reset(); }
  void reset() {
    if (h) K::destroy(h);
    h = typename K::type{};
  }
  operator typename K::type() const { return h; }
};

// A block as consecutive regions, each starting on a multiple of 256 bytes: take() returns where the region starts, `used` is
// the block's size once the last one is taken.
struct Carve {
  size_t used = 0;
  size_t take(size_t bytes) {
    const size_t at = used;
    used += (bytes + 255) & ~(size_t)255;
    return at;
  }
};

}  // namespace ttasr_detail
