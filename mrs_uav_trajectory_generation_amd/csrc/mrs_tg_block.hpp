// mrs_tg_block.hpp -- the one owner of a block of memory that a plan, a context or a scope keeps (internal).
//
// Plain C++17, no HIP include: the allocator comes in as the template parameter `Alloc`,
//   using Error = ...;  static constexpr Error ok = ...;
//   static Error alloc(void** p, size_t bytes);   // *p is only read when ok is returned
//   static void free(void* p);
//   static Error idle();   // after it nothing uses any block: what growing a block that is in use waits for by default
// The library's are PoolAlloc and PinnedAlloc (mrs_tg_pool.h); tests/host/block_harness.cpp has a counting fake.
//
// A block is either held (a pointer and the count it was allocated for) or empty (null, 0); no call leaves anything between.
// The destructor hands a held block back without waiting: whoever destroys an owner has made its stream idle first.
#pragma once
#include <cstddef>

namespace mrs_tg {

template <class T, class Alloc>
class Block {
 public:
  using Error = typename Alloc::Error;

  Block() = default;
  Block(const Block&) = delete;
  Block& operator=(const Block&) = delete;
  ~Block() { reset(); }

  T* get() const { return ptr_; }
  size_t count() const { return count_; }  // elements asked for when the block was allocated (headroom included)
  bool holds(size_t count) const { return count_ >= count && ptr_; }

  void reset() {
    if (ptr_) Alloc::free(ptr_);
    ptr_ = nullptr;
    count_ = 0;
  }

  // At least `count` elements (the one minimum-size rule: a request of zero is a request of one).  A block that is large enough
  // is left alone.  Otherwise a held block is given back first, behind `idle()`: what idle() says is returned, the old block is
  // freed whatever it says, and nothing is allocated behind an error.  Then count + headroom elements are allocated; if that
  // fails the block is empty and the allocator's error is returned.
  template <class Idle>
  Error ensure(size_t count, Idle&& idle, size_t headroom = 0) {
    if (holds(count)) return Alloc::ok;
    if (ptr_) {
      const Error waited = idle();
      reset();
      if (waited != Alloc::ok) return waited;
    }
    const size_t want = (count ? count : 1) + headroom;
    void* p = nullptr;
    const Error e = Alloc::alloc(&p, want * sizeof(T));
    if (e != Alloc::ok) return e;
    ptr_ = static_cast<T*>(p);
    count_ = want;
    return Alloc::ok;
  }
  Error ensure(size_t count) { return ensure(count, Alloc::idle); }

  // ensure(count) for a block that is filled once, when it is allocated: fill(pointer) runs right behind a fresh allocation and
  // never otherwise.  A fill that fails empties the block again (nothing of a failed fill is in flight), so the next call
  // allocates and fills anew instead of reading what the allocator left.
  template <class Fill>
  Error ensure_filled(size_t count, Fill&& fill) {
    if (holds(count)) return Alloc::ok;
    Error e = ensure(count);
    if (e == Alloc::ok && (e = fill(ptr_)) != Alloc::ok) reset();
    return e;
  }

 private:
  T* ptr_ = nullptr;
  size_t count_ = 0;
};

// Two blocks that are only of use together: afterwards both are held or, behind an error, both are empty.
template <class T, class U, class Alloc>
typename Alloc::Error ensure_both(Block<T, Alloc>& a, size_t count_a, Block<U, Alloc>& b, size_t count_b) {
  typename Alloc::Error e = a.ensure(count_a);
  if (e == Alloc::ok) e = b.ensure(count_b);
  if (e != Alloc::ok) {
    a.reset();
    b.reset();
  }
  return e;
}

}  // namespace mrs_tg
