// Bump arena over a caller-allocated workspace.  A workspace layout is ONE function that takes its regions from an Arena, in order;
// run on a measuring arena (no base) it yields the size, run on a carving arena (a base) it yields the pointers, so the
// `*_workspace_bytes` query and the entry point cannot disagree.  Plain C++ (no HIP header): a host compiler builds it alone
// (tests/arena_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace nrl {

struct Arena {
  unsigned char* base = nullptr;  // null: measuring -- every take returns null and only the offset advances
  size_t off = 0;

  Arena() = default;
  explicit Arena(void* ws) : base(static_cast<unsigned char*>(ws)) {}

  static size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

  // `count` elements of T; the region starts at a multiple of align_bytes (from the base) and its size is padded to one
  template <class T>
  T* take(size_t count, size_t align_bytes = 256) { return take_after<T>(0, count, align_bytes); }

  // a region of `count` elements whose first `lead` are slack in front of the returned pointer (count includes the slack)
  template <class T>
  T* take_after(size_t lead, size_t count, size_t align_bytes = 256) {
    const size_t at = round_up(off, align_bytes);
    off = at + round_up(count * sizeof(T), align_bytes);
    // (no arithmetic on a null base: the measuring pass never forms a pointer)
    return base != nullptr ? reinterpret_cast<T*>(base + at) + lead : nullptr;
  }

  size_t bytes() const { return off; }  // used so far
};

}  // namespace nrl
