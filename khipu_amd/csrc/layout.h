// Workspace layouts: the arrays carved out of one device buffer, each declared once --
// L.add(ptr, count) of the pointer's element type (a void*: bytes; absent: nullptr, and it still
// counts as an empty entry), L.add_all(count, ptrs...), L.pad(bytes) for slack that no pointer
// names; then buf.ensure(L.bytes()) and L.place(buf.p, buf.cap), which sets the pointers.
// Every entry starts 256-byte aligned and is followed by 16 bytes of slack (8-byte word
// over-reads); the total carries 256 bytes of tail.  Host-only, plain C++17 (the CPU tests
// compile it with g++): the owner passes its way of failing as Fail.
#pragma once

#include <cstddef>
#include <cstring>
#include <type_traits>

namespace khst {

template <void (*Fail)(const char*)>
class BasicLayout {
 public:
  static constexpr int MAX_ENTRIES = 96;  // (phase 1 of the build declares 64)
  BasicLayout() = default;
  BasicLayout(const BasicLayout&) = delete;  // (the entries point at the caller's pointers)

  // Returns the entry's byte offset: with end(), the extent of a run of consecutive entries.
  template <typename T>
  size_t add(T*& p, size_t count, bool present = true) {
    using E = std::conditional_t<std::is_void_v<T>, char, T>;
    p = nullptr;
    if (n_ == MAX_ENTRIES) Fail("workspace layout: too many entries");
    slot_[n_] = present ? &p : nullptr;
    return off_[n_++] = pad(present ? count * sizeof(E) : 0);
  }
  template <typename... T>
  void add_all(size_t count, T*&... p) {
    (add(p, count), ...);
  }
  size_t pad(size_t bytes) {
    const size_t at = (end_ + 255) & ~(size_t)255;
    end_ = at + bytes + 16;
    return at;
  }
  size_t end() const { return end_ - 16; }     // where the last entry's elements end
  size_t bytes() const { return end_ + 256; }  // what to request

  void place(void* base, size_t have) const {
    if (have < bytes()) Fail("workspace layout: placed into too few bytes");
    for (int i = 0; i < n_; ++i) {
      char* a = (char*)base + off_[i];
      if (slot_[i]) memcpy(slot_[i], &a, sizeof(a));  // (the slot is a T* of some T)
    }
  }

 private:
  void* slot_[MAX_ENTRIES];  // the caller's pointer variables (nullptr: absent)
  size_t off_[MAX_ENTRIES];
  int n_ = 0;
  size_t end_ = 0;
};

}  // namespace khst
