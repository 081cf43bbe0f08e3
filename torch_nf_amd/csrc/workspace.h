// Caller-owned workspaces, described once.  A layout function walks a Carver over a base pointer and returns a struct of
// typed region pointers plus the total: run over NULL it is the size query (every pointer NULL, only the offsets
// count), run over the caller's buffer it is the carve.  Nothing else computes an offset into a workspace.
// Plain C++17, no HIP: checked on the CPU (tests/test_workspace_host.py).
#pragma once
#include <stdint.h>

namespace tnf {

inline int64_t round_up(int64_t bytes, int64_t align) { return (bytes + align - 1) / align * align; }
inline bool is_aligned(const void* p, int64_t align) { return reinterpret_cast<uintptr_t>(p) % (uintptr_t)align == 0; }

class Carver {
  public:
    explicit Carver(void* base) : base_(static_cast<char*>(base)) {}
    // `count` elements of T at the next multiple of `align` bytes; NULL when the base is (the offset still advances)
    template <class T> T* take(int64_t count, int64_t align) {
        off_ = round_up(off_, align);
        T* p = base_ ? reinterpret_cast<T*>(base_ + off_) : nullptr;
        off_ += count * (int64_t)sizeof(T);
        return p;
    }
    void reserve(int64_t bytes) { off_ += bytes; }  // bytes no region uses, counted in the total
    // the offset after the last region, rounded up to `align`: the total, or where the next region of that alignment starts
    int64_t bytes(int64_t align = 1) const { return round_up(off_, align); }

  private:
    char* base_;
    int64_t off_ = 0;
};

}  // namespace tnf
