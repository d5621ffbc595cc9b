// carve.h — bump carving of one opaque scratch buffer into typed arrays (host code).  A layout is written once, as a function that
// takes its arrays from a Carver: called with base == nullptr it only measures (the *_scratch_bytes / size queries), called with the
// caller's pointer it hands the kernels their arrays — so the size a caller was told and the pointers the kernels get cannot drift apart.
#pragma once
#include <cstddef>

namespace surfel {

inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

struct Carver {
    char* base; size_t align; size_t off = 0;
    // align: every array starts at, and the total is, a multiple of it (256: the rasterizer's buffers; 16: the codecs' scratch)
    explicit Carver(void* b, size_t a = 256) : base(static_cast<char*>(b)), align(a) {}
    template <typename T> T* take(size_t count) {
        off = align_up(off, align);
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += count * sizeof(T);
        return p;
    }
    size_t size() const { return align_up(off, align); }
};

}  // namespace surfel
