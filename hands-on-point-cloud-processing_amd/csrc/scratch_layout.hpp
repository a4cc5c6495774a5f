// scratch_layout.hpp — one declared layout per carved device block (host only; includes nothing from HIP).
//
//   Layout L;
//   L.add(&cnt, n);            // uint32_t* cnt: n elements
//   L.add(&temp, bytes);       // void* temp: a raw byte slot (the rocPRIM sort temp block)
//   hipMalloc(&blk, L.bytes()); L.bind(blk);        // or bind_scratch(ctx, L) / bind_aux(ctx, L), pcr_internal.hpp
//
// Every slot starts on a 256-byte boundary; bytes() is the end of the last slot rounded up to 256.  A zero-count slot takes no room and
// shares the address of the next one.  ensure_scratch / ensure_aux may reallocate: pointers bound before a later ensure_* are dead.
#pragma once

#include <cstddef>
#include <cstdio>
#include <cstdlib>

namespace pcr {

inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

struct Layout {
    static constexpr int CAP = 24;         // the largest site (pcr_dbscan_f32) declares 14 slots; one more than CAP aborts
    struct Slot { void** p; size_t off; };
    Slot slot[CAP];
    int n = 0;
    size_t total = 0;

    template <class T> void add(T** p, size_t count) { add_bytes((void**)p, count * sizeof(T)); }
    void add(void** p, size_t n_bytes) { add_bytes(p, n_bytes); }
    size_t bytes() const { return total; }
    void bind(void* base) const
    {
        for (int i = 0; i < n; i++) *slot[i].p = (char*)base + slot[i].off;
    }

private:
    void add_bytes(void** p, size_t n_bytes)
    {
        if (n == CAP) { std::fprintf(stderr, "pcr: more than %d slots in one scratch Layout\n", CAP); std::abort(); }   // a programming error
        slot[n++] = { p, total };
        total += al256(n_bytes);
    }
};

}  // namespace pcr
