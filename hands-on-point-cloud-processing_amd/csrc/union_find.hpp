// union_find.hpp — the lock-free union-find of cluster.hip (DBSCAN) and range_image.hip (range-image labelling).
//
// parent[x] <= x always (a root is hooked under a SMALLER root by atomicCAS(&parent[hi], hi, lo)), so every path strictly decreases, a
// find takes at most n steps and the final root of a set is its smallest member; more steps mean a corrupt structure: a device error
// word is set and the call returns PCR_ERR_STATE.  A failed CAS means another lane hooked `hi` first; the union continues from the value
// the CAS returned.  Hooks succeed at most n - 1 times overall, so the retry loop is bounded by n as well.  Finds halve their path with
// plain atomic stores: a node that is not a root is never hooked again, and the grandparent it is pointed at is one of its ancestors for
// good, so a stale or overwritten shortcut is still a shortcut within the same set.  parent[] is read with agent-scope atomic loads
// (eight XCDs, eight L2s): only the per-location order of parent[] itself matters, no other data is published through it, so relaxed
// order suffices.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace pcr {

__device__ __forceinline__ uint32_t uf_load(const uint32_t* parent, uint32_t i)
{
    return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of x, with path halving while HALVE; at most n steps (indices strictly decrease along a path), else err |= 1
template <bool HALVE = true>
__device__ __forceinline__ uint32_t uf_find(uint32_t* parent, uint32_t x, uint32_t n, uint32_t* err)
{
    for (uint32_t step = 0; step <= n; step++) {
        const uint32_t px = uf_load(parent, x);
        if (px == x) return x;
        const uint32_t gp = uf_load(parent, px);
        if (gp == px) return px;
        if (HALVE) __hip_atomic_store(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = gp;
    }
    atomicOr(err, 1u);
    return x;
}

// a and b are roots (or ancestors of the two sets); hooks the larger root under the smaller one
__device__ __forceinline__ void uf_union(uint32_t* parent, uint32_t a, uint32_t b, uint32_t n, uint32_t* err)
{
    for (uint32_t it = 0; it <= n; it++) {
        a = uf_find(parent, a, n, err);
        b = uf_find(parent, b, n, err);
        if (a == b) return;
        const uint32_t hi = max(a, b), lo = min(a, b);
        const uint32_t old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return;
        a = old;                                            // hi was hooked by another lane in between: go on from there
        b = lo;
    }
    atomicOr(err, 2u);
}

}  // namespace pcr
