// union_find.h -- lock-free union-find on the device, over an array of parents L (cc.hip: pixels, component.hip: the slots
// of the cell table, cluster.hip: the points, segment.hip: the seeds).  A root points at itself and is the smallest index of its set, parents only ever go down, so a link
// to any ancestor is a valid link.  Flatten with atomicMin(&L[i], root), never a plain store: a neighbour's path halving
// may write L[i] at the same time.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

__device__ __forceinline__ int32_t ld(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ int32_t uf_find(int32_t *L, int32_t i)
{
    int32_t p = ld(&L[i]);
    while (p != i) {
        const int32_t gp = ld(&L[p]);
        if (gp != p) atomicMin(&L[i], gp);   // path halving: i is no root and never becomes one again
        i = p;
        p = gp;
    }
    return i;
}

__device__ void uf_unite(int32_t *L, int32_t a, int32_t b)
{
    for (;;) {
        a = uf_find(L, a);
        b = uf_find(L, b);
        if (a == b) return;
        if (a > b) { const int32_t t = a; a = b; b = t; }
        const int32_t old = atomicMin(&L[b], a);   // hang the larger root under the smaller
        if (old == b) return;
        b = old;                                    // somebody re-parented b meanwhile: retry from there
    }
}

}  // namespace
