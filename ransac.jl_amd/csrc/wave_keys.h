// wave_keys.h -- what the 64 lanes of a wave do together: one action per distinct key among them (the step behind every
// "one atomic per distinct root / label / iteration of a wave"), the butterfly reductions, and the wave's own LDS fence.
// Device code only.  Everything lives in an anonymous namespace, like union_find.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace {

// For every distinct key among the lanes with `act`, in the order of the first lane that holds it, the WHOLE wave calls
// f(leader, L, same): leader = that first lane, L = its key, same = the ballot of the lanes with `act` that hold L.
//   1. Every lane of the wave that is still running must enter, converged, the lanes without a key too (act = false); a
//      kernel whose lanes past the end have returned enters with the rest, and those lanes are in no ballot.
//   2. f runs with all of them converged, so it may ballot and shuffle; what only the leader does, it guards itself
//      (lane == leader).  f must not leave the wave diverged.
template <typename K, typename F>
__device__ __forceinline__ void wave_each_key(bool act, K key, F &&f)
{
    static_assert(std::is_integral<K>::value && sizeof(K) == 4, "a 32-bit integer key");
    uint64_t todo = __builtin_amdgcn_ballot_w64(act);
    while (todo != 0) {
        const int leader = __builtin_ctzll(todo);
        const K L = (K)__shfl((int)key, leader);
        const uint64_t same = __builtin_amdgcn_ballot_w64(key == L) & todo;   // (todo holds active lanes only, and all that hold L)
        f(leader, L, same);
        todo &= ~same;
    }
}

// reductions over the 64 lanes (a butterfly: every lane gets the result)
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op)
{
    for (int d = 32; d > 0; d >>= 1) v = op(v, __shfl_xor(v, d));
    return v;
}
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) { return wave_reduce(v, [](auto a, auto o) { return o < a ? o : a; }); }
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) { return wave_reduce(v, [](auto a, auto o) { return o > a ? o : a; }); }
__device__ __forceinline__ int32_t wave_sum_i32(int32_t v) { return wave_reduce(v, [](auto a, auto o) { return a + o; }); }
__device__ __forceinline__ int32_t wave_min_i32(int32_t v) { return wave_reduce(v, [](auto a, auto o) { return o < a ? o : a; }); }

// the wave's writes to its own LDS rows are visible to its reads behind this
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace
