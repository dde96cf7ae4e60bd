// root_labels.h -- from a root per point to the numbered labels and the lists: the tail shared by cluster.hip (rh_cluster)
// and segment.hip (rh_segment_smooth).  Both arrive with root[i] = the smallest core point (seed) of the set point i belongs
// to, -1 for none, and kind[i] = RH_PT_*; include/ransac_hip.h, rh_cluster steps 6 and 7, states what follows:
//   sizes    integer atomicAdd per root (one per distinct root of a wave), the min_size filter, an exclusive scan over the
//            root flags in index order for the numbering; BY_SIZE: a radix sort of the M keys (~size, root)
//   labels   labels, the kind counters of the stats, counts[label]; they are written even when the lists do not fit
//   lists    a stable radix sort of (label, index): label 0 first, indices ascending within a label
// No floating-point value is touched.  Everything lives in an anonymous namespace, like call_scope.h.
#pragma once

#include <algorithm>

#include <hipcub/hipcub.hpp>

#include "call_scope.h"
#include "wave_keys.h"

namespace {

// the call's scalars on the device
struct RootScal {
    unsigned long long n_core, n_border, n_noise, n_small;
    int32_t largest, m;
    int32_t aux, pad;        // aux: the caller's own (rh_cluster: its work items)
};

// size[r] = the points whose root is r: the first lane of every distinct root of a wave adds the wave's count
__global__ void rl_size_kernel(const int32_t *__restrict__ root, int64_t n, int32_t *__restrict__ size)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int32_t r = i < n ? root[i] : -1;
    wave_each_key(r >= 0 && (int64_t)r < n, r, [&](int leader, int32_t R, uint64_t same) {
        if (lane == leader) atomicAdd(&size[R], (int32_t)__popcll(same));
    });
}

// flag[r] = r is the root of a set that stays
__global__ void rl_keep_kernel(const int32_t *__restrict__ root, const int32_t *__restrict__ size, int64_t n, int32_t min_size,
                               int32_t *__restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = root[i] == (int32_t)i && size[i] >= min_size;
}

// BY_INDEX: lab[r] = num[r] + 1.  BY_SIZE: the sort key of set num[r], descending size and then ascending root
__global__ void rl_number_kernel(const int32_t *__restrict__ flag, const int32_t *__restrict__ num, const int32_t *__restrict__ size,
                                 int64_t n, int by_size, int32_t *__restrict__ lab, uint64_t *__restrict__ key)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    if (by_size) key[num[i]] = ((uint64_t)(~(uint32_t)size[i]) << 32) | (uint64_t)(uint32_t)i;
    else lab[i] = num[i] + 1;
}

__global__ void rl_rank_kernel(const uint64_t *__restrict__ sorted, int64_t m, int64_t n, int32_t *__restrict__ lab)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const uint64_t r = sorted[k] & 0xFFFFFFFFULL;
    if (r < (uint64_t)n) lab[r] = (int32_t)(k + 1);
}

// labels, the counters of the stats, the list keys; counts[label] (when wanted) from the roots
__global__ void rl_label_kernel(const int32_t *__restrict__ root, const int32_t *__restrict__ flag, const int32_t *__restrict__ lab,
                                const int32_t *__restrict__ size, const uint8_t *__restrict__ kind, int64_t n, int64_t cap,
                                int32_t *__restrict__ labels, int64_t *__restrict__ one_based, int64_t *__restrict__ counts, RootScal *sc)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = i < n;
    const int32_t r = in ? root[i] : -1;
    const bool has = r >= 0 && (int64_t)r < n;
    const int32_t l = has && flag[r] ? lab[r] : 0;
    const int k = in ? kind[i] : -1;
    if (in) {
        labels[i] = l;
        if (one_based) one_based[i] = i + 1;
        if (r == (int32_t)i && l > 0) {
            if (counts && (int64_t)l <= cap) counts[l] = size[i];
            atomicMax(&sc->largest, size[i]);
        }
    }
    const uint64_t bc = __builtin_amdgcn_ballot_w64(k == RH_PT_CORE), bb = __builtin_amdgcn_ballot_w64(k == RH_PT_BORDER),
                   bn = __builtin_amdgcn_ballot_w64(k == RH_PT_NOISE), bs = __builtin_amdgcn_ballot_w64(in && k != RH_PT_NOISE && l == 0);
    if ((threadIdx.x & 63) == 0) {
        if (bc) atomicAdd(&sc->n_core, (unsigned long long)__popcll(bc));
        if (bb) atomicAdd(&sc->n_border, (unsigned long long)__popcll(bb));
        if (bn) atomicAdd(&sc->n_noise, (unsigned long long)__popcll(bn));
        if (bs) atomicAdd(&sc->n_small, (unsigned long long)__popcll(bs));
    }
}

// counts[0] = the points without a label; the slot behind the last count stays 0 (the scan's last offset = n)
__global__ void rl_count0_kernel(const RootScal *sc, int64_t *counts)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[0] = (int64_t)(sc->n_noise + sc->n_small);
}

// What the tail reads and writes.  d_sc: zeroed by the caller apart from aux.  d_mkey, d_msorted: n words each of the
// caller's that are free by now (BY_SIZE sorts in them).  The outputs are the entry point's own arguments.
struct RootTail {
    const char *what;        // "clusters", "regions": for the error texts
    const int32_t *d_root;
    const uint8_t *d_kind;
    int64_t n;
    int32_t min_size;
    int by_size;
    int64_t cap;
    RootScal *d_sc;
    uint64_t *d_mkey, *d_msorted;
    int32_t *labels_out;
    uint8_t *kind_out;
    int64_t *counts_out, *offsets_out, *idx_out;
};

// report(h, m) is called once the labels, the kinds and the counters stand -- before RH_E_CAPACITY is returned and before
// the lists are made: there the entry point writes its *n_out and its stats.
template <typename F>
int root_labels(CallScope &S, RootTail T, F &&report)
{
    const hipStream_t st = S.st;
    const char *who = S.who;
    const int64_t n = T.n;
    const bool tally = T.counts_out != nullptr || T.offsets_out != nullptr;
    const int64_t cap = std::min(T.cap, n);                      // (there are n sets at most: nothing is written beyond)
    RootScal h;
    int32_t *d_size = nullptr, *d_flag = nullptr, *d_num = nullptr, *d_lab = nullptr, *d_labels = nullptr;
    RH_TRY(S.alloc(&d_size, n)); RH_TRY(S.alloc(&d_flag, n)); RH_TRY(S.alloc(&d_num, n)); RH_TRY(S.alloc(&d_lab, n));
    RH_TRY(S.alloc(&d_labels, n));
    int64_t *d_one = nullptr, *d_idx = nullptr, *d_counts = nullptr, *d_offsets = nullptr;
    int32_t *d_lsorted = nullptr;
    if (T.idx_out) { RH_TRY(S.alloc(&d_one, n)); RH_TRY(S.alloc(&d_idx, n)); RH_TRY(S.alloc(&d_lsorted, n)); }

    // sizes, the min_size filter, the numbering
    SCOPE_HIP(S, hipMemsetAsync(d_size, 0, sizeof(int32_t) * (size_t)n, st));
    hipLaunchKernelGGL(rl_size_kernel, dim3(blocks_for(n)), dim3(256), 0, st, T.d_root, n, d_size);
    hipLaunchKernelGGL(rl_keep_kernel, dim3(blocks_for(n)), dim3(256), 0, st, T.d_root, d_size, n, T.min_size, d_flag);
    SCOPE_HIP(S, hipGetLastError());
    RH_TRY(S.cub([&](void *t, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(t, b, d_flag, d_num, (int)n, st); }));
    hipLaunchKernelGGL(scan_total_kernel, dim3(1), dim3(64), 0, st, d_flag, d_num, n, &T.d_sc->m);   // the sets that stay
    hipLaunchKernelGGL(rl_number_kernel, dim3(blocks_for(n)), dim3(256), 0, st, d_flag, d_num, d_size, n, T.by_size, d_lab, T.d_mkey);
    SCOPE_HIP(S, hipGetLastError());
    RH_TRY(S.fetch(&h, T.d_sc));
    const int64_t m = h.m;
    if (m < 0 || m > n) { rh_set_error("%s: %lld %s of %lld points", who, (long long)m, T.what, (long long)n); return RH_E_INTERNAL; }
    if (T.by_size && m > 0) {
        RH_TRY(S.cub([&](void *t, size_t &b) { return hipcub::DeviceRadixSort::SortKeys(t, b, T.d_mkey, T.d_msorted, (int)m, 0, 64, st); }));
        hipLaunchKernelGGL(rl_rank_kernel, dim3(blocks_for(m)), dim3(256), 0, st, T.d_msorted, m, n, d_lab);
    }

    // labels and stats; they are written even when the lists do not fit
    const bool fits = !tally || m <= cap;
    if (tally && fits) {
        RH_TRY(S.alloc(&d_counts, cap + 2));
        RH_TRY(S.alloc(&d_offsets, cap + 2));
        SCOPE_HIP(S, hipMemsetAsync(d_counts, 0, sizeof(int64_t) * (size_t)(cap + 2), st));
    }
    hipLaunchKernelGGL(rl_label_kernel, dim3(blocks_for(n)), dim3(256), 0, st, T.d_root, d_flag, d_lab, d_size, T.d_kind, n, cap, d_labels,
                       d_one, d_counts, T.d_sc);
    SCOPE_HIP(S, hipGetLastError());
    SCOPE_HIP(S, hipMemcpyAsync(&h, T.d_sc, sizeof h, hipMemcpyDeviceToHost, st));
    SCOPE_HIP(S, hipMemcpyAsync(T.labels_out, d_labels, sizeof(int32_t) * (size_t)n, hipMemcpyDefault, st));
    if (T.kind_out) SCOPE_HIP(S, hipMemcpyAsync(T.kind_out, T.d_kind, (size_t)n, hipMemcpyDefault, st));
    SCOPE_HIP(S, hipStreamSynchronize(st));
    report(h, m);
    if (!fits) {
        rh_set_error("%s: %lld %s, counts / offsets hold %lld", who, (long long)m, T.what, (long long)cap);
        return RH_E_CAPACITY;
    }

    // lists
    if (tally) {
        hipLaunchKernelGGL(rl_count0_kernel, dim3(1), dim3(64), 0, st, T.d_sc, d_counts);
        SCOPE_HIP(S, hipGetLastError());
        RH_TRY(S.cub([&](void *t, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(t, b, d_counts, d_offsets, (int)(cap + 2), st); }));
        if (T.counts_out) SCOPE_HIP(S, hipMemcpyAsync(T.counts_out, d_counts, sizeof(int64_t) * (size_t)(cap + 1), hipMemcpyDefault, st));
        if (T.offsets_out) SCOPE_HIP(S, hipMemcpyAsync(T.offsets_out, d_offsets, sizeof(int64_t) * (size_t)(cap + 2), hipMemcpyDefault, st));
    }
    if (T.idx_out) {
        const int bits = sort_bits((uint64_t)m + 1);            // (the labels are 0 .. m)
        RH_TRY(S.cub([&](void *t, size_t &b) { return hipcub::DeviceRadixSort::SortPairs(t, b, d_labels, d_lsorted, d_one, d_idx, (int)n, 0, bits, st); }));
        SCOPE_HIP(S, hipMemcpyAsync(T.idx_out, d_idx, sizeof(int64_t) * (size_t)n, hipMemcpyDefault, st));
    }
    SCOPE_HIP(S, hipStreamSynchronize(st));
    return RH_OK;
}

}  // namespace
