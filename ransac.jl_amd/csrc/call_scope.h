// call_scope.h -- what an entry point on raw host arrays (rh_voxel_downsample, rh_knn, rh_remove_outliers, rh_knn_query,
// rh_cloud_distance, rh_register, rh_describe, rh_match_features, rh_register_global, rh_cluster, rh_segment_smooth, rh_orient_normals, rh_estimate_normals, rh_assign_points, rh_largestconncomp) owns for the length of the call: the device, a stream of its
// own and its device buffers, released on every way out -- among them the ONE scratch block of the call's hipcub
// launches (cub) -- and the read-back of the call's scalars (fetch).  The cloud-bound paths do not come here: a cloud has
// its stream and its grown buffers (rh_dev::grow, RH_HIP).
// Everything lives in an anonymous namespace: each translation unit that includes the header gets its own kernels.
#pragma once

#include <vector>

#include "rh_internal.h"

namespace {

inline unsigned blocks_for(int64_t n, int per = 256) { return (unsigned)((n + per - 1) / per); }
inline size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

template <typename T>
__global__ void scope_widen_kernel(const T *__restrict__ in, double *__restrict__ out, int64_t cnt)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cnt) out[i] = (double)in[i];
}

// *out = the number of flags set among flag[0 .. n - 1] (num = the exclusive scan of flag, n >= 1)
__global__ void scan_total_kernel(const int32_t *__restrict__ flag, const int32_t *__restrict__ num, int64_t n, int32_t *out)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) *out = num[n - 1] + flag[n - 1];
}

// the key bits a radix sort has to look at when the keys are 0 .. count - 1
inline int sort_bits(uint64_t count)
{
    int bits = 1;
    while (bits < 64 && (count - 1) >> bits) bits++;
    return bits;
}

// a HIP call of scope S_ that must succeed
#define SCOPE_HIP(S_, x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) { rh_set_error("%s: %s", (S_).who, hipGetErrorString(e_)); return RH_E_NODEVICE; } } while (0)

struct CallScope {
    const char *who = "";    // the entry point, for error texts
    hipStream_t st = nullptr;
    std::vector<rh_dev<char>> bufs;
    char *scratch = nullptr;    // hipcub's temporary storage: one block, as large as the largest request so far
    size_t scratch_bytes = 0;
    CallScope() = default;
    CallScope(const CallScope &) = delete;
    CallScope &operator=(const CallScope &) = delete;
    // the buffers first (hipFree waits for the device: copies still in flight at an early return end there), then the stream
    ~CallScope()
    {
        bufs.clear();
        if (st) (void)hipStreamDestroy(st);
    }

    // the usable device and a non-blocking stream of the call's own
    int open(const char *who_, int device)
    {
        who = who_;
        int ndev = 0;
        RH_TRY(rh_device_count(&ndev));
        if (ndev <= 0) { rh_set_error("no HIP device is visible; libransac_hip has no CPU fallback"); return RH_E_NODEVICE; }
        if (device < 0 || device >= ndev) { rh_set_error("device %d out of range (%d visible)", device, ndev); return RH_E_INVALID; }
        SCOPE_HIP(*this, hipSetDevice(device));
        SCOPE_HIP(*this, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        return RH_OK;
    }

    template <typename T>
    int alloc(T **p, int64_t count)
    {
        *p = nullptr;
        rh_dev<char> b;
        const int rc = b.alloc((int64_t)sizeof(T) * (count > 0 ? count : 1), who);
        if (rc != RH_OK) {
            (void)hipGetLastError();
            return rc;
        }
        *p = (T *)b.get();
        bufs.push_back(std::move(b));
        return RH_OK;
    }

    // before the call ends (null and foreign pointers are ignored)
    void release(void *p)
    {
        for (auto &b : bufs)
            if (b.get() == p) b.reset();
    }

    // cnt values of T from the caller's array into doubles on the device, widened exactly
    template <typename T>
    int upload(const T *src, double *dst, int64_t cnt, hipMemcpyKind kind)
    {
        if (sizeof(T) == sizeof(double)) {
            SCOPE_HIP(*this, hipMemcpyAsync(dst, src, sizeof(double) * (size_t)cnt, kind, st));
            return RH_OK;
        }
        T *d_in = nullptr;
        RH_TRY(alloc(&d_in, cnt));
        SCOPE_HIP(*this, hipMemcpyAsync(d_in, src, sizeof(T) * (size_t)cnt, kind, st));
        RH_TRY(widen(d_in, dst, cnt));
        SCOPE_HIP(*this, hipStreamSynchronize(st));
        release(d_in);
        return RH_OK;
    }

    // cnt values of T on the device into doubles (queued on the stream)
    template <typename T>
    int widen(const T *d_in, double *dst, int64_t cnt)
    {
        hipLaunchKernelGGL(scope_widen_kernel<T>, dim3(blocks_for(cnt)), dim3(256), 0, st, d_in, dst, cnt);
        SCOPE_HIP(*this, hipGetLastError());
        return RH_OK;
    }

    // One hipcub launch on the scope's scratch block: call(tmp, bytes) -> hipError_t is the hipcub call with these two as its
    // first arguments.  It is made twice: with tmp = null it only states its size (host code, nothing is launched), then it
    // runs on the block, which is replaced (never kept twice) when it is too small.  A replacement waits for the device
    // (hipFree) and leaves an empty entry in bufs: expected a few times per call, where a later request is the larger one --
    // not in a loop whose requests keep growing.
    template <typename F>
    int cub(F &&call)
    {
        size_t bytes = 0;
        SCOPE_HIP(*this, call(nullptr, bytes));
        if (!scratch || bytes > scratch_bytes) {
            release(scratch);
            scratch_bytes = 0;
            RH_TRY(alloc(&scratch, (int64_t)bytes));
            scratch_bytes = bytes;
        }
        SCOPE_HIP(*this, call(scratch, bytes));
        return RH_OK;
    }

    // count values of T from the device, and the wait for them (and for everything queued before)
    template <typename T>
    int fetch(T *host, const T *dev, size_t count = 1)
    {
        SCOPE_HIP(*this, hipMemcpyAsync(host, dev, sizeof(T) * count, hipMemcpyDeviceToHost, st));
        SCOPE_HIP(*this, hipStreamSynchronize(st));
        return RH_OK;
    }
};

}  // namespace
