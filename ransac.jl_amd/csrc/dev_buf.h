// dev_buf.h -- the owners of device memory, pinned host memory and events.  Host code only (a plain host compiler takes it).
//   rh_dev<T>     a device buffer of T (hipMalloc / hipFree)
//   rh_pinned<T>  the same in pinned host memory (hipHostMalloc(..., hipHostMallocDefault) / hipHostFree)
//   rh_event      an event (hipEventCreateWithFlags / hipEventDestroy)
// All three are move-only and release what they hold when they go; a struct made of them needs no free list.  Whoever
// merely reads a buffer -- kernel arguments, rh_score_job, rh_bins, rh_store_plan -- keeps a raw pointer.  A release waits
// for nothing: the owner's holder waits for the streams that may still use its buffers first (cloud_free, batch_ws_free,
// Driver::~Driver), grow() for the one stream it is given.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "ransac_hip.h"

void rh_set_error(const char *fmt, ...);

// the library's error for a failed allocation (the two buffer types and CallScope::alloc; nobody else allocates)
inline int rh_alloc_failed(const char *who, const char *call, size_t bytes, hipError_t e)
{
    rh_set_error("%s%s%s(%zu bytes) failed: %s", who, *who ? ": " : "", call, bytes, hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? RH_E_NOMEM : RH_E_NODEVICE;
}

template <typename T, bool PINNED>
class rh_buf {
    T *p_ = nullptr;
    int64_t n_ = 0;

public:
    rh_buf() = default;
    rh_buf(const rh_buf &) = delete;
    rh_buf &operator=(const rh_buf &) = delete;
    rh_buf(rh_buf &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    rh_buf &operator=(rh_buf &&o) noexcept
    {
        if (this != &o) {
            reset();
            p_ = o.p_; n_ = o.n_;
            o.p_ = nullptr; o.n_ = 0;
        }
        return *this;
    }
    ~rh_buf() { reset(); }

    T *get() const { return p_; }
    operator T *() const { return p_; }
    T *operator->() const { return p_; }
    int64_t count() const { return n_; }   // the elements it was allocated for (0: empty)

    void reset()
    {
        if (p_) (void)(PINNED ? hipHostFree((void *)p_) : hipFree((void *)p_));
        p_ = nullptr;
        n_ = 0;
    }
    // hands the block to the library's caller, who gives it back through rh_free_callers_block (rh_dev_alloc / rh_dev_free of the ABI)
    T *release() { T *p = p_; p_ = nullptr; n_ = 0; return p; }

    // `count` elements (0: one element); a failure leaves the buffer empty.  A buffer that holds a block lets it go first,
    // WITHOUT a wait -- for blocks no stream can still be using, or whose free is the wait (hipFree / hipHostFree wait for the
    // device): the sampler's set_ws / set_level / crec, the pinned h_pin and staging ring, oct_tab / oct_code_o, and growth
    // steps of several buffers that wait once themselves (window_list_grow, store_reserve_aux, the store's spare arrays).
    // Anything else in use grows through grow().
    int alloc(int64_t count, const char *who = "")
    {
        reset();
        void *p = nullptr;
        const size_t bytes = sizeof(T) * (size_t)(count > 0 ? count : 1);
        const hipError_t e = PINNED ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
        if (e != hipSuccess) return rh_alloc_failed(who, PINNED ? "hipHostMalloc" : "hipMalloc", bytes, e);
        p_ = (T *)p;
        n_ = count;
        return RH_OK;
    }
    // the one way a buffer in use grows: wait for `stream` (whatever may still read the old block), free, allocate, and only
    // then publish pointer and count; a failed allocation leaves null / 0, a failed wait the buffer as it was.  The contents
    // are not kept.  (file / line: the caller's, for the error text)
    int grow(hipStream_t stream, int64_t count, const char *file = __builtin_FILE(), int line = __builtin_LINE())
    {
        const hipError_t e = hipStreamSynchronize(stream);
        if (e != hipSuccess) {
            rh_set_error("hipStreamSynchronize before growing a buffer failed: %s (%s:%d)", hipGetErrorString(e), file, line);
            return RH_E_NODEVICE;
        }
        return alloc(count);
    }
};

template <typename T> using rh_dev = rh_buf<T, false>;
template <typename T> using rh_pinned = rh_buf<T, true>;

// a device block that rh_dev::release handed to the library's caller comes back (rh_dev_free): the runtime's verdict on the
// pointer is the caller's to see
inline hipError_t rh_free_callers_block(void *p) { return hipFree(p); }

class rh_event {
    hipEvent_t e_ = nullptr;

public:
    rh_event() = default;
    rh_event(const rh_event &) = delete;
    rh_event &operator=(const rh_event &) = delete;
    rh_event(rh_event &&o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    rh_event &operator=(rh_event &&o) noexcept
    {
        if (this != &o) { reset(); e_ = o.e_; o.e_ = nullptr; }
        return *this;
    }
    ~rh_event() { reset(); }

    hipEvent_t get() const { return e_; }
    operator hipEvent_t() const { return e_; }
    void reset()
    {
        if (e_) (void)hipEventDestroy(e_);
        e_ = nullptr;
    }
    int create(unsigned flags)
    {
        reset();
        const hipError_t e = hipEventCreateWithFlags(&e_, flags);
        if (e != hipSuccess) {
            e_ = nullptr;
            rh_set_error("hipEventCreateWithFlags failed: %s", hipGetErrorString(e));
            return RH_E_NODEVICE;
        }
        return RH_OK;
    }
};
