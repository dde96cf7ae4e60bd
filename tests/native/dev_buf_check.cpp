// dev_buf_check.cpp -- the owners of csrc/dev_buf.h (rh_dev, rh_pinned, rh_event) and the window list growth step of
// csrc/driver_internal.h against a HIP runtime made of this file: the allocators keep the set of live blocks and a log
// of calls, and fail the k-th allocation on request.  Nothing of the real runtime is linked; built with
// -fsanitize=address,undefined (tests/test_abi.py).  Prints "N checks, 0 bad".
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <string>
#include <utility>
#include <vector>

#include "driver_internal.h"

// ---- the runtime ---------------------------------------------------------------------------------------------------
static std::set<void *> g_live;          // device and pinned blocks
static std::set<void *> g_events;
static std::vector<std::string> g_log;   // "sync", "malloc", "free", "hmalloc", "hfree", "evcreate", "evdestroy"
static std::vector<size_t> g_sizes;      // bytes of every allocation that succeeded
static int g_allocs = 0;                 // allocations asked for since arm()
static int g_fail_at = -1;               // fail the allocation with this number (0-based), -1: none
static hipError_t g_fail_with = hipErrorOutOfMemory;
static bool g_fail_sync = false;         // the next stream waits fail
static bool g_fail_event = false;        // the next event creations fail
static int g_bad_frees = 0;              // a pointer freed that is not live
static char g_err[256] = "";

static void arm(int k, hipError_t e = hipErrorOutOfMemory) { g_allocs = 0; g_fail_at = k; g_fail_with = e; }

void rh_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

static hipError_t fake_alloc(void **p, size_t bytes, const char *what)
{
    g_log.push_back(what);
    if (g_allocs++ == g_fail_at) { *p = nullptr; return g_fail_with; }
    *p = malloc(bytes);
    g_live.insert(*p);
    g_sizes.push_back(bytes);
    return hipSuccess;
}
static hipError_t fake_free(void *p, const char *what)
{
    g_log.push_back(what);
    if (p == nullptr) return hipSuccess;
    if (g_live.erase(p) != 1) { g_bad_frees++; return hipErrorInvalidValue; }
    free(p);
    return hipSuccess;
}

extern "C" {
hipError_t hipMalloc(void **p, size_t bytes) { return fake_alloc(p, bytes, "malloc"); }
hipError_t hipFree(void *p) { return fake_free(p, "free"); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int) { return fake_alloc(p, bytes, "hmalloc"); }
hipError_t hipHostFree(void *p) { return fake_free(p, "hfree"); }
hipError_t hipStreamSynchronize(hipStream_t) { g_log.push_back("sync"); return g_fail_sync ? hipErrorLaunchFailure : hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned)
{
    g_log.push_back("evcreate");
    if (g_fail_event) return hipErrorInvalidValue;
    *e = (hipEvent_t)malloc(1);
    g_events.insert(*e);
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e)
{
    g_log.push_back("evdestroy");
    if (g_events.erase(e) != 1) { g_bad_frees++; return hipErrorInvalidValue; }
    free(e);
    return hipSuccess;
}
const char *hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "some error"; }
}

// ---- the checks ----------------------------------------------------------------------------------------------------
static int g_checks = 0, g_bad = 0;
#define CHECK(x) do { g_checks++; if (!(x)) { g_bad++; printf("line %d: %s\n", __LINE__, #x); } } while (0)

static int count_log(const char *what) { int n = 0; for (const std::string &s : g_log) n += s == what; return n; }

// a struct of arrays of owners, like rhdrv::DeviceStore
struct Store {
    rh_dev<double> prep[4], spare[4];
    rh_dev<int32_t> id[4];
    rh_pinned<int32_t> scr;
    rh_event ev[2];
    int64_t cap[4] = { 0, 0, 0, 0 };
};

// "reserve three buffers, then publish", like store_reserve (driver_store.hip): local owners, moved in at the end
static int reserve3(Store &st, int kind, int64_t cap)
{
    rh_dev<double> np, ns;
    rh_dev<int32_t> ni;
    RH_TRY(np.alloc(cap));
    RH_TRY(ns.alloc(cap));
    RH_TRY(ni.alloc(cap));
    st.prep[kind] = std::move(np);
    st.spare[kind] = std::move(ns);
    st.id[kind] = std::move(ni);
    st.cap[kind] = cap;
    return RH_OK;
}

template <typename Buf>
static void owner_checks(const char *alloc_name, const char *free_name)
{
    g_log.clear();
    {   // the scope end frees exactly once
        Buf a;
        CHECK(a.get() == nullptr && a.count() == 0);
        CHECK(a.alloc(10) == RH_OK && a.get() != nullptr && a.count() == 10);
        CHECK(g_live.size() == 1);
    }
    CHECK(g_live.empty() && count_log(alloc_name) == 1 && count_log(free_name) == 1);
    g_log.clear();
    {   // move construction and move assignment empty the source and free the target's old block exactly once
        Buf a, b;
        CHECK(a.alloc(4) == RH_OK && b.alloc(5) == RH_OK);
        auto *pa = a.get();
        auto *pb = b.get();
        Buf c(std::move(a));
        CHECK(a.get() == nullptr && a.count() == 0 && c.get() == pa && c.count() == 4 && count_log(free_name) == 0);
        c = std::move(b);
        CHECK(b.get() == nullptr && b.count() == 0 && c.get() == pb && c.count() == 5);
        CHECK(count_log(free_name) == 1 && g_live.count(pa) == 0 && g_live.count(pb) == 1);
        Buf &self = c;
        c = std::move(self);   // self-move is harmless
        CHECK(c.get() == pb && c.count() == 5 && g_live.count(pb) == 1);
        c.reset();
        c.reset();             // reset() twice is harmless
        CHECK(c.get() == nullptr && c.count() == 0 && count_log(free_name) == 2);
    }
    CHECK(g_live.empty() && g_bad_frees == 0 && count_log(free_name) == 2);
    {   // count 0 allocates one element
        Buf a;
        g_sizes.clear();
        CHECK(a.alloc(0) == RH_OK && a.get() != nullptr && a.count() == 0);
        CHECK(g_sizes.size() == 1 && g_sizes[0] == sizeof(*a.get()));
    }
    {   // grow: the stream wait before the free, the free before the allocation
        Buf a;
        CHECK(a.alloc(3) == RH_OK);
        g_log.clear();
        CHECK(a.grow(nullptr, 7) == RH_OK && a.count() == 7);
        CHECK(g_log.size() == 3 && g_log[0] == "sync" && g_log[1] == free_name && g_log[2] == alloc_name);
        // a failed wait: RH_E_NODEVICE, nothing freed, nothing allocated, the old block in place; the text names the caller
        auto *old = a.get();
        g_fail_sync = true;
        g_log.clear();
        CHECK(a.grow(nullptr, 9) == RH_E_NODEVICE && a.get() == old && a.count() == 7 && g_live.count(old) == 1);
        CHECK(g_log.size() == 1 && g_log[0] == "sync" && std::string(g_err).find("dev_buf_check.cpp") != std::string::npos);
        g_fail_sync = false;
        // a failed grow / alloc leaves null / 0: RH_E_NOMEM for out of memory, RH_E_NODEVICE otherwise
        arm(0);
        CHECK(a.grow(nullptr, 9) == RH_E_NOMEM && a.get() == nullptr && a.count() == 0 && g_live.empty());
        arm(0, hipErrorInvalidValue);
        CHECK(a.grow(nullptr, 9) == RH_E_NODEVICE && a.get() == nullptr && a.count() == 0);
        arm(0);
        CHECK(a.alloc(9) == RH_E_NOMEM && a.get() == nullptr && a.count() == 0 && g_err[0] != 0);
        arm(0, hipErrorInvalidValue);
        CHECK(a.alloc(9) == RH_E_NODEVICE && a.get() == nullptr && a.count() == 0);
        arm(-1);
        CHECK(a.alloc(9) == RH_OK && a.count() == 9);
    }
    CHECK(g_live.empty() && g_bad_frees == 0);
}

int main()
{
    owner_checks<rh_dev<double>>("malloc", "free");
    owner_checks<rh_pinned<int32_t>>("hmalloc", "hfree");

    {   // a block handed to the library's caller and given back: the owner lets go of it, the runtime's verdict comes through
        rh_dev<char> b;
        CHECK(b.alloc(32) == RH_OK);
        char *p = b.release();
        CHECK(b.get() == nullptr && b.count() == 0 && g_live.count(p) == 1);
        CHECK(rh_free_callers_block(p) == hipSuccess && g_live.empty());
        CHECK(rh_free_callers_block(p) != hipSuccess && g_bad_frees == 1);   // (a pointer that is no block: the caller is told)
        g_bad_frees = 0;
    }

    {   // events
        g_log.clear();
        {
            rh_event a, b;
            CHECK(a.get() == nullptr);
            CHECK(a.create(hipEventDisableTiming) == RH_OK && a.get() != nullptr && b.create(hipEventDisableTiming) == RH_OK);
            hipEvent_t ea = a.get(), eb = b.get();
            rh_event c(std::move(a));
            CHECK(a.get() == nullptr && c.get() == ea);
            c = std::move(b);
            CHECK(b.get() == nullptr && c.get() == eb && g_events.count(ea) == 0 && count_log("evdestroy") == 1);
            rh_event &self = c;
            c = std::move(self);
            CHECK(c.get() == eb && g_events.count(eb) == 1);
        }
        CHECK(g_events.empty() && count_log("evcreate") == 2 && count_log("evdestroy") == 2);
        rh_event e;
        e.reset();
        e.reset();
        CHECK(g_bad_frees == 0);
        // a failed creation: RH_E_NODEVICE and no event -- also where there was one (it went first)
        g_fail_event = true;
        CHECK(e.create(0) == RH_E_NODEVICE && e.get() == nullptr && g_events.empty());
        g_fail_event = false;
        CHECK(e.create(0) == RH_OK && e.get() != nullptr && g_events.size() == 1);
        g_fail_event = true;
        CHECK(e.create(0) == RH_E_NODEVICE && e.get() == nullptr && g_events.empty() && g_bad_frees == 0);
        g_fail_event = false;
    }

    {   // a struct of arrays of owners: std::swap of two members, a whole-struct move
        Store a;
        for (int q = 0; q < 4; q++) CHECK(reserve3(a, q, 8 + q) == RH_OK);
        CHECK(a.scr.alloc(16) == RH_OK && a.ev[0].create(0) == RH_OK);
        CHECK(g_live.size() == 13 && g_events.size() == 1);
        double *p1 = a.prep[1], *s1 = a.spare[1];
        g_log.clear();
        std::swap(a.prep[1], a.spare[1]);
        CHECK(a.prep[1].get() == s1 && a.spare[1].get() == p1 && a.prep[1].count() == 9 && count_log("free") == 0);
        Store b;
        CHECK(reserve3(b, 0, 3) == RH_OK);
        b = std::move(a);   // b's old blocks go, a is empty
        CHECK(g_live.size() == 13 && a.prep[1].get() == nullptr && a.scr.get() == nullptr && a.ev[0].get() == nullptr);
        CHECK(b.prep[1].get() == s1 && b.scr.count() == 16 && b.ev[0].get() != nullptr && count_log("free") == 3);
        a = Store();
        CHECK(g_live.size() == 13);
    }
    CHECK(g_live.empty() && g_events.empty() && g_bad_frees == 0);

    // failing the k-th allocation of "reserve three buffers, then publish": the old buffers intact, no block lost
    for (int k = 0; k < 3; k++) {
        Store st;
        arm(-1);
        CHECK(reserve3(st, 2, 100) == RH_OK);
        double *p = st.prep[2], *s = st.spare[2];
        int32_t *i = st.id[2];
        arm(k);
        CHECK(reserve3(st, 2, 200) == RH_E_NOMEM);
        CHECK(st.prep[2].get() == p && st.spare[2].get() == s && st.id[2].get() == i && st.cap[2] == 100 && st.prep[2].count() == 100);
        CHECK(g_live.size() == 3 && g_live.count(p) == 1 && g_live.count(s) == 1 && g_live.count(i) == 1);
        arm(-1);
        CHECK(reserve3(st, 2, 200) == RH_OK && st.cap[2] == 200 && g_live.size() == 3);
    }
    CHECK(g_live.empty() && g_bad_frees == 0);

    // the window list growth step (driver_internal.h): the capacity never exceeds what is allocated
    for (int k = -1; k < 2; k++) {
        rhdrv::Window w;
        arm(-1);
        g_log.clear();
        CHECK(rhdrv::window_list_grow(nullptr, w, 1 << 10) == RH_OK && w.entries_cap == 1 << 10);
        CHECK(g_log.size() == 3 && g_log[0] == "sync");
        arm(k);
        const int rc = rhdrv::window_list_grow(nullptr, w, 1 << 12);
        CHECK(rc == (k < 0 ? RH_OK : RH_E_NOMEM));
        CHECK(w.entries_cap <= w.d_entries.count() && w.entries_cap <= w.d_counts.count());
        CHECK(w.entries_cap == (k < 0 ? 1 << 12 : 0) && (int)g_live.size() == (k < 0 ? 2 : k));
        arm(-1);
        CHECK(rhdrv::window_list_grow(nullptr, w, 1 << 12) == RH_OK && w.entries_cap == 1 << 12 && g_live.size() == 2);
    }

    {   // ... and a failed wait in it: nothing freed, and the capacity says 0 rather than too much
        rhdrv::Window w;
        CHECK(rhdrv::window_list_grow(nullptr, w, 1 << 10) == RH_OK);
        g_fail_sync = true;
        CHECK(rhdrv::window_list_grow(nullptr, w, 1 << 12) == RH_E_NODEVICE && w.entries_cap == 0 && g_live.size() == 2);
        g_fail_sync = false;
        CHECK(rhdrv::window_list_grow(nullptr, w, 1 << 12) == RH_OK && w.entries_cap == 1 << 12 && g_live.size() == 2);
    }

    CHECK(g_live.empty() && g_events.empty() && g_bad_frees == 0);   // at exit the live set is empty
    printf("%d checks, %d bad\n", g_checks, g_bad);
    return g_bad == 0 ? 0 : 1;
}
