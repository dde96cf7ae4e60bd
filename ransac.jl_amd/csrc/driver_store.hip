// driver_store.hip -- how what a run of rh_ransac allocates grows and goes: the device store of prepared candidates, the
// windows' lists, the pinned staging ring, the buffers parked on the cloud between runs, and the result arenas
#include "driver_internal.h"

namespace rhdrv {

int store_reserve(rh_cloud *c, DeviceStore &st, int kind, int64_t need)
{
    if (need <= st.cap[kind]) {
        if (st.id[kind] == nullptr && st.cap[kind] > 0) {   // (a store parked by a run that kept no ids)
            RH_TRY(st.id[kind].alloc(st.cap[kind]));
            RH_TRY(st.Eb[kind].alloc(st.cap[kind]));
        }
        return RH_OK;
    }
    const int64_t cap = std::max<int64_t>(need, std::max<int64_t>(4096, st.cap[kind] * 2));
    rh_dev<rh_prep> np;   // (local owners: a failure below loses nothing and leaves the store as it was)
    rh_dev<int32_t> ni;
    rh_dev<double> ne;
    RH_TRY(np.alloc(cap));
    RH_TRY(ni.alloc(cap));
    RH_TRY(ne.alloc(cap));
    if (st.n[kind] > 0) {
        RH_HIP(hipMemcpyAsync(np, st.prep[kind], sizeof(rh_prep) * (size_t)st.n[kind], hipMemcpyDeviceToDevice, c->stream));
        if (st.id[kind] != nullptr) {
            RH_HIP(hipMemcpyAsync(ni, st.id[kind], sizeof(int32_t) * (size_t)st.n[kind], hipMemcpyDeviceToDevice, c->stream));
            RH_HIP(hipMemcpyAsync(ne, st.Eb[kind], sizeof(double) * (size_t)st.n[kind], hipMemcpyDeviceToDevice, c->stream));
        }
    }
    RH_HIP(hipStreamSynchronize(c->stream));
    st.prep[kind] = std::move(np);
    st.id[kind] = std::move(ni);
    st.Eb[kind] = std::move(ne);
    st.cap[kind] = cap;
    return RH_OK;
}

int store_reserve_aux(rh_cloud *c, DeviceStore &st, int64_t need)
{
    if (need <= st.iota_cap) return RH_OK;
    const int64_t cap = std::max<int64_t>(need, std::max<int64_t>(4096, st.iota_cap * 2));
    st.iota_cap = 0;
    RH_HIP(hipStreamSynchronize(c->stream));
    st.iota.reset(); st.counts.reset(); st.d_idx.reset();
    RH_TRY(st.iota.alloc(cap));
    RH_TRY(st.counts.alloc(cap));
    RH_TRY(st.d_idx.alloc(cap));
    RH_TRY(rhk_iota(c, st.iota, (int32_t)cap, 0));
    st.iota_cap = cap;
    return RH_OK;
}

// ---- result arenas ---------------------------------------------------------------------------
// The index lists of a run (<= 8 bytes x the points enabled at its start) land in ONE pinned host
// block: the D2H copies are asynchronous at PCIe rate and nothing is copied a second time
// (pageable destinations cost ~0.25 ms per extracted shape at 10M points).  Pinning is slow, so
// blocks are recycled through a small process-wide pool: rh_result_free hands the block back.
struct ArenaBlock { void *p; size_t cap; bool in_use; };
std::mutex g_arena_mu;
std::vector<ArenaBlock> g_arenas;

void *arena_acquire(size_t bytes)
{
    std::lock_guard<std::mutex> lk(g_arena_mu);
    int bestfit = -1;
    for (size_t i = 0; i < g_arenas.size(); i++)
        if (!g_arenas[i].in_use && g_arenas[i].cap >= bytes && (bestfit < 0 || g_arenas[i].cap < g_arenas[(size_t)bestfit].cap))
            bestfit = (int)i;
    if (bestfit >= 0) { g_arenas[(size_t)bestfit].in_use = true; return g_arenas[(size_t)bestfit].p; }
    for (size_t i = 0; i < g_arenas.size();) {   // too small to be useful again: give the pages back
        if (!g_arenas[i].in_use) { (void)hipHostFree(g_arenas[i].p); g_arenas.erase(g_arenas.begin() + (long)i); }
        else i++;
    }
    void *p = nullptr;
    const size_t cap = std::max<size_t>(bytes, 1 << 20);
    if (hipHostMalloc(&p, cap, hipHostMallocDefault) != hipSuccess) return nullptr;
    g_arenas.push_back({ p, cap, true });
    return p;
}

void arena_release(void *p)
{
    if (!p) return;
    std::lock_guard<std::mutex> lk(g_arena_mu);
    int nfree = 0;
    for (ArenaBlock &b : g_arenas) nfree += !b.in_use;
    for (size_t i = 0; i < g_arenas.size(); i++) {
        if (g_arenas[i].p != p) continue;
        if (nfree >= 2) { (void)hipHostFree(p); g_arenas.erase(g_arenas.begin() + (long)i); }
        else g_arenas[i].in_use = false;
        return;
    }
}

void pin_ring_wait(PinRing &r)
{
    for (int i = 0; i < 4; i++) {
        if (r.busy[i] && r.ev[i]) (void)hipEventSynchronize(r.ev[i]);
        r.busy[i] = false;
    }
}

// the buffers a run parked on the cloud (cloud_free, while c->stream is valid): the waits, then everything goes with the struct
void driver_cache_free(rh_cloud *c, void *p)
{
    DriverCache *dc = (DriverCache *)p;
    if (!dc) return;
    pin_ring_wait(dc->ring);
    (void)hipStreamSynchronize(c->stream);
    delete dc;
}

}  // namespace rhdrv

using namespace rhdrv;

extern "C" void rh_result_free(rh_result *r)
{
    if (!r) return;
    arena_release(r->arena);
    free(r->shapes);
    memset(r, 0, sizeof *r);
}
