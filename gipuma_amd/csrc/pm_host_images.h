// pm_host_images.h -- the images of a session of gipuma_hip.hip: making them resident, the 8-bit verdict, the window-packed
// copies of the selected views, and the cache of both per resident plane (GIPUMA_HIP_FLAG_CACHE_IMAGES).  The cache and its
// lock are private to this header: callers see make_images_resident, classify_and_pack, release_cached_images and cache_clear.
#pragma once
#include <map>
#include <mutex>

#include "pm_host_session.h"

namespace {

// what has been derived from a resident image plane (CacheKey)
struct CachedImage {
    int not_u8 = -1;              // result of the 8-bit check (-1: not run yet)
    uint32_t *packed = nullptr;   // window-packed copy (pack_kernel / pack_kernel_c4)
    int users = 0;                // live sessions whose Problem points at `packed`
};
std::map<CacheKey, CachedImage> g_cache;
std::mutex g_cache_mutex;

// images: bind resident planes, or upload the reference + the selected views (compact pitch)
int make_images_resident(Session *s, const gipuma_hip_desc *d)
{
    const bool on_device = (d->flags & GIPUMA_HIP_FLAG_IMAGES_ON_DEVICE) != 0;
    const size_t row_bytes = (size_t)d->cols * d->channels * sizeof(float);
    for (int i = 0; i <= d->n_selected; i++) {
        const int idx = i == 0 ? 0 : d->selected[i - 1];
        const float *&dst = i == 0 ? s->hp.ref.raw : s->hp.view[i - 1].img.raw;
        if (on_device) {
            dst = d->images[idx];
            continue;
        }
        float *p = nullptr;
        if (const int rc = s->alloc({&p, row_bytes * d->rows})) return rc;
        dst = p;
        HIP_OK(hipMemcpy2DAsync(p, row_bytes, d->images[idx], (size_t)d->pitch * sizeof(float), row_bytes, (size_t)d->rows,
                                hipMemcpyHostToDevice, s->stream));
    }
    return 0;
}

// U8 mode (weight table + window-packed source views) if every image handed to the path is
// integer valued in [0,255] -- 8-bit input converted to float, main.cpp:941.  With `cached`, under g_cache_mutex; `fresh`
// lists the cache entries whose `packed` this call allocated.
int classify_and_pack_locked(Session *s, bool cached, std::vector<CachedImage *> &fresh)
{
    pm::Problem &hp = s->hp;
    auto plane = [&](int i) -> const float * { return i == 0 ? hp.ref : hp.view[i - 1].img; };  // 0: the reference
    auto key = [&](int i) { return CacheKey(s->device, plane(i), s->rows, s->cols, hp.pitch, s->ch); };
    auto entry = [&](int i) -> CachedImage * { return cached ? &g_cache[key(i)] : nullptr; };
    // one flag per checked plane, planes whose verdict is cached are skipped
    const int n_planes = 1 + s->n_sel;
    int *flag = nullptr;
    if (const int rc = s->alloc({&flag, sizeof(int) * n_planes, 0})) return rc;
    const dim3 cg((s->cols + pm::kThreads - 1) / pm::kThreads, s->rows);
    auto check = s->ch == 4 ? pm::check_u8_kernel_c4 : pm::check_u8_kernel;
    std::vector<int> verdict(n_planes, -1);
    for (int i = 0; i < n_planes; i++) {
        CachedImage *e = entry(i);
        if (e && e->not_u8 >= 0)
            verdict[i] = e->not_u8;
        else
            hipLaunchKernelGGL(check, cg, dim3(pm::kThreads), 0, s->stream, plane(i), hp.rows, hp.cols, hp.pitch, flag + i);
    }
    HIP_OK(hipGetLastError());
    std::vector<int> flags(n_planes, 1);
    HIP_OK(hipMemcpyAsync(flags.data(), flag, sizeof(int) * n_planes, hipMemcpyDeviceToHost, s->stream));
    HIP_OK(hipStreamSynchronize(s->stream));
    int not_u8 = 0;
    for (int i = 0; i < n_planes; i++) {
        if (verdict[i] < 0) {
            verdict[i] = flags[i] != 0;
            if (CachedImage *e = entry(i)) e->not_u8 = verdict[i];
        }
        not_u8 |= verdict[i];
    }
    s->u8 = !not_u8 && !(s->tune & Tune::kNoLut);
    hp.pw = s->cols + 8;
    // float-encoded window offsets need every entry index of a gray packed plane below 2^21
    hp.magic_addr = s->u8 && s->ch == 1 && !(s->tune & Tune::kNoMagicAddr) &&
                    (size_t)(s->rows + 3) * hp.pw <= (size_t)pm::kMagicMaxWords;
    if (!s->u8) return 0;
    const size_t words = (size_t)(s->rows + 3) * hp.pw * (s->ch == 4 ? 3 : 1);
    auto pack = s->ch == 4 ? pm::pack_kernel_c4 : pm::pack_kernel;
    const dim3 pgid((hp.pw + pm::kThreads - 1) / pm::kThreads, s->rows + 3);
    for (int i = 0; i < s->n_sel; i++) {
        CachedImage *e = entry(i + 1);
        if (e) {  // (counted once per use: release_cached_images gives every one back)
            e->users++;
            s->cache_refs.push_back(key(i + 1));
        }
        if (e && e->packed) {  // packed for an earlier session: shared, owned by the cache
            hp.view[i].packed = e->packed;
            continue;
        }
        uint32_t *pk = nullptr;
        if (e) {
            HIP_OK(hipMalloc(&pk, words * sizeof(uint32_t)));
            e->packed = pk;
            fresh.push_back(e);
        } else if (const int rc = s->alloc({&pk, words * sizeof(uint32_t)})) {
            return rc;
        }
        hp.view[i].packed = pk;
        hipLaunchKernelGGL(pack, pgid, dim3(pm::kThreads), 0, s->stream, hp.view[i].img, hp.rows, hp.cols, hp.pitch, hp.pw, pk);
    }
    HIP_OK(hipGetLastError());
    if (cached) HIP_OK(hipStreamSynchronize(s->stream));  // other sessions' streams may read them next
    return 0;
}

// The image cache is locked while this call looks at / adds entries; a failure first takes back the packed planes this call
// put into the cache (never verified; once packed and synchronised they belong to the cache), and the lock is gone when it
// returns -- release_cached_images takes the same non-recursive mutex to give the use counts back.
int classify_and_pack(Session *s, const gipuma_hip_desc *d)
{
    const bool cached = (d->flags & GIPUMA_HIP_FLAG_IMAGES_ON_DEVICE) && (d->flags & GIPUMA_HIP_FLAG_CACHE_IMAGES);
    std::unique_lock<std::mutex> lock(g_cache_mutex, std::defer_lock);
    if (cached) lock.lock();
    std::vector<CachedImage *> fresh;
    const int rc = classify_and_pack_locked(s, cached, fresh);
    if (rc)
        for (CachedImage *e : fresh) {
            (void)hipFree(e->packed);
            e->packed = nullptr;
        }
    return rc;
}

// gipuma_hip_destroy: the use counts of the cached packed views go back
void release_cached_images(Session *s)
{
    if (s->cache_refs.empty()) return;
    std::lock_guard<std::mutex> lock(g_cache_mutex);
    for (const CacheKey &k : s->cache_refs) {
        auto it = g_cache.find(k);
        if (it != g_cache.end() && it->second.users > 0) it->second.users--;
    }
    s->cache_refs.clear();
}

// gipuma_hip_cache_clear, this flavour's part (every flavour keeps its own packed planes)
int cache_clear(void)
{
    std::lock_guard<std::mutex> lock(g_cache_mutex);
    for (auto &kv : g_cache)
        if (kv.second.users > 0)
            return fail(GIPUMA_HIP_ERR_ARG, "gipuma_hip_cache_clear: a live session still reads a cached packed image; "
                                            "destroy the sessions first");
    for (auto &kv : g_cache)
        if (kv.second.packed) {
            (void)hipSetDevice(std::get<0>(kv.first));
            (void)hipFree(kv.second.packed);
        }
    g_cache.clear();
    return 0;
}

}  // namespace
