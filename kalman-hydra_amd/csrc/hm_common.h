// Shared host-side helpers of libhydra_mi.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <unordered_map>
#include <vector>
#include "../../include/hydra_mi.h"

void hm_set_error(const char *fmt, ...);

#define HM_HIP(expr)                                                                  \
    do {                                                                              \
        hipError_t _e = (expr);                                                       \
        if (_e != hipSuccess) {                                                       \
            hm_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),       \
                         __FILE__, __LINE__);                                         \
            return HM_ERR_HIP;                                                        \
        }                                                                             \
    } while (0)

#define HM_ARG(cond, ...)                \
    do {                                 \
        if (!(cond)) {                   \
            hm_set_error(__VA_ARGS__);   \
            return HM_ERR_ARG;           \
        }                                \
    } while (0)

// return a failed call's code (the callee has set the error)
#define HM_TRY(...)                      \
    do {                                 \
        const int _r = (__VA_ARGS__);    \
        if (_r) return _r;               \
    } while (0)

static inline int hm_cdiv(int a, int b) { return (a + b - 1) / b; }

// Every device allocation of the library.  HYDRA_MI_POISON=<mask> (development aid) fills those of the classes in the
// mask -- 1 the filter's context, 2 a flow handle, 4 hm_dev_alloc (the caller's buffers: frame ring, flow planes) --
// with 0xFF bytes: NaNs as floating point, -1 as integers, so that a kernel that reads memory nobody has written shows
// at once and every time, not only when the allocator hands back a block an earlier handle left its numbers in.
#ifndef HM_ALLOC_CLASS
#define HM_ALLOC_CLASS 1
#endif
static inline hipError_t hm_malloc(void **p, size_t bytes, int cls = HM_ALLOC_CLASS)
{
    static const int poison = getenv("HYDRA_MI_POISON") ? atoi(getenv("HYDRA_MI_POISON")) : 0;
    // HYDRA_MI_POISON_ONLY=k: of the allocations of those classes (counted per translation unit, from 0) only the k-th
    // -- to find the buffer a failure under HYDRA_MI_POISON comes from
    static const int only = getenv("HYDRA_MI_POISON_ONLY") ? atoi(getenv("HYDRA_MI_POISON_ONLY")) : -1;
    static int count = 0;
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess && (poison & cls)) {
        const int k = count++;
        if (only < 0 || only == k) {
            e = hipMemset(*p, 0xFF, bytes);
            if (e == hipSuccess) e = hipDeviceSynchronize();      // before anything a non-blocking stream writes there
        }
        if (only == k) fprintf(stderr, "[hydra_mi] poisoned allocation %d: %zu bytes\n", k, bytes);
    }
    return e;
}

// The GPU resources of one native handle (hm_ctx, hm_brox): every device allocation, page-locked host allocation, stream
// and event the handle creates is recorded here, and release() frees them all.  Allocations are recorded by address, not
// by field: the handles swap and alias their pointers (render targets, state buffers, the resident covariance, the
// pool's area), and the kernel-argument structs hold them raw -- whichever field holds an address, it is freed once.
// The calls that create are idempotent on the field they fill: a non-null field is left as it is (alloc, host_alloc,
// stream, event) or kept while its allocation is large enough (grow, host_grow), so a lazily built group of resources
// can simply be built again after a failure part-way.
// No lock: one thread at a time uses a handle's owner.  For the filter handle that is the caller's thread, or the helper
// thread while it queues an update's tail (which grows the spring arrays and builds the projection buffers); every entry
// point that creates anything waits for the helper first (ctx_join), and hm_update_arm_* and the prefactor worker, which
// do not wait, create nothing.
namespace {
struct HmOwner {
    struct Mem { size_t bytes; bool host; };
    int cls;                                   // the HYDRA_MI_POISON class of the device allocations (hm_malloc)
    std::unordered_map<void *, Mem> mem;
    std::vector<hipEvent_t> events;
    std::vector<hipStream_t> streams;

    explicit HmOwner(int cls) : cls(cls) {}
    HmOwner(const HmOwner &) = delete;
    HmOwner &operator=(const HmOwner &) = delete;

    template <typename T> hipError_t alloc(T **p, size_t bytes) { return *p ? hipSuccess : grow(p, bytes); }
    template <typename T> hipError_t grow(T **p, size_t bytes) { return take((void **)p, bytes, false, 0); }
    template <typename T> hipError_t host_alloc(T **p, size_t bytes, unsigned flags)
    {
        return *p ? hipSuccess : host_grow(p, bytes, flags);
    }
    template <typename T> hipError_t host_grow(T **p, size_t bytes, unsigned flags) { return take((void **)p, bytes, true, flags); }
    // a non-blocking stream, at the device's greatest priority when it offers a range of them and `greatest` is set
    hipError_t stream(hipStream_t *s, bool greatest = true)
    {
        if (*s) return hipSuccess;
        int least = 0, most = 0;
        hipError_t e = greatest ? hipDeviceGetStreamPriorityRange(&least, &most) : hipSuccess;
        if (e == hipSuccess)
            e = greatest && most != least ? hipStreamCreateWithPriority(s, hipStreamNonBlocking, most)
                                          : hipStreamCreateWithFlags(s, hipStreamNonBlocking);
        return keep(streams, s, e);
    }
    // a stream on the compute units of `mask` (hipExtStreamCreateWithCUMask)
    hipError_t cu_stream(hipStream_t *s, const std::vector<uint32_t> &mask)
    {
        if (*s) return hipSuccess;
        return keep(streams, s, hipExtStreamCreateWithCUMask(s, (uint32_t)mask.size(), mask.data()));
    }
    hipError_t event(hipEvent_t *ev, unsigned flags = hipEventDisableTiming)
    {
        if (*ev) return hipSuccess;
        return keep(events, ev, hipEventCreateWithFlags(ev, flags));
    }
    // frees one allocation of the handle and clears the field (the caller has waited for its last use)
    template <typename T> hipError_t free(T **p)
    {
        const auto it = *p ? mem.find((void *)*p) : mem.end();
        if (it == mem.end()) return hipSuccess;
        const hipError_t e = it->second.host ? hipHostFree(it->first) : hipFree(it->first);
        mem.erase(it);
        *p = nullptr;
        return e;
    }
    // destroys one stream of the handle and clears the field
    hipError_t release(hipStream_t *s)
    {
        for (size_t i = 0; i < streams.size(); i++)
            if (streams[i] == *s) {
                streams.erase(streams.begin() + i);
                const hipError_t e = hipStreamDestroy(*s);
                *s = nullptr;
                return e;
            }
        return hipSuccess;
    }
    // waits for every stream of the handle
    void drain()
    {
        for (hipStream_t s : streams) (void)hipStreamSynchronize(s);
    }
    // everything: memory first, then events, then streams (the streams must be idle)
    void release()
    {
        for (const auto &m : mem) (void)(m.second.host ? hipHostFree(m.first) : hipFree(m.first));
        for (hipEvent_t ev : events) (void)hipEventDestroy(ev);
        for (hipStream_t s : streams) (void)hipStreamDestroy(s);
        mem.clear(); events.clear(); streams.clear();
    }

  private:
    hipError_t take(void **p, size_t bytes, bool host, unsigned flags)
    {
        const auto it = *p ? mem.find(*p) : mem.end();
        if (bytes <= (it != mem.end() ? it->second.bytes : 0)) return hipSuccess;
        if (it != mem.end()) {
            (void)(it->second.host ? hipHostFree(*p) : hipFree(*p));
            mem.erase(it);
        }
        *p = nullptr;
        const hipError_t e = host ? hipHostMalloc(p, bytes, flags) : hm_malloc(p, bytes, cls);
        if (*p) mem[*p] = Mem{bytes, host};   // (also when hm_malloc's poison fill failed: it is freed with the rest)
        return e;
    }
    template <typename H> static hipError_t keep(std::vector<H> &list, H *x, hipError_t e)
    {
        if (e == hipSuccess) list.push_back(*x);
        else *x = nullptr;
        return e;
    }
};
}  // namespace
