/* shim_arena.h — what every host-pointer (signature-exact) face shares: the fallback bookkeeping and the staging of one call
 * (shims.hip, shims_h264_hbd.hip: the codec DSP tables; sws_api.hip: the swscale per-line members; sws_uops.hip: the micro-op
 * function).  Internal to libffhip. */
#ifndef FFHIP_SHIM_ARENA_H
#define FFHIP_SHIM_ARENA_H

#include <atomic>
#include <mutex>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "common.h"

inline std::atomic<long> g_fallbacks;
inline void shim_note(const char *member, bool have_c)
{
    g_fallbacks++;
    if (!have_c)
        ffhip_set_error("ffhip: host face `%s` could not run on the device and displaced no C function: the call was NOT carried out", member);
}
/* answers a failed face through the displaced pointer */
#define SHIM_FB(tab, member, ...) do { const auto fn_ = __atomic_load_n(&(tab).member, __ATOMIC_RELAXED); shim_note(#member, fn_ != nullptr); \
                                       if (fn_) fn_(__VA_ARGS__); } while (0)

/* members of a context the init is about to overwrite: words of `incoming` that differ from what we install are the caller's
 * C functions (a second init of a table that already holds our faces must not make a face its own fallback) */
template <class T>
inline void fb_snapshot(T &fb, const T &incoming, const T &ours)
{
    static_assert(sizeof(T) % sizeof(void *) == 0, "a context is a table of function pointers");
    void *const *in = reinterpret_cast<void *const *>(&incoming), *const *ou = reinterpret_cast<void *const *>(&ours);
    void **f = reinterpret_cast<void **>(&fb);
    /* an init on one thread may run beside faces answering through the table on another: word-sized atomic stores (SHIM_FB loads
     * the same way), one writer at a time */
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    for (size_t i = 0; i < sizeof(T) / sizeof(void *); i++)
        if (in[i] != ou[i])
            __atomic_store_n(&f[i], in[i], __ATOMIC_RELAXED);
}

/* the staging image of one call.  A face lays its whole device block out in the current device's host bounce buffer (put / hole /
 * rect, each slot zero-filled and aligned), sends it in ONE copy (up), launches, brings it back in ONE copy (down) and commits from
 * the image.  It holds that device's arena mutex throughout, which guards both the device arena and the bounce buffer.  Slots are
 * byte offsets from the block's start: dev() turns one into a launch argument once up() has succeeded, img() reads or writes the
 * image (a pointer from img() lives until the next slot is added). */
#define DP 64 /* device row pitch of a staged rectangle */

/* a rectangle rows r0..r1 x byte columns c0..c1 around host pointer `host` (row step = stride, either sign) */
struct Rect {
    uint8_t *host;
    ptrdiff_t stride;
    int r0, r1, c0, c1;
};

struct Stage {
    std::unique_lock<std::mutex> lk;
    std::vector<uint8_t> &buf;
    size_t n = 0;
    uint8_t *base = nullptr;
    Stage() : lk(ffhip_scratch_mutex()), buf(ffhip_scratch_bounce()) {}

    size_t hole(size_t bytes, size_t align = 64)
    {
        const size_t off = (n + align - 1) / align * align;
        if (buf.size() < off + bytes)
            buf.resize(off + bytes);
        memset(buf.data() + n, 0, off + bytes - n);
        n = off + bytes;
        return off;
    }
    size_t put(const void *host, size_t bytes, size_t align = 64) /* host == nullptr: a zero slot */
    {
        const size_t off = hole(bytes, align);
        if (host && bytes)
            memcpy(buf.data() + off, host, bytes);
        return off;
    }
    /* rows x wbytes between host (row step hstride, either sign) and the image at `off` (row step pitch); put2d() adds the slot */
    size_t put2d(const void *host, ptrdiff_t hstride, size_t wbytes, int rows, size_t pitch)
    {
        const size_t off = hole((size_t)rows * pitch);
        put2d_at(off, pitch, host, hstride, wbytes, rows);
        return off;
    }
    void put2d_at(size_t off, size_t pitch, const void *host, ptrdiff_t hstride, size_t wbytes, int rows)
    {
        for (int y = 0; y < rows; y++)
            memcpy(buf.data() + off + y * pitch, static_cast<const uint8_t *>(host) + y * hstride, wbytes);
    }
    void get2d(void *host, ptrdiff_t hstride, size_t off, size_t pitch, size_t wbytes, int rows) const
    {
        for (int y = 0; y < rows; y++)
            memcpy(static_cast<uint8_t *>(host) + y * hstride, buf.data() + off + y * pitch, wbytes);
    }
    /* a slot for `r` at pitch DP with one spare row either side; returns the offset of the host pointer's sample (r0, c0 sits one row
     * into the slot).  rect() also stages the rectangle, fill() stages a smaller one into an area with the same origin. */
    ptrdiff_t area(const Rect &r) { return (ptrdiff_t)hole((size_t)(r.r1 - r.r0 + 3) * DP) + DP - (ptrdiff_t)r.r0 * DP - r.c0; }
    void fill(const Rect &r, ptrdiff_t org)
    {
        put2d_at(org + (ptrdiff_t)r.r0 * DP + r.c0, DP, r.host + r.r0 * r.stride + r.c0, r.stride, r.c1 - r.c0 + 1, r.r1 - r.r0 + 1);
    }
    ptrdiff_t rect(const Rect &r)
    {
        const ptrdiff_t org = area(r);
        fill(r, org);
        return org;
    }
    void commit(const Rect &r, ptrdiff_t org) const
    {
        get2d(r.host + r.r0 * r.stride + r.c0, r.stride, org + (ptrdiff_t)r.r0 * DP + r.c0, DP, r.c1 - r.c0 + 1, r.r1 - r.r0 + 1);
    }

    bool up()
    {
        const char *ef = FFHIP_KNOB("FFHIP_FAULT"); /* test hook: every face reports failure before it writes host memory */
        void *p = nullptr;
        if ((ef && ef[0] == '1') || ffhip_scratch_reserve(n, &p) < 0)
            return false;
        base = static_cast<uint8_t *>(p);
        return hipMemcpy(base, buf.data(), n, hipMemcpyHostToDevice) == hipSuccess;
    }
    bool down() { return hipStreamSynchronize(0) == hipSuccess && hipMemcpy(buf.data(), base, n, hipMemcpyDeviceToHost) == hipSuccess; }
    template <class T = uint8_t> T *dev(ptrdiff_t off) const { return reinterpret_cast<T *>(base + off); }
    template <class T = uint8_t> T *img(ptrdiff_t off) { return reinterpret_cast<T *>(buf.data() + off); }
};


#endif
