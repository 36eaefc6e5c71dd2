/* picture_check.h — what every whole-picture face (*_pictures_dev, *_frames_dev) checks on the host before it launches: the common
 * arguments, the planes' geometry, and that nothing the call writes is read or written elsewhere in the call.  Host only, included
 * by the shim files.  Internal to libffhip. */
#ifndef FFHIP_PICTURE_CHECK_H
#define FFHIP_PICTURE_CHECK_H

#include <algorithm>
#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "ffhip_internal.h"

/* ---- spans: the bytes [lo, hi) a plane, a map or a range occupies ---------------------------------------- */
struct FFHipSpan {
    uintptr_t lo, hi;
};
/* `rows` rows of `w_bytes` bytes, `stride` bytes apart (a range: one row) */
inline FFHipSpan ffhip_plane_span(const void *base, ptrdiff_t stride, ptrdiff_t w_bytes, int rows)
{
    const uintptr_t b = (uintptr_t)base;
    return { b, b + (uintptr_t)((ptrdiff_t)(rows - 1) * stride + w_bytes) };
}
/* a map of `rows` rows of `w` entries of `entry` bytes, `stride` entries apart, from its first to its last entry */
inline FFHipSpan ffhip_map_span(const void *base, int stride, int w, int rows, size_t entry)
{
    return ffhip_plane_span(base, (ptrdiff_t)stride * (ptrdiff_t)entry, (ptrdiff_t)w * (ptrdiff_t)entry, rows);
}

/* A set of spans that answers "do two members share a byte?" (seal) and "does this span share a byte with a member?" (hits).
 * Empty spans overlap nothing: add() drops them and hits() is false for them. */
class FFHipSpanSet {
public:
    void reserve(size_t n) { v.reserve(n); }
    void add(FFHipSpan s)
    {
        if (s.lo != s.hi)
            v.push_back(s);
    }
    /* after the last add(): sorts by start and turns each end into the largest end so far, so that hits() is one binary search.
     * Returns whether two members share a byte; a face that allows that ignores the answer */
    bool seal()
    {
        std::sort(v.begin(), v.end(), [](const FFHipSpan &x, const FFHipSpan &y) { return x.lo < y.lo; });
        bool shared = false;
        for (size_t k = 1; k < v.size(); k++) {
            shared |= v[k - 1].hi > v[k].lo;
            v[k].hi = std::max(v[k].hi, v[k - 1].hi);
        }
        return shared;
    }
    /* the members that start before s ends: one of them overlaps s iff the largest end among them is past s.lo */
    bool hits(FFHipSpan s) const
    {
        if (s.lo == s.hi)
            return false;
        const size_t n = (size_t)(std::lower_bound(v.begin(), v.end(), s.hi, [](const FFHipSpan &x, uintptr_t e) { return x.lo < e; }) - v.begin());
        return n && v[n - 1].hi > s.lo;
    }

private:
    std::vector<FFHipSpan> v;
};

/* ---- rows: where two planes may interleave (the two fields of a frame) a span says too little ------------- */
/* `rows` rows of `row_bytes` bytes, `stride` bytes (of any sign) apart */
struct FFHipRows {
    uintptr_t base;
    ptrdiff_t stride, row_bytes;
    int rows;
    FFHipSpan span() const
    {
        const uintptr_t last = base + (uintptr_t)((ptrdiff_t)(rows - 1) * stride);
        return { std::min(base, last), std::max(base, last) + (uintptr_t)row_bytes };
    }
};
/* Does a row of `a` share a byte with a row of `b`?  Disjoint spans: no.  Equal strides s: the rows of both lie on one lattice of
 * pitch |s|; with d = (b.base - a.base) mod |s| they are disjoint iff d >= a.row_bytes and d + b.row_bytes <= |s| (the two fields of a
 * frame).  Overlapping spans with unequal strides count as shared. */
inline bool ffhip_rows_share(const FFHipRows &a, const FFHipRows &b)
{
    const FFHipSpan sa = a.span(), sb = b.span();
    if (sa.hi <= sb.lo || sb.hi <= sa.lo)
        return false;
    if (a.stride != b.stride || a.stride == 0)
        return true;
    const uintptr_t s = (uintptr_t)(a.stride < 0 ? -a.stride : a.stride);
    const uintptr_t d = (b.base >= a.base ? (b.base - a.base) % s : (s - (a.base - b.base) % s) % s);
    return !(d >= (uintptr_t)a.row_bytes && d + (uintptr_t)b.row_bytes <= s);
}
/* Do two of the destination planes share a byte of a row?  The span set sorts out the calls whose spans are disjoint before the
 * pairwise rule; `out` is left sealed over the planes' spans for the caller's hits() */
inline bool ffhip_any_rows_share(const std::vector<FFHipRows> &dst, FFHipSpanSet &out)
{
    out.reserve(dst.size());
    for (const FFHipRows &d : dst)
        out.add(d.span());
    if (out.seal())
        for (size_t a = 0; a < dst.size(); a++)
            for (size_t b = a + 1; b < dst.size(); b++)
                if (ffhip_rows_share(dst[a], dst[b]))
                    return true;
    return false;
}

/* ---- the arguments the faces share: `who` names the face in the message; 0 or FFHIP_EINVAL ---------------- */
inline int ffhip_check_count(const char *who, int npics, const void *pics, const char *what /* "picture" or "frame" */)
{
    if (npics <= 0 || !pics) {
        ffhip_set_error("%s: npics = %d, or a NULL %s array", who, npics, what);
        return FFHIP_EINVAL;
    }
    return 0;
}
inline int ffhip_check_hevc_format(const char *who, int bit_depth, int chroma_format_idc)
{
    if ((bit_depth != 8 && bit_depth != 10 && bit_depth != 12) || chroma_format_idc < 0 || chroma_format_idc > 3) {
        ffhip_set_error("%s: bit depth %d (8, 10 or 12), chroma format %d (0..3)", who, bit_depth, chroma_format_idc);
        return FFHIP_EINVAL;
    }
    return 0;
}
/* the CTB size, then the picture size, then the picture array: all a face without samples (boundary strengths) has */
inline int ffhip_check_hevc_geometry(const char *who, int log2_ctb_size, int width, int height, int npics, const void *pics)
{
    if (log2_ctb_size < 4 || log2_ctb_size > 6) {
        ffhip_set_error("%s: log2 CTB size %d (4..6)", who, log2_ctb_size);
        return FFHIP_EINVAL;
    }
    if (width <= 0 || height <= 0 || width > 65535 || height > 65535 || (width | height) & 7) {
        ffhip_set_error("%s: picture size %d x %d (multiples of 8, at most 65535)", who, width, height);
        return FFHIP_EINVAL;
    }
    return ffhip_check_count(who, npics, pics, "picture");
}
inline int ffhip_check_hevc_pictures(const char *who, int bit_depth, int chroma_format_idc, int log2_ctb_size, int width, int height, int npics,
                                     const void *pics)
{
    const int r = ffhip_check_hevc_format(who, bit_depth, chroma_format_idc);
    return r < 0 ? r : ffhip_check_hevc_geometry(who, log2_ctb_size, width, height, npics, pics);
}
inline int ffhip_check_vp9_frames(const char *who, int bit_depth, int ss_h, int ss_v, int width, int height, int npics, const void *pics)
{
    if ((bit_depth != 8 && bit_depth != 10 && bit_depth != 12) || (ss_h & ~1) || (ss_v & ~1)) {
        ffhip_set_error("%s: bit depth %d (8, 10 or 12), subsampling %d, %d (0 or 1 each)", who, bit_depth, ss_h, ss_v);
        return FFHIP_EINVAL;
    }
    if (width <= 0 || height <= 0 || width > 65535 || height > 65535) {
        ffhip_set_error("%s: frame size %d x %d (1..65535)", who, width, height);
        return FFHIP_EINVAL;
    }
    return ffhip_check_count(who, npics, pics, "frame");
}

/* ---- the planes of a call, filled once ------------------------------------------------------------------ */
struct FFHipPlaneGeom {
    int ps;         /* bytes per sample */
    unsigned amask; /* the kernels access four samples at a time: bases and strides of planes they write are amask-aligned */
    int nplanes;
    int pw[3], ph[3]; /* the planes' sizes, samples */

    static FFHipPlaneGeom hevc(int bit_depth, int chroma_format_idc, int width, int height)
    {
        FFHipPlaneGeom g = of_depth(bit_depth, chroma_format_idc ? 3 : 1);
        for (int p = 0; p < 3; p++) {
            g.pw[p] = p && chroma_format_idc != 3 ? width >> 1 : width;
            g.ph[p] = p && chroma_format_idc == 1 ? height >> 1 : height;
        }
        return g;
    }
    /* VP9 decodes whole 8 x 8 blocks: the planes' sizes are those of the decoded area */
    static FFHipPlaneGeom vp9(int bit_depth, int ss_h, int ss_v, int width, int height)
    {
        FFHipPlaneGeom g = of_depth(bit_depth, 3);
        for (int p = 0; p < 3; p++) {
            g.pw[p] = (((width + 7) >> 3) * 8) >> (p ? ss_h : 0);
            g.ph[p] = (((height + 7) >> 3) * 8) >> (p ? ss_v : 0);
        }
        return g;
    }
    ptrdiff_t row_bytes(int p) const { return (ptrdiff_t)pw[p] * ps; }
    FFHipSpan span(const void *base, ptrdiff_t stride, int p) const { return ffhip_plane_span(base, stride, row_bytes(p), ph[p]); }

private:
    static FFHipPlaneGeom of_depth(int bit_depth, int nplanes)
    {
        FFHipPlaneGeom g = {};
        g.ps = bit_depth > 8 ? 2 : 1;
        g.amask = 4u * g.ps - 1;
        g.nplanes = nplanes;
        return g;
    }
};

/* base non-NULL, base and stride amask-aligned, stride at least min_stride bytes */
inline bool ffhip_plane_ok(const void *base, ptrdiff_t stride, unsigned amask, ptrdiff_t min_stride)
{
    return base && !(((uintptr_t)base | (size_t)stride) & amask) && stride >= min_stride;
}

#endif
