/* tx_host.h — host side shared by the av_tx files (tx_api.hip, kernels/tx_wide.hip, kernels/tx_radix.hip): the split-radix network's
 * tables, the one-allocation table blob and the launch-grid rule of the LDS-bound kernels */
#ifndef FFHIP_TX_HOST_H
#define FFHIP_TX_HOST_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#include "common.h"

/*
 * LDS layout of the complex work array: element i lives at i + (i >> 5), one pad element per 32 (= per 256-byte row
 * of the 64 LDS banks).  Every power-of-two operand stride of the split-radix levels then falls on distinct banks for
 * the 32 lanes an 8-byte access serves per cycle; with the plain layout the low levels (operands of neighbouring
 * lanes 32..512 bytes apart) serialised 4-16 ways.  The butterfly lists and the forward scatter map carry padded
 * indices from the host; a level's operand offsets k*q pad independently (no carry across bit 5: blocks are 4q
 * aligned).
 */
#define TX_PAD(i) ((i) + ((i) >> 5))

/* split_radix_permutation, libavutil/tx.c:125-135 */
static inline int sr_perm(int i, int len, int inv)
{
    len >>= 1;
    if (len <= 1)
        return i & 1;
    if (!(i & len))
        return sr_perm(i, len, inv) * 2;
    len >>= 1;
    return sr_perm(i, len, inv) * 4 + 1 - 2 * (!(i & len) ^ inv);
}

/* the reference recursion FFT(n) = FFT(n/2) + 2 x FFT(n/4) + combine(n), flattened: the size-2 blocks into b2, the combines of
 * level l into lev[l] (a0 | k << 16, padded) */
static inline void sr_schedule(int o, int n, int lg, std::vector<uint32_t> *lev, std::vector<uint16_t> *b2)
{
    if (n == 1)
        return;
    if (n == 2) {
        b2->push_back((uint16_t)TX_PAD(o));
        return;
    }
    const int q = n >> 2;
    sr_schedule(o, n >> 1, lg - 1, lev, b2);
    sr_schedule(o + 2 * q, q, lg - 2, lev, b2);
    sr_schedule(o + 3 * q, q, lg - 2, lev, b2);
    for (int k = 0; k < q; k++)
        lev[lg].push_back((uint32_t)TX_PAD(o + k) | ((uint32_t)k << 16));
}

/*
 * The level tables of nsub split-radix networks of 2^lg points each, the i-th at work-array offset i << lg: per level l = 2..lg the
 * cosine table cos(2 pi i / 2^l), i < 2^l / 4, then an exact 0 (ff_tx_init_tab_<m>, tx_template.c:69-79), each value through
 * `tab` (the sample type's conversion of a double), and the butterfly lists of all networks, concatenated per level.  Fills the
 * level fields and nblocks2 of `d` (TxDev / TxwDev); returns the longest list of a level.
 */
template <typename T, class D, class Tab>
static int tx_sr_levels(D &d, int lg, int nsub, std::vector<T> &cosv, std::vector<uint32_t> &sched, std::vector<uint16_t> &b2, Tab tab)
{
    for (int l = 2; l <= lg; l++) {
        const int m = 1 << l;
        const double freq = 2 * M_PI / m;
        d.cos_off[l] = (int)cosv.size();
        for (int i = 0; i < m / 4; i++)
            cosv.push_back(tab(cos(i * freq)));
        cosv.push_back(T(0));
    }
    std::vector<uint32_t> lev[20];
    for (int i = 0; i < nsub; i++)
        sr_schedule(i << lg, 1 << lg, lg, lev, &b2);
    int max_cnt = 0;
    for (int l = 2; l <= lg; l++) {
        d.sched_off[l] = (int)sched.size();
        d.sched_cnt[l] = (int)lev[l].size();
        sched.insert(sched.end(), lev[l].begin(), lev[l].end());
        max_cnt = d.sched_cnt[l] > max_cnt ? d.sched_cnt[l] : max_cnt;
    }
    d.nblocks2 = (int)b2.size();
    return max_cnt;
}

/* a context's tables in one device allocation: the parts at 16-byte offsets of one zero-filled image that ends in 16 zero bytes */
struct TxBlob {
    std::vector<uint8_t> img;
    template <typename V>
    size_t add(const std::vector<V> &v)
    {
        const size_t o = img.size(), bytes = v.size() * sizeof(V);
        img.resize((o + bytes + 15) & ~(size_t)15, 0);
        if (bytes)
            memcpy(img.data() + o, v.data(), bytes);
        return o;
    }
    /* one hipMalloc and one hipMemcpy; *dev is left for the caller to free if the copy fails */
    int upload(void **dev, size_t *bytes)
    {
        img.resize(img.size() + 16, 0);
        if (hipMalloc(dev, img.size()) != hipSuccess || hipMemcpy(*dev, img.data(), img.size(), hipMemcpyHostToDevice) != hipSuccess) {
            ffhip_set_error("ffhip_tx_init: table upload failed");
            return FFHIP_ENOMEM;
        }
        if (bytes)
            *bytes = img.size();
        return 0;
    }
};

/* workgroups of `waves` waves and lds_bytes of LDS each for `units` workgroups' worth of work: as many as fit the CUs at once (160 KiB
 * of LDS in 1280-byte granules, at most 32 waves per CU), at least one per CU, no more than the work */
static inline int tx_blocks(size_t lds_bytes, int waves, int units)
{
    int per_cu = (int)((160 * 1024) / (((lds_bytes + 1279) / 1280) * 1280));
    if (per_cu * waves > 32) per_cu = 32 / waves;
    if (per_cu < 1) per_cu = 1;
    const int cap = ffhip_cu_count() * per_cu;
    return units < cap ? units : cap;
}

#endif
