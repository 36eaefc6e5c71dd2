/*
 * me_interp.hip — k_me_interp<MB, SCD>: vf_minterpolate's motion-compensated interpolation (mci / bidir / obmc) of every job of a call in
 * one launch, and its scene-change fallback, the blend.  The rule is kernels/me_interp_rules.h; include/ffhip.h states it.  The SCD
 * instance serves ffhip_me_interp_sequence_scd_dev(): an MCI job whose pair is flagged in device memory takes the streaming branch.
 *
 * The reference scatters blocks into per-pixel lists; here a pixel gathers.  One workgroup (4 waves) owns a tile of MEI_TW x MEI_TH =
 * 64 x 4 luma pixels of one job, one lane per pixel — a wave takes 16 x 4 of them, so that few windows touch a wave and most of its
 * lanes lie under each that does (the blend, which walks nothing, takes a row of 64 per wave) — plus the chroma samples whose luma site
 * lies in the tile: a site's lane feeds its two chroma sums from the same walk, since the chroma samples use the site's list.
 *   1. The workgroup stages the window table and the packed relative vectors of the candidate blocks of both directions in LDS
 *      (mei_candidates() of the tile: at mb 16, mv_range 32 at most 10 x 7 blocks per direction, 560 bytes beside the 1 KB table).
 *      A malformed vector is staged as MEI_BAD.
 *   2. A wave takes the candidates 64 at a time in (dir, by, bx) order: lane l forms the window of candidate c0 + l and tests it
 *      against the wave's 16 x 4 pixels, a ballot collects the survivors (about seven per direction for typical fields), and the wave walks
 *      the set bits from the lowest, which is the reference's order.  A survivor's window travels by v_readlane, so everything about
 *      it is scalar.
 *   3. Per lane mei_contribute(): the window weight from LDS, the cap, the displacement clips, two bytes gathered per plane.
 * k_me_interp_bilat<MB, SCD> (the BILAT instance) serves ffhip_me_interp_bilat_sequence_dev(): steps 1 and 2 fall away — a lane reads
 * the vectors of the at most four blocks whose unshifted windows hold its pixel and runs step 3 on them (mei_walk_bilat()).
 * There is no wait between workgroups, no atomic and no hand-off.  Every read is inside its plane: fields are read at blocks of
 * [0, b_w) x [0, b_h) only, and the displacement clips keep x + dx in [0, W - 1], y + dy in [0, H - 1] (chroma: see mei_site()).
 *
 * Widths: a weight is w * (1024 - alpha) or w * alpha, so a contribution adds 1024 * w <= 261120 to Wt and at most 255 times that to
 * S; with the cap of 16, Wt < 2^22 and S < 2^30.  uint32_t holds both and S + (Wt >> 1); the divide is one 32-bit unsigned divide.
 */
#include <algorithm>
#include <limits.h>

#include "common.h"
#include "me_interp_rules.h"
#include "me_kernels.h"
#include "progress_pool.h"
#include "shim_arena.h"

#define MEI_TW 64                   /* a tile: 4 waves, one lane per luma pixel */
#define MEI_TH 4
#define MEI_WW 16                   /* a wave of the walk: 16 x 4 pixels */
#define MEI_BAD INT_MIN             /* a malformed vector among the staged ones */
#define MEI_TABLE_WINDOW 1024       /* a launch's table: the window table ((2 * 16)^2 bytes at most), then its jobs */
#define MEI_JOBS_PER_LAUNCH 1024

struct MeiParams {
    const uint8_t *src[3];
    uint8_t *dst[3];
    ptrdiff_t sstride[3], dstride[3];
    size_t sframe[3], sseq[3], dframe[3];
    const int16_t *mvf, *mvb;
    int W, H, range, nplanes, sw, sh, nseq, tiles_x, job0;
    const uint8_t *scene;           /* ffhip_me_interp_sequence_scd_dev(): pair-major flags, or NULL */
    int scene_action;
};

/* SCD: the launch has scene flags (ffhip_me_interp_sequence_scd_dev() with a non-NULL scene); without them the kernel is the one it was.
 * BILAT: the bilateral compensation of ffhip_me_interp_bilat_sequence_dev() (k_me_interp_bilat below): one field, P.mvf, of
 * half-vectors; a pixel computes the indices of the at most four blocks whose unshifted windows hold it instead of walking a staged
 * candidate list — no candidates in LDS, no ballot.  Tiles, planes, the streaming branch and the sums are the same code. */
template <int MB, bool SCD, bool BILAT = false>
__global__ __launch_bounds__(256) void k_me_interp(const MeiParams P, const uint8_t *__restrict__ table)
{
    constexpr int WIN = 4 * MB * MB;
    extern __shared__ __attribute__((aligned(16))) int mei_lds[];
    uint8_t *win = reinterpret_cast<uint8_t *>(mei_lds);
    int *cand = mei_lds + WIN / 4;

    const FFHipMeInterpJob job = reinterpret_cast<const FFHipMeInterpJob *>(table + MEI_TABLE_WINDOW)[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tx = blockIdx.x % P.tiles_x, ty = blockIdx.x / P.tiles_x;
    const int px0 = tx * MEI_TW, py0 = ty * MEI_TH;
    /* an MCI job whose pair is flagged runs the scene action in the streaming pass: one byte per workgroup, uniform like the job */
    const bool cut = SCD && job.mode == FFHIP_ME_INTERP_MCI && P.scene[(size_t)job.pair * P.nseq + job.seq];
    const bool blend = job.mode == FFHIP_ME_INTERP_BLEND || cut;       /* uniform over the workgroup */
    const int wx0 = px0 + MEI_WW * wave;                        /* the walk: wave w owns columns [wx0, wx0 + 16) of the tile's 4 rows */
    const int x = blend ? px0 + lane : wx0 + (lane & (MEI_WW - 1)), y = py0 + (blend ? wave : lane / MEI_WW);
    const bool valid = x < P.W && y < P.H;
    const bool site = valid && P.nplanes == 3 && mei_site(x, P.sw, P.W) && mei_site(y, P.sh, P.H);
    const int alpha = job.alpha, sw = P.sw, sh = P.sh;

    const uint8_t *A[3], *B[3];
    uint8_t *D[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
        if (i < P.nplanes) {
            A[i] = P.src[i] + (size_t)job.seq * P.sseq[i] + (size_t)job.pair * P.sframe[i];
            B[i] = A[i] + P.sframe[i];
            D[i] = P.dst[i] + (size_t)(P.job0 + (int)blockIdx.y) * P.dframe[i];
        } else {
            A[i] = B[i] = D[i] = nullptr;
        }
    const ptrdiff_t cpos = ((ptrdiff_t)(y >> sh)) * P.sstride[1] + (x >> sw);     /* a site's sample in planes 1 and 2 */
    const ptrdiff_t cpos2 = ((ptrdiff_t)(y >> sh)) * P.sstride[2] + (x >> sw);

    if (blend) {                                        /* the streaming pass */
        const int wb = mei_scene_alpha(cut, P.scene_action, alpha);     /* DUP: the blend at 0 or 1024 is picture A or B, exactly */
        if (valid) {
            const ptrdiff_t o = (ptrdiff_t)y * P.sstride[0] + x;
            D[0][(ptrdiff_t)y * P.dstride[0] + x] = (uint8_t)mei_blend(A[0][o], B[0][o], wb);
        }
        if (site) {
            D[1][((ptrdiff_t)(y >> sh)) * P.dstride[1] + (x >> sw)] = (uint8_t)mei_blend(A[1][cpos], B[1][cpos], wb);
            D[2][((ptrdiff_t)(y >> sh)) * P.dstride[2] + (x >> sw)] = (uint8_t)mei_blend(A[2][cpos2], B[2][cpos2], wb);
        }
        return;
    }

    const MeiGeom g = mei_geom(P.W, P.H, MB, P.range);
    const MeiRange r = mei_candidates(g, px0, min(px0 + MEI_TW, P.W), py0, min(py0 + MEI_TH, P.H));
    const int ncx = r.bx1 - r.bx0, nper = ncx * (r.by1 - r.by0), ncand = 2 * nper;

    /* ---- 1. the table and the candidates' vectors ---- */
    for (int i = tid; i < WIN / 4; i += 256)
        mei_lds[i] = reinterpret_cast<const int *>(table)[i];
    if (!BILAT) {
        const size_t field = 2 * (size_t)g.bw * g.bh * ((size_t)job.pair * P.nseq + job.seq);
        for (int c = tid; c < ncand; c += 256) {
            const int dir = c >= nper, rr = c - dir * nper, cy = rr / ncx, bx = r.bx0 + rr - cy * ncx, by = r.by0 + cy;
            const int16_t *e = (dir ? P.mvb : P.mvf) + field + 2 * ((size_t)by * g.bw + bx);
            int vx, vy;
            cand[c] = mei_vector(g, bx, by, e[0], e[1], vx, vy) ? (vx & 0xFFFF) | (int)((uint32_t)vy << 16) : MEI_BAD;
        }
    }
    __syncthreads();
    if (wx0 >= P.W)         /* the whole wave: columns right of the picture */
        return;

    /* ---- 2. and 3. the walk ---- */
    uint32_t S = 0, S1 = 0, S2 = 0, Wt = 0;
    int n = 0;
    /* the lane's own sample in every plane: an entry's sample is a displacement away */
    const ptrdiff_t pos = valid ? (ptrdiff_t)y * P.sstride[0] + x : 0;
    const uint8_t *const a0 = A[0] + pos, *const b0 = B[0] + pos;
    const uint8_t *const a1 = A[1] + (site ? cpos : 0), *const b1 = B[1] + (site ? cpos : 0);
    const uint8_t *const a2 = A[2] + (site ? cpos2 : 0), *const b2 = B[2] + (site ? cpos2 : 0);
    const ptrdiff_t s0 = P.sstride[0], s1 = P.sstride[1], s2 = P.sstride[2];
    auto take = [&](int wa, int dxa, int dya, int wb, int dxb, int dyb) {
        S += (uint32_t)wa * a0[dya * s0 + dxa] + (uint32_t)wb * b0[dyb * s0 + dxb];
        Wt += (uint32_t)(wa + wb);
        if (site) {
            const int ya = mei_tshift(dya, sh), xa = mei_tshift(dxa, sw), yb = mei_tshift(dyb, sh), xb = mei_tshift(dxb, sw);
            S1 += (uint32_t)wa * a1[ya * s1 + xa] + (uint32_t)wb * b1[yb * s1 + xb];
            S2 += (uint32_t)wa * a2[ya * s2 + xa] + (uint32_t)wb * b2[yb * s2 + xb];
        }
    };
    if (BILAT) {
        /* the four blocks in (by, bx) order, their vectors straight from the field: entries of [0, b_w) x [0, b_h) only */
        if (!valid)
            return;
        const int16_t *const field = P.mvf + 2 * (size_t)g.bw * g.bh * ((size_t)job.pair * P.nseq + job.seq);
        mei_walk_bilat(g, alpha, x, y, win, [&](int bx, int by) {
            const int16_t *e = field + 2 * ((size_t)by * g.bw + bx);
            int vx, vy;
            return mei_vector(g, bx, by, e[0], e[1], vx, vy) ? mei_block_bilat(g, bx, by, vx, vy) : mei_no_block();
        }, take, nullptr);
        D[0][(ptrdiff_t)y * P.dstride[0] + x] = (uint8_t)mei_sample(S, Wt);
        if (site) {
            D[1][((ptrdiff_t)(y >> sh)) * P.dstride[1] + (x >> sw)] = (uint8_t)mei_sample(S1, Wt);
            D[2][((ptrdiff_t)(y >> sh)) * P.dstride[2] + (x >> sw)] = (uint8_t)mei_sample(S2, Wt);
        }
        return;
    }
    const int wx1 = min(wx0 + MEI_WW, P.W), wy1 = min(py0 + MEI_TH, P.H);
    for (int c0 = 0; c0 < ncand; c0 += 64) {
        const int c = c0 + lane;
        MeiBlock b = mei_no_block();
        int dir = 0;
        if (c < ncand) {
            dir = c >= nper;
            const int rr = c - dir * nper, cy = rr / ncx, v = cand[c];
            if (v != MEI_BAD)
                b = mei_block(g, alpha, dir, r.bx0 + rr - cy * ncx, r.by0 + cy, (int16_t)(v & 0xFFFF), v >> 16);
        }
        /* the wave's pixels are [wx0, wx1) x [py0, wy1) */
        uint64_t hits = __ballot(b.y0 < b.y1 && b.y0 < wy1 && b.y1 > py0 && b.x0 < b.x1 && b.x0 < wx1 && b.x1 > wx0);
        const int xs = b.x0 | b.x1 << 16, ys = b.y0 | b.y1 << 16, vd = (b.vx & 0xFFFF) | (int)((uint32_t)b.vy << 17) | dir << 16;
        while (hits) {
            const int i = __builtin_ctzll(hits);
            hits &= hits - 1;
            const int uxs = __builtin_amdgcn_readlane(xs, i), uys = __builtin_amdgcn_readlane(ys, i), uvd = __builtin_amdgcn_readlane(vd, i);
            MeiBlock u;
            u.sx = __builtin_amdgcn_readlane(b.sx, i);
            u.sy = __builtin_amdgcn_readlane(b.sy, i);
            u.x0 = uxs & 0xFFFF;
            u.x1 = (int)((uint32_t)uxs >> 16);
            u.y0 = uys & 0xFFFF;
            u.y1 = (int)((uint32_t)uys >> 16);
            u.vx = (int16_t)(uvd & 0xFFFF);
            u.vy = uvd >> 17;
            if (valid)
                mei_contribute(g, alpha, u, (uvd >> 16) & 1, x, y, win, n, take, nullptr);
        }
    }
    if (!valid)
        return;
    if (!n)
        take(1024 - alpha, 0, 0, alpha, 0, 0);
    D[0][(ptrdiff_t)y * P.dstride[0] + x] = (uint8_t)mei_sample(S, Wt);
    if (site) {
        D[1][((ptrdiff_t)(y >> sh)) * P.dstride[1] + (x >> sw)] = (uint8_t)mei_sample(S1, Wt);
        D[2][((ptrdiff_t)(y >> sh)) * P.dstride[2] + (x >> sw)] = (uint8_t)mei_sample(S2, Wt);
    }
}

int ffhip_launch_me_interp(const FFHipMePlanes *src, const FFHipMePlanes *dst, int nplanes, int log2_chroma_w, int log2_chroma_h, int width,
                           int height, int nseq, int mb_size, int mv_range, const uint8_t *window, const int16_t *mv_fwd, const int16_t *mv_bwd,
                           const FFHipMeInterpJob *jobs, int njobs, hipStream_t stream)
{
    return ffhip_launch_me_interp_scd(src, dst, nplanes, log2_chroma_w, log2_chroma_h, width, height, nseq, mb_size, mv_range, window, mv_fwd, mv_bwd,
                                      jobs, njobs, nullptr, FFHIP_ME_SCENE_BLEND, stream);
}

/* the bilateral compensation kernel: k_me_interp with the four-block walk */
template <int MB, bool SCD>
static constexpr auto k_me_interp_bilat = k_me_interp<MB, SCD, true>;

/* every face's launcher.  bilat: mv_fwd is the one field of half-vectors, mv_bwd is not looked at */
static int me_interp_launch(bool bilat, const FFHipMePlanes *src, const FFHipMePlanes *dst, int nplanes, int log2_chroma_w, int log2_chroma_h, int width,
                            int height, int nseq, int mb_size, int mv_range, const uint8_t *window, const int16_t *mv_fwd, const int16_t *mv_bwd,
                            const FFHipMeInterpJob *jobs, int njobs, const uint8_t *scene, int scene_action, hipStream_t stream);

int ffhip_launch_me_interp_scd(const FFHipMePlanes *src, const FFHipMePlanes *dst, int nplanes, int log2_chroma_w, int log2_chroma_h, int width,
                               int height, int nseq, int mb_size, int mv_range, const uint8_t *window, const int16_t *mv_fwd, const int16_t *mv_bwd,
                               const FFHipMeInterpJob *jobs, int njobs, const uint8_t *scene, int scene_action, hipStream_t stream)
{
    return me_interp_launch(false, src, dst, nplanes, log2_chroma_w, log2_chroma_h, width, height, nseq, mb_size, mv_range, window, mv_fwd, mv_bwd, jobs,
                            njobs, scene, scene_action, stream);
}

int ffhip_launch_me_interp_bilat(const FFHipMePlanes *src, const FFHipMePlanes *dst, int nplanes, int log2_chroma_w, int log2_chroma_h, int width,
                                 int height, int nseq, int mb_size, int mv_range, const uint8_t *window, const int16_t *mv,
                                 const FFHipMeInterpJob *jobs, int njobs, const uint8_t *scene, int scene_action, hipStream_t stream)
{
    return me_interp_launch(true, src, dst, nplanes, log2_chroma_w, log2_chroma_h, width, height, nseq, mb_size, mv_range, window, mv, nullptr, jobs,
                            njobs, scene, scene_action, stream);
}

static int me_interp_launch(bool bilat, const FFHipMePlanes *src, const FFHipMePlanes *dst, int nplanes, int log2_chroma_w, int log2_chroma_h, int width,
                            int height, int nseq, int mb_size, int mv_range, const uint8_t *window, const int16_t *mv_fwd, const int16_t *mv_bwd,
                            const FFHipMeInterpJob *jobs, int njobs, const uint8_t *scene, int scene_action, hipStream_t stream)
{
    if (width <= 0 || height <= 0 || njobs <= 0)
        return 0;
    MeiParams P = {};
    for (int i = 0; i < nplanes; i++) {
        P.src[i] = src->base[i];
        P.dst[i] = dst->base[i];
        P.sstride[i] = src->stride[i];
        P.dstride[i] = dst->stride[i];
        P.sframe[i] = src->frame_pitch[i];
        P.sseq[i] = src->seq_pitch[i];
        P.dframe[i] = dst->frame_pitch[i];
    }
    P.mvf = mv_fwd;
    P.mvb = mv_bwd;
    P.scene = scene;
    P.scene_action = scene_action;
    P.W = width;
    P.H = height;
    P.range = mv_range;
    P.nplanes = nplanes;
    P.sw = log2_chroma_w;
    P.sh = log2_chroma_h;
    P.nseq = nseq;
    P.tiles_x = cdiv(width, MEI_TW);
    const unsigned tiles = (unsigned)P.tiles_x * (unsigned)cdiv(height, MEI_TH);      /* at most 512 * 8192 */
    const MeiGeom g = mei_geom(width, height, mb_size, mv_range);
    const int ncx = std::min(mei_max_candidates(g, MEI_TW), g.bw), ncy = std::min(mei_max_candidates(g, MEI_TH), g.bh);
    /* 39 KB at mb 8, mv_range 256; 1.6 KB at the defaults; the bilateral kernel stages the window table alone */
    const size_t lds = (size_t)4 * mb_size * mb_size + (bilat ? 0 : (size_t)8 * ncx * ncy);
    if (lds > 64 * 1024) {
        ffhip_set_error("ffhip_me_interp_sequence_dev: %zu bytes of LDS for the candidates of a tile", lds);
        return FFHIP_EINVAL;
    }
    /* the window table and a launch's jobs travel as one image, laid out with the arena helper and sent in a progress-pool slot: device
     * memory that is not handed out again before the launch behind it has finished (the arena itself is overwritten by the next call,
     * which may come while this one is still queued on the caller's stream).  A slot holds MEI_JOBS_PER_LAUNCH jobs: a longer call
     * is split, in stream order */
    static_assert(MEI_TABLE_WINDOW + MEI_JOBS_PER_LAUNCH * sizeof(FFHipMeInterpJob) <= FFHIP_PROGRESS_SLOT_INTS * sizeof(int), "a launch's table fits a slot");
    for (int j0 = 0; j0 < njobs; j0 += MEI_JOBS_PER_LAUNCH) {
        const int n = njobs - j0 < MEI_JOBS_PER_LAUNCH ? njobs - j0 : MEI_JOBS_PER_LAUNCH;
        Stage S;
        S.hole(MEI_TABLE_WINDOW);
        memcpy(S.img(0), window, (size_t)4 * mb_size * mb_size);
        S.put(jobs + j0, (size_t)n * sizeof(FFHipMeInterpJob), MEI_TABLE_WINDOW);
        P.job0 = j0;
        const char *const what = bilat ? "ffhip_me_interp_bilat_sequence_dev: copy or launch" : "ffhip_me_interp_sequence_dev: copy or launch";
        const int r = ffhip_progress_launch_table(stream, what, S.img(0), S.n, [&](uint8_t *table) {
            if (bilat && mb_size == 16 && scene)
                hipLaunchKernelGGL((k_me_interp_bilat<16, true>), dim3(tiles, (unsigned)n), dim3(256), lds, stream, P, table);
            else if (bilat && mb_size == 16)
                hipLaunchKernelGGL((k_me_interp_bilat<16, false>), dim3(tiles, (unsigned)n), dim3(256), lds, stream, P, table);
            else if (bilat && scene)
                hipLaunchKernelGGL((k_me_interp_bilat<8, true>), dim3(tiles, (unsigned)n), dim3(256), lds, stream, P, table);
            else if (bilat)
                hipLaunchKernelGGL((k_me_interp_bilat<8, false>), dim3(tiles, (unsigned)n), dim3(256), lds, stream, P, table);
            else if (mb_size == 16 && scene)
                hipLaunchKernelGGL((k_me_interp<16, true>), dim3(tiles, (unsigned)n), dim3(256), lds, stream, P, table);
            else if (mb_size == 16)
                hipLaunchKernelGGL((k_me_interp<16, false>), dim3(tiles, (unsigned)n), dim3(256), lds, stream, P, table);
            else if (scene)
                hipLaunchKernelGGL((k_me_interp<8, true>), dim3(tiles, (unsigned)n), dim3(256), lds, stream, P, table);
            else
                hipLaunchKernelGGL((k_me_interp<8, false>), dim3(tiles, (unsigned)n), dim3(256), lds, stream, P, table);
        });
        if (r < 0)
            return r;
    }
    return 0;
}
