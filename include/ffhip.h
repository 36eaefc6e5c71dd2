/*
 * ffhip.h — C-ABI of libffhip.so, the MI355X (gfx950) "hip" arch for FFmpeg's data-parallel DSP loops.
 *
 * This is the drop-in boundary.  Every entry point below names the reference
 * interface it stands in for (file:line relative to the FFmpeg tree).  Plain C: pointers, sizes,
 * ints.  No torch / C++ types.  INTEGRATION.md shows the few-line `ff_*_init_hip()` stubs a
 * maintainer adds on the FFmpeg side to bind these.
 *
 * Two faces per component (SURVEY.md §7 "granularity mismatch"):
 *   - signature-exact single-call shims taking HOST pointers: the reference's own function-pointer
 *     types, installable into SwsInternal / H264DSPContext / H264QpelContext / MECmpContext /
 *     FFTXCodelet and exercisable by checkasm.  They stage through device scratch and synchronise.
 *   - batched `_dev` entry points taking DEVICE pointers + a hipStream_t (as void *): the only form
 *     that can reach the HBM roofline.  Asynchronous on the given stream.
 *
 * Return convention: 0 (or a line count where the reference returns one) on success, negative
 * errno-style (== AVERROR(e) on POSIX) on failure.  FFHIP_ENOSYS when no HIP device is usable —
 * the caller keeps its C function pointer.  Nothing here silently falls back to a CPU path.
 */
#ifndef FFHIP_H
#define FFHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FFHIP_EINVAL (-22)
#define FFHIP_ENOMEM (-12)
#define FFHIP_ENOSYS (-38)
#define FFHIP_EIO    (-5)    /* a HIP runtime call failed; ffhip_last_error() has the text */

/* ------------------------------------------------------------------------------------------ */
/* runtime                                                                                    */
/* ------------------------------------------------------------------------------------------ */
/** Number of usable HIP devices (0 when none / no driver).  Mirrors the role of av_get_cpu_flags()
 *  & AV_CPU_FLAG_* gating in every ff_*_init_<arch>() (libavutil/cpu.h:32-62). */
int         ffhip_device_count(void);
/** Bind the calling thread to a device.  HIP's current device is per thread; context-free entry points (the batched `_dev`
 *  faces, the host-pointer shims) run on the calling thread's device, and their shared resources (staging arena, progress
 *  counters, coefficient tables, compiled op lists) live in per-device tables, so one process may drive every GPU of the node from
 *  as many threads as it likes — the reference's own model of one process with frame / slice threads
 *  (libavcodec/pthread_frame.c, libswscale/swscale.c:1645-1679).  May be called at any time, any number of times.
 *  The FIRST call of the process also sets the process default: a thread that never calls ffhip_set_device() (an FFmpeg worker
 *  thread calling a shim face) is bound to that default at its first entry instead of HIP's device 0.
 *  Contexts (FFHipSwsContext, FFHipTXContext, FFHipH264Picture, FFHipAacImdct, FFHipAacLd, FFHipSwsUOps) are bound to the device
 *  that was current when they were created: their calls make that device current for their own duration, whatever the calling
 *  thread is bound to.  The stream handed to a call must belong to the device the call runs on. */
int         ffhip_set_device(int device);
/** The calling thread's device (after the default binding described above), or FFHIP_ENOSYS. */
int         ffhip_get_device(void);
/** ffhip_set_device() for the duration of a callback that must leave the calling thread bound as it found it (AVBuffer pool
 *  callbacks run on whichever thread drops the last reference): push makes `device` current and stores in *prev what pop restores. */
int         ffhip_device_push(int device, int *prev);
void        ffhip_device_pop(int prev);
/** A stream on the calling thread's device (hipStreamNonBlocking), for callers without the HIP headers. */
int         ffhip_stream_create(void **stream);
int         ffhip_stream_destroy(void *stream);
/** Everything queued on `first` so far happens before anything queued on `then` from now on (an event recorded on one, waited for on
 *  the other).  Either may be NULL, the legacy default stream — which a non-blocking stream is not ordered against by itself. */
int         ffhip_stream_order(void *first, void *then);
/** Streaming-bandwidth probe of the current device (measurement aid: bench.py reports the box's achievable roofs beside
 *  the 8 TB/s spec).  pattern 0 read, 1 write, 2 copy, 3 read n/4 + write n (the 1080p->4K scaler's mix), 4 read n/2 + write n
 *  (yuv420p->rgb24's), 5 the runtime's hipMemcpyDtoDAsync.  Patterns 0-4 are a SWEEP of 24 ways to issue the same traffic (1 / 2 / 8
 *  16-byte accesses in flight per lane, plain or non-temporal, 256 x 4 or 256 x 16 workgroups, grid-stride or private XCD-adjacent
 *  slices) and answer with the best one.  `bytes` = the larger side's buffer; *gbps = bytes moved per second / 1e9 over `reps`
 *  launches of that variant (HIP events). */
int         ffhip_membw_probe(int pattern, size_t bytes, int reps, double *gbps);
/**
 * Device memory for frame batches whose rate does not depend on where the allocator happened to find it (round 6).  What a streaming
 * kernel over several gigabytes gets out of HBM depends on the PHYSICAL layout of its buffers: the same launch of the bench kernel runs at
 * 0.575 – 0.585 of HBM on one plain allocation and at 0.63 – 0.66 on the next, process by process and allocation by allocation — two
 * modes, the slow one most often on large physically contiguous blocks (the first big hipMalloc of a fresh process; 1 GiB physical chunks:
 * 7 of 12), whatever the virtual addresses (profiles/r06_alloc_vmm_sweep_*.txt, r06_arena_offset_sweep.txt).  ffhip_frames_alloc() builds
 * the range from physical chunks of `chunk` bytes (0: 16 MiB; a power of two, at least the device's allocation granularity) mapped
 * into one virtual range in a fixed pseudo-random order (HIP virtual memory management: hipMemCreate / hipMemMap), so that no large
 * piece of the range is physically contiguous: measured 0.60 – 0.645 on every one of 12 allocations where plain ones gave 0.575 – 0.66
 * (mean 0.628 against 0.610), and +3.6 % on average for the table converter.  *ptr: the range, ordinary device memory for every kernel,
 * copy and torch view of the current device; the tail of the last chunk is mapped too.  bench.py holds its frame batches in it; a caller
 * that keeps hundreds of frames resident (a transcoder's look-ahead, an inference batch) should too.
 * Returns 0, FFHIP_EINVAL, FFHIP_ENOMEM or FFHIP_ENOSYS (no virtual memory management on this device / runtime).
 */
int         ffhip_frames_alloc(void **ptr, size_t bytes, size_t chunk);
/** Unmaps and releases a range ffhip_frames_alloc() returned (NULL: nothing).  0 or FFHIP_EINVAL (not such a range). */
int         ffhip_frames_free(void *ptr);
const char *ffhip_last_error(void);
const char *ffhip_version(void);
/** Device memory helpers for callers that do not bring their own allocator. */
int         ffhip_malloc(void **dev_ptr, size_t bytes);
int         ffhip_free(void *dev_ptr);
int         ffhip_memcpy_h2d(void *dev_dst, const void *host_src, size_t bytes);
int         ffhip_memcpy_d2h(void *host_dst, const void *dev_src, size_t bytes);
/** The device ordinal `p` lives on, or FFHIP_EINVAL for host / unknown memory. */
int         ffhip_pointer_device(const void *p);
/** Pitched plane copies, asynchronous on `stream` (the transfer_data_to / _from of an AVHWFramesContext: integration/avutil_hwcontext_hip.c). */
int         ffhip_memcpy2d_h2d_async(void *dev_dst, size_t dpitch, const void *host_src, size_t spitch, size_t width_bytes, size_t rows, void *stream);
int         ffhip_memcpy2d_d2h_async(void *host_dst, size_t dpitch, const void *dev_src, size_t spitch, size_t width_bytes, size_t rows, void *stream);
/** hipStreamSynchronize; also the point where a row-ordered launch OF THIS STREAM (frame-order deblocking, intra wavefront, VP9
 *  frame loop filter) that timed out on a row hand-off (never in a correct run) is reported: FFHIP_EIO once, ffhip_last_error()
 *  has the text — its picture is only partly processed.  Other streams' pictures are not affected and not reported here. */
int         ffhip_stream_synchronize(void *stream);

/* ------------------------------------------------------------------------------------------ */
/* several GPUs in one process: device set, frame-batch scatter / gather over xGMI              */
/* ------------------------------------------------------------------------------------------ */
/* The path shards embarrassingly: a batch is cut into contiguous ranges, one per device, with no data-path
 * collective.  What the reference does with threads inside one process (frame threads, libavcodec/pthread_frame.c; slice threads,
 * libswscale/swscale.c:1645-1679; avfilter slice threading for the motion search, libavfilter/vf_minterpolate.c) a caller does here
 * with one host thread (or one loop) per member of an FFHipDeviceSet.  ffmpeg_amd/dist.py holds the one-process-per-GPU form of
 * the same partition (torch.distributed / RCCL). */
typedef struct FFHipDeviceSet FFHipDeviceSet;
/** ceil(n/world) contiguous items per rank; the last ranks may get fewer or none. */
void ffhip_shard_range(int64_t n_items, int rank, int world, int64_t *lo, int64_t *hi);
/** Motion search over a sequence: pair p searches frame p+1 in frame p.  Pairs [plo, phi) shard like everything else and read
 *  frames [flo, fhi) = [plo, phi] — the rank's own range plus ONE halo frame (empty when the rank has no pair). */
void ffhip_shard_frame_pairs(int64_t n_frames, int rank, int world, int64_t *plo, int64_t *phi, int64_t *flo, int64_t *fhi);
/** `n` devices (devices == NULL or n <= 0: all of them), one non-blocking stream each, peer access enabled between every pair
 *  that has a direct xGMI path.  A device may appear more than once (a member is a (device, stream) pair). */
int   ffhip_device_set_create(FFHipDeviceSet **s, const int *devices, int n);
void  ffhip_device_set_free(FFHipDeviceSet **s);
int   ffhip_device_set_size(const FFHipDeviceSet *s);
int   ffhip_device_set_device(const FFHipDeviceSet *s, int member);
void *ffhip_device_set_stream(const FFHipDeviceSet *s, int member);
/** ffhip_set_device(member's device) for the calling thread: a worker thread's first call. */
int   ffhip_device_set_bind(const FFHipDeviceSet *s, int member);
/** Waits for every member's stream (ffhip_stream_synchronize semantics); the first error wins. */
int   ffhip_device_set_synchronize(FFHipDeviceSet *s);
/** full[lo_i, hi_i) (items of item_bytes, on the root member's device) -> shards[i] on member i, hipMemcpyPeerAsync on member
 *  i's stream behind what the root's stream has queued.  _scatter uses ffhip_shard_range(); _ranges takes explicit, possibly
 *  overlapping ranges (halos); _frames_for_pairs the motion search's ranges.  shards[root] may point into `full` (no copy). */
int   ffhip_batch_scatter(FFHipDeviceSet *s, int root, const void *full, size_t item_bytes, int64_t n_items, void *const *shards);
int   ffhip_batch_scatter_ranges(FFHipDeviceSet *s, int root, const void *full, size_t item_bytes, int64_t n_items, const int64_t *lo,
                                 const int64_t *hi, void *const *shards);
int   ffhip_batch_scatter_frames_for_pairs(FFHipDeviceSet *s, int root, const void *frames, size_t frame_bytes, int64_t n_frames,
                                           void *const *shards);
/** The inverse: shards[i] -> full[lo_i, hi_i) on the root, each copy on member i's stream behind the work that produced the shard;
 *  the root's stream then waits for all copies (so work queued on it afterwards sees the whole batch). */
int   ffhip_batch_gather(FFHipDeviceSet *s, int root, void *full, size_t item_bytes, int64_t n_items, const void *const *shards);
int   ffhip_batch_gather_ranges(FFHipDeviceSet *s, int root, void *full, size_t item_bytes, int64_t n_items, const int64_t *lo,
                                const int64_t *hi, const void *const *shards);

/* ------------------------------------------------------------------------------------------ */
/* libswscale: hscale / vscale / yuv2rgb                                                      */
/* ------------------------------------------------------------------------------------------ */
/* Pixel formats: numeric values are AVPixelFormat's (libavutil/pixfmt.h). */
#define FFHIP_PIX_FMT_YUV420P 0
#define FFHIP_PIX_FMT_RGB24   2
#define FFHIP_PIX_FMT_BGR24   3
#define FFHIP_PIX_FMT_YUV422P 4    /* planar 4:2:2 and 4:4:4, 8 bits (== AV_PIX_FMT_YUV422P / _YUV444P): sources and targets of the scaler;
                                    * to packed RGB 4:4:4 sources run with SWS_FULL_CHR_H_INT, as in the reference (utils.c:1276-1285) */
#define FFHIP_PIX_FMT_YUV444P 5
#define FFHIP_PIX_FMT_YUVA420P 33  /* planar YUV with an alpha plane, 8 bits (== AV_PIX_FMT_YUVA420P / _YUVA422P / _YUVA444P).  As sources their
                                    * alpha plane is not read when the target has none (c->needAlpha = 0, utils.c:1398); as targets of sources
                                    * without alpha the plane dst[3] is filled with 255, as ff_swscale() fills it (swscale.c:536-553).  Alpha on
                                    * both sides: the alpha plane is scaled by the luma banks (FFHipSwsTables.dst_alpha_fill == 2) */
#define FFHIP_PIX_FMT_YUVA422P 78
#define FFHIP_PIX_FMT_YUVA444P 79
#define FFHIP_PIX_FMT_YUVJ420P 12  /* the full-range "J" twins (== AV_PIX_FMT_YUVJ420P / 422P / 444P): taken when BOTH sides are J formats —
                                    * equal ranges need no range conversion, the conversion is the base formats' (handle_jpeg(),
                                    * libswscale/utils.c:1019-1050); a J format on one side only, or J to packed RGB, is not on the hip path */
#define FFHIP_PIX_FMT_YUVJ422P 13
#define FFHIP_PIX_FMT_YUVJ444P 14
/* Above 8 bits (== AV_PIX_FMT_*; little-endian): planar yuv4xxp at 9 / 10 / 12 / 14 / 16 bits with the samples in the low bits, and
 * the semi-planar P010 / P012 / P016 with the samples in the HIGH bits.  Sources and targets of SCALED contexts on the legacy path
 * (hScale16To15_c / hScale16To19_c / hScale8To19_c, yuv2plane1 / yuv2planeX at the target depth, the P01x readers and writers:
 * libswscale/swscale.c:69-160, output.c:150-360, input.c p010LEToY_c / p010LEToUV_c), freely mixed with the 8-bit YUV formats above
 * (an 8-bit target fed from a deeper source is dithered with ff_dither_8x8_128, as swscale does: swscale.c:291,519-522).  Equal-size
 * YUV conversions take the reference's special converters (swscale_unscaled.c) and are not on the hip path.  Round 6: 9 .. 14-bit sources into
 * the packed 8-bit RGB targets (yuv2rgb_X / _2 / _1 from 16-bit lines, vscale.c:126-170) — even widths, subsampled sources, banks of at
 * most 16 taps; not the full-chroma writers.
 * Packed 8-bit RGB as a SOURCE (round 6): rgb24, bgr24, argb, rgba, abgr, bgra into any YUV target above — the input converters
 * (libswscale/input.c:264-400,1068-1190) run as a kernel and the context is the one of their 14-bit lines (ffhip_sws_from_tables_rgb_source);
 * not into full-range (J) or alpha-carrying targets from an alpha source, not RGB -> RGB, and bgr24 -> yuv420p at the source's size is the
 * reference's own special converter. */
#define FFHIP_PIX_FMT_YUV420P16LE 45
#define FFHIP_PIX_FMT_YUV422P16LE 47
#define FFHIP_PIX_FMT_YUV444P16LE 49
#define FFHIP_PIX_FMT_YUV420P9LE  60
#define FFHIP_PIX_FMT_YUV420P10LE 62
#define FFHIP_PIX_FMT_YUV422P10LE 64
#define FFHIP_PIX_FMT_YUV444P9LE  66
#define FFHIP_PIX_FMT_YUV444P10LE 68
#define FFHIP_PIX_FMT_YUV422P9LE  70
#define FFHIP_PIX_FMT_YUV420P12LE 123
#define FFHIP_PIX_FMT_YUV420P14LE 125
#define FFHIP_PIX_FMT_YUV422P12LE 127
#define FFHIP_PIX_FMT_YUV422P14LE 129
#define FFHIP_PIX_FMT_YUV444P12LE 131
#define FFHIP_PIX_FMT_YUV444P14LE 133
#define FFHIP_PIX_FMT_P010LE      158
#define FFHIP_PIX_FMT_P016LE      169
#define FFHIP_PIX_FMT_P012LE      209
#define FFHIP_PIX_FMT_NV12    23
#define FFHIP_PIX_FMT_NV21    24
#define FFHIP_PIX_FMT_ARGB    25   /* packed 8:8:8:8; alpha = 255 (the sources on this path carry none) */
#define FFHIP_PIX_FMT_RGBA    26
#define FFHIP_PIX_FMT_ABGR    27
#define FFHIP_PIX_FMT_BGRA    28
#define FFHIP_PIX_FMT_GBRP    71   /* planar G, B, R (== AV_PIX_FMT_GBRP): a target of the equal-size table converter only (yuv420p_gbrp_c /
                                    * yuv422p_gbrp_c, libswscale/yuv2rgb.c:533,553) */
/* The equal-size table converter (ff_yuv2rgb_get_func_ptr(), libswscale/yuv2rgb.c:562-676; chosen at swscale_unscaled.c:2425-2431 when
 * the sizes are equal, SWS_ACCURATE_RND is off and the height is even) takes yuv420p, yuv422p (each luma row with the chroma row of its
 * own, YUV422FUNC) and yuva420p sources; the alpha plane of the latter drives the alpha byte of the four 32-bit targets (yuva2rgba_c /
 * yuva2argb_c) and is not read for the others.  Targets: rgb24, bgr24, argb, rgba, abgr, bgra, gbrp; even widths (an odd width is the C
 * converter's tail case and stays there). */
/* Flags: numeric values are SwsFlags' (libswscale/swscale.h:130-153). */
#define FFHIP_SWS_FULL_CHR_H_INT 0x2000 /* full chroma interpolation for packed RGB targets (swscale.h:147) */
#define FFHIP_SWS_FULL_CHR_H_INP 0x4000 /* full chroma input from a packed RGB source (swscale.h:153): no horizontal 2:1 in the converters */
#define FFHIP_SWS_FAST_BILINEAR 0x1
#define FFHIP_SWS_BILINEAR      0x2
#define FFHIP_SWS_BICUBIC       0x4
#define FFHIP_SWS_POINT         0x10
#define FFHIP_SWS_AREA          0x20
#define FFHIP_SWS_BICUBLIN      0x40
#define FFHIP_SWS_GAUSS         0x80
#define FFHIP_SWS_SINC          0x100
#define FFHIP_SWS_LANCZOS       0x200
#define FFHIP_SWS_ACCURATE_RND  0x40000
#define FFHIP_SWS_BITEXACT      0x80000

/**
 * One separable filter bank as the reference's initFilter() produces it
 * (libswscale/utils.c:197-612): `filter[n][size]` int16 coefficients, `pos[n]` first source sample.
 * Horizontal banks sum to ~1<<14, vertical to 1<<12.
 */
typedef struct FFHipSwsFilter {
    const int16_t *filter;
    const int32_t *pos;
    int            size;   /* taps per output sample  (SwsInternal.hLumFilterSize ...) */
    int            n;      /* number of output samples (dstW, chrDstW, dstH, chrDstH)  */
} FFHipSwsFilter;

/**
 * What ff_sws_init_swscale_hip(SwsInternal *c) hands over: the context fields the hot path reads
 * (libswscale/swscale_internal.h:330-700).  All arrays are copied by ffhip_sws_from_tables().
 */
typedef struct FFHipSwsTables {
    int srcW, srcH, srcFormat;
    int dstW, dstH, dstFormat;
    int flags;
    FFHipSwsFilter hLum, hChr, vLum, vChr;   /* c->{h,v}{Lum,Chr}Filter[Pos|Size]           */
    /* yuv2rgb: the already cy-scaled coefficients the LUTs are built from
     * (libswscale/yuv2rgb.c:717-800): cy, oy, crv', cbu', cgu', cgv' and the ramp offset yoffs. */
    int64_t yuv2rgb_cy, yuv2rgb_oy, yuv2rgb_crv, yuv2rgb_cbu, yuv2rgb_cgu, yuv2rgb_cgv;
    int     yuv2rgb_yoffs;
    /* Range conversion between YUV formats (round 3): c->opts.src_range / dst_range (0 limited, 1 full) and, when they differ,
     * the constants of c->lumConvertRange / chrConvertRange (ff_sws_init_range_convert + init_range_convert_constants,
     * libswscale/swscale.c:591-660), which the scaler applies to its horizontal intermediates: lumRangeToJpeg_c & co
     * (swscale.c:160-255).  Packed RGB targets take the range through the yuv2rgb coefficients instead (not these fields). */
    int      src_range, dst_range;
    uint32_t lumConvertRange_coeff, chrConvertRange_coeff;
    int64_t  lumConvertRange_offset, chrConvertRange_offset;
    /* SWS_FULL_CHR_H_INT on a packed RGB target — asked for, or forced by an odd width or a 4:4:4 source (libswscale/utils.c:1270-1290):
     * hChr has dstW entries and the yuv2rgb_full_{1,2,X} writers run (output.c:1998-2310) with c->yuv2rgb_{y_coeff, y_offset,
     * v2r_coeff, v2g_coeff, u2g_coeff, u2b_coeff} (yuv2rgb.c:786-791), in this order */
    int      full_chr_h_int;
    int      yuv2rgb_full[6];
    /* 1: the target has an alpha plane the source does not drive: dst[3] is filled with 255 (fillPlane, swscale.c:536-553).
     * 2: both sides are planar YUVA: the alpha plane is scaled by the LUMA banks (lum_h_scale / lum_planar_vscale on plane 3,
     *    hscale.c:63-79, vscale.c:57-70) — src[3] -> dst[3] as the luma of a second pass of the context in which the planners enumerate
     *    the luma job only; not together with a range conversion (the reference converts plane 0 only).
     *    With the equal-size table converter to a 32-bit packed RGB target: src[3] drives the alpha byte (yuva2rgba_c / yuva2argb_c).
     * srcFormat / dstFormat above are then the formats without the alpha plane */
    int      dst_alpha_fill;
} FFHipSwsTables;

typedef struct FFHipSwsContext FFHipSwsContext;

/** Stand-alone construction; same argument meaning as sws_getContext() (libswscale/swscale.h,
 *  libswscale/utils.c:2043) for the formats above; srcFilter/dstFilter/param are the defaults.
 *  Filter banks come from our host restatement of initFilter() (cpu_flags == 0 => filterAlign 1).
 *  Returns NULL (and sets ffhip_last_error) for an unsupported conversion or when no device. */
FFHipSwsContext *ffhip_sws_getContext(int srcW, int srcH, int srcFormat,
                                      int dstW, int dstH, int dstFormat, int flags);
/** Drop-in construction from FFmpeg's own tables (no filter generation on our side).  A context the reference gave a special
 *  converter has no banks (ff_sws_init_single_context() returns before initFilter(), libswscale/utils.c:1625-1637): for the
 *  equal-size yuv420p -> packed RGB table converter (swscale_unscaled.c:2425-2431) the four banks may be left NULL. */
FFHipSwsContext *ffhip_sws_from_tables(const FFHipSwsTables *t);
/** The same for a packed 8-bit RGB source (rgb24 / bgr24 / rgba / bgra / argb / abgr) in front of a YUV target (round 6; ffhip_sws_getContext()
 *  takes these formats directly).  In the reference such a source is its input converters' int16 lines (lumToYV12 / chrToYV12: rgb24ToY_c,
 *  rgb24ToUV_c, rgb24ToUV_half_c and their twins, libswscale/input.c:264-400,1068-1190) scaled by hScale16To15_c at sh = 13
 *  (swscale.c:100-128) — the 16-bit path of a 14-bit planar source, undithered (swscale.c:291).  `t` describes that conversion:
 *  t->srcFormat = FFHIP_PIX_FMT_YUV422P14LE when the chroma converters read pixel pairs (c->chrSrcHSubSample == 1, utils.c:1340-1352),
 *  FFHIP_PIX_FMT_YUV444P14LE otherwise; the banks, ranges (equal) and flags are the context's own.  rgbFormat: the caller's source
 *  format; rgb2yuv: c->input_rgb2yuv_table[RY_IDX .. BV_IDX] (swscale_internal.h:468-477; sws_setColorspaceDetails() fills it).
 *  The context's source is then ONE packed plane, on every face. */
FFHipSwsContext *ffhip_sws_from_tables_rgb_source(const FFHipSwsTables *t, int rgbFormat, const int32_t rgb2yuv[9]);
/** sws_setColorspaceDetails() on a live RGB-source context (fill_rgb2yuv_table(), libswscale/utils.c:614-705,1002): the converter table
 *  replaces the context's.  0, or FFHIP_EINVAL for a context that has no RGB source. */
int ffhip_sws_set_rgb2yuv(FFHipSwsContext *c, const int32_t rgb2yuv[9]);
/** The yuv2rgb fields of the tables (yuv2rgb_cy .. yuv2rgb_yoffs, yuv2rgb_full[]) as ff_yuv2rgb_c_init_tables() derives them
 *  (libswscale/yuv2rgb.c:750-797) from what the context stores: inv_table = c->srcColorspaceTable, fullRange = sws->src_range,
 *  c->brightness / c->contrast / c->saturation (sws_setColorspaceDetails(), utils.c:848-905).  No device needed.  0 or FFHIP_EINVAL. */
int              ffhip_sws_yuv2rgb_coeffs(FFHipSwsTables *t, const int inv_table[4], int fullRange, int brightness, int contrast,
                                          int saturation);
/** sws_setColorspaceDetails() after the context was made (utils.c:990-996 re-runs ff_yuv2rgb_c_init_tables()): the yuv2rgb fields of
 *  `t` replace the context's; every other field of `t` is ignored.  0, FFHIP_EINVAL (coefficients outside the closed form's range). */
int              ffhip_sws_set_yuv2rgb(FFHipSwsContext *c, const FFHipSwsTables *t);
void             ffhip_sws_freeContext(FFHipSwsContext *c);
/** 1 when the context's banks run on the register-resident column-walking kernel (4-tap x 4-tap banks
 *  whose 4-column groups read one 8-byte source span; sws_colwalk.hip), 0 when they take the general
 *  LDS-tiled kernel; bit 1 set when the matrix-core variant (k_sws_mfma) is available too; bit 2 set when the
 *  banks (5..32 taps: down-scaling, long kernels) run on the LDS-backed wide-bank walker (sws_lwalk.hip); bit 3 set when
 *  the conversion is an exact 2x up-scale served by the static-schedule kernel (sws_up2.hip); bit 4: an exact 2:1 down-scale
 *  (sws_down2.hip); bit 5: the 16-bit column walker (sws_walk16.hip); bit 6: exact 2x of 4:2:0 (yuv420p, NV12, NV21) into packed RGB, the
 *  static-schedule kernel with the yuv2rgb_X writer fused (sws_up2rgb.hip); bit 7: the same sources into packed RGB at the source's size
 *  (sws_eqrgb.hip); bit 8: planar 4:4:4 into packed RGB at the source's size, the full-chroma writer on one-tap banks (sws_full444.hip); bit 9: 4:2:0
 *  between its planar and semi-planar layouts at the same size (sws_copy420.hip); bits 10 / 11: yuv444p -> yuv420p / yuv420p -> yuv444p at
 *  the same size: the luma plane copied, the chroma planes on the exact-2:1 / exact-2x static-schedule kernels; bit 12: an exact 3:2
 *  down-scale (sws_down32.hip); bit 13: an exact 3:2 up-scale above 8 bits (sws_up32.hip).
 *  Diagnostic only: results are identical. */
int              ffhip_sws_fast_path(const FFHipSwsContext *c);
/** Diagnostic: the workgroup numbering the context's launch tuner settled on for large launches of the table converter
 *  (yuv2rgb_c_24_rgb's replacement, libswscale/yuv2rgb.c:530) — -1 undecided (fewer than eight large launches so far), 0 plain,
 *  1 an eighth of the launch per XCD.  Which one is faster is a property of the box; results are identical. */
int              ffhip_sws_tuned_numbering(const FFHipSwsContext *c);
/** Host-side preparation of the matrix-core horizontal pass (no device needed): turns one 4-tap horizontal
 *  bank (hLumFilter/hLumFilterPos or the chroma pair's) into per-tile MFMA operand records of 2320 bytes —
 *  B_hi[64 lanes][16], B_lo[64][16] (coefficient = 256*hi + lo, zero outside the band), bias[64] = 128*sum(f),
 *  window base — for tiles of 32 samples (pair != 0: 16 U + 16 V columns of a byte-interleaved plane,
 *  src_swap: V first).  Returns the tile count (records written to `out` when non-NULL) or FFHIP_EINVAL when
 *  the bank does not fit the tiling.  Exposed for the CPU test-suite. */
int              ffhip_sws_mfma_tiles_host(const int16_t *filter, const int32_t *pos, int n, int srcW, int pair, int src_swap,
                                           uint8_t *out, size_t out_size);

/** Host-side preparation of the exact-2x kernel (no device needed): re-expresses a 4-tap bank of a 2x up-scale (n_dst ==
 *  2 n_src) as four coefficients per output on the REGULAR window start (x >> 1) - 2 + (x & 1) of the edge-replicated row —
 *  what initFilter()'s border fold (libswscale/utils.c:519-561) amounts to.  out: n_dst x 2 dwords, (c0, c1) (c2, c3) as
 *  int16 pairs.  Returns 1, or 0 when some tap of the bank does not sit on its regular window (the kernel is then not
 *  used).  Exposed for the CPU test-suite. */
int              ffhip_sws_up2_virtual_bank_host(const int16_t *filter, const int32_t *pos, int n_dst, int n_src, uint32_t *out);
/** The geometry of a launch of the exact-2x kernel (no device needed): plans one plane of `ngroups` 8-byte destination groups per row and
 *  src_h source rows in a batch of nframes frames, strips of about want_steps rows, the way the scaler plans it, and walks the launch through
 *  the inline functions the kernel itself calls.  fshift < 0: the product's choice — rows of ngroups % 64 = 0, 32 or 16 gather their two ends
 *  into waves of 1, 2 or 4 frames; 0..2: packs of 1 << fshift frames that share the rows' ragged end.  out (or NULL): 4 int32 per (wave, lane) —
 *  the frame (-1: the lane idles), the strip, the group in the row, whether the wave holds a row end.  info: the edge lanes per frame (0: ragged
 *  end), fshift, units per (pack, strip), strips.  Returns the launch's waves, FFHIP_ENOMEM when out_ints < 256 x waves, or FFHIP_EINVAL.
 *  Exposed for the CPU test-suite. */
int              ffhip_sws_up2_walk_host(int ngroups, int src_h, int nframes, int want_steps, int fshift, int32_t *out, size_t out_ints, int32_t info[4]);
/** The same at `ratio` 2 or 4 (round 5; sws_up2rgb.hip: a packed-RGB target has a chroma line per output line, so 4:2:0 chroma goes up
 *  four times vertically — output y on the regular window start ((y + 2) >> 2) - 2).  ratio 2 == the call above. */
int              ffhip_sws_upn_virtual_bank_host(const int16_t *filter, const int32_t *pos, int n_dst, int n_src, int ratio, uint32_t *out);
/** The two horizontal virtual banks of the exact-2x RGB kernel (luma: n_hl columns, chroma: n_hc; 2 dwords each, as the calls above
 *  write them) folded into the 32 dwords the kernel reads with scalar loads: [0..3] luma even c01, c23, odd c01, c23; [4..7] chroma;
 *  [8..13] / [14..19] the luma bank's first / last three columns; [20..25] / [26..31] the chroma bank's.  Returns 1, or 0 when a bank
 *  does not repeat with period 2 between its ends (the kernel is then not used). */
int              ffhip_sws_up2rgb_hco_host(const uint32_t *hl, int n_hl, const uint32_t *hc, int n_hc, uint32_t out[32]);
/** The same for the exact-2:1 kernel (sws_down2.hip): a bank of `fsize` <= 16 taps of a 2:1 down-scale (n_src == 2 n_dst) as
 *  eight coefficients per output on the regular window 2x - 3 .. 2x + 4 of the edge-replicated row.  out: n_dst x 4 dwords,
 *  (c0, c1) .. (c6, c7).  Returns 1, or 0 when some tap does not sit on its regular window. */
int              ffhip_sws_down2_virtual_bank_host(const int16_t *filter, const int32_t *pos, int fsize, int n_dst, int n_src, uint32_t *out);
/** The same for the exact-3:2 kernel (sws_down32.hip): a bank of `fsize` <= 12 taps of a 3:2 down-scale (2 n_src == 3 n_dst, n_dst
 *  even) as six coefficients per output on the regular window 3 (x >> 1) - 2 + (x & 1) .. + 5 of the edge-replicated row.  out: n_dst x 3
 *  dwords, (c0, c1) (c2, c3) (c4, c5).  Returns 1, or 0 when some tap does not sit on its regular window. */
int              ffhip_sws_d32_virtual_bank_host(const int16_t *filter, const int32_t *pos, int fsize, int n_dst, int n_src, uint32_t *out);
/** The workgroup numbering of the swscale batch kernels (sws_block_numbering, the same inline function the kernels call): out[b] =
 *  the units workgroup b of a launch of nb workgroups takes, for every b < nb.  mode 0 plain, 1 an eighth of the launch per XCD, 1 + k
 *  XCD-contiguous chunks of 2^k workgroups dealt round-robin.  Returns 0, or FFHIP_EINVAL for a mode outside 0..8 or nb == 0. */
int              ffhip_sws_block_numbering_host(int mode, uint32_t nb, uint32_t *out);

/** Host-table generation alone (no device needed): our initFilter().  `which`: 0 hLum 1 hChr 2 vLum
 *  3 vChr.  Returns filter size or <0; pointers stay valid until ffhip_sws_tables_free().  Used by
 *  the CPU test-suite to pin the host logic against the reference's tables. */
typedef struct FFHipSwsHostTables FFHipSwsHostTables;
FFHipSwsHostTables *ffhip_sws_tables_create(int srcW, int srcH, int srcFormat,
                                            int dstW, int dstH, int dstFormat, int flags);
int  ffhip_sws_tables_get(const FFHipSwsHostTables *t, FFHipSwsTables *out);
/** 1 when the (src,dst,flags) triple takes the reference's table-driven unscaled converter
 *  `yuv2rgb_c_24_rgb` (rule at libswscale/swscale_unscaled.c:2425-2431), 0 for ff_swscale(). */
int  ffhip_sws_tables_is_unscaled_yuv2rgb(const FFHipSwsHostTables *t);
/** The srcRange / dstRange arguments of sws_setColorspaceDetails() (libswscale/utils.c:848-1000) for YUV targets: 0 limited
 *  (MPEG), 1 full (JPEG).  When they differ the tables carry the constants of c->lumConvertRange / chrConvertRange and the
 *  scaler applies them to its horizontal intermediates (swscale.c:160-255); a J format on one side of
 *  ffhip_sws_tables_create() sets the same.  Call before ffhip_sws_tables_get(). */
int  ffhip_sws_tables_set_ranges(FFHipSwsHostTables *t, int src_range, int dst_range);
void ffhip_sws_tables_free(FFHipSwsHostTables *t);

/**
 * SwsFunc-shaped frame call with HOST pointers — the pointer installed as `c->convert_unscaled`
 * (typedef at libswscale/swscale_internal.h:99-101; called at libswscale/swscale.c:1185).
 * Stages src -> device, runs the kernels, copies the written lines back; returns the number of
 * output lines written (srcSliceH for unscaled, dstH for a whole-frame scaled call) or <0.
 * Scaled contexts may be fed in source slices the way sws_scale() allows (in order, top to bottom, starting on even lines;
 * src[] points at the slice's first rows): the slices are collected on the device, the calls before the last return 0 lines
 * and the last one writes the whole picture and returns dstH — the pixels do not depend on the slicing
 * (libswscale's tools/scale_slice_test.c property); a slice out of order is FFHIP_EINVAL.
 */
int ffhip_sws_scale(FFHipSwsContext *c, const uint8_t *const src[], const int srcStride[],
                    int srcSliceY, int srcSliceH, uint8_t *const dst[], const int dstStride[]);

/**
 * Batched, device-resident face.  Frame f of plane p starts at src[p] + f*srcFramePitch[p]
 * (bytes), rows are srcStride[p] bytes apart; likewise dst.  Planes: yuv420p {Y,U,V}, nv12 {Y,UV},
 * rgb24 {RGB}.  Asynchronous on `stream` (hipStream_t).  Returns 0 or <0.
 */
int ffhip_sws_scale_batch_dev(FFHipSwsContext *c, int nframes,
                              const void *const src[4], const int srcStride[4], const size_t srcFramePitch[4],
                              void *const dst[4], const int dstStride[4], const size_t dstFramePitch[4],
                              void *stream);

/** Per-line parity face (device pointers): hyScale/hcScale == hScale8To15_c
 *  (libswscale/swscale.c:128-142; pointer type swscale_internal.h:648-653), batched over `nlines`
 *  lines that share one filter bank. */
int ffhip_sws_hscale8to15_dev(int16_t *dst, int dstW, ptrdiff_t dstPitch, const uint8_t *src, ptrdiff_t srcPitch,
                              int nlines, const int16_t *filter, const int32_t *filterPos, int filterSize,
                              void *stream);
/** yuv2planeX_8_c / yuv2plane1_8_c (libswscale/output.c:468-493; type swscale_internal.h:128-144):
 *  `nsrc` int16 lines at src + j*srcPitch, one output line. dither is 8 bytes. */
int ffhip_sws_yuv2planeX8_dev(const int16_t *filter, int filterSize, const int16_t *src, ptrdiff_t srcPitch,
                              uint8_t *dest, int dstW, const uint8_t *dither8, int offset, void *stream);

/**
 * The per-line members an ff_sws_init_swscale_<arch>() installs (libswscale/swscale.c:697-714; template x86/swscale.c), with the
 * reference's exact signatures, HOST pointers — what tests/checkasm/sw_scale.c:109-458 exercises:
 *   hyScale / hcScale   swscale_internal.h:648-653 (8-bit sources: hScale8To15_c, swscale.c:128-142); `c` is passed through untouched
 *   yuv2plane1          :128 (yuv2plane1_8_c, output.c:482-493)        yuv2planeX   :144 (yuv2planeX_8_c, output.c:468-480)
 *   yuv2nv12cX          :164 (yuv2nv12cX_c, output.c:500-529)
 * One call = one launch through device scratch; lines may be over-read exactly as far as the reference's may (filterPos + filterSize).
 */
typedef struct FFHipSwsLineContext {
    void (*hyScale)(void *c, int16_t *dst, int dstW, const uint8_t *src, const int16_t *filter, const int32_t *filterPos, int filterSize);
    void (*hcScale)(void *c, int16_t *dst, int dstW, const uint8_t *src, const int16_t *filter, const int32_t *filterPos, int filterSize);
    void (*yuv2plane1)(const int16_t *src, uint8_t *dest, int dstW, const uint8_t *dither, int offset);
    void (*yuv2planeX)(const int16_t *filter, int filterSize, const int16_t **src, uint8_t *dest, int dstW, const uint8_t *dither, int offset);
    void (*yuv2nv12cX)(int dstFormat, const uint8_t *chrDither, const int16_t *chrFilter, int chrFilterSize, const int16_t **chrUSrc,
                       const int16_t **chrVSrc, uint8_t *dest, int dstW);
} FFHipSwsLineContext;
/** Fills the members that apply to the format pair (8-bit yuv420p / nv12 / nv21 sources; planar, NV or packed-RGB targets) and
 *  remembers the ones it displaces as fallbacks (see ff_h264dsp_init_hip).  Returns 0, FFHIP_EINVAL or FFHIP_ENOSYS. */
int ff_sws_init_swscale_hip(FFHipSwsLineContext *c, int srcFormat, int dstFormat);
/** yuv2packed1 / yuv2packed2 / yuv2packedX (swscale_internal.h:201-266) for the packed RGB targets (yuv2rgb_{1,2,X}_c_template,
 *  output.c:1789-1939): the reference's argument lists, except that the first argument is this library's context (the members
 *  read the yuv2rgb tables of the context) and that they return 0 or a negative FFHIP_E* — the caller then runs the C member.
 *  dstW even; alpSrc / y are accepted and unused (no alpha plane among the supported sources, no dithered target). */
int ffhip_sws_yuv2packed1(FFHipSwsContext *c, const int16_t *lumSrc, const int16_t *chrUSrc[2], const int16_t *chrVSrc[2],
                          const int16_t *alpSrc, uint8_t *dest, int dstW, int uvalpha, int y);
int ffhip_sws_yuv2packed2(FFHipSwsContext *c, const int16_t *lumSrc[2], const int16_t *chrUSrc[2], const int16_t *chrVSrc[2],
                          const int16_t *alpSrc[2], uint8_t *dest, int dstW, int yalpha, int uvalpha, int y);
int ffhip_sws_yuv2packedX(FFHipSwsContext *c, const int16_t *lumFilter, const int16_t **lumSrc, int lumFilterSize,
                          const int16_t *chrFilter, const int16_t **chrUSrc, const int16_t **chrVSrc, int chrFilterSize,
                          const int16_t **alpSrc, uint8_t *dest, int dstW, int y);

/* ------------------------------------------------------------------------------------------ */
/* libavcodec: h264dsp                                                                        */
/* ------------------------------------------------------------------------------------------ */
/**
 * H264DSPContext subset (libavcodec/h264dsp.h:42-117), same member names and signatures, HOST
 * pointers.  ff_h264dsp_init_hip() below fills it the way ff_h264dsp_init_<arch>() would
 * (libavcodec/h264dsp.c:155-169).
 */
typedef struct FFHipH264DSPContext {
    void (*v_loop_filter_luma)(uint8_t *pix, ptrdiff_t stride, int alpha, int beta, int8_t *tc0);
    void (*h_loop_filter_luma)(uint8_t *pix, ptrdiff_t stride, int alpha, int beta, int8_t *tc0);
    void (*v_loop_filter_luma_intra)(uint8_t *pix, ptrdiff_t stride, int alpha, int beta);
    void (*h_loop_filter_luma_intra)(uint8_t *pix, ptrdiff_t stride, int alpha, int beta);
    void (*v_loop_filter_chroma)(uint8_t *pix, ptrdiff_t stride, int alpha, int beta, int8_t *tc0);
    void (*h_loop_filter_chroma)(uint8_t *pix, ptrdiff_t stride, int alpha, int beta, int8_t *tc0);
    void (*v_loop_filter_chroma_intra)(uint8_t *pix, ptrdiff_t stride, int alpha, int beta);
    void (*h_loop_filter_chroma_intra)(uint8_t *pix, ptrdiff_t stride, int alpha, int beta);
    void (*idct_add)(uint8_t *dst, int16_t *block, ptrdiff_t stride);
    void (*idct8_add)(uint8_t *dst, int16_t *block, ptrdiff_t stride);
    void (*idct_dc_add)(uint8_t *dst, int16_t *block, ptrdiff_t stride);
    void (*idct8_dc_add)(uint8_t *dst, int16_t *block, ptrdiff_t stride);
    void (*idct_add16)(uint8_t *dst, const int *blockoffset, int16_t *block, ptrdiff_t stride,
                       const uint8_t nnzc[5 * 8]);
    void (*idct8_add4)(uint8_t *dst, const int *blockoffset, int16_t *block, ptrdiff_t stride,
                       const uint8_t nnzc[5 * 8]);
    void (*idct_add16intra)(uint8_t *dst, const int *blockoffset, int16_t *block, ptrdiff_t stride,
                            const uint8_t nnzc[5 * 8]);
    void (*idct_add8)(uint8_t **dst, const int *blockoffset, int16_t *block, ptrdiff_t stride,
                      const uint8_t nnzc[15 * 8]);                                   /* h264dsp.h:96-98 (4:2:0) */
    void (*luma_dc_dequant_idct)(int16_t *output, int16_t *input, int qmul);         /* h264dsp.h:102-103 */
    void (*chroma_dc_dequant_idct)(int16_t *block, int qmul);                        /* h264dsp.h:104 (4:2:0) */
    void (*add_pixels8_clear)(uint8_t *dst, int16_t *block, ptrdiff_t stride);      /* h264dsp.h:107 */
    void (*add_pixels4_clear)(uint8_t *dst, int16_t *block, ptrdiff_t stride);      /* h264dsp.h:108 */
    /* the MBAFF forms of the vertical-edge filters (h264dsp.h:50-51,57-58,63-65,70-71): half as many lines per tc0 entry */
    void (*h_loop_filter_luma_mbaff)(uint8_t *pix, ptrdiff_t stride, int alpha, int beta, int8_t *tc0);
    void (*h_loop_filter_luma_mbaff_intra)(uint8_t *pix, ptrdiff_t stride, int alpha, int beta);
    void (*h_loop_filter_chroma_mbaff)(uint8_t *pix, ptrdiff_t stride, int alpha, int beta, int8_t *tc0);
    void (*h_loop_filter_chroma_mbaff_intra)(uint8_t *pix, ptrdiff_t stride, int alpha, int beta);
} FFHipH264DSPContext;
/**
 * Fills every member, the way ff_h264dsp_init_<arch>() does at the end of ff_h264dsp_init() (libavcodec/h264dsp.c:155-169):
 * *c arrives holding the C functions (or NULL members) — the hip faces REMEMBER them, and a call that cannot run on the device
 * (a HIP error, an argument outside the staged range, or FFHIP_FAULT=1 in the environment: the test hook) is answered by the
 * displaced C function instead of returning with dst untouched; ffhip_shim_fallbacks() counts such calls.  The same holds for
 * every ff_*_init_hip() below.  Returns 0, or FFHIP_ENOSYS / FFHIP_EINVAL leaving *c untouched.
 * bit_depth 8 / 9 / 10 / 12 / 14 (every depth the reference instantiates, h264dsp.c:135-147: above 8 bits samples are uint16_t and
 * coefficients int32_t, the depth is baked into the installed functions) and chroma_format_idc 0..2: for 4:2:2 the members the
 * reference switches are the 4:2:2 ones (h_loop_filter_chroma422[_intra / _mbaff], idct_add8_422, chroma422_dc_dequant_idct,
 * h264dsp.c:74-78,98-101,121-132).  4:4:4 (chroma_format_idc 3) uses the 4:2:0 table in the reference too.
 */
int ff_h264dsp_init_hip(FFHipH264DSPContext *c, int bit_depth, int chroma_format_idc);
/** Calls a host-pointer face answered through the displaced C pointer so far (and, when there was none to call, left undone:
 *  ffhip_last_error() has the member's name). */
long ffhip_shim_fallbacks(void);

/** IDCT kinds for the batch face; one kernel per kind == one reference function
 *  (libavcodec/h264idct_template.c:33,69,145,161). */
#define FFHIP_H264_IDCT4     0
#define FFHIP_H264_IDCT8     1
#define FFHIP_H264_IDCT4_DC  2
#define FFHIP_H264_IDCT8_DC  3
#define FFHIP_H264_ADD_PIXELS4_CLEAR 4   /* add_pixels4_clear / add_pixels8_clear: dst += block (8-bit wrap-around), block cleared */
#define FFHIP_H264_ADD_PIXELS8_CLEAR 5   /* (h264addpx_template.c:28-74; the lossless transform bypass) */
/**
 * n independent blocks: block i adds into dst_base + dst_offset[i] (bytes, rows `stride` apart) from
 * coefficients blocks + i*(16|64) int16 (transposed storage as the decoder leaves them), then the
 * coefficients are zeroed — exactly ff_h264_idct{,8}{,_dc}_add_8_c.  Destinations must not overlap.
 */
int ffhip_h264_idct_add_batch_dev(int kind, uint8_t *dst_base, ptrdiff_t stride, const int32_t *dst_offset,
                                  int16_t *blocks, int n, void *stream);
/**
 * Macroblock-level dispatchers over a batch of `nmb` macroblocks: idct_add16 / idct8_add4 /
 * idct_add16intra (libavcodec/h264idct_template.c:177-214).  MB m uses dst_base + mb_offset[m],
 * blocks + m*256 int16, nnzc + m*40 (indexed through scan8, libavcodec/h264_parse.h:40),
 * blockoffset[16] shared.  which: 0 add16, 1 idct8_add4, 2 add16intra.
 */
int ffhip_h264_idct_add_mb_batch_dev(int which, uint8_t *dst_base, ptrdiff_t stride, const int32_t *mb_offset,
                                     const int32_t *blockoffset16, int16_t *blocks, const uint8_t *nnzc,
                                     int nmb, void *stream);

/** idct_add8 (4:2:0, h264idct_template.c:216-228) over `nmb` macroblocks: blocks + m*768 int16 are the decoder's sl->mb (3 x 256),
 *  of which blocks 16..19 (Cb) and 32..35 (Cr) are used; nnzc + m*120 is the 15 x 8 non-zero-count cache (scan8 indexing);
 *  blockoffset48[i] as the decoder's block_offset[]; Cb / Cr block i of MB m lands at c?_base + mb_offset[m] + blockoffset48[i]. */
int ffhip_h264_idct_add8_batch_dev(uint8_t *cb_base, uint8_t *cr_base, ptrdiff_t stride, const int32_t *mb_offset,
                                   const int32_t *blockoffset48, int16_t *blocks, const uint8_t *nnzc, int nmb, void *stream);
/** luma_dc_dequant_idct (h264idct_template.c:259-293) for n macroblocks: input + m*in_pitch (16 DC values), output + m*out_pitch
 *  (the macroblock's 256 coefficients: the 16 results land on the blocks' DC positions), qmul[m].  Pitches in int16 units. */
int ffhip_h264_luma_dc_dequant_idct_batch_dev(int16_t *output, size_t out_pitch, const int16_t *input, size_t in_pitch,
                                              const int32_t *qmul, int n, void *stream);
/** chroma_dc_dequant_idct (4:2:0, h264idct_template.c:323-345), in place on blocks[block_offset[m] + {0,16,32,48}], qmul[m]. */
int ffhip_h264_chroma_dc_dequant_idct_batch_dev(int16_t *blocks, const int32_t *block_offset, const int32_t *qmul, int n, void *stream);

/** Loop-filter kinds == H264DSPContext members (libavcodec/h264dsp_template.c:104-330). */
#define FFHIP_H264_LF_V_LUMA          0
#define FFHIP_H264_LF_H_LUMA          1
#define FFHIP_H264_LF_V_CHROMA        2
#define FFHIP_H264_LF_H_CHROMA        3
#define FFHIP_H264_LF_V_LUMA_INTRA    4
#define FFHIP_H264_LF_H_LUMA_INTRA    5
#define FFHIP_H264_LF_V_CHROMA_INTRA  6
#define FFHIP_H264_LF_H_CHROMA_INTRA  7
/** One edge descriptor of the batch face: everything the reference call takes besides pix/stride.
 *  alpha == 0 or beta == 0 leaves the edge untouched on every face (no difference is below 0).  tc0 of a bS = 4 record (an _INTRA kind) is
 *  ignored, whatever it holds.  The frame faces read kind >= 4 as bS = 4 and nothing else of `kind` (bits 0 / 1: the direction and the
 *  plane follow from the record's place in the table) and ignore `offset`. */
typedef struct FFHipH264Edge {
    int32_t offset;      /* pix = base + offset                                    */
    uint8_t kind;        /* FFHIP_H264_LF_*                                         */
    uint8_t alpha, beta; /* 8-bit tables top out at 255 / 18 (h264_loopfilter.c)   */
    uint8_t pad;
    int8_t  tc0[4];
} FFHipH264Edge;
/**
 * n edges whose touched pixels are pairwise DISJOINT (function-level batch, as checkasm's tiles).
 * Order-dependent frame deblocking is ffhip_h264_deblock_frame_dev().
 * Any `offset` and any stride are accepted: a line of a vertical edge (an h_ kind) whose address base + offset + line * stride is 4-byte
 * aligned moves as two dwords, every other line sample by sample; the choice is made line by line.  (Above 8 bits,
 * ffhip_h264_loop_filter_batch_dev_hbd(), base + offset and the stride are even: samples are uint16_t.)
 */
int ffhip_h264_loop_filter_batch_dev(uint8_t *base, ptrdiff_t stride, const FFHipH264Edge *edges, int n,
                                     void *stream);
/**
 * True frame-order luma deblocking of a whole picture (mb_w x mb_h macroblocks): for every MB in
 * raster order, vertical edges 0..3 left-to-right then horizontal edges 0..3 top-to-bottom, as
 * ff_h264_filter_mb() orders the h264dsp calls (libavcodec/h264_loopfilter.c:716).
 * edges[(mb*2 + dir)*4 + e] describes MB mb, dir 0 = vertical edges (h_loop_filter_*), 1 =
 * horizontal; kind >= 4 selects intra (bS = 4: tc0 ignored), anything below normal (tc0 used); bits 0 / 1 of `kind` and `offset` are
 * ignored; alpha == 0 or beta == 0 skips the edge.
 * Implemented as a 2-D wavefront over MBs — bit-exact with the serial order.
 */
int ffhip_h264_deblock_frame_dev(uint8_t *luma, ptrdiff_t stride, int mb_w, int mb_h,
                                 const FFHipH264Edge *edges, void *stream);
/** The same over `nframes` independent pictures in one launch (frame f at luma + f*frame_pitch, its edges at
 *  edges + f*mb_w*mb_h*8): the order inside a picture is serial, pictures run side by side. */
int ffhip_h264_deblock_frames_dev(uint8_t *luma, size_t frame_pitch, int nframes, ptrdiff_t stride, int mb_w, int mb_h,
                                  const FFHipH264Edge *edges, void *stream);

/**
 * The same for one 4:2:0 CHROMA plane (8x8 samples per macroblock; call once for Cb and once for Cr — their alpha / beta / tc0
 * come from different QPs): per MB the vertical edges at x = 0 and 4, then the horizontal ones at y = 0 and 4, as
 * filter_mb_dir() filters chroma on the even luma edges (libavcodec/h264_loopfilter.c:644-700).
 * edges[((f * mb_h * mb_w + mb) * 2 + dir) * 2 + e]; kinds FFHIP_H264_LF_*_CHROMA[_INTRA], read as kind >= 4: bS = 4; alpha == 0 or
 * beta == 0 skips an edge.
 * plane, stride and frame_pitch must be 4-byte aligned.
 */
int ffhip_h264_deblock_frames_chroma_dev(uint8_t *plane, size_t frame_pitch, int nframes, ptrdiff_t stride, int mb_w, int mb_h,
                                         const FFHipH264Edge *edges, void *stream);

/**
 * Both of the above at the depths H264DSPContext is instantiated for (libavcodec/h264dsp.c:135-147; bit_depth 8, 9, 10, 12 or 14): above
 * 8 bits the samples are uint16_t (stride and frame_pitch stay in BYTES), alpha / beta / tc0 of the edge records stay in the 8-bit
 * units the decoder passes and are scaled inside as h264dsp_template.c:104-330 scales them (alpha, beta << (depth - 8); luma tc0 *
 * (1 << (depth - 8)); chroma ((tc0 - 1) << (depth - 8)) + 1).  chroma != 0: one 4:2:0 chroma plane per frame.  Above 8 bits plane,
 * stride, frame_pitch and edges must be 16-byte aligned (the byte / dword paths are 8-bit kernels): FFHIP_EINVAL otherwise.
 */
int ffhip_h264_deblock_frames_dev_hbd(int bit_depth, int chroma, uint8_t *plane, size_t frame_pitch, int nframes, ptrdiff_t stride, int mb_w,
                                      int mb_h, const FFHipH264Edge *edges, void *stream);

/**
 * The edge tables of the three frame-order faces above, made from what the decoder has parsed: per macroblock its slice, non-zero
 * bits, qp and flags, the per-4x4 motion field, and per slice the reference lists and filter offsets.  What ff_h264_filter_mb() derives
 * on the host, macroblock by macroblock, as one gather over the picture.  Non-MBAFF pictures: frames (field 0) and field pictures
 * (field 1: the field is the picture); 4:2:0 chroma, monochrome with NULL chroma_qp / cb / cr.
 * Restated from H.264 8.7.2.1 / 8.7.2.2 and the behaviour of libavcodec/h264_loopfilter.c; NOT checked against the reference's
 * source, which the build does not have.
 *
 * For macroblock q = (mb_x, mb_y): dir 0 is the vertical edges at x = 4e, dir 1 the horizontal edges at y = 4e, e = 0..3.  On e = 0
 * p is the macroblock to the left / above, otherwise p = q.  S = slices[q.slice].
 *  1. An edge is skipped when: e = 0 at the picture border; S.idc == 1; e = 0, S.idc == 2 and p.slice != q.slice; e odd and q has
 *     the 8x8 transform; q.slice >= nslices.  A skipped edge's record is zero but for `kind` (the non-intra kind of its plane and
 *     direction) and tc0 ({-1,-1,-1,-1} luma, {0,0,0,0} chroma).
 *  2. bS of the 4-line group g (the 4x4 blocks on either side of the edge): p or q intra: 4 when e = 0 and (field == 0 or
 *     dir == 0), otherwise 3; else the nnz bit of the p-side or the q-side block: 2; else motion decides, 1 or 0:
 *     - a block's reference of a list is slices[slice of its own macroblock].ref[list][ref_idx]; ref_idx < 0 is "unused": all
 *       unused references are equal, and the list's motion vector counts as (0, 0) whatever the record holds; a ref_idx >= that
 *       slice's num_ref or >= 32, or a macroblock whose slice is >= nslices, gives a reference that differs from every other,
 *       another such one and the unused ones included, and (0, 0) as well;
 *     - lists: 2 if S is a B slice, else list 0 alone; two vectors differ when |dx| >= 4 or |dy| >= (field ? 2 : 4);
 *     - straight: ref0 differ or mv0 differ; if not, and with two lists, ref1 differ or mv1 differ;
 *     - if straight says different and there are two lists, crossed: 1 if p.ref0 != q.ref1 or p.ref1 != q.ref0, else 1 iff
 *       (p.mv0, q.mv1) differ or (p.mv1, q.mv0) differ.
 *  3. Every group 0: the skipped record.  Otherwise qp = (p.qp + q.qp + 1) >> 1 on e = 0, else q.qp; indexA = clip(qp -
 *     qp_bd_offset + S.alpha_c0_offset, 0, 51), indexB with beta_offset; alpha, beta from Tables 8-16; bS 4: the *_INTRA kind,
 *     tc0 {0,0,0,0} (unused); else the normal kind, tc0[g] = tc0'[indexA][bS_g] (Table 8-17), -1 at bS 0.  alpha or beta 0 stay: the
 *     filter disables itself.
 *  4. Chroma plane c (Cb 0, Cr 1), edge e' = 0, 1 is luma edge 2e' with its skip rule and its four bS (an 8x8-transform
 *     macroblock keeps its chroma edge 1); qp from chroma_qp[c][p.qp] and chroma_qp[c][q.qp] the same way (a qp above 87 reads
 *     entry 87); tc0[g] = tc0'[indexA][bS_g] + 1, 0 at bS 0; the *_CHROMA / *_CHROMA_INTRA kinds.
 *  5. offset and pad are 0.  Every record of every table is written exactly once, nothing else is, and no input is written; malformed
 *     input has the result defined above and never causes an access outside the maps.
 * The records are in the 8-bit units the deblock faces scale by depth.
 * Out of scope: MBAFF.  The 4:2:2 / 4:4:4 chroma tables are ffhip_h264_edge_params_pictures_fmt_dev's below (rules 6 and 7).
 */
typedef struct FFHipH264MvField {  /* one 4x4 luma block, 12 bytes, grid w4 = 4*mb_w by h4 = 4*mb_h */
    int16_t mv[2][2];              /* [list][x, y], quarter samples */
    int8_t  ref_idx[2];            /* < 0: list unused */
    uint8_t pad[2];
} FFHipH264MvField;
typedef struct FFHipH264BsMb {     /* one macroblock, 8 bytes */
    uint16_t slice;                /* index into slices */
    uint16_t nnz;                  /* bit (bx + 4*by): that 4x4 luma block has non-zero coefficients.  For a macroblock with the
                                      8x8 transform the decoder sets all four bits of an 8x8 block or none: the reference's CAVLC
                                      fix-up, the caller's job. */
    uint8_t  qp;                   /* QP'Y as the decoder stores it (0 for I_PCM; above 8 bits with the depth offset) */
    uint8_t  flags;                /* bit 0 intra (I_PCM included), bit 1 transform_size_8x8_flag */
    uint8_t  pad[2];
} FFHipH264BsMb;
typedef struct FFHipH264BsSlice {  /* 72 bytes */
    uint8_t ref[2][32];            /* [list][ref_idx] -> picture identity: equal bytes name the same reference picture.  In a field
                                      picture the two parities of a frame have different bytes. */
    uint8_t num_ref[2];
    int8_t  alpha_c0_offset, beta_offset;  /* slice_alpha_c0_offset_div2 * 2, slice_beta_offset_div2 * 2: -12 .. 12 */
    uint8_t idc;                   /* disable_deblocking_filter_idc: 0, 1, 2 */
    uint8_t flags;                 /* bit 0: B slice (both lists take part in the comparison) */
    uint8_t pad[2];
} FFHipH264BsSlice;
typedef struct FFHipH264BsPic {    /* _dev: device pointers, _host: host pointers */
    const FFHipH264BsMb    *mb;        /* mb_w * mb_h, raster */
    const FFHipH264MvField *mvf;       /* [by * mvf_stride + bx], 4-byte aligned */
    const FFHipH264BsSlice *slices;    /* nslices records */
    const uint8_t *chroma_qp;          /* [2][88]: Cb then Cr, the pps's chroma_qp_table indexed by QP'Y; NULL: no chroma tables */
    FFHipH264Edge *luma;               /* out: [(mb*2 + dir)*4 + e], the layout of ffhip_h264_deblock_frames_dev */
    FFHipH264Edge *cb, *cr;            /* out: [(mb*2 + dir)*2 + e], the layout of ..._chroma_dev; both NULL or both set */
    int32_t mvf_stride, nslices;       /* mvf_stride in records */
} FFHipH264BsPic;
/** npics pictures of mb_w x mb_h macroblocks (1..4096 each); field 0 / 1; qp_bd_offset 0, 6, 12, 24 or 36 (6 * (bit depth - 8)).
 *  Pictures go 16 to a launch.  Asynchronous on `stream`; the tables are ready for the deblock faces on the same stream with no
 *  synchronisation in between.
 *  FFHIP_EINVAL for another size, qp_bd_offset or field, npics <= 0, NULL mb / mvf / slices / luma, only one of cb / cr, cb without
 *  chroma_qp, an mvf or an output table that is not 4-byte aligned, mvf_stride < 4*mb_w, nslices < 1, or an output table whose span
 *  overlaps the span of any input or of any other output table of the call; FFHIP_ENOSYS without a device (after the argument checks). */
int ffhip_h264_edge_params_pictures_dev(int mb_w, int mb_h, int field, int qp_bd_offset, int npics,
                                        const FFHipH264BsPic *pics /* host array */, void *stream);
/** The same rules compiled for the CPU, on host arrays (device-free): the same arguments, refusals but FFHIP_ENOSYS, and bytes.
 *  The _dev face never calls it. */
int ffhip_h264_edge_params_pictures_host(int mb_w, int mb_h, int field, int qp_bd_offset, int npics, const FFHipH264BsPic *pics);
/** sizeof(FFHipH264BsMb), sizeof(FFHipH264MvField), sizeof(FFHipH264BsSlice), for bindings that mirror the records (no device needed). */
int ffhip_h264_bs_mb_record_size(void);
int ffhip_h264_bs_mvf_record_size(void);
int ffhip_h264_bs_slice_record_size(void);

/**
 * ffhip_h264_edge_params_pictures_fmt_dev: rules 1 to 5 above with the same records, and by chroma_format_idc:
 * chroma_format_idc 0: no chroma tables: chroma_qp / cb / cr are not read, and nothing is written through them.
 * chroma_format_idc 1: the face above, its bytes and return values.
 *  6. chroma_format_idc 2 (4:2:2, chroma macroblocks of 8 x 16 samples): cb / cr hold SIX records per macroblock, [mb*6 + k], the
 *     layout of ffhip_h264_picture_deblock_mb() and of ffhip_h264_deblock_pictures_fmt_dev below.
 *     - k = 0, 1: the vertical edges x = 0, 4: luma edges 0 and 2 of dir 0 with rule 1's skips and rule 2's four bS; tc0[g] belongs to
 *       the 4-line group g (h_loop_filter_chroma422 filters 16 lines with one tc0 per 4 lines).
 *     - k = 2 .. 5: the horizontal edges y = 0, 4, 8, 12: luma edges e = k - 2 of dir 1; tc0[g] covers two columns, as at 4:2:0.  The
 *       "e odd and q has the 8x8 transform" clause of rule 1 does NOT hold for these four records: the luma record of such an edge is
 *       the skipped record, the chroma record carries the bS rule 2 gives the edge (intra 3, a non-zero bit 2, otherwise motion
 *       decides).  Every other skip of rule 1 holds.
 *     - qp, indexA / indexB, tc0 = tc0' + 1 (0 at bS 0), the *_CHROMA / *_CHROMA_INTRA kinds and the skipped record as in rule 4.
 *  7. chroma_format_idc 3 (4:4:4): cb / cr hold EIGHT records per macroblock in the luma layout [(mb*2 + dir)*4 + e], with the LUMA
 *     kinds and the luma tc0 convention (tc0' without the + 1, -1 at bS 0, a skipped record's tc0 {-1,-1,-1,-1}).  Every skip of rule 1
 *     holds for all three planes, the 8x8-transform one included; bS is the luma edge's; qp from chroma_qp[c] as in rule 4 (the average
 *     of the two looked-up values on e = 0, q's otherwise).  The tables ffhip_h264_deblock_frames_dev / _dev_hbd(chroma = 0),
 *     ffhip_h264_deblock_pictures_fmt_dev and ffhip_h264_picture_deblock_mb() take for planes 1 and 2 of a 4:4:4 picture.
 * Rule 5 holds at every format.  Rule 6 restates filter_mb_dir() of libavcodec/h264_loopfilter.c ("if (!deblock_edge && (!chroma422 ||
 * dir == 0)) continue;", chroma filtered at 4 * edge * uvlinesize on every edge of dir 1); restated, NOT checked against the source,
 * which the build does not have.
 * FFHIP_EINVAL for a chroma_format_idc outside 0 .. 3 and for everything the face above refuses, the overlap spans computed with the
 * format's table sizes (mb_w * mb_h * 4, 6 or 8 records in cb / cr; at 0 cb, cr and chroma_qp are not looked at); FFHIP_ENOSYS without
 * a device (after the argument checks).  Out of scope: MBAFF.
 */
int ffhip_h264_edge_params_pictures_fmt_dev(int chroma_format_idc, int mb_w, int mb_h, int field, int qp_bd_offset, int npics,
                                            const FFHipH264BsPic *pics /* host array */, void *stream);
/** The same rules compiled for the CPU, on host arrays (device-free): the same arguments, refusals but FFHIP_ENOSYS, and bytes.
 *  The _dev face never calls it. */
int ffhip_h264_edge_params_pictures_fmt_host(int chroma_format_idc, int mb_w, int mb_h, int field, int qp_bd_offset, int npics,
                                             const FFHipH264BsPic *pics);

/**
 * Frame-order deblocking of npics whole pictures of mb_w x mb_h macroblocks at chroma_format_idc 0 .. 3 and bit_depth 8, 9, 10, 12 or
 * 14, from the tables of ffhip_h264_edge_params_pictures_fmt_dev (or a caller's own in the same layouts).  No kernel of its own: plane 0
 * at every format, and all three planes at 4:4:4, go through the luma filter of ffhip_h264_deblock_frames_dev / _dev_hbd; Cb / Cr of
 * 4:2:0 through the chroma filter of ffhip_h264_deblock_frames_chroma_dev / _dev_hbd(chroma = 1), whose bytes they are; Cb / Cr of
 * 4:2:2 (8 x 16 samples a macroblock, six records each: rule 6 above) through the 4:2:2 frame-order filter the picture object's flush
 * uses, the chroma planes of all pictures side by side.  At format 0 plane[1], plane[2] and their tables are ignored.  A NULL edges[p]
 * skips plane p.  stride_y: plane 0; stride_c: planes 1 and 2; both in bytes.  Samples above 8 bits are uint16_t.
 * Asynchronous on `stream`; the planes are complete for work queued behind the call on `stream`.
 * The face inherits the launchers' limits: at 8 bits every plane, stride and edge table 4-byte aligned; above 8 bits 16-byte aligned,
 * but for the 4:2:2 chroma planes and stride_c (8 bytes) and their tables (4 bytes); mb_w and mb_h 1 .. 4096, which is within the
 * progress pool's 8191 macroblock rows.  FFHIP_EINVAL with a text for another bit_depth, format or size, npics <= 0 or NULL pics, a
 * table without its plane, or a misaligned plane, stride or table; FFHIP_ENOSYS without a device (after the argument checks).
 */
typedef struct FFHipH264LfPic {
    uint8_t *plane[3];              /* device pointers */
    const FFHipH264Edge *edges[3];  /* device pointers; NULL: the plane is not filtered */
} FFHipH264LfPic;
int ffhip_h264_deblock_pictures_fmt_dev(int bit_depth, int chroma_format_idc, int mb_w, int mb_h, ptrdiff_t stride_y, ptrdiff_t stride_c,
                                        int npics, const FFHipH264LfPic *pics /* host array */, void *stream);
/** sizeof(FFHipH264LfPic), for bindings that mirror the record (no device needed). */
int ffhip_h264_lf_pic_record_size(void);

/**
 * The inter prediction of whole H.264 pictures in one launch, from the same two arrays the edge-parameter face above takes (mb, mvf)
 * plus one record per slice: what hl_motion() / mc_part() / mc_part_std() / mc_part_weighted() / mc_dir_part() of
 * libavcodec/h264_mb.c do macroblock by macroblock, as one gather over the picture.  Both lists and the weighting are combined in
 * registers and every sample is written once.  Non-MBAFF pictures (a frame, or one field as base + doubled stride); 4:2:0 and
 * monochrome.  Restated from memory of h264_mb.c and from H.264 8.4.2.2 / 8.4.2.3, pinned through the oracle's members; NOT checked
 * against the reference's source, which the build does not have.
 *
 * H.264 prediction is a function of the sample: its value depends only on the vector and the reference of the 4x4 block that covers
 * it, never on the partition shape, and emulated_edge_mc is a clamp of each source coordinate.  So the face takes no partition types.
 * For each 4x4 luma block b of macroblock m (and its 2x2 block of Cb and of Cr), S = slices[m.slice]:
 *  1. m intra (flags & 1): none of its samples is written.
 *  2. b is malformed, reads no reference and writes nothing (luma and chroma), when: m.slice >= nslices; no list is used
 *     (ref_idx[list] < 0 for both); a used list has ref_idx >= S.num_ref[list], ref_idx >= 32, S.num_ref[list] > 32 or the slot
 *     S.ref[list][ref_idx] >= nrefs; a log2 denominator of S is above 7; S.use_weight > 2.
 *  3. the luma sample of one list: h264qpel's put at position (mvx & 3) + ((mvy & 3) << 2), source origin the block's position plus
 *     (mvx >> 2, mvy >> 2), every source sample fetched at row clamp(y, 0, 16*mb_h - 1), column clamp(x, 0, 16*mb_w - 1) of the
 *     slot's plane.  Vectors may point anywhere in int16_t.
 *  4. the chroma sample of one list: cx = mvx, cy = mvy + ref.chroma_dy; h264chroma's put with the fractions (cx & 7, cy & 7), origin
 *     the chroma block's position plus (cx >> 3, cy >> 3), coordinates clamped to 8*mb_w x 8*mb_h.
 *  5. weighted: S.use_weight == 1; or S.use_weight == 2, both lists used and S.implicit_weight[r0][r1] != 32 (r0, r1: the ref_idx).
 *  6. not weighted: one list: its sample; two lists: (p0 + p1 + 1) >> 1.
 *  7. weighted, two lists: implicit: biweight(p0, p1, log2_denom 5, w0 = implicit_weight[r0][r1], w1 = 64 - w0, offset 0) on all
 *     planes; explicit: luma biweight(p0, p1, luma_log2_denom, luma_weight[r0][0][0], luma_weight[r1][1][0], luma_weight[r0][0][1] +
 *     luma_weight[r1][1][1]), chroma the same with chroma_weight[..][..][c] and chroma_log2_denom (always; use_weight_chroma is not
 *     consulted).
 *  8. weighted, one list L: luma weight(p, luma_log2_denom, luma_weight[r][L][0], luma_weight[r][L][1]); chroma the same way with
 *     chroma_weight only when S.use_weight_chroma is set, plain otherwise.
 *  9. weight / biweight are h264dsp's weight_h264_pixels / biweight_h264_pixels (dst = list 0 with weightd, src = list 1 with
 *     weights); offsets in 8-bit units, scaled by the depth inside as the batch faces take them.
 * 10. Every sample of every well-formed block of a non-intra macroblock is written exactly once; nothing else is: not intra
 *     macroblocks, not the stride padding, no input.
 * Out of scope: the residual (ffhip_h264_residual_pictures_dev below follows on the same stream), MBAFF; 4:2:2 / 4:4:4 are the _fmt
 * faces' (after the residual faces below).
 */
typedef struct FFHipH264InterSlice {       /* what mc_part() reads from the slice, 2888 bytes */
    uint8_t  ref[2][32];                   /* [list][ref_idx] -> slot: index into FFHipH264InterPic.ref */
    uint8_t  num_ref[2];                   /* 0..32 */
    uint8_t  use_weight;                   /* pwt.use_weight: 0 none, 1 explicit, 2 implicit */
    uint8_t  use_weight_chroma;            /* pwt.use_weight_chroma */
    uint8_t  luma_log2_denom, chroma_log2_denom;   /* 0..7 */
    uint8_t  pad[2];
    int16_t  luma_weight[32][2][2];        /* [ref_idx][list][weight, offset]: pwt.luma_weight, defaults filled in by the decoder */
    int16_t  chroma_weight[32][2][2][2];   /* [ref_idx][list][Cb, Cr][weight, offset] */
    int16_t  implicit_weight[32][32];      /* [ref_idx0][ref_idx1]: list 0's weight, -64..128 (non-MBAFF: both parities equal) */
} FFHipH264InterSlice;
typedef struct FFHipH264InterRef {         /* one reference picture (a frame, or one field as base + doubled stride), 56 bytes */
    const uint8_t *base[3];                /* device; Cb / Cr are read only where the picture has chroma */
    ptrdiff_t stride[3];                   /* bytes; a multiple of the sample size, any sign */
    int8_t  chroma_dy;                     /* added to the chroma vector's y (eighth samples) before it is split: the decoder sets
                                              2 * (current parity - reference parity) for 4:2:0 field pictures, else 0 */
    uint8_t pad[7];
} FFHipH264InterRef;
typedef struct FFHipH264InterPic {         /* 1880 bytes */
    uint8_t *dst[3];                       /* device; Cb and Cr NULL: luma only (monochrome) */
    ptrdiff_t dst_stride[3];               /* bytes; base and stride multiples of 4 samples, stride >= the plane's width */
    const FFHipH264BsMb *mb;               /* device, mb_w * mb_h raster: predicted iff !(flags & 1); `slice` indexes slices */
    const FFHipH264MvField *mvf;           /* device, [by * mvf_stride + bx], 4-byte aligned; a list is used iff ref_idx[list] >= 0 */
    const FFHipH264InterSlice *slices;     /* device, nslices records */
    int32_t mvf_stride, nslices, nrefs, pad;
    FFHipH264InterRef ref[32];             /* in this host array: the face stages it to the device */
} FFHipH264InterPic;
/** npics pictures of mb_w x mb_h macroblocks (1..4096 each) at bit_depth 8, 9, 10, 12 or 14 (uint16_t samples above 8; strides stay
 *  in bytes), chroma_format_idc 0 (Cb / Cr ignored) or 1.  Pictures go 16 to a launch.  Asynchronous on `stream`.
 *  FFHIP_ENOSYS (with a text) for chroma_format_idc 2 or 3; MBAFF pictures have no entry here: the caller keeps them on its own path.
 *  FFHIP_EINVAL for another depth, format or size, npics <= 0, a NULL or misaligned dst plane or stride, a stride below the plane's
 *  width, only one of Cb / Cr, NULL mb / mvf / slices, an mvf that is not 4-byte aligned, mvf_stride < 4*mb_w, nslices < 1, nrefs
 *  outside 0..32, a NULL or sample-misaligned plane among the first nrefs references, or an overlap: a reference row that shares a
 *  byte with a destination row of any picture of the call, or two destination planes that do.  Rows, not spans: the two fields of a
 *  frame (equal strides s, bases a row apart) are accepted, the second predicted from the first; with d = (ref.base - dst.base) mod s
 *  the rows are disjoint iff d >= dst_row_bytes and d + ref_row_bytes <= s.  Overlapping spans with unequal strides are refused.
 *  FFHIP_ENOSYS without a device (after the argument checks). */
int ffhip_h264_inter_pictures_dev(int bit_depth, int chroma_format_idc, int mb_w, int mb_h, int npics,
                                  const FFHipH264InterPic *pics /* host array */, void *stream);

/** Rules 1, 2 and 5 to 8 for one block, resolved: what the kernel computes per block before it touches a sample. */
enum { FFHIP_H264_INTER_SKIP = 0,          /* intra or malformed: nothing read, nothing written; every other field 0 */
       FFHIP_H264_INTER_UNI, FFHIP_H264_INTER_UNI_W, FFHIP_H264_INTER_BI_AVG, FFHIP_H264_INTER_BI_W };
typedef struct FFHipH264InterBlockPlan {   /* 28 bytes; fields a mode does not use are 0 */
    uint8_t mode;                          /* FFHIP_H264_INTER_* */
    uint8_t list;                          /* UNI / UNI_W: the list used (whose vector is read) */
    uint8_t slot[2];                       /* BI_*: the slots of list 0 and list 1; UNI*: slot[0] alone */
    uint8_t chroma_weighted;               /* UNI_W: S.use_weight_chroma != 0; BI_W: 1 */
    uint8_t luma_log2_denom, chroma_log2_denom;    /* *_W; chroma's only if chroma_weighted */
    uint8_t pad;
    int16_t luma_weight[2], luma_offset;   /* UNI_W: weight[0]; BI_W: weightd (list 0), weights (list 1), the summed offset */
    int16_t chroma_weight[2][2], chroma_offset[2]; /* [Cb, Cr][as luma_weight], [Cb, Cr] */
    int16_t pad2;
} FFHipH264InterBlockPlan;
typedef struct FFHipH264InterPlanPic {     /* host pointers */
    const FFHipH264BsMb *mb;
    const FFHipH264MvField *mvf;
    const FFHipH264InterSlice *slices;
    FFHipH264InterBlockPlan *plans;        /* out: [by * 4*mb_w + bx], 16 * mb_w * mb_h plans */
    int32_t mvf_stride, nslices, nrefs, pad;
} FFHipH264InterPlanPic;
/** The plan of every 4x4 block of npics pictures, by the function the kernel uses (device-free).  FFHIP_EINVAL for mb_w / mb_h
 *  outside 1..4096, npics <= 0, NULL mb / mvf / slices / plans, an mvf that is not 4-byte aligned, mvf_stride < 4*mb_w, nslices < 1,
 *  nrefs outside 0..32, or a plan array that overlaps an input or another plan array of the call. */
int ffhip_h264_inter_plan_pictures_host(int mb_w, int mb_h, int npics, const FFHipH264InterPlanPic *pics);
/** sizeof the records above, for bindings that mirror them (no device needed). */
int ffhip_h264_inter_slice_record_size(void);
int ffhip_h264_inter_ref_record_size(void);
int ffhip_h264_inter_pic_record_size(void);
int ffhip_h264_inter_plan_record_size(void);
int ffhip_h264_inter_plan_pic_record_size(void);

/**
 * The residual of every inter macroblock of whole H.264 pictures in one launch, between the inter face above and the edge-parameter
 * face: what hl_decode_mb_idct_luma() and the chroma part of hl_decode_mb() do for an inter macroblock through idct_add16 /
 * idct8_add4, chroma_dc_dequant_idct and idct_add8, from the macroblock array those faces take (its nnz bits and flags) plus one small
 * record per macroblock.  Non-MBAFF pictures (a frame, or one field as base + doubled stride); 4:2:0 and monochrome.
 *
 * The coefficients of a macroblock lie as in the decoder's sl->mb, `coeff_offset` coefficients into `coeffs`: luma block i of the
 * decoder's block order at 16*i, its position x4 = (i&1) + 2*((i>>2)&1), y4 = ((i>>1)&1) + 2*(i>>3); an 8x8 block k in the 64
 * coefficients at 64*k; Cb block j at 256 + 16*j, Cr block j at 512 + 16*j (j = x + 2*y), the chroma DC values on their blocks' first
 * coefficients; stored transposed, as the idct faces take them.  Macroblocks may lie in any order and need only what they use.
 * For macroblock m, with record r:
 *  1. m intra (flags & 1): none of its samples is touched (they belong to the intra wavefront).
 *  2. need = 768 where the picture has chroma planes and r.chroma | r.chroma_dc is non-zero (monochrome ignores both fields);
 *     otherwise 256 if m.nnz is non-zero, else 0: nothing happens.
 *  3. m is malformed and writes nothing on any plane when r.coeff_offset < 0, is not a multiple of 16, or coeff_offset + need > ncoeffs.
 *  4. luma, m without the 8x8 flag: every block i whose nnz bit (x4 + 4*y4) is set gets idct_add.
 *  5. luma, m with the 8x8 flag (flags & 2): 8x8 block k gets idct8_add iff the nnz bit of its top-left 4x4 block is set (the test of
 *     idct8_add4; the FFHipH264BsMb contract makes the four bits equal).
 *  6. chroma plane c with r.chroma_dc bit c: the first coefficients of the plane's four blocks go through chroma_dc_dequant_idct
 *     with r.qmul[c], in registers, truncated to the coefficient type as the reference stores them; then all four blocks are added:
 *     a block whose r.chroma bit is set by idct_add with that DC, a block whose bit is clear by idct_dc_add of it.
 *  7. chroma plane c without its DC bit: the blocks whose r.chroma bit is set get idct_add.
 *  8. a block whose bit is clear is not read (under rule 6 its first coefficient is).
 *  9. Bits, not counts.  idct_add16, idct8_add4 and idct_add8 choose *_dc_add from a non-zero count of 1 or from block[0];
 *     (dc + 32) >> 6 on every sample is what the full transform gives for a block with nothing but a DC, in both coefficient widths,
 *     with one exception: the transform adds the 32 in the coefficient type, so at 8 bits a DC of 32736 .. 32767 wraps there and not
 *     in *_dc_add.  The face follows the reference there too: a luma block whose other coefficients are all zero takes the *_dc_add
 *     form (what a count of 1 with block[0] set means in a decoder's data), a chroma block with its bit the transform, one without
 *     (rule 6) the *_dc_add form.  For every other content the choice does not change a byte.
 * 10. the samples of the transformed blocks are written once each; nothing else is touched: not the padding, not coeffs (the batch
 *     faces clear what they consume; this one does not), not a map.
 * 11. results clip to (1 << bit_depth) - 1.
 * 12. m.slice and m.qp are not looked at: a caller whose inter call dropped a macroblock as malformed drops it here too (nnz 0, no
 *     chroma bits).
 * Out of scope: the lossless bypass, MBAFF, luma DC (intra 16x16), I_PCM; 4:2:2 / 4:4:4 are the _fmt faces' below.
 */
typedef struct FFHipH264ResMb {            /* one macroblock, 16 bytes; parallel to FFHipH264BsMb */
    int32_t coeff_offset;                  /* in coefficients into FFHipH264ResPic.coeffs; a multiple of 16 */
    uint8_t chroma;                        /* bit j: Cb 4x4 block j has coefficients; bit 4 + j: Cr block j (j = x + 2*y) */
    uint8_t chroma_dc;                     /* bit 0: Cb DC coded (chroma_dc_dequant_idct runs on it); bit 1: Cr */
    uint8_t chroma_lo422;                  /* read at chroma_format_idc 2 alone (the _fmt faces): bit j - 4: Cb block j = 4..7 of the
                                              8 x 16 chroma, bit 4 + (j - 4): Cr block j; without effect at any other format */
    uint8_t pad;
    union {
        int32_t qmul[2];                   /* Cb, Cr: the decoder's dequant4_coeff[4 + c][chroma qp][0]; 4:2:2: [1 + c][chroma_qp[c] + 3][0] */
        uint32_t nnz444[2];                /* chroma_format_idc 3 alone (no chroma DC there): the low 16 bits are the non-zero bits of
                                              Cb, Cr in FFHipH264BsMb.nnz's layout */
    };
} FFHipH264ResMb;
typedef struct FFHipH264ResPic {           /* _dev: device pointers, _host: host pointers; 80 bytes */
    uint8_t *dst[3];                       /* as FFHipH264InterPic: Cb and Cr both NULL = monochrome */
    ptrdiff_t dst_stride[3];               /* bytes; base and stride multiples of 4 samples, stride >= the plane's width */
    const FFHipH264BsMb  *mb;              /* mb_w * mb_h raster: flags bit 0 intra, bit 1 8x8 transform, nnz */
    const FFHipH264ResMb *res;             /* mb_w * mb_h raster, 4-byte aligned */
    const void *coeffs;                    /* int16_t at 8 bits, int32_t above; 16-byte aligned; never written */
    int64_t ncoeffs;
} FFHipH264ResPic;
/** npics pictures of mb_w x mb_h macroblocks (1..4096 each) at bit_depth 8, 9, 10, 12 or 14 (uint16_t samples above 8; strides stay
 *  in bytes), chroma_format_idc 0 (Cb / Cr ignored) or 1.  Pictures go 16 to a launch.  Asynchronous on `stream`: behind
 *  ffhip_h264_inter_pictures_dev and ahead of ffhip_h264_edge_params_pictures_dev and the deblock faces with no synchronisation.
 *  FFHIP_ENOSYS (with a text) for chroma_format_idc 2 or 3.
 *  FFHIP_EINVAL for another depth, format or size, npics <= 0, NULL pics, dst[0], mb, res or coeffs, only one of Cb / Cr, a dst base
 *  or stride that is not a multiple of 4 samples, a stride below the plane's width, a res that is not 4-byte or a coeffs that is not
 *  16-byte aligned, a negative ncoeffs, or an overlap: two destination planes of the call that share a byte of a row (the row rule of
 *  ffhip_h264_inter_pictures_dev: the two fields of one frame in one call are accepted), or a coeffs, mb or res span that shares a
 *  byte with a destination span of the call.  FFHIP_ENOSYS without a device (after the argument checks). */
int ffhip_h264_residual_pictures_dev(int bit_depth, int chroma_format_idc, int mb_w, int mb_h, int npics,
                                     const FFHipH264ResPic *pics /* host array */, void *stream);
/** The same rules compiled for the CPU, on host arrays (device-free): the same arguments, refusals but FFHIP_ENOSYS without a
 *  device, and bytes.  The _dev face never calls it. */
int ffhip_h264_residual_pictures_host(int bit_depth, int chroma_format_idc, int mb_w, int mb_h, int npics, const FFHipH264ResPic *pics);

/**
 * The two faces above at every chroma format: chroma_format_idc 0 .. 3.  The existing four entry points keep their behaviour; for
 * chroma_format_idc 0 and 1 the _fmt faces give their bytes and return values (the same launcher, the same kernel instantiation).
 * The records are the same; the chroma planes are 8*mb_w x 8*mb_h at 4:2:0, 8*mb_w x 16*mb_h at 4:2:2 and 16*mb_w x 16*mb_h at 4:4:4,
 * and that size is the one of the stride minimum, of the spans and of the row-overlap rule.  Cb and Cr both NULL: luma only, at
 * every format.
 *
 * ffhip_h264_inter_pictures_fmt_dev: rules 1, 2, 3 and 5 to 10 of ffhip_h264_inter_pictures_dev; rule 4 by format, for the 4x4 luma
 * block at (bx, by) in 4x4 units:
 *  4a. chroma_format_idc 1: rule 4 as it stands (the block's 2x2 chroma block at (2*bx, 2*by)).
 *  4b. chroma_format_idc 2: the block owns the chroma block 2 wide x 4 tall at (2*bx, 4*by) of each chroma plane.  Per list
 *      cx = mvx, cy = mvy; origin the sample's position plus (cx >> 3, cy >> 2); h264chroma's put with the fractions
 *      (cx & 7, (cy << 1) & 7) (mc_dir_part with ysh = 2); coordinates clamped to 8*mb_w x 16*mb_h.  ref.chroma_dy is not read: the
 *      reference applies it at 4:2:0 alone.  The lists combine by rules 5 to 9 with the chroma values.
 *  4c. chroma_format_idc 3: Cb and Cr have luma's geometry: every sample of plane 1 + c is rule 3 (h264qpel with the luma vector and
 *      the luma clamps) on ref.base[1 + c] / ref.stride[1 + c], and the lists combine by rules 5 to 9 with the CHROMA values
 *      (chroma_weight, chroma_log2_denom, use_weight_chroma under rule 8), which the reference hands to the luma-width weight
 *      functions.  ref.chroma_dy is not read.
 * FFHIP_EINVAL for a chroma_format_idc outside 0 .. 3 and for everything ffhip_h264_inter_pictures_dev refuses, with the format's
 * plane sizes; FFHIP_ENOSYS without a device (after the argument checks).
 */
int ffhip_h264_inter_pictures_fmt_dev(int bit_depth, int chroma_format_idc, int mb_w, int mb_h, int npics,
                                      const FFHipH264InterPic *pics /* host array */, void *stream);
/** The same rules compiled for the CPU (device-free): every pointer of the records is a host pointer; the same arguments, refusals
 *  but FFHIP_ENOSYS, and bytes, at chroma_format_idc 0 .. 3.  The _dev face never calls it. */
int ffhip_h264_inter_pictures_fmt_host(int bit_depth, int chroma_format_idc, int mb_w, int mb_h, int npics, const FFHipH264InterPic *pics);
/**
 * ffhip_h264_residual_pictures_fmt_dev: rules 1 to 12 of ffhip_h264_residual_pictures_dev, and by format:
 * 13. chroma_format_idc 0 / 1: r.chroma_lo422 is not read.
 * 14. chroma_format_idc 2: a chroma plane has eight 4x4 blocks j = x + 2*y (x 0..1, y 0..3) at (4x, 4y) of the macroblock's 8 x 16
 *     chroma; Cb block j lies at 256 + 16*j, Cr block j at 512 + 16*j (sl->mb at 4:2:2).  The bits of blocks 0..3 are r.chroma's, those
 *     of blocks 4..7 r.chroma_lo422's (bit j - 4 Cb, bit 4 + (j - 4) Cr).  need (rule 2) is 768 where the picture has chroma planes and
 *     r.chroma | r.chroma_lo422 | r.chroma_dc is non-zero.  With the plane's chroma_dc bit the eight first coefficients go through
 *     chroma422_dc_dequant_idct with r.qmul[c] in the reference's unsigned arithmetic, truncated to the coefficient type, and all
 *     eight blocks are added by rule 6; without it rule 7 runs over the eight blocks.
 * 15. chroma_format_idc 3: plane p (0, 1, 2) is a luma plane whose coefficients lie at 256*p + the luma layout; rules 4, 5 and 9 run
 *     per plane with the plane's own bits: m.nnz for plane 0, the low 16 bits of r.nnz444[0] / [1] for planes 1 / 2, in m.nnz's layout
 *     and under its contract (with the 8x8 flag the four bits of an 8x8 block are equal).  The 8x8 flag of m.flags holds for all three
 *     planes.  r.chroma, r.chroma_dc and r.chroma_lo422 are not read.  need is 768 where the picture has chroma planes and
 *     (nnz444[0] | nnz444[1]) & 0xFFFF is non-zero, else 256 if m.nnz is non-zero, else 0; without chroma planes nnz444 is ignored.
 * FFHIP_EINVAL for a chroma_format_idc outside 0 .. 3 and for everything ffhip_h264_residual_pictures_dev refuses, with the format's
 * plane sizes; FFHIP_ENOSYS without a device (after the argument checks).
 * Out of scope at every format: MBAFF, the lossless bypass, luma DC / I_PCM.  The FFHipH264Edge tables of every format are
 * ffhip_h264_edge_params_pictures_fmt_dev's and the filter ffhip_h264_deblock_pictures_fmt_dev's (above), behind this face and
 * ffhip_h264_inter_pictures_fmt_dev on the same stream.
 */
int ffhip_h264_residual_pictures_fmt_dev(int bit_depth, int chroma_format_idc, int mb_w, int mb_h, int npics,
                                         const FFHipH264ResPic *pics /* host array */, void *stream);
/** The same rules compiled for the CPU, on host arrays (device-free).  The _dev face never calls it. */
int ffhip_h264_residual_pictures_fmt_host(int bit_depth, int chroma_format_idc, int mb_w, int mb_h, int npics, const FFHipH264ResPic *pics);
/** sizeof(FFHipH264ResMb), sizeof(FFHipH264ResPic), for bindings that mirror the records (no device needed). */
int ffhip_h264_res_mb_record_size(void);
int ffhip_h264_res_pic_record_size(void);

/**
 * The batched faces above at ANY depth the reference instantiates (bit_depth 8 / 9 / 10 / 12 / 14), plus the members that exist
 * only here: MBAFF and 4:2:2.  Above 8 bits samples are uint16_t and coefficients int32_t (libavcodec/bit_depth_template.c);
 * strides and offsets stay in BYTES, coefficient pitches in coefficients.  Bit-exact restatement of the reference's templates
 * (h264idct_template.c, h264addpx_template.c, h264dsp_template.c, h264qpel_template.c, h264chroma_template.c) with the depth as a
 * kernel argument; the 8-bit kernels above remain the fast path of 8-bit 4:2:0 streams.
 *   idct_add:     kinds FFHIP_H264_IDCT4 .. ADD_PIXELS8_CLEAR, n x (16 | 64) coefficients
 *   idct_mb:      which 0 idct_add16, 1 idct8_add4, 2 idct_add16intra (one plane: dst2 unused), 3 idct_add8 (4:2:0: Cb = dst_base,
 *                 Cr = dst2, 768 coefficients and a 15 x 8 cache per macroblock), 4 idct_add8_422
 *   dc_dequant:   which 0 luma_dc_dequant_idct (input + m*in_pitch -> the DC positions of output + m*out_pitch), 1 chroma_dc_dequant_idct,
 *                 2 chroma422_dc_dequant_idct (in place on output + block_offset[m])
 *   loop_filter:  FFHipH264Edge.pad = lines per tc0 entry (0: the plain member: luma 4, chroma 2; MBAFF: luma 2, chroma 1;
 *                 4:2:2 h_loop_filter_chroma422: 4, its MBAFF form 2); alpha / beta at the 8-bit scale, as the decoder's tables hold them
 */
int ffhip_h264_idct_add_batch_dev_hbd(int bit_depth, int kind, uint8_t *dst_base, ptrdiff_t stride, const int32_t *dst_offset, int16_t *blocks,
                                      int n, void *stream);
int ffhip_h264_idct_mb_batch_dev_hbd(int bit_depth, int which, uint8_t *dst_base, uint8_t *dst2, ptrdiff_t stride, const int32_t *mb_offset,
                                     const int32_t *blockoffset, int16_t *blocks, const uint8_t *nnzc, int nmb, void *stream);
int ffhip_h264_dc_dequant_batch_dev_hbd(int bit_depth, int which, int16_t *output, size_t out_pitch, const int16_t *input, size_t in_pitch,
                                        const int32_t *block_offset, const int32_t *qmul, int n, void *stream);
int ffhip_h264_loop_filter_batch_dev_hbd(int bit_depth, uint8_t *base, ptrdiff_t stride, const FFHipH264Edge *edges, int n, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* libavcodec: h264qpel                                                                       */
/* ------------------------------------------------------------------------------------------ */
/** qpel_mc_func (libavcodec/qpeldsp.h:65-67) and H264QpelContext (libavcodec/h264qpel.h:27-30). */
typedef void (*ffhip_qpel_mc_func)(uint8_t *dst, const uint8_t *src, ptrdiff_t stride);
typedef struct FFHipH264QpelContext {
    ffhip_qpel_mc_func put_h264_qpel_pixels_tab[3][16];
    ffhip_qpel_mc_func avg_h264_qpel_pixels_tab[3][16];
} FFHipH264QpelContext;
int ff_h264qpel_init_hip(FFHipH264QpelContext *c, int bit_depth);

/** One motion-compensated block of the batch face (what mc_dir_part() passes, h264_mb.c:206-250).
 *
 *  Edge emulation (round 4).  The reference allocates no border around a picture: when the 6-tap footprint of a block leaves the
 *  reference picture, mc_dir_part() copies it through h->vdsp.emulated_edge_mc() (libavcodec/videodsp_template.c:24-100: samples
 *  outside the picture repeat the nearest one inside) and filters from that copy (h264_mb.c:229-247 luma, :297-317 chroma).  A record
 *  says the same with FFHIP_MC_EMU in `flags`: src_offset then addresses sample (0, 0) of the reference PICTURE (pic->data[plane] -
 *  ref base), (src_x, src_y) is the integer-sample position of the block's origin in that picture — any value, also far outside —
 *  and the kernel reads footprint sample (x, y) at row clamp(y, 0, pic_h - 1), column clamp(x, 0, pic_w - 1): emulated_edge_mc's
 *  result, sample for sample (its whole-block-outside cases included, :37-56), for the 21 x 21 window the decoder copies as for any
 *  other.  pic_w / pic_h are those of the plane (luma: 16 * mb_width, 16 * mb_height; 4:2:0 chroma: half), handed to the *_pic
 *  entry points (the picture object knows them).  A record without the flag is read unclamped, as before. */
#define FFHIP_MC_EMU 1
typedef struct FFHipQpelBlock {
    int32_t dst_offset;  /* into dst plane                                            */
    int32_t src_offset;  /* into ref plane: integer-pel position of the block origin; FFHIP_MC_EMU: of the reference picture's (0, 0) */
    uint8_t mcxy;        /* luma_xy = (mx&3) + ((my&3)<<2)                            */
    uint8_t size_idx;    /* 0: 16x16, 1: 8x8, 2: 4x4                                   */
    uint8_t avg;         /* 0 put, 1 avg                                              */
    uint8_t flags;       /* FFHIP_MC_EMU                                              */
    int16_t src_x, src_y;/* FFHIP_MC_EMU: block origin in the reference picture, integer samples (else unused, 0) */
} FFHipQpelBlock;        /* sizeof == 16 */
/** n blocks, one stride for src & dst (as qpel_mc_func); dst blocks must not overlap. src must be
 *  readable 2 px left/up and 3 px right/down of each block (records flagged FFHIP_MC_EMU are not honoured here: use the _pic form). */
int ffhip_h264_qpel_batch_dev(uint8_t *dst, const uint8_t *src, ptrdiff_t stride,
                              const FFHipQpelBlock *blocks, int n, void *stream);
/** The same with the reference pictures' dimensions (samples of this plane): records flagged FFHIP_MC_EMU read their footprint
 *  through clamped coordinates, and only samples inside a reference picture are ever touched for them. */
int ffhip_h264_qpel_batch_dev_pic(uint8_t *dst, const uint8_t *src, ptrdiff_t stride, int pic_w, int pic_h,
                                  const FFHipQpelBlock *blocks, int n, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* libavcodec: h264chroma + explicit weighted prediction (the first "next" row) */
/* ------------------------------------------------------------------------------------------ */
/** h264_chroma_mc_func and H264ChromaContext (libavcodec/h264chroma.h:25-32): tab index 0 = 8 wide, 1 = 4, 2 = 2
 *  (ff_h264chroma_init, libavcodec/h264chroma.c:38-52); x, y are the eighth-pel fractions. */
typedef void (*ffhip_h264_chroma_mc_func)(uint8_t *dst, const uint8_t *src, ptrdiff_t srcStride, int h, int x, int y);
typedef struct FFHipH264ChromaContext {
    ffhip_h264_chroma_mc_func put_h264_chroma_pixels_tab[4];
    ffhip_h264_chroma_mc_func avg_h264_chroma_pixels_tab[4];
} FFHipH264ChromaContext;
/** Fills entries 0..2 (entry 3, the 1-wide VP9 helper, is left untouched).  8-bit only. */
int ff_h264chroma_init_hip(FFHipH264ChromaContext *c, int bit_depth);

/** One chroma MC call of the batch face (what mc_dir_part() passes to chroma_op, h264_mb.c:270-300).  FFHIP_MC_EMU as for
 *  FFHipQpelBlock: the (w + 1) x (h + 1) samples are read at clamped coordinates of the reference picture's chroma plane
 *  (emulated_edge_mc(…, 9, 8 * chroma_idc + 1, mx >> 3, my >> ysh, pic_width >> 1, pic_height >> 1), h264_mb.c:297-317). */
typedef struct FFHipChromaBlock {
    int32_t dst_offset, src_offset;
    uint8_t w_idx;       /* 0: 8 wide, 1: 4, 2: 2 */
    uint8_t h;           /* rows, <= 16            */
    uint8_t x, y;        /* eighth-pel fractions   */
    uint8_t avg, flags;  /* flags: FFHIP_MC_EMU    */
    int16_t src_x, src_y;/* FFHIP_MC_EMU: block origin in the reference picture's plane, integer samples */
    int16_t pad;
} FFHipChromaBlock;      /* sizeof == 20 */
int ffhip_h264_chroma_mc_batch_dev(uint8_t *dst, const uint8_t *src, ptrdiff_t stride, const FFHipChromaBlock *blocks, int n,
                                   void *stream);
int ffhip_h264_chroma_mc_batch_dev_pic(uint8_t *dst, const uint8_t *src, ptrdiff_t stride, int pic_w, int pic_h,
                                       const FFHipChromaBlock *blocks, int n, void *stream);

/** h264_weight_func / h264_biweight_func (libavcodec/h264dsp.h:31-37) and the two tables of H264DSPContext
 *  (:44-45): index 0 = 16 wide, 1 = 8, 2 = 4, 3 = 2 (libavcodec/h264dsp.c:100-107). */
typedef void (*ffhip_h264_weight_func)(uint8_t *block, ptrdiff_t stride, int height, int log2_denom, int weight, int offset);
typedef void (*ffhip_h264_biweight_func)(uint8_t *dst, uint8_t *src, ptrdiff_t stride, int height, int log2_denom, int weightd,
                                         int weights, int offset);
typedef struct FFHipH264WeightContext {
    ffhip_h264_weight_func   weight_pixels_tab[4];
    ffhip_h264_biweight_func biweight_pixels_tab[4];
} FFHipH264WeightContext;
int ff_h264dsp_weight_init_hip(FFHipH264WeightContext *c, int bit_depth);

/** One weight (bi == 0: dst only, weightd = the weight) or biweight call of the batch face. */
typedef struct FFHipWeightBlock {
    int32_t dst_offset, src_offset;
    uint8_t w_idx;       /* 0: 16 wide, 1: 8, 2: 4, 3: 2 */
    uint8_t height, log2_denom, bi;
    int16_t weightd, weights, offset, pad;
} FFHipWeightBlock;
int ffhip_h264_weight_batch_dev(uint8_t *dst, const uint8_t *src, ptrdiff_t stride, const FFHipWeightBlock *blocks, int n,
                                void *stream);
/** qpel / chroma MC / weighted prediction at bit_depth 8 / 9 / 10 / 12 / 14 (16-bit samples above 8; offsets and stride in bytes):
 *  h264qpel.c:87-103, h264chroma.c:38-52, h264dsp.c:102-109 at the depth. */
int ffhip_h264_qpel_batch_dev_hbd(int bit_depth, uint8_t *dst, const uint8_t *src, ptrdiff_t stride, const FFHipQpelBlock *blocks, int n,
                                  void *stream);
int ffhip_h264_chroma_mc_batch_dev_hbd(int bit_depth, uint8_t *dst, const uint8_t *src, ptrdiff_t stride, const FFHipChromaBlock *blocks, int n,
                                       void *stream);
int ffhip_h264_weight_batch_dev_hbd(int bit_depth, uint8_t *dst, const uint8_t *src, ptrdiff_t stride, const FFHipWeightBlock *blocks, int n,
                                    void *stream);
/** ... and their FFHIP_MC_EMU forms: pic_w / pic_h in samples of the plane. */
int ffhip_h264_qpel_batch_dev_hbd_pic(int bit_depth, uint8_t *dst, const uint8_t *src, ptrdiff_t stride, int pic_w, int pic_h,
                                      const FFHipQpelBlock *blocks, int n, void *stream);
int ffhip_h264_chroma_mc_batch_dev_hbd_pic(int bit_depth, uint8_t *dst, const uint8_t *src, ptrdiff_t stride, int pic_w, int pic_h,
                                           const FFHipChromaBlock *blocks, int n, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* libavcodec: caller-side batching for the H.264 macroblock loop           */
/* ------------------------------------------------------------------------------------------ */
/**
 * A picture's worth of per-block dsp calls, recorded on the host while the decoder parses the picture and run as a handful of
 * launches.  The record functions take the operands hl_decode_mb() passes to the dsp pointers (libavcodec/h264_mb_template.c:41-270,
 * h264_mb.c:206-420,612-800) and ff_h264_filter_mb() computes (h264_loopfilter.c:716); flush() runs, per plane,
 *     MC put -> picture | MC put -> bi-prediction scratch | MC avg -> picture | weight / biweight | IDCT + add |
 *     intra macroblocks (reconstruction wavefront, all three planes) | deblock (decoder order)
 * ffhip_h264_picture_create(): 4:2:0, 8 bits; the other depths and chroma formats: ffhip_h264_picture_create_hbd / _fmt below.  All planes
 * of the picture, of the references and the scratch share one stride per plane (qpel_mc_func has one).
 * ref[pl] is the base the blocks' src_offset counts from — typically the decoded-picture-buffer allocation, so that one base
 * reaches every reference picture.  One object serves one stream; begin() starts the next picture (flush() does not clear).
 */
typedef struct FFHipH264Picture FFHipH264Picture;
#define FFHIP_H264_MC_PUT 0   /* put into the picture                                              */
#define FFHIP_H264_MC_TMP 1   /* put into the bi-prediction scratch plane (sl->bipred_scratchpad)  */
#define FFHIP_H264_MC_AVG 2   /* avg onto the picture: the second list of an unweighted bi-prediction */
int  ffhip_h264_picture_create(FFHipH264Picture **p, int mb_w, int mb_h);
/** The same object for a High 10 / High 4:2:0 picture of bit_depth 9 / 10 / 12 / 14 (8: == ffhip_h264_picture_create): planes hold
 *  uint16_t samples, offsets and strides stay in BYTES (as the decoder's linesize / block_offset << pixel_shift), the blocks handed to
 *  idct_add() hold int32_t coefficients (dctcoef, libavcodec/bit_depth_template.c:39-50; sl->mb as the decoder keeps it), edge records
 *  keep alpha / beta / tc0 at the 8-bit scale (the kernels scale them as h264dsp_template.c:108-110 does), intra macroblocks hand
 *  over sl->mb / sl->mb_luma_dc / sl->intra_pcm_ptr as ffhip_h264_intra_pack_hbd() describes.  Planes and strides 8-byte aligned. */
int  ffhip_h264_picture_create_hbd(FFHipH264Picture **p, int mb_w, int mb_h, int bit_depth);
/** The same object for a picture of sps->chroma_format_idc 1 (4:2:0: == ffhip_h264_picture_create_hbd), 2 (4:2:2) or 3 (4:4:4) (round 4),
 *  at any of the depths.
 *  A 4:2:2 picture (hl_decode_mb() with block_h = 16, hl_motion_422: h264_mb_template.c:41-262,172) keeps the 4:2:0 record calls with 8 x 16
 *  chroma: ffhip_h264_picture_mc_chroma() blocks of up to 16 rows (the decoder's `height`, y fraction (my << 1) & 7: h264_mb.c:289-317), the
 *  8-wide weights over 16 rows, ffhip_h264_picture_idct_mb() which 3 = ff_h264_idct_add8_422 (eight blocks per plane after the decoder's own
 *  chroma422_dc_dequant_idct), SIX edge records per macroblock and chroma plane (the vertical edges x = 0, 4 — h_loop_filter_chroma422, 16
 *  lines, tc0 per 4 — then the horizontal ones y = 0, 4, 8, 12); ffhip_h264_picture_intra_mb() is the same call (qmul[1], qmul[2] =
 *  dequant4_coeff[1 + p][chroma_qp[p] + 3][0]; 512 I_PCM fields) and becomes a luma-only record plus an FFHipH264IntraC422.  flush() runs the
 *  luma plane through the luma kernels and the chroma planes' two dependency chains through plain kernels of their own, beside the luma
 *  ones on the object's second stream (ffhip_h264_pictures_flush(): the chroma planes of all pictures side by side in one launch); Cb and Cr
 *  share a stride when the picture has intra macroblocks.
 *  A 4:4:4 picture is what hl_decode_mb_444() (libavcodec/h264_mb_template.c:256-362) makes of it: three planes of luma geometry,
 *  all reconstructed by the LUMA members —
 *    prediction: qpix_op[luma_xy] on dest_cb / dest_cr with the luma vector (mc_dir_part(), h264_mb.c:262-288), weights of the luma width
 *                (mc_part_weighted(), :362-366): ffhip_h264_picture_mc_luma_plane() / ffhip_h264_picture_weight() with plane 1 / 2;
 *                ffhip_h264_picture_mc_chroma() is refused;
 *    residual:   idct_add16 / idct8_add4 per plane on sl->mb + 256 p with the cache rows of plane p (hl_decode_mb_idct_luma(..., p),
 *                h264_mb.c:735-800): ffhip_h264_picture_idct_mb() which 0 / 1 with plane p; which 3 (idct_add8) is refused;
 *    intra:      hl_decode_mb_predict_luma(..., p) for p = 0, 1, 2 with ONE set of prediction modes (h264_mb.c:614-733):
 *                ffhip_h264_picture_intra_mb() takes the decoder's arrays as for 4:2:0 — mb_luma_dc = sl->mb_luma_dc[0], the [3][16 * 2]
 *                int16 array as it stands (plane p's DCs 32 int16 further at every depth, libavcodec/h264dec.h), pcm = the 768 fields —
 *                and splits the macroblock into three luma-only records; flush() runs the three planes' wavefronts side by side in one
 *                launch;
 *    deblocking: filter_mb_edgev / filter_mb_edgeh on img_cb / img_cr (h264_loopfilter.c:601-703): ffhip_h264_picture_deblock_mb() takes 8
 *                luma-kind edge records for every plane.
 *  The three planes share one stride when the picture carries intra macroblocks (the decoder's linesize == uvlinesize there).
 *  chroma_format_idc 0 (monochrome) makes the 4:2:0 object: the decoder reconstructs such a picture as 4:2:0 with mid-grey chroma through the
 *  ordinary members (h264_mb_template.c:112-148); an I_PCM macroblock's record carries mid-grey chroma fields (the FFmpeg-side recorder
 *  appends them). */
int  ffhip_h264_picture_create_fmt(FFHipH264Picture **p, int mb_w, int mb_h, int bit_depth, int chroma_format_idc);
void ffhip_h264_picture_free(FFHipH264Picture **p);
void ffhip_h264_picture_begin(FFHipH264Picture *p);
/** mc_dir_part(): qpix_op[luma_xy] and chroma_op (h264_mb.c:206-300); blk->avg is set from `stage`. */
int  ffhip_h264_picture_mc_luma(FFHipH264Picture *p, int stage, const FFHipQpelBlock *blk);
/** ... on plane 0 (== mc_luma), or on Cb / Cr of a 4:4:4 picture (offsets into that plane and that plane of the references). */
int  ffhip_h264_picture_mc_luma_plane(FFHipH264Picture *p, int plane, int stage, const FFHipQpelBlock *blk);
int  ffhip_h264_picture_mc_chroma(FFHipH264Picture *p, int plane /* 1 Cb, 2 Cr */, int stage, const FFHipChromaBlock *blk);
/** mc_part_weighted(): weight_op / biweight_op (h264_mb.c:340-420); a biweight's src_offset addresses the scratch plane. */
int  ffhip_h264_picture_weight(FFHipH264Picture *p, int plane, const FFHipWeightBlock *blk);
/** idct_add / idct8_add / idct_dc_add / idct8_dc_add: the 16 / 64 coefficients are copied and the caller's block is consumed
 *  exactly as the dsp function does (zeroed; dc forms: block[0] = 0). */
int  ffhip_h264_picture_idct_add(FFHipH264Picture *p, int plane, int kind, int32_t dst_offset, int16_t *block);
/** The macroblock-level residual members of an INTER macroblock as hl_decode_mb() calls them (libavcodec/h264_mb.c:780-797,
 *  h264_mb_template.c:254-257): which 0 = idct_add16, 1 = idct8_add4 (plane's dst_offset[0]), 3 = idct_add8 (4:2:0; dst_offset[0] Cb,
 *  [1] Cr, `plane` ignored; block = sl->mb).  Expanded on the host into idct_add records the way the dsp functions dispatch
 *  (h264idct_template.c:176-228: nnz == 1 with a DC -> the dc form, …); block_offset is h->block_offset (bytes), nnzc the pointer the
 *  member is handed (sl->non_zero_count_cache); `block` is consumed as those functions consume it. */
int  ffhip_h264_picture_idct_mb(FFHipH264Picture *p, int which, int plane, const int32_t dst_offset[2], const int *block_offset, int16_t *block,
                                const uint8_t *nnzc);
/** ff_h264_filter_mb(): the macroblock's edge records, 8 for luma ((dir * 4 + e)), 4 for a chroma plane ((dir * 2 + e)); 4:4:4: 8 for
 *  every plane, luma kinds. */
int  ffhip_h264_picture_deblock_mb(FFHipH264Picture *p, int plane, int mb_x, int mb_y, const FFHipH264Edge *edges);
/**
 * An INTRA macroblock: what hl_decode_mb() does for IS_INTRA(mb_type) (libavcodec/h264_mb_template.c:137-262 with
 * hl_decode_mb_predict_luma / hl_decode_mb_idct_luma, libavcodec/h264_mb.c:612-760) as ONE record.  Intra prediction reads the
 * reconstructed, not yet deblocked samples of the left / top-left / top / top-right macroblocks and chains through the residual
 * add from block to block, so these records are not a batch of independent calls: flush() runs them as a reconstruction
 * WAVEFRONT (one wave per macroblock row; an intra macroblock starts when the row above has finished the macroblock up and to the
 * right) after the inter macroblocks' prediction and residual stages and before deblocking — the order of the reference's
 * data flow, whose in-loop filter runs behind reconstruction on samples intra prediction never sees (xchg_mb_border,
 * h264_mb.c:528-597).  Fields are the decoder's H264SliceContext state of the macroblock.  Frame macroblocks, or the field macroblocks of
 * a field picture whose object was made for the field (mb_y = the row inside the field); 4:2:2 / 4:4:4: ffhip_h264_picture_create_fmt();
 * the lossless transform bypass (a macroblock with qscale 0 in a stream with sps->transform_bypass; round 6, 8 bits, 4:2:0 and 4:4:4): the
 * caller sets FFHIP_H264_INTRA_BYPASS (and _DPCM under profile_idc 244) in `flags` — see below.
 */
#define FFHIP_H264_INTRA_16x16 0   /* IS_INTRA16x16(mb_type)                                                         */
#define FFHIP_H264_INTRA_4x4   1   /* IS_INTRA4x4(mb_type) && !IS_8x8DCT(mb_type)                                    */
#define FFHIP_H264_INTRA_8x8   2   /* IS_INTRA4x4(mb_type) &&  IS_8x8DCT(mb_type): pred8x8l + the 8x8 transform      */
#define FFHIP_H264_INTRA_PCM   3   /* IS_INTRA_PCM(mb_type): sl->intra_pcm_ptr's 384 bytes                            */
#define FFHIP_H264_INTRA_LUMA_DC 1 /* flags, set by ffhip_h264_picture_intra_mb() from the cache: nnz[scan8[LUMA_DC_BLOCK_INDEX]] */
#define FFHIP_H264_INTRA_CB_DC   2 /*   nnz[scan8[CHROMA_DC_BLOCK_INDEX + 0]] */
#define FFHIP_H264_INTRA_CR_DC   4 /*   nnz[scan8[CHROMA_DC_BLOCK_INDEX + 1]] */
/* flags the CALLER sets (every other bit of `flags` zero on entry): the macroblock is decoded with the transform bypassed
 * (hl_decode_mb()'s transform_bypass: sl->qscale == 0 && sps->transform_bypass, h264_mb_template.c:51) — its "coefficients" are residual
 * samples, added to the prediction as add_pixels4 / 8_clear add them (modulo 256, h264addpx_template.c:30-74), no DC transforms;
 * _DPCM (sps->profile_idc == 244): blocks predicted vertically / horizontally take the pred*_add forms (h264pred_template.c:1067-1330,
 * h264_mb.c:638-672,745-750, h264_mb_template.c:198-207): every sample is its neighbour along the direction plus its residual — the packer
 * turns those residuals into running sums along the direction, which makes them ordinary residuals of the V / H prediction. */
#define FFHIP_H264_INTRA_BYPASS  8
#define FFHIP_H264_INTRA_DPCM    16
typedef struct FFHipH264IntraMB {
    int16_t  mb_x, mb_y;
    uint8_t  type;            /* FFHIP_H264_INTRA_*                                                                  */
    uint8_t  pred16;          /* sl->intra16x16_pred_mode (after ff_h264_check_intra_pred_mode)                      */
    uint8_t  chroma_pred;     /* sl->chroma_pred_mode (likewise)                                                     */
    uint8_t  cbp;             /* sl->cbp & 0x3f                                                                      */
    uint16_t topleft_avail;   /* sl->topleft_samples_available  (h264_mvpred.h:599-639)                              */
    uint16_t topright_avail;  /* sl->topright_samples_available                                                      */
    uint8_t  pred4[16];       /* sl->intra4x4_pred_mode_cache[scan8[i]], i = 0..15 (8x8: entries 0, 4, 8, 12)        */
    int32_t  qmul[3];         /* pps->dequant4_coeff[0][qscale][0], [1][chroma_qp[0]][0], [2][chroma_qp[1]][0]       */
    /* ---- filled in by ffhip_h264_picture_intra_mb() ---- */
    uint8_t  flags;           /* in: 0, or FFHIP_H264_INTRA_BYPASS [| _DPCM]; out: + FFHIP_H264_INTRA_LUMA_DC | _CB_DC | _CR_DC */
    uint8_t  pad[3];          /* pad[0], out: how many regions of the macroblock (a luma block, the 16x16 block, a chroma plane) were DPCM-coded */
    uint8_t  nnz[24];         /* non_zero_count_cache[scan8[i]]: luma i = 0..15, Cb 16..19 at [16..19], Cr 32..35 at [20..23] */
    int32_t  coef;            /* the macroblock's run in the picture's packed coefficient array (int16 units)         */
    uint32_t blocks;          /* which blocks the run holds, in this order: bit i luma block i (8x8: bits 0, 4, 8, 12, 64
                                 coefficients each), bit 16 + k Cb block k, bit 20 + k Cr block k                     */
    int16_t  luma_dc[16];     /* sl->mb_luma_dc[0] (Intra16x16)                                                      */
} FFHipH264IntraMB;           /* sizeof == 108 */
/** The chroma planes of an intra macroblock of a 4:2:2 picture, as ffhip_h264_picture_intra_mb() records them on a picture made with
 *  chroma_format_idc 2 (its luma is a luma-only FFHipH264IntraMB): pred8x16 by chroma_pred_mode on both planes, chroma422_dc_dequant_idct
 *  + idct_add8_422 when cbp & 0x30 (libavcodec/h264_mb_template.c:151-262, h264idct_template.c:230-252,295-321).  Exported through
 *  ffhip_h264_picture_lists(). */
typedef struct FFHipH264IntraC422 {
    int16_t  mb_x, mb_y;
    uint8_t  type;        /* FFHIP_H264_INTRA_PCM: the run holds 2 x 128 samples; anything else: prediction + residual */
    uint8_t  chroma_pred; /* sl->chroma_pred_mode (after ff_h264_check_intra_pred_mode)                                */
    uint8_t  cbp;         /* sl->cbp & 0x30                                                                            */
    uint8_t  flags;       /* bit p: nnz[scan8[CHROMA_DC_BLOCK_INDEX + p]] — the plane's DC block is coded             */
    int32_t  qmul[2];     /* pps->dequant4_coeff[1 + p][sl->chroma_qp[p] + 3][0]                                       */
    uint16_t full;        /* bit 8 p + k: block k of plane p has a non-zero count (idct_add; else idct_dc_add if its DC != 0) */
    uint16_t blocks;      /* bit 8 p + k: block k of plane p travels in the run (16 coefficients each, in bit order)   */
    int32_t  coef;        /* the run's start in the packed coefficient array (int16 units)                             */
    int32_t  pad[2];
} FFHipH264IntraC422;     /* sizeof == 32 */
/** Records one intra macroblock: *mb with the fields above `flags` set.  non_zero_count_cache: the decoder's 15 x 8 cache
 *  (scan8 indexing, libavcodec/h264_parse.h:40-57).  mb: sl->mb (3 x 256 int16; Cb at 256, Cr at 512), CONSUMED the way the dsp
 *  functions hl_decode_mb() calls consume it (blocks zeroed after idct_add, [0] after idct_dc_add).  mb_luma_dc: sl->mb_luma_dc[0]
 *  (Intra16x16 with a coded DC block, else may be NULL).  pcm: sl->intra_pcm_ptr (FFHIP_H264_INTRA_PCM, else NULL). */
int  ffhip_h264_picture_intra_mb(FFHipH264Picture *p, const FFHipH264IntraMB *mb_desc, const uint8_t *non_zero_count_cache,
                                 int16_t *mb, const int16_t *mb_luma_dc, const uint8_t *pcm);
/** The host side of the record alone (no device involved; ffhip_h264_picture_intra_mb() is this + an append): fills the fields
 *  from `flags` down and appends the macroblock's coefficient run to coefs[*ncoefs ...] (capacity `cap` int16; a run is at most
 *  391 of them), advancing *ncoefs.  FFHIP_ENOMEM when the run does not fit. */
int  ffhip_h264_intra_pack(FFHipH264IntraMB *rec, const uint8_t *non_zero_count_cache, int16_t *mb, const int16_t *mb_luma_dc,
                           const uint8_t *pcm, int16_t *coefs, int32_t *ncoefs, int32_t cap);
/** The same at bit_depth 9 / 10 / 12 / 14 (8: == ffhip_h264_intra_pack; what ffhip_h264_picture_intra_mb() runs on a picture made by
 *  ffhip_h264_picture_create_hbd()): mb and mb_luma_dc are the decoder's arrays AS THEY STAND at that depth — 3 x 256 and 16 int32
 *  (dctcoef, libavcodec/bit_depth_template.c:39-50) behind the int16_t pointers sl->mb / sl->mb_luma_dc are declared with; pcm is
 *  sl->intra_pcm_ptr, 384 bit_depth-bit fields (h264_mb_template.c:100-131), unpacked here into uint16_t samples.  coefs, *ncoefs, cap
 *  and rec->coef keep counting int16 entries (a run is at most 807 of them); an Intra16x16 macroblock's sixteen luma DCs lead its run
 *  (rec->luma_dc stays zero: it cannot hold them). */
int  ffhip_h264_intra_pack_hbd(int bit_depth, FFHipH264IntraMB *rec, const uint8_t *non_zero_count_cache, int16_t *mb,
                               const int16_t *mb_luma_dc, const uint8_t *pcm, int16_t *coefs, int32_t *ncoefs, int32_t cap);
/** One PLANE of a 4:4:4 macroblock as a luma-only record (what ffhip_h264_picture_intra_mb() does three times on a 4:4:4 picture): the
 *  arguments are plane p's slices of the decoder's arrays — non_zero_count_cache + 5 * 8 * p (scan8[i + 16 p] == scan8[i] + 40 p, the DC
 *  entry scan8[LUMA_DC_BLOCK_INDEX + p] == 40 p), sl->mb + 256 p dctcoef, sl->mb_luma_dc[p], the plane's 256 I_PCM fields — and
 *  rec->qmul[0] = pps->dequant4_coeff[p][p ? sl->chroma_qp[p - 1] : sl->qscale][0] (hl_decode_mb_predict_luma, h264_mb.c:626,712).  The
 *  record's chroma fields are cleared; an I_PCM run keeps its 4:2:0 length (the last third zero). */
int  ffhip_h264_intra_pack_plane(int bit_depth, FFHipH264IntraMB *rec, const uint8_t *non_zero_count_cache, int16_t *mb, const int16_t *mb_luma_dc,
                                 const uint8_t *pcm, int16_t *coefs, int32_t *ncoefs, int32_t cap);
/** The intra reconstruction wavefront alone, on records already in device memory (what flush() launches): recs sorted by
 *  (mb_y, mb_x), row_start[mb_h + 1] indexes them by macroblock row, coefs is the packed coefficient array.  Planes and strides
 *  4-byte aligned.  Asynchronous on `stream`; a lost hand-off is reported by the next flush / ffhip_stream_synchronize. */
int  ffhip_h264_intra_frame_dev(uint8_t *y, uint8_t *cb, uint8_t *cr, ptrdiff_t stride_y, ptrdiff_t stride_c, int mb_w, int mb_h,
                                const FFHipH264IntraMB *recs, const int32_t *row_start, const int16_t *coefs, void *stream);
/** The same on uint16_t samples at bit_depth 9 / 10 / 12 / 14 (records and runs as ffhip_h264_intra_pack_hbd() leaves them; strides in
 *  bytes; planes and strides 8-byte aligned). */
int  ffhip_h264_intra_frame_dev_hbd(int bit_depth, uint8_t *y, uint8_t *cb, uint8_t *cr, ptrdiff_t stride_y, ptrdiff_t stride_c, int mb_w,
                                    int mb_h, const FFHipH264IntraMB *recs, const int32_t *row_start, const int16_t *coefs, void *stream);
/** N pictures' wavefronts in ONE launch (round 4): pictures of one geometry and depth, each with its own planes, sorted records, row
 *  starts and coefficient runs (all device pointers, as for the call above).  A wavefront's latency is its dependency chain (mb_w +
 *  2 mb_h macroblock steps: 2.6 ms for a 1080p I-picture) and one picture occupies 68 of the chip's 8,192 wave slots — a decoder that
 *  holds several pictures (frame threads, an all-intra stream) gets them reconstructed side by side for the latency of one.  Launches
 *  of 32 pictures; asynchronous on `stream`. */
typedef struct FFHipH264IntraPic {
    uint8_t *y, *cb, *cr;
    const FFHipH264IntraMB *recs;
    const int32_t *row_start;
    const int16_t *coefs;
} FFHipH264IntraPic;
int  ffhip_h264_intra_frames_dev(int bit_depth, int npics, const FFHipH264IntraPic *pics /* host array */, ptrdiff_t stride_y,
                                 ptrdiff_t stride_c, int mb_w, int mb_h, void *stream);
/** The same where every entry is ONE PLANE of a 4:4:4 picture: y = the plane, recs / row_start / coefs = that plane's luma-only records
 *  (ffhip_h264_intra_pack_plane); cb / cr are not touched (pass y). */
int  ffhip_h264_intra_planes_dev(int bit_depth, int nplanes, const FFHipH264IntraPic *planes /* host array */, ptrdiff_t stride, int mb_w, int mb_h,
                                 void *stream);
/** What has been recorded since begin(), as it stands: the lists flush() copies to the device, by the stage and plane it runs them in
 *  (pointers into the object, valid until the next record call or begin(); a list with no entry may be NULL).  Recording needs no HIP
 *  device — ffhip_h264_picture_create*() succeed without one and only flush() returns FFHIP_ENOSYS then — so a decoder's macroblock loop
 *  over the recording members can be checked on any machine (tests/test_h264_picture_cpu.py runs the lists through the oracle's dsp
 *  functions in flush()'s order and compares with the reference's own decode).
 *    qpel[plane][stage]  luma-table MC (4:2:0: plane 0 only), stage FFHIP_H264_MC_PUT / _TMP / _AVG
 *    cmc[plane - 1][stage]  chroma MC of Cb / Cr (4:2:0)
 *    wt[plane]           weight / biweight calls (a biweight's src_offset addresses the plane's bi-prediction scratch)
 *    idct_off / idct_coef[plane][kind]  residual blocks by FFHIP_H264_IDCT4 / IDCT8 / IDCT4_DC / IDCT8_DC: nidct offsets, 16 or 64 dctcoef each
 *    intra[set] / intra_coef[set]  intra macroblock records in recording order and their packed runs (int16 units): set 0 = whole
 *                        macroblocks (4:2:0), or one luma-only set per plane (4:4:4)
 *    edges[plane]        mb_w * mb_h * (8 | 4 | 6) edge records (zero records = not filtered), NULL when the plane has none; a 4:2:2
 *                        chroma plane: 6 per macroblock — the vertical edges at x = 0, 4 (16 lines, tc0 per 4 lines), then the horizontal
 *                        ones at y = 0, 4, 8, 12 */
typedef struct FFHipH264PictureLists {
    int mb_w, mb_h, bit_depth, chroma_format_idc;
    const FFHipQpelBlock *qpel[3][3];
    int nqpel[3][3];
    const FFHipChromaBlock *cmc[2][3];
    int ncmc[2][3];
    const FFHipWeightBlock *wt[3];
    int nwt[3];
    const int32_t *idct_off[3][4];
    const int16_t *idct_coef[3][4];
    int nidct[3][4];
    const FFHipH264IntraMB *intra[3];
    int nintra[3];
    const int16_t *intra_coef[3];
    int nintra_coef[3];
    const FFHipH264Edge *edges[3];
    /* 4:2:2: the chroma planes of the intra macroblocks (their luma: intra[0], luma-only) and their packed runs (int16 units) */
    const FFHipH264IntraC422 *intra_c422;
    int nintra_c422;
    const int16_t *intra_c422_coef;
    int nintra_c422_coef;
    /* the lossless bypass of inter macroblocks (round 6): add_pixels4_clear ([pl][0], 16 dctcoef each) / add_pixels8_clear ([pl][1], 64)
     * calls — ffhip_h264_picture_idct_add() kinds FFHIP_H264_ADD_PIXELS4_CLEAR / 8_CLEAR */
    const int32_t *addpx_off[3][2];
    const int16_t *addpx_coef[3][2];
    int naddpx[3][2];
} FFHipH264PictureLists;
int  ffhip_h264_picture_lists(const FFHipH264Picture *p, FFHipH264PictureLists *out);
/** One host-to-device copy of everything recorded since begin(), then the launches; asynchronous on `stream`. */
int  ffhip_h264_picture_flush(FFHipH264Picture *p, uint8_t *const dst[3], const int stride[3], const uint8_t *const ref[3],
                              void *stream);
/* ---- MBAFF frames (round 6): mb_adaptive_frame_field_flag, 4:2:0, 8 - 14 bits ------------------------------------------------------------
 * A frame whose macroblock pairs mix frame and field macroblocks (libavcodec/h264_mb_template.c:61-78, h264_loopfilter.c:494-560,716-760)
 * is recorded into FOUR objects over the same planes (integration/avcodec_h264_picture_hip.c does it):
 *   - three ordinary FFHipH264Picture objects for the INTER macroblocks' prediction, weight and residual lists: the frame macroblocks
 *     (mb_w x mb_h, the frame's line sizes), the top-field macroblocks and the bottom-field macroblocks (each mb_w x mb_h / 2 at TWICE the
 *     line sizes, the bottom one's planes one frame line further down) — a field macroblock of a pair is the field-picture case, which is
 *     how hl_decode_mb() addresses it; flush each with ffhip_h264_picture_flush() (they hold no intra macroblocks and no edges);
 *   - one FFHipH264Mbaff for the two chains whose order crosses macroblocks: the intra macroblocks (decoding order: pair rows, pairs
 *     left to right, top then bottom macroblock) and the in-loop filter's dsp calls, recorded call by call in the order
 *     ff_h264_filter_mb() issues them.  ffhip_h264_mbaff_flush() runs the intra reconstruction, then the filter, and goes LAST.
 */
typedef struct FFHipH264Mbaff FFHipH264Mbaff;
/** mb_w x mb_h: the frame's macroblocks (mb_h even).  FFHIP_EINVAL otherwise.  _fmt: bit_depth 8 / 9 / 10 / 12 / 14 (above 8: uint16_t samples,
 *  the decoder's arrays as they stand at that depth — see ffhip_h264_intra_pack_hbd()); 4:2:0 at every depth. */
int  ffhip_h264_mbaff_create(FFHipH264Mbaff **m, int mb_w, int mb_h);
int  ffhip_h264_mbaff_create_fmt(FFHipH264Mbaff **m, int mb_w, int mb_h, int bit_depth);
void ffhip_h264_mbaff_free(FFHipH264Mbaff **m);
void ffhip_h264_mbaff_begin(FFHipH264Mbaff *m);
/** One intra macroblock, as ffhip_h264_picture_intra_mb(): desc->mb_x, desc->mb_y = the macroblock's position in the FRAME (mb_y odd: the
 *  bottom macroblock of its pair); field != 0: a field macroblock (MB_FIELD(sl)) — its lines are every second frame line from the pair's
 *  line (mb_y & 1) on.  Macroblocks must arrive in decoding order. */
int  ffhip_h264_mbaff_intra_mb(FFHipH264Mbaff *m, const FFHipH264IntraMB *desc, int field, const uint8_t *non_zero_count_cache, int16_t *mb,
                               const int16_t *mb_luma_dc, const uint8_t *pcm);
/** One loop-filter dsp call of macroblock (mb_x, mb_y) on `plane` (0 luma, 1 Cb, 2 Cr), as the H264DSPContext member received it:
 *  call->offset = pix - the plane's first sample (a multiple of 4), call->kind = FFHIP_H264_LF_* of the member, alpha, beta, tc0, and in
 *  call->pad the flags below.  Calls arrive in the order ff_h264_filter_mb() issues them, macroblock by macroblock in decoding order. */
#define FFHIP_H264_LF_CALL_FIELD 1 /* the member was called with twice the plane's line size (a field macroblock's lines)              */
#define FFHIP_H264_LF_CALL_MBAFF 2 /* the _mbaff member: h264_h_loop_filter_luma_mbaff[_intra] (8 lines), _chroma_mbaff[_intra] (4 lines) */
int  ffhip_h264_mbaff_filter_call(FFHipH264Mbaff *m, int plane, int mb_x, int mb_y, const FFHipH264Edge *call);
/** What has been recorded since begin(), as flush() uploads it (host pointers, valid until the next record call): the CPU tier's list
 *  executor (oracle/emul_h264_mbaff.cpp) runs these. */
typedef struct FFHipH264MbaffLists {
    int mb_w, mb_h;
    const FFHipH264IntraMB *recs;   /* nrecs intra macroblocks in decoding order */
    const uint32_t *geo;            /* per record: mb_x | mb_y << 12 | field << 24 */
    const int16_t *coefs;           /* their packed runs (ncoefs int16) */
    const int32_t *intra_row;       /* mb_h / 2 + 1 starts into recs, by pair row */
    int32_t nrecs, ncoefs;
    const FFHipH264Edge *calls[3];  /* per plane: the calls in order */
    const int32_t *pair_end[3];     /* per plane and pair (row-major, mb_w x mb_h / 2): one past the pair's last call */
    int32_t ncalls[3];
    int bit_depth;
} FFHipH264MbaffLists;
int  ffhip_h264_mbaff_lists(FFHipH264Mbaff *m, FFHipH264MbaffLists *out);
/** The intra reconstruction (one wave per pair row, the tile and phases of every other picture's intra macroblocks at the
 *  macroblock's own line step), then the recorded filter calls in order (one wave per pair row and plane; pair x of row p after pair x + 1
 *  of row p - 1).  dst[] / stride[]: the FRAME's planes and line sizes (4-byte aligned; Cb and Cr share a line size).  Call after the
 *  three inter objects' flushes on the same stream.  Above 8 bits planes and line sizes are 8-byte aligned.  Asynchronous on `stream` once the
 *  lists are uploaded. */
int  ffhip_h264_mbaff_flush(FFHipH264Mbaff *m, uint8_t *const dst[3], const int stride[3], void *stream);

/** n picture objects (one geometry, depth and device; the pictures a decoder's frame threads hold at once) flushed TOGETHER (round 4):
 *  dst[3 i + pl] / ref[3 i + pl] are picture i's planes and reference bases, stride[] is shared.  Every picture's staging copy,
 *  prediction and residual launches are its own; the two stages that are a latency chain per picture — the intra reconstruction
 *  wavefront and the in-loop filter — run ONCE for all pictures, side by side (launches of up to 32 pictures; planes and strides
 *  16-byte aligned when any picture carries deblocking records).  The result per picture is flush()'s.  Asynchronous on `stream`. */
int  ffhip_h264_pictures_flush(FFHipH264Picture *const *pics, int n, uint8_t *const *dst, const int stride[3], const uint8_t *const *ref,
                               void *stream);
/** What the picture's last flush came to: 0, or the FFHIP_E* that left ITS planes incomplete.  When one picture of a
 *  ffhip_h264_pictures_flush() batch fails on the host side (staging memory, a malformed record) the others are still finished — their
 *  prediction and residual stages were queued against their planes already — and the call returns the first failure: this says which
 *  pictures it was.  A failure of a stage the pictures share marks every picture of the batch.
 *  A picture object takes records from ONE thread at a time (the record calls are plain appends): a decoder with several slice threads
 *  working on one picture gives each a recorder and serialises the calls into the shared object, or records slice by slice. */
int  ffhip_h264_picture_status(const FFHipH264Picture *p);

/* ------------------------------------------------------------------------------------------ */
/* libavcodec: AACDecDSP.imdct_and_windowing — float decoder, 1024-sample frames */
/* ------------------------------------------------------------------------------------------ */
/** AACDecDSP.imdct_and_windowing (libavcodec/aac/aacdec.h:488, body libavcodec/aac/aacdec_dsp_template.c:325-387): the inverse
 *  MDCT(s) of a channel's frame, the window and the overlap-add with the previous frame's tail.  The context owns the two inverse
 *  MDCTs (created with the scales ff_aac_decode_init() gives them, aacdec.c:1267-1285) and a device copy of the four window tables
 *  the decoder already holds (ff_sine_1024 / ff_sine_128, libavcodec/sinewin.h; ff_aac_kbd_long_1024 / ff_aac_kbd_short_128,
 *  libavcodec/aactab.h) — handed over by the caller, so that the tables in use are the decoder's own bit for bit. */
typedef struct FFHipAacImdct FFHipAacImdct;
int  ffhip_aac_imdct_create(FFHipAacImdct **c, const float *sine_1024, const float *sine_128, const float *kbd_long_1024,
                            const float *kbd_short_128, float scale_1024, float scale_128);
/** The same for the other frame lengths: 960 (AACDecDSP.imdct_and_windowing_960, aacdec_dsp_template.c:453-512; DAB+ / DRM) and 768
 *  (_768, :389-448); the tables are sine_<len>, sine_<len / 8>, the KBD windows of alpha 4 / 6 at those sizes, the scales those of
 *  mdct960 / mdct120 resp. mdct768 / mdct96 (aacdec.c:1278-1284).  Row pitches stay those of the 1024 case — coeffs / out rows 1024
 *  floats (sce->coeffs / sce->output are that wide whatever the frame length; a short window's coefficients sit 128 apart in a 960
 *  frame, 96 apart in a 768 one, as the reference reads them), saved 512 per channel — of which the first len / len / len / 2 are
 *  used.  Long-term prediction exists at 1024 only. */
int  ffhip_aac_imdct_create_len(FFHipAacImdct **c, int frame_len, const float *sine_long, const float *sine_short, const float *kbd_long,
                                const float *kbd_short, float scale_long, float scale_short);
void ffhip_aac_imdct_free(FFHipAacImdct **c);
/** One channel, one frame, host pointers: the member's effect on sce->coeffs / ics.window_sequence[2] / ics.use_kb_window[2]
 *  ([0] this frame, [1] the previous one) / sce->saved (512 floats in and out) / sce->output (1024 floats). */
int  ffhip_aac_imdct_and_windowing(FFHipAacImdct *c, const float *coeffs, const int window_sequence[2], const int use_kb_window[2],
                                   float *saved, float *out);
/** nframes consecutive frames of nch channels, device pointers, frame-major: coeffs / out [nframes][nch][1024], saved [nch][512]
 *  in and out.  window_sequence / use_kb_window [nframes][nch] and the state before the first frame, prev_* [nch], are HOST arrays
 *  (the decoder parses them; enum WindowSequence values, libavcodec/aac.h:63-68).  All frames are processed in parallel: the
 *  overlap state a frame leaves behind depends on that frame alone.  Asynchronous on `stream`; the host arrays may be released on
 *  return.  Not reentrant per context. */
int  ffhip_aac_imdct_and_windowing_batch_dev(FFHipAacImdct *c, const float *coeffs, float *out, float *saved,
                                             const uint8_t *window_sequence, const uint8_t *use_kb_window, const uint8_t *prev_sequence,
                                             const uint8_t *prev_kb_window, int nch, int nframes, void *stream);

/** AACDecDSP.apply_tns (libavcodec/aac/aacdec.h, body aacdec_dsp_template.c:164-223), float: one record per TNS filter with a
 *  non-empty range.  coef[] holds the transmitted reflection coefficients (TemporalNoiseShaping.coef[w][filt]); the LPC
 *  coefficients are derived on the device as the reference derives them (compute_lpc_coefs, lpc_functions.h:54-103). */
typedef struct FFHipAacTnsFilter {
    int32_t frame;      /* channel-frame the filter belongs to: coeffs + frame * 1024 */
    int16_t start;      /* first coefficient filtered (index into the frame, window offset included) */
    int16_t size;       /* number of coefficients */
    int8_t  inc;        /* +1 upwards, -1 downwards (TemporalNoiseShaping.direction) */
    uint8_t order;      /* 1..20 (TNS_MAX_ORDER) */
    uint8_t pad[2];
    float   coef[20];   /* sizeof == 92 */
} FFHipAacTnsFilter;
/** apply_tns's walk over windows and filters for one channel-frame (host side, from the parsed TemporalNoiseShaping and the
 *  IndividualChannelStream fields it reads); writes at most 32 records, returns their number. */
int ffhip_aac_tns_filters(FFHipAacTnsFilter *out, int frame, const int n_filt[8], const int length[8][4], const int direction[8][4],
                          const int order[8][4], const float coef[8][4][20], int num_windows, int num_swb, const uint16_t *swb_offset,
                          int tns_max_bands, int max_sfb);
/** The filters of a batch of channel-frames, in place on coeffs [nframes][1024] (device); filters is a device array.  decode != 0:
 *  the decoder's all-pole filter; 0: the moving-average form of the LTP path (apply_ltp, aacdec_dsp_template.c:252-282).  The
 *  filters of a frame cover disjoint ranges, so all of them run concurrently. */
int ffhip_aac_apply_tns_batch_dev(float *coeffs, const FFHipAacTnsFilter *filters, int nfilters, int decode, void *stream);

/** AACDecDSP.apply_prediction (AAC Main's backward-adaptive predictors; aacdec_dsp_template.c:636-664, aacdec_float_prediction.h):
 *  one record per channel-frame, one thread per predictor.  predictor_state: device array [channels][672] of PredictorState (8 floats:
 *  cor0 cor1 var0 var1 r0 r1 k1 x_est, libavcodec/aac_defines.h:130-139), carried from frame to frame by the caller — so a batch is
 *  one frame of many channels.  The host helper folds predictor_present / prediction_used[] / ff_aac_pred_sfb_max[] / swb_offset into
 *  the per-coefficient enable bits. */
enum { FFHIP_AAC_PRED_LONG = 1,          /* window_sequence[0] != EIGHT_SHORT_SEQUENCE (else: all predictors are reset) */
       FFHIP_AAC_PRED_RESET_FIRST = 2 }; /* ics.predictor_initialized was 0 */
typedef struct FFHipAacPrediction {
    int32_t  channel;      /* predictor_state + channel * 672 * 8 */
    int32_t  frame;        /* coeffs + frame * 1024 */
    int16_t  kmax;         /* swb_offset[pred_sfb_max]: predictors 0 .. kmax - 1 run */
    uint8_t  flags;
    uint8_t  reset_group;  /* ics.predictor_reset_group (0: none) */
    uint32_t enable[21];   /* bit k: coeffs[k] += prediction */
    uint32_t pad;          /* sizeof == 100 */
} FFHipAacPrediction;
int ffhip_aac_prediction_record(FFHipAacPrediction *out, int channel, int frame, int is_long, int initialized, int predictor_present,
                                const uint8_t *prediction_used, int pred_sfb_max, const uint16_t *swb_offset, int reset_group);
int ffhip_aac_apply_prediction_batch_dev(float *predictor_state, float *coeffs, const FFHipAacPrediction *recs, int n, void *stream);

/** AAC-LD and AAC-ELD: AACDecDSP.imdct_and_windowing_ld / _eld (aacdec_dsp_template.c:516-602), float.  eld == 0: 512-sample frames,
 *  w0 = ff_sine_512, w1 = ff_sine_128, scale = mdct512's ((1.0 / 512) / 32768, aacdec.c:1282).  eld != 0: frame_len 512 or 480, w0 =
 *  ff_aac_eld_window_512 / _480 (1920 / 1800 floats, libavcodec/aactab.h:61-63), w1 unused, scale that of mdct512 / mdct480.
 *  Batch: nframes consecutive frames of nch channels, frame-major, device pointers: coeffs / out rows of 1024 floats (the first
 *  frame_len used; the reference's ELD member shuffles sce->coeffs in place — this one leaves them alone), saved [nch][256] (LD) or
 *  [nch][3 * frame_len] (ELD: the three previous frames, newest first) in and out; kb_prev (LD only, HOST array [nframes][nch]) =
 *  ics->use_kb_window[1] of each frame, which selects the low-overlap window.  Asynchronous on `stream`. */
typedef struct FFHipAacLd FFHipAacLd;
int  ffhip_aac_ld_create(FFHipAacLd **c, int eld, int frame_len, const float *w0, const float *w1, float scale);
void ffhip_aac_ld_free(FFHipAacLd **c);
int  ffhip_aac_ld_batch_dev(FFHipAacLd *c, const float *coeffs, float *out, float *saved, const uint8_t *kb_prev, int nch, int nframes,
                            void *stream);

/** AACDecDSP.apply_mid_side_stereo / apply_intensity_stereo (aacdec_dsp_template.c:83-160), float, and the band-wise add that ends
 *  apply_ltp (:276-280): one record per range of coefficients.  The host walks (window groups, scalefactor bands, band types, the
 *  M/S mask — the fields decode_cpe / decode_ics leave in ChannelElement / IndividualChannelStream) produce the records; the ranges
 *  of one channel pair are disjoint (M/S bands have band_type < NOISE_BT, intensity bands 14 / 15), so a pair's M/S and intensity
 *  records — and any number of pairs — run in one launch. */
enum { FFHIP_AAC_BAND_MS = 0,         /* butterflies_float: a, b = a + b, a - b          (libavutil/float_dsp.c:112-122) */
       FFHIP_AAC_BAND_INTENSITY = 1,  /* vector_fmul_scalar: b = a * scale               (libavutil/float_dsp.c:45-51)   */
       FFHIP_AAC_BAND_ADD = 2,        /* a += b                                          (apply_ltp's last loop)         */
       FFHIP_AAC_BAND_FMAC = 3 };     /* a += scale * b   (product rounded, then the sum) (channel coupling)              */
typedef struct FFHipAacBandOp {
    int32_t frame0;     /* a = base_a + frame0 * 1024 + start */
    int32_t frame1;     /* b = base_b + frame1 * 1024 + start */
    int16_t start, len;
    float   scale;
    uint8_t kind;
    uint8_t pad[3];     /* sizeof == 20 */
} FFHipAacBandOp;
/** apply_mid_side_stereo's walk: cpe->ch[0].ics grouping, cpe->max_sfb_ste, cpe->ms_mask, both channels' band_type (enum BandType
 *  as int, 128 entries each).  Writes at most 64 records, returns their number. */
int ffhip_aac_ms_bands(FFHipAacBandOp *out, int frame0, int frame1, int num_window_groups, const uint8_t *group_len, int max_sfb_ste,
                       const uint8_t *ms_mask, const int *band_type0, const int *band_type1, const uint16_t *swb_offset);
/** apply_intensity_stereo's walk: cpe->ch[1].ics grouping and max_sfb, ms_present, cpe->ms_mask, ch[1].band_type and ch[1].sf.
 *  At most 128 records. */
int ffhip_aac_is_bands(FFHipAacBandOp *out, int frame0, int frame1, int num_window_groups, const uint8_t *group_len, int max_sfb,
                       int ms_present, const uint8_t *ms_mask, const int *band_type1, const float *sf1, const uint16_t *swb_offset);
/** apply_ltp's last loop: coeffs[frame] += predFreq[pred_frame] on ltp->used bands below min(max_sfb, MAX_LTP_LONG_SFB).  At most
 *  20 records. */
int ffhip_aac_ltp_bands(FFHipAacBandOp *out, int frame, int pred_frame, int max_sfb, const int8_t *used, const uint16_t *swb_offset);
/** The records of a batch on device arrays a / b of channel-frames (1024 floats each; the same array for the stereo tools,
 *  coeffs / predFreq for the LTP add); ops is a device array. */
int ffhip_aac_band_ops_batch_dev(float *a, float *b, const FFHipAacBandOp *ops, int n, void *stream);
/** AACDecDSP.apply_dependent_coupling (aacdec_float_coupling.h:42-71): the walk over the coupling channel's bands as FMAC records
 *  (dest_frame / src_frame index the same device array of channel-frames; run with ffhip_aac_band_ops_batch_dev(coeffs, coeffs, ..)).
 *  apply_independent_coupling (:78-88) is ONE such record over the output samples: { dest, src, 0, len, gain, FFHIP_AAC_BAND_FMAC }. */
int ffhip_aac_coupling_bands(FFHipAacBandOp *out, int dest_frame, int src_frame, int num_window_groups, const uint8_t *group_len, int max_sfb,
                             const int *band_type, const float *gain, const uint16_t *swb_offset);


/** AACDecDSP.apply_ltp (aacdec_dsp_template.c:252-282) as its three steps: (1) ffhip_aac_ltp_predict_batch_dev — the delayed state
 *  times ltp->coef, windowing_and_mdct_ltp (:225-247) and the forward 1024-point MDCT (created by ffhip_aac_ltp_init with the scale
 *  ff_aac_decode_init gives it, aacdec.c:1288-1291) -> predFreq; (2) ffhip_aac_apply_tns_batch_dev(predFreq, filters, n, 0) when
 *  the channel has TNS; (3) ffhip_aac_band_ops_batch_dev with ffhip_aac_ltp_bands' records.  A frame's prediction needs the
 *  previous frame's output, so a batch is one frame of many channels / streams, not many frames of one. */
typedef struct FFHipAacLtp {
    int32_t state;      /* the channel: ltp_state + state * 3072 */
    int16_t lag;        /* LongTermPrediction.lag (0..2047) */
    uint8_t seq0;       /* ics.window_sequence[0]; never EIGHT_SHORT_SEQUENCE (apply_ltp does nothing there: send no record) */
    uint8_t kb;         /* ics.use_kb_window[0] | use_kb_window[1] << 1 */
    float   coef;       /* LongTermPrediction.coef */
    int32_t pad;        /* sizeof == 16; record r writes pred_freq + r * 1024 */
} FFHipAacLtp;
int ffhip_aac_ltp_init(FFHipAacImdct *c, float scale_ltp);
int ffhip_aac_ltp_predict_batch_dev(FFHipAacImdct *c, const float *ltp_state, float *pred_freq, const FFHipAacLtp *recs, int n, void *stream);
/** AACDecDSP.update_ltp (aacdec_dsp_template.c:287-320) for the nch channels whose frame the preceding
 *  ffhip_aac_imdct_and_windowing_batch_dev call on this context ended with (its inverse-MDCT output — ac->buf_mdct — and overlap
 *  state are still in the context): ltp_state [nch][3072] in and out, out [nch][1024] = that frame's output samples. */
int ffhip_aac_update_ltp_batch_dev(FFHipAacImdct *c, float *ltp_state, const float *out, int nch, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* libavcodec: H264PredContext — H.264 codec, 8 bits, chroma_format_idc <= 1 */
/* ------------------------------------------------------------------------------------------ */
/** H264PredContext (libavcodec/h264pred.h:92-116), the members ff_h264_pred_init() fills for AV_CODEC_ID_H264
 *  (libavcodec/h264pred.c:448-538): same signatures, host pointers, in place on the picture like the C functions.  Mode indices are
 *  the reference's (h264pred.h:35-48 for pred4x4 / pred8x8l, :67-82 for pred8x8 / pred16x16); the _add members are filled at
 *  [VERT_PRED] / [HOR_PRED] resp. [VERT_PRED8x8] / [HOR_PRED8x8] only, as in the reference.  A face reads exactly the neighbours its
 *  C counterpart reads (a DC_128 call touches none). */
typedef struct FFHipH264PredContext {
    void (*pred4x4[9 + 3 + 3])(uint8_t *src, const uint8_t *topright, ptrdiff_t stride);
    void (*pred8x8l[9 + 3])(uint8_t *src, int topleft, int topright, ptrdiff_t stride);
    void (*pred8x8[4 + 3 + 4])(uint8_t *src, ptrdiff_t stride);
    void (*pred16x16[4 + 3 + 2])(uint8_t *src, ptrdiff_t stride);
    void (*pred4x4_add[2])(uint8_t *pix, int16_t *block, ptrdiff_t stride);
    void (*pred8x8l_add[2])(uint8_t *pix, int16_t *block, ptrdiff_t stride);
    void (*pred8x8l_filter_add[2])(uint8_t *pix, int16_t *block, int topleft, int topright, ptrdiff_t stride);
    void (*pred8x8_add[3])(uint8_t *pix, const int *block_offset, int16_t *block, ptrdiff_t stride);
    void (*pred16x16_add[3])(uint8_t *pix, const int *block_offset, int16_t *block, ptrdiff_t stride);
} FFHipH264PredContext;
#define FFHIP_CODEC_ID_H264 27  /* AV_CODEC_ID_H264 (libavcodec/codec_id.h:77) */
#define FFHIP_CODEC_ID_SVQ3 23  /* AV_CODEC_ID_SVQ3, _RV40, _VP8, _VP7 (libavcodec/codec_id.h): the codecs whose decoders share H264PredContext, with their */
#define FFHIP_CODEC_ID_RV40 69  /* own forms of some members at 8 bits (libavcodec/h264pred.c:540-578)                                                    */
#define FFHIP_CODEC_ID_VP8  139
#define FFHIP_CODEC_ID_VP7  178
/** ff_h264_pred_init_<arch>(H264PredContext *, codec_id, bit_depth, chroma_format_idc) shape (libavcodec/h264pred.h:120-127).
 *  bit_depth 8 / 9 / 10 / 12 / 14 (16-bit samples and int32 coefficients of the _add members above 8; the depth is baked into the
 *  installed functions).  chroma_format_idc 0..3: from 2 on pred8x8[] / pred8x8_add[] are the 8 wide x 16 tall forms, as
 *  ff_h264_pred_init() installs them (h264pred.c:478-535).  codec_id: FFHIP_CODEC_ID_H264, or — 8 bits, chroma_format_idc <= 1 — SVQ3 /
 *  RV40 / VP7 / VP8: the table as ff_h264_pred_init() leaves it for that codec (their own forms of pred4x4[] / pred8x8[] / pred16x16[]
 *  members, h264pred.c:540-578; members the reference does not set for the codec — RV40 / VP7 / VP8: pred8x8[]'s four "mad cow" DC
 *  slots, VP8: pred4x4[DC_128_PRED] — are left as they were).  FFHIP_EINVAL for any other codec_id. */
int ff_h264_pred_init_hip(FFHipH264PredContext *h, int codec_id, int bit_depth, int chroma_format_idc);

#define FFHIP_H264_PRED4x4             0  /* pred4x4[mode]                                 */
#define FFHIP_H264_PRED8x8L            1  /* pred8x8l[mode]                                */
#define FFHIP_H264_PRED8x8             2  /* pred8x8[mode]   (chroma, 4:2:0)               */
#define FFHIP_H264_PRED16x16           3  /* pred16x16[mode]                               */
#define FFHIP_H264_PRED4x4_ADD         4  /* pred4x4_add[mode]: mode 0 VERT_PRED, 1 HOR_PRED */
#define FFHIP_H264_PRED8x8L_ADD        5  /* pred8x8l_add[mode]                            */
#define FFHIP_H264_PRED8x8L_FILTER_ADD 6  /* pred8x8l_filter_add[mode]                     */
#define FFHIP_H264_PRED8x16            7  /* pred8x8[mode] at chroma_format_idc 2 (4:2:2): the 8 wide x 16 tall forms */
#define FFHIP_H264_PRED_CODEC          8  /* the forms ff_h264_pred_init() installs for SVQ3 / RV40 / VP7 / VP8 (8 bits): mode = a
                                           * FFHIP_H264_PREDV_* code below, which also says the block size */
/* 4x4 (aux = bytes into the plane of topright[0..3], as for PRED4x4; the RV40 forms without _NODOWN also read the four rows below the
 * block in the left column: LOAD_DOWN_LEFT_EDGE, h264pred.c:141-190) */
#define FFHIP_H264_PREDV_127_DC          0   /* pred4x4_127_dc_c               VP7 / VP8 pred4x4[DC_127_PRED]            */
#define FFHIP_H264_PREDV_129_DC          1   /* pred4x4_129_dc_c                         pred4x4[DC_129_PRED]            */
#define FFHIP_H264_PREDV_VERT_VP8        2   /* pred4x4_vertical_vp8_c                   pred4x4[VERT_PRED]              */
#define FFHIP_H264_PREDV_HOR_VP8         3   /* pred4x4_horizontal_vp8_c                 pred4x4[HOR_PRED]               */
#define FFHIP_H264_PREDV_DL_SVQ3         4   /* pred4x4_down_left_svq3_c       SVQ3      pred4x4[DIAG_DOWN_LEFT_PRED]    */
#define FFHIP_H264_PREDV_DL_RV40         5   /* pred4x4_down_left_rv40_c       RV40      pred4x4[DIAG_DOWN_LEFT_PRED]    */
#define FFHIP_H264_PREDV_DL_RV40_NODOWN  6   /* ..._nodown_c                             pred4x4[DIAG_DOWN_LEFT_PRED_RV40_NODOWN] */
#define FFHIP_H264_PREDV_VL_RV40         7   /* pred4x4_vertical_left_rv40_c             pred4x4[VERT_LEFT_PRED]         */
#define FFHIP_H264_PREDV_VL_RV40_NODOWN  8   /* ..._nodown_c                             pred4x4[VERT_LEFT_PRED_RV40_NODOWN] */
#define FFHIP_H264_PREDV_VL_VP8          9   /* pred4x4_vertical_left_vp8_c    VP7 / VP8 pred4x4[VERT_LEFT_PRED]         */
#define FFHIP_H264_PREDV_HU_RV40         10  /* pred4x4_horizontal_up_rv40_c   RV40      pred4x4[HOR_UP_PRED]            */
#define FFHIP_H264_PREDV_HU_RV40_NODOWN  11  /* ..._nodown_c                             pred4x4[HOR_UP_PRED_RV40_NODOWN] */
#define FFHIP_H264_PREDV_TM_VP8          12  /* pred4x4_tm_vp8_c               VP7 / VP8 pred4x4[TM_VP8_PRED]            */
/* 8x8 (chroma) */
#define FFHIP_H264_PREDV8_DC_RV40        16  /* pred8x8_dc_rv40_c       RV40 / VP7 / VP8 pred8x8[DC_PRED8x8]             */
#define FFHIP_H264_PREDV8_LEFT_DC_RV40   17  /* pred8x8_left_dc_rv40_c                   pred8x8[LEFT_DC_PRED8x8]        */
#define FFHIP_H264_PREDV8_TOP_DC_RV40    18  /* pred8x8_top_dc_rv40_c                    pred8x8[TOP_DC_PRED8x8]         */
#define FFHIP_H264_PREDV8_TM_VP8         19  /* pred8x8_tm_vp8_c               VP7 / VP8 pred8x8[PLANE_PRED8x8]          */
#define FFHIP_H264_PREDV8_127_DC         20  /* pred8x8_127_dc_8_c                       pred8x8[DC_127_PRED8x8]         */
#define FFHIP_H264_PREDV8_129_DC         21  /* pred8x8_129_dc_8_c                       pred8x8[DC_129_PRED8x8]         */
/* 16x16 */
#define FFHIP_H264_PREDV16_PLANE_SVQ3    32  /* pred16x16_plane_svq3_c         SVQ3      pred16x16[PLANE_PRED8x8]        */
#define FFHIP_H264_PREDV16_PLANE_RV40    33  /* pred16x16_plane_rv40_c         RV40      pred16x16[PLANE_PRED8x8]        */
#define FFHIP_H264_PREDV16_TM_VP8        34  /* pred16x16_tm_vp8_c             VP7 / VP8 pred16x16[PLANE_PRED8x8]        */
#define FFHIP_H264_PREDV16_127_DC        35  /* pred16x16_127_dc_8_c                     pred16x16[DC_127_PRED8x8]       */
#define FFHIP_H264_PREDV16_129_DC        36  /* pred16x16_129_dc_8_c                     pred16x16[DC_129_PRED8x8]       */
#define FFHIP_H264_PRED_TOPLEFT   1  /* flags: pred8x8l's has_topleft                                                       */
#define FFHIP_H264_PRED_TOPRIGHT  2  /* flags: pred8x8l's has_topright                                                      */
#define FFHIP_H264_PRED_TR_SPLAT  4  /* flags: pred4x4's topright is src[3 - stride] four times (the decoder's substitute when the
                                        top-right block is unavailable, h264_mb_template.c hl_decode_mb_predict_luma)        */
/** One block of the batch face, predicted in place from its neighbours in the plane. */
typedef struct FFHipH264Pred {
    int32_t offset;   /* bytes into the plane: the block's top-left sample */
    int32_t aux;      /* PRED4x4: bytes into the plane of topright[0..3] (unless TR_SPLAT); the _ADD kinds: index into coeffs of
                         the block's first coefficient */
    uint8_t mode;
    uint8_t flags;
    uint8_t pad[2];   /* sizeof == 12 */
} FFHipH264Pred;
/** n blocks of one kind whose neighbours are final: intra prediction chains through the reconstruction, so a decoder batches
 *  what its wavefront allows (all blocks of a launch are read-before-write independent; a launch orders after the previous one
 *  on the stream).  pred8x8_add / pred16x16_add are 4 / 16 PRED4x4_ADD records at block_offset[], row of blocks by row (VERT) or
 *  column by column (HOR).  coeffs is used (and the blocks' coefficients cleared) by the _ADD kinds only. */
int ffhip_h264_pred_batch_dev(int kind, uint8_t *plane, ptrdiff_t stride, int16_t *coeffs, const FFHipH264Pred *blocks, int n,
                              void *stream);

/* ------------------------------------------------------------------------------------------ */
/* libavutil: AVFloatDSPContext vector operations around the MDCT           */
/* ------------------------------------------------------------------------------------------ */
/** The float members of AVFloatDSPContext an (I)MDCT pipeline uses (libavutil/float_dsp.h:31-175; windowing and
 *  overlap-add of AAC & co: imdct -> vector_fmul_window).  Same signatures, host pointers.  scalarproduct_float is not
 *  offered: its sequential summation order is the result. */
typedef struct FFHipFloatDSPContext {
    void (*vector_fmul)(float *dst, const float *src0, const float *src1, int len);
    void (*vector_fmac_scalar)(float *dst, const float *src, float mul, int len);
    void (*vector_fmul_scalar)(float *dst, const float *src, float mul, int len);
    void (*vector_fmul_window)(float *dst, const float *src0, const float *src1, const float *win, int len);
    void (*vector_fmul_add)(float *dst, const float *src0, const float *src1, const float *src2, int len);
    void (*vector_fmul_reverse)(float *dst, const float *src0, const float *src1, int len);
    void (*butterflies_float)(float *v1, float *v2, int len);
} FFHipFloatDSPContext;
/** ff_float_dsp_init_<arch>(AVFloatDSPContext *) shape (libavutil/float_dsp.c:153-165). */
int ff_float_dsp_init_hip(FFHipFloatDSPContext *c);

#define FFHIP_FDSP_FMUL          0   /* dst = src0 * src1                                                   */
#define FFHIP_FDSP_FMAC_SCALAR   1   /* dst += src0 * mul                                                   */
#define FFHIP_FDSP_FMUL_SCALAR   2   /* dst = src0 * mul                                                    */
#define FFHIP_FDSP_FMUL_WINDOW   3   /* dst[2 len] = window(src0[len], src1[len], win = src2[2 len])        */
#define FFHIP_FDSP_FMUL_ADD      4   /* dst = src0 * src1 + src2                                            */
#define FFHIP_FDSP_FMUL_REVERSE  5   /* dst[i] = src0[i] * src1[len - 1 - i]                                */
#define FFHIP_FDSP_BUTTERFLIES   6   /* (dst, src0) = (dst + src0, dst - src0): src0 is WRITTEN             */
/**
 * nvec independent vectors of len floats (device pointers): vector v of an operand starts pitch bytes after vector
 * v - 1; pitch 0 shares one vector across the batch (a window).  Operands an operation does not use may be NULL.
 * Results are bit-identical to the C reference (no fused multiply-add).
 */
int ffhip_fdsp_batch_dev(int op, float *dst, size_t dst_pitch, const float *src0, size_t pitch0, const float *src1, size_t pitch1,
                         const float *src2, size_t pitch2, float mul, int len, int nvec, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* libavcodec: hevcdsp inverse transforms (north_star's "hevcdsp integer IDCT") */
/* ------------------------------------------------------------------------------------------ */
/** The transform members of HEVCDSPContext (libavcodec/hevc/dsp.h:46-61), 8-bit: index = log2_size - 2.
 *  idct leaves the residual IN PLACE in coeffs (libavcodec/hevc/dsp_template.c:261-284); col_limit bounds the
 *  non-zero coefficient columns/rows exactly as the reference's partial butterflies use it (coefficients beyond it are
 *  ignored, not assumed zero). */
typedef void (*ffhip_hevc_idct_func)(int16_t *coeffs, int col_limit);
typedef void (*ffhip_hevc_idct_dc_func)(int16_t *coeffs);
typedef void (*ffhip_hevc_add_residual_func)(uint8_t *dst, const int16_t *res, ptrdiff_t stride);
/** SAOParams (libavcodec/hevc/dsp.h:34-46), as sao_edge_restore takes it. */
typedef struct FFHipSAOParams {
    int offset_abs[3][4];
    int offset_sign[3][4];
    uint8_t band_position[3];
    int eo_class[3];
    int16_t offset_val[3][5];
    uint8_t type_idx[3];
} FFHipSAOParams;
/** hevc_{h,v}_loop_filter_luma / _chroma (hevc/dsp.h:103-124): 8 sample lines along an edge, two groups of 4 with their own
 *  tc / no_p / no_q.  h_: the edge is horizontal (samples of a line are `stride` apart). */
typedef void (*ffhip_hevc_lf_luma_func)(uint8_t *pix, ptrdiff_t stride, int beta, const int32_t *tc, const uint8_t *no_p,
                                        const uint8_t *no_q);
typedef void (*ffhip_hevc_lf_chroma_func)(uint8_t *pix, ptrdiff_t stride, const int32_t *tc, const uint8_t *no_p, const uint8_t *no_q);
typedef struct FFHipHEVCDSPContext {
    ffhip_hevc_add_residual_func add_residual[4];
    void (*transform_4x4_luma)(int16_t *coeffs);
    ffhip_hevc_idct_func    idct[4];
    ffhip_hevc_idct_dc_func idct_dc[4];
    ffhip_hevc_lf_luma_func   hevc_h_loop_filter_luma, hevc_v_loop_filter_luma;
    ffhip_hevc_lf_chroma_func hevc_h_loop_filter_chroma, hevc_v_loop_filter_chroma;
    ffhip_hevc_lf_luma_func   hevc_h_loop_filter_luma_c, hevc_v_loop_filter_luma_c;     /* the decoder's "_c" slots: same functions */
    ffhip_hevc_lf_chroma_func hevc_h_loop_filter_chroma_c, hevc_v_loop_filter_chroma_c;
    /* sample adaptive offset (hevc/dsp.h:63-69; index = width class 8/16/32/48/64, one function for all).  The edge filter
     * reads its source with the reference's fixed stride of 2*MAX_PB_SIZE + AV_INPUT_BUFFER_PADDING_SIZE = 192 bytes and needs
     * one sample of margin around the block, as in the reference. */
    void (*sao_band_filter[5])(uint8_t *dst, const uint8_t *src, ptrdiff_t stride_dst, ptrdiff_t stride_src, const int16_t *sao_offset_val,
                               int sao_left_class, int width, int height);
    void (*sao_edge_filter[5])(uint8_t *dst, const uint8_t *src, ptrdiff_t stride_dst, const int16_t *sao_offset_val, int eo, int width,
                               int height);
    /* uni-directional motion compensation (hevc/dsp.h:74-77,88-92): [width class][!!my][!!mx]; the plain forms write 14-bit
     * int16 intermediates with a row stride of MAX_PB_SIZE = 64, the _uni forms write pixels */
    void (*put_hevc_qpel[10][2][2])(int16_t *dst, const uint8_t *src, ptrdiff_t srcstride, int height, intptr_t mx, intptr_t my, int width);
    void (*put_hevc_qpel_uni[10][2][2])(uint8_t *dst, ptrdiff_t dststride, const uint8_t *src, ptrdiff_t srcstride, int height, intptr_t mx,
                                        intptr_t my, int width);
    void (*put_hevc_epel[10][2][2])(int16_t *dst, const uint8_t *src, ptrdiff_t srcstride, int height, intptr_t mx, intptr_t my, int width);
    void (*put_hevc_epel_uni[10][2][2])(uint8_t *dst, ptrdiff_t dststride, const uint8_t *src, ptrdiff_t srcstride, int height, intptr_t mx,
                                        intptr_t my, int width);
    /* the small members (hevc/dsp.h:52-54,70-72): transform-skip scaling, RDPCM running sums, SAO border fix-up.  put_pcm reads a
     * bitstream (GetBitContext) and stays with the decoder */
    void (*dequant)(int16_t *coeffs, int16_t log2_size);
    void (*transform_rdpcm)(int16_t *coeffs, int16_t log2_size, int mode);
    void (*sao_edge_restore[2])(uint8_t *dst, const uint8_t *src, ptrdiff_t stride_dst, ptrdiff_t stride_src, const FFHipSAOParams *sao,
                                const int *borders, int width, int height, int c_idx, const uint8_t *vert_edge,
                                const uint8_t *horiz_edge, const uint8_t *diag_edge);
    /* weighted and bi-directional prediction (hevc/dsp.h:78-87,93-101); src2 = the other list's put_hevc_* output (row stride 64) */
    void (*put_hevc_qpel_uni_w[10][2][2])(uint8_t *dst, ptrdiff_t dststride, const uint8_t *src, ptrdiff_t srcstride, int height, int denom,
                                          int wx, int ox, intptr_t mx, intptr_t my, int width);
    void (*put_hevc_qpel_bi[10][2][2])(uint8_t *dst, ptrdiff_t dststride, const uint8_t *src, ptrdiff_t srcstride, const int16_t *src2,
                                       int height, intptr_t mx, intptr_t my, int width);
    void (*put_hevc_qpel_bi_w[10][2][2])(uint8_t *dst, ptrdiff_t dststride, const uint8_t *src, ptrdiff_t srcstride, const int16_t *src2,
                                         int height, int denom, int wx0, int wx1, int ox, intptr_t mx, intptr_t my, int width);
    void (*put_hevc_epel_uni_w[10][2][2])(uint8_t *dst, ptrdiff_t dststride, const uint8_t *src, ptrdiff_t srcstride, int height, int denom,
                                          int wx, int ox, intptr_t mx, intptr_t my, int width);
    void (*put_hevc_epel_bi[10][2][2])(uint8_t *dst, ptrdiff_t dststride, const uint8_t *src, ptrdiff_t srcstride, const int16_t *src2,
                                       int height, intptr_t mx, intptr_t my, int width);
    void (*put_hevc_epel_bi_w[10][2][2])(uint8_t *dst, ptrdiff_t dststride, const uint8_t *src, ptrdiff_t srcstride, const int16_t *src2,
                                         int height, int denom, int wx0, int wx1, int ox, intptr_t mx, intptr_t my, int width);
} FFHipHEVCDSPContext;
/** ff_hevc_dsp_init_<arch> shape (libavcodec/hevc/dsp.h:127-140).  bit_depth 8, 10 or 12 (the depth is baked into the installed
 *  functions, as the reference's per-BIT_DEPTH instantiations are); FFHIP_EINVAL for 9 and above 12: those keep the C pointers. */
int ff_hevc_dsp_init_hip(FFHipHEVCDSPContext *c, int bit_depth);

#define FFHIP_HEVC_IDCT      0   /* idct[log2_size - 2](coeffs, col_limit)     */
#define FFHIP_HEVC_IDCT_DC   1   /* idct_dc[log2_size - 2](coeffs)             */
#define FFHIP_HEVC_DST_4X4   2   /* transform_4x4_luma(coeffs), log2_size == 2 */
#define FFHIP_HEVC_ADD_ONLY  3   /* coeffs already hold the residual           */
#define FFHIP_HEVC_DEQUANT   4   /* dequant(coeffs, log2_size): transform-skip scaling (hevc/dsp_template.c:127-143) */
#define FFHIP_HEVC_RDPCM_H   5   /* transform_rdpcm(coeffs, log2_size, 0): running sums along rows (:85-105)        */
#define FFHIP_HEVC_RDPCM_V   6   /* transform_rdpcm(coeffs, log2_size, 1): running sums down columns                */
/** One transform unit of the batch face: what hls_residual_coding / hls_transform_unit pass per TU
 *  (libavcodec/hevc/cabac.c, hevcdec.c). */
typedef struct FFHipHevcTU {
    int32_t coeff_offset; /* in int16 units into coeffs: the TU's size*size block, row-major.  coeffs + coeff_offset must be
                           * 4-byte aligned (coeff_offset even on an aligned array): the kernels move a block in 16-byte pieces
                           * where it is 16-byte aligned and as dwords otherwise, unit by unit; an odd address is undefined */
    int32_t dst_offset;   /* in bytes into dst; < 0: leave the picture alone                      */
    int32_t col_limit;    /* FFHIP_HEVC_IDCT only                                                 */
} FFHipHevcTU;
/**
 * n transform units of one size and kind: the inverse transform in place in coeffs (device), then, when dst is
 * non-NULL and the TU's dst_offset >= 0, add_residual[log2_size - 2](dst + dst_offset, residual, stride).
 * TUs of one call must not overlap in coeffs or dst.
 */
int ffhip_hevc_idct_batch_dev(int kind, int log2_size, int16_t *coeffs, uint8_t *dst, ptrdiff_t stride,
                              const FFHipHevcTU *tus, int n, void *stream);

#define FFHIP_HEVC_LF_H_LUMA    0
#define FFHIP_HEVC_LF_V_LUMA    1
#define FFHIP_HEVC_LF_H_CHROMA  2
#define FFHIP_HEVC_LF_V_CHROMA  3
/** One edge segment of the batch face: everything a hevc_*_loop_filter_* call takes besides pix/stride. */
typedef struct FFHipHevcEdge {
    int32_t offset;      /* pix = base + offset */
    uint8_t kind;        /* FFHIP_HEVC_LF_* */
    uint8_t beta;        /* luma only (betatable tops out at 64) */
    uint8_t no_p[2], no_q[2];
    int16_t tc[2];
    uint8_t pad[2];      /* sizeof == 16 */
} FFHipHevcEdge;
/**
 * n edge segments whose touched pixels are pairwise DISJOINT.  HEVC deblocking has no order dependency inside one
 * direction (edges lie on an 8x8 grid and change at most 3 samples on either side): a picture is one call with all its
 * vertical edges followed by one call with all its horizontal edges (libavcodec/hevc/filter.c ff_hevc_deblocking_boundary_strengths
 * / deblocking_filter_CTB).
 */
int ffhip_hevc_loop_filter_batch_dev(uint8_t *base, ptrdiff_t stride, const FFHipHevcEdge *edges, int n, void *stream);

/** One prediction block of the batch face: what luma_mc_uni / chroma_mc_uni pass per block (libavcodec/hevc/hevcdec.c). */
typedef struct FFHipHevcMcBlock {
    int32_t dst_offset;   /* uni: bytes into dst; plain: int16 elements into dst (rows are 64 elements apart) */
    int32_t src_offset;   /* bytes into src: the block's integer-sample origin */
    uint8_t width, height;/* 2..64 */
    uint8_t mx, my;       /* luma: quarter-sample 0..3; chroma: eighth-sample 0..7 */
} FFHipHevcMcBlock;
/**
 * n blocks: put_hevc_{qpel,epel}[..][!!my][!!mx] (uni == 0, dst = int16) or put_hevc_{qpel,epel}_uni (uni != 0, dst = pixels with
 * dststride).  src must be readable 3 (chroma: 1) samples left/up and 4 (2) right/down of each block.
 */
int ffhip_hevc_mc_batch_dev(int chroma, int uni, void *dst, ptrdiff_t dststride, const uint8_t *src, ptrdiff_t srcstride,
                            const FFHipHevcMcBlock *blocks, int n, void *stream);

/** Weighted / bi-directional prediction (luma_mc_uni with weights, luma_mc_bi, chroma_mc_bi: libavcodec/hevc/hevcdec.c:1745-1770,
 *  1795-1860, 1975-2040): one record = the operands of one put_hevc_{qpel,epel}_{uni_w,bi,bi_w} call (hevc/dsp.h:78-101). */
#define FFHIP_HEVC_MC_UNI_W 2   /* dst = clip(((v * wx0 + 2^(shift-1)) >> shift) + ox), shift = denom + 6          */
#define FFHIP_HEVC_MC_BI    3   /* dst = clip((v + src2 + 64) >> 7)                                                 */
#define FFHIP_HEVC_MC_BI_W  4   /* dst = clip((v * wx1 + src2 * wx0 + (ox + 1) << log2Wd) >> (log2Wd + 1))         */
typedef struct FFHipHevcMcWBlock {
    int32_t dst_offset;   /* bytes into dst */
    int32_t src_offset;   /* bytes into src: the block's integer-sample origin */
    int32_t src2_offset;  /* int16 elements into src2 (the other list's put_hevc_* output, rows 64 elements apart); unused by uni_w */
    uint8_t width, height;/* 2..64 */
    uint8_t mx, my;       /* luma: quarter-sample 0..3; chroma: eighth-sample 0..7 */
    int16_t wx0, wx1;     /* uni_w: wx0 = wx; bi_w: wx0 weights src2, wx1 weights this block (the reference's argument order) */
    int16_t ox;           /* uni_w: the offset; bi_w: o0 + o1 as the decoder passes it */
    uint8_t denom;        /* log2 weight denominator (0..7 from the slice header; checkasm goes to 12) */
    uint8_t pad;          /* sizeof == 24 */
} FFHipHevcMcWBlock;
int ffhip_hevc_mc_w_batch_dev(int chroma, int mode, uint8_t *dst, ptrdiff_t dststride, const uint8_t *src, ptrdiff_t srcstride,
                              const int16_t *src2, const FFHipHevcMcWBlock *blocks, int n, void *stream);

/** One SAO call of the batch face (a CTB plane or part of one). */
typedef struct FFHipHevcSao {
    int32_t dst_offset, src_offset;  /* into dst / src */
    int16_t offset_val[5];           /* sao_offset_val: [0] unused by the band filter */
    uint8_t edge;                    /* 0: sao_band_filter, 1: sao_edge_filter */
    uint8_t cls;                     /* band: sao_left_class (0..31); edge: eo = SAO_EO_* (0 horizontal, 1 vertical, 2 135 deg, 3 45 deg) */
    uint8_t width, height;           /* 1..64; larger values give undefined sample values (rows are split by a reciprocal table
                                      * that ends at 64 samples), 0 does nothing */
    uint8_t pad[2];                  /* sizeof == 24 */
} FFHipHevcSao;
/** n SAO blocks: dst[..] = clip(src[..] + offset(class)); src and dst are different buffers (the decoder filters from a
 *  copy), blocks do not overlap in dst; the edge filter reads src one sample beyond the block on every side. */
int ffhip_hevc_sao_batch_dev(uint8_t *dst, ptrdiff_t stride_dst, const uint8_t *src, ptrdiff_t stride_src, const FFHipHevcSao *blocks,
                             int n, void *stream);

/** One sao_edge_restore[variant] call of the batch face (libavcodec/hevc/filter.c:440-470 builds the operands). */
typedef struct FFHipHevcSaoRestore {
    int32_t dst_offset, src_offset;
    int16_t offset0;      /* sao->offset_val[c_idx][0]                                              */
    uint8_t width, height;/* 2..64 (the reference indexes column width - 2)                         */
    uint8_t eo;           /* sao->eo_class[c_idx] = SAO_EO_*: 0 horizontal, 1 vertical, 2 135 degrees, 3 45 degrees */
    uint8_t variant;      /* 0: sao_edge_restore[0] (borders only), 1: [1] (+ the restore part)     */
    uint8_t borders;      /* bit i = borders[i] != 0: left, top, right, bottom                     */
    uint8_t vert_edge;    /* bits 0..1 = vert_edge[0..1]                                            */
    uint8_t horiz_edge;   /* bits 0..1                                                              */
    uint8_t diag_edge;    /* bits 0..3                                                              */
    uint8_t pad[2];       /* sizeof == 20                                                           */
} FFHipHevcSaoRestore;
/** n blocks, pairwise disjoint in dst; src and dst as for ffhip_hevc_sao_batch_dev. */
int ffhip_hevc_sao_restore_batch_dev(uint8_t *dst, ptrdiff_t stride_dst, const uint8_t *src, ptrdiff_t stride_src,
                                     const FFHipHevcSaoRestore *blocks, int n, void *stream);

/**
 * hevcdsp above 8 bits (Main10 / Main12 streams): the batch faces above with the BIT_DEPTH the reference instantiates its templates
 * for (libavcodec/hevc/dsp.c:133-196; bit_depth_template.c: pixel = uint16_t, av_clip_pixel to (1 << bit_depth) - 1).  bit_depth
 * 8, 10 or 12; 8 is the face without the suffix.  Records are unchanged: pixel offsets and strides stay in BYTES as in the
 * reference's signatures (16-bit planes 2-byte aligned); beta / tc / SAO offsets / weights are the values the decoder passes —
 * the scaling by << (bit_depth - 8) happens inside, where the reference's templates do it (hevc/dsp_template.c:845,862,907;
 * h2656_inter_template.c:72; dsp_template.c:408).  Coefficients and the put_hevc_* intermediates are int16 at every depth.
 */
int ffhip_hevc_idct_batch_dev_hbd(int bit_depth, int kind, int log2_size, int16_t *coeffs, uint8_t *dst, ptrdiff_t stride,
                                  const FFHipHevcTU *tus, int n, void *stream);
int ffhip_hevc_loop_filter_batch_dev_hbd(int bit_depth, uint8_t *base, ptrdiff_t stride, const FFHipHevcEdge *edges, int n, void *stream);
int ffhip_hevc_sao_batch_dev_hbd(int bit_depth, uint8_t *dst, ptrdiff_t stride_dst, const uint8_t *src, ptrdiff_t stride_src,
                                 const FFHipHevcSao *blocks, int n, void *stream);
int ffhip_hevc_sao_restore_batch_dev_hbd(int bit_depth, uint8_t *dst, ptrdiff_t stride_dst, const uint8_t *src, ptrdiff_t stride_src,
                                         const FFHipHevcSaoRestore *blocks, int n, void *stream);
int ffhip_hevc_mc_batch_dev_hbd(int bit_depth, int chroma, int uni, void *dst, ptrdiff_t dststride, const uint8_t *src, ptrdiff_t srcstride,
                                const FFHipHevcMcBlock *blocks, int n, void *stream);
int ffhip_hevc_mc_w_batch_dev_hbd(int bit_depth, int chroma, int mode, uint8_t *dst, ptrdiff_t dststride, const uint8_t *src,
                                  ptrdiff_t srcstride, const int16_t *src2, const FFHipHevcMcWBlock *blocks, int n, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* libavcodec: HEVC intra prediction (HEVCPredContext)                                         */
/* ------------------------------------------------------------------------------------------ */
/** == HEVCPredContext (libavcodec/hevc/pred.h), member order kept.  Host pointers, pixel = uint8_t at 8 bits and uint16_t above;
 *  strides in bytes.  top[-1 .. 2N-1] and left[-1 .. 2N-1] are the reference samples (N = 4 << index, or 1 << log2_size); top[-1]
 *  and left[-1] both hold the corner, and each face reads the copy hevc/pred_template.c reads at that point.  `top` / `left` may
 *  point into `src`: every input is staged before anything is written.
 *  intra_pred[] is decoder-level (it reads HEVCLocalContext) and is never written here: the reference's C intra_pred() calls the
 *  pred_* members below, so installing these is what routes a decoder's prediction to the device. */
typedef struct FFHipHEVCPredContext {      /* == HEVCPredContext (libavcodec/hevc/pred.h) */
    void *intra_pred[4];                   /* decoder-level (reads HEVCLocalContext): never written by us */
    void (*pred_planar[4])(uint8_t *src, const uint8_t *top, const uint8_t *left, ptrdiff_t stride);
    void (*pred_dc)(uint8_t *src, const uint8_t *top, const uint8_t *left, ptrdiff_t stride, int log2_size, int c_idx);
    void (*pred_angular[4])(uint8_t *src, const uint8_t *top, const uint8_t *left, ptrdiff_t stride, int c_idx, int mode);
} FFHipHEVCPredContext;
/** ff_hevc_pred_init_<arch> shape.  bit_depth 8, 10 or 12 (baked into the installed functions); FFHIP_EINVAL for any other depth
 *  and FFHIP_ENOSYS without a device, both leaving *c untouched.  The members it displaces answer a face that cannot run. */
int ff_hevc_pred_init_hip(FFHipHEVCPredContext *c, int bit_depth);

/** One transform block of the intra batch face.  Its reference line (4N + 1 samples, N = 1 << log2_size) is stored from bottom-left
 *  to top-right, the order substitution walks it:
 *      line[k] = left[2N-1-k] for k < 2N,   line[2N] = the corner,   line[2N+1+x] = top[x] for x < 2N.
 *  Without FFHIP_HEVC_INTRA_RAW the line is what the pred_* members receive (substituted and filtered by the decoder) and the
 *  availability fields are ignored.  With it, the kernel substitutes unavailable samples (H.265 8.4.4.2.2), filters the line
 *  (8.4.4.2.3, strong bi-linear smoothing included), then predicts.  Availability is counted in units: uh samples along the top,
 *  uv samples down the left (1, 2 or 4; the decoder's minimum TU size in this plane), 2N / unit <= 16 on each side.
 *  c_idx and the two unit sizes share a byte so that the record stays 16 bytes. */
#define FFHIP_HEVC_INTRA_RAW        1  /* substitute + filter the line before predicting */
#define FFHIP_HEVC_INTRA_CORNER     2  /* RAW: the corner sample is available */
#define FFHIP_HEVC_INTRA_STRONG     4  /* RAW: sps strong_intra_smoothing_enabled_flag */
#define FFHIP_HEVC_INTRA_NO_SMOOTH  8  /* RAW: sps intra_smoothing_disabled_flag */
#define FFHIP_HEVC_INTRA_CHROMA444 16  /* RAW: ChromaArrayType == 3, chroma lines are filtered too */
typedef struct FFHipHevcIntra {
    int32_t  dst_offset;   /* bytes into dst: the block's top-left sample */
    int32_t  edge_offset;  /* bytes into edges: the block's reference line, 4N + 1 samples */
    uint16_t avail_left;   /* RAW only: bit i = left samples [i*uv, (i+1)*uv) counted from the top are available */
    uint16_t avail_top;    /* RAW only: bit i = top samples [i*uh, (i+1)*uh) counted from the left are available */
    uint8_t  log2_size;    /* 2..5 */
    uint8_t  mode;         /* 0 planar, 1 DC, 2..34 angular */
    uint8_t  flags;        /* FFHIP_HEVC_INTRA_* */
    uint8_t  c_idx_unit;   /* bits 0-1: c_idx (0 luma, 1 / 2 chroma); bits 2-3: log2 uh; bits 4-5: log2 uv (sizeof == 16) */
} FFHipHevcIntra;
/** n blocks at bit_depth 8, 10 or 12 (uint16_t samples above 8; dst, edges and stride then 2-byte aligned, and so are the record
 *  offsets).  Preconditions: blocks are pairwise disjoint in dst; edges does not alias dst; a raw line has 2N >> log2 unit <= 16 on
 *  both sides.  A record with mode > 34, log2_size outside 2..5, or a raw line whose units break that bound writes nothing.
 *  FFHIP_EINVAL for another depth, n < 0, NULL pointers or misaligned 16-bit planes; FFHIP_ENOSYS without a device.
 *  Out of scope: the RExt implicit-RDPCM case that disables the boundary filters (disableIntraBoundaryFilter with
 *  cu_transquant_bypass); the record cannot ask for it, and such blocks stay on the C path. */
int ffhip_hevc_intra_batch_dev(int bit_depth, uint8_t *dst, ptrdiff_t stride, const uint8_t *edges, const FFHipHevcIntra *blocks, int n,
                               void *stream);
/** sizeof(FFHipHevcIntra), for bindings that mirror the record (no device needed). */
int ffhip_hevc_intra_record_size(void);

/** Intra reconstruction of whole pictures in one launch: every intra transform block of a picture is predicted from the picture's
 *  own samples (H.265 8.4.4.2: substitution, filtering, prediction), its residual is added and the sum clipped to
 *  [0, (1 << bit_depth) - 1], in an order that honours HEVC's availability rules: one wave per (picture, plane, CTB row) walks its
 *  row left to right, and CTB x of a row starts once the row above has finished CTB x + 1.
 *  A block's reference samples sit at the same places as for FFHipHevcIntra with FFHIP_HEVC_INTRA_RAW; here they are read from the
 *  plane (as reconstructed so far) instead of an edges buffer.
 *
 *  Contract:
 *  - a sample a record marks available comes earlier in decoding order (6.4.1 z-scan availability, with slices, tiles and
 *    constrained_intra_pred_flag already folded into the masks by the caller);
 *  - samples no record covers (inter CUs, already reconstructed by the MC and residual stages; PCM CUs) are read as the plane holds
 *    them at launch and are never written; bytes outside the picture (the stride padding) are never written;
 *  - the planes are independent chains (intra prediction never crosses planes); monochrome uses plane 0 only;
 *  - 4:2:2 chroma blocks arrive as the two square blocks the decoder predicts, the top one first.
 *  A malformed record — mode > 34, log2_size outside 2..5, x or y not a multiple of 4, a block outside the picture or outside the
 *  CTB it is listed under, unit sizes above 4 or more than 16 units on a side — writes nothing and reads nothing outside its plane.
 *  A record that marks samples available that are not reconstructed yet predicts undefined values, but cannot hang the launch or
 *  touch memory outside its plane.
 *  Out of scope, as for the batch face: the RExt implicit-RDPCM case that disables the boundary filters (cu_transquant_bypass_flag);
 *  such CUs stay on the C path. */
typedef struct FFHipHevcIntraTU {   /* one intra transform block, 16 bytes */
    uint16_t x, y;                  /* its top-left sample in its plane */
    int32_t  res_offset;            /* int16 units into the plane's res: the block's N * N residuals, row-major; < 0: none (cbf 0) */
    uint16_t avail_left;            /* bit i = left samples [i*uv, (i+1)*uv) counted from the top are available (as FFHipHevcIntra) */
    uint16_t avail_top;             /* bit i = top samples [i*uh, (i+1)*uh) counted from the left are available */
    uint8_t  log2_size;             /* 2..5 */
    uint8_t  mode;                  /* 0 planar, 1 DC, 2..34 angular */
    uint8_t  flags;                 /* FFHIP_HEVC_INTRA_CORNER / _STRONG / _NO_SMOOTH / _CHROMA444; _RAW is implied */
    uint8_t  c_idx_unit;            /* as FFHipHevcIntra: bits 0-1 c_idx (it selects the luma-only rules), 2-3 log2 uh, 4-5 log2 uv */
} FFHipHevcIntraTU;
typedef struct FFHipHevcIntraPlane { /* device pointers */
    uint8_t *base;                  /* the plane's top-left sample */
    ptrdiff_t stride;               /* bytes, >= the plane's width in bytes */
    const FFHipHevcIntraTU *tus;    /* sorted by raster CTB address; decoding order inside a CTB */
    const int32_t *ctb_start;       /* ctb_w * ctb_h + 1 entries: the records of raster CTB a are tus[ctb_start[a] .. ctb_start[a + 1]) */
    const int16_t *res;             /* final residuals (after the transform / transform skip / RDPCM / cross-component prediction) */
} FFHipHevcIntraPlane;
typedef struct FFHipHevcIntraPic {
    FFHipHevcIntraPlane plane[3];   /* Y, Cb, Cr; chroma_format_idc 0: plane[0] only */
} FFHipHevcIntraPic;
/** npics pictures of one geometry: width x height luma samples (multiples of 8, at most 65535), CTBs of 1 << log2_ctb_size (4, 5 or 6)
 *  luma samples, bit_depth 8, 10 or 12 (uint16_t samples above 8), chroma_format_idc 0..3.  Every used plane needs non-NULL
 *  pointers; base and stride are multiples of 4 samples (4 bytes at 8 bits, 8 above).  Pictures go 16 to a launch (fewer when the
 *  progress pool cannot hold their CTB rows).  Asynchronous on `stream`; a lost row hand-off is reported by ffhip_stream_synchronize.
 *  FFHIP_EINVAL for another depth, chroma format, CTB or picture size, npics <= 0, NULL or misaligned planes, or more CTB rows than
 *  one progress-pool slot holds; FFHIP_ENOSYS without a device. */
int ffhip_hevc_intra_pictures_dev(int bit_depth, int chroma_format_idc, int width, int height, int log2_ctb_size, int npics,
                                  const FFHipHevcIntraPic *pics /* host array */, void *stream);
/** sizeof(FFHipHevcIntraTU), for bindings that mirror the record (no device needed). */
int ffhip_hevc_intra_tu_record_size(void);

/** Inter reconstruction of whole pictures in one launch: every prediction block of a picture is motion-compensated from its
 *  reference pictures in HBM, then every inter transform block adds its residual (a batching decoder's order: idct batch with
 *  dst = NULL -> inter pictures -> intra pictures -> deblocking -> SAO).  Prediction blocks never read the picture they write, so
 *  there is no dependency chain: one workgroup per (picture, CTB).
 *
 *  Semantics:
 *  - a PU samples its references with the picture-edge clamp of H.265 8.5.3.3.3.1 / .2 (xInt = Clip3(0, pic_width - 1, ...), the
 *    same for rows): the bytes of the reference decoder's emulated_edge_mc path (libavcodec/hevc/hevcdec.c luma_mc_uni,
 *    chroma_mc_uni, luma_mc_bi, chroma_mc_bi).  No padding is read and no window is refused: MVs may point anywhere;
 *  - chroma follows chroma_mc_uni / chroma_mc_bi: mx = av_mod_uintp2(mv.x, 2 + hshift) << (1 - hshift) (an eighth-sample phase),
 *    x_off = x0_c + (mv.x >> (2 + hshift)), the same vertically with vshift, for chroma formats 1, 2 and 3; the chroma block is
 *    (w >> hshift) x (h >> vshift) at (x >> hshift, y >> vshift);
 *  - the reference's operation order: a uni-predicted PU is put_hevc_{qpel,epel}_uni (_uni_w when its slice is weighted), a
 *    bi-predicted one puts list 0 into the 14-bit intermediate and combines list 1 with it through _bi (_bi_w when weighted).  Byte
 *    for byte the reference's output at 8, 10 and 12 bits; weights and offsets are the values hevcdec.c passes, the
 *    << (bit_depth - 8) offset scaling happens inside (h2656_inter_template.c);
 *  - when every PU of a CTB is predicted, the CTB's inter TUs add their residuals and clip to [0, (1 << bit_depth) - 1].  A TU only
 *    changes samples a PU of its CTB covers;
 *  - samples no PU covers (intra CUs, PCM CUs) are never written, nor is anything outside the picture (the stride padding);
 *  - a malformed record writes nothing and reads nothing outside its planes and references: a PU with w or h outside 4..64 or not a
 *    multiple of 4, outside the picture or the CTB it is listed under, flags & 3 == 0, slice >= nslices, ref_idx >= num_ref (or
 *    num_ref > 16), a DPB slot >= nrefs; a TU with log2_size outside 2..5 or outside its CTB or its plane.
 *  Trusted, as by the intra face (the ABI carries no lengths to check them against): the CTB start tables and the records they
 *  index, the slice table entries below nslices, and each TU's res_offset (its N * N residuals must lie inside the plane's res).
 *  The PUs of a CTB must be disjoint, as must the TUs of one plane of a CTB: overlapping ones leave undefined values where they
 *  overlap, inside that CTB, and nothing outside it.
 *  Out of scope: high_precision_offsets_enabled_flag (RExt; the reference's dsp scales offsets by << (bit_depth - 8)
 *  unconditionally, such streams keep the C path), MV derivation (merge / AMVP stay with the decoder) and PCM.  The deblocking
 *  boundary strengths have a face of their own, ffhip_hevc_boundary_strengths_pictures_dev(). */
typedef struct FFHipHevcInterPU {   /* one luma prediction block; it drives every plane, 20 bytes */
    uint16_t x, y;                  /* its top-left luma sample */
    uint8_t  w, h;                  /* 4..64, multiples of 4 (every partition mode, AMP included) */
    uint8_t  flags;                 /* bit 0 predFlagL0, bit 1 predFlagL1 */
    uint8_t  pad;
    uint8_t  ref_idx[2];            /* per list, 0..15: an index into the slice's ref[list] */
    uint16_t slice;                 /* index into the picture's slice table */
    int16_t  mv[2][2];              /* [list][x, y]: quarter-sample luma MVs, final after merge / AMVP */
} FFHipHevcInterPU;
typedef struct FFHipHevcInterTU {   /* one inter transform block of one plane, 12 bytes */
    uint16_t x, y;                  /* its top-left sample in its plane */
    int32_t  res_offset;            /* int16 units into the plane's res: N * N final residuals, row-major; < 0: none */
    uint8_t  log2_size;             /* 2..5; 4:2:2 chroma arrives as the two square blocks */
    uint8_t  pad[3];
} FFHipHevcInterTU;
typedef struct FFHipHevcInterSlice { /* what hls_prediction_unit reads from the slice header, 424 bytes */
    uint8_t  ref[2][16];            /* [list][ref_idx]: the DPB slot (index into FFHipHevcInterPic.ref) of that reference */
    uint8_t  num_ref[2];            /* num_ref_idx_lX_active, 0..16 */
    uint8_t  weighted;              /* P: weighted_pred_flag, B: weighted_bipred_flag (the weight_flag of hevcdec.c) */
    uint8_t  luma_log2_denom, chroma_log2_denom;
    uint8_t  pad[3];
    int16_t  luma_weight[2][16], luma_offset[2][16];             /* sh.luma_weight_lX / luma_offset_lX */
    int16_t  chroma_weight[2][16][2], chroma_offset[2][16][2];   /* sh.chroma_weight_lX / chroma_offset_lX, [.][.][Cb, Cr] */
} FFHipHevcInterSlice;
typedef struct FFHipHevcInterPlane { /* device pointers */
    uint8_t *base;                  /* the plane's top-left sample */
    ptrdiff_t stride;               /* bytes, >= the plane's width in bytes */
    const FFHipHevcInterTU *tus;    /* sorted by raster CTB address */
    const int32_t *tu_ctb_start;    /* ctb_w * ctb_h + 1 entries: the TUs of raster CTB a are tus[tu_ctb_start[a] .. [a + 1]) */
    const int16_t *res;             /* final residuals (transform, transform skip, RDPCM, cross-component prediction, bypass applied) */
} FFHipHevcInterPlane;
typedef struct FFHipHevcInterRef {  /* one DPB picture (device pointers), same geometry and depth as the pictures of the call */
    const uint8_t *base[3];         /* Y, Cb, Cr */
    ptrdiff_t stride[3];            /* bytes */
} FFHipHevcInterRef;
typedef struct FFHipHevcInterPic {
    FFHipHevcInterPlane plane[3];   /* Y, Cb, Cr; chroma_format_idc 0: plane[0] only */
    const FFHipHevcInterPU *pus;    /* device, sorted by raster CTB address */
    const int32_t *pu_ctb_start;    /* device, ctb_w * ctb_h + 1 entries, as tu_ctb_start */
    const FFHipHevcInterSlice *slices; /* device */
    int32_t nslices;
    int32_t nrefs;                  /* 0..16: the DPB slots ref[0 .. nrefs) */
    FFHipHevcInterRef ref[16];      /* in this host array: the face stages it to the device */
} FFHipHevcInterPic;
/** npics pictures of one geometry: width x height luma samples (multiples of 8, at most 65535), CTBs of 1 << log2_ctb_size (4, 5 or 6)
 *  luma samples, bit_depth 8, 10 or 12 (uint16_t samples above 8), chroma_format_idc 0..3.  Every used plane needs non-NULL
 *  pointers, base and stride multiples of 4 samples; reference planes are sample-aligned with a stride of at least the plane's width.
 *  Pictures go 16 to a launch.  Asynchronous on `stream`.
 *  FFHIP_EINVAL for another depth, chroma format, CTB or picture size, npics <= 0, NULL or misaligned planes, a stride below the
 *  width, nrefs outside 0..16, a NULL or misaligned plane among the first nrefs references, nslices < 0, or a reference plane that
 *  overlaps a destination plane of any picture of the call (the pictures of one launch must be independent); FFHIP_ENOSYS without a
 *  device. */
int ffhip_hevc_inter_pictures_dev(int bit_depth, int chroma_format_idc, int width, int height, int log2_ctb_size, int npics,
                                  const FFHipHevcInterPic *pics /* host array */, void *stream);
/** sizeof(FFHipHevcInterPU), sizeof(FFHipHevcInterTU), sizeof(FFHipHevcInterSlice), for bindings that mirror the records (no device
 *  needed). */
int ffhip_hevc_inter_pu_record_size(void);
int ffhip_hevc_inter_tu_record_size(void);
int ffhip_hevc_inter_slice_record_size(void);

/** In-loop filtering of whole pictures in one launch: deblocking (H.265 8.7.2) and SAO (8.7.3) of up to 16 pictures, from the
 *  reconstructed planes the intra and inter picture faces wrote (`src`, read only) into the DPB frames (`dst`, write only).  Out of
 *  place because intra prediction of the current picture reads unfiltered samples while the DPB holds filtered ones.
 *
 *  Semantics, byte for byte those of the reference's per-CTB filters over the whole picture (libavcodec/hevc/filter.c
 *  deblocking_filter_CTB, sao_filter_CTB, restore_tqb_pixels):
 *  - every vertical edge of the picture, then every horizontal edge on their output; edges on the picture border are skipped.  A
 *    luma segment with bS 1 or 2: qPL = (QpY(p) + QpY(q) + 1) >> 1, beta = betatable[Clip3(0, 51, qPL + beta_offset)], tC =
 *    tctable[Clip3(0, 53, qPL + 2 * (bS - 1) + (tc_offset & -2))], the offsets of the CTB that contains q0,0, the sample rules of
 *    hevc_{v,h}_loop_filter_luma (beta and tC scaled by << (bit_depth - 8) inside); no_p / no_q from `bypass` at p0 / q0;
 *  - chroma edges lie on the 8-sample chroma grid and are filtered where bS == 2; each 4-line chroma group takes the bS and QPs of
 *    the luma segment at its luma position, tC = tctable[Clip3(0, 53, QpC + 2 + tc_offset)] with QpC from qPi = Clip3(0, 57, qPL +
 *    cb/cr_qp_offset) (Table 8-10 for chroma format 1, Min(qPi, 51) otherwise);
 *  - a bS outside 0..2 leaves its segment unfiltered;
 *  - SAO per CTB and component from the fully deblocked picture (partial CTBs clipped to the picture): sao_band_filter /
 *    sao_edge_filter as the per-call faces, then for the edge type sao_edge_restore[restore] with the CTB's flags and the picture-
 *    border flags from geometry, then the samples of bypass CUs get their deblocked value back.  An out-of-range sao_type,
 *    sao_class or band position leaves that component of that CTB deblocked;
 *  - every sample of every dst plane inside the picture is written once; nothing outside the picture (the stride padding) is
 *    written, and src is never written.
 *  Trusted (the ABI carries no lengths to check them against): the maps cover the picture at their strides, `ctbs` holds ctb_w *
 *  ctb_h records.  Whatever their contents, no read or write leaves the planes and maps: bS, QP and SAO values only select
 *  table entries after clipping, or skip.
 *  Stays with the decoder: the SAO slice / tile flags below.  The boundary strengths (slice_deblocking_filter_disabled_flag, the
 *  slice and tile restrictions included) come from the decoder or from ffhip_hevc_boundary_strengths_pictures_dev() below.
 *  Out of scope: palette / SCC deblocking control, in-place filtering. */
typedef struct FFHipHevcLfCtb {     /* one CTB, 44 bytes */
    int8_t   beta_offset, tc_offset;  /* 2 * slice_beta_offset_div2, 2 * slice_tc_offset_div2 of the CTB's slice */
    uint8_t  sao_type[3];           /* per component: 0 not applied, 1 band, 2 edge (SAOParams.type_idx after the slice's flags) */
    uint8_t  sao_class[3];          /* band: band_position (0..31); edge: eo_class (0 horizontal, 1 vertical, 2 135 deg, 3 45 deg) */
    uint8_t  restore;               /* the `restore` of sao_filter_CTB: 0 sao_edge_restore[0], 1 [1] */
    uint8_t  vert_edge;             /* bits 0..1 = vert_edge[0..1] as sao_filter_CTB computes them */
    uint8_t  horiz_edge;            /* bits 0..1 = horiz_edge[0..1] */
    uint8_t  diag_edge;             /* bits 0..3 = diag_edge[0..3] */
    int16_t  sao_offset_val[3][5];  /* SaoOffsetVal per component, as the per-call SAO faces take them */
    uint8_t  pad[2];
} FFHipHevcLfCtb;
typedef struct FFHipHevcLfPlane {   /* device pointers */
    const uint8_t *src;             /* the reconstructed plane */
    ptrdiff_t src_stride;           /* bytes */
    uint8_t *dst;                   /* the filtered plane (the DPB frame's) */
    ptrdiff_t dst_stride;           /* bytes */
} FFHipHevcLfPlane;
typedef struct FFHipHevcLfPic {
    FFHipHevcLfPlane plane[3];      /* Y, Cb, Cr; chroma_format_idc 0: plane[0] only */
    const uint8_t *bs_ver, *bs_hor; /* device, [(y >> 2) * bs_stride + (x >> 2)]: the bS (0..2) of the 4-sample luma segment at
                                     * (x, y): vertical ones at x % 8 == 0 over rows y..y+3, horizontal ones at y % 8 == 0 over
                                     * columns x..x+3 (filter.c's vertical_bs / horizontal_bs with bs_stride = bs_width) */
    const int8_t *qp_y;             /* device, QpY on the min-CB grid: [(y >> log2_min_cb_size) * cb_stride + (x >> log2_min_cb_size)] */
    const uint8_t *bypass;          /* device, the same grid, != 0: pcm with pcm_loop_filter_disabled_flag or cu_transquant_bypass;
                                     * NULL: none */
    const FFHipHevcLfCtb *ctbs;     /* device, ctb_w * ctb_h records in raster order */
    int32_t bs_stride, cb_stride;   /* entries */
    int8_t cb_qp_offset, cr_qp_offset; /* pps_cb_qp_offset, pps_cr_qp_offset */
    uint8_t pad[6];
} FFHipHevcLfPic;
/** npics pictures of one geometry: width x height luma samples (multiples of 8, at most 65535), CTBs of 1 << log2_ctb_size (4..6),
 *  min CBs of 1 << log2_min_cb_size (3..log2_ctb_size), bit_depth 8, 10 or 12 (uint16_t samples above 8), chroma_format_idc 0..3.
 *  Planes: non-NULL, base and stride multiples of 4 samples, strides at least the plane's width; bs_stride at least width / 4,
 *  cb_stride at least the min-CB columns.  Pictures go 16 to a launch.  Asynchronous on `stream`.
 *  FFHIP_EINVAL for another depth, chroma format, CTB, min-CB or picture size, npics <= 0, NULL or misaligned planes, NULL bs_ver /
 *  bs_hor / qp_y / ctbs, a stride below its width, or any src plane that overlaps any dst plane of the call; FFHIP_ENOSYS without a
 *  device. */
int ffhip_hevc_loop_filter_pictures_dev(int bit_depth, int chroma_format_idc, int width, int height, int log2_ctb_size,
                                        int log2_min_cb_size, int npics, const FFHipHevcLfPic *pics /* host array */, void *stream);
/** sizeof(FFHipHevcLfCtb), for bindings that mirror the record (no device needed). */
int ffhip_hevc_lf_ctb_record_size(void);

/** Deblocking boundary strengths of whole pictures in one launch: the two maps the in-loop filter face reads (bs_ver / bs_hor of
 *  FFHipHevcLfPic), made on the device from what the decoder parsed: the motion field, the transform tree, the slice and tile maps.
 *  What libavcodec/hevc/filter.c's ff_hevc_deblocking_boundary_strengths() computes per transform unit (H.265 8.7.2.3 / 8.7.2.4), here
 *  per 4-sample segment.  The rule below is restated from the standard and from the reference's documented behaviour, not checked
 *  against the reference's source.
 *
 *  The grid is the 4 x 4 luma unit grid, w4 = width / 4 by h4 = height / 4.  The vertical segment of unit (ux, uy) has q = (ux, uy) and
 *  p = (ux - 1, uy); the horizontal one has p = (ux, uy - 1).  The first rule that applies gives its bS:
 *  1. ux (vertical) resp. uy (horizontal) odd, or 0 (the picture border): 0.
 *  2. the slice of q's CTB has flags bit 0 (slice_deblocking_filter_disabled_flag): 0.
 *  3. p and q lie in different slices and q's slice has flags bit 1 clear (slice_loop_filter_across_slices_enabled_flag == 0): 0;
 *     p and q lie in different tiles and loop_filter_across_tiles == 0: 0.
 *  4. q's tu marks that side as a transform-block edge and p or q is intra (pred_flag 0): 2.
 *  5. q's tu marks that side as a transform-block edge and p's or q's tu has cbf_luma: 1.
 *  6. otherwise motion decides, on every 8-sample line, marked or not (inside one prediction block both sides carry the same motion:
 *     0).  A reference picture is its DPB slot, slices[slice of the unit's CTB].ref[list][ref_idx], each side through the slice of its
 *     own CTB; two motion vectors differ when their x or their y components are at least 4 quarter samples apart.
 *     - one of p, q intra: 2 (possible only on a TU edge, which rule 4 has taken); both intra: 0 (inside one TU);
 *     - both bi-predicted, q from slots A0 / A1 and p from B0 / B1:
 *         A0 == B0, A0 == A1 and B0 == B1: 1 iff (mv0s differ or mv1s differ) and (p's mv1 and q's mv0 differ or p's mv0 and q's mv1 differ);
 *         else A0 == B0 and A1 == B1: 1 iff the mv0s differ or the mv1s differ;
 *         else A0 == B1 and A1 == B0: 1 iff p's mv1 and q's mv0 differ or p's mv0 and q's mv1 differ;
 *         else 1;
 *     - both uni-predicted, each from either list: 1 if the slots differ, else 1 iff the two used motion vectors differ;
 *     - one bi-predicted, one uni-predicted: 1.
 *  Malformed input has a defined result and never causes an access outside the maps: a ctb_slice entry >= nslices makes the
 *  segments of its units (as q) 0, and as p such a unit has no resolvable reference; a used ref_idx outside 0 .. num_ref - 1 (or
 *  beyond 15) or an unresolvable reference names a picture different from every other, another such one included; a pred_flag above 3
 *  counts as intra.
 *  Every entry of bs_ver and bs_hor inside w4 x h4 is written (0 off the 8-sample grid); nothing outside is, and no input is written.
 *  Stays with the decoder: the maps themselves (tab_mvf after merge / AMVP, the tu marks through ffhip_hevc_bs_mark_tu(), the slice
 *  and tile ids per CTB).  Out of scope: palette / SCC deblocking control, pps_deblocking_control beyond the per-slice disabled flag. */
typedef struct FFHipHevcMvField {   /* one 4 x 4 luma unit, 12 bytes: the decoder's tab_mvf entry */
    int16_t mv[2][2];               /* [list][x, y], quarter samples */
    int8_t  ref_idx[2];
    uint8_t pred_flag;              /* bit 0 L0, bit 1 L1; 0: intra / PCM */
    uint8_t pad;
} FFHipHevcMvField;
typedef struct FFHipHevcBsSlice {   /* 36 bytes */
    uint8_t ref[2][16];             /* [list][ref_idx] -> DPB slot: the same numbering as FFHipHevcInterSlice.ref */
    uint8_t num_ref[2];
    uint8_t flags;                  /* bit 0 slice_deblocking_filter_disabled_flag, bit 1 slice_loop_filter_across_slices_enabled_flag */
    uint8_t pad;
} FFHipHevcBsSlice;
typedef struct FFHipHevcBsPic {     /* _dev: device pointers; _host: host pointers */
    const FFHipHevcMvField *mvf;    /* [uy * mvf_stride + ux], 4-byte aligned */
    const uint8_t *tu;              /* [uy * tu_stride + ux]: bit 0 the unit's left side is a TU edge, bit 1 its top side, bit 2 cbf_luma of its TU */
    const uint16_t *ctb_slice;      /* ctb_w * ctb_h, raster: index into slices (the slice, not the slice segment) */
    const uint16_t *ctb_tile;       /* the same grid: tile id; NULL: one tile */
    const FFHipHevcBsSlice *slices; /* nslices records */
    uint8_t *bs_ver, *bs_hor;       /* out: FFHipHevcLfPic's layout, [uy * bs_stride + ux] */
    int32_t mvf_stride, tu_stride, bs_stride, nslices;   /* strides in entries */
    uint8_t loop_filter_across_tiles;  /* loop_filter_across_tiles_enabled_flag */
    uint8_t pad[7];
} FFHipHevcBsPic;
/** npics pictures of one geometry: width x height luma samples (multiples of 8, at most 65535), CTBs of 1 << log2_ctb_size (4..6).
 *  Pictures go 16 to a launch.  Asynchronous on `stream`; the maps are ready for ffhip_hevc_loop_filter_pictures_dev() on the same
 *  stream with no synchronisation in between.
 *  FFHIP_EINVAL for another CTB or picture size, npics <= 0, NULL mvf / tu / ctb_slice / slices / bs_ver / bs_hor, an mvf that is not
 *  4-byte aligned, a stride below width / 4, nslices < 1, or an output map whose span (first to last entry) overlaps the span of any
 *  input map or of any other output map of the call; FFHIP_ENOSYS without a device (after the argument checks). */
int ffhip_hevc_boundary_strengths_pictures_dev(int width, int height, int log2_ctb_size, int npics,
                                               const FFHipHevcBsPic *pics /* host array */, void *stream);
/** The same rules compiled for the CPU, on host arrays (device-free): the same arguments, refusals but FFHIP_ENOSYS, and bytes.
 *  For pictures a decoder does not send to the GPU; the _dev face never calls it. */
int ffhip_hevc_boundary_strengths_pictures_host(int width, int height, int log2_ctb_size, int npics, const FFHipHevcBsPic *pics);
/** What a decoder calls per luma transform unit of 1 << log2_size (2..5) samples at (x0, y0) (multiples of 4) on a host tu map:
 *  sets bit 0 on the units of the TU's left column, bit 1 on those of its top row, and bit 2 on all of them when cbf_luma.  The map
 *  starts zeroed.  Device-free. */
void ffhip_hevc_bs_mark_tu(uint8_t *tu, int tu_stride, int x0, int y0, int log2_size, int cbf_luma);
/** sizeof(FFHipHevcMvField), sizeof(FFHipHevcBsSlice), for bindings that mirror the records (no device needed). */
int ffhip_hevc_bs_mvf_record_size(void);
int ffhip_hevc_bs_slice_record_size(void);

/** Residuals of whole pictures in one launch: every transform unit of up to 16 pictures turned from its scaled coefficients into the
 *  final residual that the intra and inter picture faces take (their TU records' res_offset points at it).
 *
 *  Input: the scaled TransCoeffLevel values the reference's HEVCDSPContext members receive; the decoder has applied the scaling
 *  process and scaling lists while parsing (ff_hevc_hls_residual_coding).
 *  Semantics: each record runs, in this order, rotate -> its kind's operation -> RDPCM -> cross-component, with int16 storage between
 *  steps, byte for byte what the reference's per-call members produce in that order at bit_depth (libavcodec/hevc/dsp_template.c):
 *    DCT     idct[log2 - 2](c, col_limit)            DC      idct_dc[log2 - 2](c)
 *    DST     transform_4x4_luma(c), log2 2 only      SKIP    dequant(c, log2) (the tsShift scaling of transform skip)
 *    BYPASS  nothing: the coefficients are the residual (cu_transquant_bypass)
 *    ZERO    the residual is 0 and coeffs are not read (cbf 0; only useful as the luma of _CROSS or with _CROSS itself); its
 *            coeff_offset is still checked like any other, so point it at an in-range span (e.g. 0)
 *    _ROTATE     SKIP / BYPASS at log2 2: c[i] <-> c[15 - i] first (transform_skip_rotation_enabled_flag, cabac.c)
 *    _RDPCM_H/V  SKIP / BYPASS: transform_rdpcm(c, log2, 0 / 1) after the kind's operation
 *    _CROSS      planes 1 and 2 of chroma format 3 only: r[i] = (int16)(r[i] + ((res_scale_val * rY[i]) >> 3)) last, rY the FINAL
 *                residual of record `luma` of plane 0 of the same picture (0 for a luma ZERO record)
 *  The decoder decides, the face applies: it derives no implicit RDPCM, rotation or cross-component from SPS / PPS flags or intra
 *  modes.  The output depends neither on record order nor on the launch layout: a _CROSS record recomputes its luma residual itself
 *  and does not rely on the luma record having run.
 *  Malformed records write nothing and read nothing outside their planes: log2_size outside 2..5 or not that of its size_start
 *  group; an unknown kind or the reserved bit 0x80; DST or _ROTATE at log2 != 2; _ROTATE or an RDPCM flag on a kind other than
 *  SKIP / BYPASS, or both RDPCM flags set; _CROSS outside planes 1 / 2 of chroma format 3, res_scale_val not in {0, +-1, +-2, +-4, +-8}, `luma` out of plane 0's
 *  records, or a luma record that is of another size, carries _CROSS or is itself malformed; an offset not a multiple of 16, or
 *  offset + N*N beyond ncoeffs / nres.
 *  Written: the N*N residuals of each well-formed record and nothing else; coeffs is never written.  Trusted: the res ranges of one
 *  plane's records are disjoint (where two overlap the values in the overlap are undefined and nothing else is affected).
 *  Out of scope: extended_precision_processing_flag, scaling (the decoder's), boundary strengths. */
#define FFHIP_HEVC_RES_DCT      0
#define FFHIP_HEVC_RES_DC       1
#define FFHIP_HEVC_RES_DST      2
#define FFHIP_HEVC_RES_SKIP     3
#define FFHIP_HEVC_RES_BYPASS   4
#define FFHIP_HEVC_RES_ZERO     5
#define FFHIP_HEVC_RES_KIND     0x07 /* kind_flags & FFHIP_HEVC_RES_KIND: the kind */
#define FFHIP_HEVC_RES_ROTATE   0x08
#define FFHIP_HEVC_RES_RDPCM_H  0x10
#define FFHIP_HEVC_RES_RDPCM_V  0x20
#define FFHIP_HEVC_RES_CROSS    0x40
typedef struct FFHipHevcResTU {     /* one transform unit of one plane, 16 bytes */
    int32_t coeff_offset;           /* int16 units into the plane's coeffs: N*N scaled coefficients, row-major; a multiple of 16 */
    int32_t res_offset;             /* int16 units into the plane's res: the N*N residuals go here; a multiple of 16 */
    int32_t luma;                   /* _CROSS: index of the co-located luma record in plane 0's tus of the same picture */
    uint8_t log2_size;              /* 2..5 */
    uint8_t kind_flags;             /* bits 0-2 the kind, then the flags above */
    int8_t  res_scale_val;          /* _CROSS: ResScaleVal, one of 0, +-1, +-2, +-4, +-8 */
    uint8_t col_limit;              /* DCT: the col_limit cabac.c computes from the last significant position */
} FFHipHevcResTU;
typedef struct FFHipHevcResPlane {  /* device pointers, host lengths */
    const int16_t *coeffs;          /* read only */
    int32_t ncoeffs;                /* int16 elements of coeffs */
    int32_t nres;                   /* int16 elements of res */
    int16_t *res;
    const FFHipHevcResTU *tus;      /* grouped by log2_size, ascending */
    int32_t size_start[5];          /* size 2 + s is tus[size_start[s] .. size_start[s + 1]); size_start[0] == 0, non-decreasing */
    int32_t pad;
} FFHipHevcResPlane;
typedef struct FFHipHevcResPic {
    FFHipHevcResPlane plane[3];     /* Y, Cb, Cr; chroma_format_idc 0: plane[0] only */
} FFHipHevcResPic;
/** npics pictures, bit_depth 8, 10 or 12, chroma_format_idc 0..3.  Pictures go 16 to a launch; asynchronous on `stream`.
 *  A plane with records needs non-NULL, 16-byte aligned coeffs, res and tus (a plane without records is not looked at).
 *  FFHIP_EINVAL for another depth or chroma format, npics <= 0, a NULL picture array, NULL or misaligned pointers of a used plane, a
 *  size_start that does not start at 0 or decreases, negative lengths, or any res range of the call ([res, res + nres)) that
 *  overlaps any coeffs range of the call or the res range of another plane or picture; FFHIP_ENOSYS without a device. */
int ffhip_hevc_residual_pictures_dev(int bit_depth, int chroma_format_idc, int npics, const FFHipHevcResPic *pics /* host array */,
                                     void *stream);
/** sizeof(FFHipHevcResTU), for bindings that mirror the record (no device needed). */
int ffhip_hevc_res_tu_record_size(void);

/* ------------------------------------------------------------------------------------------ */
/* libavcodec: vp9dsp inverse transforms                                    */
/* ------------------------------------------------------------------------------------------ */
/** VP9DSPContext.itxfm_add (libavcodec/vp9dsp.h:71-75): [tx][txtp](dst, stride, block, eob); tx 0..3 = TX_4X4..TX_32X32,
 *  4 = the lossless 4x4 Walsh-Hadamard transform; txtp = enum TxfmType (DCT_DCT 0, DCT_ADST 1, ADST_DCT 2, ADST_ADST 3,
 *  libavcodec/vp9.h).  The transform adds to dst and consumes the block (zeroed; eob == 1 on DCT_DCT: block[0] only).
 *  8 bits; host pointers. */
typedef void (*ffhip_vp9_itxfm_add_func)(uint8_t *dst, ptrdiff_t stride, int16_t *block, int eob);
typedef struct FFHipVP9ItxfmContext {
    ffhip_vp9_itxfm_add_func itxfm_add[5][4];
} FFHipVP9ItxfmContext;
/** ff_vp9dsp_init_<arch> shape for the itxfm_add table (libavcodec/vp9dsp.c:88-112).  bpp 8, 10 or 12 (baked into the installed functions; above 8 bits samples are uint16_t and blocks hold int32 coefficients). */
int ff_vp9dsp_itxfm_init_hip(FFHipVP9ItxfmContext *c, int bpp);

/** One transform block of the batch face. */
typedef struct FFHipVp9TU {
    int32_t coeff_offset; /* int16 elements into coeffs: size * size coefficients, the decoder's layout.  coeffs + coeff_offset
                           * must be 4-byte aligned (coeff_offset even on an aligned int16 array; any value on the int32 array of the
                           * _hbd face): a block moves in 16-byte pieces where it is 16-byte aligned and as dwords otherwise, unit by
                           * unit; an odd address is undefined */
    int32_t dst_offset;   /* bytes into dst                                                           */
    uint8_t txtp;         /* enum TxfmType; ignored for 32x32 and the WHT                              */
    uint8_t dc_only;      /* eob == 1: DCT_DCT takes its dc-only shortcut                              */
    uint8_t pad[2];       /* sizeof == 12                                                              */
} FFHipVp9TU;
/** n blocks of one size (tx as above), pairwise disjoint in coeffs and dst: itxfm_add[tx][txtp] each. */
int ffhip_vp9_itxfm_add_batch_dev(int tx, int16_t *coeffs, uint8_t *dst, ptrdiff_t stride, const FFHipVp9TU *tus, int n,
                                  void *stream);

/** vp9_mc_func and VP9DSPContext.mc[size 64/32/16/8/4][filter][put/avg][!!mx][!!my] (libavcodec/vp9dsp.h:33-35,115;
 *  enum FilterMode, libavcodec/vp9.h:64-70: 0 smooth, 1 regular, 2 sharp, 3 bilinear); mx, my in sixteenths. */
typedef void (*ffhip_vp9_mc_func)(uint8_t *dst, ptrdiff_t dst_stride, const uint8_t *src, ptrdiff_t src_stride, int h, int mx, int my);
typedef struct FFHipVP9McContext {
    ffhip_vp9_mc_func mc[5][4][2][2][2];
} FFHipVP9McContext;
int ff_vp9dsp_mc_init_hip(FFHipVP9McContext *c, int bpp);
/** One prediction block of the batch face (what inter_pred / mc_luma_unscaled pass, libavcodec/vp9recon.c). */
typedef struct FFHipVp9McBlock {
    int32_t dst_offset, src_offset; /* bytes into dst / src: the block's integer-sample origin */
    uint8_t width;                  /* 4, 8, 16, 32 or 64 */
    uint8_t height;                 /* 1..64 */
    uint8_t filter;                 /* enum FilterMode 0..3 */
    uint8_t mx, my;                 /* 0..15 */
    uint8_t avg;                    /* 0 put, 1 avg (compound prediction's second reference) */
    uint8_t pad[2];                 /* sizeof == 16 */
} FFHipVp9McBlock;
/** n blocks, pairwise disjoint in dst; src must be readable 3 samples left/up and 4 right/down of each block (rows are read in
 *  whole dwords: 1 byte more on the right). */
int ffhip_vp9_mc_batch_dev(uint8_t *dst, ptrdiff_t dststride, const uint8_t *src, ptrdiff_t srcstride, const FFHipVp9McBlock *blocks,
                           int n, void *stream);

/** vp9_scaled_mc_func and VP9DSPContext.smc[size][filter][put/avg] (libavcodec/vp9dsp.h:36-38,121): prediction from a reference
 *  picture of another size; dx, dy = the step in sixteenths of a reference sample per output sample (1..32: 16x up to 2x down). */
typedef void (*ffhip_vp9_scaled_mc_func)(uint8_t *dst, ptrdiff_t dst_stride, const uint8_t *src, ptrdiff_t src_stride, int h, int mx, int my,
                                         int dx, int dy);
typedef struct FFHipVP9ScaledMcContext {
    ffhip_vp9_scaled_mc_func smc[5][4][2];
} FFHipVP9ScaledMcContext;
int ff_vp9dsp_scaled_mc_init_hip(FFHipVP9ScaledMcContext *c, int bpp);
typedef struct FFHipVp9ScaledBlock {
    int32_t dst_offset, src_offset;
    uint8_t width, height;          /* 4..64 (a power of two), 1..64 */
    uint8_t filter, mx, my, avg;    /* as FFHipVp9McBlock */
    uint8_t dx, dy;                 /* 1..32 */
} FFHipVp9ScaledBlock;
/** n blocks, pairwise disjoint in dst; src must be readable 3 samples left/up of the block origin and through column
 *  ((mx + (w - 1) dx) >> 4) + 4, row ((my + (h - 1) dy) >> 4) + 4. */
int ffhip_vp9_scaled_mc_batch_dev(uint8_t *dst, ptrdiff_t dststride, const uint8_t *src, ptrdiff_t srcstride,
                                  const FFHipVp9ScaledBlock *blocks, int n, void *stream);

/** The loop-filter tables of VP9DSPContext (libavcodec/vp9dsp.h:76-105): loop_filter_8[width 4/8/16][h col-edge / v row-edge],
 *  loop_filter_16[dir], loop_filter_mix2[wd1][wd2][dir] (two 8-sample halves, limits packed in the two low bytes). */
typedef void (*ffhip_vp9_lf_func)(uint8_t *dst, ptrdiff_t stride, int mb_lim, int lim, int hev_thr);
typedef struct FFHipVP9LoopFilterContext {
    ffhip_vp9_lf_func loop_filter_8[3][2];
    ffhip_vp9_lf_func loop_filter_16[2];
    ffhip_vp9_lf_func loop_filter_mix2[2][2][2];
} FFHipVP9LoopFilterContext;
int ff_vp9dsp_loopfilter_init_hip(FFHipVP9LoopFilterContext *c, int bpp);
/** One 8-sample segment of an edge: what one loop_filter() call of the reference covers (vp9dsp_template.c:1780-1889). */
typedef struct FFHipVp9Edge {
    int32_t offset;      /* bytes into the plane: the first q0 sample of the segment; base + offset even above 8 bits (a uint16_t
                          * sample), an odd address is undefined.  Any other alignment is allowed: a column edge's line is moved as
                          * dwords where its address is 4-byte aligned and sample by sample otherwise, line by line */
    uint8_t wd_idx;      /* 0: 4, 1: 8, 2: 16 */
    uint8_t dir;         /* 0: column edge (loop_filter_h_*), 1: row edge (loop_filter_v_*) */
    uint8_t E, I, H;     /* mb_lim, lim, hev_thr */
    uint8_t pad[3];      /* sizeof == 12 */
} FFHipVp9Edge;
/** n segments that share no sample (VP9 orders the overlapping edges of a superblock: column edges left to right, then row
 *  edges; a caller batches what is disjoint, e.g. every other 8-sample column of wd <= 8 edges). */
int ffhip_vp9_loop_filter_batch_dev(uint8_t *base, ptrdiff_t stride, const FFHipVp9Edge *edges, int n, void *stream);

/** VP9DSPContext.intra_pred[tx 4x4..32x32][enum IntraPredMode] (libavcodec/vp9dsp.h:52-55, libavcodec/vp9.h:45-62): left[] runs
 *  bottom to top, top[-1] is the corner; the 4x4 down-left / vert-left modes read top[0..7]. */
typedef void (*ffhip_vp9_intra_func)(uint8_t *dst, ptrdiff_t stride, const uint8_t *left, const uint8_t *top);
typedef struct FFHipVP9IntraContext {
    ffhip_vp9_intra_func intra_pred[4][15];
} FFHipVP9IntraContext;
int ff_vp9dsp_intrapred_init_hip(FFHipVP9IntraContext *c, int bpp);
/** One block of the batch face.  Its neighbours live in `edges` as the edge line: left[0..N-1], the corner, top[0..max(N,8)-1]
 *  (N + 1 + max(N, 8) bytes at edge_offset) — what the decoder's edge preparation (libavcodec/vp9recon.c, check_intra_mode)
 *  produces, concatenated. */
typedef struct FFHipVp9Intra {
    int32_t dst_offset;   /* bytes into dst */
    int32_t edge_offset;  /* bytes into edges */
    uint8_t mode;         /* enum IntraPredMode 0..14 */
    uint8_t pad[3];       /* sizeof == 12 */
} FFHipVp9Intra;
int ffhip_vp9_intra_pred_batch_dev(int tx, uint8_t *dst, ptrdiff_t stride, const uint8_t *edges, const FFHipVp9Intra *blocks, int n,
                                   void *stream);
/**
 * The VP9 loop filter in SUPERBLOCK (decoder) order: ff_vp9_loopfilter_sb() (libavcodec/vp9lpf.c:180-203) for a whole picture.
 * The function-level batch above takes segments that share no sample; a decoder's edges overlap (a 16-wide filter reaches 8
 * samples either way, and a superblock's left / top edges rewrite its neighbours' samples), so the picture is a dependency graph:
 * per plane all column edges of a superblock, then all its row edges, superblocks in raster order.  Here a superblock's VP9Filter
 * becomes a table of 8-line segments per edge position on the host (ffhip_vp9_lf_sb_tables, device-free) and one launch walks the
 * picture as a wavefront (one wave per superblock row; superblock (x, y) starts when row y - 1 has finished x + 1), all three
 * planes in the same step.  4:2:0; bit_depth 8, 10 or 12.
 */
typedef struct FFHipVp9Filter {          /* == VP9Filter (libavcodec/vp9dec.h:79-83) */
    uint8_t level[8 * 8];
    uint8_t mask[2 /* 0 = y, 1 = uv */][2 /* 0 = col, 1 = row */][8 /* rows */][4 /* 0 = 16, 1 = 8, 2 = 4, 3 = inner 4 */];
} FFHipVp9Filter;
typedef struct FFHipVp9LfSb {            /* entry: bit 31 valid, 24..25 width (0: 4, 1: 8, 2: 16), 16..23 H, 8..15 I (lim), 0..7 E (mblim) */
    uint32_t y[2][16][8];                /* [0 column edges / 1 row edges][position: 4 p samples along the filter axis][segment of 8 lines] */
    uint32_t uv[2][8][4];                /* the same for both chroma planes (32 x 32 samples) */
} FFHipVp9LfSb;
/** The chroma planes' table of one superblock where the two sub-sampling shifts differ — 4:2:2 (ss_h 1, ss_v 0: 32 x 64 chroma samples) and
 *  4:4:0 (ss_h 0, ss_v 1: 64 x 32): entries as in FFHipVp9LfSb; first the column edges [position][segment of 8 lines] (4:2:2: 8 x 8, 4:4:0:
 *  16 x 4), then the row edges [position][segment of 8 columns] (4:2:2: 16 x 4, 4:4:0: 8 x 8) — 128 words either way.  Both chroma planes
 *  share it (filter_plane_cols / _rows with uv_masks = lflvl->mask[1], libavcodec/vp9lpf.c:185-201). */
typedef struct FFHipVp9LfSbC {
    uint32_t t[128];
} FFHipVp9LfSbC;
int ffhip_vp9_lf_sb_ctables(FFHipVp9LfSbC *out, const FFHipVp9Filter *lflvl, int row, int col, int ss_h, int ss_v, const uint8_t *lim_lut,
                            const uint8_t *mblim_lut);
/** Host side: the tables of the superblock at (row, col) — in 8-sample units, as the reference passes them (superblock (r, c): row =
 *  8 r, col = 8 c; only "is it the first" matters) — from its VP9Filter and the frame's filter_lut (vp9.c:683-697).  ss_h = ss_v = 1
 *  (4:2:0) or 0 (4:4:4: y only, the chroma planes are filtered by the luma tables); 1, 0 / 0, 1 (4:2:2 / 4:4:0): y only as well, the chroma
 *  planes take ffhip_vp9_lf_sb_ctables(). */
int ffhip_vp9_lf_sb_tables(FFHipVp9LfSb *out, const FFHipVp9Filter *lflvl, int row, int col, int ss_h, int ss_v, const uint8_t *lim_lut,
                           const uint8_t *mblim_lut);
/** One picture of cols x rows 8x8 blocks (VP9Context.cols / .rows: (width + 7) >> 3, (height + 7) >> 3), i.e. (cols + 7) >> 3 by
 *  (rows + 7) >> 3 superblocks; tables[sb_rows * sb_cols] in device memory in raster order.  Nothing outside the picture's
 *  8 cols x 8 rows luma samples (half of that per chroma plane) is read or written — the reference touches no more, and the
 *  decoder's frame buffers are not padded to whole superblocks.  Planes and strides 4-byte aligned.  Asynchronous on `stream`; a
 *  lost hand-off is reported by ffhip_stream_synchronize. */
int ffhip_vp9_loopfilter_frame_dev(int bit_depth, uint8_t *y, uint8_t *u, uint8_t *v, ptrdiff_t stride_y, ptrdiff_t stride_uv, int cols,
                                   int rows, const FFHipVp9LfSb *tables, void *stream);
/** The same with the picture's chroma sub-sampling (VP9Context.ss_h / .ss_v).  1, 1: the call above.  0, 0 (4:4:4, profiles 1 / 3): the
 *  chroma planes are filtered exactly as luma — ff_vp9_loopfilter_sb passes luma's masks (uv_masks = lflvl->mask[ss_h | ss_v]) and
 *  levels with ss 0 (vp9lpf.c:185-201) — so all three planes use tables[].y and three luma chains run side by side; tables[].uv is not
 *  read.  4:4:0 / 4:2:2: FFHIP_EINVAL here (they need the chroma tables: ffhip_vp9_loopfilter_frame_ssc_dev). */
int ffhip_vp9_loopfilter_frame_ss_dev(int bit_depth, int ss_h, int ss_v, uint8_t *y, uint8_t *u, uint8_t *v, ptrdiff_t stride_y,
                                      ptrdiff_t stride_uv, int cols, int rows, const FFHipVp9LfSb *tables, void *stream);
/** 4:2:2 (ss_h 1, ss_v 0) and 4:4:0 (0, 1) — VP9 profiles 1 / 3 with rectangular chroma superblocks (round 4): luma by tables[].y, both
 *  chroma planes by ctables[] (one per superblock, raster order, device memory).  A plain kernel (one wave per superblock row and plane);
 *  one picture per launch. */
int ffhip_vp9_loopfilter_frame_ssc_dev(int bit_depth, int ss_h, int ss_v, uint8_t *y, uint8_t *u, uint8_t *v, ptrdiff_t stride_y,
                                       ptrdiff_t stride_uv, int cols, int rows, const FFHipVp9LfSb *tables, const FFHipVp9LfSbC *ctables,
                                       void *stream);
/** N pictures of one geometry in ONE launch (round 4; what a decoder's frame threads hold at once): each picture its own planes and
 *  tables (device pointers), strides shared.  A picture's filter is a dependency chain through it (0.9 ms for a 4K picture on a chip it
 *  cannot fill); the pictures of a batch are filtered side by side.  ss_h == ss_v (4:2:0 / 4:4:4).  `pics` is a host array. */
typedef struct FFHipVp9LfPic {
    uint8_t *y, *u, *v;
    const FFHipVp9LfSb *tables;
} FFHipVp9LfPic;
int ffhip_vp9_loopfilter_frames_dev(int bit_depth, int ss_h, int ss_v, int npics, const FFHipVp9LfPic *pics, ptrdiff_t stride_y,
                                    ptrdiff_t stride_uv, int cols, int rows, void *stream);
/** The same for the formats with rectangular chroma superblocks — 4:2:2 (ss_h 1, ss_v 0) and 4:4:0 (0, 1) (round 5): every picture brings
 *  its chroma tables as well (ffhip_vp9_lf_sb_ctables()); ffhip_vp9_loopfilter_frame_ssc_dev()'s plain kernel with the pictures of the batch
 *  side by side (libavcodec/vp9lpf.c:27-203).  ffhip_vp9_loopfilter_frames_dev() answers FFHIP_EINVAL for these formats. */
typedef struct FFHipVp9LfPicC {
    uint8_t *y, *u, *v;
    const FFHipVp9LfSb *tables;
    const FFHipVp9LfSbC *ctables;
} FFHipVp9LfPicC;
int ffhip_vp9_loopfilter_frames_ssc_dev(int bit_depth, int ss_h, int ss_v, int npics, const FFHipVp9LfPicC *pics, ptrdiff_t stride_y,
                                        ptrdiff_t stride_uv, int cols, int rows, void *stream);

/**
 * The VP9 loop-filter tables of whole frames on the device: what the tail of ff_vp9_decode_block and mask_edges
 * (libavcodec/vp9block.c:1141-1262, 1433-1447) and then ffhip_vp9_lf_sb_tables() / ffhip_vp9_lf_sb_ctables() do on the host per
 * superblock, for every superblock of up to 16 pictures in one launch, from one 4-byte record per decoded block.  The tables never
 * exist on the host: ffhip_vp9_loopfilter_frames_dev() / _ssc_dev() read them on the same stream.  Restated from the behaviour of
 * the reference, not checked against its source.
 *
 *  Per superblock (sb_row, sb_col), from its records blocks[sb_first[i] .. sb_first[i + 1]) in order:
 *  1. an all-zero VP9Filter.  (The reference clears only `mask` between superblock rows and leaves stale levels, which it reads only
 *     where a block has just written them; here every cell that no record with a level above 0 covers is 0.)
 *  2. lvl = level[lvl_idx]; a record whose lvl is 0 does nothing.  Otherwise, with row7 / col7 = pos >> 3 / pos & 7, row / col = 8 sb_row +
 *     row7 / 8 sb_col + col7, w8 x h8 the block's size in 8x8 cells (sub-8x8 sizes count as 1):
 *  3. lvl goes to the block's w8 x h8 cells of level[], clipped by the 8x8 table only;
 *  4. mask_edges(mask[0], 0, 0, row7, col7, x_end, y_end, 0, 0, tx, skip_inter), x_end = min(cols - col, w8), y_end = min(rows - row, h8);
 *  5. if ss_h | ss_v: mask_edges(mask[1], ss_h, ss_v, row7, col7, x_end, y_end, col_end, row_end, uvtx, skip_inter) with
 *     uvtx = tx - ((ss_h && w8 * 2 == 1 << tx) || (ss_v && h8 * 2 == 1 << tx)), col_end = (cols & 1 && col + w8 >= cols) ? cols & 7 : 0,
 *     row_end = (rows & 1 && row + h8 >= rows) ? rows & 7 : 0;
 *  6. tables[i] is what ffhip_vp9_lf_sb_tables(out, &filter, 8 sb_row, 8 sb_col, ss_h, ss_v, lim_lut, mblim_lut) writes (the zero `uv`
 *     part outside 4:2:0 included), ctables[i] what ffhip_vp9_lf_sb_ctables() writes, filters[i] the VP9Filter itself.
 *  Every word of every output is written, zeros included: a superblock without records gets all-zero tables.
 *
 *  Malformed records cannot be refused (they are in device memory): a record is skipped as if its level were 0 when bs > 12, a bit above
 *  bit 2 of tx_skip is set, tx is larger than the largest transform that fits the block (tx > 0 below 8x8), pos is not aligned to the
 *  block's own size (or has a bit above bit 5), the first cell lies outside the picture, or lvl_idx > 63.  sb_first entries are clamped to
 *  nblocks, a decreasing pair is an empty superblock, a superblock may have any number of records.  Where records of one superblock
 *  overlap (no stream does that) the masks are the union and a cell's level is that of any one of the records that cover it (the host
 *  face: of the last one).  Nothing outside the arrays of the call is read or written, whatever the records hold.  A 16-wide chroma entry
 *  on a tile's last 4-sample position, which the frame kernels cannot take and no record set produces (docs/KERNELS.md), is cleared.
 *
 *  FFHIP_EINVAL: cols or rows outside 1..10912 (8 x 1364 superblock rows, the filter faces' limit), ss_h / ss_v outside 0 / 1, npics
 *  outside 1..16, a NULL sb_first or tables, NULL blocks with nblocks > 0, blocks / sb_first / an output that is not 4-byte aligned, a
 *  level[] above 63, ctables present when ss_h == ss_v or absent when they differ, an output that overlaps another output or an input
 *  of the call.
 */
typedef struct FFHipVp9LfBlock {   /* one ff_vp9_decode_block call, 4 bytes */
    uint8_t pos;      /* (row & 7) << 3 | (col & 7): the block's first 8x8 cell inside its superblock */
    uint8_t bs;       /* enum BlockSize, 0 = 64x64 ... 12 = 4x4, as ffhip_vp9_inter_block_preds takes it */
    uint8_t tx_skip;  /* bits 0..1 b->tx, bit 2 skip_inter = !b->intra && b->skip */
    uint8_t lvl_idx;  /* seg_id << 3 | (b->intra ? 0 : b->ref[0] + 1) << 1 | (b->mode[3] != ZEROMV) */
} FFHipVp9LfBlock;

typedef struct FFHipVp9LfTabPic {
    const FFHipVp9LfBlock *blocks;   /* device; a superblock's records are contiguous */
    const uint32_t *sb_first;        /* device; sb_rows * sb_cols + 1 entries, raster order: records [sb_first[i], sb_first[i+1]) */
    uint32_t nblocks;
    uint8_t level[64];               /* segmentation.feat[seg].lflvl[ref][mode], indexed by lvl_idx; all 0 when filter.level is 0 */
    uint8_t lim_lut[64], mblim_lut[64];
    FFHipVp9LfSb *tables;            /* device out, sb_rows * sb_cols */
    FFHipVp9LfSbC *ctables;          /* device out; required when ss_h != ss_v, NULL otherwise */
    FFHipVp9Filter *filters;         /* device out, optional (NULL: not written) */
} FFHipVp9LfTabPic;

/** cols x rows in 8x8 blocks, as for ffhip_vp9_loopfilter_frames_dev(); `pics` is a host array.  Asynchronous on `stream`.
 *  FFHIP_ENOSYS without a device, after the checks. */
int ffhip_vp9_lf_tables_pictures_dev(int ss_h, int ss_v, int cols, int rows, int npics, const FFHipVp9LfTabPic *pics, void *stream);
/** The same rules on host arrays (device-free): every pointer of `pics` is a host pointer. */
int ffhip_vp9_lf_tables_pictures_host(int ss_h, int ss_v, int cols, int rows, int npics, const FFHipVp9LfTabPic *pics);
/** sizeof(FFHipVp9LfBlock), for bindings that mirror the record (no device needed). */
int ffhip_vp9_lf_block_record_size(void);

/**
 * VP9 inter reconstruction of whole frames in one launch: inter_pred() and the residual half of inter_recon() (libavcodec/vp9recon.c,
 * vp9_mc_template.h) for every inter block of up to 16 frames, from references resident in device memory.  A decoder records a
 * frame's prediction calls and transform blocks instead of running them; one launch then writes the frame, and
 * ffhip_vp9_loopfilter_frames_dev() filters it.
 *
 *  Semantics, byte for byte those of the reference at bit_depth (vp9dsp_template.c, the oracle's ffo_vp9_mc_bd / ffo_vp9_itxfm_add_bd):
 *  - prediction: each FFHipVp9InterPred record is one mc_luma_dir / mc_chroma_dir call: put from ref[0]; when compound, then avg from
 *    ref[1] (the rounding average (a + b + 1) >> 1 of the two clipped predictions).  Each filter pass is clip((sum + 64) >> 7) into
 *    pixel-type temporaries (the 2-D form filters rows -3 .. h + 3 horizontally first); bilinear is a + ((m (b - a) + 8) >> 4).
 *    Luma: x' = x + (mv.x >> 3), phase (mv.x & 7) << 1 in sixteenths.  Chroma: m = mv.x * (1 << !ss_h), x' = x + (m >> 4), phase
 *    m & 15; rows the same with mv.y and ss_v.  A chroma record drives Cb and Cr;
 *  - reference edge: every reference sample is read with its coordinates clamped to the reference frame's real size, [0, width) x
 *    [0, height) for luma and [0, (width + ss_h) >> ss_h) x [0, (height + ss_v) >> ss_v) for chroma: what emulated_edge_mc gives
 *    mc_luma_unscaled / mc_chroma_unscaled (vp9recon.c).  MVs may point anywhere;
 *  - residuals: when every prediction of a superblock is done, its TUs add itxfm_add[tx][txtp] (the dc-only shortcut of DCT_DCT when
 *    dc_only, as the batch face).  Coefficients are read, never zeroed.  A TU changes only samples a prediction of its superblock covers;
 *  - what is written: the covered samples inside the decoded area, cols * 8 x rows * 8 luma samples (cols = (width + 7) >> 3, rows =
 *    (height + 7) >> 3), shifted by ss_h / ss_v for chroma: what ff_vp9_decode_block copies back from its overhang buffer.  Samples no
 *    prediction covers (intra blocks, the stride padding, anything outside the decoded area) are never written;
 *  - a malformed record writes nothing and reads nothing outside its planes and references: a prediction with w or h outside
 *    {4, 8, 16, 32, 64}, filter > 3, a reference it uses at or above nrefs, flags bits other than 0 and 1, or lying outside the
 *    superblock it is listed under (in its plane); a TU with tx > 4, not aligned to its size, or outside its superblock.
 *  Trusted (the ABI carries no lengths to check them against): the superblock start tables and the records they index, each TU's
 *  coeff_offset range, and disjointness: the predictions of one plane of a superblock must be disjoint, as must its TUs; overlapping
 *  ones leave undefined values inside that superblock and nothing outside it.
 *  Every reference must have the frame's size here; references of another size take ffhip_vp9_inter_frames_scaled_dev() below.
 *  Out of scope (they stay on the C path): MV parsing and clamping.  Intra blocks of inter frames are left untouched here: ffhip_vp9_intra_frames_dev() reconstructs them afterwards.
 */
typedef struct FFHipVp9InterPred {  /* one mc_luma_dir / mc_chroma_dir call (with its compound second half), 20 bytes */
    uint16_t x, y;                  /* its top-left sample in its plane */
    uint8_t  w, h;                  /* 4, 8, 16, 32 or 64 */
    uint8_t  filter;                /* enum FilterMode 0..3 */
    uint8_t  flags;                 /* bit 0 compound, bit 1 chroma (the record drives Cb and Cr), bit 2 FFHIP_VP9_PRED_SCALED */
    uint8_t  ref[2];                /* 0..2: indices into the frame's references (b->ref[]) */
    uint8_t  box[2];                /* FFHIP_VP9_PRED_SCALED records: the call's clip box, [0] = px | py << 4, [1] = log2 pw | log2 ph << 4;
                                       0 otherwise */
    int16_t  mv[2][2];              /* [ref][x, y]: the VP9mv passed to mc_*_dir, eighths of a luma sample */
} FFHipVp9InterPred;
#define FFHIP_VP9_PRED_SCALED 4     /* flags bit 2: a call of the SCALED template (ffhip_vp9_inter_frames_scaled_dev only) */
typedef struct FFHipVp9InterTU {    /* one itxfm_add call of inter_recon, 12 bytes */
    uint16_t x, y;                  /* its top-left sample in its plane */
    int32_t  coeff_offset;          /* coefficients (int16 at 8 bits, int32 above) into the plane's coeffs: N * N, the decoder's layout */
    uint8_t  tx;                    /* 0..3: 4x4 .. 32x32, 4: the lossless WHT */
    uint8_t  txtp;                  /* enum TxfmType (DCT_DCT for inter blocks); ignored for 32x32 and the WHT */
    uint8_t  dc_only;               /* eob == 1 */
    uint8_t  pad;
} FFHipVp9InterTU;
typedef struct FFHipVp9InterPlane { /* device pointers */
    uint8_t *base;                  /* the plane's top-left sample */
    ptrdiff_t stride;               /* bytes, >= the decoded width in bytes */
    const FFHipVp9InterTU *tus;     /* sorted by raster superblock address */
    const int32_t *tu_sb_start;     /* sb_w * sb_h + 1 entries: the TUs of raster superblock a are tus[tu_sb_start[a] .. [a + 1]) */
    const void *coeffs;             /* int16 (8 bits) or int32 (10 / 12 bits) coefficients */
} FFHipVp9InterPlane;
typedef struct FFHipVp9InterRef {   /* one reference frame (device pointers) of the call's size, depth and subsampling */
    const uint8_t *base[3];         /* Y, Cb, Cr */
    ptrdiff_t stride[3];            /* bytes */
} FFHipVp9InterRef;
typedef struct FFHipVp9InterPic {
    FFHipVp9InterPlane plane[3];    /* Y, Cb, Cr */
    const FFHipVp9InterPred *preds; /* device, sorted by raster superblock (64 x 64 luma) address */
    const int32_t *pred_sb_start;   /* device, sb_w * sb_h + 1 entries, as tu_sb_start */
    int32_t nrefs;                  /* 1..3 */
    int32_t pad;
    FFHipVp9InterRef ref[3];        /* in this host array: the face stages it to the device */
} FFHipVp9InterPic;
/** npics frames of one geometry: width x height luma samples (1..65535), bit_depth 8, 10 or 12 (uint16_t samples above 8), chroma
 *  subsampling (ss_h, ss_v) in {0, 1}^2.  sb_w = (cols + 7) >> 3, sb_h = (rows + 7) >> 3.  Every plane needs non-NULL pointers, base
 *  and stride multiples of 4 samples and a stride of at least the decoded width; references are sample-aligned with a stride of at
 *  least the plane's real width.  Frames go 16 to a launch.  Asynchronous on `stream`.
 *  FFHIP_EINVAL (before any device check) for another depth or subsampling, a size outside 1..65535, npics <= 0, NULL or misaligned
 *  planes, a stride below the decoded width, nrefs outside 1..3, a NULL or misaligned plane among the first nrefs references, or a
 *  reference plane that overlaps a destination plane of any frame of the call; FFHIP_ENOSYS without a device. */
int ffhip_vp9_inter_frames_dev(int bit_depth, int ss_h, int ss_v, int width, int height, int npics,
                               const FFHipVp9InterPic *pics /* host array */, void *stream);
/** sizeof(FFHipVp9InterPred), sizeof(FFHipVp9InterTU), for bindings that mirror the records (no device needed). */
int ffhip_vp9_inter_pred_record_size(void);
int ffhip_vp9_inter_tu_record_size(void);
/** The prediction records of one decoded block, in vp9_mc_template.h's call order (device-free, like ffhip_vp9_lf_sb_tables): bs =
 *  enum BlockSize 0..12 (BS_64x64 .. BS_4x4), row / col in 8-sample units (0..8191), mv = b->mv as [sub-block][ref][x, y], comp =
 *  b->comp, ref = b->ref, filter = b->filter (0..3).  At least 8x8: one luma and one chroma call with mv[0].  8x4, 4x8 and 4x4: the
 *  template's sub-block calls, chroma MVs from ROUNDED_DIV_MVx2 / x4 (rounding half away from zero) with the libvpx 4:2:2 quirks it
 *  emulates.  Writes up to 8 records to out; returns their count, FFHIP_EINVAL for bad arguments. */
int ffhip_vp9_inter_block_preds(FFHipVp9InterPred *out, int bs, int row, int col, const int16_t mv[4][2][2], int comp, const uint8_t ref[2],
                                int filter, int ss_h, int ss_v);

/**
 * VP9 inter reconstruction of whole frames from references of another size (reference scaling: libvpx resize_mode, WebRTC / SVC
 * resolution changes, spatial layers): ffhip_vp9_inter_frames_dev() with the SCALED instantiation of vp9_mc_template.h and
 * mc_luma_scaled / mc_chroma_scaled (libavcodec/vp9recon.c), the per-reference scale and step of the frame header (vp9.c).  Stated
 * in plane coordinates; W x H is the frame's luma size, cols = (W + 7) >> 3, rows = (H + 7) >> 3, rw x rh a reference's luma size.
 *  - per reference: of the frame's size when rw == W and rh == H (unscaled); otherwise scaled, valid when 2 W >= rw, 2 H >= rh,
 *    W <= 16 rw and H <= 16 rh, with scale[0] = (rw << 14) / W, scale[1] = (rh << 14) / H, step[d] = (16 scale[d]) >> 14 (1..32)
 *    and scale_mv(n, d) = ((int64) n * scale[d]) >> 14 (an arithmetic shift: it floors);
 *  - a record without FFHIP_VP9_PRED_SCALED is a call of the unscaled template, exactly as in ffhip_vp9_inter_frames_dev().  A
 *    record with it is a call of the SCALED template (inter_recon picks it when b->ref[0]'s reference is scaled, or b->comp and
 *    b->ref[1]'s is): per reference it uses, a reference of the frame's size is read by the unscaled rule (mc_*_unscaled), a scaled
 *    one as follows.  (x, y) is the record's origin in its plane, (px, py, pw, ph) its clip box from box[]: the call's offset inside
 *    its enclosing block, and that block's size, in the record's plane;
 *  - luma, scaled reference: mv.x = clip(mv.x, -(x + pw - px + 4) * 8, (cols * 8 - x + px + 3) * 8), mx = scale_mv(mv.x * 2, 0) +
 *    scale_mv(x * 16, 0); the same with y, ph, py, rows and index 1 for my.  Output sample (i, j) of the w x h call is
 *    VP9DSPContext.smc[..][filter][put / avg](..., h, mx & 15, my & 15, step[0], step[1]) from the origin (mx >> 4, my >> 4): the
 *    oracle's ffo_vp9_smc_bd, horizontal pass first into pixel-type temporaries, phase 0 a copy;
 *  - chroma, scaled reference, with ss_h set: mv.x = clip(mv.x, -(x + pw - px + 4) * 16, (cols * 4 - x + px + 3) * 16), mx =
 *    scale_mv(mv.x, 0) + (scale_mv(x * 16, 0) & ~15) + (scale_mv(x * 32, 0) & 15) (libvpx's rounding, webm issue 820, which the
 *    reference reproduces); with ss_h clear, the luma formulas.  The same for y with ss_v, rows and index 1;
 *  - reference edge: every sample of a reference is read with its coordinates clamped to that reference's real size, [0, rw) x
 *    [0, rh) for luma, [0, (rw + ss_h) >> ss_h) x [0, (rh + ss_v) >> ss_v) for chroma.  mc_luma_scaled / mc_chroma_scaled read
 *    directly only when the whole window, rows y - 3 .. y + refbh_m1 + 4 and columns x - 3 .. x + refbw_m1 + 4, lies inside the
 *    reference, and through emulated_edge_mc of that window otherwise, which replicates the edge samples: both give this clamp;
 *  - compound averaging, the TUs, what is written and what is never written: as ffhip_vp9_inter_frames_dev().
 *  A record with FFHIP_VP9_PRED_SCALED is malformed (writes nothing) when log2 pw or log2 ph lies outside 2..6, px + w > pw or
 *  py + h > ph; the other malformed classes are ffhip_vp9_inter_frames_dev()'s.  A launch (16 frames) none of whose references is
 *  scaled runs ffhip_vp9_inter_frames_dev()'s kernel, which treats FFHIP_VP9_PRED_SCALED as malformed: rule 2 of inter_recon never
 *  gives such a record there.
 */
typedef struct FFHipVp9InterPicScaled {
    FFHipVp9InterPic pic;           /* as for ffhip_vp9_inter_frames_dev(); references of their own size */
    int32_t ref_w[3], ref_h[3];     /* the luma size of each of pic.ref[0 .. nrefs - 1] (1..65535) */
} FFHipVp9InterPicScaled;
/** ffhip_vp9_inter_frames_dev() with references of any valid size.  FFHIP_EINVAL (before any device check) for what
 *  ffhip_vp9_inter_frames_dev() refuses, with each reference plane's stride and overlap checked over that reference's own plane size,
 *  and for a reference size outside 1..65535 or outside the 2x / 16x limits above; FFHIP_ENOSYS without a device.  Frames whose
 *  references all have the frame's size give the bytes ffhip_vp9_inter_frames_dev() gives. */
int ffhip_vp9_inter_frames_scaled_dev(int bit_depth, int ss_h, int ss_v, int width, int height, int npics,
                                      const FFHipVp9InterPicScaled *pics /* host array */, void *stream);
/** The records of one decoded block for the SCALED template (arguments as ffhip_vp9_inter_block_preds()), every one with
 *  FFHIP_VP9_PRED_SCALED and its clip box, in its call order.  At least 8x8: one luma call with box (0, 0, bw, bh) and one chroma
 *  call with (0, 0, bw >> ss_h, bh >> ss_v), mv[0].  8x4, 4x8 and 4x4 take the template's 4x4 branch (8x4 and 4x8 have their own
 *  branches only under SCALED == 0): four 4x4 luma calls with mv[0..3] and boxes (0 | 4, 0 | 4, 8, 8); chroma as that branch, the
 *  boxes in the chroma plane (offset in the 8 x 8 luma area's chroma, (8 >> ss_h) x (8 >> ss_v)).  A decoder calls this when inter_recon
 *  picks the SCALED template, ffhip_vp9_inter_block_preds() otherwise.  Writes up to 8 records; returns their count, FFHIP_EINVAL
 *  for bad arguments. */
int ffhip_vp9_inter_block_preds_scaled(FFHipVp9InterPred *out, int bs, int row, int col, const int16_t mv[4][2][2], int comp,
                                       const uint8_t ref[2], int filter, int ss_h, int ss_v);

/**
 * VP9 intra reconstruction of whole frames in one launch: intra_recon() with check_intra_mode() (libavcodec/vp9recon.c) for every
 * intra block of up to 16 frames.  An intra block's edges are the reconstructed samples of earlier blocks, so a decoder records each
 * intra_pred / itxfm_add pair instead of running it; one launch then reconstructs the frames' intra blocks in decoding order, after
 * ffhip_vp9_inter_frames_dev() and before ffhip_vp9_loopfilter_frames_dev() on the same stream.
 *
 *  Semantics, byte for byte those of the reference at bit_depth (vp9dsp_template.c; the oracle's ffo_vp9_intra_pred_bd /
 *  ffo_vp9_itxfm_add_bd), stated in plane coordinates.  The decoded area of a plane is dw x dh = (cols * 8) >> hs by (rows * 8) >> vs
 *  (cols = (width + 7) >> 3, rows = (height + 7) >> 3); N = 4 << tx (4 for tx 4); base = 128 << (bit_depth - 8); P(u, v) is the plane
 *  as reconstructed so far (earlier records final, inter samples as they stand at launch, nothing loop-filtered):
 *  - availability: have_top = y > 0; have_left = x > the start of the tile column holding x, (min((i * sb_w) >> log2_tile_cols, sb_w)
 *    * 64) >> hs for tile column i (set_tile_offset, vp9.c); have_right from the record;
 *  - the coded mode becomes mode_conv[mode][have_left][have_top] (check_intra_mode), which selects the predictor; the coded mode
 *    selects txtp (the caller's ff_vp9_intra_txfm_type[mode]);
 *  - top[j], j < N: P(min(x + j, dw - 1), y - 1), or base - 1 without top.  4x4 DIAG_DOWN_LEFT / VERT_LEFT also read top[4..7]:
 *    P(x + j, y - 1) when have_top, have_right and x + 8 <= dw, else all four are top[3] (the reference's rule, kept);
 *  - the corner: P(x - 1, y - 1) with top and left, base + 1 with top but no left, base - 1 without top;
 *  - left[i], i < N rows down: P(x - 1, min(y + i, dh - 1)), or base + 1 without left;
 *  - the residual: itxfm_add[tx][txtp] when the residual flag is set (the dc-only shortcut of DCT_DCT when dc_only); coefficients are
 *    read, never zeroed;
 *  - what is written: the record's samples inside the decoded area.  Inter samples, the stride padding and anything past dw / dh keep
 *    their bytes (no read above leaves the decoded area);
 *  - a malformed record writes nothing and reads nothing outside its planes; later records run as if it were absent: tx > 4, mode >
 *    9, txtp > 3, an unknown flag bit, dc_only without residual, (x, y) not a multiple of N, the N x N square outside the superblock
 *    it is listed under, its origin outside the decoded area, or a 4x4 record with have_right whose top-right samples (x + 4 .. x + 7)
 *    leave that superblock (intra_recon never sets it there).
 *  Trusted (the ABI carries no lengths to check them against): the superblock start tables, each record's coeff_offset range, the
 *  decoding order of the records within a superblock, and that the records of one plane of a superblock are disjoint.
 */
typedef struct FFHipVp9IntraRec {    /* one iteration of intra_recon's loops: intra_pred[tx][mode], then itxfm_add; 12 bytes */
    uint16_t x, y;                   /* top-left sample in its plane */
    int32_t  coeff_offset;           /* coefficients (int16 at 8 bits, int32 above) into the plane's coeffs; read only with the residual flag */
    uint8_t  tx;                     /* 0..3: 4x4 .. 32x32; 4: 4x4 prediction and the lossless WHT (as FFHipVp9InterTU) */
    uint8_t  mode;                   /* the CODED enum IntraPredMode 0..9 (b->mode[..] / b->uvmode), before check_intra_mode converts it */
    uint8_t  txtp;                   /* ff_vp9_intra_txfm_type[mode] for luma, DCT_DCT for chroma; ignored for 32x32 and the WHT */
    uint8_t  flags;                  /* FFHIP_VP9_INTRA_* */
} FFHipVp9IntraRec;
#define FFHIP_VP9_INTRA_RESIDUAL   1 /* !skip && eob != 0: itxfm_add follows the prediction */
#define FFHIP_VP9_INTRA_DC_ONLY    2 /* eob == 1 (with the residual flag only) */
#define FFHIP_VP9_INTRA_HAVE_RIGHT 4 /* x < w4 - 1 in intra_recon's loop (read by 4x4 records only) */
typedef struct FFHipVp9IntraPlane {  /* device pointers */
    uint8_t *base;                   /* the plane's top-left sample */
    ptrdiff_t stride;                /* bytes, >= the decoded width in bytes */
    const FFHipVp9IntraRec *recs;    /* sorted by raster superblock (64 x 64 luma) address; within a superblock in decoding order */
    const int32_t *rec_sb_start;     /* sb_w * sb_h + 1 entries: the records of raster superblock a are recs[rec_sb_start[a] .. [a + 1]) */
    const void *coeffs;              /* int16 (8 bits) or int32 (10 / 12 bits) coefficients */
} FFHipVp9IntraPlane;
typedef struct FFHipVp9IntraPic {
    FFHipVp9IntraPlane plane[3];     /* Y, Cb, Cr */
    int32_t log2_tile_cols;          /* 0..6: the frame header's tile columns (they decide have_left) */
    int32_t pad;
} FFHipVp9IntraPic;
/** npics frames of one geometry: width x height luma samples (1..65535), bit_depth 8, 10 or 12 (uint16_t samples above 8), chroma
 *  subsampling (ss_h, ss_v) in {0, 1}^2.  sb_w = (cols + 7) >> 3, sb_h = (rows + 7) >> 3.  Every plane needs non-NULL pointers, base
 *  and stride multiples of 4 samples and a stride of at least the decoded width.  Asynchronous on `stream`; a lost hand-off is
 *  reported by ffhip_stream_synchronize.
 *  FFHIP_EINVAL (before any device check) for another depth or subsampling, a size outside 1..65535, npics <= 0 or a NULL array, NULL
 *  or misaligned planes, a stride below the decoded width, log2_tile_cols outside 0..6, or two planes of the call that overlap;
 *  FFHIP_ENOSYS without a device. */
int ffhip_vp9_intra_frames_dev(int bit_depth, int ss_h, int ss_v, int width, int height, int npics,
                               const FFHipVp9IntraPic *pics /* host array */, void *stream);
/** sizeof(FFHipVp9IntraRec), for bindings that mirror the record (no device needed). */
int ffhip_vp9_intra_record_size(void);
/** The records of one decoded block in one plane, in intra_recon's order (device-free, like ffhip_vp9_inter_block_preds): plane 0 takes
 *  tx = b->tx and mode = b->mode; planes 1 and 2 take tx = b->uvtx and mode[0] = b->uvmode.  bs = enum BlockSize 0..12, row / col in
 *  8-sample units, skip = b->skip, eob[n] the value intra_recon reads for transform n (td->eob / td->uveob[p]), lossless = the frame
 *  header's; cols / rows as above.  coeff_offset = 16 * n (the caller adds the block's base offset).  Writes up to 256 records to out;
 *  returns their count, FFHIP_EINVAL for bad arguments. */
int ffhip_vp9_intra_block_records(FFHipVp9IntraRec *out /* up to 256 */, int plane, int bs, int tx, int row, int col, const uint8_t mode[4],
                                  int skip, const uint16_t *eob, int lossless, int cols, int rows, int ss_h, int ss_v);

/* ------------------------------------------------------------------------------------------ */
/* libavcodec: vp8dsp (VP8DSPContext, libavcodec/vp8dsp.h) — 8 bits, the only depth VP8 has    */
/* ------------------------------------------------------------------------------------------ */
/** VP8DSPContext member for member, with the reference's signatures.  put_vp8_*_pixels_tab[w][v][h]: w = 0, 1, 2 for blocks 16, 8 and
 *  4 wide; v / h = 0 no filter along that axis, 1 the 4-tap form, 2 the 6-tap form (bilinear: 1 and 2 are the same function); mx, my
 *  in eighths (1..7 along a filtered axis).  The semantics are vp8dsp.c's C, byte for byte, side effects included:
 *  - vp8_luma_dc_wht writes the 16 second-stage DCs to block[i][j][0] and zeroes dc[0..15]; vp8_luma_dc_wht_dc writes (dc[0] + 3) >> 3
 *    to all 16 and zeroes dc[0];
 *  - vp8_idct_add adds the 4x4 inverse transform and zeroes all 16 coefficients; vp8_idct_dc_add adds (block[0] + 4) >> 3 and zeroes
 *    block[0]; dc_add4y runs it on the blocks at +0, +4, +8, +12 samples, dc_add4uv at +0, +4, +4 * stride, +4 * stride + 4, each
 *    zeroing its own block[i][0];
 *  - the loop filters take (E, I, hev_thresh) as filter_mb() passes them (the simple ones take E only) and filter 16 lines (8 per
 *    chroma plane) across the edge at dst: v_ members the row edge above dst, h_ members the column edge left of dst;
 *  - h rows of width w for 1 <= h <= 2w (the reference's temporary); a filtered axis reads 2 samples before and 3 after (6-tap), 1 and
 *    2 (4-tap), 0 and 1 (bilinear).
 *  VP7's own members (ff_vp7dsp_init: its WHT, IDCT and loop filters) are not here. */
typedef void (*ffhip_vp8_mc_func)(uint8_t *dst, ptrdiff_t dst_stride, const uint8_t *src, ptrdiff_t src_stride, int h, int mx, int my);
typedef void (*ffhip_vp8_lf_func)(uint8_t *dst, ptrdiff_t stride, int flim_E, int flim_I, int hev_thresh);
typedef void (*ffhip_vp8_lf_uv_func)(uint8_t *dst_u, uint8_t *dst_v, ptrdiff_t stride, int flim_E, int flim_I, int hev_thresh);
typedef void (*ffhip_vp8_lf_simple_func)(uint8_t *dst, ptrdiff_t stride, int flim);
typedef struct FFHipVP8DSPContext {
    void (*vp8_luma_dc_wht)(int16_t block[4][4][16], int16_t dc[16]);
    void (*vp8_luma_dc_wht_dc)(int16_t block[4][4][16], int16_t dc[16]);
    void (*vp8_idct_add)(uint8_t *dst, int16_t block[16], ptrdiff_t stride);
    void (*vp8_idct_dc_add)(uint8_t *dst, int16_t block[16], ptrdiff_t stride);
    void (*vp8_idct_dc_add4y)(uint8_t *dst, int16_t block[4][16], ptrdiff_t stride);
    void (*vp8_idct_dc_add4uv)(uint8_t *dst, int16_t block[4][16], ptrdiff_t stride);
    ffhip_vp8_lf_func vp8_v_loop_filter16y;
    ffhip_vp8_lf_func vp8_h_loop_filter16y;
    ffhip_vp8_lf_uv_func vp8_v_loop_filter8uv;
    ffhip_vp8_lf_uv_func vp8_h_loop_filter8uv;
    ffhip_vp8_lf_func vp8_v_loop_filter16y_inner;
    ffhip_vp8_lf_func vp8_h_loop_filter16y_inner;
    ffhip_vp8_lf_uv_func vp8_v_loop_filter8uv_inner;
    ffhip_vp8_lf_uv_func vp8_h_loop_filter8uv_inner;
    ffhip_vp8_lf_simple_func vp8_v_loop_filter_simple;
    ffhip_vp8_lf_simple_func vp8_h_loop_filter_simple;
    ffhip_vp8_mc_func put_vp8_epel_pixels_tab[3][3][3];
    ffhip_vp8_mc_func put_vp8_bilinear_pixels_tab[3][3][3];
} FFHipVP8DSPContext;
/** ff_vp78dsp_init shape: fills the two MC tables (shared by VP7 and VP8), nothing else.  ff_vp8dsp_init shape: fills the transforms
 *  and the loop filters, nothing else.  Each remembers the C functions it displaces and answers a call that cannot run on the device
 *  (or an argument outside the reference's range, such as mx = 0 in a filtered slot) through them.  0, FFHIP_EINVAL (NULL) or
 *  FFHIP_ENOSYS (no device; the table is left as it was). */
int ff_vp78dsp_init_hip(FFHipVP8DSPContext *c);
int ff_vp8dsp_init_hip(FFHipVP8DSPContext *c);

/** One macroblock of the WHT batch: vp8_luma_dc_wht (or _dc) from the 16 DCs at dc_offset into the block[4][4][16] array at
 *  block_offset.  Offsets in bytes into coeffs, even. */
typedef struct FFHipVp8WhtRec {
    int32_t dc_offset;
    int32_t block_offset;
    uint8_t dc_only;                /* 1: vp8_luma_dc_wht_dc (only dc[0] is read and zeroed) */
    uint8_t pad[3];                 /* sizeof == 12 */
} FFHipVp8WhtRec;
/** n macroblocks whose dc and block arrays are pairwise disjoint.  A record with an odd offset or dc_only > 1 is skipped.
 *  FFHIP_EINVAL (before any device check) for a NULL or misaligned (odd) pointer or n < 0; FFHIP_ENOSYS without a device. */
int ffhip_vp8_luma_dc_wht_batch_dev(int16_t *coeffs, const FFHipVp8WhtRec *recs, int n, void *stream);
/** One 4x4 block of the IDCT batch: vp8_idct_add, or vp8_idct_dc_add when dc_only. */
typedef struct FFHipVp8IdctRec {
    int32_t dst_offset;             /* bytes into dst: the block's top-left sample */
    int32_t coeff_offset;           /* bytes into coeffs (even): 16 int16 coefficients, consumed */
    uint8_t dc_only;                /* 0 vp8_idct_add, 1 vp8_idct_dc_add */
    uint8_t pad[3];                 /* sizeof == 12 */
} FFHipVp8IdctRec;
/** n blocks, pairwise disjoint in dst and in coeffs.  A decoder runs ffhip_vp8_luma_dc_wht_batch_dev() first on the same stream.  A
 *  record with an odd coeff_offset or dc_only > 1 is skipped.  FFHIP_EINVAL (before any device check) for NULL pointers, an odd coeffs,
 *  a stride of 0 or above 2^24 in magnitude, or n < 0; FFHIP_ENOSYS without a device. */
int ffhip_vp8_idct_add_batch_dev(uint8_t *dst, ptrdiff_t stride, int16_t *coeffs, const FFHipVp8IdctRec *recs, int n, void *stream);
/** One put_vp8_* call of the MC batch. */
typedef struct FFHipVp8McRec {
    int32_t dst_offset, src_offset; /* bytes into dst / src: the block's integer-sample origin */
    uint8_t width;                  /* 16, 8 or 4 */
    uint8_t h;                      /* 1 .. 2 * width */
    uint8_t mx, my;                 /* eighths, 1..7 along a filtered axis (ignored along the others) */
    uint8_t htaps, vtaps;           /* the table's [v][h] slot: 0 none, 1 the 4-tap form, 2 the 6-tap form */
    uint8_t bilinear;               /* 1: put_vp8_bilinear_pixels_tab (slots 1 and 2 alike), 0: put_vp8_epel_pixels_tab */
    uint8_t pad;                    /* sizeof == 16 */
} FFHipVp8McRec;
/** n calls, pairwise disjoint in dst.  src must be readable 2 samples left / up and 3 right / down of each block (only what the
 *  record's slot reads is read).  A record with another width, h outside 1..2w, a slot above 2, bilinear above 1, or mx / my outside
 *  1..7 along a filtered axis (0..7 bilinear) writes nothing.  FFHIP_EINVAL (before any device check) for NULL pointers, strides of 0 or
 *  above 2^24 in magnitude, or n < 0; FFHIP_ENOSYS without a device. */
int ffhip_vp8_mc_batch_dev(uint8_t *dst, ptrdiff_t dststride, const uint8_t *src, ptrdiff_t srcstride, const FFHipVp8McRec *recs, int n,
                           void *stream);
/** sizeof(FFHipVp8WhtRec), sizeof(FFHipVp8IdctRec), sizeof(FFHipVp8McRec), for bindings that mirror the records (no device needed). */
int ffhip_vp8_wht_record_size(void);
int ffhip_vp8_idct_record_size(void);
int ffhip_vp8_mc_record_size(void);

/**
 * The VP8 loop filter of whole frames in one launch: what filter_mb_row() (libavcodec/vp8.c) does to a reconstructed frame, every
 * macroblock in raster order, for up to 16 frames per launch (a larger npics is split into launches of 16).  A decoder stores
 * td->filter_strength of every row into the frame's record array instead of filtering, and launches this after reconstruction.
 *
 *  Semantics, byte for byte: the frame as left by running, for mb_y = 0 .. mb_h - 1 and mb_x = 0 .. mb_w - 1, filter_mb() (filter_type
 *  0, normal: Y, U and V) or filter_mb_simple() (filter_type 1: Y only, U and V untouched) of vp8.c with the record of that macroblock:
 *  - level = filter_level, nothing at all when it is 0; a record with filter_level > 63, inner_limit > 63 or inner_filter > 1 counts as
 *    level 0;
 *  - mbedge_lim = 2 * level + inner_limit + 4, bedge_lim = 2 * level + inner_limit, hev_thresh = hev_thresh_lut[keyframe][level]
 *    (0 below 15, then 1; from 20 2 for inter frames; from 40 2 for key frames and 3 for inter frames);
 *  - normal: the left MB edge (mb_x > 0: h_loop_filter16y / 8uv), the inner column edges at 4, 8, 12 (luma) and 4 (chroma) when
 *    inner_filter, the top MB edge (mb_y > 0: v_loop_filter16y / 8uv), then the inner row edges likewise; simple: the same order
 *    with h_ / v_loop_filter_simple, mbedge_lim on the MB edges and bedge_lim inside.
 *  Nothing outside mb_w * 16 x mb_h * 16 luma and mb_w * 8 x mb_h * 8 chroma samples is read or written.
 */
typedef struct FFHipVp8FilterStrength { /* == VP8FilterStrength (libavcodec/vp8.h): what filter_level_for_mb() leaves, 3 bytes */
    uint8_t filter_level;
    uint8_t inner_limit;
    uint8_t inner_filter;
} FFHipVp8FilterStrength;
typedef struct FFHipVp8LfPic {         /* device pointers */
    uint8_t *y, *u, *v;                /* the planes' top-left samples (u, v unused by the simple filter and may be NULL there) */
    const FFHipVp8FilterStrength *strength; /* mb_w * mb_h records in raster order */
} FFHipVp8LfPic;
/** filter_type 0 normal, 1 simple; keyframe 0 or 1; mb_w, mb_h 1..1024.  Planes and strides must be multiples of 4 bytes, stride_y at
 *  least 16 * mb_w and (normal) stride_uv at least 8 * mb_w.  Asynchronous on `stream`; a lost hand-off (never in a correct run) is
 *  reported by ffhip_stream_synchronize.  FFHIP_EINVAL (before any device check) for other values, npics <= 0 or a NULL array, NULL or
 *  misaligned planes, or two planes of the call that overlap; FFHIP_ENOSYS without a device. */
int ffhip_vp8_loopfilter_frames_dev(int filter_type, int keyframe, int mb_w, int mb_h, int npics, const FFHipVp8LfPic *pics /* host array */,
                                    ptrdiff_t stride_y, ptrdiff_t stride_uv, void *stream);

/**
 * VP8 reconstruction of whole frames: what decode_mb_row_no_filter() (libavcodec/vp8.c) does per macroblock between parsing and the
 * loop filter — intra_predict() or inter_predict(), then idct_mb() — for every macroblock of up to 16 frames per call (a larger npics
 * is split into launches of 16).  A decoder fills one FFHipVp8Mb per macroblock instead of calling those three, and launches this,
 * then ffhip_vp8_loopfilter_frames_dev() on the same stream: the filtered frame is the next frame's reference and never leaves the
 * device.  VP8 only (not VP7); the frame and its references have the same size.  The rules below restate vp8.c from memory of its
 * structure; treat a difference from vp8.c as a defect of this face.
 *
 *  The record holds what VP8Macroblock and the row's non_zero_count_cache hold at that point:
 *  - ref_frame 0: intra; 1, 2, 3: VP8_FRAME_PREVIOUS, _GOLDEN, _ALTREF, planes ref[ref_frame - 1][0..2] of the frame's struct.
 *  - intra: mode = FFHIP_VP8_PRED_DC / _HOR / _VERT / _TM (mb->mode's values) or FFHIP_VP8_MODE_I4x4 with the sixteen sub_mode[] =
 *    FFHIP_VP8_B_VERT .. _TM (intra4x4_pred_mode_mb, raster order); chroma_mode = FFHIP_VP8_PRED_DC .. _TM.
 *  - inter: partitioning = FFHIP_VP8_PART_NONE (mv[0] = mb->mv), _16x8 (mv[0..1] = bmv[0..1]: top, bottom), _8x16 (left, right), _8x8
 *    (mv[0..3]), _4x4 (mv[0..15] = bmv[], raster order); luma MVs in quarter-pel, { x, y }.
 *  - y2: 0 nothing (the luma DCs are already in the blocks), 1 vp8_luma_dc_wht_dc, 2 vp8_luma_dc_wht, from block_dc into the
 *    sixteen luma blocks' [0].
 *  - block_code: 2 bits per 4x4 block, block b (0..15 Y in raster order, 16..19 U, 20..23 V) in bits 2 (b & 3) of byte b >> 2:
 *    0 nothing, 1 vp8_idct_dc_add, 2 vp8_idct_add (idct_mb's dc_add4y / dc_add4uv shortcuts leave the same bytes as the per-block
 *    members).  mb->skip is "all codes 0 and y2 0".
 *  - coeff_offset: index of the macroblock's 400 coefficients in the frame's `coeffs`, a multiple of 16: td->block[6][4][16] (384)
 *    followed by td->block_dc[16]; ignored when nothing is coded.  The coefficients are READ ONLY here: unlike the VP8DSPContext
 *    members and the batch faces above (which keep their clearing side effect), this face does not clear them.
 *
 *  Inter (inter_predict, vp8_mc_part, vp8_mc_luma, vp8_mc_chroma): ffhip_vp8_mb_preds() lists the calls.
 *  - luma: mx = (mv.x * 2) & 7, my = (mv.y * 2) & 7, the source is the block's position + (mv.x >> 2, mv.y >> 2); the [v][h] table
 *    slot of a fraction is subpel_idx[0][]: 0 for 0, 1 (4 taps) for odd eighths, 2 (6 taps) for even ones; `bilinear` (s->profile != 0)
 *    takes put_vp8_bilinear_pixels_tab, whose slots 1 and 2 are one function.  A zero fraction pair is a copy.
 *  - chroma: the luma MV read as eighths of the half-size plane: mx = mv.x & 7, the source + (mv.x >> 3); with fullpel_chroma
 *    (s->profile == 3) both components & ~7 first.  4x4 partitioning: each 4x4 chroma block takes the sum s of its 2x2 group's four
 *    luma MVs, (s + 2 + (s >> 31)) >> 2 per component, then the full-pel mask; the others: each part's MV on the half-size block.
 *  - reference samples are read as emulated_edge_mc gives them against a 16 mb_w x 16 mb_h (chroma 8 mb_w x 8 mb_h) plane:
 *    coordinates clamped to the plane.  An MV may point anywhere; no padded border is read.
 *  - then the residual: the WHT per y2, then each block per its code.
 *
 *  Intra (intra_predict and its check_*_mode helpers, the VP8 branch): prediction reads the unfiltered samples of the frame being
 *  reconstructed, inter macroblocks included.  Outside the frame the border is virtual: the row above is 127, (-1, -1) included;
 *  the column to the left is 129.  ffhip_vp8_intra_modes() gives the slots taken.
 *  - 4x4 modes see that border (intra_predict's copy_dst, or the substitutes DC_127 / DC_129 / plain VERT / plain HOR, which equal
 *    it).  Top-right of a sub-block: columns 0..2 read the row above the sub-block (rows 1..3: the reconstructed sub-block above
 *    right, inside the macroblock); column 3 of EVERY row reads the four samples above-right of the macroblock (row 16 mb_y - 1,
 *    columns 16 mb_x + 16..19), which in the last macroblock column are the sample at column 16 mb_x + 15 of that row, repeated.
 *  - 16x16 and chroma modes: VERT -> DC_127 in the top row, HOR -> DC_129 in the left column, TM -> VERT / HOR / DC_129; DC uses only
 *    the sides that exist (TOP_DC / LEFT_DC at an edge, 128 in the corner macroblock).
 *  - an I4x4 macroblock: sub-blocks in raster order, each predicted, then its residual added, the next one predicts from the
 *    result; other macroblocks and chroma: the whole block is predicted, then the residuals are added.
 *
 *  A malformed record makes its macroblock write nothing; the rest of the frame is unaffected (a neighbour predicts from the bytes
 *  that were there): ref_frame > 3 or naming a reference with a NULL plane, mode > 4, chroma_mode > 3, sub_mode > 9 (I4x4),
 *  partitioning > 4, y2 > 2, a block code of 3, or (something coded) a coeff_offset that is negative, not a multiple of 16 or with
 *  coeff_offset + 400 > coeff_count.
 */
#define FFHIP_VP8_PRED_DC       0   /* 16x16 / chroma modes and the slots they take: h264pred.h's DC_PRED8x8 .. DC_129_PRED8x8 */
#define FFHIP_VP8_PRED_HOR      1
#define FFHIP_VP8_PRED_VERT     2
#define FFHIP_VP8_PRED_TM       3   /* PLANE_PRED8x8's slot */
#define FFHIP_VP8_MODE_I4x4     4   /* FFHipVp8Mb.mode only */
#define FFHIP_VP8_PRED_LEFT_DC  4   /* slots only, from here on */
#define FFHIP_VP8_PRED_TOP_DC   5
#define FFHIP_VP8_PRED_DC_128   6
#define FFHIP_VP8_PRED_DC_127   7
#define FFHIP_VP8_PRED_DC_129   8
#define FFHIP_VP8_PRED_NONE     255 /* FFHipVp8IntraModes.mode16 of an I4x4 macroblock: no pred16x16[] slot is taken */
#define FFHIP_VP8_B_VERT        0   /* 4x4 modes: h264pred.h's VERT_PRED .. HOR_UP_PRED, TM_VP8_PRED */
#define FFHIP_VP8_B_HOR         1
#define FFHIP_VP8_B_DC          2
#define FFHIP_VP8_B_DDL         3
#define FFHIP_VP8_B_DDR         4
#define FFHIP_VP8_B_VR          5
#define FFHIP_VP8_B_HD          6
#define FFHIP_VP8_B_VL          7
#define FFHIP_VP8_B_HU          8
#define FFHIP_VP8_B_TM          9
#define FFHIP_VP8_B_VERT_PLAIN  10  /* slots only: VERT_VP8_PRED, DC_127_PRED, DC_129_PRED, HOR_VP8_PRED */
#define FFHIP_VP8_B_DC_127      12
#define FFHIP_VP8_B_DC_129      13
#define FFHIP_VP8_B_HOR_PLAIN   14
#define FFHIP_VP8_PART_NONE     0
#define FFHIP_VP8_PART_16x8     1
#define FFHIP_VP8_PART_8x16     2
#define FFHIP_VP8_PART_8x8      3
#define FFHIP_VP8_PART_4x4      4
typedef struct FFHipVp8Mb {            /* 96 bytes */
    int32_t coeff_offset;
    int16_t mv[16][2];
    uint8_t sub_mode[16];
    uint8_t block_code[6];
    uint8_t ref_frame, mode, chroma_mode, partitioning, y2, reserved;
} FFHipVp8Mb;
typedef struct FFHipVp8ReconPic {      /* device pointers */
    uint8_t *y, *u, *v;                /* the frame being reconstructed */
    const uint8_t *ref[3][3];          /* [VP8_FRAME_PREVIOUS, _GOLDEN, _ALTREF - 1][Y, U, V]: same strides and geometry; NULL where no record names it */
    const FFHipVp8Mb *mbs;             /* mb_w * mb_h records in raster order */
    const int16_t *coeffs;             /* never written */
    int64_t coeff_count;
} FFHipVp8ReconPic;
/** mb_w, mb_h 1..1024; bilinear, fullpel_chroma 0 or 1.  Two launches per 16 frames on `stream`: the inter macroblocks (a wave each;
 *  intra records return at once — no keyframe hint is taken and nothing is scanned on the host), then the intra macroblocks, a
 *  wave per macroblock row that starts macroblock x once the row above has finished min(x + 2, mb_w).  Asynchronous; a lost hand-off
 *  (never in a correct run) is reported by ffhip_stream_synchronize.  FFHIP_EINVAL (before any device check) for values outside
 *  those, npics <= 0, a NULL array, a NULL y / u / v / mbs, a NULL coeffs with coeff_count > 0, planes (references too) or strides
 *  that are not multiples of 4, stride_y < 16 * mb_w, stride_uv < 8 * mb_w, a reference plane that overlaps a destination plane of
 *  the call, or two destination planes that overlap; FFHIP_ENOSYS without a device. */
int ffhip_vp8_recon_frames_dev(int mb_w, int mb_h, int bilinear, int fullpel_chroma, int npics, const FFHipVp8ReconPic *pics /* host array */,
                               ptrdiff_t stride_y, ptrdiff_t stride_uv, void *stream);
int ffhip_vp8_mb_record_size(void);
/** One put_vp8_{epel,bilinear}_pixels_tab[.][vslot][hslot] call of inter_predict(): a w x h block at (x, y) of the macroblock in
 *  `plane` (0 Y, 1 U, 2 V; chroma in chroma samples), whose source block starts at (sx, sy) of the reference plane (before clamping;
 *  the taps reach around it), with mx, my in eighths. */
typedef struct FFHipVp8Pred {
    uint8_t plane, x, y, w, h, mx, my, vslot, hslot, pad[3];
    int32_t sx, sy;
} FFHipVp8Pred;
/** Device-free.  The calls inter_predict() makes for `mb` at (mb_x, mb_y), in its order (per part luma, U, V; 4x4: the sixteen luma
 *  blocks, then U, V of each chroma block): returns their number (3, 6, 12 or 24), FFHIP_EINVAL for NULL, an intra record, ref_frame > 3, a
 *  partitioning > 4 or a negative mb_x / mb_y. */
int ffhip_vp8_mb_preds(const FFHipVp8Mb *mb, int mb_x, int mb_y, int fullpel_chroma, FFHipVp8Pred out[24]);
typedef struct FFHipVp8IntraModes {
    uint8_t mode16;                    /* the pred16x16[] slot (FFHIP_VP8_PRED_*); FFHIP_VP8_PRED_NONE for I4x4 (4 is LEFT_DC's slot) */
    uint8_t chroma;                    /* the pred8x8[] slot */
    uint8_t sub[16];                   /* I4x4: the pred4x4[] slots (FFHIP_VP8_B_*) */
    uint8_t copy[16];                  /* I4x4: 1 where intra_predict() predicts into its bordered copy_dst */
} FFHipVp8IntraModes;
/** Device-free.  The slots intra_predict() takes for `mb` at (mb_x, mb_y) after the edge substitutions.  FFHIP_EINVAL for NULL, an
 *  inter record, a mode out of range or a negative mb_x / mb_y. */
int ffhip_vp8_intra_modes(const FFHipVp8Mb *mb, int mb_x, int mb_y, FFHipVp8IntraModes *out);

/**
 * vp9dsp above 8 bits (profiles 2 / 3): the batch faces above at the bpp ff_vp9dsp_init(dsp, bpp, bitexact) instantiates its template
 * for (libavcodec/vp9dsp.c:88-112, vp9dsp_10bpp.c / vp9dsp_12bpp.c).  bit_depth 8, 10 or 12.  Samples are uint16_t above 8 bits,
 * itxfm_add's coefficients int32_t (the reference's dctcoef; FFHipVp9TU.coeff_offset counts coefficients) and its butterflies run
 * in 64 bits (dctint = int64_t); record offsets and strides stay in BYTES; E / I / H of the loop filter are the 8-bit-unit values
 * the decoder passes (scaled by << (bit_depth - 8) inside, vp9dsp_template.c:1784-1788); FFHipVp9Intra.edge_offset addresses an
 * edge line of uint16_t samples.
 */
int ffhip_vp9_itxfm_add_batch_dev_hbd(int bit_depth, int tx, void *coeffs, uint8_t *dst, ptrdiff_t stride, const FFHipVp9TU *tus, int n,
                                      void *stream);
int ffhip_vp9_mc_batch_dev_hbd(int bit_depth, uint8_t *dst, ptrdiff_t dststride, const uint8_t *src, ptrdiff_t srcstride,
                               const FFHipVp9McBlock *blocks, int n, void *stream);
int ffhip_vp9_scaled_mc_batch_dev_hbd(int bit_depth, uint8_t *dst, ptrdiff_t dststride, const uint8_t *src, ptrdiff_t srcstride,
                                      const FFHipVp9ScaledBlock *blocks, int n, void *stream);
int ffhip_vp9_loop_filter_batch_dev_hbd(int bit_depth, uint8_t *base, ptrdiff_t stride, const FFHipVp9Edge *edges, int n, void *stream);
int ffhip_vp9_intra_pred_batch_dev_hbd(int bit_depth, int tx, uint8_t *dst, ptrdiff_t stride, const uint8_t *edges,
                                       const FFHipVp9Intra *blocks, int n, void *stream);



/* ------------------------------------------------------------------------------------------ */
/* libavcodec: me_cmp + full search                                                           */
/* ------------------------------------------------------------------------------------------ */
/** me_cmp_func (libavcodec/me_cmp.h:45-48); the context argument is unused by these metrics
 *  (checkasm passes NULL, tests/checkasm/motion.c:75). */
typedef int (*ffhip_me_cmp_func)(void *c, const uint8_t *blk1, const uint8_t *blk2, ptrdiff_t stride, int h);
typedef struct FFHipMECmpContext {
    ffhip_me_cmp_func sad[2];             /* [0] 16 wide = pix_abs16_c, [1] 8 wide = pix_abs8_c */
    ffhip_me_cmp_func hadamard8_diff[2];  /* [0] hadamard8_diff16_c, [1] hadamard8_diff8x8_c     */
    ffhip_me_cmp_func pix_abs[2][1];      /* [w][0] full-pel                                     */
    /* what a motion search uses beside them (me_cmp.c:961-1012): the half-pel SADs pix_abs[w][1..3] = _x2 / _y2 / _xy2 (blk2 read
     * one column / row / both further), sse[0..1] and nsse[0..1] ([0] 16 wide, [1] 8 wide).  nsse weighs its second term with the
     * encoder's nsse_weight when the context argument is non-NULL: such calls go to the displaced C function, NULL means 8 */
    ffhip_me_cmp_func pix_abs_hpel[2][3];
    ffhip_me_cmp_func sse[2];
    ffhip_me_cmp_func nsse[2];
} FFHipMECmpContext;
int ff_me_cmp_init_hip(FFHipMECmpContext *c);

#define FFHIP_ME_SAD   0
#define FFHIP_ME_SATD  1
#define FFHIP_ME_SAD_X2  2   /* pix_abs*_x2_c: blk2 averaged with its right neighbour (w + 1 columns read) */
#define FFHIP_ME_SAD_Y2  3   /* pix_abs*_y2_c: ... with the row below (h + 1 rows read)                  */
#define FFHIP_ME_SAD_XY2 4   /* pix_abs*_xy2_c: ... with all three                                       */
#define FFHIP_ME_SSE     5   /* sse16_c / sse8_c                                                          */
#define FFHIP_ME_NSSE    6   /* nsse16_c / nsse8_c with the context-free weight 8                         */
/** n independent comparisons: out[i] = cmp(blk1 + off1[i], blk2 + off2[i], stride, h). width 16|8. */
int ffhip_me_cmp_batch_dev(int kind, int width, int h, const uint8_t *blk1, const int32_t *off1,
                           const uint8_t *blk2, const int32_t *off2, ptrdiff_t stride, int32_t *out, int n,
                           void *stream);
/**
 * Exhaustive search, semantics of ff_me_search_esa() driven as vf_mestimate does
 * (libavfilter/motion_estimation.c:78-95, COST_MV :32-40; libavfilter/vf_mestimate.c:101,119-129):
 * for every mb_size x mb_size block of `cur`, window [x_mb±R]∩[0,(b_w-1)*mb]×[y_mb±R]∩[0,(b_h-1)*mb],
 * zero-MV evaluated first (and returned at once when its cost is 0), then raster scan with strict <.
 * cost_kind FFHIP_ME_SAD reproduces the filter bit-exactly; FFHIP_ME_SATD swaps the metric for
 * hadamard8_diff (libavcodec/me_cmp.c:514-562,933-950) under the same search order.
 * Outputs per block (raster): mv_out[2*b+{0,1}] = absolute best (x,y) as int16, cost_out[b] u32.
 * nframes frame pairs, frame f at cur + f*frame_pitch / ref + f*frame_pitch.
 */
int ffhip_me_esa_batch_dev(const uint8_t *cur, const uint8_t *ref, int width, int height, ptrdiff_t stride,
                           size_t frame_pitch, int nframes, int mb_size, int search_param, int cost_kind,
                           int16_t *mv_out, uint32_t *cost_out, void *stream);

#define FFHIP_ME_METHOD_ESA   1   /* == AV_ME_METHOD_* (libavfilter/motion_estimation.h) */
#define FFHIP_ME_METHOD_TSS   2
#define FFHIP_ME_METHOD_TDLS  3
#define FFHIP_ME_METHOD_NTSS  4
#define FFHIP_ME_METHOD_FSS   5
#define FFHIP_ME_METHOD_DS    6
#define FFHIP_ME_METHOD_HEXBS 7
#define FFHIP_ME_METHOD_EPZS  8   /* ffhip_me_search_pred_batch_dev(); refused by the per-block face: FFHIP_ENOSYS */
#define FFHIP_ME_METHOD_UMH   9   /* the same */
/**
 * The filter's per-block searches (what vf_mestimate's SEARCH_MV(method) runs over a frame pair), every block of nframes pairs in one
 * launch on `stream`.  Geometry, frame addressing, metrics and outputs are ffhip_me_esa_batch_dev()'s: log2mb = log2(mb_size),
 * b_w = width >> log2mb, b_h = height >> log2mb, blocks in raster order at (x_mb, y_mb) = (bx << log2mb, by << log2mb), the window
 * x_min = max(0, x_mb - R), x_max = min(x_mb + R, (b_w - 1) << log2mb) and the same for y; mv_out[2 * b + {0, 1}] the absolute best
 * position, cost_out[b] its cost.  Every candidate evaluated lies in the window, so no read leaves the width x height plane.
 *
 * The rules below are RESTATED, NOT CHECKED AGAINST THE SOURCE (libavfilter/motion_estimation.c was not at hand); this text is the
 * definition the tests pin (kernels/me_search_rules.h is its one implementation, tests/me_search_model.py the model written from it).
 *   cost(x, y): the metric between the current block at (x_mb, y_mb) and the reference block at absolute (x, y); FFHIP_ME_SAD is
 *     ff_me_cmp_sad, FFHIP_ME_SATD hadamard8_diff16 / hadamard8_diff8x8 with blk1 = current.
 *   COST_MV(x, y): c = cost(x, y); if (c < cost_min) { cost_min = c; mv = (x, y); } — strict.  COST_P_MV(x, y): COST_MV only if (x, y)
 *     is inside the window, nothing otherwise.  The candidates of an iteration are applied in table order: on equal costs the earliest
 *     wins, and an equal cost never displaces the centre.
 *   Tables (dx, dy): sqr1 = (0,-1) (0,1) (-1,0) (1,0) (-1,-1) (-1,1) (1,-1) (1,1); dia1 = (-1,0) (0,-1) (1,0) (0,1);
 *     dia2 = (-2,0) (-1,-1) (0,-2) (1,-1) (2,0) (1,1) (0,2) (-1,1); hex2 = (-2,0) (-1,-2) (-1,2) (1,-2) (1,2) (2,0).
 *   Start: mv = (x_mb, y_mb), cost_min = cost(x_mb, y_mb); 0 returns at once.  Below (x, y) is the centre copied from mv at the top of an
 *     iteration, step0 = (R + 1) >> 1, and every candidate goes through COST_P_MV.
 *   ESA  (1): the raster scan of the window with COST_MV.  The device face forwards to ffhip_me_esa_batch_dev()'s launcher.
 *   TSS  (2): step = step0; do { the 8 of sqr1 * step; step >>= 1; } while (step > 0).
 *   TDLS (3): step = step0; do { the 4 of dia1 * step; if mv is still (x, y), step >>= 1; } while (step > 0).
 *   NTSS (4): step = step0, first = 1; do { the 8 of sqr1 * step; if (first) { the 8 of sqr1 * 1 round the same (x, y); if mv == (x, y)
 *     return; if |x - mv.x| <= 1 and |y - mv.y| <= 1 { (x, y) = mv; the 8 of sqr1 * 1 round it; return; } first = 0; } step >>= 1; }
 *     while (step > 0).
 *   FSS  (5): step = 2; do { the 8 of sqr1 * step; if mv is still (x, y), step >>= 1; } while (step > 0).
 *   DS   (6): do { the 8 of dia2 } while (mv != (x, y)); then the 4 of dia1 round the last (x, y).
 *   HEXBS(7): do { the 6 of hex2 } while (mv != (x, y)); then the 4 of dia1 round the last (x, y).
 *   EPZS (8) and UMH (9) take the neighbouring blocks' vectors of the current and the previous frame (a raster dependency plus the
 *     filter's predictor bookkeeping): FFHIP_ENOSYS with a text that names the method.
 * mb_size 16 or 8, cost_kind FFHIP_ME_SAD or FFHIP_ME_SATD, search_param >= 0 (0: each step method collapses to the centre), nframes >= 0
 * (0: nothing is done); a picture smaller than one block has no blocks.  FFHIP_EINVAL (before any device check): NULL pointers, a method
 * outside 1..9, another mb_size or cost_kind, a negative width, height, nframes or search_param, stride < width, nframes > 1 with
 * frame_pitch < stride * height, more than 2^31 - 1 blocks.  FFHIP_ENOSYS without a device, after the checks.
 */
int ffhip_me_search_batch_dev(int method, const uint8_t *cur, const uint8_t *ref, int width, int height, ptrdiff_t stride,
                              size_t frame_pitch, int nframes, int mb_size, int search_param, int cost_kind,
                              int16_t *mv_out, uint32_t *cost_out, void *stream);
/** The same rules compiled for the CPU, on host arrays (device-free): the same arguments but the stream, the same refusals but the
 *  one for a missing device, the same bytes.  Method 1 runs the start and the raster scan from the rules header too. */
int ffhip_me_search_frames_host(int method, const uint8_t *cur, const uint8_t *ref, int width, int height, ptrdiff_t stride,
                                size_t frame_pitch, int nframes, int mb_size, int search_param, int cost_kind,
                                int16_t *mv_out, uint32_t *cost_out);
/** What the calling thread's last successful ffhip_me_search_frames_host() or ffhip_me_search_pred_frames_host() did: the blocks it
 *  searched and the costs it evaluated (the start of each block included).  Either pointer may be NULL. */
void ffhip_me_search_host_counts(uint64_t *blocks, uint64_t *costs);

/**
 * The filter's two predictive searches, EPZS (8, vf_minterpolate's default) and UMH (9), every block of nframes pairs in one launch on
 * `stream`.  Geometry, frame addressing, metrics, window and outputs are ffhip_me_search_batch_dev()'s: mv_out holds absolute best
 * positions, cost_out their costs.  A block takes the vectors of its left, top and top-right neighbours of the same pair, so the blocks
 * of a pair are searched in wavefront order (one wave per block row, kernels/row_handoff.h); the nframes pairs of a call are independent
 * of each other (different streams, or the two directions of one frame).
 *
 * prev1 / prev2: the vector fields of the previous and of the one-before-previous frame pair (the filter's mv_table[1] and
 * mv_table[2]) in the layout of mv_out: nframes fields of b_w * b_h absolute positions.  rel(b), a block's relative vector, is its
 * position minus the block's origin (x_mb, y_mb); rel1 and rel2 are those of prev1 and prev2.  Either may be NULL: a field of zero
 * vectors (the filter's zero-initialised tables at the first frame).  A caller chains a sequence by rotating three buffers, one call per
 * frame on one stream — or hands the whole sequence to ffhip_me_search_pred_sequence_dev() below, which chains the pairs inside one
 * launch.  UMH reads neither.  Any int16 content is legal: relative vectors are formed in 32 bits, and a candidate outside
 * the window is refused by COST_P_MV as always.
 *
 * The rules below are RESTATED, NOT CHECKED AGAINST THE SOURCE (libavfilter/motion_estimation.c and vf_mestimate.c were not at hand);
 * this text is the definition the tests pin (kernels/me_search_pred_rules.h is its one implementation, tests/me_pred_search_model.py the
 * model written from it).  cost, COST_MV (strict <), COST_P_MV (only inside the window), dia1 and hex2 are those of
 * ffhip_me_search_batch_dev() above.
 *   Start, both methods: mv = (x_mb, y_mb), cost_min is "none yet" and the first cost evaluated always takes it; there is NO early
 *     return at cost 0.  Predictor (0,0) is always evaluated and always lies in the window, so every block ends with a real cost.
 *   Predictor lists, as vf_mestimate fills them — entries are simply appended, duplicates stay and are evaluated again:
 *     EPZS  P0 = (0,0); rel(left block) if bx > 0; rel(top block) if by > 0; rel(top-right block) if by > 0 && bx + 1 < b_w.  The median
 *           is taken from P0 as it stands at that point, n its count, mid the median of three per component: n == 4:
 *           mid(P0[1], P0[2], P0[3]); n == 3: mid((0,0), P0[1], P0[2]); n == 2: P0[1]; otherwise (0,0).  Then rel1(b), the collocated
 *           block of prev1, is appended to P0.  P1 = the accelerator 2 * rel1(b) - rel2(b); rel1 of the left neighbour if bx > 0; of the
 *           top neighbour if by > 0; of the right neighbour if bx + 1 < b_w; of the bottom neighbour if by + 1 < b_h.
 *     UMH   P0 = (0,0); rel(left block) if bx > 0; if by > 0: rel(top block), then rel(top-right block) if bx + 1 < b_w, else
 *           rel(top-left block) if bx > 0.  The median by the same rule.  No P1.
 *   EPZS (8): COST_P_MV(origin + median); each entry of P0 in order; each entry of P1 in order (all as origin + entry, through
 *     COST_P_MV); then do { (x, y) = mv; the 4 of dia1 round (x, y); } while (mv != (x, y)).
 *   UMH  (9), R = search_param:
 *     1. the median, then each entry of P0;
 *     2. the cross, (x, y) = mv: for (d = 1; d <= R; d += 2) { (x - d, y); (x + d, y); if (d <= R / 2) { (x, y - d); (x, y + d); } };
 *     3. the 5 x 5 raster with COST_MV, bounds from mv as it is after the cross: for y = max(y_min, mv.y - 2) .. min(mv.y + 2, y_max),
 *        for x likewise (mv's own position is evaluated again);
 *     4. the rings, (x, y) = mv: for (d = 1; d <= R / 4; d++) entries 1 .. 15 of hex4, scaled by d;
 *        hex4 = (-4,-2) (-4,-1) (-4,0) (-4,1) (-4,2) (4,-2) (4,-1) (4,0) (4,1) (4,2) (-2,3) (0,4) (2,3) (-2,-3) (0,-4) (2,-3);
 *        entry 0 is never evaluated;
 *     5. do { (x, y) = mv; the 6 of hex2 round (x, y); } while (mv != (x, y));
 *     6. the 4 of dia1 round the last (x, y).
 *   The d loops may stop at the first d beyond which every candidate lies outside the window: what is left out is refused anyway, so
 *   vectors, costs and cost counts do not change, and the work is bounded for any search_param >= 0.
 * FFHIP_EINVAL (before any device check, each with a text): what ffhip_me_search_batch_dev() refuses; a method other than 8
 * or 9; a width or height above 32768 (positions would not fit int16); mv_out not 4-byte aligned; mv_out sharing a byte with prev1,
 * prev2, cur, ref or cost_out.  FFHIP_ENOSYS without a device, after the checks.  A lost hand-off between rows (never in a correct run)
 * is reported by ffhip_stream_synchronize() as FFHIP_EIO.
 */
int ffhip_me_search_pred_batch_dev(int method, const uint8_t *cur, const uint8_t *ref, int width, int height, ptrdiff_t stride,
                                   size_t frame_pitch, int nframes, int mb_size, int search_param, int cost_kind,
                                   const int16_t *prev1, const int16_t *prev2, int16_t *mv_out, uint32_t *cost_out, void *stream);
/** The same rules compiled for the CPU, on host arrays (device-free), blocks in raster order: the same arguments but the stream, the
 *  same refusals but the one for a missing device, the same bytes. */
int ffhip_me_search_pred_frames_host(int method, const uint8_t *cur, const uint8_t *ref, int width, int height, ptrdiff_t stride,
                                     size_t frame_pitch, int nframes, int mb_size, int search_param, int cost_kind,
                                     const int16_t *prev1, const int16_t *prev2, int16_t *mv_out, uint32_t *cost_out);

/**
 * The same two searches of whole sequences, every pair chained to the fields of the two pairs before it inside the launch.  There are
 * nseq independent sequences of nframes pictures each; picture p of sequence s is at frames + s * seq_pitch + p * frame_pitch, and a
 * sequence has np = nframes - 1 pairs.  direction 0 is the filter's dir 0: pair k is cur = picture k + 1, ref = picture k; direction 1
 * is its dir 1: cur = picture k, ref = picture k + 1.  (The two directions of vf_minterpolate's bidirectional mode are two calls, or two
 * sequences over differently ordered pictures; they are not interleaved here.)
 *
 * Outputs are pair-major, per = b_w * b_h: the field of pair k of sequence s starts at mv_out + 2 * per * (k * nseq + s), its costs at
 * cost_out + per * (k * nseq + s), so step k's nseq fields are one contiguous batch in the layout of ffhip_me_search_pred_batch_dev().
 * init1 / init2 hold nseq fields each in that layout: the fields of the pairs before pair 0 (k = -1 and k = -2); NULL means zero vectors.
 * A caller continues a sequence across calls by passing the last two steps of the previous call's mv_out.
 *
 * DEFINITION: the bytes of mv_out and cost_out are those of this loop of calls of the pair face —
 *   for k in 0 .. np - 1:
 *       prev1 = k >= 1 ? field step k - 1 : init1;   prev2 = k >= 2 ? field step k - 2 : (k == 1 ? init1 : init2)
 *       ffhip_me_search_pred_batch_dev(method, cur_k, ref_k, ..., frame_pitch = seq_pitch, nframes = nseq, ..., prev1, prev2,
 *                                      field step k, cost step k, stream)
 * — and no search rule is added.  Block (bx, r) of pair k reads of pair k - 1 only the collocated block and its four neighbours, so pair k
 * runs about three block steps behind pair k - 1: a sequence is a wavefront over (pair, row), one wave per block row of a pair
 * (kernels/me_search_seq.hip).  UMH reads no prev field; its pairs run unchained in the same launches.
 *
 * FFHIP_EINVAL (before any device check, each with a text): what ffhip_me_search_pred_batch_dev() refuses, applied to the pictures (NULL
 * frames, mv_out or cost_out, the method, mb_size, cost_kind, negative sizes, stride < width, a width or height above 32768, mv_out not
 * 4-byte aligned); direction outside 0..1; nseq < 0; nframes > 1 with frame_pitch < stride * height; nseq > 1 with
 * seq_pitch < (nframes - 1) * frame_pitch + stride * height; mv_out sharing a byte with init1, init2, frames or cost_out; more than
 * 2^31 - 1 blocks in total.  nframes <= 1, nseq == 0 or a picture smaller than a block: nothing is done, 0.  FFHIP_ENOSYS without a
 * device, after the checks.  A lost hand-off (never in a correct run) is reported by ffhip_stream_synchronize() as FFHIP_EIO.
 */
int ffhip_me_search_pred_sequence_dev(int method, const uint8_t *frames, int width, int height, ptrdiff_t stride, size_t frame_pitch,
                                      int nframes, size_t seq_pitch, int nseq, int direction, int mb_size, int search_param, int cost_kind,
                                      const int16_t *init1, const int16_t *init2, int16_t *mv_out, uint32_t *cost_out, void *stream);
/** The same loop on host arrays (device-free), blocks in raster order: the same arguments but the stream, the same refusals but the
 *  one for a missing device, the same bytes.  ffhip_me_search_host_counts() reports the blocks and costs of all its pairs. */
int ffhip_me_search_pred_sequence_host(int method, const uint8_t *frames, int width, int height, ptrdiff_t stride, size_t frame_pitch,
                                       int nframes, size_t seq_pitch, int nseq, int direction, int mb_size, int search_param, int cost_kind,
                                       const int16_t *init1, const int16_t *init2, int16_t *mv_out, uint32_t *cost_out);

/**
 * Bilateral motion estimation (vf_minterpolate's me_mode=bilat, the filter's default): EPZS (8) and UMH (9) of nframes independent pairs
 * in one launch on `stream`, under the bilateral cost.  One search per pair: picture A is `cur`, picture B is `ref`, and the vector of a
 * block is a HALF-vector v of a block of the picture halfway between them — A is sampled at +v and B at -v.  The arguments are
 * ffhip_me_search_pred_batch_dev()'s without cost_kind.  mv_out and cost_out have the same layouts; mv_out holds the absolute positions
 * (x_mb + v.x, y_mb + v.y).
 *
 * The rule below is RESTATED FROM MEMORY and NOT CHECKED against libavfilter/vf_minterpolate.c, which was not at hand; this text is the
 * definition the tests pin (kernels/me_search_bilat_rules.h is its one implementation beside the search rules of
 * kernels/me_search_pred_rules.h, tests/me_bilat_model.py the model written from it).
 *   Geometry, the window (x_min, x_max, y_min, y_max) and COST_MV / COST_P_MV are those of ffhip_me_search_batch_dev().  The predictor
 *   lists, the median and the phases are those of ffhip_me_search_pred_batch_dev(); the list's vectors are the relative vectors of this
 *   face's own fields (mv_out, prev1, prev2).  Only cost differs.  h = mb / 2; clip(v, lo, hi) = v < lo ? lo : v > hi ? hi : v.
 *   cost(X, Y) of the block at (x_mb, y_mb) (the filter's get_sbad_ob):
 *     lo_x = x_min + h, hi_x = x_max - h;  cx = clip(x_mb, lo_x, hi_x);  rx = min(cx - lo_x, hi_x - cx);  dx = clip(X - cx, -rx, rx);
 *     the same gives cy, dy;
 *     sbad = sum of |A[cy + dy + j][cx + dx + i] - B[cy - dy + j][cx - dx + i]|, j and i each over -h .. 3 * h - 1: an overlapped window
 *       of twice the block size;
 *     cost = sbad + 64 * (|X - x_mb - pred.x| + |Y - y_mb - pred.y|), held in uint32_t.
 *   pred is the block's median predictor.  The pred rules compute it from the list as it stands; it is fixed before the block's first
 *   cost, whether or not the median candidate lies in the window.
 *   Reads stay inside the plane when lo <= hi, which holds for every block when search_param >= mb_size, b_w >= 2 and b_h >= 2; the faces
 *   refuse everything else, and the kernel takes no argument for which the inequality can fail.
 * Methods 1..7 (the per-block methods), SATD under this cost, depths above 8 bits and fusing the search with the compensation are not
 * here.
 * FFHIP_EINVAL (before any device check, each with a text): everything ffhip_me_search_pred_batch_dev() refuses; search_param < mb_size;
 * a picture of fewer than two block columns or two block rows when there is anything to search (nframes > 0 and at least one block).
 * FFHIP_ENOSYS with a text that names the method: methods 1..7.  The order: the shared argument checks; then the predictive faces'
 * checks of the field (sizes above 32768, mv_out's alignment, mv_out's overlaps), which a method 1..7 goes through like EPZS; then the
 * method (a method outside 1..9: FFHIP_EINVAL with the field checks, 1..7: FFHIP_ENOSYS); then search_param and the block counts.
 * FFHIP_ENOSYS without a device, after the checks.  A lost hand-off is reported as by the predictive faces.
 */
int ffhip_me_search_bilat_batch_dev(int method, const uint8_t *cur, const uint8_t *ref, int width, int height, ptrdiff_t stride,
                                    size_t frame_pitch, int nframes, int mb_size, int search_param, const int16_t *prev1,
                                    const int16_t *prev2, int16_t *mv_out, uint32_t *cost_out, void *stream);
/** The same rules compiled for the CPU, on host arrays (device-free), blocks in raster order: the same arguments but the stream, the
 *  same refusals but the one for a missing device, the same bytes.  ffhip_me_search_host_counts() reports its blocks and costs. */
int ffhip_me_search_bilat_frames_host(int method, const uint8_t *cur, const uint8_t *ref, int width, int height, ptrdiff_t stride,
                                      size_t frame_pitch, int nframes, int mb_size, int search_param, const int16_t *prev1,
                                      const int16_t *prev2, int16_t *mv_out, uint32_t *cost_out);
/** TEST HOOK of the host build, not part of the interface a caller should build on (it may change or go without notice): one cost of
 *  the rule above on host arrays, cost(x, y) of block (bx, by) of the pair (cur, ref) with the predictor (pred_x, pred_y), written to
 *  *cost.  It exists so that tests can pin the placement of the two windows apart from a search.  FFHIP_EINVAL with a text: what the
 *  pair face refuses of one pair's geometry, a NULL cost, a block outside the picture, a predictor component beyond +-32768, (x, y)
 *  outside the block's window. */
int ffhip_me_search_bilat_cost_host(const uint8_t *cur, const uint8_t *ref, int width, int height, ptrdiff_t stride, int mb_size,
                                    int search_param, int bx, int by, int x, int y, int pred_x, int pred_y, uint32_t *cost);
/**
 * The bilateral search of whole sequences in one launch: ffhip_me_search_pred_sequence_dev()'s arguments without cost_kind and
 * direction.  Pair k of a sequence is A = picture k, B = picture k + 1.  Outputs are pair-major, as there.
 * DEFINITION: the bytes of mv_out and cost_out are those of the loop of calls of ffhip_me_search_bilat_batch_dev() —
 *   for k in 0 .. np - 1:
 *       prev1 = k >= 1 ? field step k - 1 : init1;   prev2 = k >= 2 ? field step k - 2 : (k == 1 ? init1 : init2)
 *       ffhip_me_search_bilat_batch_dev(method, picture k, picture k + 1, ..., frame_pitch = seq_pitch, nframes = nseq, ..., prev1, prev2,
 *                                       field step k, cost step k, stream)
 * — the chaining of the existing sequence face, word for word.  Refusals: those of ffhip_me_search_pred_sequence_dev() (direction apart)
 * and of the pair face above; "anything to search" is nframes > 1, nseq > 0 and at least one block.
 */
int ffhip_me_search_bilat_sequence_dev(int method, const uint8_t *frames, int width, int height, ptrdiff_t stride, size_t frame_pitch,
                                       int nframes, size_t seq_pitch, int nseq, int mb_size, int search_param, const int16_t *init1,
                                       const int16_t *init2, int16_t *mv_out, uint32_t *cost_out, void *stream);
/** The same loop on host arrays (device-free): the same arguments but the stream, the same refusals but the one for a missing device,
 *  the same bytes.  ffhip_me_search_host_counts() reports the blocks and costs of all its pairs. */
int ffhip_me_search_bilat_sequence_host(int method, const uint8_t *frames, int width, int height, ptrdiff_t stride, size_t frame_pitch,
                                        int nframes, size_t seq_pitch, int nseq, int mb_size, int search_param, const int16_t *init1,
                                        const int16_t *init2, int16_t *mv_out, uint32_t *cost_out);

/**
 * vf_minterpolate's motion-compensated interpolation of whole sequences in one launch: mi_mode=mci, me_mode=bidir, mc_mode=obmc — the
 * overlapped-block accumulation of bidirectional_obmc() and the per-pixel weighted average of set_frame_data() — and the filter's
 * scene-change fallback, the blend.  It consumes the fields of two ffhip_me_search_pred_sequence_dev() calls (direction 0 and 1), so
 * frame-rate conversion is search forward, search backward, interpolation on one stream with no host round trip.  Fusing search and
 * compensation into one launch, mc_mode=aobmc, vsbmc and depths above 8 bits are not here (me_mode=bilat has faces of its own:
 * ffhip_me_search_bilat_sequence_dev() above, ffhip_me_interp_bilat_sequence_dev() below): in this face the caller
 * decides per job between MCI and BLEND (ffhip_me_scene_sequence_dev() and ffhip_me_interp_sequence_scd_dev() below take that decision
 * on the device), and the other modes stay on the CPU.
 *
 * Pictures are 8-bit planar, nplanes 1 (luma alone) or 3; picture p of sequence s, plane i, is at
 * base[i] + s * seq_pitch[i] + p * frame_pitch[i], rows stride[i] apart.  Job j interpolates between pictures A = `pair` and
 * B = `pair` + 1 of sequence `seq` at instant alpha (0 .. 1024; 0 is A's instant, 1024 is B's) and writes output picture j, at
 * dst->base[i] + j * dst->frame_pitch[i] (dst->seq_pitch is ignored).  Any number of jobs may name the same pair.  All jobs run in one
 * launch (in launches of 1024 jobs: a launch's jobs travel with the window table in one small device table).
 *
 * The rule below is RESTATED FROM MEMORY and NOT CHECKED against libavfilter/vf_minterpolate.c, which was not at hand; this text is the
 * definition the tests pin (kernels/me_interp_rules.h is its one implementation, tests/me_interp_model.py the model written from it).
 *   Geometry is that of the search faces: mb = mb_size (16 or 8), log2mb its logarithm, b_w = width >> log2mb, b_h = height >> log2mb,
 *     per = b_w * b_h.  Vector fields are in the sequence face's pair-major layout: the field of pair k of sequence s starts at
 *     mv + 2 * per * (k * nseq + s); entry b = by * b_w + bx holds an absolute position (X, Y), and its relative vector is
 *     v = (X - (bx << log2mb), Y - (by << log2mb)), formed in 32 bits.  mv_fwd is a direction-0 field (cur = B, ref = A), mv_bwd a
 *     direction-1 field (cur = A, ref = B).  tdiv(n) = n / 1024 is C division (towards zero); clip(v, lo, hi) is av_clip; W and H are
 *     the luma width and height.
 *   The contribution list of luma pixel (x, y) is built in the order dir = 0, 1; then by = 0 .. b_h - 1; then bx = 0 .. b_w - 1.  For
 *   each block:
 *     1. v is the block's relative vector, from mv_fwd for dir 0 and from mv_bwd for dir 1.  If |v.x| > mv_range or |v.y| > mv_range the
 *        block is malformed and contributes nothing.  (A search window guarantees |v| <= search_param: a caller passes its
 *        search_param as mv_range.)
 *     2. a = dir ? alpha : 1024 - alpha;  sx = (bx << log2mb) - mb / 2 + tdiv(v.x * a), sy the same in y.
 *     3. x0 = clip(sx, 0, W - 1), x1 = clip(sx + 2 * mb, 0, W - 1), y0 and y1 the same with H.  The block covers the pixel iff
 *        x0 <= x < x1 and y0 <= y < y1 — so column W - 1 and row H - 1 are never covered (the reference's behaviour, kept).
 *     4. w = window[(x - sx) + (y - sy) * 2 * mb].  If w == 0, skip.  If the list already holds 16 contributions, skip (the reference's
 *        nb + 1 >= NB_PIXEL_MVS with two entries per contribution).
 *     5. m = dir ? -v : v.  Append one contribution of two entries: entry one takes its sample from A with weight w * (1024 - alpha) and
 *        displacement (clip(tdiv(m.x * alpha), -x, W - 1 - x), clip(tdiv(m.y * alpha), -y, H - 1 - y)); entry two takes its sample
 *        from B with weight w * alpha and displacement (clip(tdiv(-m.x * (1024 - alpha)), -x, W - 1 - x), the same in y).  The tdiv
 *        arguments are the 32-bit products (-m.x) * (1024 - alpha), not a negated quotient.
 *   An empty list is replaced by (A, 1024 - alpha, (0, 0)), (B, alpha, (0, 0)).
 *   Luma sample (x, y): S = sum of weight_i * ref_i[y + dy_i][x + dx_i], Wt = sum of weight_i, both unsigned 64-bit; the sample is
 *     (S + (Wt >> 1)) / Wt.  (Wt is 1024 times the sum of the w taken, so never 0, and both sums fit 32 bits.)
 *   Chroma sample (cx, cy) of plane 1 or 2, shifts sw = log2_chroma_w and sh = log2_chroma_h, plane size ceil(W / 2^sw) x ceil(H / 2^sh):
 *     the reference walks luma positions and lets the last writer win, so the sample uses the list of luma pixel
 *     x = min(((cx + 1) << sw) - 1, W - 1), y = min(((cy + 1) << sh) - 1, H - 1); entry i reads ref_i's chroma plane at
 *     ((x >> sw) + dx_i / (1 << sw), (y >> sh) + dy_i / (1 << sh)), C divisions; the rounding is that of luma.
 *   The displacement clips keep every read inside its plane: 0 <= x + dx <= W - 1 gives 0 <= (x >> sw) + dx / (1 << sw) <= (W - 1) >> sw,
 *     the plane's last column; no sample outside the planes described by width, height and the shifts is read or written, and of the
 *     fields only the per entries of the jobs' pairs are read.
 *   FFHIP_ME_INTERP_BLEND: every sample of every plane is (alpha * B + (1024 - alpha) * A + 512) >> 10; the fields are not read.
 * window: the caller's table of (2 * mb_size)^2 bytes on the host (the filter passes its obmc_tab_linear[4 - log2mb]); any byte content
 * is legal.  jobs is on the host too.  A picture smaller than one block is legal: every MCI pixel then takes the empty-list fallback.
 *
 * FFHIP_EINVAL (before any device check, each with a text, identically in both faces): NULL src, dst, window or jobs; nplanes other
 * than 1 or 3; a NULL plane among the first nplanes; a chroma shift outside 0..1; another mb_size; mv_range outside 0..256; a negative
 * width, height, nframes, nseq or njobs; a width or height above 32768; a stride below its plane's width; nframes > 1 with
 * frame_pitch < stride * plane height, nseq > 1 with seq_pitch < (nframes - 1) * frame_pitch + stride * plane height, njobs > 1 with
 * dst->frame_pitch < stride * plane height (per plane); a job with seq outside 0..nseq - 1, pair outside 0..nframes - 2, alpha outside
 * 0..1024 or an unknown mode (the text names the job's index); NULL mv_fwd or mv_bwd when any job is MCI; dst sharing a byte with src or
 * with a field.  njobs == 0 (after the checks): nothing is done, 0.  FFHIP_ENOSYS without a device, after the checks.
 */
typedef struct FFHipMePlanes {   /* 8-bit planar; picture p of sequence s, plane i: base[i] + s * seq_pitch[i] + p * frame_pitch[i] */
    uint8_t *base[3]; ptrdiff_t stride[3]; size_t frame_pitch[3]; size_t seq_pitch[3];
} FFHipMePlanes;
typedef struct FFHipMeInterpJob { int32_t seq, pair, alpha, mode; } FFHipMeInterpJob;   /* 16 bytes == ffhip_me_interp_job_size() */
#define FFHIP_ME_INTERP_MCI   0
#define FFHIP_ME_INTERP_BLEND 1
int ffhip_me_interp_sequence_dev(const FFHipMePlanes *src, const FFHipMePlanes *dst, int nplanes /* 1 | 3 */, int log2_chroma_w, int log2_chroma_h,
                                 int width, int height, int nframes, int nseq, int mb_size, int mv_range,
                                 const uint8_t *window /* host, (2 * mb_size)^2 bytes */,
                                 const int16_t *mv_fwd, const int16_t *mv_bwd /* device, pair-major */,
                                 const FFHipMeInterpJob *jobs /* host */, int njobs, void *stream);
/** The same rule compiled for the CPU (device-free): the same arguments but the stream, everything on the host, the same refusals but
 *  the one for a missing device, the same bytes. */
int ffhip_me_interp_sequence_host(const FFHipMePlanes *src, const FFHipMePlanes *dst, int nplanes, int log2_chroma_w, int log2_chroma_h,
                                  int width, int height, int nframes, int nseq, int mb_size, int mv_range, const uint8_t *window,
                                  const int16_t *mv_fwd, const int16_t *mv_bwd, const FFHipMeInterpJob *jobs, int njobs);
/** What the calling thread's last successful ffhip_me_interp_sequence_host() did, over all its jobs.  Per luma pixel of an MCI job, as
 *  its list is built: [0] contributions taken, [1] skipped for weight 0, [2] skipped by the cap of 16, [5] entries (two per
 *  contribution) whose displacement a clip changed, [4] pixels on the empty-list fallback; [3] malformed blocks, per job and direction;
 *  [6] samples written, every plane and both modes; [7] those of them written by BLEND jobs. */
void ffhip_me_interp_host_counts(uint64_t counts[8]);
int ffhip_me_interp_job_size(void);

/**
 * vf_minterpolate's scene-change detection (detect_scene_change() with scd=fdiff) of whole sequences on the device, nothing read back:
 * the whole-picture SAD of every pair of consecutive pictures (the ff_scene_sad_get_fn() member that vf_scdet, vf_select and
 * vf_freezedetect call too), the score with its one carried double, and the threshold.  flags_out is what
 * ffhip_me_interp_sequence_scd_dev() takes as `scene`, so frame-rate conversion is search forward, search backward, detection,
 * interpolation: four calls on one stream with no host round trip.  Clearing the chained search's previous fields at a cut and fusing
 * the SAD into the search are not here.
 *
 * Pictures are one plane (luma); picture p of sequence s is at frames + s * seq_pitch + p * frame_pitch, rows `stride` bytes apart: the
 * layout of ffhip_me_search_pred_sequence_dev().  Samples are uint8_t at depth 8 and uint16_t at depths 9..16.
 *
 * The rule below is RESTATED FROM MEMORY and NOT CHECKED against libavfilter/vf_minterpolate.c and scene_sad.c, which were not at hand;
 * this text is the definition the tests pin (kernels/me_scene_rules.h is its one implementation, tests/me_scene_model.py the model).
 *   Pair k of sequence s is pictures A = k and B = k + 1 of that sequence.  Outputs are pair-major: pair k of sequence s is element
 *     k * nseq + s, the layout of the search and interpolation faces.
 *   sad(k, s) = the sum over the width x height samples of |A - B|, exact, uint64_t.  At depths 9..16 a sample is the full 16-bit value
 *     of its uint16_t (as ff_scene_sad16_c reads it), whatever `depth` says.  Bytes of a row beyond `width` samples are never read.
 *   mafd = (double)sad * 100.0 / (height * width) / (1 << depth): the int product, then the two divisions, in that order.
 *   diff = fabs(mafd - prev);  score = av_clipf((float)FFMIN(mafd, diff), 0.0f, 100.0f): the conversion to float is part of the rule.
 *   flag = (double)score >= threshold.
 *   prev = mafd afterwards.  Before pair 0 of sequence s, prev is mafd_in[s], or 0.0 when mafd_in is NULL; after the last pair it goes to
 *     mafd_out[s] when mafd_out is non-NULL, so a call continues another.
 *   The library is built with -ffp-contract=off and without fast-math: doubles and floats come out bit-identical on host and device.
 * sad_out (uint64_t), score_out (float) and flags_out (uint8_t, 0 or 1) hold one element per pair; any of the three may be NULL, not all.
 * Every element of every pair is overwritten: the caller clears nothing.  mafd_in and mafd_out hold nseq doubles.  All pointers are
 * device memory (naturally aligned for their type); the call is queued on `stream` and returns.  Any pair count runs: the sums of a
 * launch live in a small device table of 4096 pairs, and a call with more is split in stream order.
 * nframes <= 1 or nseq == 0: no pair output is written; mafd_out, when given, receives mafd_in (or zeros); 0.
 *
 * FFHIP_EINVAL (before any device check, each with a text, identically in both faces): NULL frames, or all three outputs NULL; depth
 * outside 8..16; width or height outside 1..32768; a negative nframes or nseq; stride below the row's bytes; above 8 bits an odd frames
 * address, stride, frame_pitch or seq_pitch; nframes > 1 with frame_pitch < stride * height; nseq > 1 with seq_pitch <
 * (nframes - 1) * frame_pitch + stride * height; threshold not a number in 0..100; an output (mafd_out counts as one) sharing a byte with
 * frames, with mafd_in or with another output; more than 2^31 - 1 pairs.  FFHIP_ENOSYS without a device, after the checks.
 */
int ffhip_me_scene_sequence_dev(const uint8_t *frames, int depth, int width, int height, ptrdiff_t stride, size_t frame_pitch, int nframes,
                                size_t seq_pitch, int nseq, double threshold, const double *mafd_in, double *mafd_out, uint64_t *sad_out,
                                float *score_out, uint8_t *flags_out, void *stream);
/** The same rule compiled for the CPU (device-free): the same arguments but the stream, everything on the host, the same refusals but
 *  the one for a missing device, the same bits. */
int ffhip_me_scene_sequence_host(const uint8_t *frames, int depth, int width, int height, ptrdiff_t stride, size_t frame_pitch, int nframes,
                                 size_t seq_pitch, int nseq, double threshold, const double *mafd_in, double *mafd_out, uint64_t *sad_out,
                                 float *score_out, uint8_t *flags_out);

/**
 * ffhip_me_interp_sequence_dev() with its MCI-or-fallback choice taken from device memory: `scene` holds one flag byte per pair,
 * pair-major (nframes - 1 steps of nseq bytes: flags_out of ffhip_me_scene_sequence_dev()).  A job whose mode is FFHIP_ME_INTERP_MCI and
 * whose pair's flag is non-zero runs `scene_action` instead:
 *   FFHIP_ME_SCENE_BLEND  the blend of FFHIP_ME_INTERP_BLEND;
 *   FFHIP_ME_SCENE_DUP    every plane of picture A is copied when alpha <= 512, else of picture B (the filter's "duplicate frame" at a
 *                         cut, alpha > ALPHA_MAX / 2).
 * Both are offered because this restatement is not certain which one the reference takes.  Job modes stay 0 or 1: DUP is reached only
 * through a flag.  A flag on a BLEND job changes nothing; scene NULL gives exactly ffhip_me_interp_sequence_dev()'s bytes.  In the
 * kernel the choice is one uniform byte load per workgroup.  ffhip_me_interp_host_counts() keeps its eight meanings after the host
 * face; samples written by either action count under [7].
 * FFHIP_EINVAL: everything ffhip_me_interp_sequence_dev() refuses, an unknown scene_action, dst sharing a byte with scene.
 */
#define FFHIP_ME_SCENE_BLEND 1
#define FFHIP_ME_SCENE_DUP   2
int ffhip_me_interp_sequence_scd_dev(const FFHipMePlanes *src, const FFHipMePlanes *dst, int nplanes, int log2_chroma_w, int log2_chroma_h,
                                     int width, int height, int nframes, int nseq, int mb_size, int mv_range, const uint8_t *window,
                                     const int16_t *mv_fwd, const int16_t *mv_bwd, const FFHipMeInterpJob *jobs, int njobs,
                                     const uint8_t *scene /* device, or NULL */, int scene_action, void *stream);
/** The same on the CPU: scene on the host. */
int ffhip_me_interp_sequence_scd_host(const FFHipMePlanes *src, const FFHipMePlanes *dst, int nplanes, int log2_chroma_w, int log2_chroma_h,
                                      int width, int height, int nframes, int nseq, int mb_size, int mv_range, const uint8_t *window,
                                      const int16_t *mv_fwd, const int16_t *mv_bwd, const FFHipMeInterpJob *jobs, int njobs,
                                      const uint8_t *scene /* host, or NULL */, int scene_action);

/**
 * The bilateral compensation (vf_minterpolate's me_mode=bilat with mc_mode=obmc: bilateral_obmc() for every block in raster order,
 * then set_frame_data()): ffhip_me_interp_sequence_scd_dev()'s arguments with ONE field `mv` — the half-vectors of
 * ffhip_me_search_bilat_sequence_dev(), pair-major — in place of mv_fwd / mv_bwd.  `scene` may be NULL; scene_action is as there.  Job
 * records, the window table, BLEND, DUP, the plane layouts and the counters of ffhip_me_interp_host_counts() keep their meanings
 * ([3] counts malformed blocks per job; entry [2] stays 0).  So a conversion under the filter's default mode is search, detection,
 * interpolation: three calls on one stream.
 *
 * RESTATED FROM MEMORY, NOT CHECKED against libavfilter/vf_minterpolate.c, which was not at hand; this text is the definition the tests
 * pin (kernels/me_interp_rules.h is its one implementation, tests/me_bilat_model.py the model written from it).  The list of luma pixel
 * (x, y) is built over by = 0 .. b_h - 1, then bx = 0 .. b_w - 1.  h = mb / 2.
 *   1. v is the block's relative vector.  If |v.x| or |v.y| exceeds mv_range, the block is malformed and contributes nothing.
 *   2. sx = (bx << log2mb) - h, sy the same in y.  The vector does not shift the window.
 *   3. x0 = clip(sx, 0, W - 1), x1 = clip(sx + 2 * mb, 0, W - 1); y0, y1 the same with H.  The pixel is covered iff x0 <= x < x1 and
 *      y0 <= y < y1.
 *   4. w = window[(x - sx) + (y - sy) * 2 * mb].  Skip when w is 0.
 *   5. m = 2 * v.  The two entries, the empty-list fallback, the luma average and the chroma rule follow the rule of
 *      ffhip_me_interp_sequence_dev() from its step 5 on, read with this m in place of its m.
 * At most four blocks reach a pixel (windows of 2 * mb stand mb apart: two per axis), so the cap of 16 never binds.
 * vsbmc, aobmc and the cluster pass that feeds them stay out.
 * FFHIP_EINVAL: everything ffhip_me_interp_sequence_scd_dev() refuses, read with `mv` for the two fields, each text naming these faces.
 */
int ffhip_me_interp_bilat_sequence_dev(const FFHipMePlanes *src, const FFHipMePlanes *dst, int nplanes, int log2_chroma_w, int log2_chroma_h,
                                       int width, int height, int nframes, int nseq, int mb_size, int mv_range, const uint8_t *window,
                                       const int16_t *mv /* device, pair-major */, const FFHipMeInterpJob *jobs, int njobs,
                                       const uint8_t *scene /* device, or NULL */, int scene_action, void *stream);
/** The same on the CPU (device-free): everything on the host, the same refusals but the one for a missing device, the same bytes. */
int ffhip_me_interp_bilat_sequence_host(const FFHipMePlanes *src, const FFHipMePlanes *dst, int nplanes, int log2_chroma_w, int log2_chroma_h,
                                        int width, int height, int nframes, int nseq, int mb_size, int mv_range, const uint8_t *window,
                                        const int16_t *mv, const FFHipMeInterpJob *jobs, int njobs, const uint8_t *scene, int scene_action);

/* ------------------------------------------------------------------------------------------ */
/* libavutil: av_tx float MDCT                                                               */
/* ------------------------------------------------------------------------------------------ */
typedef struct FFHipTXContext FFHipTXContext;
#define FFHIP_TX_FLOAT_FFT  0   /* == AV_TX_FLOAT_FFT  (libavutil/tx.h:47-132) */
#define FFHIP_TX_FLOAT_MDCT 1   /* == AV_TX_FLOAT_MDCT                          */
#define FFHIP_TX_FLOAT_RDFT 6   /* == AV_TX_FLOAT_RDFT (r2c forward, c2r inverse; libavutil/tx.h:70-90) */
#define FFHIP_TX_FLOAT_DCT  9   /* == AV_TX_FLOAT_DCT: DCT-II forward, DCT-III inverse (libavutil/tx.h:95-104), power of two 8..4096; as with av_tx_init the
                                   inverse is initialised with half the number of samples it transforms */
#define FFHIP_TX_FLOAT_DCT_I 12 /* == AV_TX_FLOAT_DCT_I, AV_TX_FLOAT_DST_I (libavutil/tx.h:107-128; ff_tx_dctI / ff_tx_dstI, tx_template.c:2006-2075): forward, */
#define FFHIP_TX_FLOAT_DST_I 15 /*    even len 4..1024 (64 in libavcodec/wmavoice.c:398-404); len reals in — `stride` bytes apart — len reals out; outputs as the
                                 *    C code's, its two middle ones at *scale != 1 included (kernels/tx_dcst1.hip); inverse contexts: FFHIP_ENOSYS */
#define FFHIP_TX_DOUBLE_FFT  2  /* == AV_TX_DOUBLE_FFT,  AV_TX_DOUBLE_MDCT (libavutil/tx.h:48-58; tx_double.c): rows of double, *scale a double */
#define FFHIP_TX_DOUBLE_MDCT 3
#define FFHIP_TX_INT32_FFT   4  /* == AV_TX_INT32_FFT, AV_TX_INT32_MDCT (libavutil/tx.h:59-69; tx_int32.c): rows of int32_t, *scale a float; the */
#define FFHIP_TX_INT32_MDCT  5  /*    fixed-point arithmetic of tx_priv.h:117-147 (64-bit products rounded to nearest, wrapping sums, the MDCT's
                                 *    input folded with >> 6).  Powers of two only: FFT 4 .. 8192 (double) / 16384 (int32) complex points, MDCT
                                 *    len 16 .. twice that; contiguous rows aligned to a complex sample; bit-identical to the C codelets
                                 *    (kernels/tx_wide.hip).  AV_TX_FULL_IMDCT is float-only. */
/* Refused — ffhip_tx_init() returns FFHIP_ENOSYS and the caller keeps the C / SIMD codelets (the reference's convention for an arch
 * that does not offer a transform: its codelet list simply has no entry, libavutil/tx.c:593-650):
 *   the RDFT / DCT / DCT-I / DST-I forms of the double and int32 types (7, 8, 10, 11, 13, 14, 16, 17) and their prime-factor lengths;
 *   inverse contexts of AV_TX_FLOAT_DCT_I / _DST_I (ff_tx_dcstI_init doubles their length, tx_template.c:2017-2021), their len 2 and len > 1024. */
#define FFHIP_TX_FULL_IMDCT        (1ULL << 2)   /* == AV_TX_FULL_IMDCT: an inverse MDCT writes 2 * len outputs (ff_tx_mdct_inv_full,
                                                  * libavutil/tx_template.c:1391-1408); batches: 8-byte aligned rows of 2 * len floats */
#define FFHIP_TX_REAL_TO_REAL      (1ULL << 3)   /* == AV_TX_REAL_TO_REAL: a forward RDFT writes the len/2 + 1 real parts only (ff_tx_rdft_r2r,
                                                  * libavutil/tx_template.c:1718-1827)                                                  */
#define FFHIP_TX_REAL_TO_IMAGINARY (1ULL << 4)   /* == AV_TX_REAL_TO_IMAGINARY: ... the len/2 imaginary parts only (ff_tx_rdft_r2i, :1829); the last one
                                                  * is, as in the reference, the underlying FFT's own value.  Both forward-only (EINVAL otherwise) */
#define FFHIP_TX_BITEXACT          (1ULL << 32)  /* libffhip's own: a bit neither AVTXFlags (bits 0..4, libavutil/tx.h:134-166) nor the
                                                  * codelet-private FF_TX_* flags (bits 58..63, tx_priv.h:154-159) use; av_tx_init() rejects
                                                  * unknown bits, so the wrapper never forwards it: float FFT (256 … 16384 points) and MDCT / RDFT / DCT contexts on 256, 512 and 1024 complex points run, by
                                                  * default, a radix-16 / -8 / -4 factorisation held in registers (kernels/tx_radix.hip) whose
                                                  * results agree with the C codelets within 2^-18 of a transform's largest output — the
                                                  * position FFmpeg's own SIMD codelets are in (tests/checkasm/av_tx.c compares with an
                                                  * epsilon).  With this flag the context runs the split-radix network in the C reference's
                                                  * operation order instead: bit-identical to ff_tx_*_float_c, at about half the rate.  Every
                                                  * other length and type is bit-identical either way. */
/** av_tx_fn (libavutil/tx.h:151) with an opaque context of ours in place of AVTXContext. */
typedef void (*ffhip_tx_fn)(FFHipTXContext *s, void *out, void *in, ptrdiff_t stride);
/**
 * Same argument meaning as av_tx_init() (libavutil/tx.h:169-172, libavutil/tx.c:903): type, inv,
 * len (MDCT: number of output coefficients of the forward transform, power of two 16..32768 (above 4096: contiguous 8-byte aligned
 * rows, one workgroup per transform) or one of the prime-factor
 * lengths 2 * 15 * 2^k, k = 2..6 = 120 / 240 / 480 / 960 / 1920 (CELT, AAC-960) and 2 * F * 2^k, F = 3 / 5 / 7 / 9, k = 2..8 (96- and
 * 768-sample AAC frames, Siren's 320, ...): ff_tx_mdct_pfa_<F>xM, libavutil/tx_template.c:1425-1600 — their batches must be
 * contiguous 8-byte aligned rows); FFT: number of complex samples, power of two 4..16384 or F * 2^k for F = 3 / 5 / 7 / 9 (k = 2..8) and
 * 15 (k = 2..7: 60 .. 1920) — ff_tx_fft_pfa over fft<F>_ns, libavutil/tx_template.c:948-1101; RDFT: number of real samples,
 * power of two 8..4096 — forward (r2c) reads len floats and writes len/2 + 1 complex bins, inverse (c2r) the other way round,
 * ff_tx_rdft_r2c / _c2r, libavutil/tx_template.c:1601-1716), *scale (FFT: ignored, may be NULL).  This is what the FFTXCodelet.init of a `ff_tx_codelet_list_float_hip[]` entry runs
 * (libavutil/tx_priv.h:199-237).  *fn receives the single-transform host-pointer shim.
 */
int  ffhip_tx_init(FFHipTXContext **ctx, ffhip_tx_fn *fn, int type, int inv, int len, const void *scale,
                   uint64_t flags);
void ffhip_tx_uninit(FFHipTXContext **ctx);
/**
 * Batched device face: transform t reads in + t*in_pitch floats... pitches in BYTES; out stride is
 * the av_tx_fn `stride` (bytes between output coefficients; sizeof(float) for contiguous).
 * Forward MDCT: in = 2*len floats, out = len floats.  Inverse: in = len floats (read with
 * `in_stride` bytes between coefficients), out = len floats (half-window iMDCT as the reference's
 * default; libavutil/tx_template.c:1312-1342).  FFT (either direction): in = out = len complex (re, im) floats,
 * contiguous and 8-byte aligned, `stride` ignored as in the reference (libavutil/tx_template.c:735-749); unnormalised.
 */
int  ffhip_tx_batch_dev(FFHipTXContext *ctx, void *out, size_t out_pitch, const void *in, size_t in_pitch,
                        ptrdiff_t stride, int ntransforms, void *stream);

/* =====================================================================================================================
 * swscale SwsOpBackend "hip" (SURVEY.md §8 f-1): the micro-op lists libswscale's new format layer hands a backend
 * (SwsOpBackend.compile / .compile_uops, libswscale/ops_dispatch.h:135-156) become one generated gfx950 kernel each.
 *
 * The structs below are LAYOUT-IDENTICAL to the reference's (the FFmpeg-side stub passes its own pointers through a cast and
 * static_asserts the sizes; oracle/refbuild/ffref_shim_ops.c holds those asserts for this repository's tests):
 *   FFHipSwsPixel == SwsPixel (uops.h:81-88), FFHipSwsFilterWeights == SwsFilterWeights (filters.h:83-121),
 *   FFHipSwsUOp == SwsUOp (uops.h:262-281), FFHipSwsOpExec == SwsOpExec (ops_dispatch.h:36-85);
 *   FFHIP_SWS_PIXEL_* == SwsPixelType (uops.h:43-50), FFHIP_SWS_UOP_* == SwsUOpType (uops.h:129-184).
 * Semantics of every micro-op are the C template backend's (libswscale/uops_tmpl.c, compiled without FP contraction,
 * uops_backend.c:24-35): results are bit-identical to backend_c for every type, floats included.
 * ===================================================================================================================== */
#define FFHIP_ENOTSUP (-95)   /* == AVERROR(ENOTSUP): the caller tries its next backend / splits the list (ops_dispatch.c:744-766) */

enum { FFHIP_SWS_PIXEL_NONE = 0, FFHIP_SWS_PIXEL_U8, FFHIP_SWS_PIXEL_U16, FFHIP_SWS_PIXEL_U32, FFHIP_SWS_PIXEL_F32 };
enum {
    FFHIP_SWS_UOP_INVALID = 0,
    FFHIP_SWS_UOP_READ_PLANAR, FFHIP_SWS_UOP_READ_PLANAR_FH, FFHIP_SWS_UOP_READ_PLANAR_FV, FFHIP_SWS_UOP_READ_PLANAR_FV_FMA,
    FFHIP_SWS_UOP_READ_PACKED, FFHIP_SWS_UOP_READ_NIBBLE, FFHIP_SWS_UOP_READ_BIT, FFHIP_SWS_UOP_READ_PALETTE,
    FFHIP_SWS_UOP_WRITE_PLANAR, FFHIP_SWS_UOP_WRITE_PACKED, FFHIP_SWS_UOP_WRITE_NIBBLE, FFHIP_SWS_UOP_WRITE_BIT,
    FFHIP_SWS_UOP_RW_SHUFFLE, FFHIP_SWS_UOP_PERMUTE, FFHIP_SWS_UOP_COPY,
    FFHIP_SWS_UOP_SWAP_BYTES, FFHIP_SWS_UOP_EXPAND_BIT, FFHIP_SWS_UOP_EXPAND_PAIR, FFHIP_SWS_UOP_EXPAND_QUAD,
    FFHIP_SWS_UOP_TO_U8, FFHIP_SWS_UOP_TO_U16, FFHIP_SWS_UOP_TO_U32, FFHIP_SWS_UOP_TO_F32,
    FFHIP_SWS_UOP_SCALE, FFHIP_SWS_UOP_ADD, FFHIP_SWS_UOP_MIN, FFHIP_SWS_UOP_MAX,
    FFHIP_SWS_UOP_UNPACK, FFHIP_SWS_UOP_PACK, FFHIP_SWS_UOP_LSHIFT, FFHIP_SWS_UOP_RSHIFT, FFHIP_SWS_UOP_CLEAR,
    FFHIP_SWS_UOP_LINEAR, FFHIP_SWS_UOP_LINEAR_FMA, FFHIP_SWS_UOP_DITHER, FFHIP_SWS_UOP_LUT_3D,
    FFHIP_SWS_UOP_TYPE_NB
};
#define FFHIP_SWS_FILTER_SCALE (1 << 14)          /* SWS_FILTER_SCALE, filters.h:39 */

typedef union FFHipSwsPixel { char data[4]; uint8_t u8; uint16_t u16; uint32_t u32; float f32; } FFHipSwsPixel;

typedef struct FFHipSwsFilterWeights {
    int     filter_size;              /* taps per output sample */
    int    *weights;                  /* [dst_size][filter_size], scaled by FFHIP_SWS_FILTER_SCALE */
    size_t  num_weights;
    int    *offsets;                  /* first source sample of every output sample */
    int     src_size, dst_size;
    double  virtual_size, offset;
    char    name[16];
    int     sum_positive, sum_negative;
} FFHipSwsFilterWeights;

typedef union FFHipSwsUOpParams {
    struct { uint8_t clear_value, read_size, write_size; } shuffle;
    struct { int32_t type; } filter;                               /* READ_PLANAR_FH / _FV: type the result is stored as */
    struct { uint8_t amount; } shift;
    struct { int32_t num_moves; int8_t dst[6], src[6]; } move;     /* PERMUTE / COPY; register -1 is a temporary */
    struct { uint8_t pattern[4]; } pack;
    struct { uint8_t one, zero; } clear;
    struct { uint32_t one, zero, exact; } lin;                     /* bit 5 * row + column */
    struct { uint8_t y_offset[4]; uint8_t size_log2; } dither;
    struct { int32_t dynamic; } lut3d;
} FFHipSwsUOpParams;

typedef struct FFHipSwsUOp {
    int32_t type;                     /* FFHIP_SWS_PIXEL_* */
    int32_t uop;                      /* FFHIP_SWS_UOP_* */
    uint8_t mask;                     /* components, bit c */
    FFHipSwsUOpParams par;
    union {
        FFHipSwsFilterWeights *kernel;
        FFHipSwsPixel *ptr;           /* DITHER: (1 << size_log2) columns, (1 << size_log2) + max(y_offset) rows */
        FFHipSwsPixel scalar;
        FFHipSwsPixel vec4[4];
        FFHipSwsPixel mat4[4][5];
        struct { int8_t mask[16]; uint8_t pixels; } shuffle;
        const void *lut3d;
        void *opaque;
    } data;
} FFHipSwsUOp;

typedef struct FFHipSwsOpExec {
    const uint8_t *in[4];
    uint8_t *out[4];
    ptrdiff_t in_stride[4], out_stride[4];
    ptrdiff_t in_bump[4], out_bump[4];
    int32_t width, height, slice_y, slice_h;
    int32_t block_size_in[4], block_size_out[4];
    uint8_t in_sub_y[4], out_sub_y[4], in_sub_x[4], out_sub_x[4];
    int32_t *in_bump_y;               /* READ_PLANAR_FV: extra source lines after output line y (absolute y) */
    int32_t *in_offset_x;             /* READ_PLANAR_FH: byte offset of the first tap of output sample x (absolute x) */
} FFHipSwsOpExec;

/** SwsOpFunc (ops_dispatch.h:93-99). */
typedef void (*FFHipSwsOpFunc)(const FFHipSwsOpExec *exec, const void *priv, int bx_start, int y_start, int bx_end, int y_end);

typedef struct FFHipSwsUOps FFHipSwsUOps;   /* one compiled micro-op list: what SwsCompiledOp.priv holds */

/** SwsOpBackend.compile_uops (ops_dispatch.h:148): generates, compiles (hiprtc, cached by program text) and loads the kernel of
 *  the list.  FFHIP_ENOTSUP for lists this backend does not take (LUT_3D, RW_SHUFFLE and the _FMA variants — a translation with
 *  flags 0, which is what bit-exactness with backend_c needs, never emits the latter two), FFHIP_EINVAL for malformed ones,
 *  FFHIP_ENOSYS without a device. */
int  ffhip_sws_uops_compile(const FFHipSwsUOp *uops, int num_uops, FFHipSwsUOps **out);
void ffhip_sws_uops_free(FFHipSwsUOps **p);
/** SwsCompiledOp.block_size: pixels per block of bx_start / bx_end — 1, or what makes a block whole bytes (8 for the 1-bit,
 *  2 for the 4-bit reads and writes).  over_read / over_write are 0 for every list: no thread touches a byte outside the blocks. */
int  ffhip_sws_uops_block_size(const FFHipSwsUOps *p);
/** The program text the list compiles to (diagnostics, and the CPU-side test of the generator); returns its length or < 0. */
int  ffhip_sws_uops_source(const FFHipSwsUOp *uops, int num_uops, char *buf, size_t size);
/** Generates and compiles the program without loading it (no device needed): 0, FFHIP_ENOTSUP, FFHIP_EINVAL or FFHIP_EIO. */
int  ffhip_sws_uops_check(const FFHipSwsUOp *uops, int num_uops);
/** Compiled programs are kept per process (by program text) and — once the application names a directory — across processes as
 *  code objects on disk, so that the ~25 ms hiprtc compile of a new op list is paid once per machine.  NULL or "" turns the disk
 *  cache off, which is the default: the library reads no environment variable; the FFmpeg-side backend chooses
 *  $XDG_CACHE_HOME/ffhip or $HOME/.cache/ffhip (integration/swscale_hw_hip.c).  The directory (and its parent) is created on the first
 *  store.  A file carries its whole key (hiprtc version, architecture, program text): a stale, damaged or foreign file is a miss and
 *  is rewritten; files appear by rename, so concurrent processes are safe.  The directory is used only while it is a real directory
 *  (lstat: no symlink) OWNED BY THE EFFECTIVE USER and not writable by group or others — code objects loaded from it run with the
 *  process's access to its device memory — else the cache silently stays off; files are opened O_NOFOLLOW, must be the user's own
 *  regular files, carry a hash of the code object that is verified on load, and are written through mkstemp().  Process-wide; returns 0. */
int  ffhip_sws_uops_set_cache_dir(const char *dir);
/** hiprtc compiles and disk hits of this process so far (either pointer may be NULL). */
void ffhip_sws_uops_cache_stats(long *compiles, long *disk_hits);
/** What the void face below runs when the device fails under it (the same list compiled by the caller's C backend). */
void ffhip_sws_uops_set_fallback(FFHipSwsUOps *p, FFHipSwsOpFunc func, const void *priv);
/** SwsCompiledOp.func for software frames: HOST pointers in `exec`, priv = the FFHipSwsUOps.  Stages exactly the bytes the
 *  C backend would read, runs the kernel, commits exactly the bytes it would write. */
void ffhip_sws_uops_func(const FFHipSwsOpExec *exec, const void *priv, int bx_start, int y_start, int bx_end, int y_end);
/** The device-resident face (an AV_PIX_FMT_HIP frame pool, SwsPass.run of an opaque compiled op): `exec->in / out` are DEVICE
 *  pointers, the two small tables (in_bump_y, in_offset_x) stay host arrays as the dispatcher built them.  `nframes` pictures
 *  that share the geometry run in one launch, plane i of picture f at in[i] + f * in_frame_pitch[i] (NULL pitches: 1 picture).
 *  Asynchronous on `stream`. */
int  ffhip_sws_uops_run_dev(FFHipSwsUOps *p, const FFHipSwsOpExec *exec, int bx_start, int y_start, int bx_end, int y_end,
                            int nframes, const ptrdiff_t *in_frame_pitch, const ptrdiff_t *out_frame_pitch, void *stream);
/** The shape both faces launch a call of `npx` pixels x `ny` lines x `nframes` pictures with, for a list whose threads own `V`
 *  pixels (4; 8 for 1-bit lists): out = grid x, y, z and the lines per thread (a power of two in 1..8; a thread walks the lines
 *  4 x grid y apart).  No device needed.  Returns 0 or FFHIP_EINVAL.  Exposed for the CPU test-suite. */
int  ffhip_sws_uops_launch_shape_host(int V, int npx, int ny, int nframes, int32_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* FFHIP_H */
