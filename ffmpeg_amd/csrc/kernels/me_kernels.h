/* me_kernels.h — launchers of the me_cmp / exhaustive-search kernels (internal to libffhip). */
#ifndef FFHIP_ME_KERNELS_H
#define FFHIP_ME_KERNELS_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "ffhip.h"

int ffhip_launch_me_cmp(int kind, int width, int h, const uint8_t *blk1, const int32_t *off1, const uint8_t *blk2,
                        const int32_t *off2, ptrdiff_t stride, int32_t *out, int n, hipStream_t stream);
int ffhip_launch_me_esa(const uint8_t *cur, const uint8_t *ref, int width, int height, ptrdiff_t stride, size_t frame_pitch,
                        int nframes, int mb_size, int R, int cost_kind, int16_t *mv_out, uint32_t *cost_out,
                        hipStream_t stream);
/* SATD search on the matrix cores (me_satd.hip): 1 = launched, 0 = not its case */
int ffhip_launch_me_esa_satd_mx(const uint8_t *cur, const uint8_t *ref, int width, int height, ptrdiff_t stride, size_t frame_pitch, int nframes,
                                int mb_size, int R, int16_t *mv_out, uint32_t *cost_out, hipStream_t stream);
/* the per-block fast searches (me_search.hip): method FFHIP_ME_METHOD_TSS .. _HEXBS, nblocks = b_w * b_h * nframes > 0 */
int ffhip_launch_me_search(int method, const uint8_t *cur, const uint8_t *ref, int width, int height, ptrdiff_t stride, size_t frame_pitch,
                           int nframes, int mb_size, int R, int cost_kind, int16_t *mv_out, uint32_t *cost_out, hipStream_t stream);
/* cost_kind of the bilateral cost (me_search_bilat_rules.h) for the two predictive launchers below, beside FFHIP_ME_SAD and
 * FFHIP_ME_SATD: picture A is `cur`, picture B `ref`.  Internal: the public faces of the bilateral search have no cost_kind. */
#define MES_COST_BILAT 2
/* the predictive searches (me_search_pred.hip): method FFHIP_ME_METHOD_EPZS or _UMH, prev1 / prev2 NULL or fields laid out as mv_out,
 * mv_out 4-byte aligned; calls of more block rows than a progress-pool slot counts are split by pairs */
int ffhip_launch_me_search_pred(int method, const uint8_t *cur, const uint8_t *ref, int width, int height, ptrdiff_t stride, size_t frame_pitch,
                                int nframes, int mb_size, int R, int cost_kind, const int16_t *prev1, const int16_t *prev2, int16_t *mv_out,
                                uint32_t *cost_out, hipStream_t stream);
/* the same of whole sequences (me_search_seq.hip): nseq sequences of nframes pictures, pair k chained to the fields of pairs k - 1 and
 * k - 2 inside the launch; outputs pair-major, init1 / init2 NULL or nseq fields each; calls of more units than a progress-pool slot
 * counts are split at pair boundaries, and by sequences where one step alone does not fit */
int ffhip_launch_me_search_seq(int method, const uint8_t *frames, int width, int height, ptrdiff_t stride, size_t frame_pitch, int nframes,
                               size_t seq_pitch, int nseq, int direction, int mb_size, int R, int cost_kind, const int16_t *init1,
                               const int16_t *init2, int16_t *mv_out, uint32_t *cost_out, hipStream_t stream);
/* vf_minterpolate's compensation (me_interp.hip): arguments checked, window and jobs on the host; calls of more jobs than a launch's
 * table holds are split in stream order */
int ffhip_launch_me_interp(const FFHipMePlanes *src, const FFHipMePlanes *dst, int nplanes, int log2_chroma_w, int log2_chroma_h, int width,
                           int height, int nseq, int mb_size, int mv_range, const uint8_t *window, const int16_t *mv_fwd, const int16_t *mv_bwd,
                           const FFHipMeInterpJob *jobs, int njobs, hipStream_t stream);
/* the same with the scene flags of ffhip_me_interp_sequence_scd_dev(): scene NULL, or pair-major flags on the device and their action */
int ffhip_launch_me_interp_scd(const FFHipMePlanes *src, const FFHipMePlanes *dst, int nplanes, int log2_chroma_w, int log2_chroma_h, int width,
                               int height, int nseq, int mb_size, int mv_range, const uint8_t *window, const int16_t *mv_fwd, const int16_t *mv_bwd,
                               const FFHipMeInterpJob *jobs, int njobs, const uint8_t *scene, int scene_action, hipStream_t stream);
/* the bilateral compensation (me_interp.hip, k_me_interp_bilat): one field `mv` of half-vectors, otherwise as the launcher above */
int ffhip_launch_me_interp_bilat(const FFHipMePlanes *src, const FFHipMePlanes *dst, int nplanes, int log2_chroma_w, int log2_chroma_h, int width,
                                 int height, int nseq, int mb_size, int mv_range, const uint8_t *window, const int16_t *mv,
                                 const FFHipMeInterpJob *jobs, int njobs, const uint8_t *scene, int scene_action, hipStream_t stream);
/* vf_minterpolate's scene-change detection (me_scene.hip): arguments checked, every pointer on the device; calls of more pairs than a
 * launch's sums hold are split in stream order */
int ffhip_launch_me_scene(const uint8_t *frames, int depth, int width, int height, ptrdiff_t stride, size_t frame_pitch, int nframes, size_t seq_pitch,
                          int nseq, double threshold, const double *mafd_in, double *mafd_out, uint64_t *sad_out, float *score_out,
                          uint8_t *flags_out, hipStream_t stream);
#endif
