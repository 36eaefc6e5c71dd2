/*
 * h264_pred_codec.inc — the per-sample rules of the forms ff_h264_pred_init() installs for the codecs that share H264PredContext
 * (libavcodec/h264pred.c:540-578, bodies :57-432; 8 bits): SVQ3, RV40, VP7 / VP8.  A switch statement, included as text by the batch
 * kernel that reads a block's neighbours from the plane (k_h264_pred_codec, h264_pred.hip) and by the VP8 frame reconstruction that
 * reads them from its tile (vp8_recon_frame.hip); text rather than a function template so that the batch kernel's code is, to the
 * instruction, what it was with the switch written in place.
 *
 * The includer provides: int mode (a FFHIP_H264_PREDV_* code, which also says the block size), x, y; int v = 0 (the result);
 * callables t(i) = the row above (i >= 4 of a 4x4 block: topright[i - 4]), lraw(i) = the left column, l(i) = the same with the
 * _NODOWN forms' repeat of l3 (i >= 4: the rows below the block, RV40's "down-left" edge), clip(v) to 0..255; and the macro
 * HP_CODEC_LT = the corner.  Only what the mode's rule names is evaluated.
 */
    switch (mode) {
    case FFHIP_H264_PREDV_127_DC: case FFHIP_H264_PREDV8_127_DC: case FFHIP_H264_PREDV16_127_DC: v = 127; break;
    case FFHIP_H264_PREDV_129_DC: case FFHIP_H264_PREDV8_129_DC: case FFHIP_H264_PREDV16_129_DC: v = 129; break;
    case FFHIP_H264_PREDV_VERT_VP8: /* pred4x4_vertical_vp8_c: the row above, smoothed */
        v = ((x ? t(x - 1) : HP_CODEC_LT) + 2 * t(x) + t(x + 1) + 2) >> 2;
        break;
    case FFHIP_H264_PREDV_HOR_VP8:  /* pred4x4_horizontal_vp8_c */
        v = ((y ? lraw(y - 1) : HP_CODEC_LT) + 2 * lraw(y) + lraw(y < 3 ? y + 1 : 3) + 2) >> 2;
        break;
    case FFHIP_H264_PREDV_DL_SVQ3: { /* pred4x4_down_left_svq3_c */
        const int i = min(x + y + 1, 3);
        v = (lraw(i) + t(i)) >> 1;
        break;
    }
    case FFHIP_H264_PREDV_DL_RV40: case FFHIP_H264_PREDV_DL_RV40_NODOWN: { /* pred4x4_down_left_rv40{,_nodown}_c */
        const int d = x + y;
        v = d < 6 ? (t(d) + t(d + 2) + 2 * t(d + 1) + 2 + l(d) + l(d + 2) + 2 * l(d + 1) + 2) >> 3 : (t(6) + t(7) + 1 + l(6) + l(7) + 1) >> 2;
        break;
    }
    case FFHIP_H264_PREDV_VL_RV40: case FFHIP_H264_PREDV_VL_RV40_NODOWN: /* pred4x4_vertical_left_rv40 (l4 = l3 without the down-left edge) */
        if (!(y & 1)) {
            const int q = x + (y >> 1);
            v = x == 0 && y == 0 ? (2 * t(0) + 2 * t(1) + l(1) + 2 * l(2) + l(3) + 4) >> 3 : (t(q) + t(q + 1) + 1) >> 1;
        } else {
            const int q = x + (y >> 1);
            v = x == 0 && y == 1 ? (t(0) + 2 * t(1) + t(2) + l(2) + 2 * l(3) + l(4) + 4) >> 3 : (t(q) + 2 * t(q + 1) + t(q + 2) + 2) >> 2;
        }
        break;
    case FFHIP_H264_PREDV_VL_VP8: { /* pred4x4_vertical_left_vp8_c: H.264's but for the last column's lower half */
        const int q = x + (y >> 1);
        if (x == 3 && y >= 2)
            v = (t(y + 2) + 2 * t(y + 3) + t(y + 4) + 2) >> 2;
        else
            v = (y & 1) ? (t(q) + 2 * t(q + 1) + t(q + 2) + 2) >> 2 : (t(q) + t(q + 1) + 1) >> 1;
        break;
    }
    case FFHIP_H264_PREDV_HU_RV40: case FFHIP_H264_PREDV_HU_RV40_NODOWN: { /* pred4x4_horizontal_up_rv40{,_nodown}_c */
        const int z = x + 2 * y;
        switch (z) {
        case 0: v = (t(1) + 2 * t(2) + t(3) + 2 * l(0) + 2 * l(1) + 4) >> 3; break;
        case 1: v = (t(2) + 2 * t(3) + t(4) + l(0) + 2 * l(1) + l(2) + 4) >> 3; break;
        case 2: v = (t(3) + 2 * t(4) + t(5) + 2 * l(1) + 2 * l(2) + 4) >> 3; break;
        case 3: v = (t(4) + 2 * t(5) + t(6) + l(1) + 2 * l(2) + l(3) + 4) >> 3; break;
        case 4: v = (t(5) + 2 * t(6) + t(7) + 2 * l(2) + 2 * l(3) + 4) >> 3; break;
        case 5: v = (t(6) + 3 * t(7) + l(2) + 3 * l(3) + 4) >> 3; break;
        case 6: v = (t(6) + t(7) + l(3) + l(4) + 2) >> 2; break;
        case 7: v = (l(3) + 2 * l(4) + l(5) + 2) >> 2; break;
        case 8: v = (l(4) + l(5) + 1) >> 1; break;
        default: v = (l(4) + 2 * l(5) + l(6) + 2) >> 2; break;
        }
        break;
    }
    case FFHIP_H264_PREDV_TM_VP8: case FFHIP_H264_PREDV8_TM_VP8: case FFHIP_H264_PREDV16_TM_VP8: /* pred{4x4,8x8,16x16}_tm_vp8_c */
        v = clip(lraw(y) + t(x) - HP_CODEC_LT);
        break;
    case FFHIP_H264_PREDV8_DC_RV40: case FFHIP_H264_PREDV8_LEFT_DC_RV40: case FFHIP_H264_PREDV8_TOP_DC_RV40: { /* pred8x8_*dc_rv40_c */
        int sl = 0, st = 0;
        for (int i = 0; i < 8; i++) {
            if (mode != FFHIP_H264_PREDV8_TOP_DC_RV40) sl += lraw(i);
            if (mode != FFHIP_H264_PREDV8_LEFT_DC_RV40) st += t(i);
        }
        v = mode == FFHIP_H264_PREDV8_DC_RV40 ? (sl + st + 8) >> 4 : (sl + st + 4) >> 3;
        break;
    }
    default: { /* FFHIP_H264_PREDV16_PLANE_SVQ3 / _RV40: pred16x16_plane_compat_8_c (h264pred_template.c:410-456) */
        int H = 0, V = 0;
        for (int q = 1; q <= 8; q++) {
            H += q * (t(7 + q) - (q == 8 ? HP_CODEC_LT : t(7 - q)));
            V += q * (lraw(7 + q) - (q == 8 ? HP_CODEC_LT : lraw(7 - q)));
        }
        if (mode == FFHIP_H264_PREDV16_PLANE_SVQ3) {
            const int h2 = (5 * (H / 4)) / 16, v2 = (5 * (V / 4)) / 16;
            H = v2; V = h2; /* "required for 100% accuracy": the two are swapped */
        } else {
            H = (H + (H >> 2)) >> 4;
            V = (V + (V >> 2)) >> 4;
        }
        const int a = 16 * (lraw(15) + t(15) + 1) - 7 * (V + H);
        v = clip((a + y * V + x * H) >> 5);
        break;
    }
    }
