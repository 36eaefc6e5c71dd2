"""A model of ffhip_me_interp_sequence_dev() written from the rule text of include/ffhip.h, in the reference's form and not in that of
kernels/me_interp_rules.h: the blocks SCATTER themselves, in (dir, by, bx) order, into explicit per-pixel lists of up to NB_PIXEL_MVS
entries (bidirectional_obmc()); then every plane is made by a walk over the LUMA positions in which, for chroma, the last writer wins
(set_frame_data()).  The rules header gathers and stores no list, so the two agree only if both follow the text.

Pictures are lists of 2-D uint8 arrays (one per plane, exactly the plane's size); fields are int arrays [b_h, b_w, 2] of absolute
positions.  The eight counters are those of ffhip_me_interp_host_counts()."""
import numpy as np

NB_PIXEL_MVS = 32
MCI, BLEND = 0, 1
COUNTS = ("taken", "zero_weight", "capped", "malformed", "fallback", "clipped", "samples", "blend")


def tdiv(n):
    """n / 1024 in C"""
    return -((-n) // 1024) if n < 0 else n // 1024


def cdiv(n, d):
    """n / d in C, d > 0"""
    return -((-n) // d) if n < 0 else n // d


def clip(v, lo, hi):
    """av_clip"""
    if v < lo:
        return lo
    if v > hi:
        return hi
    return v


def new_counts():
    return dict.fromkeys(COUNTS, 0)


def scatter(W, H, mb, mv_range, alpha, window, fwd, bwd, counts):
    """bidirectional_obmc(): lists[y][x] = [(ref, weight, dx, dy), ...], two entries per contribution"""
    log2mb = {16: 4, 8: 3}[mb]
    b_w, b_h = W >> log2mb, H >> log2mb
    lists = [[[] for _ in range(W)] for _ in range(H)]
    for d in (0, 1):
        field = bwd if d else fwd
        for by in range(b_h):
            for bx in range(b_w):
                vx = int(field[by][bx][0]) - (bx << log2mb)
                vy = int(field[by][bx][1]) - (by << log2mb)
                if abs(vx) > mv_range or abs(vy) > mv_range:
                    counts["malformed"] += 1
                    continue
                a = alpha if d else 1024 - alpha
                sx = (bx << log2mb) - mb // 2 + tdiv(vx * a)
                sy = (by << log2mb) - mb // 2 + tdiv(vy * a)
                x0, x1 = clip(sx, 0, W - 1), clip(sx + 2 * mb, 0, W - 1)
                y0, y1 = clip(sy, 0, H - 1), clip(sy + 2 * mb, 0, H - 1)
                mx, my = (-vx, -vy) if d else (vx, vy)
                ax, ay = tdiv(mx * alpha), tdiv(my * alpha)
                ex, ey = tdiv(-mx * (1024 - alpha)), tdiv(-my * (1024 - alpha))
                for y in range(y0, y1):
                    for x in range(x0, x1):
                        w = int(window[(x - sx) + (y - sy) * 2 * mb])
                        if w == 0:
                            counts["zero_weight"] += 1
                            continue
                        pm = lists[y][x]
                        if len(pm) + 1 >= NB_PIXEL_MVS:
                            counts["capped"] += 1
                            continue
                        counts["taken"] += 1
                        for ref, weight, dx, dy in ((0, w * (1024 - alpha), ax, ay), (1, w * alpha, ex, ey)):
                            cx, cy = clip(dx, -x, W - 1 - x), clip(dy, -y, H - 1 - y)
                            counts["clipped"] += (cx, cy) != (dx, dy)
                            pm.append((ref, weight, cx, cy))
    return lists


def frame_data(A, B, W, H, sw, sh, alpha, lists, counts):
    """set_frame_data(): every plane from a walk over the luma positions"""
    out = [np.zeros_like(p) for p in A]
    refs = (A, B)
    for y in range(H):
        for x in range(W):
            if not lists[y][x]:
                counts["fallback"] += 1
                lists[y][x] = [(0, 1024 - alpha, 0, 0), (1, alpha, 0, 0)]
    for i in range(len(A)):
        hs, vs = (sw, sh) if i else (0, 0)
        for y in range(H):
            for x in range(W):
                S = Wt = 0
                for ref, weight, dx, dy in lists[y][x]:
                    S += weight * int(refs[ref][i][(y >> vs) + cdiv(dy, 1 << vs)][(x >> hs) + cdiv(dx, 1 << hs)])
                    Wt += weight
                out[i][y >> vs][x >> hs] = (S + (Wt >> 1)) // Wt         # chroma: the last writer wins
        counts["samples"] += out[i].size
    return out


def blend(A, B, alpha, counts):
    out = [((alpha * B[i].astype(np.int64) + (1024 - alpha) * A[i].astype(np.int64) + 512) >> 10).astype(np.uint8) for i in range(len(A))]
    n = sum(o.size for o in out)
    counts["samples"] += n
    counts["blend"] += n
    return out


def interp_job(A, B, W, H, sw, sh, mb, mv_range, window, fwd, bwd, alpha, mode, counts):
    if mode == BLEND:
        return blend(A, B, alpha, counts)
    lists = scatter(W, H, mb, mv_range, alpha, window, fwd, bwd, counts)
    return frame_data(A, B, W, H, sw, sh, alpha, lists, counts)


def interp_sequence(pics, W, H, sw, sh, mb, mv_range, window, mv_fwd, mv_bwd, jobs):
    """pics[s][p] = a picture's planes; mv_fwd / mv_bwd[k][s] = the field of pair k of sequence s; jobs = (seq, pair, alpha, mode).
    Returns ([job j's planes], counts)."""
    counts = new_counts()
    out = []
    for seq, pair, alpha, mode in jobs:
        fwd = bwd = None
        if mode == MCI:
            fwd, bwd = mv_fwd[pair][seq], mv_bwd[pair][seq]
        out.append(interp_job(pics[seq][pair], pics[seq][pair + 1], W, H, sw, sh, mb, mv_range, window, fwd, bwd, alpha, mode, counts))
    return out, counts
