/* progress_pool.h — the progress counters of the row-ordered ("wavefront") launches in flight (the kernels of row_handoff.h) and the
 * ways a launcher takes a slot: ffhip_progress_launch() and, with a table staged in it, ffhip_progress_launch_table().  Internal to
 * libffhip (progress_pool.hip). */
#ifndef FFHIP_PROGRESS_POOL_H
#define FFHIP_PROGRESS_POOL_H

#include <hip/hip_runtime.h>

#include "ffhip_internal.h"

#define FFHIP_PROGRESS_SLOT_INTS 8192 /* 2048 until round 4: 64 4K luma planes (34 bands each) then split into launches of 60 + 4 pictures, and the 4 paid a whole latency chain (2.26 ms against 0.96 ms for 32 planes) */

struct FFHipProgressSlot {
    int *prog; /* `nints` zeroed (in stream order) progress words on the current device */
    int *fail; /* the slot's FAIL word, pinned host memory mapped into the device: a kernel sets it on a spin timeout */
    int  index, device;
};

/* A free slot of the current device's pool, its first `nints` (<= FFHIP_PROGRESS_SLOT_INTS) counters zeroed on `stream`.  The pool
 * lock is NOT held when this returns: the slot is simply owned until ffhip_progress_release(). */
int ffhip_progress_acquire(int nints, hipStream_t stream, FFHipProgressSlot *s); /* callers use ffhip_progress_launch() */
/* launched: an event behind the launch on `stream` marks when the slot may be reused; !launched (an error path): the slot is free
 * again at once. */
int ffhip_progress_release(const FFHipProgressSlot *s, hipStream_t stream, bool launched);
/* FFHIP_EIO (once) if a finished launch that was issued on `stream` lost a hand-off — keyed by stream, so the owner of picture A
 * hears about picture A and nobody else does.  Checks the current device's pool. */
int ffhip_progress_check(hipStream_t stream);
/* on: launches the calling thread queues from now on file a lost hand-off under `stream` whatever stream they run on (the picture
 * layer's chroma wavefront runs on a private second stream; its caller only ever asks about its own); off: back to the launch's. */
void ffhip_progress_report_to(hipStream_t stream, bool on);

/* One launch on a slot of `nints` zeroed counters.  launch(slot) queues the work on `stream` and returns its hipError_t: the kernel
 * launch followed by hipGetLastError().  A failed launch frees the slot at once, sets "<what> failed: <HIP's text> (<the caller's
 * file:line>)" and wins over a failed release: FFHIP_EIO.  Otherwise the acquire's or the release's error, or 0. */
template <class Launch>
static inline int ffhip_progress_launch(int nints, hipStream_t stream, const char *what, Launch &&launch, const char *file = __builtin_FILE(),
                                        int line = __builtin_LINE())
{
    FFHipProgressSlot ps;
    const int r = ffhip_progress_acquire(nints, stream, &ps);
    if (r < 0)
        return r;
    const hipError_t e = launch(ps);
    const int r2 = ffhip_progress_release(&ps, stream, e == hipSuccess);
    if (e != hipSuccess) {
        ffhip_set_error("%s failed: %s (%s:%d)", what, hipGetErrorString(e), file, line);
        return FFHIP_EIO;
    }
    return r2 < 0 ? r2 : 0;
}

/* One launch behind a table: `count` T of `host` go to the device in stream order and launch(dev) queues the kernel(s) that read
 * them.  The table travels in a slot without counters (nints 0): a slot is device memory that is not handed out again before the
 * launch behind it has finished, and a copy from pageable memory is staged by the time hipMemcpyAsync returns, so `host` may be the
 * caller's array or a local.  FFHIP_EINVAL for a table larger than a slot (the launchers' static_asserts keep theirs below it);
 * otherwise as ffhip_progress_launch(), a failed copy included. */
template <class T, class Launch>
static inline int ffhip_progress_launch_table(hipStream_t stream, const char *what, const T *host, size_t count, Launch &&launch,
                                              const char *file = __builtin_FILE(), int line = __builtin_LINE())
{
    const size_t bytes = count * sizeof(T);
    if (bytes > FFHIP_PROGRESS_SLOT_INTS * sizeof(int)) {
        ffhip_set_error("%s: a table of %zu bytes exceeds a progress-pool slot", what, bytes);
        return FFHIP_EINVAL;
    }
    return ffhip_progress_launch(0, stream, what, [&](const FFHipProgressSlot &ps) {
        T *dev = reinterpret_cast<T *>(ps.prog);
        const hipError_t e = hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, stream);
        if (e != hipSuccess)
            return e;
        launch(dev);
        return hipGetLastError();
    }, file, line);
}

#endif
