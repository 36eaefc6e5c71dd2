/*
 * row_handoff.h — the hand-off between the waves of the row-ordered kernels (cdna_hip_programming Guideline 16), once.
 *
 * A wave walks one macroblock / CTB / superblock row left to right and starts column x only after the row above has published a
 * column at or past x + lag (the lag is the kernel's: what its column reads of the row above).  The rows talk through one counter
 * per row in a progress-pool slot (progress_pool.h):
 *
 *   producer   every sample the next row reads is written with an agent-scope relaxed store (ffhip_row_st: write-through to L2, the
 *              8 XCDs' L2s are not coherent with each other).  ffhip_row_publish() then orders them with a release fence, waits until
 *              all of them are acknowledged (s_waitcnt 0) and only then moves the counter, lane 0, with an agent-scope store.
 *   consumer   ffhip_row_wait() polls the counter with agent-scope relaxed loads and, once it has seen the value, issues an acquire
 *              fence, so the neighbour loads are issued after the counter was seen; those are agent-scope loads (ffhip_row_ld: they
 *              bypass the CU's L1).  What else a wave loads nobody writes in the launch.
 *   progress   the row a wave waits on must belong to a wave that runs: either the kernel maps rows to workgroups by blockIdx and
 *              relies on dispatch in order of the linear workgroup id, or it claims its units with ffhip_row_ticket() from a counter in
 *              the slot, numbered so that the unit awaited has a smaller ticket (then the grid is min(units, resident capacity)).
 *   timeout    every spin is bounded.  A wave that runs out sets the slot's fail word (pinned host memory, system scope) from lane 0
 *              and returns false: the kernel leaves, and ffhip_progress_check() reports the lost hand-off.  Never in a correct run.
 *
 * What the sites do differently is an argument with a named default, as each site was written; nothing here was re-measured:
 * the sleep between polls, the spin limit, the scope of the two fences, and a wave_barrier between the drain and the counter store.
 */
#ifndef FFHIP_ROW_HANDOFF_H
#define FFHIP_ROW_HANDOFF_H

#include <hip/hip_runtime.h>
#include <stdint.h>

enum FFHipRowFence { FFHIP_ROW_FENCE_NONE, FFHIP_ROW_FENCE_WORKGROUP, FFHIP_ROW_FENCE_AGENT };
constexpr int FFHIP_ROW_SLEEP = 2;           /* s_sleep units (64 clocks each) between two polls of a global counter */
constexpr int FFHIP_ROW_SPINS = 1 << 24;     /* polls of a global counter before the wave gives up */
constexpr int FFHIP_ROW_LDS_SLEEP = 1;       /* between two polls of an LDS counter */
constexpr int FFHIP_ROW_LDS_SPINS = 1 << 22; /* polls of an LDS counter in ffhip_row_wait_lds(): as written in 8d3563b and 70960ba */

/* four samples: a dword at 8 bits, two above */
template <typename PIX> struct FFHipQuad { typedef uint32_t T; };
template <> struct FFHipQuad<uint16_t> { typedef uint64_t T; };

/* samples another row reads or wrote in this launch */
template <typename Q>
__device__ __forceinline__ Q ffhip_row_ld(const uint8_t *p)
{
    return __hip_atomic_load(reinterpret_cast<const Q *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename Q>
__device__ __forceinline__ void ffhip_row_st(uint8_t *p, Q v)
{
    __hip_atomic_store(reinterpret_cast<Q *>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <FFHipRowFence FENCE>
__device__ __forceinline__ void ffhip_row_fence_acquire()
{
    if (FENCE == FFHIP_ROW_FENCE_AGENT)
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    else if (FENCE == FFHIP_ROW_FENCE_WORKGROUP)
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

/* the wave gave up on a hand-off */
__device__ __forceinline__ void ffhip_row_lost(int *fail, bool lane0)
{
    if (lane0)
        __hip_atomic_store(fail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

/* Waits until `counter` (the row above) has reached `want`.  `known` is the last value this wave saw of it and is kept across
 * columns: the counter is not loaded while it already suffices.  false after a timeout.  SCOPE: __HIP_MEMORY_SCOPE_WORKGROUP for a
 * counter in LDS (CTR: int in the generic or the LDS address space). */
template <int SLEEP = FFHIP_ROW_SLEEP, int SPINS = FFHIP_ROW_SPINS, FFHipRowFence FENCE = FFHIP_ROW_FENCE_WORKGROUP,
          int SCOPE = __HIP_MEMORY_SCOPE_AGENT, typename CTR>
__device__ __forceinline__ bool ffhip_row_wait(const CTR *counter, int want, int &known, int *fail, int lane)
{
    int spins = 0;
    while (known < want) {
        known = __hip_atomic_load(counter, __ATOMIC_RELAXED, SCOPE);
        if (known >= want)
            break;
        __builtin_amdgcn_s_sleep(SLEEP);
        if (++spins > SPINS) {
            ffhip_row_lost(fail, lane == 0);
            return false;
        }
    }
    ffhip_row_fence_acquire<FENCE>(); /* the neighbour loads are issued after the counter was seen */
    return true;
}

/* The same for a wave that keeps no `known`: the counter is loaded at least once. */
template <int SLEEP = FFHIP_ROW_SLEEP, int SPINS = FFHIP_ROW_SPINS, FFHipRowFence FENCE = FFHIP_ROW_FENCE_WORKGROUP>
__device__ __forceinline__ bool ffhip_row_wait_fresh(const int *counter, int want, int *fail, int lane)
{
    int spins = 0;
    while (__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want) {
        __builtin_amdgcn_s_sleep(SLEEP);
        if (++spins > SPINS) {
            ffhip_row_lost(fail, lane == 0);
            return false;
        }
    }
    ffhip_row_fence_acquire<FENCE>();
    return true;
}

/* The always-loading wait on an LDS counter of another wave of the workgroup.  A wave's LDS operations execute in order, so no fence
 * follows: the compiler alone is kept from moving the reads up. */
template <int SLEEP = FFHIP_ROW_LDS_SLEEP, int SPINS = FFHIP_ROW_LDS_SPINS, typename CTR>
__device__ __forceinline__ bool ffhip_row_wait_lds(const CTR *ctr, int want, int *fail)
{
    int spins = 0;
    while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < want) {
        __builtin_amdgcn_s_sleep(SLEEP);
        if (++spins > SPINS) {
            ffhip_row_lost(fail, (threadIdx.x & 63) == 0);
            return false;
        }
    }
    asm volatile("" ::: "memory");
    return true;
}

/* Every store of the wave is out and acknowledged.  BARRIER: a wave_barrier behind the drain (the H.264 4:2:2 and MBAFF kernels). */
template <FFHipRowFence FENCE = FFHIP_ROW_FENCE_WORKGROUP, bool BARRIER = false>
__device__ __forceinline__ void ffhip_row_drain()
{
    if (FENCE == FFHIP_ROW_FENCE_AGENT)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    else
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_waitcnt(0);
    if (BARRIER)
        __builtin_amdgcn_wave_barrier();
}

/* ... and then the row's counter moves */
template <FFHipRowFence FENCE = FFHIP_ROW_FENCE_WORKGROUP, bool BARRIER = false>
__device__ __forceinline__ void ffhip_row_publish(int *counter, int value, int lane)
{
    ffhip_row_drain<FENCE, BARRIER>();
    if (lane == 0)
        __hip_atomic_store(counter, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* the wave's next work unit: lane 0 claims it, every lane gets it */
__device__ __forceinline__ int ffhip_row_ticket(int *ticket, int lane)
{
    int t = 0;
    if (lane == 0)
        t = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return __shfl(t, 0);
}

#endif
