/*
 * me_scene.hip — the scene-change detection of vf_minterpolate (scd=fdiff) for whole sequences, nothing read back: k_me_scene_sad<PIX>,
 * the whole-picture SAD of every pair of a launch as a streaming reduction, and k_me_scene_flags, one lane per sequence that walks its
 * pairs in order with the carried double.  The rule is kernels/me_scene_rules.h; include/ffhip.h states it.
 *
 * k_me_scene_sad.  blockIdx.y is a pair of the launch, blockIdx.x a band of MSC_ROWS rows of it; a workgroup is 4 waves and a wave
 * takes every fourth row of the band, one row at a time.  A row of picture A and the same row of picture B lie frame_pitch bytes
 * apart, so their addresses agree modulo 16 for every row or for none:
 *   - frame_pitch a multiple of 16: a head of single samples up to A's next 16-byte boundary, then 16-byte loads of both rows, lane l
 *     of the wave taking vectors l, l + 64, .., then a tail of single samples.  Bytes are summed a dword at a time with v_sad_u8,
 *     16-bit samples two at a time with v_sad_u16.  Nothing past a row's `width` samples is loaded, so a row's padding is never read
 *     and the last row of the last picture may end the allocation;
 *   - otherwise every sample is loaded alone (the two rows' dwords hold different samples).
 * Widths: a lane sums one row in 32 bits — at most 64 vectors (32768 samples of 2 bytes / 16 / 64 lanes) of 8 x 65535 plus a head and a
 * tail sample of 65535 each, below 2^26 — and adds that to a 64-bit lane total, which is what the wave (__shfl_xor of both halves),
 * the workgroup (LDS) and the launch (one 64-bit vector atomic add per workgroup into the pair's sum, which the launcher zeroed in
 * stream order) carry.  Integer sums: the order of the adds does not change the result.
 *
 * The sums of a launch live in a progress-pool slot (device memory that is not handed out again before the launch behind it has
 * finished): MSC_PAIRS_PER_LAUNCH 64-bit words.  A call with more pairs is split in stream order: into groups of at most that many
 * sequences, and a group into runs of whole steps; the carried doubles of a group whose pairs take several launches wait in a second
 * slot, held for the duration of the group.  No grid dimension bounds the pair count.
 */
#include <algorithm>

#include "common.h"
#include "me_kernels.h"
#include "me_scene_rules.h"
#include "progress_pool.h"

#define MSC_ROWS 16                 /* rows of a band: 4 per wave */
#define MSC_PAIRS_PER_LAUNCH (FFHIP_PROGRESS_SLOT_INTS / 2)
static_assert(MSC_PAIRS_PER_LAUNCH <= 65535, "blockIdx.y is a pair of the launch");
static_assert((32768 * 2 / 16 / 64) * 8ull * 65535 + 2 * 65535 < (1ull << 32), "a lane's sum over one row fits 32 bits");

struct MscParams {
    const uint8_t *frames;
    ptrdiff_t stride;
    size_t frame_pitch, seq_pitch;
    int width, height, depth;
    int nseq;                       /* of the call */
    int s0, ng, k0;                 /* the launch: sequences [s0, s0 + ng), steps from k0; local pair j is step k0 + j / ng, sequence s0 + j % ng */
    int wide;                       /* frame_pitch is a multiple of 16 */
};

template <class PIX> __device__ __forceinline__ uint32_t msc_sad_dword(uint32_t a, uint32_t b, uint32_t acc);
template <> __device__ __forceinline__ uint32_t msc_sad_dword<uint8_t>(uint32_t a, uint32_t b, uint32_t acc) { return __builtin_amdgcn_sad_u8(a, b, acc); }
template <> __device__ __forceinline__ uint32_t msc_sad_dword<uint16_t>(uint32_t a, uint32_t b, uint32_t acc) { return __builtin_amdgcn_sad_u16(a, b, acc); }

template <class PIX>
__global__ __launch_bounds__(256) void k_me_scene_sad(const MscParams P, unsigned long long *__restrict__ sums)
{
    __shared__ unsigned long long part[4];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = blockIdx.y, k = P.k0 + j / P.ng, s = P.s0 + j % P.ng;
    const uint8_t *const A = P.frames + (size_t)s * P.seq_pitch + (size_t)k * P.frame_pitch;
    const int y0 = blockIdx.x * MSC_ROWS, y1 = min(y0 + MSC_ROWS, P.height);
    constexpr int PER = 16 / (int)sizeof(PIX);          /* samples of a vector */

    unsigned long long total = 0;
    for (int y = y0 + wave; y < y1; y += 4) {
        const PIX *const a = reinterpret_cast<const PIX *>(A + (ptrdiff_t)y * P.stride);
        const PIX *const b = reinterpret_cast<const PIX *>(A + (ptrdiff_t)y * P.stride + P.frame_pitch);
        uint32_t acc = 0;
        int head = P.width, nvec = 0;                   /* samples [0, head) alone, then nvec vectors, then the rest alone */
        if (P.wide) {
            head = min((int)((16 - (reinterpret_cast<uintptr_t>(a) & 15)) & 15) / (int)sizeof(PIX), P.width);
            nvec = (P.width - head) / PER;
        }
        const uint4 *const va = reinterpret_cast<const uint4 *>(a + head), *const vb = reinterpret_cast<const uint4 *>(b + head);
        for (int v = lane; v < nvec; v += 64) {
            const uint4 p = va[v], q = vb[v];
            acc = msc_sad_dword<PIX>(p.x, q.x, acc);
            acc = msc_sad_dword<PIX>(p.y, q.y, acc);
            acc = msc_sad_dword<PIX>(p.z, q.z, acc);
            acc = msc_sad_dword<PIX>(p.w, q.w, acc);
        }
        const int tail = head + nvec * PER;
        for (int i = lane; i < head; i += 64)           /* at most 15 samples when wide */
            acc += (uint32_t)abs((int)a[i] - (int)b[i]);
        for (int i = tail + lane; i < P.width; i += 64)
            acc += (uint32_t)abs((int)a[i] - (int)b[i]);
        total += acc;
    }
    /* the wave, the workgroup, the pair */
    uint32_t lo = (uint32_t)total, hi = (uint32_t)(total >> 32);
#pragma unroll
    for (int m = 32; m; m >>= 1) {
        const uint32_t olo = (uint32_t)__shfl_xor((int)lo, m), ohi = (uint32_t)__shfl_xor((int)hi, m);
        const unsigned long long t = (((unsigned long long)hi << 32) | lo) + (((unsigned long long)ohi << 32) | olo);
        lo = (uint32_t)t;
        hi = (uint32_t)(t >> 32);
    }
    if (lane == 0)
        part[wave] = ((unsigned long long)hi << 32) | lo;
    __syncthreads();
    if (threadIdx.x == 0)
        atomicAdd(&sums[j], part[0] + part[1] + part[2] + part[3]);
}

/* lane i: sequence s0 + i of the launch walks its `nsteps` pairs from step k0 in order.  prev comes from carry_in[i] (NULL: 0.0) and
 * goes to carry_out[i] (NULL: nowhere); the launcher points them at mafd_in / mafd_out or at the group's carry slot */
__global__ __launch_bounds__(256) void k_me_scene_flags(const unsigned long long *__restrict__ sums, int ng, int nsteps, int k0, int s0, int nseq, int width,
                                                        int height, int depth, double threshold, const double *carry_in, double *carry_out,
                                                        uint64_t *sad_out, float *score_out, uint8_t *flags_out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= ng)
        return;
    const double prev = mes_scene_walk(nsteps, width, height, depth, threshold, carry_in ? carry_in[i] : 0.0,
        [&](int j) { return (uint64_t)sums[(size_t)j * ng + i]; },
        [&](int j, uint64_t sad, float score, int flag) {
            const size_t o = (size_t)(k0 + j) * nseq + s0 + i;
            if (sad_out)
                sad_out[o] = sad;
            if (score_out)
                score_out[o] = score;
            if (flags_out)
                flags_out[o] = (uint8_t)flag;
        });
    if (carry_out)
        carry_out[i] = prev;
}

int ffhip_launch_me_scene(const uint8_t *frames, int depth, int width, int height, ptrdiff_t stride, size_t frame_pitch, int nframes, size_t seq_pitch,
                          int nseq, double threshold, const double *mafd_in, double *mafd_out, uint64_t *sad_out, float *score_out,
                          uint8_t *flags_out, hipStream_t stream)
{
    static const char *const what = "ffhip_me_scene_sequence_dev: copy or launch";
    if (nseq <= 0)
        return 0;
    if (nframes <= 1) {             /* no pair: the carry passes through */
        if (mafd_out && mafd_in)
            HIP_TRY(hipMemcpyAsync(mafd_out, mafd_in, (size_t)nseq * sizeof(double), hipMemcpyDeviceToDevice, stream));
        else if (mafd_out)
            HIP_TRY(hipMemsetAsync(mafd_out, 0, (size_t)nseq * sizeof(double), stream));      /* 0.0 is all bits zero */
        return 0;
    }
    MscParams P = {};
    P.frames = frames;
    P.stride = stride;
    P.frame_pitch = frame_pitch;
    P.seq_pitch = seq_pitch;
    P.width = width;
    P.height = height;
    P.depth = depth;
    P.nseq = nseq;
    P.wide = frame_pitch % 16 == 0;
    const int steps = nframes - 1;
    const unsigned bands = (unsigned)cdiv(height, MSC_ROWS);        /* at most 2048 */
    for (int s0 = 0; s0 < nseq; s0 += MSC_PAIRS_PER_LAUNCH) {
        const int ng = std::min(nseq - s0, MSC_PAIRS_PER_LAUNCH), per = MSC_PAIRS_PER_LAUNCH / ng;    /* steps of a launch: at least 1 */
        const bool split = steps > per;
        FFHipProgressSlot carry = {};
        if (split) {                /* ng doubles <= a slot; nothing to zero: the first launch of the group writes all of them */
            const int r = ffhip_progress_acquire(0, stream, &carry);
            if (r < 0)
                return r;
        }
        double *const held = reinterpret_cast<double *>(carry.prog);
        int r = 0;
        bool launched = false;
        for (int k0 = 0; k0 < steps && r >= 0; k0 += per) {
            const int n = std::min(steps - k0, per);
            const double *cin = k0 == 0 ? (mafd_in ? mafd_in + s0 : nullptr) : held;
            double *cout = k0 + n == steps ? (mafd_out ? mafd_out + s0 : nullptr) : held;
            P.s0 = s0;
            P.ng = ng;
            P.k0 = k0;
            r = ffhip_progress_launch(2 * n * ng, stream, what, [&](const FFHipProgressSlot &ps) {
                unsigned long long *sums = reinterpret_cast<unsigned long long *>(ps.prog);
                if (depth > 8)
                    hipLaunchKernelGGL((k_me_scene_sad<uint16_t>), dim3(bands, (unsigned)(n * ng)), dim3(256), 0, stream, P, sums);
                else
                    hipLaunchKernelGGL((k_me_scene_sad<uint8_t>), dim3(bands, (unsigned)(n * ng)), dim3(256), 0, stream, P, sums);
                hipError_t e = hipGetLastError();
                if (e != hipSuccess)
                    return e;
                launched = true;
                hipLaunchKernelGGL(k_me_scene_flags, dim3((unsigned)cdiv(ng, 256)), dim3(256), 0, stream, sums, ng, n, k0, s0, nseq, width, height, depth,
                                   threshold, cin, cout, sad_out, score_out, flags_out);
                return hipGetLastError();
            });
        }
        if (split) {
            const int r2 = ffhip_progress_release(&carry, stream, launched);
            if (r >= 0 && r2 < 0)
                r = r2;
        }
        if (r < 0)
            return r;
    }
    return 0;
}
