// mcraw_noise.hip -- gfx950 kernels that measure the noise of uint16 mosaics resident in HBM (mcraw_noise_batch): per frame, CFA
// position and signal level a histogram of the local noise energy of 16 x 16 blocks, which the host fits a noise profile to.
// The contract (integers only: bit-exact whatever the order of additions) is in include/mcraw_hip.h; DESIGN.md 34 has the design.
//
// A reduction whose unit of work is a block, not a sample.  A row's dword holds one sample each of the two CFA positions of that
// row parity, so a lane that owns (block, row parity) reads 8 rows x 8 dwords -- two 16-byte loads a row, straight into registers:
// no sample is needed by two lanes, so nothing is staged in LDS and no lane exchanges anything -- and gets the sum s and the
// energy T of both positions from the halves.  A strip of 16 rows x 1024 columns fills 128 lanes, the even rows' wave and the odd
// rows'; a workgroup of 256 threads has two strips under way and owns a run of consecutive strips of one frame
// (mcraw_noise_args.h: noise_plan, noise_lane, noise_strip).  Every accepted (block, position) is one ds_add_u32 into the
// workgroup's LDS copy of hist[4][32][128] (64 KiB: 2 workgroups per CU); the counts of accepted and rejected planes stay in
// registers.  At its end a workgroup adds the non-zero counters to the frame's record with global integer atomics.
// knoise_init writes the empty records first (unless MCRAW_NOISE_ACCUMULATE).
//
// Test build (tests/test_gpu_noise.py):
//   MCRAW_NOISE_MAXSTRIPS=N  at most N strips per workgroup: many workgroups flush into one record at small sizes
// Test builds (tests/test_gpu_est_paths.py, build.EST_PATH_VARIANTS; why each is valid: the head of mcraw_est_paths.h):
//   MCRAW_PATHSA             the path census (mcraw_diag_est_paths: mcraw_align.hip)
//   MCRAW_EST_FRAMES=N       the launch loop takes N frames at a time, each launch with a plan for its own frame count
#ifdef MCRAW_PATHSA
#include "mcraw_est_paths.h"
#define EST_LD_BASE ::mcraw::EP_NS_LD
#endif
#ifdef MCRAW_EST_FRAMES
#define LAUNCH_PIECE MCRAW_EST_FRAMES
#endif
#ifndef EST_PATH
#define EST_PATH(slot, cond)
#endif
#ifndef EST_ONE
#define EST_ONE(slot, cond)
#endif
#include "mcraw_host.h"
#include "mcraw_mosaic.h"
#include "mcraw_noise_args.h"

namespace mcraw {

#ifndef MCRAW_NOISE_MAXSTRIPS
#define MCRAW_NOISE_MAXSTRIPS 0x7FFFFFFF
#endif
constexpr uint32_t NS_MAXSTRIPS = MCRAW_NOISE_MAXSTRIPS;
static_assert(NS_MAXSTRIPS >= 1u, "a workgroup has at least one strip");
static_assert(NS_HIST * sizeof(uint32_t) == 65536u && NS_T == 4 * 64 && NS_HALVES == 2u, "knoise: 64 KiB of LDS, four waves");

struct NoiseArgs {
    const uint16_t *in;
    uint32_t *out; // the launch's first record
    size_t ipitch, ifstride;
    uint32_t x0, y0;                    // the window's origin, even
    uint32_t bx, stripsX, strips, spw;  // NoisePlan
    uint32_t shift;
    uint32_t sat[4], lo[4];
    uint32_t vec; // every 8-column piece of the blocks lies on the 16-byte grid
};

// s and T of the plane in the low (PAR 0) or high (PAR 1) halves of the lane's 8 x 8 dwords.
// A second difference d = a - 2 b + c of uint16 samples is -131070 .. 131070 (18 bits signed), d * d < 2^34 does not fit 32 bits:
// each square is one 32 x 32 -> 64-bit multiply-add (v_mad_i64_i32) into a 64-bit sum, 96 of them, T < 96 * 2^34 < 2^41 (the
// contract's own bounds, |d| <= 4 * 65535 and T < 2^43, are looser).
template <uint32_t PAR>
__device__ __forceinline__ void noise_plane(const uint32_t w[8][8], uint32_t &s, uint64_t &T)
{
    int32_t v[8][8];
    s = 0u;
#pragma unroll
    for (uint32_t r = 0; r < 8u; r++)
#pragma unroll
        for (uint32_t c = 0; c < 8u; c++) {
            v[r][c] = static_cast<int32_t>(half16(w[r][c], PAR));
            s += static_cast<uint32_t>(v[r][c]);
        }
    int64_t t = 0;
#pragma unroll
    for (uint32_t r = 0; r < 8u; r++)
#pragma unroll
        for (uint32_t c = 1; c < 7u; c++) {
            const int32_t d = v[r][c - 1u] - 2 * v[r][c] + v[r][c + 1u];
            t += static_cast<int64_t>(d) * d;
        }
#pragma unroll
    for (uint32_t r = 1; r < 7u; r++)
#pragma unroll
        for (uint32_t c = 0; c < 8u; c++) {
            const int32_t d = v[r - 1u][c] - 2 * v[r][c] + v[r + 1u][c];
            t += static_cast<int64_t>(d) * d;
        }
    T = static_cast<uint64_t>(t);
}

__global__ void __launch_bounds__(NS_T) knoise(const NoiseArgs A)
{
    __shared__ uint32_t s_h[NS_HIST];
    const uint32_t f = blockIdx.y, t0 = blockIdx.x * A.spw, t1 = min(t0 + A.spw, A.strips);
    const uint32_t half = threadIdx.x / NS_SL, lane = threadIdx.x % NS_SL;
    const uint16_t *fin = A.in + static_cast<size_t>(f) * A.ifstride + static_cast<size_t>(A.y0) * A.ipitch + A.x0;
    EST_ONE(EP_NS_WG, true);
    for (uint32_t i = threadIdx.x; i < NS_HIST; i += NS_T)
        s_h[i] = 0u;
    __syncthreads();
    uint32_t nblk[2] = {0u, 0u}, nrej[2] = {0u, 0u}; // of positions 2 * rp, 2 * rp + 1
    const uint32_t rp = lane / NS_SB;                // (wave-uniform: noise_lane's)
    for (uint32_t i = 0; noise_strip(blockIdx.x, A.spw, i, 0u) < t1; i++) {
        const uint32_t t = noise_strip(blockIdx.x, A.spw, i, half);
        const NoiseLane L = noise_lane(A.bx, A.stripsX, t, lane);
        EST_PATH(EP_NS_SKIP_T1, t >= t1);
        EST_PATH(EP_NS_SKIP_INACTIVE, t < t1 && !L.active);
        if (t >= t1 || !L.active)
            continue;
        EST_PATH(EP_NS_BLOCK, true);
        const uint16_t *src = fin + static_cast<size_t>(L.y) * A.ipitch + L.x;
        uint32_t w[8][8];
#pragma unroll
        for (uint32_t r = 0; r < 8u; r++) { // only whole blocks are read: both pieces of a row are full
            load8(src + static_cast<size_t>(2u * r) * A.ipitch, 8u, A.vec != 0u, w[r]);
            load8(src + static_cast<size_t>(2u * r) * A.ipitch + 8u, 8u, A.vec != 0u, w[r] + 4);
        }
        uint32_t mn = 0xFFFFFFFFu, mx = 0u; // of both positions at once
#pragma unroll
        for (uint32_t r = 0; r < 8u; r++)
#pragma unroll
            for (uint32_t c = 0; c < 8u; c++) {
                mn = pk_min(mn, w[r][c]);
                mx = pk_max(mx, w[r][c]);
            }
        uint32_t s[2];
        uint64_t T[2];
        noise_plane<0u>(w, s[0], T[0]);
        noise_plane<1u>(w, s[1], T[1]);
#pragma unroll
        for (uint32_t par = 0; par < 2u; par++) {
            const uint32_t pos = 2u * rp + par;
            EST_PATH(EP_NS_REJ_SAT, half16(mx, par) >= A.sat[pos]);
            EST_PATH(EP_NS_REJ_LO, half16(mx, par) < A.sat[pos] && half16(mn, par) < A.lo[pos]);
            EST_PATH(EP_NS_ACCEPT, half16(mx, par) < A.sat[pos] && half16(mn, par) >= A.lo[pos]);
            if (half16(mx, par) >= A.sat[pos] || half16(mn, par) < A.lo[pos]) {
                nrej[par]++;
            } else {
                nblk[par]++;
                atomicAdd(&s_h[noise_hist_index(pos, noise_level_bin(s[par], A.shift), noise_energy_bin(T[par]))], 1u);
            }
        }
    }
    // the registers: reduce over the wave (one row parity), then one lane adds to the record
    uint32_t *rec = A.out + static_cast<size_t>(f) * NS_RECWORDS;
#pragma unroll
    for (uint32_t par = 0; par < 2u; par++) {
        uint32_t nb = nblk[par], nr = nrej[par];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            nb += __shfl_xor(nb, d);
            nr += __shfl_xor(nr, d);
        }
        EST_PATH(EP_NS_REG_FLUSH, __lane_id() == 0u && nb != 0u);
        EST_PATH(EP_NS_REG_FLUSH, __lane_id() == 0u && nr != 0u);
        if (__lane_id() == 0u) {
            if (nb)
                atomicAdd(rec + NS_HIST + 2u * rp + par, nb);
            if (nr)
                atomicAdd(rec + NS_HIST + 4u + 2u * rp + par, nr);
        }
    }
    // the histogram: the non-zero counters only
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < NS_HIST; i += NS_T) {
        const uint32_t c = s_h[i];
        EST_PATH(EP_NS_HIST_FLUSH, c != 0u);
        if (c)
            atomicAdd(rec + i, c);
    }
}

// Empty records: every counter 0.
__global__ void __launch_bounds__(256) knoise_init(uint32_t *out, size_t words)
{
    const size_t step = static_cast<size_t>(gridDim.x) * blockDim.x;
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < words; i += step)
        out[i] = 0u;
}

} // namespace mcraw

using namespace mcraw;

extern "C" size_t mcraw_noise_record_bytes(void) { return NS_REC_BYTES; }

extern "C" uint32_t mcraw_noise_energy_bin(uint64_t T) { return noise_energy_bin(T); }

extern "C" int mcraw_noise_batch(mcraw_ctx *c, const mcraw_noise *s, const uint16_t *in, size_t in_pitch, size_t in_frame_stride,
                                 int width, int height, int n, void *out, size_t out_bytes, void *stream)
{
    if (!c || !s || n < 0)
        return reject(__func__, "bad arguments");
    if (n == 0)
        return 0;
    if (!in || !out)
        return reject(__func__, "in or out missing");
    if (reinterpret_cast<uintptr_t>(in) & 1u)
        return reject(__func__, "in not aligned to uint16");
    if (reinterpret_cast<uintptr_t>(out) & 7u)
        return reject(__func__, "out not 8-byte aligned");
    const MosaicBatch I(in, in_pitch, in_frame_stride, static_cast<size_t>(n), width, height);
    if (const char *why = I.check())
        return reject(__func__, why);
    if (const char *why = noise_check(*s, width, height))
        return reject(__func__, why);
    const size_t need = static_cast<size_t>(n) * NS_REC_BYTES;
    if (out_bytes < need)
        return reject(__func__, "out_bytes below n * mcraw_noise_record_bytes()");
    if (ranges_overlap(I.base, I.bytes(), reinterpret_cast<uintptr_t>(out), need))
        return reject(__func__, "out overlaps the input");

    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = stream_of(c, stream);
    NoiseArgs A{};
    A.ipitch = in_pitch;
    A.ifstride = in_frame_stride;
    A.x0 = s->x0, A.y0 = s->y0;
    A.vec = I.on_grid() && s->x0 % 8u == 0u;
    A.shift = s->shift;
    for (uint32_t p = 0; p < 4u; p++)
        A.sat[p] = s->sat[p], A.lo[p] = s->lo[p];
    if (!(s->flags & MCRAW_NOISE_ACCUMULATE)) {
        const size_t words = need / 4u;
        const uint32_t blocks = static_cast<uint32_t>(std::min<size_t>((words + 255u) / 256u, 4096u));
        hipLaunchKernelGGL(knoise_init, dim3(blocks), dim3(256), 0, st, static_cast<uint32_t *>(out), words);
        HIP_TRY(hipGetLastError());
    }
    for (int f0 = 0; f0 < n; f0 += LAUNCH_PIECE) {
        const int nf = std::min<int>(LAUNCH_PIECE, n - f0);
        const NoisePlan P = noise_plan(s->w, s->h, static_cast<uint32_t>(nf), NS_MAXSTRIPS);
        A.bx = P.bx, A.stripsX = P.stripsX, A.strips = P.strips, A.spw = P.spw;
        A.in = in + static_cast<size_t>(f0) * in_frame_stride;
        A.out = static_cast<uint32_t *>(out) + static_cast<size_t>(f0) * NS_RECWORDS;
        hipLaunchKernelGGL(knoise, dim3(P.wgs, static_cast<uint32_t>(nf)), dim3(NS_T), 0, st, A);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}
