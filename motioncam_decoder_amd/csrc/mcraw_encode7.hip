// mcraw_encode7.hip -- the type-7 ENCODER: uint16 Bayer mosaics in HBM -> type-7 frame buffers, byte for byte what
// the input synthesiser's mcraw_synth_encode7(out, cap, img, w, h, NULL, 0) writes (synth/mcraw_synth.c), and the
// mcraw_encode_batch entry point of include/mcraw_hip.h.
//
// Two launches per batch:
//   k7e_payload  one pass over the mosaics.  A workgroup owns a SEGMENT of 64 consecutive tiles (256 blocks, four
//                side-stream records) of one frame, taken from the frame's ticket counter; it loads the tiles with
//                16-byte loads, reduces min / max per block across lanes, stages the residuals in LDS, finds the
//                segment's byte offset by a decoupled look-back over the frame's earlier segments, packs every block at
//                its class and stores it.  It also leaves each block's bits and ref and each record's header in workspace.
//   k7e_side     the two side streams (one lane per record: prefix over the record lengths, pack), the 16-byte header
//                and the frame's byte count.
#include "mcraw_dev.h"
#include "mcraw_host.h"
#ifdef MCRAW_PATHSE
#include "mcraw_census.h"
#endif

namespace mcraw {

constexpr uint32_t EB_T = 256;                 // threads per workgroup (both kernels)
constexpr uint32_t SEG_TILES = 64;             // tiles per segment of k7e_payload
constexpr uint32_t SEG_BLOCKS = 4 * SEG_TILES; // blocks per segment
constexpr uint32_t SEG_RECS = SEG_BLOCKS / 64; // side-stream records per segment
constexpr uint32_t TICKET_STRIDE7E = 64;       // uint32 words between two frames' ticket counters (256 bytes)
constexpr uint32_t SIDE_RECS = EB_T;           // records per workgroup of k7e_side (one per lane)
constexpr uint32_t SIDE_STRIDE = 9;            // uint4 per lane in k7e_side's LDS (8 used: the ninth staggers the banks)

// Look-back words (EncWork::look, never cleared): epoch << 32 | state << 30 | payload bytes / 8.  A word is complete in
// itself, so it is published by ONE relaxed device-scope store and read by relaxed device-scope loads: no fence.
constexpr uint32_t LB_AGG = 1u, LB_PREFIX = 2u, LB_FAIL = 3u;
#ifdef MCRAW_INJECT_LOSTE // test builds (below): a segment of the batch's first frame never publishes
constexpr uint32_t SPIN7E = 1u << 12;
#else
constexpr uint32_t SPIN7E = 1u << 20; // polls of an unchanged window before the frame is given up (status MCRAW_E_DEVICE)
#endif

// Test builds of the encoder (tests/test_gpu_enc7_paths.py, build.ENC7_PATH_VARIANTS; none of this is in the product library).
// Which way a workgroup of k7e_payload goes is decided by the frame's content and geometry -- loads, classes, records -- and by
// timing: whether its guess was its ticket, and what its look-back finds published.  Every switch below chooses among ways that
// are right for EVERY input:
//   MCRAW_PATHSE              the path census below
//   MCRAW_FORCE_REFETCHE      the guess is never fetched; every live workgroup fetches its segment behind the ticket.  The
//                             guess is only a prefetch: what a workgroup encodes is always the segment of its ticket.
//   MCRAW_FORCE_AGGONLYE      a segment behind the first never upgrades its word to LB_PREFIX (it still publishes LB_FAIL).  A
//                             look-back adds aggregates until it meets a prefix, and segment 0's word is a prefix from the
//                             start, so every look-back walks to segment 0: the sum of all aggregates in front, which IS the
//                             prefix.  A word that stays an aggregate says nothing wrong; it only says less.
//   MCRAW_INJECT_SLOWE        workgroups whose segment is 3 mod 8 sleep in front of their first look_put: 64 times s_sleep 127,
//                             520192 clocks.  Their successors poll meanwhile.  SPIN7E polls are 2^20 times s_sleep 1 and a
//                             load: above 2^26 clocks, 129 times the sleep, so no look-back gives up.  Only WHEN a word
//                             appears changes; the kernel is right for any time.
//   MCRAW_INJECT_LOSTE        in launches of an odd epoch, the workgroup that takes segment 3 of frame 0 returns behind its
//                             ticket (and the ticket's reset): it publishes nothing and stores nothing -- where the frame has a
//                             segment 4 to wait for it; a frame that ends with segment 3 would otherwise be left with no
//                             failure recorded and no total.  SPIN7E is 2^12, as the legacy decoder's lost-word build has
//                             SPIN6: every later segment of the frame gives up within its bound or meets the LB_FAIL of one
//                             that has, the frame comes back with MCRAW_E_DEVICE and the launch ends.  Every wait keeps its
//                             bound.  So that
//                             LB_FAIL is also MET, not only published, the frame's segments from 8 on first poll segment
//                             4's word until it says LB_FAIL -- it must give up, and they poll 2^16 times at most, bounded
//                             as well -- and then find that failure or one behind it within their first window (without the
//                             wait they add those words up and give up at segment 3 themselves: either is right).
//   MCRAW_EPOCH0E=v           the epoch a context's encode state starts from.  Any value is a valid state: it is what the
//                             counter holds after v batches, but for the workspace's words, and a fresh workspace holds zeros,
//                             which no launch's epoch equals.  0xFFFFFFFD: the third batch of a context wraps to 1.
#ifdef MCRAW_PATHSE
// What the workgroups of the two kernels did, summed over the launches since the last reset (mcraw_diag_k7e_paths).  Both kernels
// keep their counts in registers -- KE_ONE: thread 0 counts what is uniform over the workgroup or over wave 0, KE_LANE: every
// lane counts its own -- and where the workgroup ends, every early return included, KE_FLUSH sums the lanes and thread 0 adds the
// sums once.
enum PathE {
    // ---- k7e_payload
    PE_LIVE, PE_IDLE,                   // workgroups whose ticket is a segment of the frame / lies behind it (seg >= F.nseg)
    PE_HIT, PE_REFETCHED,               // live workgroups whose guess was their ticket / that fetched again behind it
    PE_LOADS16, PE_LOADS_EDGE,          // loads of the segment encoded, per lane and tile round: 16 bytes / the clamp_par loop
    PE_LOADS_CLAMPED_ROW,               // ... of a row below the frame (4 ty + r >= h)
    PE_DEAD_TILES,                      // tiles behind the frame in live segments
    PE_CLASS0,                          // blocks of the frame at each class 0..16 (17 counters)
    PE_ROWS = PE_CLASS0 + 17,           // 8-byte payload rows stored (agg)
    PE_REFS_CLAMPED,                    // refs records whose minimum is above the header's 12 bits (rmn > 4095)
    PE_LOOKBACKS,                       // look-backs started (seg > 0)
    PE_WINDOWS,                         // windows that a look-back took words from
    PE_WORDS,                           // predecessor words added into acc
    PE_POLLS,                           // polls of a window whose nearest word is not there
    PE_GAVE_UP, PE_MET_FAIL,            // look-backs that ran out of polls / that met LB_FAIL
    PE_NEVER,                           // hits of the bound check behind the look-back
    // ---- k7e_side
    PE_SIDE_BAD, PE_SIDE_FAIL, PE_SIDE_IDLE, // workgroups that return for F.bad || !F.nseg / for a failed look-back / for first >= R
    PE_SIDE_CHUNKS,                     // workgroups that write records with chunk > 0 (records of their stream in front: pre)
    PE_BITS_REC0,                       // records written in the bits stream at each header class 0..15
    PE_REFS_REC0 = PE_BITS_REC0 + 16,   // ... in the refs stream
    PE_HEADERS = PE_REFS_REC0 + 16,     // frame headers written
    PE_N,
    PE_SIDE0 = PE_SIDE_BAD              // (the first counter of k7e_side)
};
__device__ unsigned long long g_k7e_paths[PE_N];
#define KE_ONE(slot, v)                                                                                                \
    do {                                                                                                               \
        if (tid == 0u)                                                                                                 \
            pe_[slot] += static_cast<uint32_t>(v);                                                                     \
    } while (0)
#define KE_LANE(slot, v) (pe_[slot] += static_cast<uint32_t>(v))
// (every thread of the workgroup is here: the returns it stands in front of are uniform)
#define KE_FLUSH(LO, HI)                                                                                               \
    do {                                                                                                               \
        _Pragma("unroll") for (uint32_t i_ = LO; i_ < HI; i_++)                                                        \
        {                                                                                                              \
            const uint32_t v_ = wave_sum(pe_[i_]);                                                                     \
            if (lane == 0u)                                                                                            \
                s_pe[wave][i_ - LO] = v_;                                                                              \
        }                                                                                                              \
        __syncthreads();                                                                                               \
        if (tid == 0u)                                                                                                 \
            for (uint32_t i_ = 0; i_ < HI - LO; i_++) {                                                                \
                uint32_t v_ = 0;                                                                                       \
                for (uint32_t k_ = 0; k_ < EB_T / 64u; k_++)                                                           \
                    v_ += s_pe[k_][i_];                                                                                \
                if (v_)                                                                                                \
                    atomicAdd(&g_k7e_paths[LO + i_], static_cast<unsigned long long>(v_));                             \
            }                                                                                                          \
    } while (0)
#else
#define KE_ONE(slot, v)
#define KE_LANE(slot, v)
#define KE_FLUSH(LO, HI)
#endif

// One frame of an encode batch as the kernels see it (uploaded per batch).
struct EncF {
    const uint16_t *in;
    uint8_t *out;
    uint64_t *len_out; // optional (device memory)
    int32_t w, h;
    uint32_t tilesX, ntiles; // encW / 64; tiles of the frame
    uint32_t nseg, R;        // segments (k7e_payload); side-stream records = ceil(blocks / 64)
    int32_t bad;             // MCRAW_E_ARGS / MCRAW_E_CAPACITY found by the host: the kernels write nothing but the status
    uint32_t pad;
    uint64_t bound;          // mcraw_encode_bound7 (<= out_capacity): no store goes past it
};

// Workspace of a batch; every per-frame array has the stride of the batch's largest frame.
struct EncWork {
    const EncF *fr;
    uint64_t *look;    // [n][smax] look-back words
    uint32_t *tickets; // [n][TICKET_STRIDE7E] segment tickets (zero between launches: the last ticket of a frame resets it)
    uint8_t *bnb;      // [n][64 rmax] bits of every block (the bits stream's entries), 0 behind the frame's blocks
    uint16_t *bref;    // [n][64 rmax] ref of every block (the refs stream's entries)
    uint16_t *rh;      // [n][2][rmax] record headers: hb << 12 | ref
    uint32_t *tot;     // [n] payload bytes / 8
    uint32_t *fail;    // [n] the epoch of the last launch in which a look-back of the frame gave up (never cleared)
    uint64_t *wlen;    // [n] bytes written (0 on failure)
    int32_t *wst;      // [n] status
    uint32_t n, smax, rmax, epoch;
};

// Past the frame's edge: the last pixel of the same Bayer parity (mcraw_synth_encode7's padding rule).
__device__ __forceinline__ uint32_t clamp_par(uint32_t x, uint32_t n)
{
    if (x < n)
        return x;
    const int32_t c = static_cast<int32_t>(n - 1u) - static_cast<int32_t>(((n - 1u) ^ x) & 1u);
    return c < 0 ? 0u : static_cast<uint32_t>(c);
}

__device__ __forceinline__ uint32_t swz_xor(uint32_t v, int m)
{
    // ds_swizzle bit mode inside 32 lanes: and 0x1F, or 0, xor m
    switch (m) {
    case 1: return static_cast<uint32_t>(__builtin_amdgcn_ds_swizzle(static_cast<int>(v), 0x041F));
    case 2: return static_cast<uint32_t>(__builtin_amdgcn_ds_swizzle(static_cast<int>(v), 0x081F));
    case 4: return static_cast<uint32_t>(__builtin_amdgcn_ds_swizzle(static_cast<int>(v), 0x101F));
    default: return static_cast<uint32_t>(__builtin_amdgcn_ds_swizzle(static_cast<int>(v), 0x401F)); // 16
    }
}

__device__ __forceinline__ u16x2 as_u16x2(uint32_t v) { return __builtin_bit_cast(u16x2, v); }
__device__ __forceinline__ uint32_t as_u32(u16x2 v) { return __builtin_bit_cast(uint32_t, v); }

__device__ __forceinline__ uint32_t wave_min(uint32_t v)
{
    for (int m = 32; m >= 1; m >>= 1)
        v = min(v, static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), m)));
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
    for (int m = 32; m >= 1; m >>= 1)
        v = max(v, static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), m)));
    return v;
}

// Sample j (0..7) of a row of eight residuals held as uint4.
template <int J>
__device__ __forceinline__ uint32_t el(const uint4 &r)
{
    const uint32_t w = J < 2 ? r.x : (J < 4 ? r.y : (J < 6 ? r.z : r.w));
    return (J & 1) ? w >> 16 : w & 0xFFFFu;
}

// Row `i` (8 bytes) of a block of 64 residuals v[0..63] (sample 8k + j = element j of vv[k]) stored at class `nb`:
// out byte 8 i + j of mcraw_synth_pack_block7 -- the layouts unpack8 / item_decode in mcraw_type7.hip read.  Every byte of
// a row is an OR of terms ((v[8k + j] >> sh) & (2^wb - 1)) << pos over a few k.
__device__ __forceinline__ uint2 pack_row7(uint32_t nb, uint32_t i, const uint4 *vv)
{
    if (nb >= 11u) { // raw 16: samples 4i .. 4i + 3, little-endian
        const uint4 r = vv[i >> 1];
        return (i & 1u) ? make_uint2(r.z, r.w) : make_uint2(r.x, r.y);
    }
    uint32_t b0 = 0, b1 = 0, b2 = 0, b3 = 0, b4 = 0, b5 = 0, b6 = 0, b7 = 0;
    auto T = [&](uint32_t k, uint32_t sh, uint32_t wb, uint32_t pos) {
        const uint4 r = vv[k];
        const uint32_t m = (1u << wb) - 1u;
        b0 |= ((el<0>(r) >> sh) & m) << pos;
        b1 |= ((el<1>(r) >> sh) & m) << pos;
        b2 |= ((el<2>(r) >> sh) & m) << pos;
        b3 |= ((el<3>(r) >> sh) & m) << pos;
        b4 |= ((el<4>(r) >> sh) & m) << pos;
        b5 |= ((el<5>(r) >> sh) & m) << pos;
        b6 |= ((el<6>(r) >> sh) & m) << pos;
        b7 |= ((el<7>(r) >> sh) & m) << pos;
    };
    switch (nb) {
    case 1:
        for (uint32_t k = 0; k < 8u; k++)
            T(k, 0, 1, k);
        break;
    case 2:
        for (uint32_t k = 0; k < 4u; k++)
            T(4u * i + k, 0, 2, 2u * k);
        break;
    case 3:
        if (i < 2u) {
            T(3u * i, 0, 3, 0);
            T(3u * i + 1u, 0, 3, 3);
            T(3u * i + 2u, 0, 2, 6);
        } else {
            T(6, 0, 3, 0);
            T(7, 0, 3, 3);
            T(2, 2, 1, 6);
            T(5, 2, 1, 7);
        }
        break;
    case 4:
        T(2u * i, 0, 4, 0);
        T(2u * i + 1u, 0, 4, 4);
        break;
    case 5:
        T(i, 0, 5, 0);
        if (i < 3u) {
            T(5u + i, 0, 3, 5);
        } else {
            T(2u + i, 3, 2, 5); // row 3: v[40 + j] >> 3, row 4: v[48 + j] >> 3
            T(7, i, 1, 7);      // row 3: bit 3 of v[56 + j], row 4: bit 4
        }
        break;
    case 6:
        T(i, 0, 6, 0);
        T(i < 3u ? 6u : 7u, 2u * (i < 3u ? i : i - 3u), 2, 6);
        break;
    case 7:
    case 8:
        T(i, 0, 8, 0);
        break;
    case 9:
    case 10: {
        const uint32_t h = i >= 5u ? 1u : 0u, ii = i - 5u * h;
        if (ii < 4u) {
            T(4u * h + ii, 0, 8, 0);
        } else {
            for (uint32_t t = 0; t < 4u; t++)
                T(4u * h + t, 8, 2, 2u * t);
        }
        break;
    }
    default:
        break;
    }
    return make_uint2(b0 | b1 << 8 | b2 << 16 | b3 << 24, b4 | b5 << 8 | b6 << 16 | b7 << 24);
}

typedef uint32_t u32x4_a2 __attribute__((ext_vector_type(4), aligned(2)));
typedef uint32_t u32x2_a1 __attribute__((ext_vector_type(2), aligned(1)));
typedef uint32_t u32x4_a1 __attribute__((ext_vector_type(4), aligned(1)));
typedef uint16_t u16_a1 __attribute__((aligned(1)));
typedef uint32_t u32_a1 __attribute__((aligned(1)));

// (pointers loaded from the frame table are generic to the compiler: gptr keeps these global, not FLAT, accesses)
__device__ __forceinline__ void st8(uint8_t *p, uint2 v) { *gptr<u32x2_a1>(p) = u32x2_a1{v.x, v.y}; }

// ---------------------------------------------------------------------------------------------------- k7e_payload
// Grid: n * smax workgroups, the frames interleaved (workgroup b is one of frame b % n's smax): a frame's segments start in
// order and far apart.  The segment itself comes from the frame's ticket counter, so every segment a workgroup waits for
// was taken by a workgroup that is running or done, whatever order the hardware starts workgroups in.
__global__ __launch_bounds__(EB_T) void k7e_payload(const EncWork W)
{
    __shared__ __attribute__((aligned(16))) uint16_t s_v[SEG_BLOCKS * 64]; // residuals, block m at [64 m], sample order
    __shared__ uint32_t s_off[SEG_BLOCKS];                                  // byte offset of block m inside the segment
    __shared__ uint8_t s_row[SEG_BLOCKS * 16];                              // 8-byte row q of the segment's payload -> its block
    __shared__ uint8_t s_nb[SEG_BLOCKS];
    __shared__ uint16_t s_ref[SEG_BLOCKS];
    __shared__ uint32_t s_wsum[EB_T / 64], s_ticket, s_base;
#ifdef MCRAW_PATHSE
    __shared__ uint32_t s_pe[EB_T / 64][PE_SIDE0];
    uint32_t pe_[PE_N] = {};
#endif

    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint32_t f = blockIdx.x % W.n, guess = blockIdx.x / W.n;
    const EncF F = W.fr[f];
    const uint32_t w = static_cast<uint32_t>(F.w), h = static_cast<uint32_t>(F.h);
    if (tid == 0)
        s_ticket = atomicAdd(W.tickets + f * TICKET_STRIDE7E, 1u);

    // lane -> (tile of the round, row r, 8-pixel column c): a wave covers two tiles per 16-byte load
    const uint32_t r = (lane >> 3) & 3u, c = lane & 7u;
    uint4 v[SEG_TILES / 8];
    auto fetch = [&](uint32_t seg) {
#pragma unroll
        for (uint32_t q = 0; q < SEG_TILES / 8u; q++) {
            const uint32_t t = seg * SEG_TILES + q * 8u + wave * 2u + (lane >> 5);
            if (t >= F.ntiles) {
                v[q] = make_uint4(0u, 0u, 0u, 0u);
                continue;
            }
            const uint32_t ty = t / F.tilesX, tx = t - ty * F.tilesX;
            const uint32_t y = clamp_par(4u * ty + r, h), x0 = 64u * tx + 8u * c;
            const uint16_t *row = F.in + static_cast<size_t>(y) * w;
            KE_LANE(PE_LOADS_CLAMPED_ROW, 4u * ty + r >= h);
            if (x0 + 8u <= w) {
                KE_LANE(PE_LOADS16, 1);
                const u32x4_a2 a = *gptr<const u32x4_a2>(row + x0);
                v[q] = make_uint4(a.x, a.y, a.z, a.w);
            } else { // the frame's right edge
                KE_LANE(PE_LOADS_EDGE, 1);
                uint32_t p[8];
#pragma unroll
                for (uint32_t k = 0; k < 8u; k++)
                    p[k] = *gptr<const uint16_t>(row + clamp_par(x0 + k, w));
                v[q] = make_uint4(p[0] | p[1] << 16, p[2] | p[3] << 16, p[4] | p[5] << 16, p[6] | p[7] << 16);
            }
        }
    };
#ifndef MCRAW_FORCE_REFETCHE
    if (guess < F.nseg)
        fetch(guess);
#endif
    __syncthreads();
    const uint32_t seg = s_ticket;
    if (seg == W.smax - 1u && tid == 0) // the frame's last ticket: its counter is back at zero for the next launch
        __hip_atomic_store(W.tickets + f * TICKET_STRIDE7E, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (seg >= F.nseg) {
        KE_ONE(PE_IDLE, 1);
        KE_FLUSH(0, PE_LOADS16); // (what the lanes counted while they fetched the guess is of no segment)
        return;
    }
    KE_ONE(PE_LIVE, 1);
#ifdef MCRAW_FORCE_REFETCHE
    (void)guess;
    KE_ONE(PE_REFETCHED, 1);
    fetch(seg);
#else
    KE_ONE(PE_HIT, seg == guess);
    KE_ONE(PE_REFETCHED, seg != guess);
#ifdef MCRAW_PATHSE
    if (seg != guess) // (the loads counted are those of the segment encoded)
        pe_[PE_LOADS16] = pe_[PE_LOADS_EDGE] = pe_[PE_LOADS_CLAMPED_ROW] = 0u;
#endif
    if (seg != guess)
        fetch(seg);
#endif
#ifdef MCRAW_INJECT_LOSTE
    if ((W.epoch & 1u) && f == 0u && seg == 3u && F.nseg > 4u) {
        KE_FLUSH(0, PE_LOADS16); // (it encodes no segment: its loads are not counted)
        return;
    }
#endif

    // ---- per block: min / max across the 16 lanes that hold it (rows r and r + 2, columns 0..7), residuals -> LDS
#pragma unroll
    for (uint32_t q = 0; q < SEG_TILES / 8u; q++) {
        const uint32_t tl = q * 8u + wave * 2u + (lane >> 5); // tile inside the segment
        const bool live = seg * SEG_TILES + tl < F.ntiles;
        const u16x2 a0 = as_u16x2(v[q].x), a1 = as_u16x2(v[q].y), a2 = as_u16x2(v[q].z), a3 = as_u16x2(v[q].w);
        // (even-column sample, odd-column sample) pairs: the two blocks of row parity r & 1
        u16x2 mn = __builtin_elementwise_min(__builtin_elementwise_min(a0, a1), __builtin_elementwise_min(a2, a3));
        u16x2 mx = __builtin_elementwise_max(__builtin_elementwise_max(a0, a1), __builtin_elementwise_max(a2, a3));
#pragma unroll
        for (int m = 1; m <= 16; m <<= 1) {
            if (m == 8)
                continue;
            mn = __builtin_elementwise_min(mn, as_u16x2(swz_xor(as_u32(mn), m)));
            mx = __builtin_elementwise_max(mx, as_u16x2(swz_xor(as_u32(mx), m)));
        }
        const uint32_t mb = 4u * tl + 2u * (r & 1u); // block of the even columns; +1: odd columns
        KE_LANE(PE_DEAD_TILES, !live && (lane & 31u) == 0u);
        if (live) {
            const uint32_t mnw = as_u32(mn);
            const uint32_t d0 = as_u32(a0 - mn), d1 = as_u32(a1 - mn), d2 = as_u32(a2 - mn), d3 = as_u32(a3 - mn);
            const uint32_t i0 = (r >> 1) * 32u + 4u * c; // first of my four samples in each block
            *reinterpret_cast<uint2 *>(&s_v[mb * 64u + i0]) =
                make_uint2(__builtin_amdgcn_perm(d1, d0, 0x05040100u), __builtin_amdgcn_perm(d3, d2, 0x05040100u));
            *reinterpret_cast<uint2 *>(&s_v[(mb + 1u) * 64u + i0]) =
                make_uint2(__builtin_amdgcn_perm(d1, d0, 0x07060302u), __builtin_amdgcn_perm(d3, d2, 0x07060302u));
            if (c == 0u && r < 2u) {
                const uint32_t mxw = as_u32(mx);
                const uint32_t de = (mxw & 0xFFFFu) - (mnw & 0xFFFFu), dod = (mxw >> 16) - (mnw >> 16);
                s_nb[mb] = static_cast<uint8_t>(32 - __clz(de));
                s_nb[mb + 1u] = static_cast<uint8_t>(32 - __clz(dod));
                s_ref[mb] = static_cast<uint16_t>(mnw & 0xFFFFu);
                s_ref[mb + 1u] = static_cast<uint16_t>(mnw >> 16);
            }
        } else if (c == 0u && r < 2u) { // blocks behind the frame: zero entries in both side streams, no payload
            s_nb[mb] = s_nb[mb + 1u] = 0;
            s_ref[mb] = s_ref[mb + 1u] = 0;
        }
    }
    __syncthreads();

    // ---- block lengths: prefix inside the segment; entries and record headers -> workspace
    const uint32_t m = tid;
    const uint32_t nbm = s_nb[m], refm = s_ref[m];
    const uint32_t lm = len7_of(nbm);
#ifdef MCRAW_PATHSE
#pragma unroll
    for (uint32_t k = 0; k <= 16u; k++)
        pe_[PE_CLASS0 + k] += seg * SEG_BLOCKS + m < 4u * F.ntiles && nbm == k;
#endif
    uint32_t wtot;
    const uint32_t excl = wave_excl_scan(lm, lane, &wtot);
    if (lane == 0u)
        s_wsum[wave] = wtot;
    const size_t fb = static_cast<size_t>(f) * W.rmax * 64u; // the frame's entries
    const uint32_t gb = seg * SEG_BLOCKS + m;
    const uint32_t rec = seg * SEG_RECS + wave;
    if (rec < F.R) { // my wave's record: entries 64 rec .. 64 rec + 63 (zero behind the frame's blocks)
        W.bnb[fb + gb] = static_cast<uint8_t>(nbm);
        W.bref[fb + gb] = static_cast<uint16_t>(refm);
        const uint32_t bmn = wave_min(nbm), bmx = wave_max(nbm), rmn = wave_min(refm), rmx = wave_max(refm);
        if (lane == 0u) {
            const uint32_t bref = bmn, rref = min(rmn, 4095u);
            KE_LANE(PE_REFS_CLAMPED, rmn > 4095u);
            const uint32_t bhb = min(15u, 32u - __clz(bmx - bref)), rhb = min(15u, 32u - __clz(rmx - rref));
            const size_t rb = static_cast<size_t>(f) * 2u * W.rmax;
            W.rh[rb + rec] = static_cast<uint16_t>(bhb << 12 | bref);
            W.rh[rb + W.rmax + rec] = static_cast<uint16_t>(rhb << 12 | rref);
        }
    }
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (uint32_t k = 0; k < EB_T / 64u; k++) {
        before += k < wave ? s_wsum[k] : 0u;
        total += s_wsum[k];
    }
    s_off[m] = before + excl;
    for (uint32_t i = 0; i < lm >> 3; i++)
        s_row[((before + excl) >> 3) + i] = static_cast<uint8_t>(m);

    // ---- the segment's offset in the frame: decoupled look-back (wave 0)
    uint64_t *const look = W.look + static_cast<size_t>(f) * W.smax;
    const uint32_t agg = total >> 3; // every block length is a multiple of 8
    if (wave == 0u) {
#ifdef MCRAW_INJECT_SLOWE
        if (seg % 8u == 3u)
            for (uint32_t k = 0; k < 64u; k++)
                __builtin_amdgcn_s_sleep(127);
#endif
        if (tid == 0)
            look_put(look + seg, W.epoch, (seg ? LB_AGG : LB_PREFIX) << 30 | agg);
        uint32_t acc = 0;
        bool failed = false;
#ifdef MCRAW_INJECT_LOSTE
        if ((W.epoch & 1u) && f == 0u && seg >= 8u && F.nseg > 4u) // (until segment 4 has given up, sixteen give-ups long at most)
            for (uint32_t k = 0; k < 16u * SPIN7E; k++) {
                uint32_t w4;
                if (look_get(look + 4, W.epoch, &w4) && w4 >> 30 == LB_FAIL)
                    break;
                __builtin_amdgcn_s_sleep(1);
            }
#endif
        if (seg > 0u) {
            KE_ONE(PE_LOOKBACKS, 1);
            int32_t i = static_cast<int32_t>(seg) - 1;
            uint32_t spins = 0;
            while (true) {
                const int32_t j = i - static_cast<int32_t>(lane);
                uint32_t wd = LB_PREFIX << 30; // (in front of segment 0: nothing)
                const bool ready = j < 0 || look_get(look + j, W.epoch, &wd);
                const uint32_t st = wd >> 30, val = wd & 0x3FFFFFFFu;
                const uint64_t notready = __ballot(!ready), stop = __ballot(ready && st != LB_AGG);
                const uint32_t fnr = notready ? static_cast<uint32_t>(__builtin_ctzll(notready)) : 64u;
                const uint32_t fst = stop ? static_cast<uint32_t>(__builtin_ctzll(stop)) : 64u;
                if (fst < fnr) { // a prefix (or a failure) with only aggregates in front of it
                    acc += wave_sum(lane <= fst ? val : 0u);
                    failed = __shfl(static_cast<int>(st), static_cast<int>(fst)) == static_cast<int>(LB_FAIL);
                    KE_ONE(PE_WINDOWS, 1);
                    KE_ONE(PE_WORDS, min(static_cast<int32_t>(fst), i) + 1); // (lanes in front of segment 0 hold no word)
                    KE_ONE(PE_MET_FAIL, failed);
                    break;
                }
                if (fnr > 0u) {
                    acc += wave_sum(lane < fnr ? val : 0u);
                    i -= static_cast<int32_t>(fnr);
                    spins = 0;
                    KE_ONE(PE_WINDOWS, 1);
                    KE_ONE(PE_WORDS, fnr);
                } else if (++spins > SPIN7E) {
                    failed = true;
                    KE_ONE(PE_GAVE_UP, 1);
                    break;
                } else {
                    KE_ONE(PE_POLLS, 1);
                    __builtin_amdgcn_s_sleep(1);
                }
            }
            if (tid == 0) {
#ifdef MCRAW_FORCE_AGGONLYE
                if (failed)
#endif
                look_put(look + seg, W.epoch, (failed ? LB_FAIL : LB_PREFIX) << 30 | ((acc + agg) & 0x3FFFFFFFu));
                if (failed)
                    W.fail[f] = W.epoch;
            }
        }
        if (!failed && 16u + 8ull * (acc + agg) + 2u * (4u + 130ull * F.R) > F.bound) { // (never: a look-back word is wrong)
            failed = true;
            KE_ONE(PE_NEVER, 1);
            if (tid == 0)
                W.fail[f] = W.epoch;
        }
        if (tid == 0) {
            s_base = failed ? 0xFFFFFFFFu : acc;
            if (!failed && seg + 1u == F.nseg)
                W.tot[f] = acc + agg;
        }
    }
    __syncthreads();
    const uint32_t base = s_base;
    if (base == 0xFFFFFFFFu) {
        KE_FLUSH(0, PE_SIDE0);
        return;
    }

    // ---- pack and store: task = 8-byte row q of the segment's payload (only rows that exist: 16 per block would leave most
    // lanes idle on natural frames), consecutive lanes -> consecutive bytes
    uint8_t *const dst = F.out + 16u + 8ull * base;
    const uint4 *const sv = reinterpret_cast<const uint4 *>(s_v);
    for (uint32_t q = tid; q < agg; q += EB_T) {
        const uint32_t mb = s_row[q];
        st8(dst + 8u * q, pack_row7(s_nb[mb], q - (s_off[mb] >> 3), sv + mb * 8u));
    }
    KE_ONE(PE_ROWS, agg);
    KE_FLUSH(0, PE_SIDE0);
}

// ---------------------------------------------------------------------------------------------------- k7e_side
// Grid: n * 2 * ceil(rmax / 256) workgroups: (frame, stream, 256 records).  Lane = record.
__global__ __launch_bounds__(EB_T) void k7e_side(const EncWork W)
{
    __shared__ __attribute__((aligned(16))) uint4 s_v[EB_T * SIDE_STRIDE];
    __shared__ uint32_t s_red[3][EB_T / 64];
#ifdef MCRAW_PATHSE
    __shared__ uint32_t s_pe[EB_T / 64][PE_N - PE_SIDE0];
    uint32_t pe_[PE_N] = {};
#endif

    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint32_t f = blockIdx.x % W.n, rest = blockIdx.x / W.n, s = rest % 2u, chunk = rest / 2u;
    const EncF F = W.fr[f];
    const uint32_t R = F.R;
    const bool head = s == 1u && chunk == 0u; // the workgroup that writes the header, the count fields and the outcome
    if (F.bad || !F.nseg) {
        if (head && tid == 0) {
            W.wst[f] = F.bad ? F.bad : MCRAW_E_ARGS;
            W.wlen[f] = 0;
            if (F.len_out)
                *F.len_out = 0;
        }
        KE_ONE(PE_SIDE_BAD, 1);
        KE_FLUSH(PE_SIDE0, PE_N);
        return;
    }
    if (W.fail[f] == W.epoch) { // a look-back of this launch gave up
        if (head && tid == 0) {
            W.wst[f] = MCRAW_E_DEVICE;
            W.wlen[f] = 0;
            if (F.len_out)
                *F.len_out = 0;
        }
        KE_ONE(PE_SIDE_FAIL, 1);
        KE_FLUSH(PE_SIDE0, PE_N);
        return;
    }
    const uint32_t first = chunk * SIDE_RECS;
    if (first >= R) {
        KE_ONE(PE_SIDE_IDLE, 1);
        KE_FLUSH(PE_SIDE0, PE_N);
        return;
    }
    KE_ONE(PE_SIDE_CHUNKS, chunk > 0u);
    const uint16_t *const rh = W.rh + static_cast<size_t>(f) * 2u * W.rmax;

    // ---- lengths: my stream's records in front of my chunk; the bits stream's total (refs); the refs stream's total (head)
    uint32_t pre = 0, btot = 0, rtot = 0;
    for (uint32_t k = tid; k < R; k += EB_T) {
        const uint32_t lb = 2u + len7_of(rh[k] >> 12), lr = 2u + len7_of(rh[W.rmax + k] >> 12);
        if (k < first)
            pre += s ? lr : lb;
        btot += lb;
        rtot += lr;
    }
    pre = wave_sum(pre);
    btot = wave_sum(btot);
    rtot = wave_sum(rtot);
    if (lane == 0u) {
        s_red[0][wave] = pre;
        s_red[1][wave] = btot;
        s_red[2][wave] = rtot;
    }
    const uint32_t rec = first + tid;
    const bool live = rec < R;
    const uint32_t hdr = live ? rh[s * W.rmax + rec] : 0u, hb = hdr >> 12, ref = hdr & 0xFFFu;
    const uint32_t mylen = live ? 2u + len7_of(hb) : 0u;
    uint32_t wtot;
    const uint32_t excl = wave_excl_scan(mylen, lane, &wtot);
    __syncthreads();
    pre = btot = rtot = 0;
    for (uint32_t k = 0; k < EB_T / 64u; k++) {
        pre += s_red[0][k];
        btot += s_red[1][k];
        rtot += s_red[2][k];
    }
    __syncthreads();
    if (lane == 0u)
        s_red[0][wave] = wtot;
    __syncthreads();
    uint32_t wbefore = 0;
    for (uint32_t k = 0; k < wave; k++)
        wbefore += s_red[0][k];

    const uint64_t boff = 16ull + 8ull * W.tot[f];
    const uint64_t roff = boff + 4u + btot;
    const uint64_t soff = s ? roff : boff;
    if (head && tid == 0) {
        const uint32_t encW = F.tilesX * 64u, encH = (static_cast<uint32_t>(F.h) + 3u) & ~3u;
        *reinterpret_cast<u32x4_a1 *>(F.out) = u32x4_a1{encW, encH, static_cast<uint32_t>(boff), static_cast<uint32_t>(roff)};
        *reinterpret_cast<u32_a1 *>(F.out + boff) = 64u * R;
        *reinterpret_cast<u32_a1 *>(F.out + roff) = 64u * R;
        const uint64_t len = roff + 4u + rtot;
        W.wlen[f] = len;
        W.wst[f] = MCRAW_OK;
        if (F.len_out)
            *F.len_out = len;
        KE_ONE(PE_HEADERS, 1);
    }
#ifdef MCRAW_PATHSE
#pragma unroll
    for (uint32_t k = 0; k < 16u; k++) { // (the record every live lane writes below)
        pe_[PE_BITS_REC0 + k] += live && s == 0u && hb == k;
        pe_[PE_REFS_REC0 + k] += live && s == 1u && hb == k;
    }
#endif
    KE_FLUSH(PE_SIDE0, PE_N); // (in front of the lanes' own return: the workgroup is whole here)
    if (!live)
        return;

    // ---- my record: entries - ref -> LDS, header, rows
    const size_t eb = static_cast<size_t>(f) * W.rmax * 64u + 64u * rec;
    uint4 *const my = s_v + tid * SIDE_STRIDE;
    const uint32_t rr = ref | ref << 16;
    if (s == 0u) {
        const uint4 *src = reinterpret_cast<const uint4 *>(W.bnb + eb);
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            const uint4 a = src[k]; // 16 entries, a byte each -> two rows of eight u16
            const uint32_t e[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (uint32_t hh = 0; hh < 2u; hh++) {
                const uint32_t lo = e[2u * hh], hi = e[2u * hh + 1u];
                uint4 o;
                o.x = as_u32(as_u16x2(__builtin_amdgcn_perm(0u, lo, 0x0C010C00u)) - as_u16x2(rr));
                o.y = as_u32(as_u16x2(__builtin_amdgcn_perm(0u, lo, 0x0C030C02u)) - as_u16x2(rr));
                o.z = as_u32(as_u16x2(__builtin_amdgcn_perm(0u, hi, 0x0C010C00u)) - as_u16x2(rr));
                o.w = as_u32(as_u16x2(__builtin_amdgcn_perm(0u, hi, 0x0C030C02u)) - as_u16x2(rr));
                my[2u * k + hh] = o;
            }
        }
    } else {
        const uint4 *src = reinterpret_cast<const uint4 *>(W.bref + eb);
#pragma unroll
        for (uint32_t k = 0; k < 8u; k++) {
            const uint4 a = src[k];
            my[k] = make_uint4(as_u32(as_u16x2(a.x) - as_u16x2(rr)), as_u32(as_u16x2(a.y) - as_u16x2(rr)),
                               as_u32(as_u16x2(a.z) - as_u16x2(rr)), as_u32(as_u16x2(a.w) - as_u16x2(rr)));
        }
    }
    uint8_t *const p = F.out + soff + 4u + pre + wbefore + excl;
    *reinterpret_cast<u16_a1 *>(p) = static_cast<uint16_t>((hb << 4 | ref >> 8) | (ref & 255u) << 8);
    const uint32_t rows = len7_of(hb) >> 3;
    for (uint32_t i = 0; i < rows; i++)
        st8(p + 2u + 8u * i, pack_row7(hb, i, my));
}

// ---------------------------------------------------------------------------------------------------- host side

// The encode arena of a context: grown on first use, grow-only; independent of every decode slot.
struct EncState {
    Buf fr, look, tickets, bnb, bref, rh, tot, fail, wlen, wst; // HBM
#ifdef MCRAW_EPOCH0E // test builds (above)
    uint32_t epoch = MCRAW_EPOCH0E;
#else
    uint32_t epoch = 0;
#endif
    hipEvent_t done = nullptr; // behind the last batch's kernels (the next batch, on whatever stream, waits for it)
    std::vector<EncF> hfr;
    std::vector<uint64_t> hlen;
    std::vector<int32_t> hst;
};

void enc_release(EncState *e)
{
    if (!e)
        return;
    for (Buf *b : {&e->fr, &e->look, &e->tickets, &e->bnb, &e->bref, &e->rh, &e->tot, &e->fail, &e->wlen, &e->wst})
        if (b->p)
            (void)hipFree(b->p);
    if (e->done)
        (void)hipEventDestroy(e->done);
    delete e;
}

size_t enc_bound7(int width, int height)
{
    if (width <= 0 || height <= 0)
        return 0;
    const size_t encW = (static_cast<size_t>(width) + 63u) / 64u * 64u, encH = (static_cast<size_t>(height) + 3u) / 4u * 4u;
    const size_t nblk = encW * encH / 64u, nrec = (nblk + 63u) / 64u;
    return 16u + 128u * nblk + 2u * (4u + 130u * nrec);
}

namespace {

// Grow a zero-initialised workspace array (its old contents are not kept: the caller has waited for every earlier batch).  The
// zeros are written on the batch's own stream, in front of its kernels: a context's streams do not wait for the null stream,
// and a hipMemset there may still be queued -- behind another thread's work -- when the kernels run.
int grow_zero(Buf &b, size_t bytes, hipStream_t st, bool *grew)
{
    if (bytes <= b.cap)
        return 0;
    if (b.p)
        HIP_TRY(hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
    const size_t want = up(std::max<size_t>(bytes, 4096), 1 << 16);
    HIP_TRY(hipMalloc(&b.p, want));
    HIP_TRY(hipMemsetAsync(b.p, 0, want, st));
    b.cap = want;
    *grew = true;
    return 0;
}

int encode_device(mcraw_ctx *c, const mcraw_enc_frame *frames, int n, hipStream_t st, size_t *written, int32_t *status)
{
    if (!c->enc)
        c->enc = new EncState();
    EncState &E = *c->enc;
    if (!E.done)
        HIP_TRY(hipEventCreateWithFlags(&E.done, hipEventDisableTiming));
    E.hfr.assign(static_cast<size_t>(n), EncF{});
    uint32_t smax = 0, rmax = 0;
    for (int i = 0; i < n; i++) {
        const mcraw_enc_frame &fr = frames[i];
        EncF &F = E.hfr[static_cast<size_t>(i)];
        F.in = fr.in;
        F.out = fr.out;
        F.len_out = fr.len_out;
        F.w = fr.width;
        F.h = fr.height;
        const bool dims = fr.width > 0 && fr.height > 0 &&
                          static_cast<uint64_t>(fr.width) * static_cast<uint64_t>(fr.height) < (1ull << 31);
        const size_t bound = dims ? enc_bound7(fr.width, fr.height) : 0;
        if (!dims || !fr.in || !fr.out || (reinterpret_cast<uintptr_t>(fr.in) & 1u) || bound >= (1ull << 32)) {
            F.bad = MCRAW_E_ARGS;
            continue;
        }
        if (fr.out_capacity < bound) {
            F.bad = MCRAW_E_CAPACITY;
            continue;
        }
        F.bound = bound;
        F.tilesX = static_cast<uint32_t>((fr.width + 63) / 64);
        F.ntiles = F.tilesX * static_cast<uint32_t>((fr.height + 3) / 4);
        F.nseg = (F.ntiles + SEG_TILES - 1u) / SEG_TILES;
        F.R = (4u * F.ntiles + 63u) / 64u;
        smax = std::max(smax, F.nseg);
        rmax = std::max(rmax, F.R);
    }
    smax = std::max(smax, 1u);
    rmax = std::max(rmax, 1u);
    const size_t nn = static_cast<size_t>(n);
    // every earlier batch of the context (on any stream) is done with the workspace before it is reused or replaced
    const bool big = nn * sizeof(EncF) > E.fr.cap || nn * smax * 8u > E.look.cap || nn * TICKET_STRIDE7E * 4u > E.tickets.cap ||
                     nn * rmax * 64u > E.bnb.cap || nn * rmax * 128u > E.bref.cap || nn * 2u * rmax * 2u > E.rh.cap ||
                     nn * 8u > E.wlen.cap;
    if (big)
        HIP_TRY(hipEventSynchronize(E.done));
    bool grew = false;
    int rc = 0;
    if ((rc = grow_zero(E.fr, nn * sizeof(EncF), st, &grew)) || (rc = grow_zero(E.look, nn * smax * 8u, st, &grew)) ||
        (rc = grow_zero(E.tickets, nn * TICKET_STRIDE7E * 4u, st, &grew)) || (rc = grow_zero(E.bnb, nn * rmax * 64u, st, &grew)) ||
        (rc = grow_zero(E.bref, nn * rmax * 128u, st, &grew)) || (rc = grow_zero(E.rh, nn * 2u * rmax * 2u, st, &grew)) ||
        (rc = grow_zero(E.tot, nn * 4u, st, &grew)) || (rc = grow_zero(E.fail, nn * 4u, st, &grew)) ||
        (rc = grow_zero(E.wlen, nn * 8u, st, &grew)) || (rc = grow_zero(E.wst, nn * 4u, st, &grew)))
        return rc;
    if (++E.epoch == 0u) // (a fresh look-back array holds zeros: epoch 0 never matches)
        E.epoch = 1u;
    HIP_TRY(hipStreamWaitEvent(st, E.done, 0));
    HIP_TRY(hipMemcpyAsync(E.fr.p, E.hfr.data(), nn * sizeof(EncF), hipMemcpyHostToDevice, st));
    EncWork W;
    W.fr = static_cast<const EncF *>(E.fr.p);
    W.look = static_cast<uint64_t *>(E.look.p);
    W.tickets = static_cast<uint32_t *>(E.tickets.p);
    W.bnb = static_cast<uint8_t *>(E.bnb.p);
    W.bref = static_cast<uint16_t *>(E.bref.p);
    W.rh = static_cast<uint16_t *>(E.rh.p);
    W.tot = static_cast<uint32_t *>(E.tot.p);
    W.fail = static_cast<uint32_t *>(E.fail.p);
    W.wlen = static_cast<uint64_t *>(E.wlen.p);
    W.wst = static_cast<int32_t *>(E.wst.p);
    W.n = static_cast<uint32_t>(n);
    W.smax = smax;
    W.rmax = rmax;
    W.epoch = E.epoch;
    {
        KTimer kt(c, MCRAW_K7E_PAYLOAD, st);
        hipLaunchKernelGGL(k7e_payload, dim3(static_cast<uint32_t>(n) * smax), dim3(EB_T), 0, st, W);
    }
    HIP_TRY(hipGetLastError());
    {
        KTimer kt(c, MCRAW_K7E_SIDE, st);
        const uint32_t chunks = (rmax + SIDE_RECS - 1u) / SIDE_RECS;
        hipLaunchKernelGGL(k7e_side, dim3(static_cast<uint32_t>(n) * 2u * chunks), dim3(EB_T), 0, st, W);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(E.done, st));
    if (!written && !status)
        return 0;
    E.hlen.assign(nn, 0);
    E.hst.assign(nn, 0);
    HIP_TRY(hipMemcpyAsync(E.hlen.data(), W.wlen, nn * 8u, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(E.hst.data(), W.wst, nn * 4u, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t i = 0; i < nn; i++) {
        if (written)
            written[i] = static_cast<size_t>(E.hlen[i]);
        if (status)
            status[i] = E.hst[i];
    }
    return 0;
}

// MCRAW_MEM_HOST: upload, encode, download of the written bytes (synchronous, no performance target).
int encode_host(mcraw_ctx *c, const mcraw_enc_frame *frames, int n, size_t *written, int32_t *status)
{
    std::vector<mcraw_enc_frame> dev(frames, frames + n);
    std::vector<void *> bufs;
    struct Free {
        std::vector<void *> &b;
        ~Free() { for (void *p : b) (void)hipFree(p); }
    } guard{bufs};
    std::vector<int32_t> pre(static_cast<size_t>(n), 0);
    for (int i = 0; i < n; i++) {
        const mcraw_enc_frame &fr = frames[i];
        mcraw_enc_frame &d = dev[static_cast<size_t>(i)];
        d.len_out = nullptr;
        const bool dims = fr.width > 0 && fr.height > 0 &&
                          static_cast<uint64_t>(fr.width) * static_cast<uint64_t>(fr.height) < (1ull << 31);
        if (!dims || !fr.in || !fr.out)
            continue; // encode_device reports it
        const size_t bound = enc_bound7(fr.width, fr.height);
        if (fr.out_capacity < bound)
            continue;
        void *din = nullptr, *dout = nullptr;
        const size_t inb = static_cast<size_t>(fr.width) * static_cast<size_t>(fr.height) * 2u;
        HIP_TRY(hipMalloc(&din, inb));
        bufs.push_back(din);
        HIP_TRY(hipMalloc(&dout, bound));
        bufs.push_back(dout);
        HIP_TRY(hipMemcpyAsync(din, fr.in, inb, hipMemcpyHostToDevice, c->stream));
        d.in = static_cast<const uint16_t *>(din);
        d.out = static_cast<uint8_t *>(dout);
        d.out_capacity = bound;
    }
    std::vector<size_t> wr(static_cast<size_t>(n), 0);
    std::vector<int32_t> stv(static_cast<size_t>(n), 0);
    int rc = encode_device(c, dev.data(), n, c->stream, wr.data(), stv.data());
    if (rc)
        return rc;
    for (int i = 0; i < n; i++) {
        const size_t k = static_cast<size_t>(i);
        if (stv[k] == 0 && wr[k] && dev[k].out != frames[i].out)
            HIP_TRY(hipMemcpy(frames[i].out, dev[k].out, wr[k], hipMemcpyDeviceToHost));
        else
            wr[k] = 0;
        if (frames[i].len_out)
            *frames[i].len_out = wr[k];
        if (written)
            written[i] = wr[k];
        if (status)
            status[i] = stv[k];
    }
    return 0;
}

} // namespace

} // namespace mcraw

using namespace mcraw;

#ifdef MCRAW_PATHSE
// The census, in the order of PathE (up to n counters; returns how many there are); `reset`: and start it over.
extern "C" int mcraw_diag_k7e_paths(uint64_t *out, int n, int reset) { return census_read<PE_N>(g_k7e_paths, out, n, reset); }
#endif

extern "C" {

size_t mcraw_encode_bound7(int width, int height) { return enc_bound7(width, height); }

int mcraw_encode_batch(mcraw_ctx *c, const mcraw_enc_frame *frames, int nframes, int mem, void *stream, size_t *written,
                       int32_t *status)
{
    if (!c || (!frames && nframes > 0) || nframes < 0 || static_cast<uint64_t>(nframes) > (1u << 20)) {
        g_err = "mcraw_encode_batch: bad arguments";
        return -1;
    }
    if (nframes == 0)
        return 0;
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    if (mem == MCRAW_MEM_DEVICE)
        return encode_device(c, frames, nframes, stream ? static_cast<hipStream_t>(stream) : c->stream, written, status);
    if (mem == MCRAW_MEM_HOST)
        return encode_host(c, frames, nframes, written, status);
    g_err = "mcraw_encode_batch: unknown memory kind";
    return -1;
}

} // extern "C"
