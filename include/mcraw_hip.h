/*
 * mcraw_hip.h -- C ABI of the MI355X (gfx950) MCRAW frame-decode path.
 *
 * This is the drop-in boundary: the entry points a maintainer of
 * mirsadm/motioncam-decoder binds instead of the CPU codec.  Plain pointers
 * and sizes only; no C++ or torch types.  INTEGRATION.md shows the
 * reference-side change (lib/Decoder.cpp:224-231).
 *
 * There is NO CPU fallback behind these symbols: without a HIP device every
 * entry point fails (returns 0 / a negative status).
 */
#ifndef MCRAW_HIP_H
#define MCRAW_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCRAW_TYPE_LEGACY 6 /* lib/Decoder.cpp:20 MOTIONCAM_COMPRESSION_TYPE_LEGACY */
#define MCRAW_TYPE_BLOCK  7 /* lib/Decoder.cpp:21 MOTIONCAM_COMPRESSION_TYPE        */

/* Per-frame status bits reported by mcraw_decode_batch (0 = decoded). */
#define MCRAW_OK            0
#define MCRAW_E_ARGS        0x0001 /* bad width/height/type/pointer                      */
#define MCRAW_E_HEADER      0x0002 /* offsets > len, encodedWidth%64, encodedWidth<width */
                                   /*   (reference returns 0: lib/RawData.cpp:547-554)   */
#define MCRAW_E_TRUNCATED   0x0004 /* a block or record crosses `len` (the reference     */
                                   /*   skips it and leaves stale samples, :419-420)     */
#define MCRAW_E_SIDESTREAM  0x0008 /* side-stream entry count < blocks, or bits > 16     */
#define MCRAW_E_CAPACITY    0x0010 /* out_capacity < width * rows                        */
#define MCRAW_E_DEVICE      0x0100 /* HIP runtime error                                  */

/* Where the `in` / `out` pointers of a batch live. */
#define MCRAW_MEM_DEVICE 0 /* HBM of the context's device: no copies, decode only      */
#define MCRAW_MEM_HOST   1 /* host memory: staged H2D / D2H on the context's streams,   */
                           /*   copies of one sub-batch overlap decode of the previous  */

typedef struct mcraw_ctx mcraw_ctx;

/* One frame of a batch.  Mirrors the arguments of motioncam::raw::Decode /
 * DecodeLegacy (lib/include/motioncam/RawData.hpp:25-37) plus the explicit
 * output capacity the reference lacks. */
typedef struct mcraw_frame {
    const uint8_t *in;   /* compressed frame buffer (BUFFER item payload), any      */
                         /*   byte alignment -- e.g. a payload inside a .mcraw file */
                         /*   image resident in HBM; with MCRAW_MEM_DEVICE up to 3  */
                         /*   bytes behind in + len may be read (never used)        */
    size_t len;          /* its length in bytes                                    */
    int32_t width;       /* frame JSON "width"   (lib/Decoder.cpp:216)             */
    int32_t height;      /* frame JSON "height"  (lib/Decoder.cpp:217)             */
    int32_t type;        /* frame JSON "compressionType": 6 or 7 (:218)            */
    int32_t reserved;
    uint16_t *out;       /* row-major uint16 LE mosaic, width * height             */
    size_t out_capacity; /* in uint16 elements                                     */
} mcraw_frame;

/* ---- context ------------------------------------------------------------ */

/* Create a decode context on HIP device `device` (-1: env MCRAW_DEVICE, else
 * the current device).  Returns 0 or a negative hipError. */
int mcraw_ctx_create(int device, mcraw_ctx **ctx);
void mcraw_ctx_destroy(mcraw_ctx *ctx);
const char *mcraw_last_error(void);

/* ---- drop-in single-frame entry points ---------------------------------- */

/* Replace motioncam::raw::Decode (lib/RawData.cpp:528-612) and
 * motioncam::raw::DecodeLegacy (lib/RawData_Legacy.cpp:445-495): same five
 * arguments, same return convention (uint16 elements written, 0 = failure).
 * Host pointers; `output` must hold width*height elements.  They run on a
 * process-wide default context (device: MCRAW_DEVICE or 0). */
size_t mcraw_decode7(uint16_t *output, int width, int height, const uint8_t *input, size_t len);
size_t mcraw_decode6(uint16_t *output, int width, int height, const uint8_t *input, size_t len);

/* ---- batched entry point (replaces the per-frame loop, lib/Decoder.cpp:184-235,
 *      example.cpp:187-195) ------------------------------------------------ */

/* Decode `nframes` independent frames.  `mem` says where in/out live.
 * `stream` is a hipStream_t (NULL = the context's own stream); with
 * MCRAW_MEM_DEVICE all work is enqueued on it and the call returns without
 * synchronising unless `written`/`status` are requested:
 *   written[i] : uint16 elements produced for frame i (0 on failure), or NULL
 *   status[i]  : MCRAW_* bits for frame i, or NULL
 * Passing either forces a stream synchronisation before returning.
 * Returns 0, or a negative value when the batch could not be submitted. */
int mcraw_decode_batch(mcraw_ctx *ctx, const mcraw_frame *frames, int nframes, int mem,
                       void *stream, size_t *written, int32_t *status);

/* Asynchronous host-memory batches (MCRAW_MEM_HOST semantics; buffers should be pinned): the call
 * returns when the batch is queued, so the next one can be submitted while this one is still moving
 * over PCIe -- the upload / kernel / download lanes then run back to back ACROSS batches, which a
 * sequence of synchronous mcraw_decode_batch calls cannot do.  `frames` is copied; the in / out buffers
 * must stay valid until mcraw_ticket_wait has returned for the ticket.  mcraw_ticket_wait blocks for that
 * batch only, fills `written` / `status` (either may be NULL) and releases the ticket.  Wait for every
 * ticket before mcraw_ctx_destroy.  Returns 0 or a negative value.
 * Scheduling: the copy lanes run best with two batches of a few hundred MB under way (about 3 000 UHD frames/s
 * host to host).  The library keeps to that by itself -- a third ticket's submission waits for the oldest one's
 * downloads (not for its mcraw_ticket_wait), and a batch of more than 384 MB is dealt out in such pieces inside the
 * call, which then returns when the last piece is queued -- so neither the size of a batch nor the number of tickets
 * a caller keeps in flight (two is enough) has to be tuned.  How the per-frame statuses travel (written home behind the
 * kernels, or fetched at the wait) is measured by every context on its first batches, because the better way depends on
 * what the process did with the GPU before the context existed; MCRAW_SHORT_WAY=0|1 in the environment decides it
 * beforehand (1: written home), MCRAW_TRACE=1 prints what was measured. */
typedef struct mcraw_ticket mcraw_ticket;
int mcraw_decode_batch_async(mcraw_ctx *ctx, const mcraw_frame *frames, int nframes, mcraw_ticket **ticket);
int mcraw_ticket_wait(mcraw_ticket *ticket, size_t *written, int32_t *status);

/* Wait for everything submitted on the context; fetch the statuses of the
 * last batch (status may be NULL).  Returns 0 or negative. */
int mcraw_ctx_synchronize(mcraw_ctx *ctx, int32_t *status, int nframes);
/* Device-memory batches submitted WITHOUT a status request, several in a row (the reference's loop, example.cpp:187-195, run as
 * batches that follow each other on the GPU): every device-memory batch of a context has a serial number (the last one
 * submitted: mcraw_ctx_last_serial); mcraw_ctx_batch_status waits for that batch and returns its statuses (0; 1 when the
 * serial is not one of the last 64 such batches); mcraw_ctx_errors returns the OR of the statuses of all frames of such
 * batches whose statuses became known since the last call with `reset` (mcraw_ctx_synchronize makes all of them known). */
uint64_t mcraw_ctx_last_serial(mcraw_ctx *ctx);
int mcraw_ctx_batch_status(mcraw_ctx *ctx, uint64_t serial, int32_t *status, int nframes);
int32_t mcraw_ctx_errors(mcraw_ctx *ctx, int reset);

/* ---- encoder: uint16 mosaics -> type-7 frame buffers ---------------------
 *
 * The bytes are exactly those of the project's canonical type-7 writer (the
 * test synthesiser's mcraw_synth_encode7 with no forced classes and flags 0):
 * 16-byte header {encW, encH, bits offset, refs offset}, the payload blocks in
 * tile order at their natural class, then the bits stream and the refs stream
 * (entry counts rounded up to 64, padded entries 0).  No CPU fallback: without
 * a device these calls fail. */
typedef struct mcraw_enc_frame {
    const uint16_t *in;  /* row-major mosaic, width*height uint16, 2-byte aligned          */
    int32_t width, height;
    uint8_t *out;        /* any byte alignment                                             */
    size_t out_capacity; /* bytes; must be >= mcraw_encode_bound7(width, height)            */
    uint64_t *len_out;   /* optional, same memory space as out: bytes written, stream order */
} mcraw_enc_frame;
/* Exact worst case of an encoded frame: 16 + 128 nblk + 2 (4 + 130 ceil(nblk / 64)) with
 * nblk = ceil64(width) * ceil4(height) / 64.  Host only, no device needed; 0 for width or height < 1. */
size_t mcraw_encode_bound7(int width, int height);
/* Encode `nframes` mosaics; the conventions of mcraw_decode_batch: with MCRAW_MEM_DEVICE the work is
 * enqueued on `stream` (NULL: the context's stream) and the call synchronises only when `written` or
 * `status` is requested (len_out gives the sizes in stream order without a synchronisation);
 * MCRAW_MEM_HOST uploads, encodes and downloads the written bytes before it returns.
 *   written[i] : bytes written for frame i (0 on failure), or NULL
 *   status[i]  : MCRAW_E_ARGS (width or height < 1, width*height >= 2^31, a bound >= 2^32, a NULL or odd
 *                pointer), MCRAW_E_CAPACITY (out_capacity below the bound: nothing is written),
 *                MCRAW_E_DEVICE, or 0
 * Encode batches do not touch the decode side's state: they take no serial number and leave
 * mcraw_ctx_last_serial / mcraw_ctx_batch_status / mcraw_ctx_errors as they are.
 * Returns 0, or a negative value when the batch could not be submitted. */
int mcraw_encode_batch(mcraw_ctx *ctx, const mcraw_enc_frame *frames, int nframes, int mem, void *stream,
                       size_t *written, int32_t *status);
/* Single frame, host pointers, on the process-wide default context (beside mcraw_decode7): returns the
 * bytes written, or 0 on failure. */
size_t mcraw_encode7(uint8_t *output, size_t capacity, const uint16_t *input, int width, int height);
/* ---- several GPUs of one node (device pool) --------------------------------------------------
 *
 * The reference walks a clip frame by frame on one thread (example.cpp:187-195 over
 * lib/Decoder.cpp:184-235).  Frames are independent, so a batch shards by frame index: frame i is
 * decoded by pool member i mod G -- no exchange between devices.  Every member is a context of its
 * own, driven by one host thread of its own that is bound to the CPUs of its GPU's NUMA node (those of them the
 * process may run on).  Results do not depend on the pool size.  Buffers are host memory (MCRAW_MEM_HOST semantics)
 * except for mcraw_pool_decode_batch_device. */
typedef struct mcraw_pool mcraw_pool;
typedef struct mcraw_pool_ticket mcraw_pool_ticket;
struct mcraw_post;
struct mcraw_float_out;

/* The partition rule, usable without a GPU: which member decodes frame `index` (index mod ndevices;
 * -1 on bad arguments), and how many of `nframes` frames member `member` gets. */
int mcraw_shard_of(long index, int ndevices);
int mcraw_shard_count(long nframes, int member, int ndevices);

/* devices[0..ndevices): HIP device indices.  ndevices == 0: env MCRAW_DEVICES ("all" or "0,1,5"),
 * else one member on MCRAW_DEVICE / the current device.  Returns 0 or a negative value. */
int mcraw_pool_create(const int *devices, int ndevices, mcraw_pool **pool);
void mcraw_pool_destroy(mcraw_pool *pool);
const char *mcraw_pool_last_error(void);
int mcraw_pool_size(const mcraw_pool *pool);
int mcraw_pool_device(const mcraw_pool *pool, int member);    /* its HIP device index */
int mcraw_pool_numa_cpus(const mcraw_pool *pool, int member); /* CPUs its host thread is bound to (0: not bound) */
mcraw_ctx *mcraw_pool_ctx(mcraw_pool *pool, int member);      /* for the measurement calls below */
int mcraw_pool_set_post(mcraw_pool *pool, const struct mcraw_post *post);
int mcraw_pool_set_float_out(mcraw_pool *pool, const struct mcraw_float_out *f); /* every member: mcraw_ctx_set_float_out */
/* Pinned host memory allocated by the member's own (NUMA-bound) thread: local to its GPU.  Free with mcraw_host_free. */
void *mcraw_pool_host_alloc(mcraw_pool *pool, int member, size_t bytes);
/* One batch over all members; the asynchronous form returns when every member has queued its share.
 * The pool may be used from several host threads at once (batches are dealt one at a time, every member runs its tasks
 * in the order they were handed to it); a ticket is waited for by one thread. */
int mcraw_pool_decode_batch(mcraw_pool *pool, const mcraw_frame *frames, int nframes, size_t *written, int32_t *status);
/* The same for buffers that are already resident: frames[i].in / .out are device pointers in the HBM of the GPU that
 * decodes frame i, mcraw_pool_device(pool, i % mcraw_pool_size(pool)) -- BASELINE config 5's form (a clip sharded over
 * the node's GPUs by frame index; lib/Decoder.cpp:184-235 run as one batch).  With `written` or `status` it returns when
 * every member's share is decoded.  Where a frame's buffers live is CHECKED (hipPointerGetAttributes): a frame whose `in`
 * or `out` is not device memory of the GPU that decodes it gets MCRAW_E_ARGS and is not decoded -- it would be decoded
 * over xGMI at a fraction of the rate, or fault. */
int mcraw_pool_decode_batch_device(mcraw_pool *pool, const mcraw_frame *frames, int nframes, size_t *written, int32_t *status);
/* With `written` and `status` both NULL the call above only queues every member's share (each on its context's own stream)
 * and returns; several batches in a row then run back to back on every GPU.  mcraw_pool_synchronize waits for everything
 * the members have queued and fetches the statuses of the CALLING THREAD's last such batch (status may be NULL) -- the pool
 * may be used from several host threads at once, each sees its own.  It returns a negative value for a runtime failure, else
 * the OR of the statuses of all frames of all queued batches (of any thread) whose outcome became known since the last
 * call: 0 = every frame of every queued batch decoded. */
int mcraw_pool_synchronize(mcraw_pool *pool, int32_t *status, int nframes);
int mcraw_pool_decode_batch_async(mcraw_pool *pool, const mcraw_frame *frames, int nframes, mcraw_pool_ticket **ticket);
int mcraw_pool_ticket_wait(mcraw_pool_ticket *ticket, size_t *written, int32_t *status);

/* The order in which the legacy kernel's workgroups take the segments (16 KiB of stream each) of a batch's legacy frames,
 * as the library builds it for every batch; exported so that the rule can be checked without a GPU.  `nseg[n]`: segments per
 * frame.  The launch goes round by round -- round r = segment r of every frame that has one --, the frames by falling
 * number of segments; stage t = the rounds in which all but the t smallest frames are in play.  `tab` receives 3 n + 1
 * words: [0, n]: first workgroup of every stage (tab[n] = workgroups in all = segments of all frames); [n + 1, 2n]: first
 * round of every stage; [2n + 1, 3n]: the frames in that order.  Workgroup b of stage t works on frame
 * tab[2n + 1 + (b - tab[t]) % (n - t)] and is given -- if workgroups start in order -- segment
 * tab[n + 1 + t] + (b - tab[t]) / (n - t). */
void mcraw_legacy_launch_order(const uint32_t *nseg, int n, uint32_t *tab);

/* The order the tile kernel's workgroups take their work in: block `b` of a grid of `n` blocks works on logical workgroup
 * mcraw_tile_order(b, n, runs) -- runs of `runs` consecutive workgroups per XCD (0: the grid in eight parts; see
 * mcraw_ctx_xcd_runs).  A permutation of 0..n-1 for every n and runs; exported so that this can be checked without a GPU. */
uint32_t mcraw_tile_order(uint32_t b, uint32_t n, uint32_t runs);

/* ---- measurement -------------------------------------------------------- */

/* Kernel ids for mcraw_ctx_kernel_ms. */
#define MCRAW_K7_SIDE    0 /* side streams: chain, records, payload offsets (one launch) */
                           /* ids 1 and 2 are retired (former separate chain kernels)  */
#define MCRAW_K7_TILES   3 /* tile decode (the roofline kernel)   */
                           /* ids 4 and 5 are retired (former legacy map / resolve kernels) */
#define MCRAW_K6_DECODE  6 /* legacy: the whole decode (one launch) */
#define MCRAW_K7E_PAYLOAD 7 /* encoder: payload of every frame (mcraw_encode_batch) */
#define MCRAW_K7E_SIDE   8 /* encoder: side streams, header, byte count           */
#define MCRAW_KRGB_MHC   9 /* demosaic, full resolution (mcraw_demosaic_batch)     */
#define MCRAW_KRGB_BIN2 10 /* demosaic, 2x2 binning                                */
#define MCRAW_K_COUNT   11

/* hipEvent bracketing of kernel launches on the launch stream: 0 = off, 1 = every
 * kernel, MCRAW_PROFILE_ONLY(id) [| MCRAW_PROFILE_ONLY(id2) ...] = those kernels only
 * (each bracket costs two event records in the stream).  mcraw_ctx_kernel_ms returns,
 * for kernel `id`, the summed duration (ms) and launch count since the last reset
 * (synchronises). */
#define MCRAW_PROFILE_ONLY(id) (2 << (id))
int mcraw_ctx_profile(mcraw_ctx *ctx, int enable);
/* Bracket only every n-th launch of a profiled kernel (n >= 1; default 1): an event pair costs the stream
 * several microseconds, a sample of the launches gives the same average duration. */
int mcraw_ctx_profile_every(mcraw_ctx *ctx, int n);
int mcraw_ctx_kernel_ms(mcraw_ctx *ctx, int id, double *ms, int *launches, int reset);
/* How the tile kernel's workgroups are dealt to the GPU's eight XCDs for large resident batches: the library measures two
 * mappings on the first launches of a geometry (frames per batch, groups per frame) -- which one is faster depends on where
 * the caller's buffers lie in physical memory --, keeps the faster, and times one launch in 64 afterwards (the chosen mapping
 * and the other one in turn) so that the choice follows the caller's buffers; a caller that never reuses a buffer is not kept
 * measuring.  Returns the choice for the geometry of the last such batch: the length of the runs in workgroups (0: the grid
 * in eight parts), -1 while the first measurements are under way or nothing was measured (small or host-memory batches use
 * runs of 128).  Environment MCRAW_XCD_CHUNK pins the mapping (then always -1 here). */
int mcraw_ctx_xcd_runs(mcraw_ctx *ctx);
/* How many workgroups resolve each side stream of the frames of large-frame resident batches (lib/RawData.cpp:463-498 is one chain
 * per stream; which of a frame's two streams is the slow one depends on its content): chosen by measurement on the first launches
 * of a geometry, re-checked by one timed launch in 64.  Returns 16 * (parts of the bits stream) + (parts of the refs stream) for
 * the geometry of the last such batch, -1 while measuring or when nothing was measured. */
int mcraw_ctx_side_parts(mcraw_ctx *ctx);
/* Host-memory batches (MCRAW_MEM_HOST): how the status words of a large batch come home -- 0: fetched when the batch is waited
 * for, 1: written into pinned memory behind the kernels, -1: the context is still comparing the two on its own batches (which is
 * faster depends on what else the process has done with the GPU; MCRAW_SHORT_WAY decides beforehand). */
int mcraw_ctx_host_way(mcraw_ctx *ctx);

/* Optional stage fused behind the decode, for consumers that take the mosaic further on the
 * device or ship it as a DNG strip (what example.cpp:80-92 hands to the DNG writer: the raw strip,
 * BlackLevel, BitsPerSample).  It applies to every batch submitted on `ctx` after the call;
 * NULL (or flags 0) restores the reference's output, the plain uint16 mosaic.
 *   MCRAW_POST_BLACK   sample = max(sample - black[(row & 1) * 2 + (col & 1)], 0)   (after the decode)
 *   MCRAW_POST_PACK12  rows are written as 12-bit strips: ceil(width * 12 / 8) bytes per row, rows
 *                      back to back, samples MSB-first, 3 bytes per 2 samples (TIFF / DNG
 *                      BitsPerSample = 12, FillOrder 1); samples above 4095 saturate.  `out` must be
 *                      2-byte aligned (4-byte aligned and width % 8 == 0 for the vector-store path);
 *                      `out_capacity` still counts uint16 units (2 bytes) of the buffer and `written`
 *                      still counts samples. */
#define MCRAW_POST_BLACK  1u
#define MCRAW_POST_PACK12 2u
/* The same strip form at 10 or 14 bits per sample (5 bytes per 4 samples / 7 bytes per 4 samples; samples above
 * 1023 / 16383 saturate): pick the width from the container's whiteLevel, so that 10-bit footage crosses the
 * host link at 1.25 bytes per sample.  At most one of the three PACK flags.  `out` 2-byte aligned. */
#define MCRAW_POST_PACK10 4u
#define MCRAW_POST_PACK14 8u
typedef struct mcraw_post {
    uint32_t flags;
    uint16_t black[4];
} mcraw_post;
int mcraw_ctx_set_post(mcraw_ctx *ctx, const mcraw_post *post);

/* The other kind of fused stage: normalised float samples, for a model's input (raw denoising, raw-to-RGB networks).
 * A context has ONE stage: mcraw_ctx_set_float_out replaces any mcraw_ctx_set_post stage, and mcraw_ctx_set_post (NULL
 * included) replaces a float stage.  It applies to every batch submitted afterwards, in every mode (device and host
 * memory, tickets, pools, mixed type-6 / type-7 batches); NULL restores the plain uint16 mosaic.  Per sample, at CFA
 * position p = (row & 1) * 2 + (col & 1), bit-exact:
 *   inv[p] = 1.0f / (white - (float)black[p])                  (host, IEEE f32 division)
 *   v      = (float)((int)sample - (int)black[p]) * inv[p]      (the difference is exact; one f32 multiply, RNE; no FMA)
 *   v      = CLIP ? min(max(v, 0.0f), 1.0f) : v                 (negatives are kept without CLIP)
 *   out    = v as f32, or rounded to nearest even into f16 (overflow: +inf) / bf16
 * Layouts: MCRAW_LAYOUT_MOSAIC = width x height row-major, like the uint16 output (any width); MCRAW_LAYOUT_PLANES = four
 * planes of (height/2) x (width/2), plane-major, position (r, c) to plane plane[p], row r/2, column c/2 (width and height
 * must be even, else the frame gets MCRAW_E_ARGS and nothing is written).  `out_capacity` still counts uint16 units (2
 * bytes): f32 needs 2 * width * height, f16 / bf16 width * height (mosaic rows: as far as the rows are written); less gives
 * MCRAW_E_CAPACITY and nothing is written.  `written` counts samples.  `out` must be 2-byte aligned (f16 / bf16) or
 * 4-byte aligned (f32: else MCRAW_E_ARGS); the vector-store path takes 16-byte aligned outputs (8-byte for f16 / bf16
 * planes) and width % 8 == 0.  Rows the frame header does not provide are left untouched.
 * Rejected (returns < 0, mcraw_last_error says why): an unknown dtype, layout or flag; white <= black[p] for some p;
 * a white that is not finite; a plane map that is not a permutation of 0..3. */
#define MCRAW_FLOAT_F32     1
#define MCRAW_FLOAT_F16     2
#define MCRAW_FLOAT_BF16    3
#define MCRAW_LAYOUT_MOSAIC 0  /* width x height, row-major, like the uint16 output            */
#define MCRAW_LAYOUT_PLANES 1  /* 4 planes of (height/2) x (width/2), plane-major               */
#define MCRAW_FLOAT_CLIP    1u /* flags: clamp to [0, 1] after normalising                      */
typedef struct mcraw_float_out {
    uint32_t dtype;    /* MCRAW_FLOAT_*                                                        */
    uint32_t layout;   /* MCRAW_LAYOUT_*                                                       */
    uint32_t flags;    /* MCRAW_FLOAT_CLIP or 0                                                */
    uint16_t black[4]; /* by CFA position p = (row & 1) * 2 + (col & 1), as mcraw_post         */
    float white;       /* container "whiteLevel"; must be > every black[p]                     */
    uint8_t plane[4];  /* PLANES: output plane of CFA position p; a permutation of 0..3         */
} mcraw_float_out;
int mcraw_ctx_set_float_out(mcraw_ctx *ctx, const mcraw_float_out *f);

/* ---- uint16 mosaics -> planar linear RGB ------------------------------------------------------------------------
 *
 * Demosaics `n` uint16 mosaics that are resident in HBM into (n, 3, Ho, Wo) planar RGB at `out`: contiguous, frames back to
 * back, channel-major per frame (R, G, B planes), row-major planes.  `in_pitch` and `in_frame_stride` count uint16 elements.
 *   MCRAW_RGB_MHC   Ho = height, Wo = width: Malvar-He-Cutler 5x5 gradient-corrected bilinear interpolation
 *   MCRAW_RGB_BIN2  Ho = height / 2, Wo = width / 2: one output pixel per 2x2 CFA quad, R = r, G = mean(g1, g2), B = b
 * Bit-exact arithmetic, at CFA position p = (y & 1) * 2 + (x & 1):
 *   d(y, x) = (int)s(y, x) - (int)black[p]   (int32; MHC reads outside the frame are reflected 101-style: -k -> k,
 *                                             H-1+k -> H-1-k, the same for columns, which keeps the CFA parity)
 *   integer estimates E_c, in units of 1/16 (MHC) or 1/2 (BIN2), C = d at the pixel:
 *     MHC native channel            16 C
 *     G at R or B                   8 C + 4 (4 axial neighbours at distance 1) - 2 (4 axial at distance 2)
 *     R or B at G, colour left/right  10 C + 8 (d[y][x-1] + d[y][x+1]) - 2 (d[y][x-2] + d[y][x+2]) - 2 (4 diagonals)
 *                                   + (d[y-2][x] + d[y+2][x]);  colour above/below: the transpose
 *     R at B, B at R                12 C + 4 (4 diagonals) - 3 (4 axial at distance 2)
 *     BIN2                          E_R = 2 d(r), E_G = d(g1) + d(g2), E_B = 2 d(b)
 *   (|E_c| <= 28 * 65535 < 2^24: (float)E_c is exact)
 *   host, f32: inv = 1.0f / (white - 0.25f * (float)(black[0] + black[1] + black[2] + black[3]));
 *              k[c] = (gain[c] * inv) * (MHC ? 0.0625f : 0.5f)
 *   device, f32, every product and sum rounded on its own (no FMA):
 *              v_c = (float)E_c * k[c];  o_i = (m[3i] v_0 + m[3i+1] v_1) + m[3i+2] v_2
 *   o_i clamped to [0, 1] with MCRAW_FLOAT_CLIP, then stored as f32, f16 (RNE, overflow to inf) or bf16 (RNE), as
 *   mcraw_ctx_set_float_out does.
 * `colors` is host memory: ncolors == 1 applies to every frame, ncolors == n gives one per frame.  The values travel with
 * the launches, so batches queued back to back (on one stream or several) never see each other's colours.
 * `stream`: a hipStream_t, NULL = the context's own stream; the call queues the work and returns without synchronising.
 * It takes no decode serial and leaves the decode slots, mcraw_ctx_errors, mcraw_ctx_last_serial and the context's
 * stage (set_post / set_float_out) alone.  n == 0 is a no-op.
 * Rejected (returns < 0, mcraw_last_error says why, nothing is written): an odd width or height, or one below 4 or above
 * 65536; in_pitch < width; n > 1 and in_frame_stride < (height - 1) * in_pitch + width; an unknown algo, dtype, cfa or
 * flag; a white that is not finite or not above 0.25 * (sum of black); a non-finite gain or matrix entry; ncolors not 1
 * or n; out_bytes < n * 3 * Ho * Wo * element size; a NULL or odd `in`; a NULL `out` or one not aligned to the element
 * size.  Kernels: MCRAW_KRGB_MHC / MCRAW_KRGB_BIN2 (mcraw_ctx_kernel_ms). */
#define MCRAW_RGB_MHC  1
#define MCRAW_RGB_BIN2 2
#define MCRAW_CFA_RGGB 0
#define MCRAW_CFA_BGGR 1
#define MCRAW_CFA_GRBG 2
#define MCRAW_CFA_GBRG 3
typedef struct mcraw_rgb {
    uint32_t algo;     /* MCRAW_RGB_MHC, MCRAW_RGB_BIN2 or MCRAW_RGB_HA (below)               */
    uint32_t dtype;    /* MCRAW_FLOAT_F32 / _F16 / _BF16                                      */
    uint32_t flags;    /* MCRAW_FLOAT_CLIP or 0                                               */
    uint32_t cfa;      /* MCRAW_CFA_* (the container's sensorArrangment)                      */
    uint16_t black[4]; /* by CFA position p = (y & 1) * 2 + (x & 1)                           */
    float white;       /* container "whiteLevel"                                              */
} mcraw_rgb;
typedef struct mcraw_rgb_color {
    float gain[3]; /* white balance, R G B (1 / asShotNeutral)                                */
    float m[9];    /* row-major 3x3, out = m . v                                              */
} mcraw_rgb_color;
int mcraw_demosaic_batch(mcraw_ctx *ctx, const mcraw_rgb *p, const mcraw_rgb_color *colors, int ncolors,
                         const uint16_t *in, size_t in_pitch, size_t in_frame_stride, int width, int height, int n,
                         void *out, size_t out_bytes, void *stream);

/* ---- uint16 mosaics -> display-ready uint8 / uint16 RGB through a transfer-curve LUT ------------------------------
 *
 * The demosaic and colour arithmetic of mcraw_demosaic_batch, bit for bit, up to o_i; then, per output sample (f32, no FMA):
 *   c   = (o_i > 0.0f) ? fminf(o_i, 1.0f) : 0.0f      always clamped; NaN -> 0
 *   i   = (uint32_t) rintf(c * (float)(L - 1))        one f32 multiply (RNE), round half to even; 0 <= i <= L - 1
 *   out = U8 ? (uint8_t)(lut[i] & 0xFF) : lut[i]
 * Layouts: MCRAW_DISP_CHW = (n, 3, Ho, Wo) as mcraw_demosaic_batch; MCRAW_DISP_HWC = (n, Ho, Wo, 3), interleaved R G B.
 * `p->dtype` and `p->flags` must be 0 (`d` decides the output type; the clamp is unconditional); everything else in `p`
 * and `colors` means what it means for mcraw_demosaic_batch, whose argument rules hold here as well.
 * The LUT (L = 1 << lut_log2 uint16 entries) is the caller's DEVICE memory, read by the queued kernels in stream order and
 * never copied into or cached by the context: two calls with the same pointer and new contents in between each see their
 * own.  The call takes no decode serial and leaves the decode slots, mcraw_ctx_errors and the context's stage alone.
 * Rejected besides (returns < 0, mcraw_last_error says why, nothing is written): a NULL `d`; a NULL or not 16-byte aligned
 * `lut`; lut_log2 outside 8 .. 16; an unknown dtype or layout; a non-zero `reserved`; a non-zero p->dtype or p->flags;
 * out_bytes < n * 3 * Ho * Wo * (1 or 2); an `out` not aligned to its element size.
 * Kernels: MCRAW_KRGB_MHC / MCRAW_KRGB_BIN2 (mcraw_ctx_kernel_ms). */
#define MCRAW_DISP_U8   1
#define MCRAW_DISP_U16  2
#define MCRAW_DISP_CHW  0   /* (n, 3, Ho, Wo), as mcraw_demosaic_batch            */
#define MCRAW_DISP_HWC  1   /* (n, Ho, Wo, 3), interleaved R G B                   */
typedef struct mcraw_display {
    uint32_t dtype;        /* MCRAW_DISP_U8 / MCRAW_DISP_U16                        */
    uint32_t layout;       /* MCRAW_DISP_CHW / MCRAW_DISP_HWC                       */
    uint32_t lut_log2;     /* 8 .. 16: the LUT has L = 1 << lut_log2 entries        */
    uint32_t reserved;     /* must be 0                                             */
    const uint16_t *lut;   /* DEVICE memory, 16-byte aligned, read in stream order  */
} mcraw_display;           /* sizeof 24, lut at offset 16                           */
int mcraw_demosaic_display_batch(mcraw_ctx *ctx, const mcraw_rgb *p, const mcraw_display *d,
                                 const mcraw_rgb_color *colors, int ncolors, const uint16_t *in, size_t in_pitch,
                                 size_t in_frame_stride, int width, int height, int n, void *out, size_t out_bytes,
                                 void *stream);

/* ---- uint16 mosaics -> video-ready Y'CbCr 4:2:0: NV12 (8 bit) / P010 (10 bit) --------------------------------------
 *
 * Everything up to the LUT lookup is mcraw_demosaic_display_batch, bit for bit: the integer estimates, the colour stage,
 * the clamp, i = rint(c * (L - 1)) and the LUT rules (the caller's DEVICE memory, 16-byte aligned, L = 1 << lut_log2 uint16
 * entries, read in stream order, never copied or cached).  Then, in integers (int32 sums, `>>` arithmetic: floor):
 *   P_c = lut[i_c] & ((1 << in_bits) - 1)                                   c = R', G', B'
 *   Y   = clamp(((cy . P + (1 << (sh - 1))) >> sh) + y_off, 0, top)         per output pixel; top = 2^bits - 1
 *   S_c = sum of P_c over the 2x2 block of output pixels (rows 2j, 2j + 1; columns 2k, 2k + 1)
 *   Cb  = clamp(((cb . S + (1 << (sh + 1))) >> (sh + 2)) + c_off, 0, top)   per 2x2 block
 *   Cr  = clamp(((cr . S + (1 << (sh + 1))) >> (sh + 2)) + c_off, 0, top)
 * The box average puts the chroma sample at the centre of its 2x2 block (JPEG / MPEG-1 siting), not on the left column.
 * Formats: MCRAW_YUV_NV12: bits = 8, uint8 samples; MCRAW_YUV_P010: bits = 10, uint16 samples holding code << 6.
 * Output per frame, frames back to back: the Y plane, Ho x Wo samples, row-major; directly behind it Ho / 2 rows of Wo / 2
 * interleaved (Cb, Cr) pairs: Ho * Wo * 3 / 2 samples, what `-f rawvideo -pix_fmt nv12` / `p010le` reads.  Ho, Wo as for
 * mcraw_demosaic_batch.  `p`, `colors`, `in` follow mcraw_demosaic_display_batch's rules (p->dtype and p->flags 0).
 * Rejected besides (returns < 0, mcraw_last_error says why, nothing is written): a NULL `y`; an unknown format; a non-zero
 * `reserved`; a NULL or not 16-byte aligned `lut`; lut_log2 outside 8 .. 16; in_bits outside 8 .. 16; sh outside 1 .. 24;
 * y_off or c_off outside 0 .. top; an odd Ho or Wo (BIN2: a width or height that is no multiple of 4); out_bytes <
 * n * Ho * Wo * 3 / 2 * sample size; an `out` not aligned to the sample size; and, for any of cy, cb, cr,
 *   4 * (2^in_bits - 1) * (|c0| + |c1| + |c2|) + 2^(sh + 1) >= 2^31.
 * With that rule and the mask on P_c no LUT content can make an int32 sum wrap.
 * The call queues on `stream` and returns; it takes no decode serial and leaves the decode slots, mcraw_ctx_errors and the
 * context's stage alone.  n == 0 is a no-op.  Kernels: MCRAW_KRGB_MHC / MCRAW_KRGB_BIN2 (mcraw_ctx_kernel_ms). */
#define MCRAW_YUV_NV12  1
#define MCRAW_YUV_P010  2
typedef struct mcraw_yuv {
    uint32_t format;       /* MCRAW_YUV_NV12 / MCRAW_YUV_P010                       */
    uint32_t lut_log2;     /* 8 .. 16: the LUT has L = 1 << lut_log2 entries        */
    uint32_t in_bits;      /* 8 .. 16: bits of a LUT entry that are used            */
    uint32_t sh;           /* 1 .. 24: binary point of the coefficients             */
    int32_t y_off, c_off;  /* 0 .. top                                              */
    int32_t cy[3], cb[3], cr[3]; /* rows of the matrix, times 2^sh                  */
    uint32_t reserved;     /* must be 0                                             */
    const uint16_t *lut;   /* DEVICE memory, 16-byte aligned, read in stream order  */
} mcraw_yuv;               /* sizeof 72; y_off 16, c_off 20, cy 24, cb 36, cr 48, reserved 60, lut 64 */
int mcraw_demosaic_yuv_batch(mcraw_ctx *ctx, const mcraw_rgb *p, const mcraw_yuv *y, const mcraw_rgb_color *colors,
                             int ncolors, const uint16_t *in, size_t in_pitch, size_t in_frame_stride, int width,
                             int height, int n, void *out, size_t out_bytes, void *stream);

/* ---- the edge-directed demosaic: MCRAW_RGB_HA, in all three output families ----------------------------------------
 *
 * A second full-resolution algorithm beside MCRAW_RGB_MHC, accepted by mcraw_demosaic_batch, mcraw_demosaic_display_batch and
 * mcraw_demosaic_yuv_batch with every rule of theirs: Ho = height, Wo = width, no further struct, no scratch.  Hamilton-Adams
 * adaptive colour-plane interpolation in integers: green is interpolated along the axis with the smaller gradient, R and B from
 * their differences against green.  The area, resample and warp entry points keep rejecting it, and the latter two keep
 * sampling MCRAW_RGB_MHC's estimates.
 * Bit-exact arithmetic.  d(y, x) = (int)s(y, x) - (int)black[p] as for MHC; reads outside the frame are reflected 101-style, by
 * up to 3 samples (frames are at least 4 x 4: one reflection is enough).  role = p ^ shift(cfa) in RGGB terms.
 *   The green plane g, in 1/8 DN, on the frame and a ring of one pixel around it (the ring from the reflected d):
 *     at a green site     g = 8 d
 *     at an R or B site, C = d there:
 *       ch = 2 C - d[y][x-2] - d[y][x+2]                  cv: the transpose
 *       gh = 2 (d[y][x-1] + d[y][x+1]) + ch               gv: the transpose
 *       DH = |d[y][x-1] - d[y][x+1]| + |ch|               DV: the transpose
 *       g  = 2 gh if DH < DV, 2 gv if DV < DH, gh + gv if they are equal
 *   The estimates E_c, in 1/32 DN:
 *     E_G = 4 g;  the native channel 32 d
 *     for a pair of opposite neighbours a, b that carry the wanted colour:
 *       n(a, b) = 8 (d_a + d_b) + (2 g - g_a - g_b)       D(a, b) = 8 |d_a - d_b| + |2 g - g_a - g_b|
 *     R or B at a green site    2 n(left, right) or 2 n(up, down), whichever axis carries that colour
 *     R at B, B at R            N = (nw, se), P = (ne, sw): 2 n(N) if D(N) < D(P), 2 n(P) if D(P) < D(N), n(N) + n(P) if equal
 *   Range, with |d| <= 65535 =: M, each step a sum of bounded terms:
 *     |ch| <= 4 M, |gh| <= 4 M + 4 M = 8 M, so |g| <= 16 M at an R or B site and 8 M at a green one: |g| <= 16 * 65535;
 *     |E_G| = 4 |g| <= 64 M;  at a green site the neighbours a, b are R / B sites: |2 g - g_a - g_b| <= 16 M + 32 M = 48 M,
 *     |n| <= 16 M + 48 M = 64 M, |E| <= 128 M;  at an R or B site |2 g - g_a - g_b| <= 32 M + 32 M = 64 M, |n| <= 80 M,
 *     |E| <= 160 M = 10 485 600 < 2^24;  D <= 16 M + 64 M.  Everything fits int32 and (float)E_c is exact.
 *   From E_c on it is MHC's stage, unchanged: k[c] = (gain[c] * inv) * 0.03125f, then v_c, o_i, the clip and the float,
 *   display and YUV stores.
 * What follows: a flat frame gives E_c = 32 d everywhere; transposing the mosaic, its black levels and its CFA transposes the
 * result, bit for bit; mirroring the columns mirrors it.
 * Kernel: krgb_ha (csrc/mcraw_ha.hip); it has no kernel id (mcraw_ctx_kernel_ms does not see it). */
#define MCRAW_RGB_HA 6   /* valid where MCRAW_RGB_MHC is: the three entry points above */

/* ---- uint16 mosaics -> any output size: an area downscale of a crop window, into all three output families ---------
 *
 * BIN2 generalised from "one quad per output pixel" to "the quads under the pixel's footprint": a crop of cw x ch samples at
 * (x0, y0) of every mosaic, Qw = cw / 2 by Qh = ch / 2 CFA quads, becomes out_h x out_w pixels, each the area average of the
 * quads that its footprint covers.  One pass over the cropped mosaic, integers up to the colour stage, no interpolation.
 * Output family: `d` and `y` NULL: the float family (mcraw_demosaic_batch: p->dtype, p->flags); `d`: the display family
 * (mcraw_demosaic_display_batch); `y`: the YUV family (mcraw_demosaic_yuv_batch); both: rejected.  p->algo must be
 * MCRAW_RGB_AREA, which the three other entry points keep rejecting.
 * Bit-exact arithmetic.  e_c(qy, qx): BIN2's estimates of quad (qy, qx) of the crop, E_R = 2 d(r), E_G = d(g1) + d(g2),
 * E_B = 2 d(b), d = s - black[p] (int32).  Per axis, Q quads (Qw, Qh) onto O pixels (out_w, out_h):
 *   c(k, q)    = clamp(floor((256 * (q * O - k * Q) + (Q >> 1)) / Q), 0, 256)     64-bit, floor division
 *   w(k, q)    = c(k, q + 1) - c(k, q)                                             q from q0(k) = floor(k * Q / O)
 *   h_c(qy, k) = sum_q wx(k, q) * e_c(qy, q)                                       int32, |h| <= 256 * 131070
 *   t_c(qy, k) = (h_c + 8) >> 4                                                    arithmetic shift; units of 1/32
 *   v_c(j, k)  = sum_q wy(j, q) * t_c(q, k)                                        int32, |v| < 2^30
 *   E_c(j, k)  = (v_c + 128) >> 8                                                  units of 1/32; |E| < 2^22, exact as float
 *   host, f32: k[c] = (gain[c] * inv) * 0.03125f                                   inv as in mcraw_demosaic_batch
 * The weights are the overlap of the footprint [k Q / O, (k + 1) Q / O) with each quad, rounded cumulatively: 256 per pixel
 * in all, none negative, at most 17 per axis.  A flat frame comes out flat (E = 32 d), greys stay neutral, and with
 * cw = 2 out_w, ch = 2 out_h the result is MCRAW_RGB_BIN2's of the crop, bit for bit.  From E_c and k[c] on everything is the
 * family's own entry point: colour stage, clamp, LUT, matrix, layouts, with Ho = out_h, Wo = out_w.
 * Accepted: x0, y0, cw, ch even, cw, ch >= 2, x0 + cw <= width, y0 + ch <= height; 1 <= out_w <= Qw <= 16 out_w and likewise
 * out_h; the YUV family needs an even out_w and out_h; width, height, in, in_pitch, in_frame_stride, colors, out and
 * out_bytes follow the family's entry point.  A ratio under 2 samples per pixel (more pixels than quads) needs a real
 * demosaic in front of a resampler and is out of scope: run MCRAW_RGB_MHC and resize its output.
 * `work`: the caller's DEVICE memory, 16-byte aligned, at least mcraw_area_work_bytes(a) bytes.  A small kernel queued on
 * `stream` in front of the demosaic writes the per-column and per-row weight tables into it; nothing is cached in the
 * context, nothing waits for the host, and calls queued on one stream may share one `work`.
 * Rejected (returns < 0, mcraw_last_error says why, starting with "mcraw_demosaic_area_batch: ", nothing is written):
 * everything the family's own entry point rejects; a NULL `a`; a p->algo other than MCRAW_RGB_AREA; both `d` and `y`; an odd,
 * empty or out-of-frame crop; a size outside the ratio rule; a non-zero `reserved`; a NULL or misaligned `work`; work_bytes
 * below mcraw_area_work_bytes(a).  n == 0 is a no-op.  The call takes no decode serial, leaves the decode slots,
 * mcraw_ctx_errors and the context's stage alone, and has no kernel id of its own (time it with events on `stream`). */
#define MCRAW_RGB_AREA 3   /* valid in mcraw_demosaic_area_batch only */
typedef struct mcraw_area {
    uint32_t x0, y0;        /* crop origin in the mosaic, both even                 */
    uint32_t cw, ch;        /* crop size, both even, >= 2; x0 + cw <= width, ...    */
    uint32_t out_w, out_h;  /* Wo, Ho                                               */
    uint32_t reserved[2];   /* must be 0                                            */
} mcraw_area;               /* sizeof 32; y0 4, cw 8, ch 12, out_w 16, out_h 20, reserved 24 */
size_t mcraw_area_work_bytes(const mcraw_area *a);  /* 0 for a rejected geometry */
int mcraw_demosaic_area_batch(mcraw_ctx *ctx, const mcraw_rgb *p, const mcraw_area *a, const mcraw_display *d,
                              const mcraw_yuv *y, const mcraw_rgb_color *colors, int ncolors, const uint16_t *in,
                              size_t in_pitch, size_t in_frame_stride, int width, int height, int n, void *work,
                              size_t work_bytes, void *out, size_t out_bytes, void *stream);

/* ---- uint16 mosaics -> any output size from half to twice a crop window: MHC behind a polyphase filter ---------------
 *
 * The band that the area downscale leaves out: a crop of cw x ch samples at (x0, y0) of every mosaic becomes out_h x out_w
 * pixels, ceil(cw / 2) <= out_w <= 2 cw and likewise out_h, by resampling the full-resolution Malvar-He-Cutler image with a
 * separable linear or cubic (Catmull-Rom) filter, horizontally first.  Output family: `d` and `y` NULL: the float family;
 * `d`: the display family; `y`: the YUV family; both: rejected, as in mcraw_demosaic_area_batch.  p->algo must be
 * MCRAW_RGB_RESAMPLE, which every other entry point keeps rejecting.
 * Bit-exact arithmetic.  e_c(y, x): MCRAW_RGB_MHC's integer estimates of the WHOLE frame, in 1/16 DN, |e| < 2^22; outside the
 * frame e_c(y, x) = e_c(reflect101(y, height), reflect101(x, width)) (taps reach at most 4 samples beyond the crop and MHC 2
 * more: one reflection suffices for frames of 8 and up).  Taps that leave the crop but stay in the frame read the real
 * pixels there.  Per axis, C crop samples (cw, ch) onto O pixels (out_w, out_h), pixel centres aligned, the filter stretched
 * by max(1, C / O); j counts from the crop's origin and may be negative or >= C:
 *   D = 2 max(C, O);  n(k, j) = 2 O j - ((2 k + 1) C - O);  a = floor((1024 |n| + D / 2) / D)          64-bit
 *   linear: f = max(0, 1024 - a)
 *   cubic:  f = 3 a^3 - 5 * 1024 a^2 + 2 * 1024^3                      a <= 1024
 *           f = -a^3 + 5 * 1024 a^2 - 8 * 1024^2 a + 4 * 1024^3        1024 < a < 2048;  0 otherwise
 *   F = sum_j f;  w(k, j) = floor((4096 f + F / 2) / F)               floor division; then the residual 4096 - sum_j w is
 *           added to the tap of smallest |n|; two taps of equal smallest |n| take half of it each (it is even then)
 *   t_c(y, k) = (sum_j wx(k, j) e_c(y, x0 + j) + 2048) >> 12          exact sum, arithmetic shift; 1/16 DN; |t| < 2^23
 *   E_c(i, k) = (sum_j wy(i, j) t_c(y0 + j, k) + 2048) >> 12          likewise; |E| < 2^24, exact as float
 *   host, f32: k[c] = (gain[c] * inv) * 0.0625f                       as MCRAW_RGB_MHC
 * The weights of a pixel add up to 4096 exactly, sum |w| <= 5600 (cubic; 4096 linear), at most 5 (linear) or 9 (cubic) taps
 * per axis, the taps of pixel k mirror those of pixel O - 1 - k, and O = C gives the single tap 4096 at j = k.  The sums do not
 * fit int32 as they stand (2^22 * 5600); with v = 256 vh + vl, vl = v & 255, A = sum w vh and B = sum w vl fit (|A| < 2^28,
 * 0 <= |B| < 2^21) and (256 A + B + 2048) >> 12 == (A + ((B + 2048) >> 8)) >> 4.  A flat frame comes out flat (E = 16 d),
 * greys stay neutral, and with out_w = cw, out_h = ch the result is MCRAW_RGB_MHC's output cut to the crop, bit for bit, in
 * every family.  From E_c and k[c] on everything is the family's own entry point: colour stage, clamp, LUT, matrix, layouts,
 * with Ho = out_h, Wo = out_w.
 * Accepted: width, height even and >= 8; x0, y0, cw, ch even, cw, ch >= 2, x0 + cw <= width, y0 + ch <= height; the size
 * rule above; filter MCRAW_FILTER_LINEAR or MCRAW_FILTER_CUBIC; the YUV family needs an even out_w and out_h; in, in_pitch,
 * in_frame_stride, colors, out and out_bytes follow the family's entry point.
 * `work`: the caller's DEVICE memory, 16-byte aligned, at least mcraw_resample_work_bytes(r) bytes; a small kernel queued on
 * `stream` in front writes the tap tables into it, as for the area downscale: nothing is cached, nothing waits for the host,
 * and calls queued on one stream may share one `work`.
 * Rejected (returns < 0, mcraw_last_error says why, starting with "mcraw_demosaic_resample_batch: ", nothing is written):
 * everything the family's own entry point rejects; a NULL `r`; a p->algo other than MCRAW_RGB_RESAMPLE; both `d` and `y`; a
 * frame under 8 x 8; an odd, empty or out-of-frame crop; a size outside the rule; an unknown filter; a non-zero `reserved`;
 * a NULL or misaligned `work`; work_bytes below mcraw_resample_work_bytes(r).  n == 0 is a no-op.  The call takes no decode
 * serial, leaves the decode slots, mcraw_ctx_errors and the context's stage alone, and has no kernel id of its own. */
#define MCRAW_RGB_RESAMPLE 4   /* valid in mcraw_demosaic_resample_batch only */
#define MCRAW_FILTER_LINEAR 0
#define MCRAW_FILTER_CUBIC 1
typedef struct mcraw_resample {
    uint32_t x0, y0;        /* crop origin in the mosaic, both even                 */
    uint32_t cw, ch;        /* crop size, both even, >= 2; x0 + cw <= width, ...    */
    uint32_t out_w, out_h;  /* Wo, Ho                                               */
    uint32_t filter;        /* MCRAW_FILTER_*                                       */
    uint32_t reserved;      /* must be 0                                            */
} mcraw_resample;           /* sizeof 32; y0 4, cw 8, ch 12, out_w 16, out_h 20, filter 24, reserved 28 */
size_t mcraw_resample_work_bytes(const mcraw_resample *r);  /* 0 for a rejected geometry */
int mcraw_demosaic_resample_batch(mcraw_ctx *ctx, const mcraw_rgb *p, const mcraw_resample *r, const mcraw_display *d,
                                  const mcraw_yuv *y, const mcraw_rgb_color *colors, int ncolors, const uint16_t *in,
                                  size_t in_pitch, size_t in_frame_stride, int width, int height, int n, void *work,
                                  size_t work_bytes, void *out, size_t out_bytes, void *stream);

/* ---- uint16 mosaics -> the MHC image sampled along one affine map per frame: the stabilisation warp ----------------
 *
 * out_h x out_w pixels per frame, each the full-resolution Malvar-He-Cutler image of its mosaic sampled at an affine position:
 * translation to 1/256 sample, roll up to about 14 degrees, zoom 0.75 .. 1.25.  Output family: `d` and `y` NULL: the float
 * family; `d`: the display family; `y`: the YUV family; both: rejected.  p->algo must be MCRAW_RGB_WARP, which every other
 * entry point keeps rejecting.
 * A map is six int32 in HOST memory, {ayy, ayx, ty, axy, axx, tx}: the linear part in 1/65536, the translation in 1/256
 * sample; `maps` holds nmaps of them, 1 (one map for the batch) or n, read before the call returns, like `colors`.  Output
 * pixel (i, k) of frame f reads the position (64-bit, arithmetic shifts; integer coordinates are sample centres)
 *   Y = ty + ((ayy i + ayx k + 128) >> 8)      iy = Y >> 8,  py = Y & 255
 *   X = tx + ((axy i + axx k + 128) >> 8)      ix = X >> 8,  px = X & 255
 * so that {65536, 0, 0, 0, 65536, 0} reads sample (i, k).  One table of 256 phases x 4 taps, at j = -1 .. 2 about iy (or ix),
 * serves both axes:
 *   linear: w(p) = (0, 16 (256 - p), 16 p, 0)
 *   cubic:  a = 4 |256 j - p|; f(a), F = sum_j f, w = floor((4096 f + F / 2) / F) and the residual rule are those of
 *           mcraw_demosaic_resample_batch (Catmull-Rom): the residual goes to the tap of smallest distance, half each to two
 *           equally near.  F = 2 * 1024^3 for every phase, sum w = 4096, sum |w| <= 5120, w >= -303, w(0) = (0, 4096, 0, 0),
 *           w(128) = (-256, 2304, 2304, -256), and w(p) mirrors w(256 - p).
 * e_c(y, x): MCRAW_RGB_MHC's integer estimates of the WHOLE frame, in 1/16 DN, |e| < 2^22; outside the frame
 * e_c(y, x) = e_c(reflect101(y, height), reflect101(x, width)).  Horizontally first, with the resample's two roundings:
 *   t_c(r, k) = (sum_j w(px)[j] e_c(r, ix - 1 + j) + 2048) >> 12      r = iy - 1 .. iy + 2; exact sum, arithmetic shift
 *   E_c(i, k) = (sum_j w(py)[j] t_c(iy - 1 + j, k) + 2048) >> 12      likewise; exact as float
 *   host, f32: k[c] = (gain[c] * inv) * 0.0625f                       as MCRAW_RGB_MHC
 * (the sums through v = 256 vh + vl, as the resample).  From E_c and k[c] on everything is the family's own entry point, with
 * Ho = out_h, Wo = out_w.  With the identity linear part and a translation of whole samples (256 a, 256 b) the result is
 * MCRAW_RGB_MHC's output cut at (a, b), bit for bit, in every family and for both filters; a flat frame comes out flat and
 * greys stay neutral.  The filter is not stretched: zoom-out (a linear part above 65536, down to 0.75 of the size) aliases
 * slightly.
 * Accepted: width, height even and >= 8; out_w, out_h 1 .. 65536, both even for the YUV family; filter MCRAW_FILTER_LINEAR or
 * MCRAW_FILTER_CUBIC; nmaps 1 or n; per map |ayy - 65536|, |axx - 65536|, |ayx|, |axy| <= 16384, and the four corner pixels
 * (0, 0), (0, Wo - 1), (Ho - 1, 0), (Ho - 1, Wo - 1) with 0 <= Y <= 256 (height - 1) and 0 <= X <= 256 (width - 1): Y and X are
 * monotone in i and k, so the corners bound every pixel, taps and MHC's halo leave the frame by at most 4 samples and one
 * reflection suffices.  in, in_pitch, in_frame_stride, colors, out and out_bytes follow the family's entry point.
 * Rejected (returns < 0, mcraw_last_error says why, starting with "mcraw_demosaic_warp_batch: ", nothing is written; a
 * message about a map names the frame of the first bad one): everything the family's own entry point rejects; a NULL `wp` or
 * `maps`; a p->algo other than MCRAW_RGB_WARP; both `d` and `y`; a frame under 8 x 8; a non-zero `reserved`; an unknown
 * filter; a size outside 1 .. 65536; a linear part or a corner outside the rules above; nmaps other than 1 or n.  n == 0 is
 * a no-op.  The call needs no scratch, takes no decode serial, leaves the decode slots, mcraw_ctx_errors and the context's
 * stage alone, and has no kernel id of its own. */
#define MCRAW_RGB_WARP 5       /* valid in mcraw_demosaic_warp_batch only */
typedef struct mcraw_warp {
    uint32_t out_w, out_h;  /* Wo, Ho                                               */
    uint32_t filter;        /* MCRAW_FILTER_*                                       */
    uint32_t reserved;      /* must be 0                                            */
} mcraw_warp;               /* sizeof 16; out_h 4, filter 8, reserved 12 */
int mcraw_demosaic_warp_batch(mcraw_ctx *ctx, const mcraw_rgb *p, const mcraw_warp *wp, const mcraw_display *d,
                              const mcraw_yuv *y, const mcraw_rgb_color *colors, int ncolors, const int32_t *maps, int nmaps,
                              const uint16_t *in, size_t in_pitch, size_t in_frame_stride, int width, int height, int n,
                              void *out, size_t out_bytes, void *stream);

/* ---- uint16 mosaics -> the MHC image sampled along one displacement mesh per frame: lens geometry, local motion ------
 *
 * The affine warp above with the position of every output pixel taken from a mesh of source positions in DEVICE memory instead
 * of six numbers in host memory: lens distortion (DNG WarpRectilinear, a vendor grid), rolling-shutter wobble, parallax, a
 * projective map.  Output family, `p`, `d`, `y`, `colors`, in, out: as mcraw_demosaic_warp_batch; p->algo must be
 * MCRAW_RGB_MESH, which every other entry point keeps rejecting.
 * A mesh is My x Mx nodes, My = ceil(out_h / 32) + 1, Mx = ceil(out_w / 32) + 1 (MCRAW_MESH_STEP output pixels between nodes,
 * both axes: one node per corner of the kernel's tile).  A node is two int32, (Y, X): node (a, b) is the source position of
 * output pixel (32 a, 32 b) in 1/256 sample.  Row-major, contiguous, 8-byte aligned, meshes back to back; nmesh is 1 (one mesh
 * for the batch: a lens) or n (one per frame: a clip).  The nodes are read by the queued kernel in stream order and never copied:
 * a kernel that wrote them earlier on the stream is seen, and nothing waits for the host.
 * Output pixel (i, k) has a = i >> 5, u = i & 31, b = k >> 5, v = k & 31 and, with Y00 .. Y11 the Y of nodes (a, b), (a, b + 1),
 * (a + 1, b), (a + 1, b + 1), the position (exact in 64 bits, arithmetic shift)
 *   Yr = (Y00 (32-u)(32-v) + Y01 (32-u) v + Y10 u (32-v) + Y11 u v + 512) >> 10        Y = min(max(Yr, 0), 256 (height - 1))
 * and X likewise with `width`.  The clamp is per pixel, not per node (a node behind the last partial tile may lie anywhere): a
 * position that leaves the frame reads the frame's edge.  Adjacent tiles agree on their common edge.
 * The window of a tile (its rows i0 .. i1, columns k0 .. k1): over the clamped positions of its four corner pixels (i0 | i1,
 * k0 | k1), with ylo, yhi, xlo, xhi their extremes,
 *   pb = ((ylo >> 8) - 1) & ~1     np = (((yhi >> 8) + 2 - pb) >> 1) + 1     np' = min(np, 26)
 *   eb = ((xlo >> 8) - 1) & ~7     ne = (((xhi >> 8) + 2 - eb) >> 3) + 1     ne' = min(ne, 8)
 * A pixel's first tap row iy - 1 is clamped to [pb, pb + 2 np' - 4], its first tap column ix - 1 to [eb, eb + 8 ne' - 4]; the
 * phases py, px stay those of (Y, X).  A bilinear function takes its extremes over a rectangle at its corners, and the floor and
 * the clamp are monotone, so the four corner pixels bound every position of the tile: in the regime np <= 26, ne <= 8 -- every
 * map inside the affine warp's bounds, and zoom-out to 0.75 anywhere -- the tap clamp never acts.  Outside it the result is
 * still defined and deterministic for ANY node content: no tap and no staged sample leaves the frame by more than 4.
 * From (Y, X) and the tap origin on everything is mcraw_demosaic_warp_batch's: the phase table of `filter`, horizontally first
 * with the two roundings, e_c = MCRAW_RGB_MHC's estimates of the whole frame reflected 101, k[c] = (gain[c] * inv) * 0.0625f,
 * then the family's stage.  A mesh with nodes 256 (32 a + ty, 32 b + tx) gives MCRAW_RGB_MHC's output cut at (ty, tx), bit for
 * bit, in every family and for both filters; the mesh of a map with the identity linear part (fractional translation included)
 * gives mcraw_demosaic_warp_batch's output under that map, bit for bit; a flat frame stays flat and greys stay neutral.
 * mcraw_mesh_nodes: My * Mx, or 0 for a rejected geometry.  mcraw_mesh_check: nmesh >= 1 meshes in HOST memory against width x
 * height frames, without a GPU or a context: 0, or < 0 with mcraw_last_error ("mcraw_mesh_check: ...") naming the first frame
 * and tile (ty, tx) whose window leaves the regime; with flags & 1 also the first tile where a corner pixel's unclamped position
 * leaves the frame.
 * Rejected (returns < 0, mcraw_last_error says why, starting with "mcraw_demosaic_mesh_batch: ", nothing is written):
 * everything the family's own entry point rejects; a NULL `m` or `nodes`; a p->algo other than MCRAW_RGB_MESH; both `d` and
 * `y`; a frame under 8 x 8 or odd; a non-zero `reserved`; an unknown filter; a size outside 1 .. 65536, or odd for the YUV
 * family; nmesh other than 1 or n; `nodes` not 8-byte aligned; nodes_bytes below nmesh * My * Mx * 8.  n == 0 is a no-op.  The
 * call needs no scratch, takes no decode serial, leaves the decode slots, mcraw_ctx_errors and the context's stage alone, and
 * has no kernel id of its own. */
#define MCRAW_RGB_MESH  7      /* valid in mcraw_demosaic_mesh_batch only */
#define MCRAW_MESH_STEP 32     /* output pixels between nodes, both axes   */
typedef struct mcraw_mesh {
    uint32_t out_w, out_h;  /* Wo, Ho                                               */
    uint32_t filter;        /* MCRAW_FILTER_*                                       */
    uint32_t reserved;      /* must be 0                                            */
} mcraw_mesh;               /* sizeof 16; out_h 4, filter 8, reserved 12 */
size_t mcraw_mesh_nodes(const mcraw_mesh *m);  /* My * Mx, 0 for a rejected geometry */
int mcraw_mesh_check(const mcraw_mesh *m, const int32_t *nodes_host, int nmesh, int width, int height, int flags);
int mcraw_demosaic_mesh_batch(mcraw_ctx *ctx, const mcraw_rgb *p, const mcraw_mesh *m, const mcraw_display *d,
                              const mcraw_yuv *y, const mcraw_rgb_color *colors, int ncolors, const int32_t *nodes,
                              size_t nodes_bytes, int nmesh, const uint16_t *in, size_t in_pitch, size_t in_frame_stride,
                              int width, int height, int n, void *out, size_t out_bytes, void *stream);

/* ---- uint16 mosaics -> uint16 mosaics with a lens-shading gain map applied ----------------------------------------
 *
 * Multiplies what `n` uint16 mosaics of width x height hold above their black level by a per-pixel gain that is bilinearly
 * interpolated from a small map, and writes mosaics of the same black level: the stage in front of a demosaic that takes
 * the vignetting and its colour cast out (Android's LensShadingMap, a DNG GainMap opcode).  Pitches and frame strides count
 * uint16 elements.  A map has four planes of map_h x map_w uint16 entries in Q3.12 (4096 is a gain of 1.0), indexed by CFA
 * position p = (y & 1) * 2 + (x & 1) like black[4] (the call never needs the CFA).  Bit 15 of an entry is ignored:
 * g = entry & 0x7FFF, so gains stay below 8 and no map content can make a sum wrap.  Map point (j, i) sits on pixel
 * (j * (H - 1) / (map_h - 1), i * (W - 1) / (map_w - 1)): the corner points sit on the corner pixels.  Bit-exact, in integers:
 *   host:   sx = W > 1 ? floor((map_w - 1) * 2^24 / (W - 1)) : 0        sy likewise from map_h, H
 *   pixel:  ux = x * sx;  i0 = ux >> 24;  fx = (ux >> 12) & 4095;  i1 = min(i0 + 1, map_w - 1)
 *           uy = y * sy;  j0 = uy >> 24;  fy = (uy >> 12) & 4095;  j1 = min(j0 + 1, map_h - 1)
 *           V0 = (g[p][j0][i0] * (4096 - fy) + g[p][j1][i0] * fy + 2048) >> 12        vertical first
 *           V1 = (g[p][j0][i1] * (4096 - fy) + g[p][j1][i1] * fy + 2048) >> 12
 *           G  = (V0 * (4096 - fx) + V1 * fx + 2048) >> 12                            0 <= G <= 32767
 *           d  = (int)s - (int)black[p]
 *           c  = black[p] + ((d * G + 2048) >> 12)                                   arithmetic shift: floor
 *           out = (uint16) min(max(c, 0), top)
 * The order is fixed, vertical then horizontal, because each stage rounds.  map_w, map_h <= 64 gives ux < 2^30;
 * |d * G| + 2048 <= 65535 * 32767 + 2048 < 2^31; every factor fits in 24 bits.  An all-4096 map returns the input (below
 * `top`) bit for bit.
 * The map is the caller's DEVICE memory, read by the queued kernel in stream order and never copied into or cached by the
 * context: two calls with the same pointer and new contents in between each see their own.  nmaps == 1 applies one map to
 * every frame, nmaps == n gives one per frame, back to back.
 * In place is allowed: out == in with the same pitch and (n > 1) the same frame stride; each pixel reads only itself.
 * `stream`: a hipStream_t, NULL = the context's own stream; the call queues the work and returns without synchronising.
 * It takes no decode serial and leaves the decode slots, mcraw_ctx_errors, mcraw_ctx_last_serial and the context's stage
 * alone.  n == 0 is a no-op.  The launch has no id in mcraw_ctx_kernel_ms (time it with stream events).
 * Rejected (returns < 0, mcraw_last_error says why, nothing is written): a NULL `s`, `in`, `out` or `map`; an odd `in` or
 * `out` address; a `map` that is not 16-byte aligned; width or height outside 1 .. 65536 (odd sizes are fine); a pitch
 * below width; n > 1 and a frame stride below (height - 1) * pitch + width; map_w or map_h outside 1 .. 64; nmaps not 1 or
 * n; top outside 1 .. 65535; a non-zero `reserved`; input and output extents that overlap other than in place. */
typedef struct mcraw_shade {
    uint32_t map_w, map_h;   /* 1 .. 64 each                                                  */
    uint32_t nmaps;          /* 1: one map for the batch; n: one per frame, back to back      */
    uint32_t top;            /* 1 .. 65535: the output saturates here                         */
    uint16_t black[4];       /* by CFA position                                               */
    uint32_t reserved[2];    /* must be 0                                                     */
    const uint16_t *map;     /* DEVICE memory, 16-byte aligned: (nmaps, 4, map_h, map_w)      */
} mcraw_shade;               /* sizeof 40; black 16, reserved 24, map 32                      */
int mcraw_shade_batch(mcraw_ctx *ctx, const mcraw_shade *s, const uint16_t *in, size_t in_pitch, size_t in_frame_stride,
                      int width, int height, int n, uint16_t *out, size_t out_pitch, size_t out_frame_stride, void *stream);

/* ---- uint16 mosaics -> per-frame statistics by CFA position ----------------------------------------------------------
 *
 * Counts what `n` uint16 mosaics of width x height hold inside one window, per frame and per CFA position
 * p = (y & 1) * 2 + (x & 1): what measures the `white`, `black` and `gain` the other stages take, a clip's exposure, its
 * clipping.  Pitches and frame strides count uint16 elements.  Everything is an integer, so the result does not depend on
 * the order of the additions: it is bit-exact.  With B = 1 << bins_log2, for frame f and every pixel (y, x) with
 * y0 <= y < y0 + h and x0 <= x < x0 + w (frame coordinates: a window at an odd offset keeps the frame's CFA positions),
 * v = in[f * in_frame_stride + y * in_pitch + x]:
 *   hist[p][min(v >> shift, B - 1)] += 1            the last bin takes everything above it
 *   cnt[p]  += 1
 *   nsat[p] += 1          if v >= sat[p]             (sat[p] = 0: every sample is saturated)
 *   sum[p]  += v          otherwise                  the unsaturated samples only
 *   min[p] = min(min[p], v),  max[p] = max(max[p], v)    over all samples of the window, saturated ones included
 * A CFA position without a sample in the window (a window one pixel wide or high) keeps min = 65535 and max = 0.
 * The record of one frame, records back to back in `out` (8-byte aligned):
 *   uint32 hist[4][B];  uint32 cnt[4], nsat[4], min[4], max[4];  uint64 sum[4]        16 * B + 96 bytes
 * With width, height <= 65536 a CFA position has at most 2^30 samples: no uint32 counter can wrap, and sum < 2^46.
 * Without MCRAW_STATS_ACCUMULATE the call initialises the n records itself, on the stream (the caller never clears `out`;
 * a second call into the same `out` gives the same bytes).  With it the call adds to the records that are there and takes
 * min / max against them: a clip's histogram over several batches, a frame's over several windows.  The uint32 counters
 * then wrap modulo 2^32 (sum modulo 2^64) once the caller's total passes them.
 * `in` may sit at any 2-byte alignment with any pitch (16-byte loads where base, pitch and stride allow it).  Only the
 * window's samples are read.
 * `stream`: a hipStream_t, NULL = the context's own stream; the call queues the work and returns without synchronising.
 * It takes no decode serial and leaves the decode slots, mcraw_ctx_errors, mcraw_ctx_last_serial and the context's stage
 * alone.  n == 0 is a no-op; n may exceed 65535.  The launches have no id in mcraw_ctx_kernel_ms (time them with stream
 * events).
 * Rejected (returns < 0, mcraw_last_error says why, starting with "mcraw_stats_batch: ", nothing is written): a NULL `s`, `in`
 * or `out`; an odd `in` address; an `out` that is not 8-byte aligned; width or height outside 1 .. 65536; a pitch below
 * width; n > 1 and a frame stride below (height - 1) * pitch + width; bins_log2 outside 6 .. 12; shift above 15; w or h of 0;
 * a window that leaves the frame (x0 + w > width or y0 + h > height, computed without overflow); an unknown flag; a non-zero
 * `reserved`; out_bytes < n * mcraw_stats_record_bytes(bins_log2); an `out` range that overlaps the input's extent. */
#define MCRAW_STATS_ACCUMULATE 1u   /* flags: add to the records already at `out` instead of initialising them */
typedef struct mcraw_stats {
    uint32_t bins_log2;      /* 6 .. 12: B = 1 << bins_log2 bins per CFA position                 */
    uint32_t shift;          /* 0 .. 15: bin of sample s = min(s >> shift, B - 1)                 */
    uint32_t x0, y0, w, h;   /* the window counted, in frame pixels; w, h >= 1                    */
    uint16_t sat[4];         /* by CFA position: s >= sat[p] counts as saturated                  */
    uint32_t flags;          /* MCRAW_STATS_ACCUMULATE or 0                                       */
    uint32_t reserved;       /* must be 0                                                         */
} mcraw_stats;               /* sizeof 40; x0 8, sat 24, flags 32, reserved 36                    */
size_t mcraw_stats_record_bytes(uint32_t bins_log2);   /* 16 * B + 96; 0 for a bins_log2 outside 6 .. 12 */
int mcraw_stats_batch(mcraw_ctx *ctx, const mcraw_stats *s, const uint16_t *in, size_t in_pitch, size_t in_frame_stride,
                      int width, int height, int n, void *out, size_t out_bytes, void *stream);

/* ---- uint16 mosaics -> per-frame histograms of local noise energy by CFA position and signal level --------------------
 *
 * Measures what a noise profile (variance = S * x + O per CFA position: the table of mcraw_denoise_batch and
 * mcraw_merge_batch) is fitted to.  Pitches and frame strides count uint16 elements.  Everything is an integer, so the
 * result does not depend on the order of the additions: it is bit-exact.
 * One window (x0, y0, w, h) in frame pixels, x0 and y0 even, w, h >= 16, is cut into blocks of 16 x 16 samples at
 * (y0 + 16 j, x0 + 16 i); only whole blocks count, floor(h / 16) x floor(w / 16) of them, and only their samples are
 * read.  Within a block each CFA position p = (y & 1) * 2 + (x & 1) holds an 8 x 8 plane b[r][c] of same-colour samples:
 *   s = sum of b[r][c]                                                                        (below 2^22)
 *   T = sum over r, c = 1 .. 6 of (b[r][c-1] - 2 b[r][c] + b[r][c+1])^2
 *     + sum over r = 1 .. 6, c of (b[r-1][c] - 2 b[r][c] + b[r+1][c])^2
 * 96 squared second differences: each has expectation 6 sigma^2 under white noise and is 0 on a linear gradient, so
 * E[T] = 576 sigma^2.  |d| <= 4 * 65535, d^2 < 2^37, T < 2^43: 64-bit sums.  No halo, so nothing reflects.
 * The (block, position) is rejected, nrej[p] += 1, if any of its 64 samples is >= sat[p] or < lo[p] (clipping at either
 * end shrinks the variance; lo[p] = 0 disables the lower test, sat[p] = 0 rejects everything).  Otherwise
 *   l  = min((s >> 6) >> shift, 31)                                                           the level bin
 *   vb = 0 if T < 16, else with e = floor(log2 T), f = (T >> (e - 2)) & 3:  vb = min(4 * (e - 4) + f + 1, 127)
 *   hist[p][l][vb] += 1;  nblk[p] += 1
 * The energy bins are quarter octaves whose lower edges are 2^e * (1 + f / 4); mcraw_noise_energy_bin(T) is that formula.
 * The record of one frame, records back to back in `out` (8-byte aligned):
 *   uint32 hist[4][32][128];  uint32 nblk[4];  uint32 nrej[4]                                 65 568 bytes
 * A frame of at most 65536 x 65536 has at most 2^24 blocks: no counter can wrap.
 * Without MCRAW_NOISE_ACCUMULATE the call initialises the n records itself, on the stream; with it the call adds to the
 * records that are there (a clip over several batches), and the counters wrap modulo 2^32 once the caller's total does.
 * `in` may sit at any 2-byte alignment with any pitch (16-byte loads where base, pitch, stride and x0 allow it).
 * `stream`: a hipStream_t, NULL = the context's own stream; the call queues the work and returns without synchronising.
 * It takes no decode serial and leaves the decode slots, mcraw_ctx_errors, mcraw_ctx_last_serial and the context's stage
 * alone.  n == 0 is a no-op; n may exceed 65535.  The launches have no id in mcraw_ctx_kernel_ms.
 * Rejected (returns < 0, mcraw_last_error says why, starting with "mcraw_noise_batch: ", nothing is written): a NULL `s`, `in`
 * or `out`; an odd `in` address; an `out` that is not 8-byte aligned; width or height outside 1 .. 65536; a pitch below
 * width; n > 1 and a frame stride below (height - 1) * pitch + width; shift above 15; an odd x0 or y0; w or h below 16; a
 * window that leaves the frame (computed without overflow); an unknown flag; a non-zero `reserved`;
 * out_bytes < n * mcraw_noise_record_bytes(); an `out` range that overlaps the input's extent. */
#define MCRAW_NOISE_ACCUMULATE 1u   /* flags: add to the records already at `out` instead of initialising them */
typedef struct mcraw_noise {
    uint32_t shift;          /* 0 .. 15: level bin of a plane = min(mean >> shift, 31)            */
    uint32_t x0, y0, w, h;   /* the window, in frame pixels; x0, y0 even; w, h >= 16              */
    uint16_t sat[4];         /* by CFA position: a plane with a sample >= sat[p] is rejected      */
    uint16_t lo[4];          /* by CFA position: ... or with a sample < lo[p]                     */
    uint32_t flags;          /* MCRAW_NOISE_ACCUMULATE or 0                                       */
    uint32_t reserved;       /* must be 0                                                         */
} mcraw_noise;               /* sizeof 44; x0 4, sat 20, lo 28, flags 36, reserved 40             */
size_t mcraw_noise_record_bytes(void);                 /* 65568 */
uint32_t mcraw_noise_energy_bin(uint64_t T);           /* the energy bin vb of T, on the host */
int mcraw_noise_batch(mcraw_ctx *ctx, const mcraw_noise *s, const uint16_t *in, size_t in_pitch, size_t in_frame_stride,
                      int width, int height, int n, void *out, size_t out_bytes, void *stream);

/* ---- uint16 mosaics -> uint16 mosaics with the defective pixels taken out ------------------------------------------------
 *
 * Finds hot, dead and stuck pixels in `n` uint16 mosaics of width x height and replaces them, and replaces the pixels of an
 * optional static list: a DNG FixBadPixelsConstant / FixBadPixelsList, Android's hotPixelMap.  The output is a mosaic of the
 * same black level, so everything that takes a mosaic takes the result.  Pitches and frame strides count uint16 elements.
 * black[4] and abs_thr[4] are indexed by CFA position p = (y & 1) * 2 + (x & 1) (the call never needs the CFA).  Integers
 * only: bit-exact.
 * Neighbours.  All neighbours lie on the pixel's own lattice, at distance 2: the same colour for every Bayer arrangement.
 * For d in {-2, +2} the neighbour coordinate of c is c' = c + d; if that is outside [0, size), c' = c - d; if that is outside
 * too, c' = c -- for rows and columns independently.  The eight neighbours as (dy, dx), in this order: NW (-2,-2), N (-2,0),
 * NE (-2,2), W (0,-2), E (0,2), SW (2,-2), S (2,0), SE (2,2).  Duplicates that the reflection makes count with their
 * multiplicity.  With height <= 2 (width <= 2) the centre stands in for its vertical (horizontal) neighbours.  The
 * centre is then among its own neighbours and the dynamic detector finds nothing: defined behaviour, not an error.
 * Dynamic detection, for every pixel, from the values of `in` only (v: the pixel):
 *   Hk = the rank-th largest of the eight neighbour values, Lk = the rank-th smallest              rank: 1 or 2
 *   thr(m) = abs_thr[p] + ((max(m - black[p], 0) * rel_thr) >> 8)       rel_thr in Q8, 0 .. 65535; everything below 2^32
 *   hot:   MCRAW_FIXPIX_HOT  is set, v > Hk and v - Hk > thr(Hk)
 *   cold:  MCRAW_FIXPIX_COLD is set, v < Lk and Lk - v > thr(Lk)
 * rank 2 lets two adjacent defects of one colour both be found; a line one pixel wide is kept at either rank.
 * Replacement of a hot or cold pixel: of the four opposite pairs in the order (W,E), (N,S), (NW,SE), (NE,SW) the one with the
 * smallest |a - b|, the first such pair on a tie: out = (a + b + 1) >> 1.  Every other pixel is copied.
 * counts: NULL, or 4-byte aligned DEVICE memory for n records of uint32 hot[4], cold[4] (32 bytes each, indexed by p), which
 * the call initialises itself on the stream: the pixels that the dynamic detector flagged, except those that the search below
 * finds in the list.
 * list: DEVICE memory, 4-byte aligned, of nlist <= 1 << 20 entries y << 16 | x, for every frame of the batch; read by the
 * queued kernels in stream order and never copied into or cached by the context (two calls with the same pointer and new
 * contents in between each see their own).  Entries with x >= width or y >= height are skipped.  A listed pixel is replaced
 * unconditionally, after and over the dynamic result, from the values of `in`: by the rule above among the pairs of which
 * NEITHER member is listed; if there is no such pair, the dynamic pass's result for the pixel stands.  "Listed" is what
 * this search finds, for the kernels and for the reference alike:
 *   lo = 0, hi = nlist;  while (lo < hi) { mid = (lo + hi) >> 1;  list[mid] < key ? lo = mid + 1 : hi = mid; }
 *   member = lo < nlist && list[lo] == key
 * so an ascending list means what it says, and a list that is not ascending still has one defined result.  The dynamic
 * detector does not consult the list.
 * There is no in-place form: every pixel reads its neighbours.  `in` and `out` may sit at any 2-byte alignment with any pitch
 * (16-byte accesses where base, pitch and stride allow it).
 * `stream`: a hipStream_t, NULL = the context's own stream; the call queues the work and returns without synchronising.
 * It takes no decode serial and leaves the decode slots, mcraw_ctx_errors, mcraw_ctx_last_serial and the context's stage
 * alone.  n == 0 is a no-op.  The launches have no id in mcraw_ctx_kernel_ms (time them with stream events).
 * Rejected (returns < 0, mcraw_last_error says why, starting with "mcraw_fixpix_batch: ", nothing is written): a NULL `f`, `in`
 * or `out`; an odd `in` or `out` address; width or height outside 1 .. 65536; a pitch below width; n > 1 and a frame stride
 * below (height - 1) * pitch + width; rank not 1 or 2; rel_thr > 65535; an unknown flag; nlist > 0 with a NULL or misaligned
 * `list`; nlist > 1 << 20; a misaligned `counts`; a non-zero `reserved`; input and output extents that overlap at all; a
 * `counts` range that overlaps the input's or the output's extent. */
#define MCRAW_FIXPIX_HOT 1u    /* flags: replace pixels far above their neighbours */
#define MCRAW_FIXPIX_COLD 2u   /* flags: replace pixels far below their neighbours */
typedef struct mcraw_fixpix {
    uint32_t flags;          /* MCRAW_FIXPIX_HOT | MCRAW_FIXPIX_COLD, or 0 (the list alone)       */
    uint32_t rank;           /* 1 or 2: the neighbour a pixel is compared with                    */
    uint32_t rel_thr;        /* 0 .. 65535, Q8: the part of the threshold that grows with level   */
    uint32_t nlist;          /* 0 .. 1 << 20 entries of `list`                                    */
    uint16_t black[4];       /* by CFA position                                                   */
    uint16_t abs_thr[4];     /* by CFA position                                                   */
    const uint32_t *list;    /* DEVICE memory, 4-byte aligned: y << 16 | x; NULL with nlist 0     */
    uint32_t *counts;        /* DEVICE memory, 4-byte aligned: n x (hot[4], cold[4]); or NULL     */
    uint32_t reserved[2];    /* must be 0                                                         */
} mcraw_fixpix;              /* sizeof 56; rank 4, rel_thr 8, nlist 12, black 16, abs_thr 24, list 32, counts 40, reserved 48 */
int mcraw_fixpix_batch(mcraw_ctx *ctx, const mcraw_fixpix *f, const uint16_t *in, size_t in_pitch, size_t in_frame_stride,
                       int width, int height, int n, uint16_t *out, size_t out_pitch, size_t out_frame_stride, void *stream);

/* ---- uint16 mosaics -> denoised uint16 mosaics ----------------------------------------------------------------------------
 *
 * Noise-adaptive smoothing of `n` uint16 mosaics of width x height on the raw sensor values, where the noise follows
 * variance = S * signal + O per CFA position (Android's noiseProfile, DNG's NoiseProfile): in front of the lens-shading
 * gains, the demosaic and the transfer curve, which make that model position-dependent, correlated and non-linear.  The
 * output is a mosaic of the same black level, so everything that takes a mosaic takes the result.  Pitches and frame strides
 * count uint16 elements.  Integers only: bit-exact.
 * Neighbours.  All neighbours lie on the pixel's own lattice (the same colour for every Bayer arrangement; the call never
 * needs the CFA): the offsets (dy, dx) run over {-2R .. 2R step 2}^2 without (0, 0), R = radius: 8 neighbours at radius 1,
 * 24 at radius 2.  For each axis independently and d in {-4, -2, +2, +4} the neighbour coordinate of c is c' = c + d; if that
 * is outside [0, size), c' = c - d; if that is outside too, c' = c (the rule of the defective-pixel stage, extended to
 * distance 4).  Duplicates that the reflection makes count with their multiplicity, so frames of width or height 1 .. 8
 * are defined, not rejected.
 * Per pixel of value c at CFA position p = (y & 1) * 2 + (x & 1), in frame f, with L = 1 << lut_log2 and the table
 * t = (nluts == 1 ? 0 : f):
 *   r   = lut[t][p][min(c >> shift, L - 1)]              uint16: 4096 / (the cut-off in DN) at the pixel's level
 *   for every neighbour value a:
 *       x = min((|a - c| * r) >> 8, 16)                  |a - c| * r <= 65535 * 65535 < 2^32
 *       w = 256 - x * x                                  0 .. 256: 1 - (difference / cut-off)^2 in Q8
 *   num = 256 * c + sum(w * a)                           <= 6400 * 65535 < 2^29
 *   den = 256     + sum(w)                               256 .. 6400
 *   m   = (num + (den >> 1)) / den                       unsigned integer division (floor)
 *   out = c + (((m - c) * amount + 128) >> 8)            signed, arithmetic shift (floor); amount 256 gives m
 * out lies between c and m, so there is no clamp.  A table of all 65535 is the identity (any |a - c| >= 1 gives x = 16), a
 * table of all 0 is the reflected box mean, and a flat frame comes back bit for bit.
 * lut: the caller's DEVICE memory, 16-byte aligned, (nluts, 4, L) uint16; read by the queued kernel in stream order and never
 * copied into or cached by the context (two calls with the same pointer and new contents in between each see their own).
 * There is no in-place form: every pixel reads its neighbours.  `in` and `out` may sit at any 2-byte alignment with any pitch
 * (16-byte accesses where base, pitch and stride allow it).
 * `stream`: a hipStream_t, NULL = the context's own stream; the call queues the work and returns without synchronising.
 * It takes no decode serial and leaves the decode slots, mcraw_ctx_errors, mcraw_ctx_last_serial and the context's stage
 * alone.  n == 0 is a no-op.  The launches have no id in mcraw_ctx_kernel_ms (time them with stream events).
 * Rejected (returns < 0, mcraw_last_error says why, starting with "mcraw_denoise_batch: ", nothing is written): a NULL `d`,
 * `in`, `out` or `lut`; an odd `in` or `out` address; a `lut` that is not 16-byte aligned; width or height outside
 * 1 .. 65536; a pitch below width; n > 1 and a frame stride below (height - 1) * pitch + width; radius not 1 or 2; amount
 * outside 1 .. 256; lut_log2 outside 6 .. 10; shift above 15; nluts not 1 or n; a non-zero `reserved`; input and output
 * extents that overlap at all. */
typedef struct mcraw_denoise {
    uint32_t radius;       /* 1: the 8 neighbours at distance 2;  2: the 24 at distances 2 and 4        */
    uint32_t amount;       /* 1 .. 256: how much of the correction is applied, 256 = all                */
    uint32_t lut_log2;     /* 6 .. 10: L = 1 << lut_log2 entries per CFA position                       */
    uint32_t shift;        /* 0 .. 15: entry of a pixel of value c = min(c >> shift, L - 1)             */
    uint32_t nluts;        /* 1: one table for the batch;  n: one per frame, back to back               */
    uint32_t reserved[3];  /* must be 0                                                                 */
    const uint16_t *lut;   /* DEVICE memory, 16-byte aligned: (nluts, 4, L)                             */
} mcraw_denoise;           /* sizeof 40; amount 4, lut_log2 8, shift 12, nluts 16, reserved 20, lut 32  */
int mcraw_denoise_batch(mcraw_ctx *ctx, const mcraw_denoise *d, const uint16_t *in, size_t in_pitch, size_t in_frame_stride,
                        int width, int height, int n, uint16_t *out, size_t out_pitch, size_t out_frame_stride, void *stream);

/* ---- uint16 mosaics -> temporally merged uint16 mosaics --------------------------------------------------------------------
 *
 * Noise-adaptive merge along time of `n` uint16 mosaics of width x height that show the same scene (a burst, or the
 * neighbouring frames of a clip): output j is the base frame b = first + j, every pixel replaced by the weighted mean of
 * itself and the samples of the other frames of b's window at the same (or a shifted) position.  A sample's weight falls with
 * a motion measure over the cut-off that the denoiser's table gives at the pixel's level, so what moved is left out and the
 * result costs no resolution.  `count` outputs with their own pitch and stride; pitches and frame strides count uint16
 * elements.  Integers only: bit-exact.
 * Members.  The members of b's window are the frames t in max(0, b - before) .. min(n - 1, b + after) with t != b: clipped at
 * the ends of the batch, not wrapped; before + after <= 15.  A burst stacked onto its first frame is before = 0,
 * after = n - 1, first = 0, count = 1; a sliding video filter is before = after = T, first = 0, count = n; a clip processed
 * in overlapping batches uses first = T, count = n - 2T.
 * Shifts.  pos: NULL, or DEVICE memory (n, 2) of int16 as (y, x) per frame, the frame's global position.  The shift of member
 * t against base b is sy = (pos[t].y - pos[b].y) & ~1 and sx likewise, in int32 (the low bit is dropped towards minus
 * infinity): a shift is always even and a sample keeps its CFA position.  NULL: every shift is 0.  Member t's sample for the
 * base pixel (y, x) is a = in[t][y + sy][x + sx]; where that position is outside the frame the member weighs 0 for the pixel.
 * Motion measure.  With e(dy, dx) = in[t][y + dy + sy][x + dx + sx] - in[b][y + dy][x + dx] and e0 = e(0, 0) = a - c:
 *   support 0:  D = |e0|
 *   support 1:  s = the sum over dy, dx in -1 .. 1 of e(dy, dx); a term whose base position or member position lies outside
 *               the frame counts e0 instead (nine terms always, no reflection rule; a 1 x 1 frame is defined)
 *               D = max(min(|s| >> 3, 65535), |e0| >> 1)
 *   (the second operand is a per-pixel guard: without it an isolated outlier in a member leaks into the result)
 * Per pixel of value c at CFA position p = (y & 1) * 2 + (x & 1), with L = 1 << lut_log2 and the table
 * f = (nluts == 1 ? 0 : b) -- the denoiser's lines and the denoiser's table, so one noise table serves both stages:
 *   r   = lut[f][p][min(c >> shift, L - 1)]              uint16: 4096 / (the cut-off in DN) at the pixel's level
 *   for every member's sample a with its D:
 *       x = min((D * r) >> 8, 16)                        D * r <= 65535 * 65535 < 2^32
 *       w = 256 - x * x                                  0 .. 256; 0 where the member's position is outside the frame
 *   num = 256 * c + sum(w * a)                           <= 4096 * 65535 < 2^28
 *   den = 256 + sum(w)                                   256 .. 4096
 *   m   = (num + (den >> 1)) / den                       unsigned integer division (floor)
 *   out = c + (((m - c) * amount + 128) >> 8)            signed, arithmetic shift (floor); amount 256 gives m
 * out lies between c and m, so there is no clamp.  A table of all 65535 returns the base frames bit for bit (any D >= 1
 * gives x = 16; with support 1, D = 0 also admits e0 = +-1 under |s| < 8, and a sample one ABOVE c then rounds m up to c + 1:
 * content whose samples differ by 0 or by 2 and more comes back exactly); so does before = after = 0, and so do shifts that
 * leave the frame.  A table of all 0 with no shifts returns the rounded mean of the window, whatever `support` is.
 * lut: the caller's DEVICE memory, 16-byte aligned, (nluts, 4, L) uint16, indexed by the base frame's index in the batch; lut
 * and pos are read by the queued kernel in stream order and never copied into or cached by the context.
 * There is no in-place form.  `in` and `out` may sit at any 2-byte alignment with any pitch (16-byte accesses where base,
 * pitch, stride and shift allow it).
 * `stream`: a hipStream_t, NULL = the context's own stream; the call queues the work and returns without synchronising.
 * It takes no decode serial and leaves the decode slots, mcraw_ctx_errors, mcraw_ctx_last_serial and the context's stage
 * alone.  count == 0 or n == 0 is a no-op.  The launches have no id in mcraw_ctx_kernel_ms (time them with stream events).
 * Rejected (returns < 0, mcraw_last_error says why, starting with "mcraw_merge_batch: ", nothing is written): a NULL `m`,
 * `in`, `out` or `lut`; an odd `in`, `out` or `pos` address; a `lut` that is not 16-byte aligned; width or height outside
 * 1 .. 65536; a pitch below width; more than one frame on a side and a frame stride below (height - 1) * pitch + width;
 * before + after above 15; first + count above n; support not 0 or 1; amount outside 1 .. 256; lut_log2 outside 6 .. 10;
 * shift above 15; nluts not 1 or n; a non-zero `reserved`; input and output extents that overlap at all. */
typedef struct mcraw_merge {
    uint32_t before;       /* frames in front of the base that its window holds                         */
    uint32_t after;        /* frames behind it; before + after <= 15                                    */
    uint32_t first;        /* the base of output 0                                                      */
    uint32_t count;        /* outputs: the bases first .. first + count - 1; first + count <= n         */
    uint32_t support;      /* 0: per-pixel differences;  1: the 3x3 motion measure                      */
    uint32_t amount;       /* 1 .. 256: how much of the correction is applied, 256 = all                */
    uint32_t lut_log2;     /* 6 .. 10: L = 1 << lut_log2 entries per CFA position                       */
    uint32_t shift;        /* 0 .. 15: entry of a pixel of value c = min(c >> shift, L - 1)             */
    uint32_t nluts;        /* 1: one table for the batch;  n: one per input frame, back to back         */
    uint32_t reserved;     /* must be 0                                                                 */
    const uint16_t *lut;   /* DEVICE memory, 16-byte aligned: (nluts, 4, L)                             */
    const int16_t *pos;    /* DEVICE memory, 2-byte aligned: (n, 2) as (y, x); or NULL                  */
} mcraw_merge;             /* sizeof 56; after 4, first 8, count 12, support 16, amount 20, lut_log2 24, shift 28, nluts 32, reserved 36, lut 40, pos 48 */
int mcraw_merge_batch(mcraw_ctx *ctx, const mcraw_merge *m, const uint16_t *in, size_t in_pitch, size_t in_frame_stride,
                      int width, int height, int n, uint16_t *out, size_t out_pitch, size_t out_frame_stride, void *stream);

/* ---- uint16 mosaics -> the frames' global positions (what mcraw_merge_batch takes as `pos`) ---------------------------------
 *
 * Estimates, for `n` uint16 mosaics of width x height that show the same scene, one global shift per frame: a coarse-to-fine
 * search of the smallest sum of absolute differences between grey planes of half the mosaic's size.  The result is the
 * (n, 2) int16 array that mcraw_merge_batch reads as `pos`, so a hand-held clip is merged along its motion.  Pitches and frame
 * strides count uint16 elements.  Integers only: bit-exact, whatever the order of the additions.
 * Grey plane.  Frame f gives G0[f] of h0 = height / 2 rows by w0 = width / 2 columns (floor: a trailing odd row or column is
 * not looked at), stored as uint16; with s the sample at CFA position p = (row & 1) * 2 + (col & 1):
 *   G0[y][x] = min((sum over the 4 samples of quad (y, x) of max(s - black[p], 0) + 2) >> 2, 65535)
 * Pyramid.  Levels 0 .. levels - 1, h(l+1) = h(l) / 2, w(l+1) = w(l) / 2 (floor):
 *   G(l+1)[y][x] = (the 4 samples of G(l) in quad (y, x), summed, + 2) >> 2
 * Bounds.  B(l) bounds the displacement at level l and is the margin of the comparison window, so every candidate of a
 * level is summed over the same pixels:
 *   B(levels - 1) = radius
 *   B(l) = 2 * B(l + 1) + 1
 * One pair, base b and member t.  At level l, for a displacement (dy, dx), exact in 64 bits:
 *   SAD_l(dy, dx) = sum over B(l) <= y < h(l) - B(l), B(l) <= x < w(l) - B(l) of |G_l[t][y + dy][x + dx] - G_l[b][y][x]|
 * At the coarsest level the centre is (0, 0) and the candidates are dy, dx in -radius .. radius about it; at each finer level
 * the centre is twice the winner of the level above and the candidates are -1 .. 1 about it.  With (ddy, ddx) the offset
 * from the centre, the winner is the candidate with the smallest
 *   key = (SAD, ddy * ddy + ddx * ddx, ddy, ddx)
 * compared lexicographically: a flat or an identical pair gives (0, 0).  d(t|b) is the level-0 winner, in quads (2 samples).
 * Sign.  d(t|b) is the (dy, dx) for which in[t][y + 2 dy][x + 2 dx] looks like in[b][y][x]: the meaning of pos[t] - pos[b]
 * in mcraw_merge_batch.
 * Positions, accumulated in int32:
 *   ref = -1 (chain):    pos[0] = (0, 0),   pos[t] = pos[t - 1] + 2 * d(t|t - 1)       the pairs are (t - 1, t)
 *   ref in 0 .. n - 1:   pos[ref] = (0, 0), pos[t] = 2 * d(t|ref)                      the pairs are (ref, t): a burst
 * stored as int16 (n, 2) as (y, x), each component clamped to -32768 .. 32767.  Differences across a clamped entry are
 * meaningless: a chain that drifts that far is to be cut into pieces by the caller.  (The int32 sums themselves cannot wrap
 * below 3.7 million frames: a step is at most 2 * B(0) <= 574.)
 * sad: NULL, or DEVICE memory, 8-byte aligned, n uint64: the level-0 winning SAD of the frame's pair, 0 for the frame that
 * has no pair (frame 0 of a chain, frame ref).  A scene cut shows as a jump.  The window has
 * (h0 - 2 * B(0)) * (w0 - 2 * B(0)) pixels, which normalises it.
 * work: the caller's DEVICE memory, 16-byte aligned, of at least mcraw_align_work_bytes(width, height, n, levels, radius)
 * bytes (0 for arguments the call would reject): the pyramids, the candidates' 64-bit sums and the levels' winners.  The call
 * initialises what it accumulates into, on the stream; nothing is cached in the context, and two calls under way at once
 * need two scratch areas.  pos, sad and work are written in stream order; no level waits for the host.
 * `in` may sit at any 2-byte alignment with any pitch (16-byte loads where base, pitch and stride allow it); it is read once.
 * `stream`: a hipStream_t, NULL = the context's own stream; the call queues the work and returns without synchronising.
 * It takes no decode serial and leaves the decode slots, mcraw_ctx_errors, mcraw_ctx_last_serial and the context's stage
 * alone.  n == 0 is a no-op; n == 1 writes (0, 0).  The launches have no id in mcraw_ctx_kernel_ms (time them with stream
 * events).
 * One shift per frame: local or tile-wise motion and rotation are mcraw_align_cells_batch's, which takes this call's result as its
 * centre.  Out of scope: precision below a quad (the merge drops the low bit of a shift anyway), a region of interest, and
 * reading gyro metadata.
 * Rejected (returns < 0, mcraw_last_error says why, starting with "mcraw_align_batch: ", nothing is written): a NULL `a`,
 * `in`, `pos` or `work`; an odd `in` or `pos` address; a `sad` that is not 8-byte aligned; a `work` that is not 16-byte
 * aligned; width or height outside 1 .. 65536; a pitch below width; n > 1 and a frame stride below (height - 1) * pitch +
 * width; levels outside 1 .. 6; radius outside 1 .. 8; ref outside -1 .. n - 1; a non-zero `reserved`; a window that is
 * empty at any level (h(l) - 2 * B(l) < 1 or w(l) - 2 * B(l) < 1); work_bytes below mcraw_align_work_bytes(...); `work`,
 * `pos` or `sad` overlapping the input's extent or one another. */
typedef struct mcraw_align {
    uint32_t levels;       /* 1 .. 6: levels of the pyramid                                             */
    uint32_t radius;       /* 1 .. 8: the search radius at the coarsest level, in its pixels            */
    int32_t ref;           /* -1: a chain, frame t against frame t - 1;  0 .. n - 1: all against ref    */
    uint32_t reserved;     /* must be 0                                                                 */
    uint16_t black[4];     /* by CFA position                                                           */
    int16_t *pos;          /* DEVICE memory, 2-byte aligned: (n, 2) as (y, x), written                  */
    uint64_t *sad;         /* DEVICE memory, 8-byte aligned: n, written; or NULL                        */
    void *work;            /* DEVICE memory, 16-byte aligned: scratch of work_bytes bytes               */
    size_t work_bytes;     /* at least mcraw_align_work_bytes(width, height, n, levels, radius)         */
} mcraw_align;             /* sizeof 56; radius 4, ref 8, reserved 12, black 16, pos 24, sad 32, work 40, work_bytes 48 */
size_t mcraw_align_work_bytes(int width, int height, int n, uint32_t levels, uint32_t radius);
int mcraw_align_batch(mcraw_ctx *ctx, const mcraw_align *a, const uint16_t *in, size_t in_pitch, size_t in_frame_stride,
                      int width, int height, int n, void *stream);

/* ---- uint16 mosaics -> a field of local positions, one per cell of every frame, and the merge that follows it ----------------
 *
 * The position field.  A cell is cell_h x cell_w samples of the mosaic: cell_w a multiple of 256 and cell_h a multiple of 32
 * (each at most 65536), so that no tile of the merge straddles a cell and a cell is a whole number of pixels at pyramid levels
 * 0 .. 2; anything else is rejected.  cells_y = ceil(height / cell_h), cells_x = ceil(width / cell_w): the last row and column
 * of cells may be partial.  A field is DEVICE memory, 2-byte aligned, (n, cells_y, cells_x, 2) int16 as (y, x): the position of
 * that cell of that frame, with the meaning of `pos` in mcraw_merge_batch.  Roll of a hand-held camera, rolling-shutter wobble
 * and parallax move the parts of a frame against each other; one shift per frame leaves everything off the dominant motion to
 * the merge's weights, which can only reject it.
 *
 * mcraw_align_cells_batch estimates the field.  Integers only: bit-exact, whatever the order of the additions.  Pitches and
 * frame strides count uint16 elements.
 * Grey plane and pyramid.  G0 and G(l + 1) of mcraw_align_batch, word for word (the same black[4], the same rounding, built by
 * the same kernel); levels in 1 .. 3; h(l) = height >> (l + 1), w(l) = width >> (l + 1), and a plane may be empty.
 * Pairs.  As in mcraw_align_batch: ref = -1 gives the chain (t - 1, t), ref = r gives (r, t).
 * Centre.  gpos: NULL (zeros), or DEVICE memory, 2-byte aligned, (n, 2) int16 as (y, x), read in stream order: the global
 * estimate, what mcraw_align_batch writes.  For the pair (b, t), g = (gpos[t] - gpos[b]) >> 1 per component, in int32 with an
 * arithmetic shift (quads); the centre at the coarsest level K - 1 = levels - 1 is g >> (K - 1) (arithmetic).
 * Per cell (i, j), level l, displacement (dy, dx), exact in 64 bits:
 *   SAD = sum over the cell's pixels (y, x) of G_l[b] of |G_l[t][clamp(y + dy, 0, h(l) - 1)][clamp(x + dx, 0, w(l) - 1)] - G_l[b][y][x]|
 * The cell's pixels at level l are the rows (i * cell_h) >> (l + 1) up to min(((i + 1) * cell_h) >> (l + 1), h(l)), and the
 * columns likewise with j, cell_w and w(l).  A cell with no pixel at a level has SAD 0 for every candidate.  Coordinates are
 * clamped (edge replicate): there is no margin, and border cells are defined like all others.
 * Search.  The candidates are -radius .. radius (radius 1 .. 4) about the centre at level K - 1, and -1 .. 1 about twice the
 * winner at each finer level.  With (ddy, ddx) the offset from the level's centre, the winner is the candidate with the smallest
 *   key = (SAD, ddy * ddy + ddx * ddx, ddy, ddx)
 * compared lexicographically (mcraw_align_batch's key), so a flat or an identical cell keeps its centre.  d(t|b)[i][j] is the
 * level-0 winner in quads, absolute (the centre included).
 * Field, accumulated in int32 per cell, mcraw_align_batch's formulas cell by cell:
 *   ref = -1 (chain):    pos[0][i][j] = (0, 0),   pos[t][i][j] = pos[t - 1][i][j] + 2 * d(t|t - 1)[i][j]
 *   ref in 0 .. n - 1:   pos[ref][i][j] = (0, 0), pos[t][i][j] = 2 * d(t|ref)[i][j]
 * each component clamped to -32768 .. 32767 on store.  (A step is below 2^16 + 64, so the int32 sums cannot wrap below 32 000
 * frames.)  Chaining per cell ignores that the content of a cell drifts between cells over a long chain: the sum at cell (i, j)
 * adds steps that were measured where the content was at each frame's own cell (i, j), not where the base frame's content has
 * gone.  This is exact for ref = r, and a second-order error over a merge window (the drift inside a window times the field's
 * gradient).
 * sad: NULL, or DEVICE memory, 8-byte aligned, (n, cells_y, cells_x) uint64: the level-0 winning SAD, 0 where a frame has no
 * pair.
 * work: the caller's DEVICE memory, 16-byte aligned, of at least mcraw_align_cells_work_bytes(width, height, n, levels, radius,
 * cell_h, cell_w) bytes (0 for arguments the call would reject): the pyramids, the candidates' 64-bit sums per cell and the
 * levels' winners.  The call initialises what it accumulates into, on the stream; nothing is cached in the context, and two
 * calls under way at once need two scratch areas.  pos, sad and work are written in stream order; no level waits for the host.
 * `stream`: a hipStream_t, NULL = the context's own stream; the call queues the work and returns without synchronising.  It
 * takes no decode serial and leaves the decode slots, mcraw_ctx_errors, mcraw_ctx_last_serial and the context's stage alone.
 * n == 0 is a no-op; n == 1 writes zeros.  The launches have no id in mcraw_ctx_kernel_ms (time them with stream events).
 * Rejected (returns < 0, mcraw_last_error says why, starting with "mcraw_align_cells_batch: ", nothing is written): a NULL `a`,
 * `in`, `pos` or `work`; an odd `in`, `pos` or `gpos` address; a `sad` that is not 8-byte aligned; a `work` that is not
 * 16-byte aligned; width or height outside 1 .. 65536; a pitch below width; n > 1 and a frame stride below (height - 1) * pitch
 * + width; levels outside 1 .. 3; radius outside 1 .. 4; ref outside -1 .. n - 1; cell_h no multiple of 32 or cell_w no
 * multiple of 256 in 1 .. 65536; a non-zero `reserved`; work_bytes below mcraw_align_cells_work_bytes(...); `work`, `pos` or
 * `sad` overlapping the input's extent or one another; `gpos` overlapping `pos`, `sad` or `work`.
 * The steps that follow, not done here: precision below a quad (the merge drops the low bit); cells smaller than a merge tile;
 * smoothing or regularising the field; pairwise estimation of every (base, member) pair of a sliding window; gyro metadata; a
 * cells path for the resampling demosaic's stabilisation window. */
typedef struct mcraw_align_cells {
    uint32_t levels;       /* 1 .. 3: levels of the pyramid                                             */
    uint32_t radius;       /* 1 .. 4: the search radius at the coarsest level, in its pixels            */
    int32_t ref;           /* -1: a chain, frame t against frame t - 1;  0 .. n - 1: all against ref    */
    uint32_t reserved;     /* must be 0                                                                 */
    uint32_t cell_h;       /* a multiple of 32                                                          */
    uint32_t cell_w;       /* a multiple of 256                                                         */
    uint16_t black[4];     /* by CFA position                                                           */
    const int16_t *gpos;   /* DEVICE memory, 2-byte aligned: (n, 2) as (y, x), the centres; or NULL     */
    int16_t *pos;          /* DEVICE memory, 2-byte aligned: (n, cells_y, cells_x, 2), written          */
    uint64_t *sad;         /* DEVICE memory, 8-byte aligned: (n, cells_y, cells_x), written; or NULL    */
    void *work;            /* DEVICE memory, 16-byte aligned: scratch of work_bytes bytes               */
    size_t work_bytes;     /* at least mcraw_align_cells_work_bytes(...)                                */
} mcraw_align_cells;       /* sizeof 72; radius 4, ref 8, reserved 12, cell_h 16, cell_w 20, black 24, gpos 32, pos 40, sad 48, work 56, work_bytes 64 */
size_t mcraw_align_cells_work_bytes(int width, int height, int n, uint32_t levels, uint32_t radius, uint32_t cell_h, uint32_t cell_w);
int mcraw_align_cells_batch(mcraw_ctx *ctx, const mcraw_align_cells *a, const uint16_t *in, size_t in_pitch, size_t in_frame_stride,
                            int width, int height, int n, void *stream);

/* mcraw_merge_cells_batch is mcraw_merge_batch, word for word, except for the shift of member t at the base pixel (y, x), which
 * comes from a position field F = cells->pos:
 *   sy = (F[t][y / cell_h][x / cell_w].y - F[b][y / cell_h][x / cell_w].y) & ~1, and sx likewise
 * All nine terms of support 1 use the shift of the base pixel's own cell, also where a neighbour lies in the next cell (what a
 * tile that stages its own halo computes); "outside the frame" keeps its meaning, with that shift.  m->pos must be NULL.  A
 * field that is the same in every cell gives mcraw_merge_batch with that `pos`, bit for bit.  The field is read by the queued
 * kernel in stream order and never copied.
 * Rejected, each starting with "mcraw_merge_cells_batch: " and with nothing written: everything mcraw_merge_batch rejects; a
 * NULL `cells`; a non-NULL m->pos; cell_h no multiple of 32 or cell_w no multiple of 256; cells_y or cells_x that are not
 * ceil(height / cell_h), ceil(width / cell_w); a non-zero cells->reserved; a NULL or odd cells->pos; a field overlapping the
 * output's extent. */
typedef struct mcraw_cells {
    uint32_t cell_h;       /* a multiple of 32                                                          */
    uint32_t cell_w;       /* a multiple of 256                                                         */
    uint32_t cells_y;      /* ceil(height / cell_h)                                                     */
    uint32_t cells_x;      /* ceil(width / cell_w)                                                      */
    uint32_t reserved;     /* must be 0                                                                 */
    const int16_t *pos;    /* DEVICE memory, 2-byte aligned: (n, cells_y, cells_x, 2) as (y, x)         */
} mcraw_cells;             /* sizeof 32; cell_w 4, cells_y 8, cells_x 12, reserved 16, pos 24 */
int mcraw_merge_cells_batch(mcraw_ctx *ctx, const mcraw_merge *m, const mcraw_cells *cells, const uint16_t *in, size_t in_pitch,
                            size_t in_frame_stride, int width, int height, int n, uint16_t *out, size_t out_pitch,
                            size_t out_frame_stride, void *stream);

/* ---- uint16 mosaics -> uint16 mosaics with the clipped highlights neutralised or rebuilt ------------------------------------
 *
 * A clipped sensor reaches the colour stage as (gain_r, gain_g, gain_b) x range, and a colour matrix with negative off-diagonal
 * terms turns that magenta.  This stage sits in front of the lens-shading gains (which move the clip level by position) and of
 * the demosaic, and either clips every CFA position to the lowest white-balanced clip level (MCRAW_HL_CLIP: a blown region becomes
 * exactly neutral) or rebuilds the clipped samples from their unclipped neighbours of the other colours (MCRAW_HL_REBUILD).  The
 * output is a mosaic of the same black level whose samples may exceed `sat`: everything that takes a mosaic takes it, and with
 * the demosaic's `white` left as it was the rebuilt samples map above 1.0 in front of the matrix.  Pitches and frame strides count
 * uint16 elements.  Integers only: bit-exact.
 * By CFA position p = (y & 1) * 2 + (x & 1): black[4]; sat[4], a sample s >= sat[p] is clipped, sat[p] > black[p]; gain[4], the
 * white-balance gain in Q4.12 (4096 is 1.0), 256 .. 65535; lo[4], used by the measure call only.  cfa: MCRAW_CFA_*, which says
 * which two positions are green (RGGB and BGGR: 1 and 2; GRBG and GBRG: 0 and 3).  top: 1 .. 65535.  The host derives
 *   inv[p] = ((1 << 24) + gain[p] / 2) / gain[p]                                            256 .. 65536
 * Width and height are 2 .. 65536, odd sizes are fine.  Neighbour coordinates reflect as -1 -> 1 and n -> n - 2, for rows and
 * columns independently, which keeps the CFA parity (hence no size of 1).
 * The white-balanced value of a sample s at position q:
 *   d = max(s - black[q], 0);   v = (d * gain[q] + 2048) >> 12          d * gain + 2048 < 2^32 and v < 2^20: uint32 suffices
 * The reference at a pixel, from the v of its eight neighbours:
 *   Hm = (left + right + 1) >> 1;   Vm = (up + down + 1) >> 1;   Dm = (the four diagonals + 2) >> 2
 *   at a green position  ref = (Hm + Vm + 1) >> 1                         the two other colours (the diagonals are green again)
 *   at a red or blue one ref = (((Hm + Vm + 1) >> 1) + Dm + 1) >> 1       the mean of green and the opposite colour
 * Measure (mcraw_highlights_measure_batch) writes records of int64 sum[4]; uint32 cnt[4]; uint32 pad[4] (64 bytes, indexed by p,
 * pad written as 0) to `rec`, 8-byte aligned DEVICE memory: nrec == n, one per frame, or nrec == 1, one for the whole batch.
 * A pixel of the frame takes part when lo[p] <= s < sat[p] and all eight neighbours are below their own sat; for each such
 * pixel sum[p] += v - ref and cnt[p] += 1.  |v - ref| < 2^20 and a frame has at most 2^30 samples per position, so the sums fit;
 * integer sums do not depend on the order.  The call initialises the records itself on the stream; with MCRAW_HL_ACCUMULATE in
 * `flags` it adds to what is there instead (one record over a clip, against flicker; cnt then wraps modulo 2^32).
 * mode, top and `out` mean nothing to it, but mode and top are checked all the same.
 * Apply (mcraw_highlights_batch), by `mode`:
 *   MCRAW_HL_CLIP     m = min over p of (((sat[p] - black[p]) * gain[p] + 2048) >> 12)
 *                     cap[p] = black[p] + ((m * inv[p] + 2048) >> 12)     in uint64 on the host
 *                     out = min(s, cap[p])                                never raises a sample; rec, nrec and top unused
 *   MCRAW_HL_REBUILD  chroma[p] = cnt[p] ? sum[p] / cnt[p] : 0, C's int64 division (towards zero), then clamped to
 *                     -2^20 .. 2^20 (a record that the measure call wrote never reaches that); of the frame's record, of
 *                     record 0 with nrec == 1, 0 with rec == NULL and nrec == 0.
 *                     An unclipped sample is copied bit for bit.  A clipped one with cand = ref + chroma[p] <= v (signed) too.
 *                     Otherwise out = max(s, min(black[p] + ((cand * inv[p] + 2048) >> 12), top)), the product in uint64
 *                     (cand <= 2^21, inv <= 65536).  It never lowers a sample.
 * MCRAW_HL_ACCUMULATE in `flags` means nothing to the apply call.  The apply kernel reads the records and does the four
 * divisions itself, so measure and apply are queued back to back with no host round trip between them.
 * `rec` is the caller's memory, read (written) by the queued kernels in stream order and never copied into or cached by the
 * context (two calls with the same pointer and new contents in between each see their own).
 * There is no in-place form: every pixel reads its neighbours.  `in` and `out` may sit at any 2-byte alignment with any pitch
 * (16-byte accesses where base, pitch and stride allow it).
 * `stream`: a hipStream_t, NULL = the context's own stream; the calls queue the work and return without synchronising.
 * They take no decode serial and leave the decode slots, mcraw_ctx_errors, mcraw_ctx_last_serial and the context's stage
 * alone.  n == 0 is a no-op.  The launches have no id in mcraw_ctx_kernel_ms (time them with stream events).
 * Rejected (returns < 0, mcraw_last_error says why, starting with the function's name and ": ", nothing is written): a NULL `h`,
 * `in` or `out`; an odd `in` or `out` address; width or height outside 2 .. 65536; a pitch below width; n > 1 and a frame stride
 * below (height - 1) * pitch + width; an unknown mode, cfa or flag; gain[p] < 256; sat[p] <= black[p]; top outside 1 .. 65535;
 * nrec not 0, 1 or n (measure: not 1 or n); a NULL `rec` with nrec > 0, a non-NULL one with nrec == 0, or one that is not 8-byte
 * aligned; a non-zero `reserved`; input and output extents that overlap at all; records that overlap either extent. */
#define MCRAW_HL_CLIP 0u        /* mode: min(s, cap[p])                                          */
#define MCRAW_HL_REBUILD 1u     /* mode: clipped samples from their neighbours' colour           */
#define MCRAW_HL_ACCUMULATE 1u  /* flags: the measure call adds to the records that are there    */
typedef struct mcraw_highlights {
    uint32_t mode;           /* MCRAW_HL_CLIP or MCRAW_HL_REBUILD                                 */
    uint32_t cfa;            /* MCRAW_CFA_*                                                       */
    uint32_t flags;          /* MCRAW_HL_ACCUMULATE or 0                                          */
    uint32_t top;            /* 1 .. 65535: the largest sample REBUILD writes                     */
    uint16_t black[4];       /* by CFA position                                                   */
    uint16_t sat[4];         /* by CFA position: s >= sat[p] is clipped; above black[p]           */
    uint16_t gain[4];        /* by CFA position, Q4.12, 256 .. 65535                              */
    uint16_t lo[4];          /* by CFA position: measure takes lo[p] <= s < sat[p]                */
    void *rec;               /* DEVICE memory, 8-byte aligned: nrec records of 64 bytes; or NULL  */
    uint32_t nrec;           /* 0 (no record: chroma 0), 1 (one for the batch) or n (per frame)   */
    uint32_t reserved;       /* must be 0                                                         */
} mcraw_highlights;          /* sizeof 64; cfa 4, flags 8, top 12, black 16, sat 24, gain 32, lo 40, rec 48, nrec 56, reserved 60 */
int mcraw_highlights_measure_batch(mcraw_ctx *ctx, const mcraw_highlights *h, const uint16_t *in, size_t in_pitch,
                                   size_t in_frame_stride, int width, int height, int n, void *stream);
int mcraw_highlights_batch(mcraw_ctx *ctx, const mcraw_highlights *h, const uint16_t *in, size_t in_pitch, size_t in_frame_stride,
                           int width, int height, int n, uint16_t *out, size_t out_pitch, size_t out_frame_stride, void *stream);

/* ---- environment ------------------------------------------------------------------------------
 * Read when a context (or pool) is created, never afterwards:
 *   MCRAW_DEVICE=n, MCRAW_DEVICES=all|0,1,5   default device of the five-argument entry points / members of a default pool
 *   MCRAW_XCD_CHUNK=n                          pins the tile kernel's workgroup-to-XCD mapping (mcraw_ctx_xcd_runs)
 *   MCRAW_SIDE_SPLIT=b[,r]                     pins the workgroups per bits / refs side stream (mcraw_ctx_side_parts)
 *   MCRAW_SIDE_LASTC=0|1                       the last part of a split side stream counts its pieces too (default: by batch size)
 *   MCRAW_SHORT_WAY=0|1                        host-memory pipeline: status words fetched at the wait / written home behind the
 *                                              kernels (default: every context measures which is faster in its process)
 *   MCRAW_TRACE=1                              the verdicts of the contexts' own measurements on stderr
 * Of the HIP runtime (docs/lab_notes.md): GPU_MAX_HW_QUEUES (hardware queues per process and priority). */

/* Pinned host memory for MCRAW_MEM_HOST batches (hipHostMalloc / hipHostFree). */
void *mcraw_host_alloc(size_t bytes);
void mcraw_host_free(void *p);

#ifdef __cplusplus
}
#endif
#endif /* MCRAW_HIP_H */
