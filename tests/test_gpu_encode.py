"""GPU: the type-7 encoder (mcraw_encode_batch / mcraw_encode7) writes byte for byte what the synthesiser's canonical
encoder writes (synthlib.encode7 = mcraw_synth_encode7 with no forced classes, flags 0), and its frames decode back to
their input on the device, through the oracle and through the reference decoder.  The look-back between a frame's
segments is checked under uneven load (mixed batches, 240 UHD frames, two contexts at once); pointers of any byte
alignment, host memory, the len_out words, the capacity check and the independence of the decode side's state."""
import threading

import numpy as np
import pytest
import torch

import _libs as L
import motioncam_decoder_amd as M
from _enc7_model import BIG65, BIG130, KINDS, SHAPES, classes_image, content, records_image  # noqa: F401  (the corpus lives with its model)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def encode_device(ctx, imgs, out_off=0, in_off=0, with_len=False, want_status=True, fill=0xA5):
    """Encode every image (HBM-resident in and out); returns (written, status, [np.uint8 encoded], [len_out])."""
    ins, outs, descs = [], [], []
    lens = torch.zeros(max(len(imgs), 1), dtype=torch.int64, device=DEV) if with_len else None
    for i, img in enumerate(imgs):
        h, w = img.shape
        flat = np.zeros(w * h + 8, dtype=np.uint16)
        flat[in_off: in_off + w * h] = img.reshape(-1)
        ti = _dev(flat)
        cap = M.encode_bound7(w, h)
        to = torch.full((cap + out_off + 64,), fill, dtype=torch.uint8, device=DEV)
        ins.append(ti)
        outs.append(to)
        descs.append((ti.data_ptr() + 2 * in_off, w, h, to.data_ptr() + out_off, cap,
                      lens.data_ptr() + 8 * i if with_len else None))
    torch.cuda.synchronize()
    frames = M.Context.make_enc_frames(descs)
    res = ctx.encode_batch(frames, mem=M.MEM_DEVICE, want_status=want_status)
    torch.cuda.synchronize()
    got = [to.cpu().numpy()[out_off:] for to in outs]
    lo = [int(v) for v in lens.cpu().numpy()] if with_len else None
    if want_status:
        written, status = res
    else:
        written, status = lo, [0] * len(imgs)
    return written, status, got, lo, outs


def check_equal(img, written, status, got, what=""):
    want = L.encode7(img)
    assert status == 0, (what, img.shape, status)
    assert written == len(want), (what, img.shape, written, len(want))
    g = got[:written]
    if not np.array_equal(g, want):
        bad = np.nonzero(g != want)[0]
        raise AssertionError("%s %s: %d bytes differ, first at %d" % (what, img.shape, bad.size, bad[0]))
    assert (got[written: written + 64] == 0xA5).all(), "bytes written behind the frame"


@pytest.mark.parametrize("kind", KINDS)
def test_bytes_equal_small_shapes(gpu_ctx, kind):
    imgs = [content(kind, w, h, 11 + i) for i, (w, h) in enumerate(SHAPES)]
    written, status, got, _, _ = encode_device(gpu_ctx, imgs)
    for img, wr, st, g in zip(imgs, written, status, got):
        check_equal(img, wr, st, g, kind)


@pytest.mark.parametrize("shape", [(4032, 3024), (3840, 2160), (7680, 4320)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", ["nat12", "uni16", "zero"])
def test_bytes_equal_large(gpu_ctx, shape, kind):
    w, h = shape
    img = content(kind, w, h, 3)
    written, status, got, _, _ = encode_device(gpu_ctx, [img])
    check_equal(img, written[0], status[0], got[0], kind)


def test_every_class_occurs(gpu_ctx):
    img = classes_image()
    want = L.encode7(img)
    bits = decode_bits(want, (256 // 64) * (64 // 4) * 4)
    assert set(bits) == set(range(17)), sorted(set(bits))
    written, status, got, _, _ = encode_device(gpu_ctx, [img])
    check_equal(img, written[0], status[0], got[0], "classes")


def test_every_record_class_occurs(gpu_ctx):
    """28 side-stream records made for their header classes: refs records of every class 0..15 (with the 12-bit ref clamp at
    4095, 4096, 50000 and 65535), bits records of every class 0..5 (tests/test_enc7_model.py checks that on the synthesiser)."""
    img = records_image()
    written, status, got, _, _ = encode_device(gpu_ctx, [img])
    check_equal(img, written[0], status[0], got[0], "records")


def test_segment_behind_the_first_window(gpu_ctx):
    """1024 x 1028: 65 segments (one look-back of more than a window of 64) and 257 records (one in k7e_side's second chunk)."""
    kind, w, h, seed = BIG65
    img = content(kind, w, h, seed)
    written, status, got, _, _ = encode_device(gpu_ctx, [img])
    check_equal(img, written[0], status[0], got[0], "65 segments")


def test_big_tiny_big_on_one_context():
    """The workspace's strides (segments and records of the batch's largest frame) shrink and grow over stale contents."""
    ctx = M.Context(0)
    kind, w, h, seed = BIG130
    big, tiny = content(kind, w, h, seed), content("zero", 1, 1, 0)
    for img in (big, tiny, big):
        written, status, got, _, _ = encode_device(ctx, [img])
        check_equal(img, written[0], status[0], got[0], "big / tiny / big")
    ctx.close()


def test_fresh_workspace_is_zeroed_in_front_of_its_first_kernels():
    """A context's first encode batch allocates its workspace and zeroes it.  The zeros must be written in order with the batch's
    kernels, whatever the null stream is busy with: a context's streams do not wait for the null stream, and a hipMemset of
    device memory returns before it has run (measured on an MI355X: back after 0.012 ms with the null stream busy for another
    20.8 ms).  Zeroed there, the workspace of test_two_contexts_two_threads was cleared behind the other thread's fills, under
    the running kernels: one frame of one run came back 33360 bytes short with status 0.  Here the null stream spins while a
    fresh context encodes its first batch; a context that encoded another frame of the same shape at the same epoch was closed
    just before, so memory handed out again would hold its look-back words, record headers and totals.  (The old code passed
    this in its one run -- the allocator handed out other memory, and zeros that arrive behind the kernels do no harm; what
    this pins is the condition, the order is in encode_device.)"""
    kind, w, h, seed = BIG65
    first, second = content("uni8", w, h, seed + 1), content(kind, w, h, seed)
    ctx = M.Context(0)
    written, status, got, _, _ = encode_device(ctx, [first])
    check_equal(first, written[0], status[0], got[0], "first context")
    ctx.close()
    ctx = M.Context(0)
    cap = M.encode_bound7(w, h)
    ti, to = _dev(second), torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    frames = M.Context.make_enc_frames([(ti.data_ptr(), w, h, to.data_ptr(), cap)])
    torch.cuda.synchronize()
    torch.cuda._sleep(20_000_000)  # (a few milliseconds on the null stream; the call returns at once)
    written, status = ctx.encode_batch(frames)
    torch.cuda.synchronize()
    check_equal(second, written[0], status[0], to.cpu().numpy(), "second context")
    ctx.close()


def decode_bits(buf, nblk):
    """The bits stream's first nblk entries (records of 64 entries: {hb << 4 | ref >> 8, ref & 255}, block at class hb)."""
    off = int(np.frombuffer(buf[8:12].tobytes(), "<u4")[0])
    rec = off + 4
    out = []
    while len(out) < nblk:
        hb, ref = buf[rec] >> 4, ((buf[rec] & 15) << 8) | buf[rec + 1]
        rec += 2
        vals = unpack_block(buf[rec:], hb)
        out.extend(int(v) + ref for v in vals)
        rec += [0, 8, 16, 24, 32, 40, 48, 64, 64, 80, 80, 128, 128, 128, 128, 128][hb]
    return out[:nblk]


def unpack_block(p, bits):
    """Entries of a side-stream record stored at `bits` <= 5 (what a bits stream uses)."""
    P = lambda i, j: int(p[8 * i + j])  # noqa: E731
    v = [0] * 64
    for j in range(8):
        if bits == 0:
            pass
        elif bits == 1:
            for k in range(8):
                v[8 * k + j] = (P(0, j) >> k) & 1
        elif bits == 2:
            for h in range(2):
                for k in range(4):
                    v[32 * h + 8 * k + j] = (P(h, j) >> (2 * k)) & 3
        elif bits == 3:
            v[j], v[8 + j], v[16 + j] = P(0, j) & 7, (P(0, j) >> 3) & 7, ((P(0, j) >> 6) & 3) | (((P(2, j) >> 6) & 1) << 2)
            v[24 + j], v[32 + j], v[40 + j] = P(1, j) & 7, (P(1, j) >> 3) & 7, ((P(1, j) >> 6) & 3) | (((P(2, j) >> 7) & 1) << 2)
            v[48 + j], v[56 + j] = P(2, j) & 7, (P(2, j) >> 3) & 7
        elif bits == 4:
            for g in range(4):
                v[16 * g + j], v[16 * g + 8 + j] = P(g, j) & 15, P(g, j) >> 4
        elif bits == 5:
            for i in range(5):
                v[8 * i + j] = P(i, j) & 31
            v[40 + j] = (P(0, j) >> 5) | (((P(3, j) >> 5) & 3) << 3)
            v[48 + j] = (P(1, j) >> 5) | (((P(4, j) >> 5) & 3) << 3)
            v[56 + j] = (P(2, j) >> 5) | ((P(3, j) >> 7) << 3) | ((P(4, j) >> 7) << 4)
        else:
            raise AssertionError("bits stream record class %d" % bits)
    return v


def test_round_trip_device_oracle_reference(gpu_ctx):
    imgs = [content(k, w, h, 21 + i) for i, (k, (w, h)) in enumerate(
        [("nat12", (200, 100)), ("uni16", (127, 7)), ("highref", (65, 5)), ("nat14", (640, 480)), ("zero", (64, 4)),
         ("max", (3, 5))])]
    imgs.append(classes_image())
    written, status, got, _, outs = encode_device(gpu_ctx, imgs)
    # device-resident: the encoded buffers go straight back into mcraw_decode_batch
    dec_out, descs = [], []
    for img, wr, to in zip(imgs, written, outs):
        h, w = img.shape
        o = torch.zeros(w * h * 2, dtype=torch.uint8, device=DEV)
        dec_out.append(o)
        descs.append((to.data_ptr(), wr, w, h, 7, o.data_ptr(), w * h))
    dw, ds = gpu_ctx.decode_batch(M.Context.make_frames(descs), mem=M.MEM_DEVICE)
    torch.cuda.synchronize()
    ref_ok = L.ref_path() is not None
    for img, wr, st, g, o, w2, s2 in zip(imgs, written, status, got, dec_out, dw, ds):
        h, w = img.shape
        assert st == 0 and s2 == 0 and w2 == w * h
        assert np.array_equal(o.cpu().numpy().view(np.uint16).reshape(h, w), img)
        buf = g[:wr].copy()
        ret, back = L.oracle_decode7(buf, w, h)
        assert ret == w * h and np.array_equal(back, img)
        if ref_ok and h % 4 == 0:
            ret, back = L.ref_decode7(buf, w, h)  # (rows h .. h + 3: the reference's spare rows)
            assert ret == w * h and np.array_equal(back[:h], img)


def test_mixed_batch_uneven(gpu_ctx):
    rng = np.random.default_rng(99)
    shapes = [(1, 1), (64, 4), (4032, 3024), (3840, 2160), (200, 100), (1920, 1080), (65, 5), (7680, 64), (127, 7), (640, 480)]
    kinds = ["nat12", "uni16", "zero", "nat10", "highref", "uni8", "max", "nat14"]
    imgs = []
    for i in range(100):
        w, h = shapes[int(rng.integers(0, len(shapes)))] if i % 7 else (3840, 2160)
        imgs.append(content(kinds[i % len(kinds)], w, h, 1000 + i))
    written, status, got, _, _ = encode_device(gpu_ctx, imgs)
    for img, wr, st, g in zip(imgs, written, status, got):
        check_equal(img, wr, st, g, "mixed")


def test_240_uhd_one_batch(gpu_ctx):
    w, h = 3840, 2160
    base = [L.natural_image_np(w, h, 12, 12.0, s) for s in range(4)] + [L.uniform_image_np(w, h, 16, 9)]
    want = [L.encode7(b) for b in base]
    cap = M.encode_bound7(w, h)
    ins = [_dev(b) for b in base]
    out = torch.full((240, cap), 0xA5, dtype=torch.uint8, device=DEV)
    frames = M.Context.make_enc_frames([(ins[i % 5].data_ptr(), w, h, out[i].data_ptr(), cap) for i in range(240)])
    torch.cuda.synchronize()
    written, status = gpu_ctx.encode_batch(frames)
    got = out.cpu().numpy()
    for i in range(240):
        wnt = want[i % 5]
        assert status[i] == 0 and written[i] == len(wnt), (i, status[i], written[i])
        assert np.array_equal(got[i, :written[i]], wnt), i


def test_two_contexts_two_threads():
    imgs = [L.natural_image_np(3840, 2160, 12, 6.0, 40 + i) for i in range(3)] + [L.uniform_image_np(1000, 600, 16, 5)]
    errs = []

    def run(k):
        try:
            ctx = M.Context(0)
            for rep in range(3):
                order = imgs[k:] + imgs[:k]
                written, status, got, _, _ = encode_device(ctx, order * 4)
                for img, wr, st, g in zip(order * 4, written, status, got):
                    check_equal(img, wr, st, g, "thread %d" % k)
            ctx.close()
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs


@pytest.mark.parametrize("out_off", [1, 3, 7])
def test_unaligned_output(gpu_ctx, out_off):
    imgs = [content("nat12", 200, 100, 5), content("uni16", 127, 7, 6), content("nat14", 3840, 16, 7)]
    written, status, got, _, _ = encode_device(gpu_ctx, imgs, out_off=out_off)
    for img, wr, st, g in zip(imgs, written, status, got):
        check_equal(img, wr, st, g, "out+%d" % out_off)


def test_input_2_byte_aligned(gpu_ctx):
    imgs = [content("nat12", 200, 100, 8), content("uni16", 256, 8, 9), content("nat10", 63, 3, 10)]
    for in_off in (1, 3, 5):
        written, status, got, _, _ = encode_device(gpu_ctx, imgs, in_off=in_off)
        for img, wr, st, g in zip(imgs, written, status, got):
            check_equal(img, wr, st, g, "in+%d" % (2 * in_off))


def test_host_memory_mode(gpu_ctx):
    imgs = [content("nat12", 200, 100, 12), content("uni16", 65, 5, 13), content("zero", 1, 1, 0)]
    outs = [np.full(M.encode_bound7(i.shape[1], i.shape[0]) + 3, 0xA5, dtype=np.uint8) for i in imgs]
    lens = np.zeros(len(imgs), dtype=np.uint64)
    descs = [(img.ctypes.data, img.shape[1], img.shape[0], o.ctypes.data + 3, o.size - 3, lens.ctypes.data + 8 * i)
             for i, (img, o) in enumerate(zip(imgs, outs))]
    written, status = gpu_ctx.encode_batch(M.Context.make_enc_frames(descs), mem=M.MEM_HOST)
    for i, (img, o) in enumerate(zip(imgs, outs)):
        assert int(lens[i]) == written[i]
        check_equal(img, written[i], status[i], o[3:], "host")


def test_len_out_async(gpu_ctx):
    imgs = [content("nat12", 640, 480, 14), content("uni8", 200, 100, 15), content("max", 63, 3, 0)]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        written, status, got, lens, _ = encode_device(gpu_ctx, imgs, with_len=True, want_status=False)
    for img, wr, g in zip(imgs, lens, got):
        check_equal(img, wr, 0, g, "len_out")


def test_encode7_single(gpu_ctx):
    lib = M.load()
    img = content("nat12", 200, 100, 16)
    out = np.full(M.encode_bound7(200, 100) + 16, 0xA5, dtype=np.uint8)
    n = lib.mcraw_encode7(out.ctypes.data, out.size - 16, img.ctypes.data, 200, 100)
    check_equal(img, n, 0, out, "encode7")
    assert lib.mcraw_encode7(out.ctypes.data, M.encode_bound7(200, 100) - 1, img.ctypes.data, 200, 100) == 0
    assert lib.mcraw_encode7(out.ctypes.data, out.size, img.ctypes.data, 0, 100) == 0


def test_capacity_one_byte_short(gpu_ctx):
    img = content("nat12", 200, 100, 17)
    cap = M.encode_bound7(200, 100)
    canary = torch.full((cap + 128,), 0x5A, dtype=torch.uint8, device=DEV)
    ti = _dev(img)
    frames = M.Context.make_enc_frames([(ti.data_ptr(), 200, 100, canary.data_ptr() + 64, cap - 1),
                                        (ti.data_ptr(), 0, 100, canary.data_ptr() + 64, cap)])
    torch.cuda.synchronize()
    written, status = gpu_ctx.encode_batch(frames)
    assert status[0] == M.E_CAPACITY and written[0] == 0
    assert status[1] == M.E_ARGS and written[1] == 0
    assert (canary.cpu().numpy() == 0x5A).all()


def test_decode_state_unaffected(gpu_ctx):
    """Decode batches interleaved with encode batches on one context: statuses, serials and the sticky error word are
    those of the decode batches alone."""
    ctx = M.Context(0)
    good = L.natural_image_np(256, 32, 12, 8.0, 3)
    buf = L.encode7(good)
    bad = buf.copy()
    bad[8:12] = 0xFF  # a bits-stream offset past the frame: MCRAW_E_HEADER
    keep = []

    def dec_descs():
        descs = []
        for b in (buf, bad):
            ti = _dev(b)
            to = torch.zeros(256 * 32 * 2, dtype=torch.uint8, device=DEV)
            keep.extend([ti, to])
            descs.append((ti.data_ptr(), ti.numel(), 256, 32, 7, to.data_ptr(), 256 * 32))
        return descs

    def run(with_encode):
        ctx.errors(reset=True)
        s0 = ctx.last_serial()
        seen = []
        for k in range(3):
            if with_encode:
                encode_device(ctx, [good], want_status=(k != 1), with_len=True)
            ctx.decode_batch(M.Context.make_frames(dec_descs()), mem=M.MEM_DEVICE, want_status=False)
            if with_encode:
                encode_device(ctx, [good], want_status=(k == 1), with_len=True)
            seen.append(ctx.last_serial() - s0)
        torch.cuda.synchronize()
        st = ctx.synchronize(2)
        serial = ctx.last_serial()
        return seen, st, ctx.batch_status(serial, 2), ctx.errors(reset=True)

    a = run(False)
    b = run(True)
    assert a == b, (a, b)
    assert a[1][0] == 0 and a[1][1] != 0 and a[3] != 0
    ctx.close()
