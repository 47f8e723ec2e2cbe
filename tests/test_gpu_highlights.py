"""Highlight reconstruction (mcraw_highlights_batch, mcraw_highlights_measure_batch, Context.highlights / highlight_chroma,
highlights= on the demosaic / decode methods) on the GPU: every output sample and every record equals the numpy statement of
the contract (_highlights_ref), nothing outside the output and the records is written, the input is left as it was, each queued
call reads the records' contents in stream order, and the context's decode state and the sibling entry points are undisturbed."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import _highlights_ref as HL
import _libs as L
import motioncam_decoder_amd as M

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SENT = 0xA5A5
# (H, W): the smallest, odd sizes, one below / at / above the tile (32 rows, 256 columns), a row end that is no multiple of 8, and
# several tiles both ways
GEOMS = ((2, 2), (2, 3), (3, 2), (5, 7), (31, 255), (32, 256), (33, 257), (35, 264), (70, 1002))
CFAS = ("rggb", "bggr", "grbg", "gbrg")
SRGBISH = np.array([[1.7, -0.5, -0.2], [-0.25, 1.4, -0.15], [0.05, -0.45, 1.4]], np.float32)
SAT, BLACK, GAINQ = (3000, 3100, 2900, 3050), (60, 64, 68, 72), (7800, 4096, 4200, 6100)
TOP = 3400


def _np(t):
    a = t.detach()
    if a.dtype == torch.uint16:
        return a.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    return a.cpu().numpy()


def _dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).to(DEV).view(torch.uint16)


def _frames(rng, n, H, W, sat=SAT):
    """Frames that hold, where the size allows it: isolated clipped samples, runs of them, 8-column pieces and whole tiles without
    one, a tile that is clipped throughout, clipped samples on all four edges and in the corners, and neighbourhoods that are
    brighter and darker than the clipped sample's own level (cand > v and cand <= v)."""
    satm = HL.by_position(sat, H, W)
    imgs = np.empty((n, H, W), np.int64)
    for f in range(n):
        img = np.minimum(rng.integers(200, 3600, size=(H, W)), satm - 1)
        img[:, W // 2:] = np.minimum(img[:, W // 2:] // 3 + 1900, satm[:, W // 2:] - 1)  # bright, nearly flat: neighbours above a clipped sample's level
        img = np.where(rng.random((H, W)) < 0.03, satm + rng.integers(0, 400, size=(H, W)), img)  # isolated
        for k in range(max(1, H // 6)):  # runs along a row
            y, x = int(rng.integers(0, H)), int(rng.integers(0, max(1, W - 3)))
            img[y, x:x + 24] = satm[y, x:x + 24] + 7
        if W >= 768 and H >= 64:
            img[32:64, 256:512] = np.minimum(img[32:64, 256:512], satm[32:64, 256:512] - 1)  # a tile without a clipped sample
            img[0:32, 512:768] = satm[0:32, 512:768] + 1  # a tile that is clipped throughout
        if W >= 64:
            img[:, 16:40] = np.minimum(img[:, 16:40], satm[:, 16:40] - 1)  # 8-column pieces without a clipped sample
        for y in (0, H - 1):
            for x in (0, W // 2, W - 1):
                img[y, x] = satm[y, x]  # corners and the edges' middles, exactly at sat
        img[H // 2, 0] = satm[H // 2, 0] + 1
        img[H // 2, W - 1] = 65535
        imgs[f] = img
    return np.clip(imgs, 0, 65535).astype(np.uint16)


def _census(img, rec, cfa):
    """What the frame holds, counted on the CPU with the statement's own pieces."""
    H, W = img.shape
    s = img.astype(np.int64)
    clipped = s >= HL.by_position(SAT, H, W)
    v = HL.wb(img, BLACK, GAINQ)
    cand = HL.reference(v, cfa) + HL.by_position(HL.chroma(*rec)[0], H, W)
    back = HL.by_position(BLACK, H, W) + ((np.maximum(cand, 0) * HL.by_position(HL.inv(GAINQ), H, W) + 2048) >> 12)
    nb = sum(np.pad(clipped, 1)[1 + dy:1 + dy + H, 1 + dx:1 + dx + W].astype(int) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx)
    pieces = clipped[:, :W // 8 * 8].reshape(H, W // 8, 8).any(axis=2)
    tiles = [clipped[y:y + 32, x:x + 256] for y in range(0, H - 31, 32) for x in range(0, W - 255, 256)]
    return dict(isolated=int((clipped & (nb == 0)).sum()), runs=int((clipped[:, :-2] & clipped[:, 1:-1] & clipped[:, 2:]).sum()),
                clean_pieces=int((~pieces).sum()), clean_tiles=sum(1 for t in tiles if not t.any()), full_tiles=sum(1 for t in tiles if t.all()),
                top=int(clipped[0].sum()), bottom=int(clipped[-1].sum()), left=int(clipped[:, 0].sum()), right=int(clipped[:, -1].sum()),
                corners=int(clipped[0, 0]) + int(clipped[0, -1]) + int(clipped[-1, 0]) + int(clipped[-1, -1]),
                raised=int((clipped & (cand > v)).sum()), kept=int((clipped & (cand <= v)).sum()),
                cut=int((clipped & (cand > v) & (back > TOP) & (s < TOP)).sum()), below_top=int((clipped & (cand > v) & (back < TOP)).sum()))


def test_the_content_holds_every_case():
    rng = np.random.default_rng(zlib.crc32(b"70x1002"))
    img = _frames(rng, 1, 70, 1002)[0]
    rec = HL.measure(img[None], SAT, BLACK, GAINQ, 0, HL.default_lo(SAT, BLACK))
    c = _census(img, rec, 0)
    print(c)
    assert c["corners"] == 4 and min(c.values()) >= 1, c
    assert min(c["isolated"], c["runs"], c["clean_pieces"], c["raised"], c["kept"], c["cut"], c["below_top"]) >= 20, c
    assert rec[1].min() >= 100  # every position measures


def _records(gpu_ctx, t, cfa, scope, **kw):
    return gpu_ctx.highlight_chroma(t, sat=SAT, black=BLACK, gain=GAINQ, cfa=cfa, scope=scope, **kw)


def _check_all(gpu_ctx, imgs, cfa, what=""):
    """Both calls in every form against the statement, for one batch."""
    n, H, W = imgs.shape
    code = HL.CFA[cfa]
    t = _dev16(imgs)
    lo = HL.default_lo(SAT, BLACK)
    kw = dict(sat=SAT, black=BLACK, gain=GAINQ, cfa=cfa)
    per, one = _records(gpu_ctx, t, cfa, "frame"), _records(gpu_ctx, t, cfa, "batch")
    wper, wone = HL.measure(imgs, SAT, BLACK, GAINQ, code, lo), HL.measure(imgs, SAT, BLACK, GAINQ, code, lo, nrec=1)
    outs = [gpu_ctx.highlights(t, chroma=per, top=TOP, **kw), gpu_ctx.highlights(t, chroma=one, top=TOP, **kw),
            gpu_ctx.highlights(t, chroma=None, top=TOP, **kw), gpu_ctx.highlights(t, chroma=None, **kw),
            gpu_ctx.highlights(t, mode="clip", **kw), gpu_ctx.highlights(t, chroma="frame", **kw)]
    torch.cuda.synchronize()
    assert tuple(per.raw.shape) == (n, 8) and tuple(one.raw.shape) == (1, 8)
    assert np.array_equal(per.raw.cpu().numpy(), HL.raw(*wper)), (what, cfa, per.raw.cpu().numpy().tolist(), HL.raw(*wper).tolist())
    assert np.array_equal(one.raw.cpu().numpy(), HL.raw(*wone)), (what, cfa)
    wants = [HL.apply(imgs, HL.REBUILD, SAT, BLACK, GAINQ, code, wper, TOP), HL.apply(imgs, HL.REBUILD, SAT, BLACK, GAINQ, code, wone, TOP),
             HL.apply(imgs, HL.REBUILD, SAT, BLACK, GAINQ, code, None, TOP), HL.apply(imgs, HL.REBUILD, SAT, BLACK, GAINQ, code, None),
             HL.apply(imgs, HL.CLIP, SAT, BLACK, GAINQ, code), HL.apply(imgs, HL.REBUILD, SAT, BLACK, GAINQ, code, wper)]
    for k, (o, want) in enumerate(zip(outs, wants)):
        assert tuple(o.shape) == (n, H, W) and o.dtype == torch.uint16
        bad = np.argwhere(_np(o) != want)
        assert bad.size == 0, (what, cfa, k, len(bad), bad[:4].tolist())
    assert np.array_equal(_np(t), imgs), "the input was written"


@pytest.mark.parametrize("geom", GEOMS)
def test_matches_reference(gpu_ctx, geom):
    H, W = geom
    rng = np.random.default_rng(zlib.crc32(("%dx%d" % (H, W)).encode()))
    imgs = _frames(rng, 2, H, W)
    for cfa in CFAS if H * W <= 6 else (CFAS[(H + W) % 4],):
        _check_all(gpu_ctx, imgs, cfa)


def test_extreme_parameters(gpu_ctx):
    """The largest products of the contract: full-range samples, gains 256 and 65535, sat 65535 and 1, records that drive chroma
    into its clamp either way."""
    rng = np.random.default_rng(17)
    H, W = 35, 264
    imgs = rng.integers(0, 1 << 16, size=(2, H, W), dtype=np.uint16)
    imgs[:, ::3, ::5] = 65535
    t = _dev16(imgs)
    for sat, black, gain, top in (((65535,) * 4, (0,) * 4, (256, 65535, 65535, 256), 65535), ((1, 65535, 40000, 2), (0, 65534, 0, 1), (65535, 256, 4096, 65535), 60000),
                                  ((65535,) * 4, (0,) * 4, (65535,) * 4, 1)):
        lo = HL.default_lo(sat, black)
        for k, sums in enumerate((None, np.array([[1 << 62, -(1 << 62), 1 << 20, -5]], np.int64))):
            rec = None if sums is None else (sums, np.array([[1, 1, 1, 2]], np.uint32))
            raw = None if rec is None else torch.from_numpy(HL.raw(*rec)).to(DEV)
            got = gpu_ctx.highlights(t, sat=sat, black=black, gain=gain, cfa="grbg", chroma=raw, top=top)
            clp = gpu_ctx.highlights(t, sat=sat, black=black, gain=gain, cfa="grbg", mode="clip")
            m = gpu_ctx.highlight_chroma(t, sat=sat, black=black, gain=gain, cfa="grbg")
            torch.cuda.synchronize()
            assert np.array_equal(_np(got), HL.apply(imgs, HL.REBUILD, sat, black, gain, 2, rec, top)), (sat, k)
            assert np.array_equal(_np(clp), HL.apply(imgs, HL.CLIP, sat, black, gain, 2)), (sat, k)
            assert np.array_equal(m.raw.cpu().numpy(), HL.raw(*HL.measure(imgs, sat, black, gain, 2, lo))), (sat, k)


def test_35_frames(gpu_ctx):
    rng = np.random.default_rng(35)
    _check_all(gpu_ctx, _frames(rng, 35, 33, 257), "bggr", "35 frames")


def test_accumulate_over_two_calls(gpu_ctx):
    rng = np.random.default_rng(2)
    a, b = _frames(rng, 3, 35, 264), _frames(rng, 3, 35, 264)
    lo = HL.default_lo(SAT, BLACK)
    for scope, nrec in (("frame", None), ("batch", 1)):
        rec = _records(gpu_ctx, _dev16(a), "rggb", scope)
        again = _records(gpu_ctx, _dev16(b), "rggb", scope, into=rec)
        torch.cuda.synchronize()
        assert again is rec
        want = HL.measure(b, SAT, BLACK, GAINQ, 0, lo, nrec=nrec, into=HL.measure(a, SAT, BLACK, GAINQ, 0, lo, nrec=nrec))
        assert np.array_equal(rec.raw.cpu().numpy(), HL.raw(*want)), scope
        s, c = rec.cpu()
        assert np.array_equal(s, want[0]) and np.array_equal(c, want[1])
        assert np.array_equal(rec.sum.cpu().numpy(), want[0]) and np.array_equal(rec.cnt.cpu().numpy().view(np.uint32), want[1])
    # a raw tensor does as well, and a fresh call starts anew whatever the records held
    raw = torch.full((1, 8), -1, dtype=torch.int64, device=DEV)
    fresh = gpu_ctx.highlight_chroma(_dev16(a), sat=SAT, black=BLACK, gain=GAINQ, scope="batch")
    s = M._hl_struct("t", SAT, BLACK, GAINQ, "rggb", None, 65535, "rebuild")
    s.rec, s.nrec = raw.data_ptr(), 1
    ta = _dev16(a)
    torch.cuda.synchronize()  # (the context's own stream does not wait for torch's)
    assert M.load().mcraw_highlights_measure_batch(gpu_ctx._h, C.byref(s), C.c_void_p(ta.data_ptr()), 264, 35 * 264, 264, 35, 3, None) == 0
    gpu_ctx.synchronize()
    assert torch.equal(raw, fresh.raw)  # sums, counts, and the pad written as 0


def test_same_rec_pointer_new_contents_between_queued_calls(gpu_ctx):
    rng = np.random.default_rng(9)
    imgs = _frames(rng, 2, 70, 1002)
    t = _dev16(imgs)
    recs = [(rng.integers(-300000, 300000, size=(2, 4)), rng.integers(1, 900, size=(2, 4)).astype(np.uint32)) for _ in range(4)]
    staged = [torch.from_numpy(HL.raw(*r)).to(DEV) for r in recs]
    live = torch.zeros((2, 8), dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    outs = []
    with torch.cuda.stream(s):
        for k in range(4):  # no host sync between: the records are rewritten in stream order between the calls
            live.copy_(staged[k])
            outs.append(gpu_ctx.highlights(t, sat=SAT, black=BLACK, gain=GAINQ, chroma=live, top=TOP))
        # measure then apply back to back: the apply reads what the measure queued in front of it wrote
        live2 = gpu_ctx.highlight_chroma(t, sat=SAT, black=BLACK, gain=GAINQ)
        outs.append(gpu_ctx.highlights(t, sat=SAT, black=BLACK, gain=GAINQ, chroma=live2))
    s.synchronize()
    for k in range(4):
        assert np.array_equal(_np(outs[k]), HL.apply(imgs, HL.REBUILD, SAT, BLACK, GAINQ, 0, recs[k], TOP)), k
    assert len({zlib.crc32(_np(o).tobytes()) for o in outs[:4]}) == 4  # (the records matter to the result)
    want = HL.measure(imgs, SAT, BLACK, GAINQ, 0, HL.default_lo(SAT, BLACK))
    assert np.array_equal(_np(outs[4]), HL.apply(imgs, HL.REBUILD, SAT, BLACK, GAINQ, 0, want))


def _strided(base, n, h, w, fstride, pitch, off):
    return torch.as_strided(base, (n, h, w), (fstride, pitch, 1), off).view(torch.uint16)


# (H, W, input pitch, input frame slack, input offset, output pitch, output frame slack, output offset): offsets in samples;
# 1 = an odd base address in samples (off the dword grid), 4 = on the 8-byte grid only, 8 with pitches and strides that are
# multiples of 8 = the 16-byte path; a pitch % 8 != 0 or a slack % 8 != 0 takes rows or frames off the 16-byte grid
VIEWS = ((35, 41, 53, 29, 1, 47, 3, 4), (34, 520, 520, 0, 4, 531, 17, 1), (70, 1002, 1008, 8, 8, 1016, 16, 8),
         (16, 64, 64, 0, 0, 72, 8, 1), (33, 2, 3, 5, 1, 2, 0, 1), (2, 64, 64, 0, 8, 64, 3, 0), (34, 520, 528, 4, 0, 528, 0, 0))


@pytest.mark.parametrize("view", VIEWS)
def test_pitched_strided_offset_views_and_guards(gpu_ctx, view):
    H, W, ipitch, islack, ioff, opitch, oslack, ooff = view
    rng = np.random.default_rng(zlib.crc32(repr(view).encode()))
    n, guard = 3, 4096
    ifs, ofs = H * ipitch + islack, H * opitch + oslack
    imgs = _frames(rng, n, H, W)
    ibase = torch.from_numpy(rng.integers(0, 1 << 16, size=n * ifs + 64, dtype=np.uint16).view(np.int16)).to(DEV)
    src = _strided(ibase, n, H, W, ifs, ipitch, ioff)
    src.view(torch.int16).copy_(torch.from_numpy(imgs.view(np.int16)).to(DEV))
    before = ibase.clone()
    total = guard + ooff + n * ofs + guard
    obase = torch.full((total,), SENT - 65536, dtype=torch.int16, device=DEV)  # 0xA5A5 as int16
    dst = _strided(obase, n, H, W, ofs, opitch, guard + ooff)
    # the records between sentinels
    rbase = torch.full((8 + n * 8 + 8,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    lo = HL.default_lo(SAT, BLACK)
    for nrec in (n, 1):
        rbase.fill_(0x5A5A5A5A5A5A5A5A)
        raw = rbase[8:8 + nrec * 8].view(nrec, 8)
        rec = gpu_ctx.highlight_chroma(src, sat=SAT, black=BLACK, gain=GAINQ, cfa="gbrg", scope="frame" if nrec == n else "batch",
                                       into=raw.zero_())
        wrec = HL.measure(imgs, SAT, BLACK, GAINQ, 3, lo, nrec=nrec)
        for mode, chroma in (("rebuild", rec), ("clip", None)):
            res = gpu_ctx.highlights(src, sat=SAT, black=BLACK, gain=GAINQ, cfa="gbrg", mode=mode, chroma=chroma, top=TOP, out=dst)
            torch.cuda.synchronize()
            assert res is dst
            want = HL.apply(imgs, HL.CLIP if mode == "clip" else HL.REBUILD, SAT, BLACK, GAINQ, 3, wrec, TOP)
            expect = np.full(total, SENT, np.uint16)
            np.lib.stride_tricks.as_strided(expect[guard + ooff:], (n, H, W), (ofs * 2, opitch * 2, 2))[...] = want
            got = obase.cpu().numpy().view(np.uint16)
            assert np.array_equal(got, expect), (mode, nrec, np.argwhere(got != expect)[:4].tolist())  # guards, and the padding of rows and frames
            assert torch.equal(ibase, before), "the input was written"
            obase.fill_(SENT - 65536)
        r = rbase.cpu().numpy()
        assert np.array_equal(r[8:8 + nrec * 8].reshape(nrec, 8), HL.raw(*wrec)), nrec
        assert (r[:8] == 0x5A5A5A5A5A5A5A5A).all() and (r[8 + nrec * 8:] == 0x5A5A5A5A5A5A5A5A).all(), "around the records"


def test_python_shapes_and_errors(gpu_ctx):
    rng = np.random.default_rng(21)
    H, W = 35, 41
    imgs = _frames(rng, 2, H, W)
    t = _dev16(imgs)
    kw = dict(sat=4000, black=64, gain=(1.9, 1.0, 1.45))
    gq = M.highlight_gains((1.9, 1.0, 1.45), "rggb")
    lo = HL.default_lo((4000,) * 4, (64,) * 4)
    # an (H, W) mosaic drops N in the output; its record is (1, 8)
    one = gpu_ctx.highlights(t[1], **kw)
    rec = gpu_ctx.highlight_chroma(t[1], **kw)
    torch.cuda.synchronize()
    assert tuple(one.shape) == (H, W) and tuple(rec.raw.shape) == (1, 8) and rec.raw.dtype == torch.int64
    assert tuple(rec.sum.shape) == (1, 4) and tuple(rec.cnt.shape) == (1, 4) and rec.cnt.dtype == torch.int32
    w1 = HL.measure(imgs[1:], (4000,) * 4, (64,) * 4, gq, 0, lo)
    assert np.array_equal(rec.raw.cpu().numpy(), HL.raw(*w1))
    assert np.array_equal(_np(one), HL.apply(imgs[1:], HL.REBUILD, (4000,) * 4, (64,) * 4, gq, 0, w1)[0])
    # out=, chroma="batch", a side stream
    out = torch.empty((2, H, W), dtype=torch.int16, device=DEV).view(torch.uint16)
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        res = gpu_ctx.highlights(t, chroma="batch", out=out, lo=100, **kw)
    s.synchronize()
    assert res is out
    wb = HL.measure(imgs, (4000,) * 4, (64,) * 4, gq, 0, (100,) * 4, nrec=1)
    assert np.array_equal(_np(out), HL.apply(imgs, HL.REBUILD, (4000,) * 4, (64,) * 4, gq, 0, wb))
    # empty batches
    e = gpu_ctx.highlights(t[:0], **kw)
    r0 = gpu_ctx.highlight_chroma(t[:0], **kw)
    assert tuple(e.shape) == (0, H, W) and tuple(r0.raw.shape) == (0, 8)
    for bad in (dict(mode="inpaint"), dict(chroma="clip"), dict(chroma=torch.zeros((3, 8), dtype=torch.int64, device=DEV)),
                dict(chroma=torch.zeros((2, 8), dtype=torch.int32, device=DEV)), dict(top=0), dict(sat=64), dict(gain=(0.01, 1, 1)),
                dict(out=torch.zeros((2, H, W + 1), dtype=torch.int16, device=DEV).view(torch.uint16)), dict(cfa="xyzw")):
        with pytest.raises(ValueError):
            gpu_ctx.highlights(t, **{**kw, **bad})
    for bad in (dict(scope="clip"), dict(into=torch.zeros((1, 8), dtype=torch.int64, device=DEV)), dict(lo=(1, 2))):
        with pytest.raises(ValueError):
            gpu_ctx.highlight_chroma(t, **{**kw, **bad})
    with pytest.raises(ValueError):
        gpu_ctx.highlights(t[:, :1], **kw)  # a frame of one row
    with pytest.raises(TypeError):
        gpu_ctx.highlights(t, sat=4000)  # gain has no default
    with pytest.raises(M.McrawError, match="mcraw_highlights_batch: .*overlap"):
        gpu_ctx.highlights(t, out=t, **kw)
    torch.cuda.synchronize()


def test_highlights_keyword(gpu_ctx):
    rng = np.random.default_rng(4)
    n, h, w = 2, 96, 512
    white, black, cfa, gain = 3200, (64, 64, 64, 64), "grbg", (1.7, 1.0, 1.4)
    imgs = np.stack([L.natural_image_np(w, h, 12, 12.0, 40 + i) for i in range(n)])
    imgs = np.minimum(imgs, white)  # a sensor that clips at `white`
    assert 0.1 < (imgs >= white).mean() < 0.5
    t = _dev16(imgs)
    kw = dict(white=float(white), black=black, cfa=cfa, gain=gain, matrix=SRGBISH)
    gq = M.highlight_gains(gain, cfa)
    lo = HL.default_lo((white,) * 4, black)
    rec = HL.measure(imgs, (white,) * 4, black, gq, 2, lo)
    reb = _dev16(HL.apply(imgs, HL.REBUILD, (white,) * 4, black, gq, 2, rec))
    clp = _dev16(HL.apply(imgs, HL.CLIP, (white,) * 4, black, gq, 2))
    own = dict(mode="rebuild", chroma=None, sat=2900, gain=(1.5, 1.0, 1.2), top=5000, lo=1000, black=(60,) * 4, cfa="rggb")  # nothing from the call
    owned = _dev16(HL.apply(imgs, HL.REBUILD, (2900,) * 4, (60,) * 4, M.highlight_gains((1.5, 1.0, 1.2), "rggb"), 0, None, 5000))
    assert not torch.equal(reb, t) and not torch.equal(clp, t) and not torch.equal(owned, reb)
    # one call each: the statement's mosaic through the same method, byte for byte
    a = gpu_ctx.demosaic(t, algo="mhc", dtype="f32", highlights={}, **kw)
    assert torch.equal(a.view(torch.int32), gpu_ctx.demosaic(reb, algo="mhc", dtype="f32", **kw).view(torch.int32))
    b = gpu_ctx.demosaic(t, algo="ha", dtype="f16", highlights=dict(mode="clip"), **kw)
    assert torch.equal(b.view(torch.int16), gpu_ctx.demosaic(clp, algo="ha", dtype="f16", **kw).view(torch.int16))
    d = gpu_ctx.demosaic_display(t, algo="mhc", transfer="srgb", highlights=own, **kw)
    assert torch.equal(d, gpu_ctx.demosaic_display(owned, algo="mhc", transfer="srgb", **kw))
    v = gpu_ctx.demosaic_yuv(t, algo="bin2", fmt="nv12", highlights=dict(chroma="frame"), **kw)
    assert torch.equal(v, gpu_ctx.demosaic_yuv(reb, algo="bin2", fmt="nv12", **kw))
    torch.cuda.synchronize()
    assert np.array_equal(_np(t), imgs), "the caller's mosaic was written"
    # the order: defects, denoise, highlights, shading
    defects = dict(abs_thr=96, rel_thr=26 / 256, rank=2)
    nlut, nshift = M.noise_lut(0.4, 30.0, black, white)
    denoise = dict(lut=nlut, shift=nshift, radius=1)
    y = np.linspace(-1, 1, 13)[:, None]
    x = np.linspace(-1, 1, 17)[None, :]
    gm = M.gain_map(np.stack([1.0 + (s - 1.0) * (x * x + y * y) / 2 for s in (1.9, 1.4, 1.45, 2.3)]), cfa)
    step = gpu_ctx.denoise(gpu_ctx.fix_pixels(t, black=black, **defects), **denoise)
    torch.cuda.synchronize()
    mid = _np(step)
    mid = _dev16(HL.apply(mid, HL.REBUILD, (white,) * 4, black, gq, 2, HL.measure(mid, (white,) * 4, black, gq, 2, lo)))
    chain = gpu_ctx.demosaic(gpu_ctx.shade(mid, gm, black=black), algo="mhc", dtype="f32", **kw)
    allin = gpu_ctx.demosaic(t, algo="mhc", dtype="f32", defects=defects, denoise=denoise, highlights={}, shading=gm, **kw)
    torch.cuda.synchronize()
    assert torch.equal(allin.view(torch.int32), chain.view(torch.int32))
    # without the keyword the methods give their old bytes
    import _rgb_ref as R
    p0 = gpu_ctx.demosaic(t, algo="mhc", dtype="f16", highlights=None, **kw)
    p1 = gpu_ctx.demosaic(t, algo="mhc", dtype="f16", **kw)
    torch.cuda.synchronize()
    assert torch.equal(p0.view(torch.int16), p1.view(torch.int16))
    assert np.array_equal(p0[1].cpu().numpy().view(np.uint16), R.ref_bits(imgs[1], "mhc", "f16", float(white), black=black, cfa=cfa, gain=gain, matrix=SRGBISH))
    # the decode siblings
    ins = [torch.from_numpy(L.encode7(img)).to(DEV) for img in imgs]
    s0 = gpu_ctx.last_serial()
    r = gpu_ctx.decode_rgb(ins, w, h, 7, algo="mhc", dtype="f32", defects=defects, denoise=denoise, highlights={}, shading=gm, **kw)
    torch.cuda.synchronize()
    assert torch.equal(r.view(torch.int32), allin.view(torch.int32))
    s1 = gpu_ctx.last_serial()
    dd = gpu_ctx.decode_display(ins, w, h, 7, algo="mhc", transfer="srgb", highlights=own, **kw)
    vv = gpu_ctx.decode_yuv(ins, w, h, 7, algo="bin2", fmt="nv12", highlights=dict(chroma="frame"), **kw)
    r0 = gpu_ctx.decode_rgb(ins, w, h, 7, algo="mhc", dtype="f16", **kw)
    torch.cuda.synchronize()
    assert torch.equal(dd, d) and torch.equal(vv, v) and torch.equal(r0.view(torch.int16), p1.view(torch.int16))
    assert gpu_ctx.last_serial() == s1 + 3 * (s1 - s0)  # three more decodes; the highlight stage takes no serial
    # what the keyword refuses
    with pytest.raises(ValueError, match="one gain for the batch"):
        gpu_ctx.demosaic(t, algo="mhc", dtype="f16", white=float(white), black=black, cfa=cfa, gain=np.ones((n, 3)), highlights={})
    ok = gpu_ctx.demosaic(t, algo="mhc", dtype="f16", white=float(white), black=black, cfa=cfa, gain=np.ones((n, 3)), highlights=dict(gain=(1, 1, 1)))
    assert tuple(ok.shape) == (n, 3, h, w)
    for bad in (dict(out=None), dict(strength=2), dict(mode="inpaint")):
        with pytest.raises(ValueError):
            gpu_ctx.demosaic_yuv(t, algo="mhc", highlights=bad, **kw)
    with pytest.raises(ValueError):
        gpu_ctx.decode_display(ins, w, h, 7, highlights=dict(nope=1), **kw)
    with pytest.raises(TypeError):
        gpu_ctx.decode_merge(ins, w, h, 7, lut=nlut, shift=nshift, highlights={})
    torch.cuda.synchronize()
    assert gpu_ctx.errors() == 0


def test_decode_state_and_siblings_untouched(gpu_ctx):
    rng = np.random.default_rng(3)
    w, h = 512, 96
    items = []
    for _ in range(2):
        img = L.natural_image_np(w, h, 12, 12.0, int(rng.integers(1 << 30)))
        buf = L.encode7(img)
        ret, want = L.oracle_decode7(buf, w, h)
        assert ret == w * h
        items.append((buf, want))
    ins = [torch.from_numpy(b).to(DEV) for b, _ in items]
    imgs = np.stack([want for _, want in items])
    t = _dev16(imgs)
    kw = dict(algo="mhc", dtype="f16", white=4095.0, black=(64,) * 4, gain=(1.9, 1.0, 1.4), matrix=SRGBISH)
    hk = dict(sat=2000, black=64, gain=(1.9, 1.0, 1.4))
    gq = M.highlight_gains((1.9, 1.0, 1.4), "rggb")
    gpu_ctx.set_float_out("f32", 4095.0, layout="mosaic", black=(64,) * 4)
    try:
        f0 = gpu_ctx.demosaic(t, **kw)
        torch.cuda.synchronize()
        serial, errs = gpu_ctx.last_serial(), gpu_ctx.errors(reset=False)
        rec = gpu_ctx.highlight_chroma(t, **hk)
        res = gpu_ctx.highlights(t, chroma=rec, **hk)
        clp = gpu_ctx.highlights(t, mode="clip", **hk)
        torch.cuda.synchronize()
        assert gpu_ctx.last_serial() == serial and gpu_ctx.errors(reset=False) == errs
        want = HL.measure(imgs, (2000,) * 4, (64,) * 4, gq, 0, HL.default_lo((2000,) * 4, (64,) * 4))
        assert np.array_equal(rec.raw.cpu().numpy(), HL.raw(*want))
        assert np.array_equal(_np(res), HL.apply(imgs, HL.REBUILD, (2000,) * 4, (64,) * 4, gq, 0, want))
        assert np.array_equal(_np(clp), HL.apply(imgs, HL.CLIP, (2000,) * 4, (64,) * 4, gq, 0))
        assert (imgs >= 2000).sum() > 100
        f1 = gpu_ctx.demosaic(t, **kw)
        torch.cuda.synchronize()
        assert torch.equal(f0.view(torch.int16), f1.view(torch.int16))
        # the context's stage is as it was: the next plain batch is still the float mosaic
        o = torch.full((w * h * 4,), 0xA5, dtype=torch.uint8, device=DEV)
        written, status = gpu_ctx.decode_batch(M.Context.make_frames([(ins[0].data_ptr(), ins[0].numel(), w, h, 7, o.data_ptr(), w * h * 2)]))
        assert status == [0]
        import _float_ref as FR
        assert np.array_equal(o.cpu().numpy(), FR.ref_bytes(items[0][1], "f32", 4095.0, "mosaic", (64,) * 4))
        assert gpu_ctx.last_serial() == serial + 1
    finally:
        gpu_ctx.set_post()
    assert gpu_ctx.errors() == 0
