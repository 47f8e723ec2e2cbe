"""Defective pixels of mosaics (mcraw_fixpix_batch, Context.fix_pixels, defects= on the demosaic / decode methods) on the GPU:
every output sample and every count equals the numpy statement of the contract (_fixpix_ref), nothing outside the output is
written, the input is left as it was, rejected calls write nothing and say why, each queued call reads its list's contents
in stream order, and the context's decode state and the sibling entry points are undisturbed."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import _fixpix_ref as F
import _libs as L
import motioncam_decoder_amd as M

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SENT = 0xA5A5
GEOMS = ((1, 1), (2, 2), (3, 5), (1, 64), (33, 1), (16, 64), (35, 41), (34, 520), (70, 1002))  # (H, W); and the full size below
# (black, abs_thr, rel_thr in Q8)
PSETS = (((0,) * 4, (0,) * 4, 0), ((64, 65, 66, 67), (96, 97, 98, 99), 26), ((0, 1023, 512, 7), (0,) * 4, 65535),
         ((4000, 100, 65535, 256), (3000, 20000, 5, 65535), 300))
SRGBISH = np.array([[1.7, -0.5, -0.2], [-0.25, 1.4, -0.15], [0.05, -0.45, 1.4]], np.float32)


def _np(t):
    a = t.detach()
    if a.dtype == torch.uint16:
        return a.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    return a.cpu().numpy()


def _dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).to(DEV).view(torch.uint16)


def _dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(DEV)


def _kw(pset, rank, flags):
    black, abs_thr, rel = pset
    return dict(black=black, abs_thr=abs_thr, rel_thr=rel / 256.0, rank=rank, hot=bool(flags & 1), cold=bool(flags & 2))


def _check(res, cnt, imgs, flags, rank, pset, lst=None, what=""):
    black, abs_thr, rel = pset
    want, wc = F.fixpix(imgs, flags, rank, rel, black, abs_thr, lst)
    got = _np(res)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, flags, rank, pset, len(bad), bad[:4].tolist())
    if cnt is not None:
        assert np.array_equal(cnt.cpu().numpy().view(np.uint32), wc), (what, flags, rank, pset, cnt.cpu().numpy().tolist(), wc.tolist())
    return want


def _struct(flags=3, rank=2, rel=0, black=(0,) * 4, abs_thr=(0,) * 4, lst=0, nlist=0, counts=0, reserved=(0, 0)):
    s = M.FixPix()
    s.flags, s.rank, s.rel_thr, s.nlist = flags, rank, rel, nlist
    for i in range(4):
        s.black[i], s.abs_thr[i] = black[i], abs_thr[i]
    s.list, s.counts = lst or None, counts or None
    s.reserved[0], s.reserved[1] = reserved
    return s


def _raw(ctx, s, in_ptr, ip, ifs, w, h, n, out_ptr, op, ofs, stream=None):
    return M.load().mcraw_fixpix_batch(ctx._h, C.byref(s) if s is not None else None, C.c_void_p(in_ptr), ip, ifs, w, h, n,
                                       C.c_void_p(out_ptr), op, ofs, C.c_void_p(stream))


@pytest.mark.parametrize("geom", GEOMS)
def test_fixpix_matches_reference(gpu_ctx, geom):
    H, W = geom
    rng = np.random.default_rng(zlib.crc32(("%dx%d" % (H, W)).encode()))
    n = 2
    imgs = rng.integers(0, 1 << 16, size=(n, H, W), dtype=np.uint16)  # full range: the rare path on about four pixels in nine
    t = _dev16(imgs)
    for pset in PSETS:
        for rank in (1, 2):
            for flags in (1, 2, 3):
                res, cnt = gpu_ctx.fix_pixels(t, counts=True, **_kw(pset, rank, flags))
                torch.cuda.synchronize()
                assert tuple(res.shape) == (n, H, W) and res.dtype == torch.uint16 and tuple(cnt.shape) == (n, 2, 4)
                _check(res, cnt, imgs, flags, rank, pset)
    assert np.array_equal(_np(t), imgs), "the input was written"
    # 12-bit content (neighbours tie), without counts
    low = rng.integers(0, 1 << 12, size=(n, H, W), dtype=np.uint16) >> 6 << 6
    res = gpu_ctx.fix_pixels(_dev16(low), **_kw(PSETS[0], 2, 3))
    torch.cuda.synchronize()
    _check(res, None, low, 3, 2, PSETS[0], what="ties")


def test_full_size(gpu_ctx):
    H, W, n = 2160, 3840, 2
    rng = np.random.default_rng(11)
    imgs = rng.integers(0, 1 << 16, size=(n, H, W), dtype=np.uint16)
    res, cnt = gpu_ctx.fix_pixels(_dev16(imgs), counts=True, **_kw(PSETS[1], 2, 3))
    torch.cuda.synchronize()
    _check(res, cnt, imgs, 3, 2, PSETS[1])


def _strided(base, n, h, w, fstride, pitch, off):
    return torch.as_strided(base, (n, h, w), (fstride, pitch, 1), off).view(torch.uint16)


# (H, W, input pitch, input frame slack, input offset, output pitch, output frame slack, output offset): offsets in samples;
# 1 = an odd base address in samples (off the dword grid), 4 = on the 8-byte grid only, 8 with pitches and strides that are
# multiples of 8 = the 16-byte path; a pitch % 8 != 0 or a slack % 8 != 0 takes rows or frames off the 16-byte grid
VIEWS = ((35, 41, 53, 29, 1, 47, 3, 4), (34, 520, 520, 0, 4, 531, 17, 1), (70, 1002, 1008, 8, 8, 1016, 16, 8),
         (16, 64, 64, 0, 0, 72, 8, 1), (33, 1, 3, 5, 1, 1, 0, 1), (1, 64, 64, 0, 8, 64, 3, 0), (70, 1002, 1003, 1, 0, 1002, 0, 4),
         (34, 520, 528, 4, 0, 528, 0, 0))


@pytest.mark.parametrize("view", VIEWS)
def test_pitched_strided_offset_views_and_guards(gpu_ctx, view):
    H, W, ipitch, islack, ioff, opitch, oslack, ooff = view
    rng = np.random.default_rng(zlib.crc32(repr(view).encode()))
    n, guard = 3, 4096
    ifs, ofs = H * ipitch + islack, H * opitch + oslack
    imgs = rng.integers(0, 1 << 16, size=(n, H, W), dtype=np.uint16)
    ibase = torch.from_numpy(rng.integers(0, 1 << 16, size=n * ifs + 64, dtype=np.uint16).view(np.int16)).to(DEV)
    src = _strided(ibase, n, H, W, ifs, ipitch, ioff)
    src.view(torch.int16).copy_(torch.from_numpy(imgs.view(np.int16)).to(DEV))
    before = ibase.clone()
    total = guard + ooff + n * ofs + guard
    obase = torch.full((total,), SENT - 65536, dtype=torch.int16, device=DEV)  # 0xA5A5 as int16
    dst = _strided(obase, n, H, W, ofs, opitch, guard + ooff)
    pix = np.stack([rng.integers(0, W, 24), rng.integers(0, H, 24)], axis=1)
    for pset, rank, flags, pixels in ((PSETS[0], 2, 3, None), (PSETS[1], 1, 3, pix), (PSETS[3], 2, 1, None)):
        res, cnt = gpu_ctx.fix_pixels(src, counts=True, pixels=pixels, out=dst, **_kw(pset, rank, flags))
        torch.cuda.synchronize()
        assert res is dst
        want = _check(res, cnt, imgs, flags, rank, pset, None if pixels is None else M.pack_pixels(pixels))
        expect = np.full(total, SENT, np.uint16)
        np.lib.stride_tricks.as_strided(expect[guard + ooff:], (n, H, W), (ofs * 2, opitch * 2, 2))[...] = want
        got = obase.cpu().numpy().view(np.uint16)
        assert np.array_equal(got[:guard + ooff], expect[:guard + ooff]) and np.array_equal(got[-guard:], expect[-guard:]), "guards"
        assert np.array_equal(got, expect), np.argwhere(got != expect)[:4].tolist()  # the padding of rows and frames too
        assert torch.equal(ibase, before), "the input was written"
        obase.fill_(SENT - 65536)


def _lists(rng, H, W):
    """Packed lists as the call gets them: (name, entries)."""
    K = max(2, H * W // 5)
    rand = np.stack([rng.integers(0, W, K), rng.integers(0, H, K)], axis=1)
    cy, cx = H // 2, W // 2  # a cluster: a block around the centre, every neighbour of its inner pixels listed
    clus = np.array([(x, y) for y in range(max(cy - 4, 0), min(cy + 5, H)) for x in range(max(cx - 4, 0), min(cx + 5, W))])
    edge = np.array(sorted({(x, y) for y in (0, 1, H - 2, H - 1) for x in (0, 1, W // 2, W - 2, W - 1) if 0 <= y < H and 0 <= x < W}
                           | {(x, y) for x in (0, W - 1) for y in range(0, H, 3)} | {(x, y) for y in (0, H - 1) for x in range(0, W, 5)}))
    out = [(min(W, 65535), 0), (0, min(H, 65535)), (65535, 65535), (W // 2, min(H + 3, 65535))]
    pack = lambda a: M.pack_pixels(np.asarray(a).reshape(-1, 2))
    mixed = np.concatenate([rand, clus, edge, np.array(out)])
    unsorted = (mixed[:, 1].astype(np.uint32) << 16 | mixed[:, 0].astype(np.uint32))[rng.permutation(len(mixed))]
    return [("random", pack(rand)), ("cluster", pack(clus)), ("edges", pack(edge)), ("outside", pack(out)),
            ("one", pack([(W - 1, H - 1)])), ("mixed", pack(mixed)), ("unsorted", unsorted.astype(np.uint32))]


@pytest.mark.parametrize("geom", ((1, 1), (2, 2), (3, 5), (1, 64), (33, 1), (35, 41), (70, 1002)))
def test_lists(gpu_ctx, geom):
    H, W = geom
    rng = np.random.default_rng(H * 131 + W)
    n = 2
    imgs = rng.integers(0, 1 << 16, size=(n, H, W), dtype=np.uint16)
    t = _dev16(imgs)
    for k, (name, lst) in enumerate(_lists(rng, H, W)):
        # the list alone (both flags off), then over the dynamic pass
        for flags, rank, pset in ((0, 1, PSETS[0]), (3, 1 + k % 2, PSETS[k % 2])):
            res, cnt = gpu_ctx.fix_pixels(t, pixels=_dev32(lst), counts=True, **_kw(pset, rank, flags))  # a device tensor: as it is
            torch.cuda.synchronize()
            _check(res, cnt, imgs, flags, rank, pset, lst, what=name)
    assert np.array_equal(_np(t), imgs), "the input was written"


def test_same_list_pointer_new_contents_between_queued_calls(gpu_ctx):
    rng = np.random.default_rng(9)
    n, h, w, K = 2, 70, 1002, 512
    imgs = rng.integers(0, 1 << 14, size=(n, h, w), dtype=np.uint16)
    t = _dev16(imgs)
    s = torch.cuda.Stream(DEV)
    dl = torch.empty((K,), dtype=torch.int32, device=DEV)
    lists = []
    for _ in range(4):
        a = M.pack_pixels(np.stack([rng.integers(0, w, 2 * K), rng.integers(0, h, 2 * K)], axis=1))[:K]
        assert a.size == K
        lists.append(a)
    staged = [_dev32(a) for a in lists]
    torch.cuda.synchronize()
    outs = []
    with torch.cuda.stream(s):
        for k in range(4):  # no host sync between: the list is rewritten in stream order between the calls
            dl.copy_(staged[k])
            outs.append(gpu_ctx.fix_pixels(t, pixels=dl, **_kw(PSETS[1], 2, 3)))
    s.synchronize()
    for k, o in enumerate(outs):
        _check(o, None, imgs, 3, 2, PSETS[1], lists[k], what=k)


def test_rejections_write_nothing_and_say_why(gpu_ctx):
    w, h, n = 24, 10, 2
    buf = torch.full((8192,), SENT - 65536, dtype=torch.int16, device=DEV)
    aux = torch.full((1024,), SENT - 65536, dtype=torch.int16, device=DEV)  # counts, and a list
    base, ab = buf.data_ptr(), aux.data_ptr()
    ip, op = base, base + 2 * 4096
    good = dict(in_ptr=ip, ip=w, ifs=w * h, w=w, h=h, n=n, out_ptr=op, op=w, ofs=w * h)

    def call(st=None, **kw):
        a = dict(good)
        a.update(kw)
        return _raw(gpu_ctx, st if st is not None else _struct(), a["in_ptr"], a["ip"], a["ifs"], a["w"], a["h"], a["n"],
                    a["out_ptr"], a["op"], a["ofs"])

    cases = [
        ("no struct", lambda: _raw(gpu_ctx, None, ip, w, w * h, w, h, n, op, w, w * h)),
        ("NULL in", lambda: call(in_ptr=0)),
        ("NULL out", lambda: call(out_ptr=0)),
        ("odd in", lambda: call(in_ptr=ip + 1)),
        ("odd out", lambda: call(out_ptr=op + 1)),
        ("width 0", lambda: call(w=0)),
        ("width 65537", lambda: call(w=65537, ip=65537, op=65537, n=1)),
        ("height 0", lambda: call(h=0)),
        ("height 65537", lambda: call(h=65537, n=1)),
        ("negative width", lambda: call(w=-4)),
        ("in pitch below width", lambda: call(ip=w - 1)),
        ("out pitch below width", lambda: call(op=w - 1)),
        ("in frame stride too small", lambda: call(ifs=w * h - 1)),
        ("out frame stride too small", lambda: call(ofs=(h - 1) * w + w - 1)),
        ("rank 0", lambda: call(_struct(rank=0))),
        ("rank 3", lambda: call(_struct(rank=3))),
        ("rel_thr 65536", lambda: call(_struct(rel=65536))),
        ("unknown flag", lambda: call(_struct(flags=4))),
        ("unknown flag beside known ones", lambda: call(_struct(flags=3 | 0x80000000))),
        ("list NULL with nlist", lambda: call(_struct(lst=0, nlist=3))),
        ("list misaligned", lambda: call(_struct(lst=ab + 2, nlist=3))),
        ("nlist above 1 << 20", lambda: call(_struct(lst=ab, nlist=(1 << 20) + 1))),
        ("counts misaligned", lambda: call(_struct(counts=ab + 2))),
        ("counts odd", lambda: call(_struct(counts=ab + 1))),
        ("reserved[0]", lambda: call(_struct(reserved=(1, 0)))),
        ("reserved[1]", lambda: call(_struct(reserved=(0, 1)))),
        ("negative n", lambda: call(n=-1)),
        ("in place", lambda: call(out_ptr=ip)),
        ("in place, one frame", lambda: call(out_ptr=ip, n=1)),
        ("out inside in", lambda: call(out_ptr=ip + 16)),
        ("out ends inside in", lambda: call(in_ptr=op + 2 * (n * w * h - 8))),
        ("same base, other pitch", lambda: call(out_ptr=ip, op=w + 8, ofs=(w + 8) * h)),
        ("counts inside in", lambda: call(_struct(counts=ip + 64))),
        ("counts ends inside out", lambda: call(_struct(counts=op - 32 * n + 4))),
        ("counts inside out", lambda: call(_struct(counts=op + 2 * (n * w * h) - 4))),
    ]
    serial = gpu_ctx.last_serial()
    for name, fn in cases:
        rc = fn()
        assert rc < 0, name
        msg = M.load().mcraw_last_error().decode()
        assert msg.startswith("mcraw_fixpix_batch: ") and len(msg) > len("mcraw_fixpix_batch: "), name
    assert call(n=0) == 0  # n == 0: a no-op
    assert call(_struct(counts=ab), n=0) == 0
    torch.cuda.synchronize()
    gpu_ctx.synchronize()
    assert (buf.cpu().numpy().view(np.uint16) == SENT).all() and (aux.cpu().numpy().view(np.uint16) == SENT).all()
    assert gpu_ctx.last_serial() == serial
    # good calls next to them do write: the edges of the ranges, counts right behind the output, counts = NULL
    img = np.random.default_rng(1).integers(0, 1 << 16, size=(n, h, w), dtype=np.uint16)
    buf[:n * w * h].copy_(torch.from_numpy(img.reshape(-1).view(np.int16)).to(DEV))
    cptr = op + 2 * n * w * h
    assert cptr % 4 == 0
    assert call(_struct(counts=cptr)) == 0
    torch.cuda.synchronize()
    a = buf.cpu().numpy().view(np.uint16)
    want, wc = F.fixpix(img, 3, 2)
    assert np.array_equal(a[4096:4096 + n * w * h], want.reshape(-1))
    assert np.array_equal(a[4096 + n * w * h:4096 + n * w * h + 16 * n].view(np.uint32).reshape(n, 2, 4), wc)
    assert (a[4096 + n * w * h + 16 * n:] == SENT).all() and (a[n * w * h:4096] == SENT).all()
    buf[4096:].fill_(SENT - 65536)
    assert call(_struct(flags=1, rank=1)) == 0  # counts = NULL
    torch.cuda.synchronize()
    a = buf.cpu().numpy().view(np.uint16)
    assert np.array_equal(a[4096:4096 + n * w * h], F.fixpix(img, 1, 1)[0].reshape(-1)) and (a[4096 + n * w * h:] == SENT).all()
    # nlist = 0 with a list pointer, and a misaligned pointer that is not used
    assert call(_struct(lst=ab + 2, nlist=0)) == 0
    torch.cuda.synchronize()
    # Python: what the wrapper checks itself
    t = torch.zeros((2, 8, 8), dtype=torch.int16, device=DEV).view(torch.uint16)
    for kw in (dict(abs_thr=(1, 2, 3)), dict(abs_thr=70000), dict(abs_thr=0, rel_thr=256.0), dict(abs_thr=0, rel_thr=-1.0),
               dict(abs_thr=0, rank=3), dict(abs_thr=0, black=(1, 2)), dict(abs_thr=0, black=64.5), dict(abs_thr=(96, 96, 96.25, 96)), dict(abs_thr=0, pixels=np.zeros((3, 3), np.int32)),
               dict(abs_thr=0, pixels=torch.zeros(4, dtype=torch.float32, device=DEV)),
               dict(abs_thr=0, out=torch.zeros((2, 8, 9), dtype=torch.int16, device=DEV).view(torch.uint16))):
        with pytest.raises(ValueError):
            gpu_ctx.fix_pixels(t, **kw)
    with pytest.raises(TypeError):
        gpu_ctx.fix_pixels(t)  # abs_thr has no default
    with pytest.raises(M.McrawError, match="mcraw_fixpix_batch: .*overlap"):
        gpu_ctx.fix_pixels(t, abs_thr=0, out=t)
    with pytest.raises(ValueError):
        gpu_ctx.demosaic(t, dtype="f16", white=4095.0, defects=dict(abs_thr=0, counts=True))
    with pytest.raises(ValueError):  # the call's own fractional black is forwarded, not truncated
        gpu_ctx.demosaic(t, dtype="f16", white=4095.0, black=(64.5,) * 4, defects=dict(abs_thr=0))
    ok = gpu_ctx.fix_pixels(t, abs_thr=96.0, black=np.float32(64.0))  # integral floats are levels
    assert tuple(ok.shape) == (2, 8, 8)
    torch.cuda.synchronize()


def _frames(rng, shapes, typ):
    items = []
    for (w, h) in shapes:
        img = L.natural_image_np(w, h, 12, 12.0, int(rng.integers(1 << 30)))
        buf = L.encode7(img) if typ == 7 else L.encode6(img)
        ret, want = (L.oracle_decode7 if typ == 7 else L.oracle_decode6)(buf, w, h)
        assert ret == w * h
        items.append((buf, want))
    return items


def test_decode_state_and_siblings_untouched(gpu_ctx):
    rng = np.random.default_rng(3)
    w, h = 512, 96
    items = _frames(rng, [(w, h)] * 2, 7)
    ins = [torch.from_numpy(b).to(DEV) for b, _ in items]
    imgs = np.stack([want for _, want in items])
    t = _dev16(imgs)
    kw = dict(algo="mhc", dtype="f16", white=4095.0, black=(64,) * 4, gain=(1.9, 1.0, 1.4), matrix=SRGBISH)
    gpu_ctx.set_float_out("f32", 4095.0, layout="mosaic", black=(64,) * 4)
    try:
        f0 = gpu_ctx.demosaic(t, **kw)
        torch.cuda.synchronize()
        serial, errs = gpu_ctx.last_serial(), gpu_ctx.errors(reset=False)
        res, cnt = gpu_ctx.fix_pixels(t, counts=True, pixels=np.array([[5, 7], [100, 50]]), **_kw(PSETS[0], 2, 3))
        torch.cuda.synchronize()
        assert gpu_ctx.last_serial() == serial and gpu_ctx.errors(reset=False) == errs
        _check(res, cnt, imgs, 3, 2, PSETS[0], M.pack_pixels(np.array([[5, 7], [100, 50]])))
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


def test_fix_pixels_shapes(gpu_ctx):
    rng = np.random.default_rng(21)
    H, W = 35, 41
    imgs = rng.integers(0, 1 << 16, size=(2, H, W), dtype=np.uint16)
    t = _dev16(imgs)
    pix = np.array([[0, 0], [40, 34], [7, 9], [7, 9], [8, 9]])
    # an (H, W) mosaic drops N, for the counts too
    one, cnt = gpu_ctx.fix_pixels(t[1], counts=True, pixels=pix, **_kw(PSETS[1], 2, 3))
    torch.cuda.synchronize()
    assert tuple(one.shape) == (H, W) and tuple(cnt.shape) == (2, 4) and cnt.dtype == torch.int32
    want, wc = F.fixpix(imgs[1:], 3, 2, PSETS[1][2], PSETS[1][0], PSETS[1][1], M.pack_pixels(pix))
    assert np.array_equal(_np(one), want[0]) and np.array_equal(cnt.cpu().numpy().view(np.uint32), wc[0])
    # out=, scalar thresholds, a host list given as a list of pairs
    out = torch.empty((2, H, W), dtype=torch.int16, device=DEV).view(torch.uint16)
    res = gpu_ctx.fix_pixels(t, black=64, abs_thr=96, rel_thr=26 / 256, rank=1, cold=False, pixels=[(3, 4)], out=out)
    torch.cuda.synchronize()
    assert res is out
    assert np.array_equal(_np(out), F.fixpix(imgs, 1, 1, 26, (64,) * 4, (96,) * 4, M.pack_pixels([(3, 4)]))[0])
    # empty batches and empty lists
    e, c = gpu_ctx.fix_pixels(t[:0], abs_thr=0, counts=True)
    assert tuple(e.shape) == (0, H, W) and tuple(c.shape) == (0, 2, 4)
    res = gpu_ctx.fix_pixels(t, abs_thr=0, pixels=np.zeros((0, 2), np.int64))
    torch.cuda.synchronize()
    assert np.array_equal(_np(res), F.fixpix(imgs, 3, 2)[0])
    # on the null stream and on a side stream
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        r2 = gpu_ctx.fix_pixels(t, abs_thr=0)
    s.synchronize()
    assert torch.equal(r2.view(torch.int16), res.view(torch.int16))


def test_defects_keyword(gpu_ctx):
    rng = np.random.default_rng(4)
    n, h, w = 2, 96, 512
    clean = np.stack([L.natural_image_np(w, h, 12, 12.0, 40 + i) for i in range(n)])
    imgs = clean.copy()
    ys, xs = np.meshgrid(np.arange(3, h - 3, 7), np.arange(3, w - 3, 9), indexing="ij")
    imgs[:, ys, xs] = np.clip(imgs[:, ys, xs].astype(np.int64) + np.where((ys + xs) & 1, 600, -600), 0, 4095).astype(np.uint16)
    t = _dev16(imgs)
    black, cfa, gain = (64, 64, 64, 64), "grbg", (1.7, 1.0, 1.4)
    kw = dict(white=4095.0, black=black, cfa=cfa, gain=gain, matrix=SRGBISH)
    defects = dict(abs_thr=96, rel_thr=26 / 256, rank=2, pixels=np.array([[10, 11], [500, 70]]))
    fixed = gpu_ctx.fix_pixels(t, black=black, **defects)
    torch.cuda.synchronize()
    want = F.fixpix(imgs, 3, 2, 26, black, (96,) * 4, M.pack_pixels(defects["pixels"]))[0]
    assert np.array_equal(_np(fixed), want) and (want != imgs).sum() > ys.size  # (the injected defects are found)
    y = np.linspace(-1, 1, 13)[:, None]
    x = np.linspace(-1, 1, 17)[None, :]
    gm = M.gain_map(np.stack([1.0 + (s - 1.0) * (x * x + y * y) / 2 for s in (1.9, 1.4, 1.45, 2.3)]), cfa)
    shaded = gpu_ctx.shade(fixed, gm, black=black)
    # one call each: the two-step route, byte for byte; defects first, then the gains
    a = gpu_ctx.demosaic(t, algo="mhc", dtype="f32", defects=defects, **kw)
    b = gpu_ctx.demosaic(t, algo="mhc", dtype="f32", defects=defects, shading=gm, **kw)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), gpu_ctx.demosaic(fixed, algo="mhc", dtype="f32", **kw).view(torch.int32))
    assert torch.equal(b.view(torch.int32), gpu_ctx.demosaic(shaded, algo="mhc", dtype="f32", **kw).view(torch.int32))
    d = gpu_ctx.demosaic_display(t, algo="mhc", transfer="srgb", defects=defects, **kw)
    assert torch.equal(d, gpu_ctx.demosaic_display(fixed, algo="mhc", transfer="srgb", **kw))
    v = gpu_ctx.demosaic_yuv(t, algo="bin2", fmt="nv12", defects=defects, shading=gm, **kw)
    assert torch.equal(v, gpu_ctx.demosaic_yuv(shaded, algo="bin2", fmt="nv12", **kw))
    torch.cuda.synchronize()
    assert np.array_equal(_np(t), imgs), "the caller's mosaic was written"
    # defects=None is the call as it always was
    p0 = gpu_ctx.demosaic(t, algo="mhc", dtype="f16", defects=None, **kw)
    p1 = gpu_ctx.demosaic(t, algo="mhc", dtype="f16", **kw)
    d0 = gpu_ctx.demosaic_display(t, algo="bin2", defects=None, **kw)
    y0 = gpu_ctx.demosaic_yuv(t, algo="mhc", fmt="p010", defects=None, **kw)
    torch.cuda.synchronize()
    import _rgb_ref as R
    assert torch.equal(p0.view(torch.int16), p1.view(torch.int16))
    assert np.array_equal(p0[1].cpu().numpy().view(np.uint16),
                          R.ref_bits(imgs[1], "mhc", "f16", 4095.0, black=black, cfa=cfa, gain=gain, matrix=SRGBISH))
    assert torch.equal(d0, gpu_ctx.demosaic_display(t, algo="bin2", **kw))
    assert torch.equal(y0, gpu_ctx.demosaic_yuv(t, algo="mhc", fmt="p010", **kw))
    # the decode siblings: frames that carry the defects, decoded and fixed in one call
    ins = [torch.from_numpy(L.encode7(img)).to(DEV) for img in imgs]
    s0 = gpu_ctx.last_serial()
    r = gpu_ctx.decode_rgb(ins, w, h, 7, algo="mhc", dtype="f32", defects=defects, shading=gm, **kw)
    torch.cuda.synchronize()
    assert torch.equal(r.view(torch.int32), b.view(torch.int32))
    s1 = gpu_ctx.last_serial()
    r0 = gpu_ctx.decode_rgb(ins, w, h, 7, algo="mhc", dtype="f32", defects=None, **kw)
    dd = gpu_ctx.decode_display(ins, w, h, 7, algo="mhc", transfer="srgb", defects=defects, **kw)
    vv = gpu_ctx.decode_yuv(ins, w, h, 7, algo="bin2", fmt="nv12", defects=defects, shading=gm, **kw)
    torch.cuda.synchronize()
    assert torch.equal(r0.view(torch.int32), gpu_ctx.demosaic(t, algo="mhc", dtype="f32", **kw).view(torch.int32))
    assert torch.equal(dd, d) and torch.equal(vv, v)
    assert gpu_ctx.last_serial() == s1 + 3 * (s1 - s0)  # three more decodes; the defect stage takes no serial
    assert gpu_ctx.errors() == 0
