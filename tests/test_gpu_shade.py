"""Lens-shading gain maps on mosaics (mcraw_shade_batch, Context.shade, shading= on the demosaic / decode methods) on the
GPU: every output sample equals the numpy statement of the contract (_shade_ref), nothing outside the output is written, the
input is left as it was out of place, rejected calls write nothing and say why, each queued call reads its map's contents in
stream order, and the context's decode state and the sibling entry points are undisturbed."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import _display_ref as D
import _libs as L
import _rgb_ref as R
import _shade_ref as S
import _yuv_ref as Y
import motioncam_decoder_amd as M

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SENT = 0xA5A5
GEOMS = ((16, 64), (34, 520), (70, 1002), (2160, 3840), (35, 41), (1, 64), (33, 1), (71, 1001))  # (H, W)
MAPS = ((1, 1), (2, 2), (13, 17), (64, 64), (3, 64))  # (gh, gw)
BLACKS = ((64, 65, 66, 67), (0, 1023, 512, 7), (4000, 100, 65535, 256), (1, 2, 3, 4))
TOPS = (65535, 4095, 1023, 16383, 1)
SRGBISH = np.array([[1.7, -0.5, -0.2], [-0.25, 1.4, -0.15], [0.05, -0.45, 1.4]], np.float32)


def _np(t):
    a = t.detach()
    if a.dtype == torch.uint16:
        return a.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    return a.cpu().numpy()


def _dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).to(DEV).view(torch.uint16)


def _rand_map(rng, gh, gw, n=None):
    """Random entries over the full 16 bits (bit 15 is ignored by the contract)."""
    shape = (4, gh, gw) if n is None else (n, 4, gh, gw)
    return rng.integers(0, 1 << 16, size=shape, dtype=np.uint16)


def _vignette_map(gh, gw, cfa="rggb"):
    y = np.linspace(-1, 1, gh)[:, None] if gh > 1 else np.zeros((1, 1))
    x = np.linspace(-1, 1, gw)[None, :] if gw > 1 else np.zeros((1, 1))
    r2 = (x * x + y * y) / 2
    return M.gain_map(np.stack([1.0 + (s - 1.0) * r2 for s in (1.9, 1.4, 1.45, 2.3)]), cfa)


def _want(imgs, gmaps, black, top):
    """The reference for a batch; the gains of a map shared by all frames are made once."""
    if gmaps.ndim == 3:
        G, _ = S.gains(imgs.shape[1], imgs.shape[2], gmaps)
        return np.stack([S.apply(im, G, black, top) for im in imgs])
    return S.shade_batch_ref(imgs, gmaps, black, top)


def _shade(map_ptr, gw, gh, nmaps=1, top=65535, black=(0, 0, 0, 0), reserved=(0, 0)):
    s = M.Shade()
    s.map_w, s.map_h, s.nmaps, s.top = gw, gh, nmaps, top
    for i in range(4):
        s.black[i] = black[i]
    s.reserved[0], s.reserved[1] = reserved
    s.map = map_ptr
    return s


def _raw(ctx, s, in_ptr, ip, ifs, w, h, n, out_ptr, op, ofs, stream=None):
    return M.load().mcraw_shade_batch(ctx._h, C.byref(s) if s is not None else None, C.c_void_p(in_ptr), ip, ifs, w, h, n,
                                      C.c_void_p(out_ptr), op, ofs, C.c_void_p(stream))


@pytest.mark.parametrize("mp", MAPS)
@pytest.mark.parametrize("geom", GEOMS)
def test_shade_matches_reference(gpu_ctx, geom, mp):
    (H, W), (gh, gw) = geom, mp
    k = GEOMS.index(geom) * len(MAPS) + MAPS.index(mp)
    rng = np.random.default_rng(zlib.crc32(("%dx%d %dx%d" % (H, W, gh, gw)).encode()))
    big = H * W > 1 << 20
    n = 2 if big else 3
    imgs = rng.integers(0, 1 << 16, size=(n, H, W), dtype=np.uint16)
    t = _dev16(imgs)
    runs = [("broadcast", False), ("per-frame", True)]
    if big:  # the large frames: one of the two forms per map size (both for the 13 x 17 map)
        runs = runs if mp == (13, 17) else [runs[k % 2]]
    for j, (form, inplace) in enumerate(runs):
        gm = _rand_map(rng, gh, gw, n if form == "per-frame" else None)
        black, top = BLACKS[(k + j) % len(BLACKS)], TOPS[(k + 2 * j) % len(TOPS)]
        want = _want(imgs, gm, black, top)
        if inplace:
            work = t.clone()
            res = gpu_ctx.shade(work, _dev16(gm), black=black, top=top, out=work)
            assert res is work
        else:
            res = gpu_ctx.shade(t, gm, black=black, top=top)  # (a host array: uploaded on the current stream)
        torch.cuda.synchronize()
        assert tuple(res.shape) == (n, H, W) and res.dtype == torch.uint16
        got = _np(res)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (form, inplace, black, top, len(bad), bad[:4].tolist())
        assert np.array_equal(_np(t), imgs), "the input was written"
    # a single (H, W) mosaic drops N
    one = gpu_ctx.shade(t[0], _dev16(gm[0] if gm.ndim == 4 else gm), black=black, top=top)
    torch.cuda.synchronize()
    assert tuple(one.shape) == (H, W) and np.array_equal(_np(one), want[0])


def _strided(base, n, h, w, fstride, pitch, off):
    return torch.as_strided(base, (n, h, w), (fstride, pitch, 1), off).view(torch.uint16)


# (H, W, input pitch, input frame slack, input offset, output pitch, output frame slack, output offset): offsets in samples;
# 1 = off the dword grid, 4 = 8 bytes (on the 8-byte grid only), 8 with a pitch that is a multiple of 8 = the 16-byte path
VIEWS = ((35, 41, 53, 29, 1, 47, 3, 4), (34, 520, 520, 0, 4, 531, 17, 1), (71, 1001, 1008, 8, 8, 1016, 16, 8),
         (16, 64, 64, 0, 0, 72, 8, 1), (33, 1, 3, 5, 1, 1, 0, 1), (1, 64, 64, 0, 8, 64, 3, 0), (70, 1002, 1003, 1, 0, 1002, 0, 4))


@pytest.mark.parametrize("view", VIEWS)
def test_pitched_strided_offset_views_and_guards(gpu_ctx, view):
    H, W, ipitch, islack, ioff, opitch, oslack, ooff = view
    rng = np.random.default_rng(zlib.crc32(repr(view).encode()))
    n, gh, gw, guard = 3, 13, 17, 4096
    ifs, ofs = H * ipitch + islack, H * opitch + oslack
    imgs = rng.integers(0, 1 << 16, size=(n, H, W), dtype=np.uint16)
    ibase = torch.from_numpy(rng.integers(0, 1 << 16, size=n * ifs + 64, dtype=np.uint16).view(np.int16)).to(DEV)
    src = _strided(ibase, n, H, W, ifs, ipitch, ioff)
    src.view(torch.int16).copy_(torch.from_numpy(imgs.view(np.int16)).to(DEV))
    before = ibase.clone()
    total = guard + ooff + n * ofs + guard
    obase = torch.full((total,), SENT - 65536, dtype=torch.int16, device=DEV)  # 0xA5A5 as int16
    dst = _strided(obase, n, H, W, ofs, opitch, guard + ooff)
    black, top = (200, 210, 220, 230), 16383
    for form in ("broadcast", "per-frame"):
        gm = _rand_map(rng, gh, gw, n if form == "per-frame" else None)
        res = gpu_ctx.shade(src, _dev16(gm), black=black, top=top, out=dst)
        torch.cuda.synchronize()
        assert res is dst
        want = _want(imgs, gm, black, top)
        expect = np.full(total, SENT, np.uint16)
        ev = np.lib.stride_tricks.as_strided(expect[guard + ooff:], (n, H, W), (ofs * 2, opitch * 2, 2))
        ev[...] = want
        got = obase.cpu().numpy().view(np.uint16)
        assert np.array_equal(got[:guard + ooff], expect[:guard + ooff]) and np.array_equal(got[-guard:], expect[-guard:]), "guards"
        assert np.array_equal(got, expect), (form, np.argwhere(got != expect)[:4].tolist())
        assert torch.equal(ibase, before), "the input was written"
        obase.fill_(SENT - 65536)
    # in place on the strided view: the samples change, what lies between rows and frames does not
    gm = _rand_map(rng, gh, gw)
    res = gpu_ctx.shade(src, _dev16(gm), black=black, top=top, out=src)
    torch.cuda.synchronize()
    expect = before.cpu().numpy().view(np.uint16).copy()
    np.lib.stride_tricks.as_strided(expect[ioff:], (n, H, W), (ifs * 2, ipitch * 2, 2))[...] = _want(imgs, gm, black, top)
    assert np.array_equal(ibase.cpu().numpy().view(np.uint16), expect)


def test_rejections_write_nothing_and_say_why(gpu_ctx):
    w, h, n, gh, gw = 24, 10, 2, 5, 6
    buf = torch.full((8192,), SENT - 65536, dtype=torch.int16, device=DEV)
    mapb = torch.full((4 * 64 * 64 * n + 64,), 4096, dtype=torch.int16, device=DEV)
    base = buf.data_ptr()
    ip, op, mp = base, base + 2 * 4096, mapb.data_ptr()
    assert mp % 16 == 0
    good = dict(s=None, in_ptr=ip, ip=w, ifs=w * h, w=w, h=h, n=n, out_ptr=op, op=w, ofs=w * h)

    def call(sh=None, **kw):
        a = dict(good)
        a.update(kw)
        a["s"] = sh if sh is not None else _shade(mp, gw, gh)
        return _raw(gpu_ctx, a["s"], a["in_ptr"], a["ip"], a["ifs"], a["w"], a["h"], a["n"], a["out_ptr"], a["op"], a["ofs"])

    cases = [
        ("no struct", lambda: _raw(gpu_ctx, None, ip, w, w * h, w, h, n, op, w, w * h)),
        ("NULL in", lambda: call(in_ptr=0)),
        ("NULL out", lambda: call(out_ptr=0)),
        ("NULL map", lambda: call(_shade(0, gw, gh))),
        ("odd in", lambda: call(in_ptr=ip + 1)),
        ("odd out", lambda: call(out_ptr=op + 1)),
        ("map off the 16-byte grid", lambda: call(_shade(mp + 8, gw, gh))),
        ("map off the 16-byte grid by 2", lambda: call(_shade(mp + 2, gw, gh))),
        ("width 0", lambda: call(w=0)),
        ("width 65537", lambda: call(w=65537, ip=65537, op=65537, n=1)),
        ("height 0", lambda: call(h=0)),
        ("height 65537", lambda: call(h=65537, n=1)),
        ("negative width", lambda: call(w=-4)),
        ("in pitch below width", lambda: call(ip=w - 1)),
        ("out pitch below width", lambda: call(op=w - 1)),
        ("in frame stride too small", lambda: call(ifs=w * h - 1)),
        ("out frame stride too small", lambda: call(ofs=(h - 1) * w + w - 1)),
        ("map_w 0", lambda: call(_shade(mp, 0, gh))),
        ("map_w 65", lambda: call(_shade(mp, 65, gh))),
        ("map_h 0", lambda: call(_shade(mp, gw, 0))),
        ("map_h 65", lambda: call(_shade(mp, gw, 65))),
        ("nmaps 0", lambda: call(_shade(mp, gw, gh, nmaps=0))),
        ("nmaps 3 for n 2", lambda: call(_shade(mp, gw, gh, nmaps=3))),
        ("top 0", lambda: call(_shade(mp, gw, gh, top=0))),
        ("top 65536", lambda: call(_shade(mp, gw, gh, top=65536))),
        ("reserved[0]", lambda: call(_shade(mp, gw, gh, reserved=(1, 0)))),
        ("reserved[1]", lambda: call(_shade(mp, gw, gh, reserved=(0, 1)))),
        ("negative n", lambda: call(n=-1)),
        # overlapping extents that are not the in-place case
        ("out inside in", lambda: call(out_ptr=ip + 16)),
        ("out ends inside in", lambda: call(in_ptr=op + 2 * (n * w * h - 8))),
        ("same base, other pitch", lambda: call(out_ptr=ip, op=w + 8, ofs=(w + 8) * h)),
        ("same base, other frame stride", lambda: call(out_ptr=ip, ofs=w * h + 8)),
    ]
    serial = gpu_ctx.last_serial()
    for name, fn in cases:
        rc = fn()
        assert rc < 0, name
        msg = M.load().mcraw_last_error().decode()
        assert msg.startswith("mcraw_shade_batch: ") and len(msg) > len("mcraw_shade_batch: "), name
    assert call(n=0) == 0  # n == 0: a no-op
    torch.cuda.synchronize()
    gpu_ctx.synchronize()
    assert (buf.cpu().numpy().view(np.uint16) == SENT).all()
    assert gpu_ctx.last_serial() == serial
    # good calls next to them do write: out of place with the edges of the ranges (a unit map: the output is the input) ...
    img = torch.arange(n * w * h, dtype=torch.int16, device=DEV)
    buf[:n * w * h].copy_(img)
    assert call(_shade(mp, 64, 64, nmaps=n, top=65535)) == 0
    torch.cuda.synchronize()
    a = buf.cpu().numpy()
    assert np.array_equal(a[4096:4096 + n * w * h], img.cpu().numpy()) and (a[4096 + n * w * h:].view(np.uint16) == SENT).all()
    # ... in place, saturating at top 1 ...
    assert call(_shade(mp, 1, 1, top=1), out_ptr=ip) == 0
    torch.cuda.synchronize()
    a = buf.cpu().numpy()
    assert np.array_equal(a[:n * w * h], np.minimum(img.cpu().numpy(), 1)) and (a[n * w * h:4096].view(np.uint16) == SENT).all()
    # ... and a single frame in place, whose frame strides do not matter
    assert call(n=1, out_ptr=ip, ofs=12345) == 0
    torch.cuda.synchronize()
    # Python: what the wrapper checks itself
    t = torch.zeros((2, 8, 8), dtype=torch.int16, device=DEV).view(torch.uint16)
    for bad in (np.ones((4, 3, 3), np.float32), np.ones((3, 3, 3), np.uint16), np.ones((3, 4, 3, 3), np.uint16)):
        with pytest.raises(ValueError):
            gpu_ctx.shade(t, bad)
    with pytest.raises(ValueError):
        gpu_ctx.shade(t, np.full((4, 3, 3), 4096, np.uint16), out=torch.zeros((2, 8, 9), dtype=torch.int16, device=DEV).view(torch.uint16))
    with pytest.raises(M.McrawError, match="mcraw_shade_batch: .*64"):
        gpu_ctx.shade(t, np.full((4, 3, 65), 4096, np.uint16))
    with pytest.raises(M.McrawError, match="mcraw_shade_batch: .*top"):
        gpu_ctx.shade(t, np.full((4, 3, 3), 4096, np.uint16), top=0)


@pytest.mark.parametrize("mp", ((13, 17), (64, 64)))
def test_same_map_pointer_new_contents_between_queued_calls(gpu_ctx, mp):
    gh, gw = mp
    rng = np.random.default_rng(gh)
    n, h, w = 3, 70, 1002
    imgs = rng.integers(0, 1 << 14, size=(n, h, w), dtype=np.uint16)
    t = _dev16(imgs)
    s = torch.cuda.Stream(DEV)
    dm = torch.empty((4, gh, gw), dtype=torch.int16, device=DEV)
    maps = [_rand_map(rng, gh, gw) for _ in range(4)]
    staged = [torch.from_numpy(x.view(np.int16)).to(DEV) for x in maps]
    torch.cuda.synchronize()
    outs = []
    with torch.cuda.stream(s):
        for k in range(4):  # no host sync between: the map is rewritten in stream order between the calls
            dm.copy_(staged[k])
            outs.append(gpu_ctx.shade(t, dm.view(torch.uint16), black=(64,) * 4, top=16383))
    s.synchronize()
    for k, o in enumerate(outs):
        assert np.array_equal(_np(o), _want(imgs, maps[k], (64,) * 4, 16383)), k


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
    gm = _vignette_map(13, 17)
    kw = dict(algo="mhc", dtype="f16", white=4095.0, black=(64,) * 4, gain=(1.9, 1.0, 1.4), matrix=SRGBISH)
    gpu_ctx.set_float_out("f32", 4095.0, layout="mosaic", black=(64,) * 4)
    try:
        f0 = gpu_ctx.demosaic(t, **kw)
        torch.cuda.synchronize()
        serial, errs = gpu_ctx.last_serial(), gpu_ctx.errors(reset=False)
        res = gpu_ctx.shade(t, gm, black=(64,) * 4, top=4095)
        torch.cuda.synchronize()
        assert gpu_ctx.last_serial() == serial and gpu_ctx.errors(reset=False) == errs
        assert np.array_equal(_np(res), _want(imgs, gm, (64,) * 4, 4095))
        f1 = gpu_ctx.demosaic(t, **kw)
        torch.cuda.synchronize()
        assert torch.equal(f0.view(torch.int16), f1.view(torch.int16))
        # the context's stage is as it was: the next plain batch is still the float mosaic
        o = torch.full((w * h * 4,), 0xA5, dtype=torch.uint8, device=DEV)
        written, status = gpu_ctx.decode_batch(M.Context.make_frames([(ins[0].data_ptr(), ins[0].numel(), w, h, 7, o.data_ptr(), w * h * 2)]))
        assert status == [0]
        import _float_ref as FR
        assert np.array_equal(o.cpu().numpy(), FR.ref_bytes(items[0][1], "f32", 4095.0, "mosaic", (64,) * 4))
    finally:
        gpu_ctx.set_post()
    assert gpu_ctx.errors() == 0


@pytest.mark.parametrize("algo", ("mhc", "bin2"))
def test_demosaic_methods_with_shading(gpu_ctx, algo):
    rng = np.random.default_rng(len(algo))
    n, h, w = 3, 72, 520
    imgs = rng.integers(0, 4096, size=(n, h, w), dtype=np.uint16)
    t = _dev16(imgs)
    black, cfa, gain = (60, 61, 62, 63), "grbg", (1.7, 1.0, 1.4)
    kw = dict(algo=algo, white=4095.0, black=black, cfa=cfa, gain=gain, matrix=SRGBISH)
    for gm in (_vignette_map(13, 17, cfa), np.stack([_vignette_map(5, 9, cfa), _rand_map(rng, 5, 9) & 0x1FFF, _vignette_map(5, 9, cfa)])):
        dm = _dev16(gm)
        shaded = gpu_ctx.shade(t, dm, black=black)
        torch.cuda.synchronize()
        want = _want(imgs, gm, black, 65535)
        assert np.array_equal(_np(shaded), want)
        # linear RGB
        for shading in (dm, gm):  # a device tensor and a host array
            f = gpu_ctx.demosaic(t, dtype="f32", shading=shading, **kw)
            torch.cuda.synchronize()
            assert torch.equal(f.view(torch.int32), gpu_ctx.demosaic(shaded, dtype="f32", **kw).view(torch.int32))
        for i in range(n):
            assert np.array_equal(f[i].cpu().numpy().view(np.uint32),
                                  R.ref_bits(want[i], algo, "f32", 4095.0, black=black, cfa=cfa, gain=gain, matrix=SRGBISH))
        # display-ready RGB
        d = gpu_ctx.demosaic_display(t, transfer="srgb", dtype=torch.uint8, layout="hwc", shading=dm, **kw)
        torch.cuda.synchronize()
        assert torch.equal(d, gpu_ctx.demosaic_display(shaded, transfer="srgb", dtype=torch.uint8, layout="hwc", **kw))
        lut8 = M.transfer_lut("srgb", 4096, 8)
        for i in range(n):
            assert np.array_equal(_np(d[i]), D.display_ref(want[i], algo, 4095.0, lut8, "u8", "hwc", black, cfa, gain, SRGBISH))
        # NV12
        y = gpu_ctx.demosaic_yuv(t, fmt="nv12", shading=dm, **kw)
        torch.cuda.synchronize()
        assert torch.equal(y, gpu_ctx.demosaic_yuv(shaded, fmt="nv12", **kw))
        lut = M.transfer_lut("bt709", 4096, 12)
        coef = M.yuv_matrix("bt709", "limited", 8, 12)
        for i in range(n):
            assert np.array_equal(_np(y[i]), Y.yuv_ref(want[i], algo, 4095.0, lut, "nv12", coef, 12, black, cfa, gain, SRGBISH))
        torch.cuda.synchronize()
        assert np.array_equal(_np(t), imgs), "the caller's mosaic was written"
    # a single (H, W) mosaic, and shading=None is the call as it always was
    one = gpu_ctx.demosaic(t[0], dtype="f16", shading=_vignette_map(13, 17, cfa), **kw)
    plain = gpu_ctx.demosaic(t, dtype="f16", shading=None, **kw)
    torch.cuda.synchronize()
    G, _ = S.gains(h, w, _vignette_map(13, 17, cfa))
    assert np.array_equal(one.cpu().numpy().view(np.uint16),
                          R.ref_bits(S.apply(imgs[0], G, black), algo, "f16", 4095.0, black=black, cfa=cfa, gain=gain, matrix=SRGBISH))
    assert np.array_equal(plain[1].cpu().numpy().view(np.uint16),
                          R.ref_bits(imgs[1], algo, "f16", 4095.0, black=black, cfa=cfa, gain=gain, matrix=SRGBISH))


@pytest.mark.parametrize("typ", (7, 6))
def test_decode_methods_with_shading(gpu_ctx, typ):
    rng = np.random.default_rng(typ)
    w, h = 512, 96
    items = _frames(rng, [(w, h)] * 3, typ)
    ins = [torch.from_numpy(b).to(DEV) for b, _ in items]
    imgs = np.stack([want for _, want in items])
    black, cfa, gain = (64, 64, 64, 64), "bggr", (1.9, 1.0, 1.4)
    gm = np.stack([_vignette_map(13, 17, cfa), _vignette_map(13, 17, cfa) // 2 + 3000, _rand_map(rng, 13, 17) & 0x3FFF])
    want = _want(imgs, gm, black, 65535)
    kw = dict(white=4095.0, black=black, cfa=cfa, gain=gain, matrix=SRGBISH)
    s0 = gpu_ctx.last_serial()
    gpu_ctx.decode_rgb(ins, w, h, typ, algo="bin2", dtype="f16", **kw)
    s1 = gpu_ctx.last_serial()
    for algo in ("mhc", "bin2"):
        out = gpu_ctx.decode_rgb(ins, w, h, typ, algo=algo, dtype="f32", shading=gm, **kw)
        torch.cuda.synchronize()
        for i in range(3):
            assert np.array_equal(out[i].cpu().numpy().view(np.uint32),
                                  R.ref_bits(want[i], algo, "f32", 4095.0, black=black, cfa=cfa, gain=gain, matrix=SRGBISH)), (algo, i)
    d = gpu_ctx.decode_display(ins, w, h, typ, algo="mhc", transfer="srgb", shading=_dev16(gm), **kw)
    y = gpu_ctx.decode_yuv(ins, w, h, typ, algo="bin2", fmt="p010", shading=gm[0], **kw)
    torch.cuda.synchronize()
    lut8, lut16 = M.transfer_lut("srgb", 4096, 8), M.transfer_lut("bt709", 4096, 16)
    coef = M.yuv_matrix("bt709", "limited", 10, 16)
    w0 = _want(imgs, gm[0], black, 65535)
    for i in range(3):
        assert np.array_equal(_np(d[i]), D.display_ref(want[i], "mhc", 4095.0, lut8, "u8", "hwc", black, cfa, gain, SRGBISH))
        assert np.array_equal(_np(y[i]), Y.yuv_ref(w0[i], "bin2", 4095.0, lut16, "p010", coef, 16, black, cfa, gain, SRGBISH))
    assert gpu_ctx.last_serial() == s1 + 4 * (s1 - s0)  # four more decodes; the shading stage takes no serial
    assert gpu_ctx.errors() == 0
