"""The affine warp of the demosaic (mcraw_demosaic_warp_batch; algo="warp" of Context.demosaic / demosaic_display / demosaic_yuv
and the decode_* methods) on the GPU: every output sample equals the numpy statement of the contract (_warp_ref) bit for bit,
with a whole-sample translation it is algo "mhc" cut there, nothing outside `out` is written, rejected calls write nothing, and
the sibling entry points are undisturbed."""
import ctypes as C

import numpy as np
import pytest
import torch

import _rgb_ref as R
import _warp_ref as W
import _yuv_ref as Y
import motioncam_decoder_amd as M
from _demosaic_gpu import CFAS, DEV, GUARD, SENT, SRGBISH
from _demosaic_gpu import dev16 as _dev16, frames as _frames, mosaic as _mosaic, rand_lut as _rand_lut, rgb_color as _color
from _demosaic_gpu import raw_call, rgb_params as _params, to_np as _np
from _demosaic_gpu import FLOATS, IN_BITS, TD, as_int as _as_int, bits as _bits, colours as _colours, display as _display, yuv as _yuv

pytestmark = pytest.mark.gpu

SYM = "mcraw_demosaic_warp_batch"


def _m(ayy=65536, ayx=0, ty=0, axy=0, axx=65536, tx=0):
    return (ayy, ayx, ty, axy, axx, tx)


def _place(lin, size, h, w, fy=0.5, fx=0.5):
    """The map with linear part lin = (ayy, ayx, axy, axx) whose output window sits at fraction (fy, fx) of the room the frame
    leaves it: 0 puts its smallest corner on the frame's first sample, 1 its largest on the last."""
    m = [lin[0], lin[1], 0, lin[2], lin[3], 0]
    Yp, Xp = W.positions(m, size)
    roomy, roomx = 256 * (h - 1) - int(Yp.max() - Yp.min()), 256 * (w - 1) - int(Xp.max() - Xp.min())
    assert roomy >= 0 and roomx >= 0
    m[2], m[5] = -int(Yp.min()) + int(roomy * fy), -int(Xp.min()) + int(roomx * fx)
    assert W.map_ok(m, size, h, w)
    return tuple(m)


def _wparams(white=4095.0, black=(0, 0, 0, 0), cfa="rggb", dtype=1, flags=0, algo=5):
    p = _params("mhc", white, black, cfa, dtype, flags)
    p.algo = algo
    return p


def _warp(size, filt=1, reserved=0):
    w = M.Warp()
    w.out_h, w.out_w = size
    w.filter, w.reserved = filt, reserved
    return w


def _raw(ctx, prm, wp, d, y, cols, ncol, maps, nmaps, in_ptr, pitch, fstride, w, h, n, out_ptr, out_bytes, stream=None):
    """The C entry point as it is: prm, wp, d, y and maps may be None (NULL pointers)."""
    arr = (M.RgbColor * max(ncol, 1))()
    for i in range(min(ncol, len(cols))):
        arr[i] = cols[i]
    ref = [C.byref(s) if s is not None else None for s in (prm, wp, d, y)]
    mp = None
    if maps is not None:
        keep = np.ascontiguousarray(np.asarray(maps, dtype=np.int32).reshape(-1, 6))
        mp = keep.ctypes.data_as(C.POINTER(C.c_int32))
    return getattr(M.load(), SYM)(ctx._h, *ref, arr, ncol, mp, nmaps, C.c_void_p(in_ptr), pitch, fstride, w, h, n, C.c_void_p(out_ptr),
                                  out_bytes, C.c_void_p(stream))


def _values(imgs, maps, size, filt, black, cfa, white, gain, matrix):
    n = len(imgs)
    return [W.values(W.warp_estimates(imgs[i], maps[i if len(maps) > 1 else 0], size, filt, black, cfa), white, black, *_colours(gain, matrix, i))
            for i in range(n)]


def _check_families(ctx, t, imgs, maps, size, cfa="rggb", black=(0, 0, 0, 0), white=4095.0, gain=(1.8, 1.0, 1.3), matrix=SRGBISH,
                    lut=None, filt="cubic", floats=("f32", "f16", "bf16"), display=(("u8", "hwc"), ("u16", "chw")), yuv=None, tag=None):
    """The families and kinds of the Python methods on the (n, h, w) tensor t of the frames imgs against the numpy statement;
    maps: one map, or one per frame."""
    n = len(imgs)
    ho, wo = size
    maps = [tuple(int(v) for v in m) for m in np.asarray(maps).reshape(-1, 6)]
    affine = np.asarray(maps, dtype=np.int32)
    yuv = ((ho % 2 == 0 and wo % 2 == 0) and ("nv12", "p010")) if yuv is None else yuv
    o = _values(imgs, maps, size, filt, black, cfa, white, gain, matrix)
    kw = dict(algo="warp", size=size, affine=affine, filter=filt, white=white, black=black, cfa=cfa, gain=gain, matrix=matrix)
    for dt, view in FLOATS:
        if dt not in floats:
            continue
        clip = dt == "f16"
        out = ctx.demosaic(t, dtype=dt, clip=clip, **kw)
        torch.cuda.synchronize()
        assert tuple(out.shape) == (n, 3, ho, wo)
        got = _bits(out, view)
        for i in range(n):
            want = W.float_bits(np.clip(o[i], np.float32(0), np.float32(1)) if clip else o[i], dt)
            assert np.array_equal(got[i], want), (tag, dt, i)
    lut = _rand_lut(np.random.default_rng(ho * 131 + wo), 4096) if lut is None else lut
    dl = _dev16(lut)
    for dt, layout in display:
        out = ctx.demosaic_display(t, dtype=TD[dt], layout=layout, transfer=dl, **kw)
        torch.cuda.synchronize()
        got = _np(out)
        assert got.shape == ((n, ho, wo, 3) if layout == "hwc" else (n, 3, ho, wo))
        for i in range(n):
            assert np.array_equal(got[i], W.display_from_o(o[i], lut, dt, layout)), (tag, dt, layout, i)
    for fmt in yuv or ():
        out = ctx.demosaic_yuv(t, fmt=fmt, transfer=dl, in_bits=IN_BITS, **kw)
        torch.cuda.synchronize()
        got = _np(out)
        assert got.shape == (n, ho * 3 // 2, wo) and out.dtype == TD[fmt]
        coef = M.yuv_matrix("bt709", "limited", Y.BITS[fmt], IN_BITS)
        for i in range(n):
            assert np.array_equal(got[i], W.yuv_from_o(o[i], lut, fmt, coef, IN_BITS)), (tag, fmt, i)


@pytest.mark.parametrize("cfa", CFAS)
def test_whole_sample_translations_equal_mhc_cut(gpu_ctx, cfa):
    rng = np.random.default_rng(R.CFA_CODE[cfa])
    imgs = [_mosaic(rng, 24, 40, 12) for _ in range(2)]
    t = _dev16(np.stack(imgs))
    kw = dict(white=4095.0, black=(60, 61, 62, 63), cfa=cfa, gain=(1.8, 1.0, 1.3), matrix=SRGBISH)
    dl = _dev16(_rand_lut(rng, 4096))
    h, w = 16, 24
    for y0, x0 in ((2, 4), (0, 0), (8, 16), (3, 7)):
        ar = dict(algo="warp", size=(h, w), affine=np.array(_m(ty=256 * y0, tx=256 * x0), dtype=np.int32))
        for filt in ("cubic", "linear"):
            for dt, view in FLOATS:
                a, b = gpu_ctx.demosaic(t, dtype=dt, filter=filt, **ar, **kw), gpu_ctx.demosaic(t, algo="mhc", dtype=dt, **kw)
                assert torch.equal(a.view(view), b[:, :, y0:y0 + h, x0:x0 + w].contiguous().view(view)), (y0, x0, filt, dt)
            for dt in (torch.uint8, torch.uint16):
                for layout in ("hwc", "chw"):
                    a = gpu_ctx.demosaic_display(t, dtype=dt, layout=layout, transfer=dl, filter=filt, **ar, **kw)
                    b = gpu_ctx.demosaic_display(t, algo="mhc", dtype=dt, layout=layout, transfer=dl, **kw)
                    b = b[:, y0:y0 + h, x0:x0 + w] if layout == "hwc" else b[:, :, y0:y0 + h, x0:x0 + w]
                    assert torch.equal(_as_int(a), _as_int(b.contiguous())), (y0, x0, dt, layout)
            if (y0 | x0) & 1:
                continue  # (mhc's chroma blocks start on even samples)
            for fmt in ("nv12", "p010"):
                a = gpu_ctx.demosaic_yuv(t, fmt=fmt, transfer=dl, in_bits=IN_BITS, filter=filt, **ar, **kw)
                b = gpu_ctx.demosaic_yuv(t, algo="mhc", fmt=fmt, transfer=dl, in_bits=IN_BITS, **kw)
                ya, ca = M.yuv_planes(a, h)
                yb, cb = M.yuv_planes(b, 24)
                assert torch.equal(_as_int(ya), _as_int(yb[:, y0:y0 + h, x0:x0 + w].contiguous())), (y0, x0, fmt)
                assert torch.equal(_as_int(ca), _as_int(cb[:, y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2].contiguous())), (y0, x0, fmt)
    _check_families(gpu_ctx, t, imgs, [_m(ty=256 * 3, tx=256 * 7)], (h, w), cfa, kw["black"], tag=cfa)


@pytest.mark.parametrize("filt", ("cubic", "linear"))
def test_fractional_translations(gpu_ctx, filt):
    rng = np.random.default_rng(3)
    black = (64, 67, 61, 70)
    imgs = [_mosaic(rng, 24, 40, 12) for _ in range(2)]
    t = _dev16(np.stack(imgs))
    one = dict(floats=("f32",), display=(("u8", "hwc"),), yuv=("nv12",))
    for py, px in ((1, 255), (128, 128), (255, 1), (0, 128), (128, 0)):
        _check_families(gpu_ctx, t, imgs, [_m(ty=256 * 3 + py, tx=256 * 9 + px)], (16, 24), "grbg", black, filt=filt, tag=(py, px), **one)
    _check_families(gpu_ctx, t, imgs, [_m(ty=256 * 2 + 77, tx=256 * 5 + 201)], (17, 23), "bggr", black, filt=filt, yuv=False, tag="odd size")


EXTREMES = ((49152, 0, 0, 65536), (81920, 0, 0, 65536), (65536, 0, 0, 49152), (65536, 0, 0, 81920),
            (65536, 16384, 0, 65536), (65536, -16384, 0, 65536), (65536, 0, 16384, 65536), (65536, 0, -16384, 65536),
            (81920, 16384, -16384, 81920), (81920, -16384, 16384, 81920), (49152, 16384, -16384, 49152), (49152, -16384, 16384, 49152))


@pytest.fixture(scope="module")
def big():
    rng = np.random.default_rng(21)
    img = _mosaic(rng, 120, 328, 14)
    return img, _dev16(img[None])


@pytest.mark.parametrize("lin", EXTREMES, ids=lambda v: "%d_%d_%d_%d" % v)
def test_extreme_linear_parts_over_several_tiles(gpu_ctx, big, lin):
    """Each bound of the linear part on its own and all four at once in both roll directions, at both zooms: 40 x 70 pixels span
    2 x 3 tiles, and the last lane of a row holds 6 of its 8 columns.  The window sits off the frame's centre, at a fraction."""
    img, t = big
    size = (40, 70)
    m = _place(lin, size, 120, 328, 0.3, 0.7)
    m = (m[0], m[1], m[2] + 37, m[3], m[4], m[5] - 91) if W.map_ok((m[0], m[1], m[2] + 37, m[3], m[4], m[5] - 91), size, 120, 328) else m
    _check_families(gpu_ctx, t, [img], [m], size, "gbrg", (256, 257, 258, 259), 16383.0, floats=("f16",), display=(("u8", "chw"),),
                    yuv=("nv12",), tag=lin)
    _check_families(gpu_ctx, t, [img], [m], size, "rggb", (256, 257, 258, 259), 16383.0, filt="linear", floats=("f32",), display=(), yuv=(), tag=lin)


@pytest.mark.parametrize("shape", ((8, 8), (40, 72)))
def test_corners_on_the_frames_edges_reflect_on_every_side(gpu_ctx, shape):
    rng = np.random.default_rng(shape[0])
    h, w = shape
    imgs = [_mosaic(rng, h, w, 12) for _ in range(2)]
    t = _dev16(np.stack(imgs))
    one = dict(floats=("f32",), display=(("u16", "hwc"),))
    # the identity over the whole frame: the corners on all four edges at once
    _check_families(gpu_ctx, t, imgs, [_m()], (h, w), "grbg", (64, 64, 64, 64), tag="whole", **one)
    # half a sample short of the last row and column, and fractional zooms whose far corners land exactly on the edges
    size = (h - 2, w - 2) if h == 8 else (30, 54)  # (room for the zoom-out's 1.0625 samples per pixel)
    for lin in ((65536, 0, 0, 65536), (65536 + 4096, 2048, -2048, 65536 + 1024), (65536 - 4096, -1024, 1024, 65536 - 2048)):
        for fy in (0.0, 1.0):
            for fx in (0.0, 1.0):
                m = _place(lin, size, h, w, fy, fx)
                Yp, Xp = W.positions(m, size)
                assert (Yp.min() == 0 if fy == 0 else Yp.max() == 256 * (h - 1)) and (Xp.min() == 0 if fx == 0 else Xp.max() == 256 * (w - 1))
                _check_families(gpu_ctx, t, imgs, [m], size, "gbrg", (64, 64, 64, 64), tag=(lin, fy, fx), **one)


def test_35_frames_cross_a_piece_with_per_frame_maps_and_colours(gpu_ctx):
    rng = np.random.default_rng(9)
    n, h, w, size = 35, 16, 24, (10, 14)
    imgs = [_mosaic(rng, h, w, 12) for _ in range(n)]
    t = _dev16(np.stack(imgs))
    gain = np.stack([np.array([1.0 + 0.03 * i, 1.0, 2.0 - 0.02 * i], np.float32) for i in range(n)])
    matrix = np.stack([SRGBISH * np.float32(1.0 - 0.005 * i) for i in range(n)])
    maps = [_place((65536 + 300 * (i - 17), 400 * (i - 17), -350 * (i - 17), 65536 - 200 * (i - 17)), size, h, w, (i % 7) / 6.0, (i % 5) / 4.0)
            for i in range(n)]
    assert len(set(maps)) == n
    one = dict(floats=("f16",), display=(("u8", "hwc"),), yuv=("nv12",))
    _check_families(gpu_ctx, t, imgs, maps, size, "bggr", (60, 61, 62, 63), gain=gain, matrix=matrix, tag="per frame", **one)
    _check_families(gpu_ctx, t, imgs, maps, size, "bggr", (60, 61, 62, 63), tag="maps per frame, one colour", floats=("f32",), display=(), yuv=())
    _check_families(gpu_ctx, t, imgs, [maps[3]], size, "bggr", (60, 61, 62, 63), gain=gain, matrix=matrix, tag="one map, colours per frame",
                    floats=("f32",), display=(), yuv=())
    # nmaps = 1 against nmaps = n with equal maps
    kw = dict(algo="warp", size=size, white=4095.0, dtype="f32")
    a = gpu_ctx.demosaic(t, affine=np.asarray(maps[5], dtype=np.int32), **kw)
    b = gpu_ctx.demosaic(t, affine=np.asarray([maps[5]] * n, dtype=np.int32), **kw)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_strided_input_misaligned_out_sentinels(gpu_ctx):
    rng = np.random.default_rng(8)
    n, h, w, pitch = 3, 36, 68, 83
    fstride = h * pitch + 29
    size = (27, 45)
    maps = [_place((65536 + 2000 * i, 3000, -3000, 65536 - 1500 * i), size, h, w, 0.4, 0.6) for i in range(n)]
    imgs = [_mosaic(rng, h, w, 14) for _ in range(n)]
    base = torch.from_numpy(rng.integers(0, 1 << 16, size=n * fstride + 64, dtype=np.uint16).view(np.int16)).to(DEV)
    v16 = torch.as_strided(base, (n, h, w), (fstride, pitch, 1), 5)  # an odd element offset, an odd pitch: uint16 loads
    for i in range(n):
        v16[i].copy_(torch.from_numpy(imgs[i].view(np.int16)).to(DEV))
    view = v16.view(torch.uint16)
    before = base.clone()
    black = (512, 500, 510, 520)
    lut = _rand_lut(rng, 4096)
    dl = _dev16(lut)
    kw = dict(algo="warp", size=size, affine=np.asarray(maps, dtype=np.int32), white=16383.0, black=black, cfa="bggr", gain=(1.4, 1.0, 1.9),
              matrix=SRGBISH)
    o = _values(imgs, maps, size, "cubic", black, "bggr", 16383.0, (1.4, 1.0, 1.9), SRGBISH)
    coef = M.yuv_matrix("bt709", "limited", 8, IN_BITS)
    size2 = (26, 44)
    o2 = _values(imgs, maps, size2, "cubic", black, "bggr", 16383.0, (1.4, 1.0, 1.9), SRGBISH)
    kw2 = dict(kw, size=size2)
    packed = gpu_ctx.demosaic(_dev16(np.stack(imgs)), dtype="f16", **kw)  # the 16-byte path beside it: the same frames on the grid
    cases = [("f16", torch.float16, (n, 3) + size, lambda out: gpu_ctx.demosaic(view, dtype="f16", out=out, **kw),
              lambda i: W.float_bits(o[i], "f16")),
             ("u8", torch.uint8, (n,) + size + (3,), lambda out: gpu_ctx.demosaic_display(view, transfer=dl, out=out, **kw),
              lambda i: W.display_from_o(o[i], lut, "u8", "hwc")),
             ("u16", torch.uint16, (n, 3) + size, lambda out: gpu_ctx.demosaic_display(view, transfer=dl, dtype=torch.uint16, layout="chw",
                                                                                      out=out, **kw),
              lambda i: W.display_from_o(o[i], lut, "u16", "chw")),
             ("nv12", torch.uint8, (n, size2[0] * 3 // 2, size2[1]), lambda out: gpu_ctx.demosaic_yuv(view, transfer=dl, in_bits=IN_BITS, out=out, **kw2),
              lambda i: W.yuv_from_o(o2[i], lut, "nv12", coef, IN_BITS))]
    for name, td, shape, run, want in cases:
        es = torch.empty((), dtype=td).element_size()
        nbytes = int(np.prod(shape)) * es
        for misalign in (0, es, 8 + es):
            buf = torch.full((nbytes + 2 * GUARD + 64,), SENT, dtype=torch.uint8, device=DEV)
            skew = (-buf.data_ptr()) % 64 + misalign
            out = buf[GUARD + skew:GUARD + skew + nbytes].view(td).view(shape)
            run(out)
            torch.cuda.synchronize()
            host = buf.cpu().numpy()
            assert (host[:GUARD + skew] == SENT).all() and (host[GUARD + skew + nbytes:] == SENT).all(), (name, misalign)
            got = host[GUARD + skew:GUARD + skew + nbytes].view({1: np.uint8, 2: np.uint16}[es]).reshape(shape)
            for i in range(n):
                assert np.array_equal(got[i], want(i)), (name, misalign, i)
    assert torch.equal(base, before)  # the input, and the gaps between its rows and frames, are as they were
    assert np.array_equal(_bits(packed, torch.int16), np.stack([W.float_bits(o[i], "f16") for i in range(n)]))


@pytest.mark.parametrize("entries", (256, 65536))
def test_lut_sizes_lds_and_global(gpu_ctx, entries):
    rng = np.random.default_rng(entries)
    imgs = [_mosaic(rng, 40, 72, 10) for _ in range(2)]
    t = _dev16(np.stack(imgs))
    m = _place((65536 + 3000, -5000, 5000, 65536 + 3000), (34, 38), 40, 72, 0.5, 0.2)
    _check_families(gpu_ctx, t, imgs, [m], (34, 38), "grbg", (16, 16, 16, 16), 1023.0, lut=_rand_lut(rng, entries), floats=(), tag=entries)


def test_p010_u16_bf16_at_16_bits(gpu_ctx):
    rng = np.random.default_rng(16)
    imgs = [_mosaic(rng, 24, 40, 16) for _ in range(2)]
    t = _dev16(np.stack(imgs))
    m = _place((65536 - 9000, 7000, -7000, 65536 - 9000), (18, 26), 24, 40, 0.5, 0.5)
    _check_families(gpu_ctx, t, imgs, [m], (18, 26), "rggb", (1024, 1000, 1010, 1030), 65535.0, floats=("bf16",), display=(("u16", "hwc"), ("u16", "chw")),
                    yuv=("p010",))


def test_rejections_write_nothing(gpu_ctx):
    rng = np.random.default_rng(10)
    h, w, n, size = 24, 40, 2, (12, 16)
    t = _dev16(np.stack([_mosaic(rng, h, w, 12) for _ in range(n)]))
    out = torch.full((n * 3 * size[0] * size[1] * 4,), SENT, dtype=torch.uint8, device=DEV)
    lut = _dev16(_rand_lut(rng, 4096))
    cols = [_color()]
    ok = _m(ty=256 * 3, tx=256 * 5)
    good = dict(prm=_wparams(), wp=_warp(size), d=None, y=None, ncol=1, maps=[ok], nmaps=1, inp=t.data_ptr(), pitch=w, fstride=w * h, w=w, h=h, n=n,
                out=out.data_ptr(), out_bytes=out.numel())

    def call(**kw):
        a = dict(good, **kw)
        rc = _raw(gpu_ctx, a["prm"], a["wp"], a["d"], a["y"], cols, a["ncol"], a["maps"], a["nmaps"], a["inp"], a["pitch"], a["fstride"], a["w"],
                  a["h"], a["n"], a["out"], a["out_bytes"])
        return rc, M.load().mcraw_last_error().decode()

    bad = [dict(prm=None), dict(wp=None), dict(maps=None), dict(prm=_wparams(algo=1)), dict(prm=_wparams(algo=4)), dict(wp=_warp(size, reserved=1)),
           dict(wp=_warp(size, filt=2)), dict(wp=_warp((0, 16))), dict(d=_display(lut.data_ptr()), y=_yuv(lut.data_ptr()), prm=_wparams(dtype=0)),
           dict(y=_yuv(lut.data_ptr()), prm=_wparams(dtype=0), wp=_warp((12, 15))), dict(nmaps=0), dict(maps=[ok] * 3, nmaps=3), dict(ncol=0),
           dict(w=6), dict(out_bytes=out.numel() - 1), dict(out=out.data_ptr() + 2),
           dict(maps=[_m(ty=-1)]), dict(maps=[_m(ty=256 * 12 + 1)]), dict(maps=[_m(tx=256 * 24 + 1)]), dict(maps=[_m(ayy=65536 + 16385)]),
           dict(maps=[ok, _m(ayx=16385, ty=256 * 3, tx=256 * 5)], nmaps=2)]
    for kw in bad:
        rc, msg = call(**kw)
        assert rc < 0 and msg.startswith(SYM + ": "), (kw, rc, msg)
    assert "frame 1" in msg
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
    rc, msg = call(n=0, maps=[_m(ty=-1)])
    torch.cuda.synchronize()
    assert rc == 0 and bool((out == SENT).all())
    # the bounds themselves are accepted
    for m in (_m(ty=256 * 12, tx=256 * 24), _m(), _m(ayy=81920, ty=0, tx=0)):
        rc, msg = call(maps=[m])
        assert rc == 0, (m, msg)
    torch.cuda.synchronize()
    # the siblings keep rejecting algo 5
    rc = raw_call(gpu_ctx, "mcraw_demosaic_batch", _wparams(), None, cols, 1, t.data_ptr(), w, w * h, w, h, n, out.data_ptr(), out.numel(), staged=False)
    assert rc < 0 and "unknown algo" in M.load().mcraw_last_error().decode()


def test_python_argument_rules(gpu_ctx):
    rng = np.random.default_rng(11)
    t = _dev16(np.stack([_mosaic(rng, 24, 40, 12) for _ in range(2)]))
    ident = np.array(_m(ty=256, tx=512), dtype=np.int32)
    kw = dict(dtype="f32", white=4095.0)
    for algo in ("mhc", "bin2"):
        with pytest.raises(ValueError):
            gpu_ctx.demosaic(t, algo=algo, affine=ident, **kw)
    with pytest.raises(ValueError):
        gpu_ctx.demosaic(t, algo="resample", size=(12, 20), affine=ident, **kw)
    with pytest.raises(ValueError):
        gpu_ctx.demosaic(t, algo="area", size=(12, 20), affine=ident, **kw)
    with pytest.raises(ValueError):
        gpu_ctx.demosaic(t, algo="warp", affine=ident, **kw)
    with pytest.raises(ValueError):
        gpu_ctx.demosaic(t, algo="warp", size=(12, 20), **kw)
    with pytest.raises(ValueError):
        gpu_ctx.demosaic(t, algo="warp", size=(12, 20), affine=ident, crop=(0, 0, 24, 40), **kw)
    with pytest.raises(ValueError):
        gpu_ctx.demosaic(t, algo="warp", size=(12, 20), affine=ident, filter="lanczos", **kw)
    for algo, extra in (("mhc", {}), ("bin2", {}), ("area", dict(size=(6, 10)))):
        with pytest.raises(ValueError):
            gpu_ctx.demosaic(t, algo=algo, filter="cubic", **extra, **kw)
    for bad in (np.zeros((3, 6), np.int32), np.zeros((6,), np.int64), np.zeros((2, 2), np.float64), np.zeros((3, 2, 3)), "x"):
        with pytest.raises(ValueError):
            gpu_ctx.demosaic(t, algo="warp", size=(12, 20), affine=bad, **kw)
    with pytest.raises(ValueError):
        M.fit_crop(24, 40, 12, 20, algo="warp")
    with pytest.raises(M.McrawError):  # the library's own rule: a corner outside the frame
        gpu_ctx.demosaic(t, algo="warp", size=(24, 40), affine=ident, **kw)
    # the forms of affine=: int32 (6,) and (N, 6), float (2, 3) and (N, 2, 3), numpy and torch, host and device
    f = np.array([[1.0, 0.0, 1.0], [0.0, 1.0, 2.0]])
    want = gpu_ctx.demosaic(t, algo="warp", size=(12, 20), affine=ident, **kw).view(torch.int32)
    for a in (np.stack([ident, ident]), f, np.stack([f, f]), f.astype(np.float32), torch.from_numpy(ident), torch.from_numpy(ident).to(DEV),
              torch.from_numpy(f), torch.from_numpy(np.stack([f, f])).to(DEV)):
        assert torch.equal(gpu_ctx.demosaic(t, algo="warp", size=(12, 20), affine=a, **kw).view(torch.int32), want)
    assert torch.equal(want, gpu_ctx.demosaic(t, algo="mhc", **kw)[:, :, 1:13, 2:22].contiguous().view(torch.int32))
    # an (H, W) mosaic drops N; out= is checked
    one = gpu_ctx.demosaic(t[0], algo="warp", size=(12, 20), affine=ident, **kw)
    assert tuple(one.shape) == (3, 12, 20) and torch.equal(one.view(torch.int32), want[0])
    with pytest.raises(ValueError):
        gpu_ctx.demosaic(t, algo="warp", size=(12, 20), affine=ident, out=torch.empty((2, 3, 12, 21), dtype=torch.float32, device=DEV), **kw)
    empty = gpu_ctx.demosaic(t[:0], algo="warp", size=(12, 20), affine=ident, **kw)
    assert tuple(empty.shape) == (0, 3, 12, 20)


@pytest.mark.parametrize("typ", (7, 6))
def test_decode_yuv_warp_equals_demosaic_yuv_of_the_plain_decode(gpu_ctx, typ):
    rng = np.random.default_rng(typ)
    items = _frames(rng, [(64, 32)] * 3, typ)
    ins = [torch.from_numpy(buf).to(DEV) for buf, _ in items]
    size = (24, 48)
    maps = np.asarray([_place((65536 + 1500 * i, 2500 * (i - 1), -2500 * (i - 1), 65536 + 1500 * i), size, 32, 64, 0.5, 0.5) for i in range(3)],
                      dtype=np.int32)
    kw = dict(white=4095.0, black=(64, 64, 64, 64), cfa="grbg", gain=(1.9, 1.0, 1.5), matrix=SRGBISH, algo="warp", size=size, affine=maps,
              filter="cubic")
    plain = _dev16(np.stack([want for _, want in items]))
    for fmt in ("nv12", "p010"):
        a = gpu_ctx.decode_yuv(ins, 64, 32, typ, fmt=fmt, **kw)
        b = gpu_ctx.demosaic_yuv(plain, fmt=fmt, **kw)
        assert tuple(a.shape) == (3, 36, 48) and torch.equal(_as_int(a), _as_int(b))
    a = gpu_ctx.decode_rgb(ins, 64, 32, typ, dtype="f16", **kw)
    assert torch.equal(a.view(torch.int16), gpu_ctx.demosaic(plain, dtype="f16", **kw).view(torch.int16))
    a = gpu_ctx.decode_display(ins, 64, 32, typ, **kw)
    assert torch.equal(a, gpu_ctx.demosaic_display(plain, **kw))
    _check_families(gpu_ctx, plain, [want for _, want in items], maps, size, "grbg", (64, 64, 64, 64), floats=("f32",), display=(), yuv=("nv12",))


def test_stages_in_front_equal_the_stages_run_by_hand(gpu_ctx):
    rng = np.random.default_rng(12)
    imgs = np.stack([_mosaic(rng, 48, 96, 11) for _ in range(2)]) + 64
    imgs[:, 5::11, 7::13] = 4000  # defects to find
    t = _dev16(imgs)
    black, cfa = (64, 64, 64, 64), "grbg"
    lut, shift = M.noise_lut(S=2e-4, O=2e-6, black=64, white=4095)
    denoise = dict(lut=lut, shift=shift, radius=2, amount=0.75)
    defects = dict(abs_thr=200, rel_thr=26 / 256, rank=2)
    y, x = np.linspace(-1, 1, 13)[:, None], np.linspace(-1, 1, 17)[None, :]
    gm = M.gain_map(np.stack([1.0 + (s - 1.0) * (x * x + y * y) / 2 for s in (1.9, 1.4, 1.45, 2.3)]), cfa)
    three = gpu_ctx.shade(gpu_ctx.denoise(gpu_ctx.fix_pixels(t, black=black, **defects), **denoise), gm, black=black)
    assert not torch.equal(three.view(torch.int16), t.view(torch.int16))
    size = (30, 62)
    m = np.asarray(_place((65536 - 2000, 4000, -4000, 65536 - 2000), size, 48, 96), dtype=np.int32)
    kw = dict(algo="warp", size=size, affine=m, white=4095.0, black=black, cfa=cfa, gain=(1.7, 1.0, 1.4), matrix=SRGBISH)
    a = gpu_ctx.demosaic(t, dtype="f32", defects=defects, denoise=denoise, shading=gm, **kw)
    assert torch.equal(a.view(torch.int32), gpu_ctx.demosaic(three, dtype="f32", **kw).view(torch.int32))
    assert not torch.equal(a.view(torch.int32), gpu_ctx.demosaic(t, dtype="f32", **kw).view(torch.int32))
    b = gpu_ctx.demosaic_yuv(t, defects=defects, denoise=denoise, shading=gm, **kw)
    assert torch.equal(b, gpu_ctx.demosaic_yuv(three, **kw))
    host = _np(three)
    ref = np.stack([W.warp_ref(host[i], m, size, "f32", 4095.0, "cubic", black, cfa, (1.7, 1.0, 1.4), SRGBISH) for i in range(2)])
    assert np.array_equal(_bits(a, torch.int32), ref)


def test_siblings_are_unchanged_by_interleaved_warp_calls(gpu_ctx):
    rng = np.random.default_rng(13)
    imgs = [_mosaic(rng, 40, 72, 12) for _ in range(2)]
    t = _dev16(np.stack(imgs))
    kw = dict(dtype="f16", white=4095.0, black=(60, 61, 62, 63), cfa="gbrg", gain=(1.5, 1.0, 1.7), matrix=SRGBISH)
    res = dict(algo="resample", size=(30, 50), crop=(2, 4, 36, 64))
    m = np.asarray(_place((65536 + 5000, -6000, 6000, 65536 + 5000), (28, 44), 40, 72), dtype=np.int32)
    mhc0, res0 = gpu_ctx.demosaic(t, algo="mhc", **kw), gpu_ctx.demosaic(t, **res, **kw)
    w0 = gpu_ctx.demosaic(t, algo="warp", size=(28, 44), affine=m, **kw)
    for _ in range(3):
        w1 = gpu_ctx.demosaic(t, algo="warp", size=(28, 44), affine=m, **kw)
        mhc1 = gpu_ctx.demosaic(t, algo="mhc", **kw)
        w2 = gpu_ctx.demosaic_display(t, algo="warp", size=(28, 44), affine=m, white=4095.0)
        res1 = gpu_ctx.demosaic(t, **res, **kw)
        assert torch.equal(mhc0.view(torch.int16), mhc1.view(torch.int16)) and torch.equal(res0.view(torch.int16), res1.view(torch.int16))
        assert torch.equal(w0.view(torch.int16), w1.view(torch.int16))
    want = np.stack([R.ref_bits(imgs[i], "mhc", "f16", 4095.0, black=kw["black"], cfa="gbrg", gain=kw["gain"], matrix=SRGBISH) for i in range(2)])
    assert np.array_equal(_bits(mhc0, torch.int16), want)
    assert w2.shape == (2, 28, 44, 3)


def test_flat_and_grey_stay_flat_and_neutral(gpu_ctx):
    flat = np.full((2, 64, 96), 1234, dtype=np.uint16)
    grey = np.zeros((2, 64, 96), dtype=np.uint16)
    for p, b in enumerate((60, 70, 80, 90)):
        grey[:, p >> 1::2, p & 1::2] = 1000 + b
    size = (30, 46)
    for lin in ((65536, 0, 0, 65536), (81920, 16384, -16384, 81920), (49152, -16384, 16384, 49152), (65536 + 777, 3333, -2222, 65536 - 999)):
        m = np.asarray(_place(lin, size, 64, 96, 0.37, 0.61), dtype=np.int32)
        m[2] += 19 if W.map_ok(tuple(m + np.array([0, 0, 19, 0, 0, 0])), size, 64, 96) else 0
        for filt in ("cubic", "linear"):
            a = gpu_ctx.demosaic(_dev16(flat), algo="warp", size=size, affine=m, filter=filt, dtype="f32", white=4095.0, black=(64, 64, 64, 64), cfa="grbg")
            v = np.float32(16 * (1234 - 64)) * np.float32((np.float32(1.0) * (np.float32(1.0) / np.float32(4095.0 - 64.0))) * np.float32(0.0625))
            assert bool((a == float(v)).all()), (lin, filt)
            g = gpu_ctx.demosaic(_dev16(grey), algo="warp", size=size, affine=m, filter=filt, dtype="f32", white=4095.0, black=(60, 70, 80, 90), cfa="bggr")
            assert bool((g[:, 0] == g[:, 1]).all()) and bool((g[:, 1] == g[:, 2]).all()) and bool((g == g[0, 0, 0, 0]).all()), (lin, filt)
