"""The area downscale (mcraw_demosaic_area_batch; algo="area" of Context.demosaic / demosaic_display / demosaic_yuv and the
decode_* methods) on the GPU: every output sample equals the numpy statement of the contract (_area_ref) bit for bit, nothing
outside `out` and `work` is written, rejected calls write nothing, queued calls share neither LUT contents nor scratch, and the
sibling entry points are undisturbed."""
import numpy as np
import pytest
import torch

import _area_ref as A
import _display_ref as D
import _rgb_ref as R
import _yuv_ref as Y
import motioncam_decoder_amd as M
from _demosaic_gpu import CFAS, DEV, GUARD, SENT, SRGBISH
from _demosaic_gpu import dev16 as _dev16, frames as _frames, mosaic as _mosaic, rand_lut as _rand_lut, rgb_color as _color
from _demosaic_gpu import rgb_params as _params, to_np as _np
from _demosaic_gpu import FLOATS, IN_BITS, TD, as_int as _as_int, bits as _bits, colours as _colours, display as _display, yuv as _yuv
from _demosaic_gpu import raw_scaled_call, work_bytes

pytestmark = pytest.mark.gpu

SYM = "mcraw_demosaic_area_batch"


def _aparams(white=4095.0, black=(0, 0, 0, 0), cfa="rggb", dtype=1, flags=0, algo=3):
    """mcraw_rgb for the area call: dtype 1 = MCRAW_FLOAT_F32 (the display and YUV families take 0)."""
    p = _params("bin2", white, black, cfa, dtype, flags)
    p.algo = algo
    return p


def _area(crop, size, reserved=(0, 0)):
    a = M.Area()
    a.y0, a.x0, a.ch, a.cw = crop
    a.out_h, a.out_w = size
    a.reserved[0], a.reserved[1] = reserved
    return a


def _raw(ctx, *args, **kw):
    """The C entry point as it is: prm, area, d and y may be None (NULL pointers)."""
    return raw_scaled_call(SYM, ctx, *args, **kw)


def _work_bytes(crop, size):
    return work_bytes("mcraw_area_work_bytes", _area(crop, size))


def _check_families(ctx, t, imgs, crop, size, cfa="rggb", black=(0, 0, 0, 0), white=4095.0, gain=(1.8, 1.0, 1.3), matrix=SRGBISH,
                    lut=None, floats=True, display=True, yuv=None, tag=None):
    """Every family and kind of the Python methods on the (n, h, w) tensor t of the frames imgs against the numpy statement."""
    n = len(imgs)
    h, w = imgs[0].shape
    ccrop = (0, 0, h, w) if crop is None else crop
    ho, wo = size
    yuv = (ho % 2 == 0 and wo % 2 == 0) if yuv is None else yuv
    o = [A.values(A.area_estimates(imgs[i], ccrop, size, black, cfa), white, black, *_colours(gain, matrix, i)) for i in range(n)]
    kw = dict(algo="area", size=size, crop=crop, white=white, black=black, cfa=cfa, gain=gain, matrix=matrix)
    if floats:
        for dt, view in FLOATS:
            clip = dt == "f16"
            out = ctx.demosaic(t, dtype=dt, clip=clip, **kw)
            torch.cuda.synchronize()
            assert tuple(out.shape) == (n, 3, ho, wo)
            got = _bits(out, view)
            for i in range(n):
                want = A.float_bits(np.clip(o[i], np.float32(0), np.float32(1)) if clip else o[i], dt)
                assert np.array_equal(got[i], want), (tag, dt, i)
    lut = _rand_lut(np.random.default_rng(ho * 131 + wo), 4096) if lut is None else lut
    dl = _dev16(lut)
    if display:
        for dt in ("u8", "u16"):
            for layout in ("hwc", "chw"):
                out = ctx.demosaic_display(t, dtype=TD[dt], layout=layout, transfer=dl, **kw)
                torch.cuda.synchronize()
                got = _np(out)
                assert got.shape == ((n, ho, wo, 3) if layout == "hwc" else (n, 3, ho, wo))
                for i in range(n):
                    assert np.array_equal(got[i], A.display_from_o(o[i], lut, dt, layout)), (tag, dt, layout, i)
    if yuv:
        for fmt in ("nv12", "p010"):
            out = ctx.demosaic_yuv(t, fmt=fmt, transfer=dl, in_bits=IN_BITS, **kw)
            torch.cuda.synchronize()
            got = _np(out)
            assert got.shape == (n, ho * 3 // 2, wo) and out.dtype == TD[fmt]
            coef = M.yuv_matrix("bt709", "limited", Y.BITS[fmt], IN_BITS)
            for i in range(n):
                assert np.array_equal(got[i], Y.yuv_from_o(o[i], lut, fmt, coef, IN_BITS)), (tag, fmt, i)
            yp, cp = M.yuv_planes(out, ho)
            assert tuple(yp.shape) == (n, ho, wo) and tuple(cp.shape) == (n, ho // 2, wo // 2, 2)


@pytest.mark.parametrize("cfa", CFAS)
def test_one_quad_per_pixel_equals_bin2(gpu_ctx, cfa):
    rng = np.random.default_rng(R.CFA_CODE[cfa])
    imgs = [_mosaic(rng, 16, 24, 12) for _ in range(2)]
    t = _dev16(np.stack(imgs))
    kw = dict(white=4095.0, black=(60, 61, 62, 63), cfa=cfa, gain=(1.8, 1.0, 1.3), matrix=SRGBISH)
    ar = dict(algo="area", size=(8, 12))
    dl = _dev16(_rand_lut(rng, 4096))
    for dt, view in FLOATS:
        a, b = gpu_ctx.demosaic(t, dtype=dt, **ar, **kw), gpu_ctx.demosaic(t, algo="bin2", dtype=dt, **kw)
        assert torch.equal(a.view(view), b.view(view)), dt
    for dt in (torch.uint8, torch.uint16):
        for layout in ("hwc", "chw"):
            a = gpu_ctx.demosaic_display(t, dtype=dt, layout=layout, transfer=dl, **ar, **kw)
            b = gpu_ctx.demosaic_display(t, algo="bin2", dtype=dt, layout=layout, transfer=dl, **kw)
            assert torch.equal(_as_int(a), _as_int(b)), (dt, layout)
    for fmt in ("nv12", "p010"):
        a = gpu_ctx.demosaic_yuv(t, fmt=fmt, transfer=dl, in_bits=IN_BITS, **ar, **kw)
        b = gpu_ctx.demosaic_yuv(t, algo="bin2", fmt=fmt, transfer=dl, in_bits=IN_BITS, **kw)
        assert torch.equal(_as_int(a), _as_int(b)), fmt
    _check_families(gpu_ctx, t, imgs, None, (8, 12), cfa, kw["black"], tag=cfa)


def test_fractional_ratios_offset_crop_off_the_grid(gpu_ctx):
    rng = np.random.default_rng(3)
    imgs = [_mosaic(rng, 36, 52, 12) for _ in range(2)]  # rows of 104 bytes: off the 16-byte grid
    for cfa in ("grbg", "bggr"):
        _check_families(gpu_ctx, _dev16(np.stack(imgs)), imgs, (2, 6, 30, 42), (6, 10), cfa, (64, 65, 66, 67), tag=cfa)


def test_seventeen_taps_full_range_samples(gpu_ctx):
    rng = np.random.default_rng(4)
    imgs = [(rng.integers(0, 2, size=(96, 128)) * 65535).astype(np.uint16) for _ in range(2)]
    t = _dev16(np.stack(imgs))
    assert int((A.weights(63, 4)[1] > 0).sum(axis=1).max()) == 17 and int((A.weights(47, 3)[1] > 0).sum(axis=1).max()) == 17
    kw = dict(cfa="gbrg", black=(64, 64, 64, 64), white=65535.0, gain=(1.0, 1.0, 1.0), matrix=np.eye(3, dtype=np.float32))
    _check_families(gpu_ctx, t, imgs, (2, 2, 94, 126), (3, 4), yuv=False, tag="3x4", **kw)
    _check_families(gpu_ctx, t, imgs, (2, 2, 94, 126), (4, 4), floats=False, display=False, yuv=True, tag="4x4", **kw)


def test_ratio_limit(gpu_ctx):
    rng = np.random.default_rng(5)
    imgs = [_mosaic(rng, 64, 64, 14)]
    _check_families(gpu_ctx, _dev16(np.stack(imgs)), imgs, None, (2, 2), "bggr", (256, 257, 258, 259), 16383.0)


@pytest.mark.parametrize("wo", (1, 7, 9, 10, 15))
def test_last_lane_holds_a_part_of_its_columns(gpu_ctx, wo):
    rng = np.random.default_rng(wo)
    imgs = [_mosaic(rng, 12, 5 * wo + 2 + wo % 2, 12) for _ in range(2)]  # about 2.5 quads per pixel, and columns to spare
    _check_families(gpu_ctx, _dev16(np.stack(imgs)), imgs, (0, 2, 12, 5 * wo - wo % 2), (2, wo), "grbg", (10, 20, 30, 40), tag=wo)


def test_row_wider_than_one_workgroup(gpu_ctx):
    rng = np.random.default_rng(6)
    imgs = [_mosaic(rng, 8, 4112, 12)]
    _check_families(gpu_ctx, _dev16(np.stack(imgs)), imgs, None, (2, 2050), "rggb", (64, 64, 64, 64))


def test_strided_input_misaligned_out_sentinels(gpu_ctx):
    rng = np.random.default_rng(7)
    n, h, w, pitch = 3, 36, 68, 83
    fstride = h * pitch + 29
    crop, size = (4, 2, 30, 62), (7, 13)
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
    kw = dict(algo="area", size=size, crop=crop, white=16383.0, black=black, cfa="bggr", gain=(1.4, 1.0, 1.9), matrix=SRGBISH)
    o = [A.values(A.area_estimates(imgs[i], crop, size, black, "bggr"), 16383.0, black, (1.4, 1.0, 1.9), SRGBISH) for i in range(n)]
    cases = [("f16", torch.float16, (n, 3) + size, lambda out: gpu_ctx.demosaic(view, dtype="f16", out=out, **kw),
              lambda i: A.float_bits(o[i], "f16")),
             ("u8", torch.uint8, (n,) + size + (3,), lambda out: gpu_ctx.demosaic_display(view, transfer=dl, out=out, **kw),
              lambda i: A.display_from_o(o[i], lut, "u8", "hwc")),
             ("u16", torch.uint16, (n, 3) + size, lambda out: gpu_ctx.demosaic_display(view, transfer=dl, dtype=torch.uint16, layout="chw",
                                                                                      out=out, **kw),
              lambda i: A.display_from_o(o[i], lut, "u16", "chw"))]
    for name, td, shape, run, want in cases:
        es = torch.empty((), dtype=td).element_size()
        nbytes = int(np.prod(shape)) * es
        for misalign in (0, es, 8 + es):
            buf = torch.full((GUARD + misalign + nbytes + GUARD,), SENT, dtype=torch.uint8, device=DEV)
            out = buf[GUARD + misalign: GUARD + misalign + nbytes].view(td).view(shape)
            run(out)
            torch.cuda.synchronize()
            a = buf.cpu().numpy()
            assert (a[:GUARD + misalign] == SENT).all() and (a[GUARD + misalign + nbytes:] == SENT).all(), (name, misalign)
            got = a[GUARD + misalign: GUARD + misalign + nbytes].view(np.uint8 if es == 1 else np.uint16).reshape(shape)
            for i in range(n):
                assert np.array_equal(got[i], want(i)), (name, misalign, i)
    # the C entry point with sentinels round `work` as well (its strides in elements, as the Python layer passes them)
    need = _work_bytes(crop, size)
    wbuf = torch.full((GUARD + need + GUARD,), SENT, dtype=torch.uint8, device=DEV)
    nbytes = n * 3 * size[0] * size[1] * 4
    obuf = torch.full((GUARD + nbytes + GUARD,), SENT, dtype=torch.uint8, device=DEV)
    rc = _raw(gpu_ctx, _aparams(16383.0, black, "bggr"), _area(crop, size), None, None, [_color((1.4, 1.0, 1.9), SRGBISH)], 1,
              view.data_ptr(), pitch, fstride, w, h, n, wbuf.data_ptr() + GUARD, need, obuf.data_ptr() + GUARD, nbytes,
              torch.cuda.current_stream().cuda_stream)
    assert rc == 0, M.load().mcraw_last_error().decode()
    torch.cuda.synchronize()
    a, wk = obuf.cpu().numpy(), wbuf.cpu().numpy()
    assert (a[:GUARD] == SENT).all() and (a[GUARD + nbytes:] == SENT).all()
    assert (wk[:GUARD] == SENT).all() and (wk[GUARD + need:] == SENT).all()
    got = a[GUARD:GUARD + nbytes].view(np.uint32).reshape((n, 3) + size)
    for i in range(n):
        assert np.array_equal(got[i], A.float_bits(o[i], "f32")), i
    assert torch.equal(base, before), "the input was written"


def test_per_frame_colours_across_launch_pieces(gpu_ctx):
    rng = np.random.default_rng(8)
    n = 33
    imgs = [_mosaic(rng, 8, 8, 12) for _ in range(n)]
    gains = rng.uniform(0.8, 2.4, size=(n, 3)).astype(np.float32)
    mats = (SRGBISH[None] * rng.uniform(0.6, 1.4, size=(n, 3, 3))).astype(np.float32)
    _check_families(gpu_ctx, _dev16(np.stack(imgs)), imgs, None, (2, 2), "grbg", (64, 64, 64, 64), gain=gains, matrix=mats)


@pytest.mark.parametrize("size", (256, 4096, 65536))
def test_lut_sizes_and_new_contents_between_queued_calls(gpu_ctx, size):
    rng = np.random.default_rng(size)
    n, h, w, crop, osz = 2, 40, 72, (2, 4, 36, 64), (8, 14)
    imgs = [_mosaic(rng, h, w, 12) for _ in range(n)]
    t = _dev16(np.stack(imgs))
    o = [A.values(A.area_estimates(imgs[i], crop, osz, (0, 0, 0, 0), "rggb"), 4095.0, gain=(1.5, 1.0, 1.3)) for i in range(n)]
    s = torch.cuda.Stream(DEV)
    dl = torch.empty(size, dtype=torch.int16, device=DEV)
    luts = [_rand_lut(rng, size) for _ in range(4)]
    staged = [torch.from_numpy(x.view(np.int16)).to(DEV) for x in luts]
    torch.cuda.synchronize()
    outs = []
    kw = dict(algo="area", size=osz, crop=crop, white=4095.0, gain=(1.5, 1.0, 1.3), transfer=dl.view(torch.uint16))
    with torch.cuda.stream(s):
        for k in range(4):  # no host sync between: the LUT is rewritten in stream order between the calls
            dl.copy_(staged[k])
            outs.append(gpu_ctx.demosaic_yuv(t, fmt="p010", in_bits=16, **kw) if k % 2 else gpu_ctx.demosaic_display(t, **kw))
    s.synchronize()
    coef = M.yuv_matrix("bt709", "limited", 10, 16)
    for k, out in enumerate(outs):
        got = _np(out)
        for i in range(n):
            want = Y.yuv_from_o(o[i], luts[k], "p010", coef, 16) if k % 2 else A.display_from_o(o[i], luts[k], "u8", "hwc")
            assert np.array_equal(got[i], want), (k, i)


def test_two_queued_calls_share_one_work_buffer(gpu_ctx):
    rng = np.random.default_rng(9)
    h, w = 48, 80
    imgs = [_mosaic(rng, h, w, 12) for _ in range(2)]
    t = _dev16(np.stack(imgs))
    geoms = (((0, 0, 48, 80), (5, 9)), ((2, 6, 40, 70), (20, 30)), ((0, 0, 48, 80), (24, 40)))
    need = max(_work_bytes(c, s) for c, s in geoms)
    work = torch.full((need,), SENT, dtype=torch.uint8, device=DEV)
    outs = [torch.full((2, 3) + s, -1.0, dtype=torch.float32, device=DEV) for _, s in geoms]
    st = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    for (crop, size), out in zip(geoms, outs):  # queued back to back on one stream, no host sync between
        rc = _raw(gpu_ctx, _aparams(), _area(crop, size), None, None, [_color()], 1, t.data_ptr(), w, h * w, w, h, 2, work.data_ptr(), need,
                  out.data_ptr(), out.numel() * 4, st.cuda_stream)
        assert rc == 0, M.load().mcraw_last_error().decode()
    st.synchronize()
    for (crop, size), out in zip(geoms, outs):
        for i in range(2):
            assert np.array_equal(_bits(out[i], torch.int32), A.area_ref(imgs[i], crop, size, "f32", 4095.0)), (crop, size, i)


def test_rejections_write_nothing(gpu_ctx):
    w, h, n = 16, 8, 2
    img = torch.full((n, h, w), 1000, dtype=torch.int16, device=DEV).view(torch.uint16)
    crop, size = (0, 0, 8, 16), (2, 4)
    nbytes = n * 3 * 2 * 4 * 4
    buf = torch.full((nbytes + 64,), SENT, dtype=torch.uint8, device=DEV)
    need = _work_bytes(crop, size)
    work = torch.full((need + 64,), SENT, dtype=torch.uint8, device=DEV)
    lutb = torch.zeros(4096 + 64, dtype=torch.int16, device=DEV)
    ip, op, wp, lp = img.data_ptr(), buf.data_ptr(), work.data_ptr(), lutb.data_ptr()
    ok = _color()

    def call(prm=_aparams(), area=_area(crop, size), d=None, y=None, cols=(ok,), ncol=1, in_ptr=ip, pitch=w, fstride=h * w, width=w,
             height=h, frames=n, work_ptr=wp, work_bytes=need, out_ptr=op, out_bytes=nbytes):
        return _raw(gpu_ctx, prm, area, d, y, cols, ncol, in_ptr, pitch, fstride, width, height, frames, work_ptr, work_bytes, out_ptr,
                    out_bytes)

    P0 = _aparams(dtype=0)
    bad_d, bad_y = _display(lp), _yuv(lp)
    bad_d.reserved, bad_y.reserved = 1, 1
    bits7 = _yuv(lp)
    bits7.in_bits = 7
    cases = [
        dict(prm=None), dict(area=None),                                                  # NULL p, NULL a
        dict(prm=_aparams(algo=1)), dict(prm=_aparams(algo=2)), dict(prm=_aparams(algo=0)), dict(prm=_aparams(algo=4)),  # a wrong algo
        dict(prm=P0, d=_display(lp), y=_yuv(lp)),                                              # both stages
        dict(area=_area((1, 0, 8, 16), size)), dict(area=_area((0, 1, 8, 16), size)),     # an odd crop
        dict(area=_area((0, 0, 7, 16), size)), dict(area=_area((0, 0, 8, 15), size)),
        dict(area=_area((0, 0, 0, 16), size)), dict(area=_area((0, 0, 8, 0), size)),      # an empty crop
        dict(area=_area((2, 0, 8, 16), size)), dict(area=_area((0, 2, 8, 16), size)),     # a crop that leaves the frame
        dict(area=_area((0, 0, 10, 16), size)), dict(area=_area((0, 0, 8, 18), size)),
        dict(area=_area(crop, (5, 4))), dict(area=_area(crop, (2, 9))),                   # more pixels than quads
        dict(area=_area(crop, (0, 4))), dict(area=_area(crop, (2, 0))),
        dict(area=_area((0, 0, 8, 16), (2, 4), reserved=(1, 0))), dict(area=_area((0, 0, 8, 16), (2, 4), reserved=(0, 7))),
        dict(work_ptr=0), dict(work_ptr=wp + 8), dict(work_bytes=need - 1), dict(work_bytes=0),
        # the family's own rules
        dict(d=_display(lp), prm=_aparams(dtype=2)), dict(prm=P0, d=_display(lp + 8)), dict(prm=P0, d=_display(lp, log2=7)),
        dict(prm=P0, d=bad_d), dict(prm=P0, y=bad_y), dict(prm=P0, y=bits7),
        dict(prm=P0, y=_yuv(lp), area=_area(crop, (1, 4))), dict(prm=P0, y=_yuv(lp), area=_area(crop, (2, 3))), dict(prm=P0),
        dict(prm=_aparams(dtype=7)), dict(prm=_aparams(flags=2)), dict(prm=_aparams(white=float("inf"))),
        dict(out_bytes=nbytes - 1), dict(out_ptr=op + 2), dict(out_ptr=0), dict(in_ptr=ip + 1), dict(in_ptr=0),
        dict(width=15), dict(height=2), dict(pitch=w - 2), dict(fstride=h * w - w), dict(ncol=3, cols=(ok, ok, ok)),
        dict(cols=(_color(gain=(float("nan"), 1, 1)),)), dict(frames=-1),
    ]
    bad_cfa = _aparams()
    bad_cfa.cfa = 4
    cases.append(dict(prm=bad_cfa))
    # over the ratio limit: 68 quads onto 4 pixels
    wide = torch.zeros((1, 8, 136), dtype=torch.int16, device=DEV)
    cases.append(dict(in_ptr=wide.data_ptr(), pitch=136, fstride=8 * 136, width=136, frames=1, area=_area((0, 0, 8, 136), (2, 4))))
    serial = gpu_ctx.last_serial()
    for i, c in enumerate(cases):
        assert call(**c) < 0, (i, sorted(c))
        assert M.load().mcraw_last_error().decode().startswith(SYM + ": "), (i, M.load().mcraw_last_error().decode())
    # algo 3 stays unknown to the three other entry points
    from _demosaic_gpu import raw_call
    p3 = _aparams()
    std = ([ok], 1, ip, w, h * w, w, h, n, op, nbytes)
    assert raw_call(gpu_ctx, "mcraw_demosaic_batch", p3, None, *std, staged=False) < 0
    assert M.load().mcraw_last_error().decode() == "mcraw_demosaic_batch: unknown algo"
    assert raw_call(gpu_ctx, "mcraw_demosaic_display_batch", p3, _display(lp), *std) < 0
    assert M.load().mcraw_last_error().decode() == "mcraw_demosaic_display_batch: unknown algo"
    assert raw_call(gpu_ctx, "mcraw_demosaic_yuv_batch", p3, _yuv(lp), *std) < 0
    assert M.load().mcraw_last_error().decode() == "mcraw_demosaic_yuv_batch: unknown algo"
    assert call(frames=0) == 0  # n == 0: a no-op
    torch.cuda.synchronize()
    gpu_ctx.synchronize()
    assert (buf.cpu().numpy() == SENT).all() and (work.cpu().numpy() == SENT).all()
    assert gpu_ctx.last_serial() == serial and gpu_ctx.errors() == 0
    # a good call next to them does write: a flat frame comes out flat
    assert call() == 0
    torch.cuda.synchronize()
    a = buf.cpu().numpy()
    assert (a[nbytes:] == SENT).all() and (work.cpu().numpy()[need:] == SENT).all()
    assert (a[:nbytes].view(np.float32) == np.float32(1000.0) * (np.float32(1.0) / np.float32(4095.0))).all()
    # ... and so do the other two families with their own structs
    assert call(prm=P0, d=_display(lp), out_bytes=nbytes // 4) == 0 and call(prm=P0, y=_yuv(lp), out_bytes=nbytes // 8) == 0
    torch.cuda.synchronize()


def test_python_argument_rules(gpu_ctx):
    t = torch.zeros((8, 16), dtype=torch.int16, device=DEV).view(torch.uint16)
    for kw in (dict(algo="bin2", size=(2, 4)), dict(algo="mhc", crop=(0, 0, 8, 16)), dict(algo="area"), dict(algo="area", size=(2, 4, 1)),
               dict(algo="area", size=(2, 4), crop=(0, 0, 8)), dict(algo="area", size=(2, 4), crop=(1, 0, 6, 16)),
               dict(algo="area", size=(5, 4)), dict(algo="nearest", size=(2, 4))):
        with pytest.raises(ValueError):
            gpu_ctx.demosaic(t, dtype="f32", white=4095.0, **kw)
    with pytest.raises(ValueError):
        gpu_ctx.demosaic_display(t, white=4095.0, size=(2, 4))
    with pytest.raises(ValueError):
        gpu_ctx.demosaic_yuv(t, white=4095.0, algo="area")
    with pytest.raises(M.McrawError, match=SYM):  # a crop that leaves the frame is the library's to reject
        gpu_ctx.demosaic(t, dtype="f32", white=4095.0, algo="area", size=(2, 4), crop=(2, 0, 8, 16))
    with pytest.raises(M.McrawError, match=SYM):  # 4:2:0 needs an even size
        gpu_ctx.demosaic_yuv(t, white=4095.0, algo="area", size=(2, 3))
    out = gpu_ctx.demosaic(t, dtype="f32", white=4095.0, algo="area", size=(2, 4))  # an (H, W) mosaic drops N
    assert tuple(out.shape) == (3, 2, 4)
    empty = gpu_ctx.demosaic(t[None][:0], dtype="f16", white=4095.0, algo="area", size=(2, 4))
    assert tuple(empty.shape) == (0, 3, 2, 4)


@pytest.mark.parametrize("typ", (7, 6))
def test_decode_yuv_equals_demosaic_yuv_of_plain_decode(gpu_ctx, typ):
    rng = np.random.default_rng(typ)
    w, h = 256, 64
    items = _frames(rng, [(w, h)] * 2, typ)
    ins = [torch.from_numpy(b).to(DEV) for b, _ in items]
    mos = _dev16(np.stack([want for _, want in items]))
    crop, size = M.fit_crop(h, w, 12, 40), (12, 40)
    kw = dict(algo="area", size=size, crop=crop, white=4095.0, black=(64, 64, 64, 64), cfa="grbg", gain=(1.9, 1.0, 1.4), matrix=SRGBISH,
              fmt="nv12", standard="bt601")
    serial = gpu_ctx.last_serial()
    ref = gpu_ctx.demosaic_yuv(mos, **kw)
    torch.cuda.synchronize()
    assert gpu_ctx.last_serial() == serial  # the area call takes no decode serial
    out = gpu_ctx.decode_yuv(ins, w, h, typ, **kw)
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    lut = M.transfer_lut("bt709", 4096, 12)
    coef = M.yuv_matrix("bt601", "limited", 8, 12)
    for i, (_, want) in enumerate(items):
        assert np.array_equal(_np(out[i]), A.area_yuv_ref(want, crop, size, 4095.0, lut, "nv12", coef, 12, (64, 64, 64, 64), "grbg",
                                                          (1.9, 1.0, 1.4), SRGBISH))
    f = gpu_ctx.decode_rgb(ins, w, h, typ, dtype="f16", **{k: v for k, v in kw.items() if k not in ("fmt", "standard")})
    d = gpu_ctx.decode_display(ins, w, h, typ, **{k: v for k, v in kw.items() if k not in ("fmt", "standard")})
    assert tuple(f.shape) == (2, 3) + size and tuple(d.shape) == (2,) + size + (3,)
    assert torch.equal(d, gpu_ctx.demosaic_display(mos, **{k: v for k, v in kw.items() if k not in ("fmt", "standard")}))
    assert gpu_ctx.errors() == 0


def test_stages_in_front_equal_the_stages_run_by_hand(gpu_ctx):
    rng = np.random.default_rng(12)
    n, h, w = 2, 48, 96
    imgs = np.clip(rng.normal(800.0, 40.0, size=(n, h, w)), 0, 4095).astype(np.uint16)
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
    kw = dict(algo="area", size=(10, 18), crop=(2, 4, 44, 88), white=4095.0, black=black, cfa=cfa, gain=(1.7, 1.0, 1.4), matrix=SRGBISH)
    a = gpu_ctx.demosaic(t, dtype="f32", defects=defects, denoise=denoise, shading=gm, **kw)
    assert torch.equal(a.view(torch.int32), gpu_ctx.demosaic(three, dtype="f32", **kw).view(torch.int32))
    assert not torch.equal(a.view(torch.int32), gpu_ctx.demosaic(t, dtype="f32", **kw).view(torch.int32))
    b = gpu_ctx.demosaic_yuv(t, defects=defects, denoise=denoise, shading=gm, **kw)
    assert torch.equal(b, gpu_ctx.demosaic_yuv(three, **kw))
    got = _bits(a, torch.int32)
    three_np = _np(three)
    for i in range(n):
        assert np.array_equal(got[i], A.area_ref(three_np[i], kw["crop"], kw["size"], "f32", 4095.0, black, cfa, kw["gain"], SRGBISH))


def test_siblings_unchanged_by_interleaved_area_calls(gpu_ctx):
    rng = np.random.default_rng(21)
    n, h, w = 2, 40, 264
    imgs = [_mosaic(rng, h, w, 12) for _ in range(n)]
    t = _dev16(np.stack(imgs))
    kw = dict(white=4095.0, black=(60, 61, 62, 63), cfa="grbg", gain=(1.7, 1.0, 1.4), matrix=SRGBISH)
    ar = dict(algo="area", size=(8, 60), crop=(2, 4, 36, 256))
    lut8 = M.transfer_lut("srgb", 4096, 8)
    for algo in ("mhc", "bin2"):
        d0 = gpu_ctx.demosaic_display(t, algo=algo, **kw)
        a0 = gpu_ctx.demosaic_display(t, **ar, **kw)
        f0 = gpu_ctx.demosaic(t, algo=algo, dtype="f16", **kw)
        a1 = gpu_ctx.demosaic(t, dtype="f16", **ar, **kw)
        y0 = gpu_ctx.demosaic_yuv(t, algo=algo, **kw)
        a2 = gpu_ctx.demosaic_yuv(t, **ar, **kw)
        d1 = gpu_ctx.demosaic_display(t, algo=algo, **kw)
        f1 = gpu_ctx.demosaic(t, algo=algo, dtype="f16", **kw)
        y1 = gpu_ctx.demosaic_yuv(t, algo=algo, **kw)
        torch.cuda.synchronize()
        assert torch.equal(d0, d1) and torch.equal(f0.view(torch.int16), f1.view(torch.int16)) and torch.equal(y0, y1)
        coef = M.yuv_matrix("bt709", "limited", 8, 12)
        for i in range(n):
            assert np.array_equal(_np(d1[i]), D.display_ref(imgs[i], algo, 4095.0, lut8, "u8", "hwc", kw["black"], "grbg", kw["gain"], SRGBISH))
            assert np.array_equal(_bits(f1[i], torch.int16), R.ref_bits(imgs[i], algo, "f16", 4095.0, black=kw["black"], cfa="grbg",
                                                                         gain=kw["gain"], matrix=SRGBISH))
            assert np.array_equal(_np(y1[i]), Y.yuv_ref(imgs[i], algo, 4095.0, M.transfer_lut("bt709", 4096, 12), "nv12", coef, 12,
                                                        kw["black"], "grbg", kw["gain"], SRGBISH))
            assert np.array_equal(_np(a0[i]), A.area_display_ref(imgs[i], ar["crop"], ar["size"], 4095.0, lut8, "u8", "hwc", kw["black"],
                                                                 "grbg", kw["gain"], SRGBISH))
            assert np.array_equal(_bits(a1[i], torch.int16), A.area_ref(imgs[i], ar["crop"], ar["size"], "f16", 4095.0, kw["black"], "grbg",
                                                                        kw["gain"], SRGBISH))
            assert np.array_equal(_np(a2[i]), A.area_yuv_ref(imgs[i], ar["crop"], ar["size"], 4095.0, M.transfer_lut("bt709", 4096, 12),
                                                             "nv12", coef, 12, kw["black"], "grbg", kw["gain"], SRGBISH))


def test_grey_input_is_neutral_at_a_fractional_ratio(gpu_ctx):
    for fmt, c_off in (("nv12", 128), ("p010", 512 << 6)):
        grey = torch.full((50, 84), 2000, dtype=torch.int16, device=DEV).view(torch.uint16)
        out = gpu_ctx.demosaic_yuv(grey, algo="area", size=(10, 18), crop=(2, 2, 46, 80), white=4095.0, fmt=fmt)
        yp, cp = M.yuv_planes(out, 10)
        torch.cuda.synchronize()
        assert (_np(cp) == c_off).all() and len(np.unique(_np(yp))) == 1
