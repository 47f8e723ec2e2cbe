"""The resampling demosaic (mcraw_demosaic_resample_batch; algo="resample" of Context.demosaic / demosaic_display / demosaic_yuv
and the decode_* methods) on the GPU: every output sample equals the numpy statement of the contract (_resample_ref) bit for bit,
at the crop's own size it is algo "mhc" cut to the crop, nothing outside `out` and `work` is written, rejected calls write nothing,
queued calls share neither LUT contents nor scratch, and the sibling entry points are undisturbed."""
import ctypes as C

import numpy as np
import pytest
import torch

import _area_ref as A
import _display_ref as D
import _resample_ref as S
import _rgb_ref as R
import _yuv_ref as Y
import motioncam_decoder_amd as M
from _demosaic_gpu import CFAS, DEV, GUARD, SENT, SRGBISH
from _demosaic_gpu import dev16 as _dev16, frames as _frames, mosaic as _mosaic, rand_lut as _rand_lut, rgb_color as _color
from _demosaic_gpu import rgb_params as _params, to_np as _np
from _demosaic_gpu import FLOATS, IN_BITS, TD, as_int as _as_int, bits as _bits, colours as _colours, display as _display, yuv as _yuv
from _demosaic_gpu import raw_scaled_call, work_bytes

pytestmark = pytest.mark.gpu

SYM = "mcraw_demosaic_resample_batch"


def _rparams(white=4095.0, black=(0, 0, 0, 0), cfa="rggb", dtype=1, flags=0, algo=4):
    """mcraw_rgb for the resample call: dtype 1 = MCRAW_FLOAT_F32 (the display and YUV families take 0)."""
    p = _params("mhc", white, black, cfa, dtype, flags)
    p.algo = algo
    return p


def _res(crop, size, filt=1, reserved=0):
    r = M.Resample()
    r.y0, r.x0, r.ch, r.cw = crop
    r.out_h, r.out_w = size
    r.filter, r.reserved = filt, reserved
    return r


def _raw(ctx, *args, **kw):
    """The C entry point as it is: prm, res, d and y may be None (NULL pointers)."""
    return raw_scaled_call(SYM, ctx, *args, **kw)


def _work_bytes(crop, size):
    return work_bytes("mcraw_resample_work_bytes", _res(crop, size))


def _check_families(ctx, t, imgs, crop, size, cfa="rggb", black=(0, 0, 0, 0), white=4095.0, gain=(1.8, 1.0, 1.3), matrix=SRGBISH,
                    lut=None, filt="cubic", floats=("f32", "f16", "bf16"), display=(("u8", "hwc"), ("u16", "chw")), yuv=None, tag=None):
    """The families and kinds of the Python methods on the (n, h, w) tensor t of the frames imgs against the numpy statement."""
    n = len(imgs)
    h, w = imgs[0].shape
    ccrop = (0, 0, h, w) if crop is None else crop
    ho, wo = size
    yuv = ((ho % 2 == 0 and wo % 2 == 0) and ("nv12", "p010")) if yuv is None else yuv
    o = [S.values(S.resample_estimates(imgs[i], ccrop, size, filt, black, cfa), white, black, *_colours(gain, matrix, i)) for i in range(n)]
    kw = dict(algo="resample", size=size, crop=crop, filter=filt, white=white, black=black, cfa=cfa, gain=gain, matrix=matrix)
    for dt, view in FLOATS:
        if dt not in floats:
            continue
        clip = dt == "f16"
        out = ctx.demosaic(t, dtype=dt, clip=clip, **kw)
        torch.cuda.synchronize()
        assert tuple(out.shape) == (n, 3, ho, wo)
        got = _bits(out, view)
        for i in range(n):
            want = S.float_bits(np.clip(o[i], np.float32(0), np.float32(1)) if clip else o[i], dt)
            assert np.array_equal(got[i], want), (tag, dt, i)
    lut = _rand_lut(np.random.default_rng(ho * 131 + wo), 4096) if lut is None else lut
    dl = _dev16(lut)
    for dt, layout in display:
        out = ctx.demosaic_display(t, dtype=TD[dt], layout=layout, transfer=dl, **kw)
        torch.cuda.synchronize()
        got = _np(out)
        assert got.shape == ((n, ho, wo, 3) if layout == "hwc" else (n, 3, ho, wo))
        for i in range(n):
            assert np.array_equal(got[i], S.display_from_o(o[i], lut, dt, layout)), (tag, dt, layout, i)
    for fmt in yuv or ():
        out = ctx.demosaic_yuv(t, fmt=fmt, transfer=dl, in_bits=IN_BITS, **kw)
        torch.cuda.synchronize()
        got = _np(out)
        assert got.shape == (n, ho * 3 // 2, wo) and out.dtype == TD[fmt]
        coef = M.yuv_matrix("bt709", "limited", Y.BITS[fmt], IN_BITS)
        for i in range(n):
            assert np.array_equal(got[i], S.yuv_from_o(o[i], lut, fmt, coef, IN_BITS)), (tag, fmt, i)


@pytest.mark.parametrize("cfa", CFAS)
def test_crop_size_equals_mhc_cut_to_the_crop(gpu_ctx, cfa):
    rng = np.random.default_rng(R.CFA_CODE[cfa])
    imgs = [_mosaic(rng, 24, 40, 12) for _ in range(2)]
    t = _dev16(np.stack(imgs))
    kw = dict(white=4095.0, black=(60, 61, 62, 63), cfa=cfa, gain=(1.8, 1.0, 1.3), matrix=SRGBISH)
    dl = _dev16(_rand_lut(rng, 4096))
    for crop in ((2, 4, 16, 24), (0, 0, 24, 40)):
        y0, x0, h, w = crop
        ar = dict(algo="resample", size=(h, w), crop=crop)
        for filt in ("cubic", "linear"):
            for dt, view in FLOATS:
                a, b = gpu_ctx.demosaic(t, dtype=dt, filter=filt, **ar, **kw), gpu_ctx.demosaic(t, algo="mhc", dtype=dt, **kw)
                assert torch.equal(a.view(view), b[:, :, y0:y0 + h, x0:x0 + w].contiguous().view(view)), (crop, filt, dt)
        for dt in (torch.uint8, torch.uint16):
            for layout in ("hwc", "chw"):
                a = gpu_ctx.demosaic_display(t, dtype=dt, layout=layout, transfer=dl, **ar, **kw)
                b = gpu_ctx.demosaic_display(t, algo="mhc", dtype=dt, layout=layout, transfer=dl, **kw)
                b = b[:, y0:y0 + h, x0:x0 + w] if layout == "hwc" else b[:, :, y0:y0 + h, x0:x0 + w]
                assert torch.equal(_as_int(a), _as_int(b.contiguous())), (crop, dt, layout)
        for fmt in ("nv12", "p010"):
            a = gpu_ctx.demosaic_yuv(t, fmt=fmt, transfer=dl, in_bits=IN_BITS, **ar, **kw)
            b = gpu_ctx.demosaic_yuv(t, algo="mhc", fmt=fmt, transfer=dl, in_bits=IN_BITS, **kw)
            ya, ca = M.yuv_planes(a, h)
            yb, cb = M.yuv_planes(b, 24)
            assert torch.equal(_as_int(ya), _as_int(yb[:, y0:y0 + h, x0:x0 + w].contiguous())), (crop, fmt)
            assert torch.equal(_as_int(ca), _as_int(cb[:, y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2].contiguous())), (crop, fmt)
        _check_families(gpu_ctx, t, imgs, crop, (h, w), cfa, kw["black"], tag=(cfa, crop))


@pytest.mark.parametrize("filt", ("cubic", "linear"))
def test_exact_and_fractional_ratios_both_ways(gpu_ctx, filt):
    rng = np.random.default_rng(3)
    black = (64, 67, 61, 70)
    big = [_mosaic(rng, 44, 88, 12) for _ in range(2)]
    small = [_mosaic(rng, 20, 36, 12) for _ in range(2)]
    tb, ts = _dev16(np.stack(big)), _dev16(np.stack(small))
    one = dict(floats=("f16",), display=(("u8", "hwc"),), yuv=("nv12",))
    _check_families(gpu_ctx, tb, big, None, (22, 44), "grbg", black, filt=filt, tag="2:1", **one)
    _check_families(gpu_ctx, ts, small, None, (40, 72), "bggr", black, filt=filt, tag="1:2", **one)
    _check_families(gpu_ctx, tb, big, None, (30, 58), "gbrg", black, filt=filt, tag="down")
    _check_families(gpu_ctx, ts, small, None, (31, 47), "rggb", black, filt=filt, yuv=False, tag="up")
    _check_families(gpu_ctx, ts, small, None, (32, 46), "rggb", black, filt=filt, floats=(), display=(), tag="up, 4:2:0")


@pytest.mark.parametrize("shape", ((8, 8), (28, 36)))
def test_a_crop_in_each_corner_reflects_at_every_edge(gpu_ctx, shape):
    rng = np.random.default_rng(shape[0])
    h, w = shape
    imgs = [_mosaic(rng, h, w, 12) for _ in range(2)]
    t = _dev16(np.stack(imgs))
    ch, cw = (6, 6) if h == 8 else (12, 16)
    one = dict(floats=("f32",), display=(("u16", "hwc"),))  # (and both YUV formats wherever the size is even)
    for y0 in (0, h - ch):
        for x0 in (0, w - cw):
            _check_families(gpu_ctx, t, imgs, (y0, x0, ch, cw), (ch // 2, cw // 2 + 2), "grbg", (64, 64, 64, 64), tag=("down", y0, x0), **one)
            _check_families(gpu_ctx, t, imgs, (y0, x0, ch, cw), (ch + 4, cw * 2 - 2), "gbrg", (64, 64, 64, 64), tag=("up", y0, x0), **one)
    _check_families(gpu_ctx, t, imgs, None, (h // 2, w // 2), "bggr", tag="whole, 2:1", **one)


def test_taps_outside_an_interior_crop_read_the_frame(gpu_ctx):
    rng = np.random.default_rng(5)
    imgs = [_mosaic(rng, 40, 56, 12)]
    t = _dev16(np.stack(imgs))
    crop, size = (10, 12, 20, 28), (14, 20)
    kw = dict(algo="resample", size=size, white=4095.0, dtype="f32")
    _check_families(gpu_ctx, t, imgs, crop, size, "rggb", floats=("f32",), display=(), yuv=())
    inside = gpu_ctx.demosaic(t, crop=crop, **kw)
    alone = gpu_ctx.demosaic(t[:, 10:30, 12:40].contiguous(), **kw)  # the same crop as its own frame: reflected, not read
    assert not torch.equal(inside.view(torch.int32), alone.view(torch.int32))


@pytest.mark.parametrize("wo", (1, 7, 9, 10, 15))
def test_last_lane_holds_a_part_of_its_columns(gpu_ctx, wo):
    rng = np.random.default_rng(wo)
    cw = 2 * ((3 * wo + 1) // 4 + 1) if wo > 1 else 2  # about 1.5 samples per pixel
    imgs = [_mosaic(rng, 12, cw + 6, 12) for _ in range(2)]
    _check_families(gpu_ctx, _dev16(np.stack(imgs)), imgs, (2, 4, 8, cw), (6, wo), "grbg", (10, 20, 30, 40), tag=wo,
                    floats=("f32", "bf16"), yuv=("nv12",) if wo % 2 == 0 else ())


def test_more_than_one_tile_both_ways(gpu_ctx):
    rng = np.random.default_rng(6)
    imgs = [_mosaic(rng, 76, 200, 12)]  # 150 columns: three column tiles; 70 rows: more than one band of row pairs
    one = dict(floats=("f16",), display=(("u8", "chw"),), yuv=("nv12",))
    _check_families(gpu_ctx, _dev16(np.stack(imgs)), imgs, (2, 2, 72, 196), (70, 150), "rggb", (64, 64, 64, 64), **one)


def test_ratio_limits(gpu_ctx):
    rng = np.random.default_rng(7)
    imgs = [_mosaic(rng, 26, 38, 14)]
    t = _dev16(np.stack(imgs))
    crop = (2, 4, 22, 30)
    one = dict(floats=("f32",), display=(("u8", "hwc"),))
    for size in ((44, 60), (11, 15), (44, 15), (11, 60)):  # 2 crop and ceil(crop / 2), on both axes and mixed
        for filt in ("cubic", "linear"):
            _check_families(gpu_ctx, t, imgs, crop, size, "bggr", (256, 257, 258, 259), 16383.0, filt=filt, tag=(size, filt), **one)


def test_strided_input_misaligned_out_sentinels(gpu_ctx):
    rng = np.random.default_rng(8)
    n, h, w, pitch = 3, 36, 68, 83
    fstride = h * pitch + 29
    crop, size = (4, 2, 30, 62), (27, 45)
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
    kw = dict(algo="resample", size=size, crop=crop, white=16383.0, black=black, cfa="bggr", gain=(1.4, 1.0, 1.9), matrix=SRGBISH)
    o = [S.values(S.resample_estimates(imgs[i], crop, size, "cubic", black, "bggr"), 16383.0, black, (1.4, 1.0, 1.9), SRGBISH) for i in range(n)]
    # the 16-byte path beside it: the same frames on the grid
    packed = gpu_ctx.demosaic(_dev16(np.stack(imgs)), dtype="f16", **kw)
    cases = [("f16", torch.float16, (n, 3) + size, lambda out: gpu_ctx.demosaic(view, dtype="f16", out=out, **kw),
              lambda i: S.float_bits(o[i], "f16")),
             ("u8", torch.uint8, (n,) + size + (3,), lambda out: gpu_ctx.demosaic_display(view, transfer=dl, out=out, **kw),
              lambda i: S.display_from_o(o[i], lut, "u8", "hwc")),
             ("u16", torch.uint16, (n, 3) + size, lambda out: gpu_ctx.demosaic_display(view, transfer=dl, dtype=torch.uint16, layout="chw",
                                                                                      out=out, **kw),
              lambda i: S.display_from_o(o[i], lut, "u16", "chw"))]
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
    for i in range(n):
        assert np.array_equal(_bits(packed[i], torch.int16), S.float_bits(o[i], "f16")), i
    # the C entry point with sentinels round `work` as well (its strides in elements, as the Python layer passes them)
    need = _work_bytes(crop, size)
    wbuf = torch.full((GUARD + need + GUARD,), SENT, dtype=torch.uint8, device=DEV)
    nbytes = n * 3 * size[0] * size[1] * 4
    obuf = torch.full((GUARD + nbytes + GUARD,), SENT, dtype=torch.uint8, device=DEV)
    rc = _raw(gpu_ctx, _rparams(16383.0, black, "bggr"), _res(crop, size), None, None, [_color((1.4, 1.0, 1.9), SRGBISH)], 1,
              view.data_ptr(), pitch, fstride, w, h, n, wbuf.data_ptr() + GUARD, need, obuf.data_ptr() + GUARD, nbytes,
              torch.cuda.current_stream().cuda_stream)
    assert rc == 0, M.load().mcraw_last_error().decode()
    torch.cuda.synchronize()
    a, wk = obuf.cpu().numpy(), wbuf.cpu().numpy()
    assert (a[:GUARD] == SENT).all() and (a[GUARD + nbytes:] == SENT).all()
    assert (wk[:GUARD] == SENT).all() and (wk[GUARD + need:] == SENT).all()
    got = a[GUARD:GUARD + nbytes].view(np.uint32).reshape((n, 3) + size)
    for i in range(n):
        assert np.array_equal(got[i], S.float_bits(o[i], "f32")), i
    assert torch.equal(base, before), "the input was written"


def test_per_frame_colours_across_launch_pieces(gpu_ctx):
    rng = np.random.default_rng(9)
    n = 33
    imgs = [_mosaic(rng, 8, 8, 12) for _ in range(n)]
    gains = rng.uniform(0.8, 2.4, size=(n, 3)).astype(np.float32)
    mats = (SRGBISH[None] * rng.uniform(0.6, 1.4, size=(n, 3, 3))).astype(np.float32)
    _check_families(gpu_ctx, _dev16(np.stack(imgs)), imgs, None, (6, 10), "grbg", (64, 64, 64, 64), gain=gains, matrix=mats,
                    floats=("f32",), display=(("u8", "hwc"),), yuv=("nv12",))


@pytest.mark.parametrize("size", (256, 4096, 65536))
def test_lut_sizes_and_new_contents_between_queued_calls(gpu_ctx, size):
    rng = np.random.default_rng(size)
    n, h, w, crop, osz = 2, 40, 72, (2, 4, 36, 64), (26, 50)
    imgs = [_mosaic(rng, h, w, 12) for _ in range(n)]
    t = _dev16(np.stack(imgs))
    o = [S.values(S.resample_estimates(imgs[i], crop, osz), 4095.0, gain=(1.5, 1.0, 1.3)) for i in range(n)]
    s = torch.cuda.Stream(DEV)
    dl = torch.empty(size, dtype=torch.int16, device=DEV)
    luts = [_rand_lut(rng, size) for _ in range(4)]
    staged = [torch.from_numpy(x.view(np.int16)).to(DEV) for x in luts]
    torch.cuda.synchronize()
    outs = []
    kw = dict(algo="resample", size=osz, crop=crop, white=4095.0, gain=(1.5, 1.0, 1.3), transfer=dl.view(torch.uint16))
    with torch.cuda.stream(s):
        for k in range(4):  # no host sync between: the LUT is rewritten in stream order between the calls
            dl.copy_(staged[k])
            outs.append(gpu_ctx.demosaic_yuv(t, fmt="p010", in_bits=16, **kw) if k % 2 else gpu_ctx.demosaic_display(t, **kw))
    s.synchronize()
    coef = M.yuv_matrix("bt709", "limited", 10, 16)
    for k, out in enumerate(outs):
        got = _np(out)
        for i in range(n):
            want = Y.yuv_from_o(o[i], luts[k], "p010", coef, 16) if k % 2 else S.display_from_o(o[i], luts[k], "u8", "hwc")
            assert np.array_equal(got[i], want), (k, i)


def test_two_queued_calls_share_one_work_buffer(gpu_ctx):
    rng = np.random.default_rng(10)
    h, w = 48, 80
    imgs = [_mosaic(rng, h, w, 12) for _ in range(2)]
    t = _dev16(np.stack(imgs))
    geoms = (((0, 0, 48, 80), (25, 41)), ((2, 6, 40, 70), (60, 100)), ((0, 0, 48, 80), (48, 80)))
    need = max(_work_bytes(c, s) for c, s in geoms)
    work = torch.full((need,), SENT, dtype=torch.uint8, device=DEV)
    outs = [torch.full((2, 3) + s, -1.0, dtype=torch.float32, device=DEV) for _, s in geoms]
    st = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    for (crop, size), out in zip(geoms, outs):  # queued back to back on one stream, no host sync between
        rc = _raw(gpu_ctx, _rparams(), _res(crop, size), None, None, [_color()], 1, t.data_ptr(), w, h * w, w, h, 2, work.data_ptr(), need,
                  out.data_ptr(), out.numel() * 4, st.cuda_stream)
        assert rc == 0, M.load().mcraw_last_error().decode()
    st.synchronize()
    for (crop, size), out in zip(geoms, outs):
        for i in range(2):
            assert np.array_equal(_bits(out[i], torch.int32), S.resample_ref(imgs[i], crop, size, "f32", 4095.0)), (crop, size, i)


def test_rejections_write_nothing(gpu_ctx):
    w, h, n = 16, 8, 2
    img = torch.full((n, h, w), 1000, dtype=torch.int16, device=DEV).view(torch.uint16)
    crop, size = (0, 0, 8, 16), (6, 10)
    nbytes = n * 3 * 6 * 10 * 4
    buf = torch.full((nbytes + 64,), SENT, dtype=torch.uint8, device=DEV)
    need = _work_bytes(crop, size)
    work = torch.full((need + 64,), SENT, dtype=torch.uint8, device=DEV)
    lutb = torch.zeros(4096 + 64, dtype=torch.int16, device=DEV)
    ip, op, wp, lp = img.data_ptr(), buf.data_ptr(), work.data_ptr(), lutb.data_ptr()
    ok = _color()

    def call(prm=_rparams(), res=_res(crop, size), d=None, y=None, cols=(ok,), ncol=1, in_ptr=ip, pitch=w, fstride=h * w, width=w,
             height=h, frames=n, work_ptr=wp, work_bytes=need, out_ptr=op, out_bytes=nbytes):
        return _raw(gpu_ctx, prm, res, d, y, cols, ncol, in_ptr, pitch, fstride, width, height, frames, work_ptr, work_bytes, out_ptr,
                    out_bytes)

    P0 = _rparams(dtype=0)
    bad_d, bad_y = _display(lp), _yuv(lp)
    bad_d.reserved, bad_y.reserved = 1, 1
    bits7 = _yuv(lp)
    bits7.in_bits = 7
    cases = [
        dict(prm=None), dict(res=None),                                                   # NULL p, NULL r
        dict(prm=_rparams(algo=1)), dict(prm=_rparams(algo=2)), dict(prm=_rparams(algo=0)), dict(prm=_rparams(algo=3)),
        dict(prm=_rparams(algo=5)),                                                       # a wrong algo
        dict(prm=P0, d=_display(lp), y=_yuv(lp)),                                         # both stages
        dict(res=_res((1, 0, 6, 16), size)), dict(res=_res((0, 1, 8, 14), size)),         # an odd crop
        dict(res=_res((0, 0, 7, 16), size)), dict(res=_res((0, 0, 8, 15), size)),
        dict(res=_res((0, 0, 0, 16), size)), dict(res=_res((0, 0, 8, 0), size)),          # an empty crop
        dict(res=_res((2, 0, 8, 16), size)), dict(res=_res((0, 2, 8, 16), size)),         # a crop that leaves the frame
        dict(res=_res(crop, (3, 10))), dict(res=_res(crop, (6, 7))),                      # under half the crop
        dict(res=_res(crop, (17, 10))), dict(res=_res(crop, (6, 33))),                    # over twice the crop
        dict(res=_res(crop, (0, 10))), dict(res=_res(crop, (6, 0))),
        dict(res=_res(crop, size, filt=2)), dict(res=_res(crop, size, reserved=1)),
        dict(work_ptr=0), dict(work_ptr=wp + 8), dict(work_bytes=need - 1), dict(work_bytes=0),
        # the family's own rules
        dict(d=_display(lp), prm=_rparams(dtype=2)), dict(prm=P0, d=_display(lp + 8)), dict(prm=P0, d=_display(lp, log2=7)),
        dict(prm=P0, d=bad_d), dict(prm=P0, y=bad_y), dict(prm=P0, y=bits7),
        dict(prm=P0, y=_yuv(lp), res=_res(crop, (5, 10))), dict(prm=P0, y=_yuv(lp), res=_res(crop, (6, 9))), dict(prm=P0),
        dict(prm=_rparams(dtype=7)), dict(prm=_rparams(flags=2)), dict(prm=_rparams(white=float("inf"))),
        dict(out_bytes=nbytes - 1), dict(out_ptr=op + 2), dict(out_ptr=0), dict(in_ptr=ip + 1), dict(in_ptr=0),
        dict(width=15), dict(height=6, res=_res((0, 0, 6, 16), size)), dict(pitch=w - 2), dict(fstride=h * w - w),
        dict(ncol=3, cols=(ok, ok, ok)), dict(cols=(_color(gain=(float("nan"), 1, 1)),)), dict(frames=-1),
    ]
    bad_cfa = _rparams()
    bad_cfa.cfa = 4
    cases.append(dict(prm=bad_cfa))
    serial = gpu_ctx.last_serial()
    for i, c in enumerate(cases):
        assert call(**c) < 0, (i, sorted(c))
        assert M.load().mcraw_last_error().decode().startswith(SYM + ": "), (i, M.load().mcraw_last_error().decode())
    # algo 4 stays unknown to the other entry points
    from _demosaic_gpu import raw_call
    p4 = _rparams()
    std = ([ok], 1, ip, w, h * w, w, h, n, op, nbytes)
    assert raw_call(gpu_ctx, "mcraw_demosaic_batch", p4, None, *std, staged=False) < 0
    assert M.load().mcraw_last_error().decode() == "mcraw_demosaic_batch: unknown algo"
    assert raw_call(gpu_ctx, "mcraw_demosaic_display_batch", p4, _display(lp), *std) < 0
    assert M.load().mcraw_last_error().decode() == "mcraw_demosaic_display_batch: unknown algo"
    assert raw_call(gpu_ctx, "mcraw_demosaic_yuv_batch", p4, _yuv(lp), *std) < 0
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
    assert (a[:nbytes].view(np.float32) == np.float32(16000.0) * (np.float32(1.0) / np.float32(4095.0) * np.float32(0.0625))).all()
    # ... and so do the other two families with their own structs
    assert call(prm=P0, d=_display(lp), out_bytes=nbytes // 4) == 0 and call(prm=P0, y=_yuv(lp), out_bytes=nbytes // 8) == 0
    torch.cuda.synchronize()


def test_python_argument_rules(gpu_ctx):
    t = torch.zeros((8, 16), dtype=torch.int16, device=DEV).view(torch.uint16)
    for kw in (dict(algo="mhc", filter="cubic"), dict(algo="bin2", filter="linear"), dict(algo="area", size=(2, 4), filter="cubic"),
               dict(algo="resample"), dict(algo="resample", filter="linear"), dict(algo="resample", size=(6, 10), filter="lanczos"),
               dict(algo="resample", size=(6, 10, 1)), dict(algo="resample", size=(6, 10), crop=(0, 0, 8)),
               dict(algo="resample", size=(6, 10), crop=(1, 0, 6, 16)), dict(algo="resample", size=(3, 10)),
               dict(algo="resample", size=(6, 33))):
        with pytest.raises(ValueError):
            gpu_ctx.demosaic(t, dtype="f32", white=4095.0, **kw)
    with pytest.raises(ValueError):
        gpu_ctx.demosaic_display(t, white=4095.0, filter="cubic")
    with pytest.raises(ValueError):
        gpu_ctx.demosaic_yuv(t, white=4095.0, algo="resample")
    with pytest.raises(M.McrawError, match=SYM):  # a crop that leaves the frame is the library's to reject
        gpu_ctx.demosaic(t, dtype="f32", white=4095.0, algo="resample", size=(6, 10), crop=(2, 0, 8, 16))
    with pytest.raises(M.McrawError, match=SYM):  # 4:2:0 needs an even size
        gpu_ctx.demosaic_yuv(t, white=4095.0, algo="resample", size=(6, 9))
    out = gpu_ctx.demosaic(t, dtype="f32", white=4095.0, algo="resample", size=(6, 10))  # an (H, W) mosaic drops N
    assert tuple(out.shape) == (3, 6, 10)
    empty = gpu_ctx.demosaic(t[None][:0], dtype="f16", white=4095.0, algo="resample", size=(6, 10), filter="linear")
    assert tuple(empty.shape) == (0, 3, 6, 10)
    assert M.fit_crop(3024, 4032, 2160, 3840, algo="resample") == (378, 0, 2268, 4032)
    with pytest.raises(ValueError):
        M.fit_crop(3024, 4032, 2160, 3840)  # outside the area rule, as before
    assert (M.RGB_RESAMPLE, M.FILTER_LINEAR, M.FILTER_CUBIC) == (4, 0, 1) and C.sizeof(M.Resample) == 32


@pytest.mark.parametrize("typ", (7, 6))
def test_decode_yuv_equals_demosaic_yuv_of_plain_decode(gpu_ctx, typ):
    rng = np.random.default_rng(typ)
    w, h = 256, 64
    items = _frames(rng, [(w, h)] * 2, typ)
    ins = [torch.from_numpy(b).to(DEV) for b, _ in items]
    mos = _dev16(np.stack([want for _, want in items]))
    size = (40, 120)
    crop = M.fit_crop(h, w, *size, algo="resample")
    kw = dict(algo="resample", size=size, crop=crop, white=4095.0, black=(64, 64, 64, 64), cfa="grbg", gain=(1.9, 1.0, 1.4), matrix=SRGBISH,
              fmt="nv12", standard="bt601")
    serial = gpu_ctx.last_serial()
    ref = gpu_ctx.demosaic_yuv(mos, **kw)
    torch.cuda.synchronize()
    assert gpu_ctx.last_serial() == serial  # the resample call takes no decode serial
    out = gpu_ctx.decode_yuv(ins, w, h, typ, **kw)
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    lut = M.transfer_lut("bt709", 4096, 12)
    coef = M.yuv_matrix("bt601", "limited", 8, 12)
    for i, (_, want) in enumerate(items):
        assert np.array_equal(_np(out[i]), S.resample_yuv_ref(want, crop, size, 4095.0, lut, "nv12", coef, 12, "cubic", (64, 64, 64, 64), "grbg",
                                                              (1.9, 1.0, 1.4), SRGBISH))
    rest = {k: v for k, v in kw.items() if k not in ("fmt", "standard")}
    f = gpu_ctx.decode_rgb(ins, w, h, typ, dtype="f16", filter="linear", **rest)
    d = gpu_ctx.decode_display(ins, w, h, typ, **rest)
    assert tuple(f.shape) == (2, 3) + size and tuple(d.shape) == (2,) + size + (3,)
    assert torch.equal(d, gpu_ctx.demosaic_display(mos, **rest))
    assert torch.equal(f.view(torch.int16), gpu_ctx.demosaic(mos, dtype="f16", filter="linear", **rest).view(torch.int16))
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
    kw = dict(algo="resample", size=(30, 62), crop=(2, 4, 44, 88), white=4095.0, black=black, cfa=cfa, gain=(1.7, 1.0, 1.4), matrix=SRGBISH)
    a = gpu_ctx.demosaic(t, dtype="f32", defects=defects, denoise=denoise, shading=gm, **kw)
    assert torch.equal(a.view(torch.int32), gpu_ctx.demosaic(three, dtype="f32", **kw).view(torch.int32))
    assert not torch.equal(a.view(torch.int32), gpu_ctx.demosaic(t, dtype="f32", **kw).view(torch.int32))
    b = gpu_ctx.demosaic_yuv(t, defects=defects, denoise=denoise, shading=gm, **kw)
    assert torch.equal(b, gpu_ctx.demosaic_yuv(three, **kw))
    got = _bits(a, torch.int32)
    three_np = _np(three)
    for i in range(n):
        assert np.array_equal(got[i], S.resample_ref(three_np[i], kw["crop"], kw["size"], "f32", 4095.0, "cubic", black, cfa, kw["gain"], SRGBISH))


def test_siblings_unchanged_by_interleaved_resample_calls(gpu_ctx):
    rng = np.random.default_rng(21)
    n, h, w = 2, 40, 264
    imgs = [_mosaic(rng, h, w, 12) for _ in range(n)]
    t = _dev16(np.stack(imgs))
    kw = dict(white=4095.0, black=(60, 61, 62, 63), cfa="grbg", gain=(1.7, 1.0, 1.4), matrix=SRGBISH)
    rs = dict(algo="resample", size=(30, 200), crop=(2, 4, 36, 256))
    ar = dict(algo="area", size=(8, 60), crop=(2, 4, 36, 256))
    lut8, lut12 = M.transfer_lut("srgb", 4096, 8), M.transfer_lut("bt709", 4096, 12)
    coef = M.yuv_matrix("bt709", "limited", 8, 12)
    for algo in ("mhc", "bin2", "area"):
        sib = ar if algo == "area" else dict(algo=algo)
        d0 = gpu_ctx.demosaic_display(t, **sib, **kw)
        r0 = gpu_ctx.demosaic_display(t, **rs, **kw)
        f0 = gpu_ctx.demosaic(t, dtype="f16", **sib, **kw)
        r1 = gpu_ctx.demosaic(t, dtype="f16", **rs, **kw)
        y0 = gpu_ctx.demosaic_yuv(t, **sib, **kw)
        r2 = gpu_ctx.demosaic_yuv(t, **rs, **kw)
        d1 = gpu_ctx.demosaic_display(t, **sib, **kw)
        f1 = gpu_ctx.demosaic(t, dtype="f16", **sib, **kw)
        y1 = gpu_ctx.demosaic_yuv(t, **sib, **kw)
        torch.cuda.synchronize()
        assert torch.equal(d0, d1) and torch.equal(f0.view(torch.int16), f1.view(torch.int16)) and torch.equal(y0, y1)
        for i in range(n):
            if algo == "area":
                assert np.array_equal(_np(d1[i]), A.area_display_ref(imgs[i], ar["crop"], ar["size"], 4095.0, lut8, "u8", "hwc", kw["black"],
                                                                     "grbg", kw["gain"], SRGBISH))
                assert np.array_equal(_bits(f1[i], torch.int16), A.area_ref(imgs[i], ar["crop"], ar["size"], "f16", 4095.0, kw["black"],
                                                                            "grbg", kw["gain"], SRGBISH))
                assert np.array_equal(_np(y1[i]), A.area_yuv_ref(imgs[i], ar["crop"], ar["size"], 4095.0, lut12, "nv12", coef, 12,
                                                                 kw["black"], "grbg", kw["gain"], SRGBISH))
            else:
                assert np.array_equal(_np(d1[i]), D.display_ref(imgs[i], algo, 4095.0, lut8, "u8", "hwc", kw["black"], "grbg", kw["gain"], SRGBISH))
                assert np.array_equal(_bits(f1[i], torch.int16), R.ref_bits(imgs[i], algo, "f16", 4095.0, black=kw["black"], cfa="grbg",
                                                                             gain=kw["gain"], matrix=SRGBISH))
                assert np.array_equal(_np(y1[i]), Y.yuv_ref(imgs[i], algo, 4095.0, lut12, "nv12", coef, 12, kw["black"], "grbg", kw["gain"],
                                                            SRGBISH))
            assert np.array_equal(_np(r0[i]), S.resample_display_ref(imgs[i], rs["crop"], rs["size"], 4095.0, lut8, "u8", "hwc", "cubic",
                                                                     kw["black"], "grbg", kw["gain"], SRGBISH))
            assert np.array_equal(_bits(r1[i], torch.int16), S.resample_ref(imgs[i], rs["crop"], rs["size"], "f16", 4095.0, "cubic",
                                                                            kw["black"], "grbg", kw["gain"], SRGBISH))
            assert np.array_equal(_np(r2[i]), S.resample_yuv_ref(imgs[i], rs["crop"], rs["size"], 4095.0, lut12, "nv12", coef, 12, "cubic",
                                                                 kw["black"], "grbg", kw["gain"], SRGBISH))


def test_flat_and_grey_stay_flat_and_neutral(gpu_ctx):
    for fmt, c_off in (("nv12", 128), ("p010", 512 << 6)):
        grey = torch.full((50, 84), 2000, dtype=torch.int16, device=DEV).view(torch.uint16)
        out = gpu_ctx.demosaic_yuv(grey, algo="resample", size=(34, 58), crop=(2, 2, 46, 80), white=4095.0, fmt=fmt)
        yp, cp = M.yuv_planes(out, 34)
        torch.cuda.synchronize()
        assert (_np(cp) == c_off).all() and len(np.unique(_np(yp))) == 1
