"""Display-ready integer RGB (mcraw_demosaic_display_batch, Context.demosaic_display / decode_display) on the GPU: every
output byte equals the numpy reference (_display_ref), nothing outside the output is written, the input is left as it
was, rejected calls write nothing, and each queued call reads its LUT's contents in stream order."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import _display_ref as D
import _libs as L
import _rgb_ref as R
import motioncam_decoder_amd as M
from _demosaic_gpu import CFAS, DEV, GUARD, SENT, SRGBISH, raw_call
from _demosaic_gpu import dev16 as _lut_dev, frames as _frames, mosaic as _mosaic, rand_lut as _rand_lut, rgb_color as _color
from _demosaic_gpu import rgb_params as _params, to_np as _np

pytestmark = pytest.mark.gpu

TD = {"u8": torch.uint8, "u16": torch.uint16}
ES = {"u8": 1, "u16": 2}


def _shape(algo, h, w, layout, n=None):
    ho, wo = (h, w) if algo == "mhc" else (h // 2, w // 2)
    s = (ho, wo, 3) if layout == "hwc" else (3, ho, wo)
    return s if n is None else (n,) + s


@pytest.mark.parametrize("layout", ("hwc", "chw"))
@pytest.mark.parametrize("dtype", ("u8", "u16"))
@pytest.mark.parametrize("cfa", CFAS)
@pytest.mark.parametrize("algo", ("mhc", "bin2"))
def test_display_matches_reference(gpu_ctx, algo, cfa, dtype, layout):
    rng = np.random.default_rng(zlib.crc32(("%s%s%s%s" % (algo, cfa, dtype, layout)).encode()))
    for (w, h, nbits, size) in ((66, 18, 10, 256), (64, 16, 12, 4096), (40, 12, 14, 65536), (1002, 70, 12, 4096),
                                (520, 34, 16, 65536)):
        white = float((1 << nbits) - 1)
        black = tuple(int(b) for b in rng.integers(0, 1 << (nbits - 4), size=4))
        imgs = [_mosaic(rng, h, w, nbits) for _ in range(2)]
        lut = _rand_lut(rng, size)
        gain = (1.8, 1.0, 1.3)
        t = torch.from_numpy(np.stack(imgs).view(np.int16)).to(DEV).view(torch.uint16)
        out = gpu_ctx.demosaic_display(t, algo=algo, white=white, black=black, cfa=cfa, gain=gain, matrix=SRGBISH,
                                       transfer=_lut_dev(lut), dtype=TD[dtype], layout=layout)
        torch.cuda.synchronize()
        assert tuple(out.shape) == _shape(algo, h, w, layout, 2) and out.dtype == TD[dtype]
        for i in range(2):
            want = D.display_ref(imgs[i], algo, white, lut, dtype, layout, black, cfa, gain, SRGBISH)
            assert np.array_equal(_np(out[i]), want), (w, h, nbits, size, i)


@pytest.mark.parametrize("size", (256, 4096, 65536))
@pytest.mark.parametrize("w,h", [(4, 4), (6, 4), (3840, 2160), (8, 1000), (1000, 6)])
def test_display_sizes_builtin_curves(gpu_ctx, w, h, size):
    rng = np.random.default_rng(w * 7 + h + size)
    img = _mosaic(rng, h, w, 12)
    t = torch.from_numpy(img.view(np.int16)).to(DEV).view(torch.uint16)
    for algo, dtype, layout, curve in (("mhc", "u8", "hwc", "srgb"), ("bin2", "u16", "chw", "bt709"),
                                       ("mhc", "u16", "hwc", 2.2), ("bin2", "u8", "chw", "linear")):
        out = gpu_ctx.demosaic_display(t, algo=algo, white=4095.0, black=(64, 65, 66, 67), cfa="gbrg", gain=(2.0, 1.0, 1.5),
                                       matrix=SRGBISH, transfer=curve, lut_size=size, dtype=TD[dtype], layout=layout)
        torch.cuda.synchronize()
        assert tuple(out.shape) == _shape(algo, h, w, layout)
        lut = M.transfer_lut(curve, size, 8 if dtype == "u8" else 16)
        want = D.display_ref(img, algo, 4095.0, lut, dtype, layout, (64, 65, 66, 67), "gbrg", (2.0, 1.0, 1.5), SRGBISH)
        assert np.array_equal(_np(out), want), (algo, dtype, layout, curve)


@pytest.mark.parametrize("algo", ("mhc", "bin2"))
def test_strided_input_per_frame_colours_misaligned_out_sentinels(gpu_ctx, algo):
    rng = np.random.default_rng(11)
    n, h, w, pitch, fstride = 35, 34, 70, 83, 34 * 83 + 29  # n > 32: per-frame colours cross the launch pieces
    imgs = [_mosaic(rng, h, w, 14) for _ in range(n)]
    base = torch.from_numpy(rng.integers(0, 1 << 16, size=n * fstride + 64, dtype=np.uint16).view(np.int16)).to(DEV)
    v16 = torch.as_strided(base, (n, h, w), (fstride, pitch, 1), 5)  # 5: odd element offset, not 16-byte aligned
    for i in range(n):
        v16[i].copy_(torch.from_numpy(imgs[i].view(np.int16)).to(DEV))
    view = v16.view(torch.uint16)
    before = base.clone()
    gains = rng.uniform(0.8, 2.4, size=(n, 3)).astype(np.float32)
    mats = (SRGBISH[None] * rng.uniform(0.6, 1.4, size=(n, 3, 3))).astype(np.float32)
    lut = _rand_lut(rng, 4096)
    dl = _lut_dev(lut)
    black = (512, 500, 510, 520)
    for dtype in ("u8", "u16"):
        nbytes = int(np.prod(_shape(algo, h, w, "hwc", n))) * ES[dtype]
        for misalign in (0, 8, ES[dtype]):  # aligned; 8-byte only; element-aligned only (odd byte for u8)
            for layout in ("hwc", "chw"):
                buf = torch.full((GUARD + misalign + nbytes + GUARD,), SENT, dtype=torch.uint8, device=DEV)
                out = buf[GUARD + misalign: GUARD + misalign + nbytes].view(TD[dtype]).view(_shape(algo, h, w, layout, n))
                for per in (True, False):
                    gpu_ctx.demosaic_display(view, algo=algo, white=16383.0, black=black, cfa="bggr",
                                             gain=gains if per else gains[0], matrix=mats if per else mats[0], transfer=dl,
                                             dtype=TD[dtype], layout=layout, out=out)
                    torch.cuda.synchronize()
                    a = buf.cpu().numpy()
                    assert (a[:GUARD + misalign] == SENT).all() and (a[GUARD + misalign + nbytes:] == SENT).all()
                    got = _np(out)
                    for i in range(n):
                        k = i if per else 0
                        want = D.display_ref(imgs[i], algo, 16383.0, lut, dtype, layout, black, "bggr", gains[k], mats[k])
                        assert np.array_equal(got[i], want), (dtype, misalign, layout, per, i)
    assert torch.equal(base, before), "the input was written"


def test_identity_lut_gives_index(gpu_ctx):
    rng = np.random.default_rng(3)
    img = _mosaic(rng, 64, 520, 12)
    t = torch.from_numpy(img.view(np.int16)).to(DEV).view(torch.uint16)
    ident = np.arange(65536, dtype=np.uint16)
    for algo in ("mhc", "bin2"):
        out = gpu_ctx.demosaic_display(t, algo=algo, white=4095.0, gain=(1.7, 1.0, 1.4), matrix=SRGBISH, transfer=ident,
                                       dtype=torch.uint16, layout="chw")
        torch.cuda.synchronize()
        o = R.rgb_values(img, algo, 4095.0, gain=(1.7, 1.0, 1.4), matrix=SRGBISH)
        assert np.array_equal(_np(out), D.lut_index(o, 65536).astype(np.uint16))


def test_inf_and_nan_outputs_index_top_and_zero(gpu_ctx):
    # white 1 and gain 3e38 make v = E * k overflow to +inf wherever E > 16; matrix row (1, -1, 1) gives inf - inf = NaN
    rng = np.random.default_rng(6)
    img = rng.integers(100, 4096, size=(16, 64), dtype=np.uint16)
    t = torch.from_numpy(img.view(np.int16)).to(DEV).view(torch.uint16)
    m = np.array([[1, 1, 1], [1, -1, 1], [-1, -1, -1]], np.float32)
    gain = (3e38, 3e38, 3e38)
    lut = np.arange(4096, dtype=np.uint16) * 16 + 5
    for algo in ("mhc", "bin2"):
        out = gpu_ctx.demosaic_display(t, algo=algo, white=1.0, gain=gain, matrix=m, transfer=lut, dtype=torch.uint16,
                                       layout="chw")
        torch.cuda.synchronize()
        with np.errstate(over="ignore", invalid="ignore"):
            o = R.rgb_values(img, algo, 1.0, gain=gain, matrix=m)
            want = D.display_ref(img, algo, 1.0, lut, "u16", "chw", gain=gain, matrix=m)
        assert np.isposinf(o[0]).any() and np.isnan(o[1]).any() and np.isneginf(o[2]).any()
        got = _np(out)
        assert (got[0][np.isposinf(o[0])] == lut[4095]).all()
        assert (got[1][np.isnan(o[1])] == lut[0]).all()
        assert (got[2][np.isneginf(o[2])] == lut[0]).all()
        assert np.array_equal(got, want)


def _raw(ctx, prm, d, *args, **kw):
    return raw_call(ctx, "mcraw_demosaic_display_batch", prm, d, *args, **kw)


def _disp(lut_ptr, dtype=1, layout=1, log2=12, reserved=0):
    d = M.Display()
    d.dtype, d.layout, d.lut_log2, d.reserved, d.lut = dtype, layout, log2, reserved, lut_ptr
    return d


def test_rejections_write_nothing(gpu_ctx):
    w, h, n = 16, 8, 2
    img = torch.full((n, h, w), 1000, dtype=torch.int16, device=DEV).view(torch.uint16)
    nbytes = n * 3 * h * w * 2
    buf = torch.full((nbytes + 64,), SENT, dtype=torch.uint8, device=DEV)
    lutb = torch.zeros(65536 + 64, dtype=torch.int16, device=DEV)
    ip, op, lp = img.data_ptr(), buf.data_ptr(), lutb.data_ptr()
    ok = _color()
    u8b = n * 3 * h * w
    cases = [
        (_params(), None, [ok], 1, ip, w, h * w, w, h, n, op, nbytes),                      # no display
        (_params(), _disp(0), [ok], 1, ip, w, h * w, w, h, n, op, nbytes),                  # NULL lut
        (_params(), _disp(lp + 8), [ok], 1, ip, w, h * w, w, h, n, op, nbytes),             # lut not 16-byte aligned
        (_params(), _disp(lp, log2=7), [ok], 1, ip, w, h * w, w, h, n, op, nbytes),         # lut_log2 below 8
        (_params(), _disp(lp, log2=17), [ok], 1, ip, w, h * w, w, h, n, op, nbytes),        # ... above 16
        (_params(), _disp(lp, dtype=0), [ok], 1, ip, w, h * w, w, h, n, op, nbytes),        # unknown dtype
        (_params(), _disp(lp, dtype=3), [ok], 1, ip, w, h * w, w, h, n, op, nbytes),
        (_params(), _disp(lp, layout=2), [ok], 1, ip, w, h * w, w, h, n, op, nbytes),       # unknown layout
        (_params(), _disp(lp, reserved=1), [ok], 1, ip, w, h * w, w, h, n, op, nbytes),     # reserved
        (_params(dtype=2), _disp(lp), [ok], 1, ip, w, h * w, w, h, n, op, nbytes),          # p->dtype
        (_params(flags=1), _disp(lp), [ok], 1, ip, w, h * w, w, h, n, op, nbytes),          # p->flags
        (_params(), _disp(lp, dtype=1), [ok], 1, ip, w, h * w, w, h, n, op, u8b - 1),       # out too small, u8
        (_params(), _disp(lp, dtype=2), [ok], 1, ip, w, h * w, w, h, n, op, nbytes - 1),    # ... u16
        (_params(algo="bin2"), _disp(lp, dtype=2), [ok], 1, ip, w, h * w, w, h, n, op, nbytes // 4 - 2),
        (_params(), _disp(lp, dtype=2), [ok], 1, ip, w, h * w, w, h, n, op + 1, nbytes),    # out not element aligned
        # the rules of mcraw_demosaic_batch
        (_params(), _disp(lp), [ok], 1, ip, w, h * w, 15, h, n, op, nbytes),                # odd width
        (_params(), _disp(lp), [ok], 1, ip, w, h * w, w, 2, n, op, nbytes),                 # height below 4
        (_params(), _disp(lp), [ok], 1, ip, w - 2, h * w, w, h, n, op, nbytes),             # pitch < width
        (_params(), _disp(lp), [ok], 1, ip, w, h * w - w, w, h, n, op, nbytes),             # frame stride too small
        (_params(), _disp(lp), [ok, ok, ok], 3, ip, w, h * w, w, h, n, op, nbytes),         # ncolors not 1 or n
        (_params(), _disp(lp), [_color(gain=(float("nan"), 1, 1))], 1, ip, w, h * w, w, h, n, op, nbytes),
        (_params(white=float("inf")), _disp(lp), [ok], 1, ip, w, h * w, w, h, n, op, nbytes),
        (_params(cfa="rggb"), _disp(lp), [ok], 1, ip + 1, w, h * w, w, h, n, op, nbytes),   # odd in
        (None, _disp(lp), [ok], 1, ip, w, h * w, w, h, n, op, nbytes),
    ]
    bad_algo = _params()
    bad_algo.algo = 3
    bad_cfa = _params()
    bad_cfa.cfa = 4
    cases += [(bad_algo, _disp(lp), [ok], 1, ip, w, h * w, w, h, n, op, nbytes),
              (bad_cfa, _disp(lp), [ok], 1, ip, w, h * w, w, h, n, op, nbytes)]
    serial = gpu_ctx.last_serial()
    for i, c in enumerate(cases):
        rc = _raw(gpu_ctx, *c)
        assert rc < 0, i
        assert M.load().mcraw_last_error().decode().startswith("mcraw_demosaic_display_batch"), i
    assert _raw(gpu_ctx, _params(), _disp(lp), [ok], 1, ip, w, h * w, w, h, 0, op, 0) == 0  # n == 0: a no-op
    torch.cuda.synchronize()
    gpu_ctx.synchronize()
    assert (buf.cpu().numpy() == SENT).all()
    assert gpu_ctx.last_serial() == serial
    # the good call next to them does write (LUT of zeros)
    assert _raw(gpu_ctx, _params(), _disp(lp, dtype=2), [ok], 1, ip, w, h * w, w, h, n, op, nbytes) == 0
    torch.cuda.synchronize()
    a = buf.cpu().numpy()
    assert (a[:nbytes] == 0).all() and (a[nbytes:] == SENT).all()


@pytest.mark.parametrize("size", (4096, 65536))
def test_same_lut_pointer_new_contents_between_queued_calls(gpu_ctx, size):
    rng = np.random.default_rng(size)
    n, h, w = 3, 64, 256
    imgs = [_mosaic(rng, h, w, 12) for _ in range(n)]
    t = torch.from_numpy(np.stack(imgs).view(np.int16)).to(DEV).view(torch.uint16)
    s = torch.cuda.Stream(DEV)
    dl = torch.empty(size, dtype=torch.int16, device=DEV)
    luts = [_rand_lut(rng, size) for _ in range(4)]
    staged = [torch.from_numpy(x.view(np.int16)).to(DEV) for x in luts]
    torch.cuda.synchronize()
    outs = []
    with torch.cuda.stream(s):
        for k in range(4):  # no host sync between: the LUT is rewritten in stream order between the calls
            dl.copy_(staged[k])
            outs.append(gpu_ctx.demosaic_display(t, algo="mhc" if k % 2 == 0 else "bin2", white=4095.0, gain=(1.5, 1.0, 1.3),
                                                 transfer=dl.view(torch.uint16), dtype=torch.uint16, layout="hwc"))
    s.synchronize()
    for k, o in enumerate(outs):
        algo = "mhc" if k % 2 == 0 else "bin2"
        got = _np(o)
        for i in range(n):
            assert np.array_equal(got[i], D.display_ref(imgs[i], algo, 4095.0, luts[k], "u16", "hwc", gain=(1.5, 1.0, 1.3))), k


@pytest.mark.parametrize("typ", (7, 6))
def test_decode_display_matches_reference_of_oracle(gpu_ctx, typ):
    rng = np.random.default_rng(typ)
    w, h = 512, 96
    items = _frames(rng, [(w, h)] * 3, typ)
    ins = [torch.from_numpy(b).to(DEV) for b, _ in items]
    black, cfa, gain = (64, 64, 64, 64), "grbg", (1.9, 1.0, 1.4)
    for algo, dtype, layout in (("mhc", "u8", "hwc"), ("bin2", "u16", "chw"), ("mhc", "u16", "hwc")):
        out = gpu_ctx.decode_display(ins, w, h, typ, algo=algo, white=4095.0, black=black, cfa=cfa, gain=gain,
                                     matrix=SRGBISH, transfer="srgb", dtype=TD[dtype], layout=layout)
        torch.cuda.synchronize()
        lut = M.transfer_lut("srgb", 4096, 8 if dtype == "u8" else 16)
        for i, (_, want) in enumerate(items):
            assert np.array_equal(_np(out[i]), D.display_ref(want, algo, 4095.0, lut, dtype, layout, black, cfa, gain,
                                                             SRGBISH))


def test_decode_display_truncated_frame_raises(gpu_ctx):
    rng = np.random.default_rng(4)
    w, h = 256, 64
    items = _frames(rng, [(w, h)] * 3, 7)
    ins = [torch.from_numpy(b).to(DEV) for b, _ in items]
    ins[1] = ins[1][: ins[1].numel() // 2].clone()
    with pytest.raises(M.McrawError, match="decode_display: .*frame 1"):
        gpu_ctx.decode_display(ins, w, h, 7, white=4095.0)


def test_stage_and_serial_left_alone(gpu_ctx):
    rng = np.random.default_rng(8)
    w, h = 128, 32
    items = _frames(rng, [(w, h)], 7)
    t = torch.from_numpy(items[0][0]).to(DEV)
    mos = torch.from_numpy(items[0][1].view(np.int16)).to(DEV).view(torch.uint16)
    gpu_ctx.set_float_out("f32", 4095.0, layout="mosaic", black=(64,) * 4)
    try:
        serial = gpu_ctx.last_serial()
        gpu_ctx.demosaic_display(mos, white=4095.0)
        torch.cuda.synchronize()
        assert gpu_ctx.last_serial() == serial
        gpu_ctx.decode_display([t], w, h, 7, white=4095.0)
        out = torch.full((w * h * 4,), SENT, dtype=torch.uint8, device=DEV)
        written, status = gpu_ctx.decode_batch(M.Context.make_frames([(t.data_ptr(), t.numel(), w, h, 7, out.data_ptr(), w * h * 2)]))
        assert status == [0]
        import _float_ref as FR
        assert np.array_equal(out.cpu().numpy(), FR.ref_bytes(items[0][1], "f32", 4095.0, "mosaic", (64,) * 4))
    finally:
        gpu_ctx.set_post()
    assert gpu_ctx.errors() == 0


def test_launches_counted_under_rgb_kernels(gpu_ctx):
    rng = np.random.default_rng(16)
    n, h, w = 4, 256, 1024
    t = torch.from_numpy(np.stack([_mosaic(rng, h, w, 12) for _ in range(n)]).view(np.int16)).to(DEV).view(torch.uint16)
    gpu_ctx.profile(only=["krgb_mhc", "krgb_bin2"])
    try:
        for k in ("krgb_mhc", "krgb_bin2"):
            gpu_ctx.kernel_ms(k, reset=True)
        gpu_ctx.demosaic_display(t, algo="mhc", white=4095.0)
        gpu_ctx.demosaic_display(t, algo="bin2", white=4095.0, gain=np.ones((n, 3), np.float32))
        torch.cuda.synchronize()
        ms, launches = gpu_ctx.kernel_ms("krgb_mhc", reset=True)
        assert launches == 1 and ms > 0
        ms, launches = gpu_ctx.kernel_ms("krgb_bin2", reset=True)
        assert launches == 1 and ms > 0
    finally:
        gpu_ctx.profile(enable=False)


def test_srgb_u8_within_one_code_of_float64(gpu_ctx):
    n, h, w = 2, 128, 512
    imgs = [L.natural_image_np(w, h, 12, 12.0, 40 + i) for i in range(n)]
    t = torch.from_numpy(np.stack(imgs).view(np.int16)).to(DEV).view(torch.uint16)
    kw = dict(algo="mhc", white=4095.0, black=(64,) * 4, gain=(2.0, 1.0, 1.6), matrix=SRGBISH)
    lin = gpu_ctx.demosaic(t, dtype="f32", clip=True, **kw)
    disp = gpu_ctx.demosaic_display(t, transfer="srgb", lut_size=4096, dtype=torch.uint8, layout="chw", **kw)
    torch.cuda.synchronize()
    x = lin.cpu().numpy().astype(np.float64)
    want = np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(x, 1 / 2.4) - 0.055) * 255.0
    diff = np.abs(disp.cpu().numpy().astype(np.float64) - want)
    assert diff.max() <= 1.0 + 1e-9, diff.max()
