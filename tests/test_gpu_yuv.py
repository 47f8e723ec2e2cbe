"""Y'CbCr 4:2:0 output (mcraw_demosaic_yuv_batch, Context.demosaic_yuv / decode_yuv) on the GPU: every output sample
equals the numpy reference (_yuv_ref), nothing outside the output is written, the input is left as it was, rejected calls
write nothing, each queued call reads its LUT's contents in stream order, and the sibling entry points are undisturbed."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import _display_ref as D
import _libs as L
import _rgb_ref as R
import _yuv_ref as Y
import motioncam_decoder_amd as M
from _demosaic_gpu import CFAS, DEV, GUARD, SENT, SRGBISH, raw_call
from _demosaic_gpu import dev16 as _dev16, frames as _frames, mosaic as _mosaic, rand_lut as _rand_lut, rgb_color as _color
from _demosaic_gpu import rgb_params as _params, to_np as _np

pytestmark = pytest.mark.gpu

TD = {"nv12": torch.uint8, "p010": torch.uint16}
ES = {"nv12": 1, "p010": 2}
FMT_CODE = {"nv12": 1, "p010": 2}
DEF_IN = {"nv12": 12, "p010": 16}
GEOMS = {"mhc": ((66, 18), (64, 16), (40, 12), (1002, 70), (520, 34)),
         "bin2": ((68, 20), (64, 16), (40, 12), (1004, 72), (520, 36))}


def _rand_coef(rng, fmt, in_bits):
    """Hand-made coefficients of both signs that pass the overflow rule, with offsets inside 0 .. top."""
    sh = int(rng.integers(1, 25))
    budget = ((1 << 31) - (1 << (sh + 1))) // (4 * ((1 << in_bits) - 1)) - 1  # |c0| + |c1| + |c2| may reach this
    rows = []
    for _ in range(3):
        mag = rng.dirichlet(np.ones(3)) * budget * rng.uniform(0.5, 1.0)
        rows.append(tuple(int(m) * int(s) for m, s in zip(mag, rng.choice((-1, 1), size=3))))
    top = 255 if fmt == "nv12" else 1023
    coef = (rows[0], rows[1], rows[2], sh, int(rng.integers(0, top + 1)), int(rng.integers(0, top + 1)))
    assert Y.rule_ok(rows, sh, in_bits)
    return coef


def _shape(algo, h, w, n=None):
    ho, wo = (h, w) if algo == "mhc" else (h // 2, w // 2)
    s = (ho * 3 // 2, wo)
    return s if n is None else (n,) + s


def _raw(ctx, prm, y, *args, **kw):
    return raw_call(ctx, "mcraw_demosaic_yuv_batch", prm, y, *args, **kw)


def _yuv(lut_ptr, fmt="nv12", log2=12, in_bits=8, coef=None, reserved=0, code=None):
    cy, cb, cr, sh, y_off, c_off = coef if coef is not None else M.yuv_matrix("bt709", "limited", 8 if fmt == "nv12" else 10, in_bits)
    y = M.Yuv()
    y.format, y.lut_log2, y.in_bits, y.sh, y.y_off, y.c_off = FMT_CODE[fmt] if code is None else code, log2, in_bits, sh, y_off, c_off
    for i in range(3):
        y.cy[i], y.cb[i], y.cr[i] = cy[i], cb[i], cr[i]
    y.reserved, y.lut = reserved, lut_ptr
    return y


def _call_raw(ctx, t, algo, fmt, lut_t, coef, in_bits, white, black, cfa, gain, matrix, out):
    """The C entry point with hand-made coefficients (Context.demosaic_yuv takes yuv_matrix's)."""
    n, h, w = t.shape
    y = _yuv(lut_t.data_ptr(), fmt, int(lut_t.numel()).bit_length() - 1, in_bits, coef)
    rc = _raw(ctx, _params(algo, white, black, cfa), y, [_color(gain, matrix)], 1, t.data_ptr(), w, h * w, w, h, n,
              out.data_ptr(), out.numel() * out.element_size(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, M.load().mcraw_last_error().decode()


@pytest.mark.parametrize("fmt", ("nv12", "p010"))
@pytest.mark.parametrize("cfa", CFAS)
@pytest.mark.parametrize("algo", ("mhc", "bin2"))
def test_yuv_matches_reference(gpu_ctx, algo, cfa, fmt):
    rng = np.random.default_rng(zlib.crc32(("%s%s%s" % (algo, cfa, fmt)).encode()))
    cases = zip(GEOMS[algo], (10, 12, 14, 12, 16), (256, 4096, 65536, 4096, 65536), (8, 12, 16, 10, 13))
    for ((w, h), nbits, size, in_bits) in cases:
        white = float((1 << nbits) - 1)
        black = tuple(int(b) for b in rng.integers(0, 1 << (nbits - 4), size=4))
        imgs = [_mosaic(rng, h, w, nbits) for _ in range(2)]
        lut = _rand_lut(rng, size)
        dl = _dev16(lut)
        gain = (1.8, 1.0, 1.3)
        t = _dev16(np.stack(imgs))
        # yuv_matrix's coefficients through the Python call (a caller's LUT may use any in_bits) ...
        std, rg = ("bt601", "bt709", "bt2020")[int(rng.integers(3))], ("limited", "full")[int(rng.integers(2))]
        out = gpu_ctx.demosaic_yuv(t, algo=algo, white=white, black=black, cfa=cfa, gain=gain, matrix=SRGBISH, fmt=fmt,
                                   standard=std, range=rg, transfer=dl, in_bits=in_bits)
        torch.cuda.synchronize()
        assert tuple(out.shape) == _shape(algo, h, w, 2) and out.dtype == TD[fmt]
        coef = M.yuv_matrix(std, rg, Y.BITS[fmt], in_bits)
        for i in range(2):
            want = Y.yuv_ref(imgs[i], algo, white, lut, fmt, coef, in_bits, black, cfa, gain, SRGBISH)
            assert np.array_equal(_np(out[i]), want), (w, h, nbits, size, std, rg, i)
        # ... and hand-made random ones through the C entry point
        coef = _rand_coef(rng, fmt, in_bits)
        out2 = torch.empty_like(out)
        _call_raw(gpu_ctx, t, algo, fmt, dl, coef, in_bits, white, black, cfa, gain, SRGBISH, out2)
        torch.cuda.synchronize()
        for i in range(2):
            want = Y.yuv_ref(imgs[i], algo, white, lut, fmt, coef, in_bits, black, cfa, gain, SRGBISH)
            assert np.array_equal(_np(out2[i]), want), (w, h, nbits, size, coef, i)


@pytest.mark.parametrize("size", (256, 4096, 65536))
@pytest.mark.parametrize("algo,w,h", [("mhc", 4, 4), ("mhc", 6, 4), ("mhc", 3840, 2160), ("mhc", 8, 1000), ("mhc", 1000, 6),
                                      ("bin2", 4, 4), ("bin2", 3840, 2160), ("bin2", 8, 1000)])
def test_yuv_sizes_builtin_curves(gpu_ctx, algo, w, h, size):
    rng = np.random.default_rng(w * 7 + h + size)
    img = _mosaic(rng, h, w, 12)
    t = _dev16(img)
    for fmt, curve, std, rg in (("nv12", "bt709", "bt709", "limited"), ("p010", "srgb", "bt2020", "full"),
                                ("nv12", 2.2, "bt601", "full"), ("p010", "linear", "bt709", "limited")):
        out = gpu_ctx.demosaic_yuv(t, algo=algo, white=4095.0, black=(64, 65, 66, 67), cfa="gbrg", gain=(2.0, 1.0, 1.5),
                                   matrix=SRGBISH, fmt=fmt, standard=std, range=rg, transfer=curve, lut_size=size)
        torch.cuda.synchronize()
        assert tuple(out.shape) == _shape(algo, h, w) and out.dtype == TD[fmt]
        lut = M.transfer_lut(curve, size, DEF_IN[fmt])
        coef = M.yuv_matrix(std, rg, Y.BITS[fmt], DEF_IN[fmt])
        want = Y.yuv_ref(img, algo, 4095.0, lut, fmt, coef, DEF_IN[fmt], (64, 65, 66, 67), "gbrg", (2.0, 1.0, 1.5), SRGBISH)
        assert np.array_equal(_np(out), want), (fmt, curve)
        ho = h if algo == "mhc" else h // 2
        yp, cp = M.yuv_planes(out, ho)
        assert np.array_equal(_np(yp), want[:ho]) and np.array_equal(_np(cp), want[ho:].reshape(ho // 2, -1, 2))


@pytest.mark.parametrize("algo", ("mhc", "bin2"))
def test_strided_input_per_frame_colours_misaligned_out_sentinels(gpu_ctx, algo):
    rng = np.random.default_rng(11)
    # n > 32: per-frame colours cross the launch pieces; Wo (70, 34) is no multiple of 8, so rows, chroma planes and frames
    # fall on and off the 8- / 16-byte grid
    n, h, w, pitch = 35, 36, (70 if algo == "mhc" else 68), 83
    fstride = h * pitch + 29
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
    dl = _dev16(lut)
    black = (512, 500, 510, 520)
    for fmt in ("nv12", "p010"):
        coef = M.yuv_matrix("bt709", "limited", Y.BITS[fmt], 11)
        nbytes = int(np.prod(_shape(algo, h, w, n))) * ES[fmt]
        for misalign in (0, 8, ES[fmt]):  # aligned; 8-byte only; sample-aligned only (odd byte for nv12)
            buf = torch.full((GUARD + misalign + nbytes + GUARD,), SENT, dtype=torch.uint8, device=DEV)
            out = buf[GUARD + misalign: GUARD + misalign + nbytes].view(TD[fmt]).view(_shape(algo, h, w, n))
            for per in (True, False):
                gpu_ctx.demosaic_yuv(view, algo=algo, white=16383.0, black=black, cfa="bggr", gain=gains if per else gains[0],
                                     matrix=mats if per else mats[0], fmt=fmt, transfer=dl, in_bits=11, out=out)
                torch.cuda.synchronize()
                a = buf.cpu().numpy()
                assert (a[:GUARD + misalign] == SENT).all() and (a[GUARD + misalign + nbytes:] == SENT).all()
                got = _np(out)
                for i in range(n):
                    k = i if per else 0
                    want = Y.yuv_ref(imgs[i], algo, 16383.0, lut, fmt, coef, 11, black, "bggr", gains[k], mats[k])
                    assert np.array_equal(got[i], want), (fmt, misalign, per, i)
                buf.fill_(SENT)
    assert torch.equal(base, before), "the input was written"


@pytest.mark.parametrize("size", (4096, 65536))
def test_same_lut_pointer_new_contents_between_queued_calls(gpu_ctx, size):
    rng = np.random.default_rng(size)
    n, h, w = 3, 64, 256
    imgs = [_mosaic(rng, h, w, 12) for _ in range(n)]
    t = _dev16(np.stack(imgs))
    s = torch.cuda.Stream(DEV)
    dl = torch.empty(size, dtype=torch.int16, device=DEV)
    luts = [_rand_lut(rng, size) for _ in range(4)]
    staged = [torch.from_numpy(x.view(np.int16)).to(DEV) for x in luts]
    torch.cuda.synchronize()
    outs = []
    with torch.cuda.stream(s):
        for k in range(4):  # no host sync between: the LUT is rewritten in stream order between the calls
            dl.copy_(staged[k])
            outs.append(gpu_ctx.demosaic_yuv(t, algo="mhc" if k % 2 == 0 else "bin2", white=4095.0, gain=(1.5, 1.0, 1.3),
                                             fmt="p010", transfer=dl.view(torch.uint16), in_bits=16))
    s.synchronize()
    coef = M.yuv_matrix("bt709", "limited", 10, 16)
    for k, o in enumerate(outs):
        algo = "mhc" if k % 2 == 0 else "bin2"
        got = _np(o)
        for i in range(n):
            assert np.array_equal(got[i], Y.yuv_ref(imgs[i], algo, 4095.0, luts[k], "p010", coef, 16, gain=(1.5, 1.0, 1.3))), k


def test_rejections_write_nothing(gpu_ctx):
    w, h, n = 16, 8, 2
    img = torch.full((n, h, w), 1000, dtype=torch.int16, device=DEV).view(torch.uint16)
    nbytes = n * h * w * 3 // 2 * 2  # p010
    buf = torch.full((nbytes + 64,), SENT, dtype=torch.uint8, device=DEV)
    lutb = torch.zeros(65536 + 64, dtype=torch.int16, device=DEV)
    ip, op, lp = img.data_ptr(), buf.data_ptr(), lutb.data_ptr()
    ok = _color()
    good = M.yuv_matrix("bt709", "limited", 8, 8)

    def coef(**kw):
        d = dict(zip(("cy", "cb", "cr", "sh", "y_off", "c_off"), good))
        d.update(kw)
        return tuple(d[k] for k in ("cy", "cb", "cr", "sh", "y_off", "c_off"))

    # the largest row magnitude the rule admits for in_bits 8, sh 1 -- and one more, which it does not
    edge = ((1 << 31) - 4 - 1) // (4 * 255)
    img6 = torch.full((n, 6, w), 1000, dtype=torch.int16, device=DEV).view(torch.uint16)
    std = (ok,), 1, ip, w, h * w, w, h, n, op, nbytes
    cases = [
        (_params(), None) + std,                                                             # no yuv
        (_params(), _yuv(0)) + std,                                                          # NULL lut
        (_params(), _yuv(lp + 8)) + std,                                                     # lut not 16-byte aligned
        (_params(), _yuv(lp, log2=7)) + std,                                                 # lut_log2 below 8
        (_params(), _yuv(lp, log2=17)) + std,                                                # ... above 16
        (_params(), _yuv(lp, code=0)) + std,                                                 # unknown format
        (_params(), _yuv(lp, code=3)) + std,
        (_params(), _yuv(lp, reserved=1)) + std,                                             # reserved
        (_params(), _yuv(lp, in_bits=7, coef=good)) + std,                                   # in_bits outside 8 .. 16
        (_params(), _yuv(lp, in_bits=17, coef=good)) + std,
        (_params(), _yuv(lp, coef=coef(sh=0))) + std,                                        # sh outside 1 .. 24
        (_params(), _yuv(lp, coef=coef(sh=25, cy=(1, 1, 1), cb=(0, 0, 0), cr=(0, 0, 0)))) + std,
        (_params(), _yuv(lp, coef=coef(y_off=-1))) + std,                                    # offsets outside 0 .. top
        (_params(), _yuv(lp, coef=coef(y_off=256))) + std,
        (_params(), _yuv(lp, coef=coef(c_off=-1))) + std,
        (_params(), _yuv(lp, coef=coef(c_off=256))) + std,
        (_params(), _yuv(lp, "p010", coef=coef(c_off=1024))) + std,
        (_params(), _yuv(lp, coef=coef(sh=1, cy=(edge + 1, 0, 0)))) + std,                   # the overflow rule, each row
        (_params(), _yuv(lp, coef=coef(sh=1, cb=(0, -(edge + 1), 0)))) + std,
        (_params(), _yuv(lp, coef=coef(sh=1, cr=(1, -edge // 2, edge // 2 + 1)))) + std,
        (_params(), _yuv(lp, coef=coef(cy=(-(1 << 31), 0, 0)))) + std,
        (_params(), _yuv(lp, in_bits=9, coef=good)) + std,                                   # fine for 8 bits, too large for 9
        (_params(dtype=2), _yuv(lp)) + std,                                                  # p->dtype
        (_params(flags=1), _yuv(lp)) + std,                                                  # p->flags
        (_params(), _yuv(lp), (ok,), 1, ip, w, h * w, w, h, n, op, n * h * w * 3 // 2 - 1),   # out too small, nv12
        (_params(), _yuv(lp, "p010"), (ok,), 1, ip, w, h * w, w, h, n, op, nbytes - 1),      # ... p010
        (_params(algo="bin2"), _yuv(lp, "p010"), (ok,), 1, ip, w, h * w, w, h, n, op, nbytes // 4 - 2),
        (_params(), _yuv(lp, "p010"), (ok,), 1, ip, w, h * w, w, h, n, op + 1, nbytes),      # out not sample aligned
        # 4:2:0 needs an even Ho and Wo: BIN2 on a width or height that is no multiple of 4
        (_params(algo="bin2"), _yuv(lp), (ok,), 1, img6.data_ptr(), w, 6 * w, w, 6, n, op, nbytes),   # 16 x 6: Ho = 3
        (_params(algo="bin2"), _yuv(lp), (ok,), 1, ip, w, h * w, 14, h, n, op, nbytes),               # 14 x 8: Wo = 7
        (_params(algo="bin2"), _yuv(lp), (ok,), 1, ip, 6, 4 * 6, 6, 4, 1, op, nbytes),                # (6, 4)
        # the rules of mcraw_demosaic_batch
        (_params(), _yuv(lp), (ok,), 1, ip, w, h * w, 15, h, n, op, nbytes),                 # odd width
        (_params(), _yuv(lp), (ok,), 1, ip, w, h * w, w, 2, n, op, nbytes),                  # height below 4
        (_params(), _yuv(lp), (ok,), 1, ip, w - 2, h * w, w, h, n, op, nbytes),              # pitch < width
        (_params(), _yuv(lp), (ok,), 1, ip, w, h * w - w, w, h, n, op, nbytes),              # frame stride too small
        (_params(), _yuv(lp), (ok, ok, ok), 3, ip, w, h * w, w, h, n, op, nbytes),           # ncolors not 1 or n
        (_params(), _yuv(lp), (_color(gain=(float("nan"), 1, 1)),), 1, ip, w, h * w, w, h, n, op, nbytes),
        (_params(white=float("inf")), _yuv(lp)) + std,
        (_params(), _yuv(lp), (ok,), 1, ip + 1, w, h * w, w, h, n, op, nbytes),              # odd in
        (None, _yuv(lp)) + std,
    ]
    bad_algo = _params()
    bad_algo.algo = 3
    bad_cfa = _params()
    bad_cfa.cfa = 4
    cases += [(bad_algo, _yuv(lp)) + std, (bad_cfa, _yuv(lp)) + std]
    serial = gpu_ctx.last_serial()
    for i, c in enumerate(cases):
        rc = _raw(gpu_ctx, *c)
        assert rc < 0, i
        assert M.load().mcraw_last_error().decode().startswith("mcraw_demosaic_yuv_batch"), i
    # BIN2 on 1000 x 6 (Ho = 3), with buffers of that size
    big = torch.zeros((1, 6, 1000), dtype=torch.int16, device=DEV)
    assert _raw(gpu_ctx, _params(algo="bin2"), _yuv(lp), (ok,), 1, big.data_ptr(), 1000, 6000, 1000, 6, 1, op, nbytes) < 0
    assert M.load().mcraw_last_error().decode().startswith("mcraw_demosaic_yuv_batch")
    assert _raw(gpu_ctx, _params(), _yuv(lp), (ok,), 1, ip, w, h * w, w, h, 0, op, 0) == 0  # n == 0: a no-op
    torch.cuda.synchronize()
    gpu_ctx.synchronize()
    assert (buf.cpu().numpy() == SENT).all()
    assert gpu_ctx.last_serial() == serial
    # good calls next to them do write: the rule's edge (LUT of zeros: Y = y_off, chroma = c_off) ...
    at_edge = coef(sh=1, cy=(edge, 0, 0), cb=(0, -edge, 0), cr=(1, -(edge // 2), edge // 2 - 1), y_off=7, c_off=9)
    assert _raw(gpu_ctx, _params(), _yuv(lp, "p010", coef=at_edge), (ok,), 1, ip, w, h * w, w, h, n, op, nbytes) == 0
    torch.cuda.synchronize()
    a = buf.cpu().numpy()
    assert (a[nbytes:] == SENT).all()
    got = a[:nbytes].view(np.uint16).reshape(n, h * 3 // 2, w)
    assert (got[:, :h] == 7 << 6).all() and (got[:, h:] == 9 << 6).all()
    # ... and BIN2 nv12 into exactly its bytes
    buf.fill_(SENT)
    nb2 = n * (h // 2) * (w // 2) * 3 // 2
    assert _raw(gpu_ctx, _params(algo="bin2"), _yuv(lp), (ok,), 1, ip, w, h * w, w, h, n, op, nb2) == 0
    torch.cuda.synchronize()
    a = buf.cpu().numpy()
    assert (a[nb2:] == SENT).all()
    got = a[:nb2].reshape(n, (h // 2) * 3 // 2, w // 2)
    assert (got[:, :h // 2] == 16).all() and (got[:, h // 2:] == 128).all()


def test_python_rejects_odd_output_for_bin2(gpu_ctx):
    for (w, h) in ((6, 4), (1000, 6)):
        t = torch.zeros((h, w), dtype=torch.int16, device=DEV).view(torch.uint16)
        with pytest.raises(M.McrawError, match="mcraw_demosaic_yuv_batch"):
            gpu_ctx.demosaic_yuv(t, algo="bin2", white=4095.0)
    with pytest.raises(ValueError):
        gpu_ctx.demosaic_yuv(torch.zeros((8, 8), dtype=torch.int16, device=DEV).view(torch.uint16), white=4095.0, fmt="i420")
    with pytest.raises(ValueError):  # a built-in curve needs a depth transfer_lut makes
        gpu_ctx.demosaic_yuv(torch.zeros((8, 8), dtype=torch.int16, device=DEV).view(torch.uint16), white=4095.0, in_bits=11)


@pytest.mark.parametrize("typ", (7, 6))
def test_decode_yuv_equals_demosaic_yuv_of_plain_decode(gpu_ctx, typ):
    rng = np.random.default_rng(typ)
    w, h = 512, 96
    items = _frames(rng, [(w, h)] * 3, typ)
    ins = [torch.from_numpy(b).to(DEV) for b, _ in items]
    mos = _dev16(np.stack([want for _, want in items]))
    black, cfa, gain = (64, 64, 64, 64), "grbg", (1.9, 1.0, 1.4)
    gpu_ctx.set_float_out("f32", 4095.0, layout="mosaic", black=(64,) * 4)
    try:
        for algo, fmt in (("mhc", "nv12"), ("bin2", "p010"), ("mhc", "p010")):
            kw = dict(algo=algo, white=4095.0, black=black, cfa=cfa, gain=gain, matrix=SRGBISH, fmt=fmt, standard="bt601")
            serial = gpu_ctx.last_serial()
            ref = gpu_ctx.demosaic_yuv(mos, **kw)
            torch.cuda.synchronize()
            assert gpu_ctx.last_serial() == serial  # demosaic_yuv takes no decode serial
            out = gpu_ctx.decode_yuv(ins, w, h, typ, **kw)
            torch.cuda.synchronize()
            assert np.array_equal(_np(out), _np(ref))
            lut = M.transfer_lut("bt709", 4096, DEF_IN[fmt])
            coef = M.yuv_matrix("bt601", "limited", Y.BITS[fmt], DEF_IN[fmt])
            for i, (_, want) in enumerate(items):
                assert np.array_equal(_np(out[i]), Y.yuv_ref(want, algo, 4095.0, lut, fmt, coef, DEF_IN[fmt], black, cfa, gain,
                                                             SRGBISH))
        # the context's stage is restored: the next plain batch is still the float mosaic
        t = ins[0]
        o = torch.full((w * h * 4,), SENT, dtype=torch.uint8, device=DEV)
        written, status = gpu_ctx.decode_batch(M.Context.make_frames([(t.data_ptr(), t.numel(), w, h, typ, o.data_ptr(), w * h * 2)]))
        assert status == [0]
        import _float_ref as FR
        assert np.array_equal(o.cpu().numpy(), FR.ref_bytes(items[0][1], "f32", 4095.0, "mosaic", (64,) * 4))
    finally:
        gpu_ctx.set_post()
    assert gpu_ctx.errors() == 0


def test_decode_yuv_truncated_frame_raises(gpu_ctx):
    rng = np.random.default_rng(4)
    w, h = 256, 64
    items = _frames(rng, [(w, h)] * 3, 7)
    ins = [torch.from_numpy(b).to(DEV) for b, _ in items]
    ins[1] = ins[1][: ins[1].numel() // 2].clone()
    with pytest.raises(M.McrawError, match="decode_yuv: .*frame 1"):
        gpu_ctx.decode_yuv(ins, w, h, 7, white=4095.0)


def test_siblings_unchanged_by_interleaved_yuv_calls(gpu_ctx):
    rng = np.random.default_rng(21)
    n, h, w = 3, 72, 520
    imgs = [_mosaic(rng, h, w, 12) for _ in range(n)]
    t = _dev16(np.stack(imgs))
    kw = dict(white=4095.0, black=(60, 61, 62, 63), cfa="grbg", gain=(1.7, 1.0, 1.4), matrix=SRGBISH)
    lut8 = M.transfer_lut("srgb", 4096, 8)
    for algo in ("mhc", "bin2"):
        d0 = gpu_ctx.demosaic_display(t, algo=algo, transfer="srgb", dtype=torch.uint8, layout="hwc", **kw)
        f0 = gpu_ctx.demosaic(t, algo=algo, dtype="f16", **kw)
        y0 = gpu_ctx.demosaic_yuv(t, algo=algo, fmt="nv12", **kw)
        y1 = gpu_ctx.demosaic_yuv(t, algo=algo, fmt="p010", **kw)
        d1 = gpu_ctx.demosaic_display(t, algo=algo, transfer="srgb", dtype=torch.uint8, layout="hwc", **kw)
        y2 = gpu_ctx.demosaic_yuv(t, algo=algo, fmt="nv12", **kw)
        f1 = gpu_ctx.demosaic(t, algo=algo, dtype="f16", **kw)
        torch.cuda.synchronize()
        assert torch.equal(d0, d1) and torch.equal(f0.view(torch.int16), f1.view(torch.int16)) and torch.equal(y0, y2)
        for i in range(n):
            assert np.array_equal(_np(d1[i]), D.display_ref(imgs[i], algo, 4095.0, lut8, "u8", "hwc", kw["black"], "grbg",
                                                            kw["gain"], SRGBISH))
            assert np.array_equal(f1[i].cpu().numpy().view(np.uint16),
                                  R.ref_bits(imgs[i], algo, "f16", 4095.0, black=kw["black"], cfa="grbg", gain=kw["gain"],
                                             matrix=SRGBISH))
            for fmt, got in (("nv12", y0), ("p010", y1)):
                want = Y.yuv_ref(imgs[i], algo, 4095.0, M.transfer_lut("bt709", 4096, DEF_IN[fmt]), fmt,
                                 M.yuv_matrix("bt709", "limited", Y.BITS[fmt], DEF_IN[fmt]), DEF_IN[fmt], kw["black"], "grbg",
                                 kw["gain"], SRGBISH)
                assert np.array_equal(_np(got[i]), want)


def test_launches_counted_under_rgb_kernels(gpu_ctx):
    rng = np.random.default_rng(16)
    n, h, w = 4, 256, 1024
    t = _dev16(np.stack([_mosaic(rng, h, w, 12) for _ in range(n)]))
    gpu_ctx.profile(only=["krgb_mhc", "krgb_bin2"])
    try:
        for k in ("krgb_mhc", "krgb_bin2"):
            gpu_ctx.kernel_ms(k, reset=True)
        gpu_ctx.demosaic_yuv(t, algo="mhc", white=4095.0)
        gpu_ctx.demosaic_yuv(t, algo="bin2", white=4095.0, fmt="p010", gain=np.ones((n, 3), np.float32))
        torch.cuda.synchronize()
        ms, launches = gpu_ctx.kernel_ms("krgb_mhc", reset=True)
        assert launches == 1 and ms > 0
        ms, launches = gpu_ctx.kernel_ms("krgb_bin2", reset=True)
        assert launches == 1 and ms > 0
    finally:
        gpu_ctx.profile(enable=False)


def test_grey_input_is_neutral_and_white_hits_the_range_end(gpu_ctx):
    """Identity colours and a grey mosaic: every chroma sample is exactly c_off; a saturated one gives Y = 235 / 940 << 6."""
    for fmt, white_code, c_off in (("nv12", 235, 128), ("p010", 940 << 6, 512 << 6)):
        for algo in ("mhc", "bin2"):
            h, w = 64, 520
            grey = torch.full((h, w), 2000, dtype=torch.int16, device=DEV).view(torch.uint16)
            sat = torch.full((h, w), 4095, dtype=torch.int16, device=DEV).view(torch.uint16)
            ho = h if algo == "mhc" else h // 2
            yg, cg = M.yuv_planes(gpu_ctx.demosaic_yuv(grey, algo=algo, white=4095.0, fmt=fmt), ho)
            ys, cs = M.yuv_planes(gpu_ctx.demosaic_yuv(sat, algo=algo, white=4095.0, fmt=fmt), ho)
            torch.cuda.synchronize()
            assert (_np(cg) == c_off).all() and (_np(cs) == c_off).all()
            assert (_np(ys) == white_code).all() and len(np.unique(_np(yg))) == 1
