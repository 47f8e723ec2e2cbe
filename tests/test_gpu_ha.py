"""The edge-directed demosaic (MCRAW_RGB_HA; algo="ha" of Context.demosaic / demosaic_display / demosaic_yuv and the decode_*
methods) on the GPU: every output sample equals the numpy statement of the contract (_ha_ref) bit for bit -- in the three output
families, at frames where every read reflects, over partial tiles, strided inputs and outputs off the vector grids, with content
that takes every way of both three-way choices --, nothing outside `out` is written, the stages in front run as for "mhc", and
"mhc" and "bin2" are undisturbed."""
import ctypes as C

import numpy as np
import pytest
import torch

import _display_ref as D
import _ha_ref as HA
import _rgb_ref as R
import _yuv_ref as Y
import motioncam_decoder_amd as M
from _demosaic_gpu import CFAS, DEV, GUARD, SENT, SRGBISH, FLOATS, IN_BITS, TD
from _demosaic_gpu import bits as _bits, colours as _colours, dev16 as _dev16, frames as _frames, rand_lut as _rand_lut, to_np as _np

pytestmark = pytest.mark.gpu

BLACK2 = (3, 1, 2, 3)  # above many samples of the 2-bit frames: d is negative there


def ha_params(white=4095.0, black=(0, 0, 0, 0), cfa="rggb", dtype=0, flags=0, algo=6):
    """struct mcraw_rgb for the raw entry points (the shared helper of the older tests knows the codes 1 and 2 only)."""
    p = M.RgbParams()
    p.algo, p.dtype, p.flags, p.cfa, p.white = algo, dtype, flags, R.CFA_CODE[cfa], white
    for i in range(4):
        p.black[i] = black[i]
    return p


def content(seed, h, w):
    """Six frames that take every way of the two choices: 2-bit noise (all three outcomes), 16-bit noise (no ties), one-pixel
    stripes both ways (full swing), a flat frame (only ties), and 2-bit noise again."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([rng.integers(0, 4, (h, w)), rng.integers(0, 1 << 16, (h, w)), (xx & 1) * 65535, (yy & 1) * 65535,
                     np.full((h, w), 2), rng.integers(0, 4, (h, w))]).astype(np.uint16)


_o_cache = {}


def values(imgs, white, black, cfa, gain, matrix, key=None):
    """The f32 outputs of the frames, from the numpy statement; worked out once per `key`."""
    if key is not None and key in _o_cache:
        return _o_cache[key]
    o = [HA.rgb_values(imgs[i], white, black, cfa, *_colours(gain, matrix, i)) for i in range(len(imgs))]
    if key is not None:
        _o_cache[key] = o
    return o


def float_bits(o, dt, clip):
    if clip:
        o = np.minimum(np.maximum(o, np.float32(0.0)), np.float32(1.0))
    if dt == "f32":
        return np.ascontiguousarray(o).view(np.uint32)
    if dt == "f16":
        with np.errstate(over="ignore"):
            return np.ascontiguousarray(o.astype(np.float16)).view(np.uint16)
    from _float_ref import bf16_bits
    return bf16_bits(o).view(np.uint16)


def display_from_o(o, lut, dt, layout):
    q = D.apply_lut(o, lut, dt)
    return np.ascontiguousarray(q.transpose(1, 2, 0)) if layout == "hwc" else q


def check_families(ctx, t, o, cfa, black, white, gain, matrix, lut, floats=(("f32", False), ("f16", True), ("bf16", False)),
                   display=(("u8", "hwc"), ("u16", "chw")), yuv=("nv12", "p010"), tag=None):
    """The Python methods on the (n, h, w) tensor t against the f32 outputs o of the numpy statement."""
    n, h, w = len(o), o[0].shape[1], o[0].shape[2]
    kw = dict(algo="ha", white=white, black=black, cfa=cfa, gain=gain, matrix=matrix)
    views = dict(FLOATS)
    for dt, clip in floats:
        out = ctx.demosaic(t, dtype=dt, clip=clip, **kw)
        torch.cuda.synchronize()
        assert tuple(out.shape) == (n, 3, h, w)
        got = _bits(out, views[dt])
        for i in range(n):
            assert np.array_equal(got[i], float_bits(o[i], dt, clip)), (tag, dt, clip, i)
    dl = _dev16(lut)
    for dt, layout in display:
        out = ctx.demosaic_display(t, dtype=TD[dt], layout=layout, transfer=dl, **kw)
        torch.cuda.synchronize()
        got = _np(out)
        assert got.shape == ((n, h, w, 3) if layout == "hwc" else (n, 3, h, w))
        for i in range(n):
            assert np.array_equal(got[i], display_from_o(o[i], lut, dt, layout)), (tag, dt, layout, i)
    for fmt in yuv:
        out = ctx.demosaic_yuv(t, fmt=fmt, transfer=dl, in_bits=IN_BITS, **kw)
        torch.cuda.synchronize()
        got = _np(out)
        assert got.shape == (n, h * 3 // 2, w) and out.dtype == TD[fmt]
        coef = M.yuv_matrix("bt709", "limited", Y.BITS[fmt], IN_BITS)
        for i in range(n):
            assert np.array_equal(got[i], Y.yuv_from_o(o[i], lut, fmt, coef, IN_BITS)), (tag, fmt, i)


SIZES = ((4, 4), (4, 6), (44, 300), (34, 264))  # (h, w): every read reflects; 2 x 2 tiles, the last partial, w % 8 != 0


def every_way(imgs, black, cfa):
    """Counted from the numpy statement, and asserted: each outcome of the green choice and of the diagonal choice occurs at least 8
    times in the frames a test is about to run."""
    gw, dw = np.zeros(3, int), np.zeros(3, int)
    for img in imgs:
        a, b = HA.ways(img, black, cfa)
        gw += a
        dw += b
    assert gw.min() >= 8 and dw.min() >= 8, (cfa, gw, dw)


def content_facts():
    """What the content is made of: 16-bit noise has no ties -- but on the frame's outermost pixels, where the reflection makes both
    diagonals the same pair --, a flat frame has only ties, 2-bit noise all three outcomes."""
    c = content(12016, 12, 16)
    _, gway, dway = HA.ha_detail(c[1], BLACK2, "rggb")
    assert (gway != 2).all() and (dway[1:-1, 1:-1] != 2).all() and (dway[0][dway[0] >= 0] == 2).all()
    a, b = HA.ways(c[4], BLACK2, "rggb")
    assert a[:2] == [0, 0] and b[:2] == [0, 0]
    a, b = HA.ways(c[0], BLACK2, "rggb")
    assert min(a) >= 8 and min(b) >= 8


@pytest.mark.parametrize("h,w", SIZES)
def test_sizes(gpu_ctx, h, w):
    imgs = content(h * 1000 + w, h, w)
    cfa = CFAS[(h + w) % 4]
    gain, matrix = (1.8, 1.0, 1.3), SRGBISH
    lut = _rand_lut(np.random.default_rng(h + w), 4096)
    if h * w > 24:  # (the 4 x 4 and 6 x 4 frames have 8 and 12 R / B sites in all)
        every_way(imgs, BLACK2, cfa)
    o = values(imgs, 3.5, BLACK2, cfa, gain, matrix)
    check_families(gpu_ctx, _dev16(imgs), o, cfa, BLACK2, 3.5, gain, matrix, lut, tag=(h, w))


@pytest.mark.parametrize("lutn", (4096, 65536))
@pytest.mark.parametrize("cfa", CFAS)
def test_every_cfa_kind_layout_and_lut_place(gpu_ctx, cfa, lutn):
    h, w = 34, 264  # two tile rows, two tile columns; the last lane of a row is whole, the last tile 8 columns wide
    imgs = content(h * 1000 + w, h, w)
    black = BLACK2 if lutn == 4096 else (40000, 3, 64, 65535)  # (d far below zero at two CFA positions)
    white = 3.5 if lutn == 4096 else 65535.0
    gain, matrix = (1.8, 1.0, 1.3), SRGBISH
    every_way(imgs, black, cfa)
    o = values(imgs, white, black, cfa, gain, matrix, key=(cfa, lutn))
    lut = _rand_lut(np.random.default_rng(lutn), lutn)
    floats = tuple((dt, clip) for dt in ("f32", "f16", "bf16") for clip in (False, True)) if lutn == 4096 else ()
    check_families(gpu_ctx, _dev16(imgs), o, cfa, black, white, gain, matrix, lut, floats=floats,
                   display=(("u8", "hwc"), ("u8", "chw"), ("u16", "hwc"), ("u16", "chw")), tag=(cfa, lutn))


def test_strided_input_misaligned_outputs_sentinels(gpu_ctx):
    """Pitch above width, a strided batch at an odd element offset (no 16-byte loads), `out` one element off its grid and on an
    8-byte boundary only, guard bands around it."""
    rng = np.random.default_rng(31)
    h, w, pitch = 34, 70, 83
    imgs = content(34070, h, w)
    n, fstride = len(imgs), 34 * 83 + 29
    base = torch.from_numpy(rng.integers(0, 1 << 16, size=n * fstride + 64, dtype=np.uint16).view(np.int16)).to(DEV)
    v16 = torch.as_strided(base, (n, h, w), (fstride, pitch, 1), 5)
    for i in range(n):
        v16[i].copy_(torch.from_numpy(imgs[i].view(np.int16)).to(DEV))
    view = v16.view(torch.uint16)
    before = base.clone()
    cfa, black, white = "bggr", BLACK2, 3.5
    every_way(imgs, black, cfa)
    gains = np.stack([np.array([1.5 + 0.1 * i, 1.0, 1.9 - 0.1 * i], np.float32) for i in range(n)])
    mats = np.stack([SRGBISH * np.float32(1.0 - 0.03 * i) for i in range(n)])
    o = values(imgs, white, black, cfa, gains, mats)
    lut = _rand_lut(rng, 4096)
    dl = _dev16(lut)
    kw = dict(algo="ha", white=white, black=black, cfa=cfa, gain=gains, matrix=mats)
    coef = {f: M.yuv_matrix("bt709", "limited", Y.BITS[f], IN_BITS) for f in ("nv12", "p010")}
    cases = [("f32", None), ("f16", None), ("u8", "hwc"), ("u8", "chw"), ("u16", "hwc"), ("u16", "chw"), ("nv12", None), ("p010", None)]
    tdf = {"f32": torch.float32, "f16": torch.float16}
    for kind, layout in cases:
        es = 4 if kind == "f32" else 1 if kind in ("u8", "nv12") else 2
        yuv, flt = kind in ("nv12", "p010"), kind in tdf
        shape = (n, h * 3 // 2, w) if yuv else (n, h, w, 3) if layout == "hwc" else (n, 3, h, w)
        nbytes = int(np.prod(shape)) * es
        for off in (0, es, 8):
            buf = torch.full((GUARD + off + nbytes + GUARD,), SENT, dtype=torch.uint8, device=DEV)
            out = buf[GUARD + off:GUARD + off + nbytes].view(tdf[kind] if flt else TD[kind]).view(shape)
            if flt:
                gpu_ctx.demosaic(view, dtype=kind, out=out, **kw)
            elif yuv:
                gpu_ctx.demosaic_yuv(view, fmt=kind, transfer=dl, in_bits=IN_BITS, out=out, **kw)
            else:
                gpu_ctx.demosaic_display(view, dtype=TD[kind], layout=layout, transfer=dl, out=out, **kw)
            torch.cuda.synchronize()
            a = buf.cpu().numpy()
            assert (a[:GUARD + off] == SENT).all() and (a[GUARD + off + nbytes:] == SENT).all(), (kind, layout, off)
            for i in range(n):
                want = (float_bits(o[i], kind, False) if flt else Y.yuv_from_o(o[i], lut, kind, coef[kind], IN_BITS) if yuv
                        else display_from_o(o[i], lut, kind, layout))
                got = a[GUARD + off:GUARD + off + nbytes].copy().view(want.dtype).reshape((n,) + want.shape)[i]
                assert np.array_equal(got, want), (kind, layout, off, i)
    assert torch.equal(base, before), "the input was written"


def test_35_frames_with_their_own_colours(gpu_ctx):
    """More frames than one launch carries colours for (RGB_MAXF = 32): two pieces."""
    n, h, w = 35, 12, 16
    base = content(12016, h, w)
    imgs = np.stack([np.roll(base[i % 6], i, axis=1) if i % 2 == 0 else base[i % 6] ^ np.uint16(i % 4) for i in range(n)])
    gains = np.stack([np.array([1.2 + 0.03 * i, 1.0, 2.2 - 0.03 * i], np.float32) for i in range(n)])
    mats = np.stack([SRGBISH * np.float32(1.0 - 0.01 * i) for i in range(n)])
    content_facts()
    every_way(imgs, BLACK2, "grbg")
    o = values(imgs, 3.5, BLACK2, "grbg", gains, mats)
    assert len({o[i].tobytes() for i in range(n)}) == n
    check_families(gpu_ctx, _dev16(imgs), o, "grbg", BLACK2, 3.5, gains, mats, _rand_lut(np.random.default_rng(35), 4096),
                   floats=(("f16", False),), display=(("u8", "hwc"),), yuv=("nv12",), tag="35")


def test_raw_entry_points_and_rejections_write_nothing(gpu_ctx):
    """The C entry points as they are, with algo 6: the three accept it; a defect is turned down and nothing is written."""
    h, w, n = 12, 16, 2
    imgs = content(12016, h, w)[:n]
    t = _dev16(imgs)
    lib = M.load()
    col = (M.RgbColor * 1)()
    for i in range(3):
        col[0].gain[i] = 1.0
        col[0].m[4 * i] = 1.0
    nbytes = n * 3 * h * w * 4
    buf = torch.full((nbytes + 8,), SENT, dtype=torch.uint8, device=DEV)
    p = ha_params(3.5, BLACK2, "rggb", dtype=1)
    for bad in (dict(dtype=7), dict(cfa=9), dict(white=0.0)):
        q = ha_params(3.5, BLACK2, "rggb", dtype=1)
        for k, v in bad.items():
            setattr(q, k, v)
        rc = lib.mcraw_demosaic_batch(gpu_ctx._h, C.byref(q), col, 1, C.c_void_p(t.data_ptr()), w, h * w, w, h, n, C.c_void_p(buf.data_ptr()),
                                      nbytes, None)
        assert rc < 0 and "unknown algo" not in lib.mcraw_last_error().decode(), bad
    rc = lib.mcraw_demosaic_batch(gpu_ctx._h, C.byref(p), col, 1, C.c_void_p(t.data_ptr()), w, h * w, w, h, n, C.c_void_p(buf.data_ptr()),
                                  nbytes - 1, None)
    assert rc < 0
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == SENT).all()
    rc = lib.mcraw_demosaic_batch(gpu_ctx._h, C.byref(p), col, 1, C.c_void_p(t.data_ptr()), w, h * w, w, h, n, C.c_void_p(buf.data_ptr()),
                                  nbytes, None)
    assert rc == 0, lib.mcraw_last_error().decode()
    torch.cuda.synchronize()
    a = buf.cpu().numpy()
    assert (a[nbytes:] == SENT).all()
    for i in range(n):
        assert np.array_equal(a[:nbytes].view(np.uint32).reshape(n, 3, h, w)[i], HA.ref_bits(imgs[i], "f32", 3.5, black=BLACK2))


def _gain_map(cfa_seed, gh=5, gw=9):
    """A smooth Q3.12 lens-shading map (4, gh, gw): 1.0 in the middle, up to about 1.6 in the corners."""
    yy, xx = np.mgrid[0:gh, 0:gw]
    r2 = ((yy - (gh - 1) / 2) / gh) ** 2 + ((xx - (gw - 1) / 2) / gw) ** 2
    return np.stack([np.rint(4096 * (1.0 + (1.0 + 0.1 * p + 0.05 * cfa_seed) * r2)) for p in range(4)]).astype(np.uint16)


def test_decode_methods_and_the_stages_in_front(gpu_ctx):
    """decode_rgb / decode_display / decode_yuv with algo="ha" against the numpy statement on the oracle's mosaics, and one call with
    denoise= and shading= in front against the stages run one by one."""
    rng = np.random.default_rng(41)
    w, h, typ = 264, 40, 7
    items = _frames(rng, [(w, h)] * 2, typ)
    ins = [torch.from_numpy(b).to(DEV) for b, _ in items]
    imgs = np.stack([want for _, want in items])
    black, cfa, gain = (64, 64, 64, 64), "gbrg", (1.9, 1.0, 1.4)
    kw = dict(white=4095.0, black=black, cfa=cfa, gain=gain, matrix=SRGBISH)
    o = values(imgs, 4095.0, black, cfa, gain, SRGBISH)
    f = gpu_ctx.decode_rgb(ins, w, h, typ, algo="ha", dtype="f32", **kw)
    d = gpu_ctx.decode_display(ins, w, h, typ, algo="ha", transfer="srgb", **kw)
    y = gpu_ctx.decode_yuv(ins, w, h, typ, algo="ha", fmt="p010", **kw)
    torch.cuda.synchronize()
    lut8, lut16 = M.transfer_lut("srgb", 4096, 8), M.transfer_lut("bt709", 4096, 16)
    coef = M.yuv_matrix("bt709", "limited", 10, 16)
    for i in range(2):
        assert np.array_equal(f[i].cpu().numpy().view(np.uint32), float_bits(o[i], "f32", False))
        assert np.array_equal(_np(d[i]), display_from_o(o[i], lut8, "u8", "hwc"))
        assert np.array_equal(_np(y[i]), Y.yuv_from_o(o[i], lut16, "p010", coef, 16))
    # the stages in front, as for "mhc": denoise, then shading, each into a scratch tensor
    nl, shift = M.noise_lut(S=2e-2, O=2e-3, black=64, white=4095)
    gm = _gain_map(1)
    den = dict(lut=nl, shift=shift, radius=1)
    got = gpu_ctx.decode_rgb(ins, w, h, typ, algo="ha", dtype="f16", denoise=den, shading=gm, **kw)
    t = _dev16(imgs)
    staged = gpu_ctx.shade(gpu_ctx.denoise(t, **den), gm, black=black)
    want = gpu_ctx.demosaic(staged, algo="ha", dtype="f16", **kw)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    smos = _np(staged)
    assert not np.array_equal(smos, imgs)
    for i in range(2):
        assert np.array_equal(got[i].cpu().numpy().view(np.uint16), HA.ref_bits(smos[i], "f16", 4095.0, black=black, cfa=cfa, gain=gain, matrix=SRGBISH))
    assert np.array_equal(_np(t), imgs), "the caller's mosaic was written"
    assert gpu_ctx.errors() == 0


def test_mhc_and_bin2_are_undisturbed(gpu_ctx):
    rng = np.random.default_rng(51)
    h, w = 36, 264
    imgs = rng.integers(0, 4096, (2, h, w), dtype=np.uint16)
    t = _dev16(imgs)
    kw = dict(white=4095.0, black=(60, 61, 62, 63), cfa="grbg", gain=(1.7, 1.0, 1.4), matrix=SRGBISH)
    lut = _rand_lut(rng, 4096)
    dl = _dev16(lut)

    def siblings():
        for algo in ("mhc", "bin2"):
            a = gpu_ctx.demosaic(t, algo=algo, dtype="f32", **kw)
            b = gpu_ctx.demosaic_display(t, algo=algo, dtype=torch.uint8, layout="hwc", transfer=dl, **kw)
            torch.cuda.synchronize()
            for i in range(2):
                assert np.array_equal(a[i].cpu().numpy().view(np.uint32), R.ref_bits(imgs[i], algo, "f32", 4095.0, black=kw["black"], cfa=kw["cfa"], gain=kw["gain"], matrix=SRGBISH))
                assert np.array_equal(_np(b[i]), D.display_ref(imgs[i], algo, 4095.0, lut, "u8", "hwc", kw["black"], kw["cfa"], kw["gain"], SRGBISH))

    siblings()
    o = values(imgs, 4095.0, kw["black"], kw["cfa"], kw["gain"], SRGBISH)
    check_families(gpu_ctx, t, o, kw["cfa"], kw["black"], 4095.0, kw["gain"], SRGBISH, lut, floats=(("f32", False),), display=(("u8", "hwc"),),
                   yuv=("nv12",), tag="between")
    siblings()
