"""The mesh warp of the demosaic (mcraw_demosaic_mesh_batch; algo="mesh" of Context.demosaic / demosaic_display / demosaic_yuv and
the decode_* methods) on the GPU: every output byte equals the numpy statement of the contract (_mesh_ref), also where a mesh leaves
the regime and the frame and both clamps act; a whole-sample translation mesh is algo "mhc" cut there and a fractional one is algo
"warp"; nothing outside `out` is written."""
import ctypes as C

import numpy as np
import pytest
import torch

import _mesh_ref as MR
import _warp_ref as W
import _yuv_ref as Y
import motioncam_decoder_amd as M
from _demosaic_gpu import CFAS, DEV, GUARD, SENT, SRGBISH
from _demosaic_gpu import dev16 as _dev16, frames as _frames, mosaic as _mosaic, rand_lut as _rand_lut
from _demosaic_gpu import FLOATS, IN_BITS, TD, as_int as _as_int, bits as _bits, colours as _colours, to_np as _np

pytestmark = pytest.mark.gpu

H, WD, SIZE = 72, 136, (40, 70)  # 2 x 3 tiles with partial last tiles; the last lane of a row holds 6 of its 8 columns
# tests/test_gpu_warp_paths.py's three extreme maps, placed as there
LINS = ((65536 + 9000, 12000, -12000, 65536 + 9000), (65536 - 11000, -14000, 14000, 65536 - 11000), (65536, 3000, 5000, 65536 + 16384))


def _maps():
    maps = []
    for i, lin in enumerate(LINS):
        m = [lin[0], lin[1], 0, lin[2], lin[3], 0]
        Yp, Xp = W.positions(m, SIZE)
        m[2] = -int(Yp.min()) + (256 * (H - 1) - int(Yp.max() - Yp.min())) * (i + 1) // 4
        m[5] = -int(Xp.min()) + (256 * (WD - 1) - int(Xp.max() - Xp.min())) * (3 - i) // 4
        assert W.map_ok(m, SIZE, H, WD)
        maps.append(m)
    return np.asarray(maps, dtype=np.int32)


def _hostile(size, h, w):
    """One tile 120 samples across and far outside the regime, nodes outside the frame on two sides: both clamps act."""
    mesh = MR.translation_mesh(size, 4, 6)
    mesh[:, 1:, 1] += 256 * 88       # tile column 0 reads 32 + 88 = 120 samples across
    mesh[0, :, 0] -= 256 * 9         # the first rows read above the frame
    mesh[-1, -1] = (256 * (h + 50), 256 * (w + 70))
    Yr, Xr = MR.raw_positions(mesh, size)
    Yc, Xc, r, c = MR.tap_origins(mesh, size, h, w)
    assert not MR.in_regime(mesh, size, h, w) and (Yr != Yc).any() and (Xr != Xc).any() and ((Xc >> 8) - 1 != c).any()
    return mesh


def _values(imgs, meshes, size, filt, black, cfa, white, gain, matrix):
    return [MR.values(MR.mesh_estimates(imgs[i], meshes[i if len(meshes) > 1 else 0], size, filt, black, cfa), white, black, *_colours(gain, matrix, i))
            for i in range(len(imgs))]


def _check_families(ctx, t, imgs, meshes, size, cfa="rggb", black=(0, 0, 0, 0), white=4095.0, gain=(1.8, 1.0, 1.3), matrix=SRGBISH, lut=None,
                    filt="cubic", floats=("f32", "f16", "bf16"), display=(("u8", "hwc"), ("u16", "chw")), yuv=None, tag=None, device_mesh=True):
    """The families and kinds of the Python methods on the (n, h, w) tensor t of the frames imgs against the numpy statement; meshes
    (nmesh, My, Mx, 2): one mesh, or one per frame; as a CUDA tensor or as the numpy array."""
    n = len(imgs)
    ho, wo = size
    meshes = np.ascontiguousarray(np.asarray(meshes, dtype=np.int32).reshape((-1,) + MR.grid(size) + (2,)))
    yuv = ((ho % 2 == 0 and wo % 2 == 0) and ("nv12", "p010")) if yuv is None else yuv
    o = _values(imgs, meshes, size, filt, black, cfa, white, gain, matrix)
    arg = torch.from_numpy(meshes).to(DEV) if device_mesh else meshes
    kw = dict(algo="mesh", size=size, mesh=arg, filter=filt, white=white, black=black, cfa=cfa, gain=gain, matrix=matrix, check=False)
    for dt, view in FLOATS:
        if dt not in floats:
            continue
        clip = dt == "f16"
        out = ctx.demosaic(t, dtype=dt, clip=clip, **kw)
        torch.cuda.synchronize()
        assert tuple(out.shape) == (n, 3, ho, wo)
        got = _bits(out, view)
        for i in range(n):
            want = MR.float_bits(np.clip(o[i], np.float32(0), np.float32(1)) if clip else o[i], dt)
            assert np.array_equal(got[i], want), (tag, dt, i)
    lut = _rand_lut(np.random.default_rng(ho * 131 + wo), 4096) if lut is None else lut
    dl = _dev16(lut)
    for dt, layout in display:
        out = ctx.demosaic_display(t, dtype=TD[dt], layout=layout, transfer=dl, **kw)
        torch.cuda.synchronize()
        got = _np(out)
        assert got.shape == ((n, ho, wo, 3) if layout == "hwc" else (n, 3, ho, wo))
        for i in range(n):
            assert np.array_equal(got[i], MR.display_from_o(o[i], lut, dt, layout)), (tag, dt, layout, i)
    for fmt in yuv or ():
        out = ctx.demosaic_yuv(t, fmt=fmt, transfer=dl, in_bits=IN_BITS, **kw)
        torch.cuda.synchronize()
        got = _np(out)
        assert got.shape == (n, ho * 3 // 2, wo) and out.dtype == TD[fmt]
        coef = M.yuv_matrix("bt709", "limited", Y.BITS[fmt], IN_BITS)
        for i in range(n):
            assert np.array_equal(got[i], MR.yuv_from_o(o[i], lut, fmt, coef, IN_BITS)), (tag, fmt, i)


@pytest.fixture(scope="module")
def frames3():
    rng = np.random.default_rng(20261101)
    imgs = [_mosaic(rng, H, WD, 12) for _ in range(3)]
    return imgs, _dev16(np.stack(imgs))


@pytest.mark.parametrize("cfa", CFAS)
def test_whole_sample_translation_mesh_equals_mhc_cut(gpu_ctx, frames3, cfa):
    imgs, t = frames3
    kw = dict(white=4095.0, black=(60, 61, 62, 63), cfa=cfa, gain=(1.8, 1.0, 1.3), matrix=SRGBISH)
    dl = _dev16(_rand_lut(np.random.default_rng(1), 4096))
    h, w = SIZE
    for y0, x0 in ((2, 4), (31, 65)):
        ar = dict(algo="mesh", size=SIZE, mesh=torch.from_numpy(MR.translation_mesh(SIZE, y0, x0)).to(DEV))
        for filt in ("cubic", "linear"):
            for dt, view in FLOATS:
                a, b = gpu_ctx.demosaic(t, dtype=dt, filter=filt, **ar, **kw), gpu_ctx.demosaic(t, algo="mhc", dtype=dt, **kw)
                assert torch.equal(a.view(view), b[:, :, y0:y0 + h, x0:x0 + w].contiguous().view(view)), (y0, x0, filt, dt)
            for dt, layout in ((torch.uint8, "hwc"), (torch.uint16, "chw")):
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
                yb, cb = M.yuv_planes(b, H)
                assert torch.equal(_as_int(ya), _as_int(yb[:, y0:y0 + h, x0:x0 + w].contiguous())), (y0, x0, fmt)
                assert torch.equal(_as_int(ca), _as_int(cb[:, y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2].contiguous())), (y0, x0, fmt)


@pytest.mark.parametrize("filt", ("cubic", "linear"))
def test_fractional_translation_equals_algo_warp(gpu_ctx, frames3, filt):
    imgs, t = frames3
    dl = _dev16(_rand_lut(np.random.default_rng(2), 4096))
    kw = dict(size=SIZE, filter=filt, white=4095.0, black=(64, 67, 61, 70), cfa="grbg", gain=(1.8, 1.0, 1.3), matrix=SRGBISH)
    for ty, tx in ((256 * 3 + 1, 256 * 9 + 255), (256 * 31 + 128, 128), (77, 256 * 66)):
        m = np.array([65536, 0, ty, 0, 65536, tx], dtype=np.int32)
        mesh = M.affine_mesh(m, SIZE)
        a = gpu_ctx.demosaic(t, algo="mesh", mesh=mesh, dtype="f32", **kw)
        b = gpu_ctx.demosaic(t, algo="warp", affine=m, dtype="f32", **kw)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (ty, tx)
        a = gpu_ctx.demosaic_display(t, algo="mesh", mesh=mesh, transfer=dl, **kw)
        assert torch.equal(a, gpu_ctx.demosaic_display(t, algo="warp", affine=m, transfer=dl, **kw)), (ty, tx)
        a = gpu_ctx.demosaic_yuv(t, algo="mesh", mesh=mesh, transfer=dl, in_bits=IN_BITS, **kw)
        assert torch.equal(a, gpu_ctx.demosaic_yuv(t, algo="warp", affine=m, transfer=dl, in_bits=IN_BITS, **kw)), (ty, tx)
    _check_families(gpu_ctx, t, imgs, M.affine_mesh([65536, 0, 256 * 2 + 77, 0, 65536, 256 * 5 + 201], SIZE), SIZE, "grbg", (64, 67, 61, 70), filt=filt,
                    floats=("f32",), display=(("u8", "hwc"),), yuv=("nv12",), tag="statement")


@pytest.mark.parametrize("cfa", CFAS)
def test_extreme_affine_meshes_per_frame(gpu_ctx, frames3, cfa):
    """affine_mesh of the three extreme maps, one mesh per frame (nmesh = n), and the first of them for the batch (nmesh = 1)."""
    imgs, t = frames3
    meshes = M.affine_mesh(_maps(), SIZE)
    assert all(MR.in_regime(m, SIZE, H, WD) for m in meshes)
    filt = "linear" if cfa == "gbrg" else "cubic"
    _check_families(gpu_ctx, t, imgs, meshes, SIZE, cfa, (256, 257, 258, 259), 16383.0, filt=filt, floats=("f16",), display=(("u8", "chw"),),
                    yuv=("nv12",), tag=cfa)
    _check_families(gpu_ctx, t, imgs, meshes[1:2], SIZE, cfa, (256, 257, 258, 259), 16383.0, filt=filt, floats=("f32",), display=(), yuv=("p010",),
                    tag=(cfa, "one mesh"), device_mesh=False)


def test_barrel_mesh(gpu_ctx, frames3):
    imgs, t = frames3
    mesh = M.distortion_mesh(H, WD, SIZE, radial=(1.0, -0.35, 0.08, 0.0), tangential=(0.004, -0.003), center=(0.47, 0.52))
    assert MR.in_regime(mesh, SIZE, H, WD) and mesh.shape == MR.grid(SIZE) + (2,)
    M.mesh_check(mesh, H, WD, SIZE)
    _check_families(gpu_ctx, t, imgs, mesh, SIZE, "bggr", (60, 61, 62, 63), tag="barrel")
    # a numpy mesh goes through mesh_check and is uploaded; (My, Mx, 2) and (1, My, Mx, 2) are the same call
    kw = dict(algo="mesh", size=SIZE, white=4095.0, dtype="f32")
    a = gpu_ctx.demosaic(t, mesh=mesh, **kw)
    b = gpu_ctx.demosaic(t, mesh=torch.from_numpy(mesh[None]).to(DEV), **kw)
    c = gpu_ctx.demosaic(t, mesh=torch.from_numpy(mesh), **kw)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32))


@pytest.mark.parametrize("filt", ("cubic", "linear"))
def test_mesh_outside_the_regime_and_the_frame_is_defined(gpu_ctx, frames3, filt):
    """One tile 120 samples across, nodes outside the frame: the tap clamp and the border rule act, and the result is the statement's
    bit for bit.  The host check names the tile; check=False and a CUDA tensor take the mesh as it is."""
    imgs, t = frames3
    mesh = _hostile(SIZE, H, WD)
    with pytest.raises(ValueError, match=r"demosaic: mesh: mcraw_mesh_check: the mesh of frame 0: tile \(0, 0\) reads"):
        gpu_ctx.demosaic(t, algo="mesh", size=SIZE, mesh=mesh, dtype="f32", white=4095.0)
    one = dict(floats=("f32",), display=(("u8", "hwc"),), yuv=("nv12",))
    _check_families(gpu_ctx, t, imgs, mesh, SIZE, "grbg", (64, 64, 64, 64), filt=filt, tag="hostile", **one)
    _check_families(gpu_ctx, t, imgs, mesh, SIZE, "rggb", (64, 64, 64, 64), filt=filt, tag="hostile, numpy", device_mesh=False, floats=("bf16",),
                    display=(), yuv=())
    rng = np.random.default_rng(5)
    wild = rng.integers(-2 ** 31, 2 ** 31, size=(3,) + MR.grid(SIZE) + (2,)).astype(np.int32)  # any node content: the 64-bit form
    _check_families(gpu_ctx, t, imgs, wild, SIZE, "gbrg", (64, 64, 64, 64), filt=filt, tag="wild", floats=("f32",), display=(), yuv=("nv12",))


def test_8x8_mosaic_onto_2x2_every_tap_reflects(gpu_ctx):
    rng = np.random.default_rng(8)
    imgs = [_mosaic(rng, 8, 8, 12) for _ in range(2)]
    t = _dev16(np.stack(imgs))
    for k, (ty, tx) in enumerate(((0, 0), (6 * 256, 6 * 256), (0, 6 * 256 + 128), (3 * 256 + 200, 77))):
        mesh = M.affine_mesh([65536, 0, ty, 0, 65536, tx], (2, 2))
        _check_families(gpu_ctx, t, imgs, mesh, (2, 2), CFAS[k], (64, 64, 64, 64), tag=(ty, tx), floats=("f32",), display=(("u16", "hwc"),), yuv=("nv12",))
    far = np.array([[[-70000, 90000], [5, -3]], [[2 ** 31 - 1, -2 ** 31], [900, 2000]]], dtype=np.int32)  # the corners of the frame and beyond
    _check_families(gpu_ctx, t, imgs, far, (2, 2), "rggb", (64, 64, 64, 64), tag="far", floats=("f16",), display=(("u8", "chw"),), yuv=("p010",))


def test_35_frames_cross_a_piece_with_per_frame_meshes_and_colours(gpu_ctx):
    rng = np.random.default_rng(9)
    n, h, w, size = 35, 16, 24, (10, 14)
    imgs = [_mosaic(rng, h, w, 12) for _ in range(n)]
    t = _dev16(np.stack(imgs))
    gain = np.stack([np.array([1.0 + 0.03 * i, 1.0, 2.0 - 0.02 * i], np.float32) for i in range(n)])
    matrix = np.stack([SRGBISH * np.float32(1.0 - 0.005 * i) for i in range(n)])
    maps = np.asarray([[65536 + 300 * (i - 17), 400 * (i - 17), 256 * 3 + 7 * i, -350 * (i - 17), 65536 - 200 * (i - 17), 256 * 5 + 11 * i] for i in range(n)])
    meshes = M.affine_mesh(maps, size)
    assert len({m.tobytes() for m in meshes}) == n
    one = dict(floats=("f16",), display=(("u8", "hwc"),), yuv=("nv12",))
    _check_families(gpu_ctx, t, imgs, meshes, size, "bggr", (60, 61, 62, 63), gain=gain, matrix=matrix, tag="per frame", **one)
    _check_families(gpu_ctx, t, imgs, meshes, size, "bggr", (60, 61, 62, 63), tag="meshes per frame, one colour", floats=("f32",), display=(), yuv=())
    _check_families(gpu_ctx, t, imgs, meshes[3:4], size, "bggr", (60, 61, 62, 63), gain=gain, matrix=matrix, tag="one mesh, colours per frame",
                    floats=("f32",), display=(), yuv=())


def test_strided_input_misaligned_out_sentinels(gpu_ctx):
    rng = np.random.default_rng(8)
    n, h, w, pitch = 3, 36, 68, 83
    fstride = h * pitch + 29
    size, size2 = (27, 45), (26, 44)
    meshes = np.stack([M.distortion_mesh(h, w, size, radial=(1.0, -0.1 * (i + 1), 0.0, 0.0)) for i in range(n)])
    meshes2 = np.stack([M.distortion_mesh(h, w, size2, radial=(1.0, -0.1 * (i + 1), 0.0, 0.0)) for i in range(n)])
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
    kw = dict(algo="mesh", size=size, mesh=torch.from_numpy(meshes).to(DEV), white=16383.0, black=black, cfa="bggr", gain=(1.4, 1.0, 1.9), matrix=SRGBISH)
    kw2 = dict(kw, size=size2, mesh=torch.from_numpy(meshes2).to(DEV))
    o = _values(imgs, meshes, size, "cubic", black, "bggr", 16383.0, (1.4, 1.0, 1.9), SRGBISH)
    o2 = _values(imgs, meshes2, size2, "cubic", black, "bggr", 16383.0, (1.4, 1.0, 1.9), SRGBISH)
    coef = M.yuv_matrix("bt709", "limited", 8, IN_BITS)
    packed = gpu_ctx.demosaic(_dev16(np.stack(imgs)), dtype="f16", **kw)  # the 16-byte path beside it: the same frames on the grid
    cases = [("f16", torch.float16, (n, 3) + size, lambda out: gpu_ctx.demosaic(view, dtype="f16", out=out, **kw), lambda i: MR.float_bits(o[i], "f16")),
             ("u8", torch.uint8, (n,) + size + (3,), lambda out: gpu_ctx.demosaic_display(view, transfer=dl, out=out, **kw),
              lambda i: MR.display_from_o(o[i], lut, "u8", "hwc")),
             ("nv12", torch.uint8, (n, size2[0] * 3 // 2, size2[1]), lambda out: gpu_ctx.demosaic_yuv(view, transfer=dl, in_bits=IN_BITS, out=out, **kw2),
              lambda i: MR.yuv_from_o(o2[i], lut, "nv12", coef, IN_BITS))]
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
    assert np.array_equal(_bits(packed, torch.int16), np.stack([MR.float_bits(o[i], "f16") for i in range(n)]))


@pytest.mark.parametrize("entries", (256, 65536))
def test_lut_sizes_lds_and_global(gpu_ctx, frames3, entries):
    imgs, t = frames3
    mesh = M.distortion_mesh(H, WD, SIZE, radial=(0.9, 0.2, 0.0, 0.0))
    _check_families(gpu_ctx, t, imgs, mesh, SIZE, "grbg", (16, 16, 16, 16), 1023.0, lut=_rand_lut(np.random.default_rng(entries), entries), floats=(),
                    tag=entries)


def test_rejections_write_nothing_and_python_argument_rules(gpu_ctx, frames3):
    imgs, t = frames3
    n = len(imgs)
    lib = M.load()
    out = torch.full((n * 3 * SIZE[0] * SIZE[1] * 4,), SENT, dtype=torch.uint8, device=DEV)
    nodes = torch.from_numpy(MR.translation_mesh(SIZE, 2, 4)).to(DEV)
    p = M.RgbParams()
    p.algo, p.dtype, p.white = 7, 1, 4095.0
    col = (M.RgbColor * 1)()
    for i in range(3):
        col[0].gain[i] = 1.0
        col[0].m[4 * i] = 1.0

    def call(algo=7, reserved=0, nmesh=1, nodes_ptr=nodes.data_ptr(), nodes_bytes=nodes.numel() * 4, n=n, out_bytes=out.numel()):
        p.algo = algo
        m = M.Mesh()
        m.out_h, m.out_w, m.filter, m.reserved = SIZE[0], SIZE[1], 1, reserved
        rc = lib.mcraw_demosaic_mesh_batch(gpu_ctx._h, C.byref(p), C.byref(m), None, None, col, 1, C.c_void_p(nodes_ptr), nodes_bytes, nmesh,
                                           C.c_void_p(t.data_ptr()), WD, WD * H, WD, H, n, C.c_void_p(out.data_ptr()), out_bytes, None)
        return rc, lib.mcraw_last_error().decode()

    for kw in (dict(algo=5), dict(reserved=1), dict(nmesh=2), dict(nodes_ptr=nodes.data_ptr() + 4), dict(nodes_bytes=nodes.numel() * 4 - 1),
               dict(nmesh=n), dict(nodes_ptr=0), dict(out_bytes=out.numel() - 1)):
        rc, msg = call(**kw)
        assert rc < 0 and msg.startswith("mcraw_demosaic_mesh_batch: "), (kw, msg)
    assert call(n=0, nmesh=9)[0] == 0
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
    assert call()[0] == 0
    torch.cuda.synchronize()
    want = gpu_ctx.demosaic(t, algo="mhc", dtype="f32", white=4095.0)[:, :, 2:2 + SIZE[0], 4:4 + SIZE[1]].contiguous()
    assert torch.equal(out.view(torch.int32), want.view(torch.int32).reshape(-1))
    # Python
    kw = dict(dtype="f32", white=4095.0)
    mesh = MR.translation_mesh(SIZE, 2, 4)
    for algo, extra in (("mhc", {}), ("bin2", {}), ("ha", {}), ("area", dict(size=(20, 30))), ("resample", dict(size=SIZE)),
                        ("warp", dict(size=SIZE, affine=np.array(W.IDENTITY, dtype=np.int32)))):
        with pytest.raises(ValueError, match="mesh= belongs to algo='mesh'"):
            gpu_ctx.demosaic(t, algo=algo, mesh=mesh, **extra, **kw)
    with pytest.raises(ValueError, match="needs size"):
        gpu_ctx.demosaic(t, algo="mesh", mesh=mesh, **kw)
    with pytest.raises(ValueError, match="needs size"):
        gpu_ctx.demosaic_display(t, algo="mesh", size=SIZE, white=4095.0)
    with pytest.raises(ValueError, match="crop= and affine= do not go"):
        gpu_ctx.demosaic_yuv(t, algo="mesh", size=SIZE, mesh=mesh, crop=(0, 0, 40, 70), white=4095.0)
    with pytest.raises(ValueError, match="crop= and affine= do not go"):
        gpu_ctx.demosaic(t, algo="mesh", size=SIZE, mesh=mesh, affine=np.array(W.IDENTITY, dtype=np.int32), **kw)
    with pytest.raises(ValueError, match="filter must be"):
        gpu_ctx.demosaic(t, algo="mesh", size=SIZE, mesh=mesh, filter="lanczos", **kw)
    for bad in (mesh.astype(np.int64), mesh[:, :3], np.stack([mesh] * 2), mesh.astype(np.float32), torch.from_numpy(mesh).to(DEV)[:, :, :1],
                torch.from_numpy(np.stack([mesh] * 2)).to(DEV), torch.from_numpy(mesh).to(DEV).to(torch.int64),
                torch.from_numpy(np.stack([mesh] * 2)).to(DEV)[:, :, :, ::2]):
        with pytest.raises(ValueError, match="mesh"):
            gpu_ctx.demosaic(t, algo="mesh", size=SIZE, mesh=bad, **kw)
    one = gpu_ctx.demosaic(t[0], algo="mesh", size=SIZE, mesh=mesh, **kw)
    assert tuple(one.shape) == (3,) + SIZE and torch.equal(one.view(torch.int32), want[0].view(torch.int32))
    empty = gpu_ctx.demosaic(t[:0], algo="mesh", size=SIZE, mesh=mesh, **kw)
    assert tuple(empty.shape) == (0, 3) + SIZE


@pytest.mark.parametrize("typ", (7, 6))
def test_six_methods_with_a_stage_in_front(gpu_ctx, typ):
    rng = np.random.default_rng(typ)
    items = _frames(rng, [(64, 32)] * 3, typ)
    ins = [torch.from_numpy(buf).to(DEV) for buf, _ in items]
    size = (24, 48)
    meshes = torch.from_numpy(np.stack([M.distortion_mesh(32, 64, size, radial=(1.0, -0.05 * (i + 1), 0.0, 0.0)) for i in range(3)])).to(DEV)
    y, x = np.linspace(-1, 1, 13)[:, None], np.linspace(-1, 1, 17)[None, :]
    gm = M.gain_map(np.stack([1.0 + (s - 1.0) * (x * x + y * y) / 2 for s in (1.9, 1.4, 1.45, 2.3)]), "grbg")
    black = (64, 64, 64, 64)
    kw = dict(white=4095.0, black=black, cfa="grbg", gain=(1.9, 1.0, 1.5), matrix=SRGBISH, algo="mesh", size=size, mesh=meshes, filter="cubic")
    plain = _dev16(np.stack([want for _, want in items]))
    shaded = gpu_ctx.shade(plain, gm, black=black)
    assert not torch.equal(shaded.view(torch.int16), plain.view(torch.int16))
    for fmt in ("nv12", "p010"):
        a = gpu_ctx.decode_yuv(ins, 64, 32, typ, fmt=fmt, shading=gm, **kw)
        assert tuple(a.shape) == (3, 36, 48) and torch.equal(_as_int(a), _as_int(gpu_ctx.demosaic_yuv(shaded, fmt=fmt, **kw)))
        assert torch.equal(_as_int(a), _as_int(gpu_ctx.demosaic_yuv(plain, fmt=fmt, shading=gm, **kw)))
    a = gpu_ctx.decode_rgb(ins, 64, 32, typ, dtype="f16", shading=gm, **kw)
    assert torch.equal(a.view(torch.int16), gpu_ctx.demosaic(shaded, dtype="f16", **kw).view(torch.int16))
    assert torch.equal(a.view(torch.int16), gpu_ctx.demosaic(plain, dtype="f16", shading=gm, **kw).view(torch.int16))
    a = gpu_ctx.decode_display(ins, 64, 32, typ, shading=gm, **kw)
    assert torch.equal(a, gpu_ctx.demosaic_display(shaded, **kw)) and torch.equal(a, gpu_ctx.demosaic_display(plain, shading=gm, **kw))
    host = _np(shaded)
    _check_families(gpu_ctx, shaded, [host[i] for i in range(3)], meshes.cpu().numpy(), size, "grbg", black, gain=(1.9, 1.0, 1.5), floats=("f32",),
                    display=(), yuv=("nv12",))
