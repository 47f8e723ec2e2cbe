"""The position field's estimator (mcraw_align_cells_batch, Context.align_cells) on the GPU: pos and sad equal the numpy
statement of the contract (_align_cells_ref) bit for bit over cells that are partial, cut by an odd frame, one workgroup or
several, and empty at a level; the centres from align(), from hand-made positions and from nothing; views with a pitch and an odd
base; and decode_merge(align={"cell": ...}) equals the three separate calls."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import _align_cells_ref as CR
import _merge_cells_ref as MC
import motioncam_decoder_amd as M
from _cells_scenes import halves_field, halves_frames

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BLACK = (64, 64, 64, 64)
N = 4
# (W, H), cell.  A cell of 256 columns is one piece of the SAD kernel's 128 x 32 pixels at level 0, one of 512 is two (64-bit atomics).
GEOMS = (((600, 100), (32, 256)),    # three cell columns, the last partial; four cell rows, the last 4 rows tall
         ((601, 101), (32, 256)),    # ... and an odd trailing row and column
         ((1030, 130), (64, 512)),   # cells of two pieces
         ((256, 32), (32, 256)),     # one cell
         ((16, 8), (32, 256)),       # planes of 4 x 8, 2 x 4 and 1 x 2 pixels
         ((16, 6), (32, 256)))       # ... and a cell that is empty at level 2 (3 x 8, 1 x 4, 0 x 2)
# levels, radius, ref, the centres, sad: every levels x radius once, the chain and the anchor, the three kinds of centres
COMBOS = ((3, 2, None, "none", True), (3, 4, 2, "align", True), (2, 1, None, "hand", False), (1, 4, None, "hand", True),
          (1, 1, 2, "none", True), (2, 2, 2, "hand", True), (3, 1, None, "align", True), (2, 4, None, "none", False),
          (1, 2, None, "align", True))


def _dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).to(DEV).view(torch.uint16)


def _contents(W, H, seed):
    halves = halves_frames(seed, H, W, 9, n=N, reach=8, noise=8.0, seam=min(256, W // 2))[0]
    flat = np.stack([np.full((H, W), v, np.uint16) for v in (1000, 1300, 200, 1000)])
    return (("halves", halves), ("flat", flat))


def _hand(W, H):
    """Odd components, and steps larger than the frame."""
    return np.array([[0, 0], [5, -7], [-2 * H - 101, 9], [3, 2 * W + 33]], np.int16)


def _check(got, want, sad, what):
    pos, sums = got if sad else (got, None)
    assert pos.dtype == torch.int16 and tuple(pos.shape) == want[0].shape and pos.is_contiguous(), what
    gp = pos.cpu().numpy()
    assert np.array_equal(gp, want[0]), (what, gp.tolist(), want[0].tolist())
    if sad:
        assert sums.dtype == torch.int64 and tuple(sums.shape) == want[1].shape, what
        assert np.array_equal(sums.cpu().numpy(), want[1].astype(np.int64)), (what, sums.cpu().tolist(), want[1].tolist())


@pytest.mark.parametrize("geom", GEOMS)
def test_align_cells_matches_reference(gpu_ctx, geom):
    (W, H), cell = geom
    for name, imgs in _contents(W, H, zlib.crc32(repr(geom).encode())):
        t = _dev16(imgs)
        centres = {"none": None, "hand": _hand(W, H), "align": gpu_ctx.align(t, black=BLACK, levels=1, radius=1).cpu().numpy()}
        for levels, radius, ref, kind, sad in COMBOS:
            g = centres[kind]
            got = gpu_ctx.align_cells(t, pos=None if g is None else torch.from_numpy(g).to(DEV), black=BLACK, cell=cell, levels=levels,
                                      radius=radius, ref=ref, sad=sad)
            torch.cuda.synchronize()
            want = CR.align_cells(imgs, BLACK, cell, levels, radius, -1 if ref is None else ref, g)
            _check(got, want, sad, (name, levels, radius, ref, kind))
            if name == "flat" and ref is None:  # every candidate ties: the centres are kept, level by level
                c = np.zeros((N, 2), np.int64) if g is None else (np.diff(g.astype(np.int64), axis=0, prepend=g[:1].astype(np.int64)) >> 1) >> (levels - 1)
                assert np.array_equal(want[0].astype(np.int64)[:, 0, 0], np.clip(np.cumsum(2 * (c << (levels - 1)), axis=0), -32768, 32767))
        assert np.array_equal(t.view(torch.int16).cpu().numpy().view(np.uint16), imgs), "the input was written"
        for m in (1, 2):  # n = 1 writes zeros; n = 2 is one pair
            got = gpu_ctx.align_cells(t[:m], pos=centres["hand"][:m], black=BLACK, cell=cell, sad=True)
            torch.cuda.synchronize()
            _check(got, CR.align_cells(imgs[:m], BLACK, cell, 3, 2, -1, centres["hand"][:m]), True, (name, "n", m))
            assert m == 2 or (not got[0].cpu().numpy().any() and not got[1].cpu().numpy().any())
    empty = gpu_ctx.align_cells(t[:0], cell=cell, sad=True)  # n == 0
    cy, cx = M.cell_grid(H, W, cell)
    assert tuple(empty[0].shape) == (0, cy, cx, 2) and tuple(empty[1].shape) == (0, cy, cx)


def test_local_motion_is_found(gpu_ctx):
    """The two halves of the CPU test's scene, scaled down to 3 x 4 cells of 32 x 256 with noise: the cell columns off the seam
    follow their half exactly, about no centre and about align()'s."""
    H, W, cell = 96, 1024, (32, 256)
    frames, off = halves_frames(11, H, W, 19, n=N, reach=8, noise=4.0)
    want = halves_field(off, 3, 4, 2)
    t = _dev16(frames)
    for gpos in (None, gpu_ctx.align(t, black=BLACK, levels=2, radius=2)):
        pos = gpu_ctx.align_cells(t, pos=gpos, black=BLACK, cell=cell, levels=2, radius=4)  # (within reach of the halves' steps about either centre)
        torch.cuda.synchronize()
        g = None if gpos is None else gpos.cpu().numpy()
        assert np.array_equal(pos.cpu().numpy(), CR.align_cells(frames, BLACK, cell, 2, 4, -1, g)[0])
        assert np.array_equal(pos.cpu().numpy()[:, :, [0, 3]].astype(np.int64), want[:, :, [0, 3]])


def test_cell_sums_beyond_32_bits(gpu_ctx):
    """One cell of 8 x 4 pieces whose candidates each sum to 256 * 512 * 65535 > 2^32: the 32 pieces' 64-bit atomics carry (a piece
    alone adds 4096 * 65535 < 2^32).  The cell counterpart of test_gpu_align.py's test_sums_beyond_32_bits."""
    H, W, cell = 512, 1024, (512, 1024)
    imgs = np.stack([np.zeros((H, W), np.uint16), np.full((H, W), 65535, np.uint16)])
    want = CR.align_cells(imgs, (0, 0, 0, 0), cell, 1, 1)
    assert int(want[1][1, 0, 0]) == 256 * 512 * 65535 > 1 << 32 and not want[0].any()
    got = gpu_ctx.align_cells(_dev16(imgs), black=(0, 0, 0, 0), cell=cell, levels=1, radius=1, sad=True)
    torch.cuda.synchronize()
    _check(got, want, True, "beyond 32 bits")


# (W, H, pitch, frame slack, offset in samples): an odd base off the dword grid, the 16-byte path, an odd pitch
VIEWS = ((600, 100, 613, 29, 1), (600, 100, 608, 8, 8), (601, 101, 601, 0, 3))


@pytest.mark.parametrize("view", VIEWS)
def test_pitched_strided_offset_views(gpu_ctx, view):
    W, H, pitch, slack, off = view
    rng = np.random.default_rng(zlib.crc32(repr(view).encode()))
    fs = H * pitch + slack
    imgs = halves_frames(W + H, H, W, 9, n=N, reach=8, noise=8.0, seam=256)[0]
    base = torch.from_numpy(rng.integers(0, 1 << 16, size=N * fs + 64, dtype=np.uint16).view(np.int16)).to(DEV)
    src = torch.as_strided(base, (N, H, W), (fs, pitch, 1), off).view(torch.uint16)
    src.view(torch.int16).copy_(torch.from_numpy(imgs.view(np.int16)).to(DEV))
    before = base.clone()
    for ref in (None, 3):
        got = gpu_ctx.align_cells(src, pos=_hand(W, H), black=BLACK, cell=(32, 256), ref=ref, sad=True)
        torch.cuda.synchronize()
        _check(got, CR.align_cells(imgs, BLACK, (32, 256), 3, 2, -1 if ref is None else ref, _hand(W, H)), True, ref)
    assert torch.equal(base, before), "the input was written"


def test_a_call_writes_its_outputs_only_and_python_checks(gpu_ctx):
    lib = M.load()
    W, H, cell = 600, 100, (32, 256)
    SENT = 0x5A
    buf = torch.full((1 << 20,), SENT, dtype=torch.uint8, device=DEV)
    base = buf.data_ptr()
    assert base % 256 == 0
    ip, pp, sp, kp = base, base + (1 << 19), base + (1 << 19) + 4096, base + (1 << 19) + 8192
    need = lib.mcraw_align_cells_work_bytes(W, H, N, 3, 2, *cell)
    assert 0 < need <= (1 << 19) - 8192 and 2 * N * W * H <= 1 << 19
    imgs = halves_frames(5, H, W, 9, n=N, reach=8, noise=8.0, seam=256)[0]
    buf[:2 * N * W * H].copy_(torch.from_numpy(imgs.reshape(-1).view(np.uint8)).to(DEV))
    a = M.AlignCells()
    a.levels, a.radius, a.ref, a.reserved, a.cell_h, a.cell_w = 3, 2, -1, 0, *cell
    for i in range(4):
        a.black[i] = BLACK[i]
    a.gpos, a.pos, a.sad, a.work, a.work_bytes = None, pp, sp, kp, need
    serial = gpu_ctx.last_serial()
    assert lib.mcraw_align_cells_batch(gpu_ctx._h, C.byref(a), C.c_void_p(ip), W, W * H, W, H, N, None) == 0, lib.mcraw_last_error()
    torch.cuda.synchronize()
    gpu_ctx.synchronize()
    got = buf.cpu().numpy()
    want = CR.align_cells(imgs, BLACK, cell, 3, 2)
    np_, ns = N * 12 * 4, N * 12 * 8
    assert np.array_equal(got[1 << 19:(1 << 19) + np_].view(np.int16).reshape(N, 4, 3, 2), want[0])
    assert np.array_equal(got[(1 << 19) + 4096:(1 << 19) + 4096 + ns].view(np.uint64).reshape(N, 4, 3), want[1])
    assert (got[2 * N * W * H:1 << 19] == SENT).all() and (got[(1 << 19) + np_:(1 << 19) + 4096] == SENT).all()
    assert (got[(1 << 19) + 4096 + ns:(1 << 19) + 8192] == SENT).all() and (got[(1 << 19) + 8192 + need:] == SENT).all()
    assert np.array_equal(got[:2 * N * W * H].view(np.uint16).reshape(N, H, W), imgs)
    a.levels = 4  # a rejected call next to it writes nothing
    buf[1 << 19:].fill_(SENT)
    assert lib.mcraw_align_cells_batch(gpu_ctx._h, C.byref(a), C.c_void_p(ip), W, W * H, W, H, N, None) < 0
    assert lib.mcraw_last_error().decode().startswith("mcraw_align_cells_batch: ")
    torch.cuda.synchronize()
    assert (buf[1 << 19:].cpu().numpy() == SENT).all()
    assert gpu_ctx.last_serial() == serial and gpu_ctx.errors(reset=False) == 0
    # Python: what the wrapper checks itself
    t = torch.zeros((3, 64, 300), dtype=torch.int16, device=DEV).view(torch.uint16)
    for kw in (dict(levels=0), dict(levels=4), dict(levels=1.5), dict(radius=0), dict(radius=5), dict(ref=3), dict(ref=-1), dict(cell=(16, 256)),
               dict(cell=(32, 128)), dict(cell=64), dict(black=(1, 2, 3)), dict(black=-1), dict(pos=np.zeros((2, 2), np.int16)),
               dict(pos=np.zeros((3, 2))), dict(pos=torch.zeros((3, 2), dtype=torch.int32, device=DEV))):
        with pytest.raises(ValueError):
            gpu_ctx.align_cells(t, **kw)
    for bad in (t.view(torch.int16), t[0], t.cpu()):
        with pytest.raises(ValueError):
            gpu_ctx.align_cells(bad)
    ok = gpu_ctx.align_cells(t, black=64, levels=np.int64(1), radius=np.int32(2), ref=np.int64(1), cell=(np.int64(32), 256))
    torch.cuda.synchronize()
    assert tuple(ok.shape) == (3, 2, 2, 2) and not ok.cpu().numpy().any()


def test_decode_merge_with_cells(gpu_ctx):
    """decode_merge(align={"cell": ...}) is the decode, align(), align_cells() about its result and the merge with the field."""
    import _align_ref as R
    import _libs as L
    w, h, n, levels, radius, cell = 512, 96, 4, 2, 2, (32, 256)
    scene = L.natural_image_np(w + 64, h + 64, 12, 12.0, 9)
    offs = (((16, 16), (16, 16)), ((20, 10), (18, 14)), ((14, 22), (20, 12)), ((18, 18), (12, 20)))  # the halves move apart
    imgs = np.stack([np.concatenate([scene[ly:ly + h, lx:lx + w // 2], scene[ry:ry + h, rx + w // 2:rx + w]], axis=1) for (ly, lx), (ry, rx) in offs])
    ins = [torch.from_numpy(L.encode7(f)).to(DEV) for f in imgs]
    lut, shift = M.noise_lut(S=2e-4, O=2e-6, black=64, white=4095)
    gpos = R.align(imgs, BLACK, levels, radius)[0]
    field = CR.align_cells(imgs, BLACK, cell, 3, 1, -1, gpos)[0]
    assert (field[:, :, 0] != field[:, :, 1]).any()
    try:
        got = gpu_ctx.decode_merge(ins, w, h, 7, lut=lut, shift=shift, before=1, after=2,
                                   align=dict(black=BLACK, levels=levels, radius=radius, cell=cell, cell_radius=1))
        t = _dev16(imgs)
        g = gpu_ctx.align(t, black=BLACK, levels=levels, radius=radius)
        f = gpu_ctx.align_cells(t, pos=g, black=BLACK, cell=cell, levels=3, radius=1)
        three = gpu_ctx.merge(t, lut, shift, before=1, after=2, pos=f, cell=cell)
        torch.cuda.synchronize()
        assert np.array_equal(f.cpu().numpy(), field)
        assert torch.equal(got.view(torch.int16), three.view(torch.int16))
        assert np.array_equal(got.view(torch.int16).cpu().numpy().view(np.uint16), MC.merge(imgs, lut, shift, field, cell, 1, 2))
        for bad in (dict(align=dict(cell=cell), cell=cell), dict(align=dict(cell_levels=2)), dict(align=dict(cell=(16, 256)))):
            with pytest.raises(ValueError):
                gpu_ctx.decode_merge(ins, w, h, 7, lut=lut, shift=shift, **bad)
    finally:
        gpu_ctx.set_post()
    assert gpu_ctx.errors() == 0
