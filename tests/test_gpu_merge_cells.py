"""The merge that follows a position field (mcraw_merge_cells_batch, Context.merge(pos=<4-D>, cell=)) on the GPU: equal to the
numpy statement (_merge_cells_ref) bit for bit over partial cells and odd frames, for fields with even and odd components, with
shifts on and off the 16-byte grid in one launch, with shifts that leave a cell's tiles, and, for a constant field, equal to
merge(pos=) itself; views with an odd base and pitch; the build with tiles of 16 rows."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

import _merge_cells_ref as MC
import motioncam_decoder_amd as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
N = 5
# (W, H), cell: the estimator's small geometries.  The merge's tile is 256 x 32 samples (16 rows in the alt build).
GEOMS = (((600, 100), (32, 256)), ((601, 101), (32, 256)), ((1030, 130), (64, 512)), ((256, 32), (32, 256)), ((16, 8), (32, 256)))


def _dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).to(DEV).view(torch.uint16)


def _bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _inputs(geom):
    (W, H), cell = geom
    rng = np.random.default_rng(zlib.crc32(repr(geom).encode()))
    base = rng.integers(200, 3000, size=(H, W))
    imgs = np.clip(base[None] + rng.normal(0, 30, size=(N, H, W)), 0, 4095).astype(np.uint16)  # one scene, fresh noise per frame
    cy, cx = M.cell_grid(H, W, cell)
    return rng, imgs, cy, cx


def _field_a(rng, cy, cx):
    """Random even and odd components per cell."""
    return rng.integers(-9, 10, size=(N, cy, cx, 2)).astype(np.int16)


def _field_b(rng, cy, cx):
    """sx a multiple of 8 in the even cells and not in the odd ones, for every pair of frames: positions 16 t in the even cells
    and 16 t + 2 t in the odd ones (t >= 1 apart: 2 (t - b) is no multiple of 8 inside a window of 2)."""
    f = np.zeros((N, cy, cx, 2), np.int64)
    t = np.arange(N)[:, None, None]
    odd = ((np.arange(cy)[:, None] + np.arange(cx)[None, :]) & 1)[None]
    f[..., 1] = 16 * t + 2 * t * odd
    f[..., 0] = rng.integers(-3, 4, size=(N, cy, cx)) * 2
    return f.astype(np.int16)


def _field_c(rng, cy, cx, W, H):
    """Cells whose members are wholly off their tiles (a shift beyond the frame), cells that are partly off, cells at rest."""
    f = np.zeros((N, cy, cx, 2), np.int64)
    kind = rng.integers(0, 4, size=(cy, cx))
    kind.flat[0], kind.flat[-1] = 1, 2  # (both kinds occur whatever the draw)
    t = np.arange(N)[:, None, None]
    f[..., 1] = np.where(kind[None] == 1, 2 * W * t, np.where(kind[None] == 3, -(W // 2) * t, 0))
    f[..., 0] = np.where(kind[None] == 2, -2 * H * t, np.where(kind[None] == 3, (H // 2 + 3) * t, 0))
    return np.clip(f, -32768, 32767).astype(np.int16)


@pytest.mark.parametrize("geom", GEOMS)
def test_merge_cells_matches_reference(gpu_ctx, geom):
    (W, H), cell = geom
    rng, imgs, cy, cx = _inputs(geom)
    t = _dev16(imgs)
    lut, shift = M.noise_lut(S=2e-2, O=2e-3, black=64, white=4095)
    luts = np.stack([M.noise_lut(S=2e-2 * (1 + f), O=2e-3, black=64, white=4095)[0] for f in range(N)])
    whole = W * H <= 4096  # the smallest frames: every base, so the windows are clipped at both ends of the batch
    first, count = (0, N) if whole else (2, 1)
    fb = _field_b(rng, cy, cx)
    if cy * cx > 1 and W % 8 == 0:  # both staging paths in one launch, read off the field itself: for every base of the launch and each of its members ...
        assert t.data_ptr() % 16 == 0
        for b in range(first, first + count):
            for m in range(max(0, b - 2), min(N - 1, b + 2) + 1):
                if m != b:
                    sx = (fb[m, :, :, 1].astype(np.int64) - fb[b, :, :, 1]) & ~1
                    assert (sx % 8 == 0).any() and (sx % 8 != 0).any(), (b, m)  # ... some tiles take 16-byte loads, some cannot
    for field, support, table, amount in ((_field_a(rng, cy, cx), 1, lut, 1.0), (fb, 0, luts, 100 / 256), (_field_c(rng, cy, cx, W, H), 1, luts, 1.0),
                                          (_field_a(rng, cy, cx), 0, lut, 100 / 256)):
        got = gpu_ctx.merge(t, table, shift, 2, 2, first, count, support=support, amount=amount, pos=torch.from_numpy(field).to(DEV), cell=cell)
        torch.cuda.synchronize()
        want = MC.merge(imgs, table, shift, field, cell, 2, 2, first, count, support, int(round(amount * 256)))
        assert np.array_equal(_bits(got), want), (support, amount, np.argwhere(_bits(got) != want)[:4].tolist())
    assert np.array_equal(_bits(t), imgs), "the input was written"
    # D: a constant field is merge(pos=), on the GPU, bit for bit; a host array works like a tensor
    pos = rng.integers(-9, 10, size=(N, 2)).astype(np.int16)
    const = np.broadcast_to(pos[:, None, None, :], (N, cy, cx, 2)).copy()
    for support in (0, 1):
        a = gpu_ctx.merge(t, lut, shift, support=support, pos=const, cell=cell)
        b = gpu_ctx.merge(t, lut, shift, support=support, pos=pos)
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), support


def test_stack_and_python_checks(gpu_ctx):
    (W, H), cell = GEOMS[0]
    rng, imgs, cy, cx = _inputs(GEOMS[0])
    t = _dev16(imgs)
    lut, shift = M.noise_lut(S=2e-2, O=2e-3, black=64, white=4095)
    field = _field_a(rng, cy, cx)
    st = gpu_ctx.stack(t, lut, shift, ref=2, pos=field, cell=cell)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(st), MC.merge(imgs, lut, shift, field, cell, 2, 2, 2, 1)[0])
    as_list = gpu_ctx.stack(t, lut, shift, ref=2, pos=field.tolist(), cell=cell)  # a nested list is a host array too
    torch.cuda.synchronize()
    assert torch.equal(as_list.view(torch.int16), st.view(torch.int16))
    for kw in (dict(pos=field), dict(cell=cell), dict(pos=field[:, :, :2], cell=cell), dict(pos=field, cell=(16, 256)), dict(pos=field, cell=(64, 256)),
               dict(pos=field.astype(np.float32), cell=cell), dict(pos=np.zeros((N, 2), np.int16), cell=cell),
               dict(pos=torch.from_numpy(field).to(DEV)[:, :, :, :1], cell=cell)):
        with pytest.raises(ValueError):
            gpu_ctx.merge(t, lut, shift, **kw)


def test_pitched_offset_views(gpu_ctx):
    """An input at an odd element with an odd pitch, an output likewise: no 16-byte path anywhere."""
    (W, H), cell = GEOMS[1]
    rng, imgs, cy, cx = _inputs(GEOMS[1])
    lut, shift = M.noise_lut(S=2e-2, O=2e-3, black=64, white=4095)
    field = _field_b(rng, cy, cx)
    pitch, fs = W + 6, H * (W + 6) + 11
    ibase = torch.zeros(N * fs + 64, dtype=torch.int16, device=DEV)
    src = torch.as_strided(ibase, (N, H, W), (fs, pitch, 1), 3).view(torch.uint16)
    src.view(torch.int16).copy_(torch.from_numpy(imgs.view(np.int16)).to(DEV))
    obase = torch.full((2 * fs + 64,), 0x5A5A, dtype=torch.int16, device=DEV)
    out = torch.as_strided(obase, (2, H, W), (fs, pitch, 1), 5).view(torch.uint16)
    gpu_ctx.merge(src, lut, shift, 2, 2, 1, 2, pos=field, cell=cell, out=out)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out), MC.merge(imgs, lut, shift, field, cell, 2, 2, 1, 2))
    mask = torch.ones_like(obase, dtype=torch.bool)
    torch.as_strided(mask, (2, H, W), (fs, pitch, 1), 5).fill_(False)
    assert (obase[mask] == 0x5A5A).all(), "something outside the output's samples was written"


def test_tiles_of_16_rows(gpu_ctx):
    """The alt build (MCRAW_MERGE_TH=16) through tools/altlib.py: two tiles per 32 rows of a cell, the same result."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from altlib import AltLib
    from motioncam_decoder_amd import build as B
    (W, H), cell = GEOMS[0]
    rng, imgs, cy, cx = _inputs(GEOMS[0])
    t = _dev16(imgs)
    lut, shift = M.noise_lut(S=2e-2, O=2e-3, black=64, white=4095)
    field = _field_a(rng, cy, cx)
    alt = AltLib(B.build_merge_alt())
    try:
        out = torch.empty_like(t)
        s = torch.cuda.current_stream(DEV)
        alt.merge_cells(t, out, s, torch.from_numpy(lut).to(DEV), shift, 2, 1, torch.from_numpy(field).to(DEV), cell)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out), MC.merge(imgs, lut, shift, field, cell, 2, 2))
    finally:
        alt.close()
