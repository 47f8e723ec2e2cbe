"""Per-frame global shifts of mosaics (mcraw_align_batch) without a GPU: the ABI's symbols and struct, the numpy statement of the
contract (_align_ref) against a scalar one written straight from the header, the consequences the contract names, the recovery of
known shifts of a textured scene, the sign convention against the merge's, and what the Python layer checks itself."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _align_ref as R
from _align_scenes import clamp_frames, scene_frames
import _merge_ref as MR
import motioncam_decoder_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (H, W), levels, radius, blur: the recovery scenes (the texture is coarser than the coarsest level's pixel: k >= 2^(levels + 1) + 1)
SCENES = (((24, 24), 1, 2, 9), ((40, 48), 2, 2, 9), ((72, 136), 3, 2, 17), ((96, 200), 3, 2, 17), ((160, 192), 3, 2, 17),
          ((256, 256), 4, 2, 33))
BLACK = (64, 64, 64, 64)


def _hdr():
    return open(os.path.join(ROOT, "include", "mcraw_hip.h")).read()


def test_align_symbols_exported_and_listed():
    hdr = _hdr()
    lib = M.load()
    for sym in ("mcraw_align_batch", "mcraw_align_work_bytes"):
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
        assert sym in M.ABI_SYMBOLS and hasattr(lib, sym), sym
    assert re.search(r"#define MCRAW_K_COUNT\s+11\b", hdr)
    assert "Align" in M.__all__ and "align_window" in M.__all__
    block = hdr[hdr.index("the frames' global positions"):hdr.index("} mcraw_align;")]
    for line in ("G0[y][x] = min((sum over the 4 samples of quad (y, x) of max(s - black[p], 0) + 2) >> 2, 65535)",
                 "p = (row & 1) * 2 + (col & 1)", "G(l+1)[y][x] = (the 4 samples of G(l) in quad (y, x), summed, + 2) >> 2",
                 "B(levels - 1) = radius", "B(l) = 2 * B(l + 1) + 1",
                 "SAD_l(dy, dx) = sum over B(l) <= y < h(l) - B(l), B(l) <= x < w(l) - B(l) of |G_l[t][y + dy][x + dx] - G_l[b][y][x]|",
                 "key = (SAD, ddy * ddy + ddx * ddx, ddy, ddx)", "pos[t] = pos[t - 1] + 2 * d(t|t - 1)", "pos[t] = 2 * d(t|ref)",
                 "in[t][y + 2 dy][x + 2 dx] looks like in[b][y][x]", "clamped to -32768 .. 32767",
                 "Differences across a clamped entry are", "(h0 - 2 * B(0)) * (w0 - 2 * B(0))"):
        assert line in block, line
    for word in ("rotation", "region of interest", "gyro", "tile-wise"):  # what the stage does not do is said
        assert word in block, word


def test_align_struct_layout():
    names = ("levels", "radius", "ref", "reserved", "black", "pos", "sad", "work", "work_bytes")
    assert C.sizeof(M.Align) == 56
    assert [getattr(M.Align, f).offset for f in names] == [0, 4, 8, 12, 16, 24, 32, 40, 48]
    m = re.search(r"\}\s*mcraw_align;\s*/\*\s*sizeof (\d+); radius (\d+), ref (\d+), reserved (\d+), black (\d+), pos (\d+), sad (\d+), "
                  r"work (\d+), work_bytes (\d+)", _hdr())
    assert m and [int(v) for v in m.groups()] == [56, 4, 8, 12, 16, 24, 32, 40, 48]


def test_work_bytes():
    wb = M.load().mcraw_align_work_bytes
    assert wb(3840, 2160, 240, 4, 4) > 0
    small = wb(6, 6, 1, 1, 1)
    assert small > 0 and wb(6, 6, 2, 1, 1) >= small
    # at least the pyramid (rows of whole 16-byte pieces) and the candidates' 64-bit sums
    assert wb(3840, 2160, 240, 4, 4) >= 240 * (2 * (1080 * 1920 + 540 * 960 + 270 * 480 + 135 * 240) + 8 * (81 + 27))
    for bad in ((6, 6, 1, 0, 1), (6, 6, 1, 7, 1), (6, 6, 1, 1, 0), (6, 6, 1, 1, 9), (5, 6, 1, 1, 1), (6, 5, 1, 1, 1), (0, 6, 1, 1, 1),
                (6, 65537, 1, 1, 1), (6, 6, 0, 1, 1), (6, 6, -1, 1, 1), (20, 20, 2, 2, 2)):
        assert wb(*bad) == 0, bad


def _scalar(imgs, black, levels, radius, ref):
    """The header's statement, one pixel at a time, in Python integers."""
    n, H, W = imgs.shape

    def plane0(f):
        return [[min((sum(max(int(imgs[f, 2 * y + r, 2 * x + c]) - black[r * 2 + c], 0) for r in (0, 1) for c in (0, 1)) + 2) >> 2, 65535)
                 for x in range(W // 2)] for y in range(H // 2)]

    def half(g):
        return [[(g[2 * y][2 * x] + g[2 * y][2 * x + 1] + g[2 * y + 1][2 * x] + g[2 * y + 1][2 * x + 1] + 2) >> 2
                 for x in range(len(g[0]) // 2)] for y in range(len(g) // 2)]

    pyr = []
    for f in range(n):
        p = [plane0(f)]
        for _ in range(levels - 1):
            p.append(half(p[-1]))
        pyr.append(p)
    B = [0] * levels
    B[levels - 1] = radius
    for l in range(levels - 2, -1, -1):
        B[l] = 2 * B[l + 1] + 1

    def d_of(t, b):
        cy = cx = 0
        for l in range(levels - 1, -1, -1):
            gb, gt = pyr[b][l], pyr[t][l]
            h, w = len(gb), len(gb[0])
            assert h - 2 * B[l] >= 1 and w - 2 * B[l] >= 1
            rad = radius if l == levels - 1 else 1
            if l != levels - 1:
                cy, cx = 2 * cy, 2 * cx
            best = None
            for ddy in range(-rad, rad + 1):
                for ddx in range(-rad, rad + 1):
                    s = sum(abs(gt[y + cy + ddy][x + cx + ddx] - gb[y][x]) for y in range(B[l], h - B[l]) for x in range(B[l], w - B[l]))
                    key = (s, ddy * ddy + ddx * ddx, ddy, ddx)
                    if best is None or key < best:
                        best = key
            cy, cx = cy + best[2], cx + best[3]
        return cy, cx, best[0]

    pos, sad = [[0, 0] for _ in range(n)], [0] * n
    for t in range(n):
        if ref < 0 and t > 0:
            dy, dx, sad[t] = d_of(t, t - 1)
            pos[t] = [pos[t - 1][0] + 2 * dy, pos[t - 1][1] + 2 * dx]
        elif ref >= 0 and t != ref:
            dy, dx, sad[t] = d_of(t, ref)
            pos[t] = [2 * dy, 2 * dx]
    return np.clip(np.array(pos), -32768, 32767).astype(np.int16), np.array(sad, np.uint64)


SMALL = (((6, 6), 1, 1), ((7, 9), 1, 1), ((24, 24), 1, 2), ((40, 48), 2, 2), ((25, 31), 2, 1), ((72, 136), 3, 2))


@pytest.mark.parametrize("case", SMALL)
def test_numpy_statement_equals_the_scalar_one(case):
    (H, W), levels, radius = case
    rng = np.random.default_rng(H * 977 + W)
    n = 3
    contents = [rng.integers(0, 1 << 16, size=(n, H, W), dtype=np.uint16),
                (rng.integers(0, 8, size=(n, H, W)) * 100).astype(np.uint16),  # few values: ties between candidates
                scene_frames(H + W, H, W, levels, radius, 9, n)[0]]
    for imgs in contents:
        for black in ((0, 0, 0, 0), (64, 60, 70, 65535)):
            for ref in (-1, 0, 1, 2):
                got = R.align(imgs, black, levels, radius, ref)
                want = _scalar(imgs, black, levels, radius, ref)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (black, ref)


def test_consequences_of_the_contract():
    rng = np.random.default_rng(4)
    for (H, W), levels, radius in SMALL + (((160, 192), 3, 2),):
        wh, ww = M.align_window(H, W, levels, radius)
        img = rng.integers(0, 1 << 16, size=(H, W), dtype=np.uint16)
        # identical frames: all zeros, sad 0
        pos, sad = R.align(np.stack([img] * 3), (0, 0, 0, 0), levels, radius)
        assert not pos.any() and not sad.any()
        # flat frames of different levels: every candidate ties, the key picks (0, 0); sad = |difference| * window pixels
        flat = np.stack([np.full((H, W), v, np.uint16) for v in (1000, 1300, 200)])
        for ref, diffs in ((-1, (0, 300, 1100)), (1, (300, 0, 1100))):
            pos, sad = R.align(flat, (0, 0, 0, 0), levels, radius, ref)
            assert not pos.any() and sad.tolist() == [d * wh * ww for d in diffs], (H, W, ref)
        # n = 1
        pos, sad = R.align(img[None], (0, 0, 0, 0), levels, radius)
        assert pos.tolist() == [[0, 0]] and sad.tolist() == [0]
        # odd sizes equal the even crop
        noisy = rng.integers(0, 4096, size=(3, H | 1, W | 1), dtype=np.uint16)
        a, b = R.align(noisy, BLACK, levels, radius), R.align(noisy[:, :(H | 1) - 1, :(W | 1) - 1], BLACK, levels, radius)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        # black above every sample: the planes are 0
        pos, sad = R.align(noisy, (4096,) * 4, levels, radius)
        assert not pos.any() and not sad.any()
    with pytest.raises(ValueError):
        R.align(np.zeros((2, 5, 6), np.uint16), levels=1, radius=1)
    with pytest.raises(ValueError):
        R.align(np.zeros((2, 20, 20), np.uint16), levels=2, radius=2)
    assert R.bounds(4, 4) == [39, 19, 9, 4] and R.bounds(6, 8) == [287, 143, 71, 35, 17, 8] and R.bounds(1, 3) == [3]


def test_the_clamp():
    # the accumulation itself: 2100 steps of 8 quads leave int16 on the way, in int32 they do not wrap
    d = np.tile(np.array([[8, -8]]), (2100, 1))
    pos = R.positions(d)
    t = np.arange(2100)
    assert pos.dtype == np.int16 and pos.shape == (2100, 2)
    assert np.array_equal(pos[:, 0], np.minimum(16 * t, 32767)) and np.array_equal(pos[:, 1], np.maximum(-16 * t, -32768))
    assert pos[-1].tolist() == [32767, -32768] and pos[2047].tolist() == [32752, -32752] and pos[2048].tolist() == [32767, -32768]
    assert R.positions(d, ref=3)[3].tolist() == [0, 0] and R.positions(d, ref=3)[0].tolist() == [16, -16]
    assert R.positions(np.array([[20000, -20000], [1, 1]]), ref=1).tolist() == [[32767, -32768], [0, 0]]
    # and driven through the search: a strip that moves 16 samples per frame under a 40 x 40 crop, levels 1, radius 8
    frames, off = clamp_frames(40)
    pos, sad = R.align(frames, BLACK, 1, 8)
    assert np.array_equal(pos[:, 1], -16 * np.arange(40)) and not pos[:, 0].any() and not sad.any()


@pytest.mark.parametrize("scene", SCENES)
def test_known_shifts_are_recovered(scene):
    (H, W), levels, radius, k = scene
    assert k >= 2 ** (levels + 1) + 1
    for seed in (1, 2):
        frames, off = scene_frames(1000 * seed + H + W, H, W, levels, radius, k)
        pos, sad = R.align(frames, BLACK, levels, radius)
        assert np.array_equal(np.diff(pos.astype(np.int64), axis=0), off[:-1] - off[1:]), (seed, pos.tolist(), off.tolist())
        assert sad[0] == 0 and (sad[1:] > 0).all()
        # the anchor form: every frame against frame 2
        pos, _ = R.align(frames, BLACK, levels, radius, ref=2)
        B0 = R.bounds(levels, radius)[0]
        for t in range(len(frames)):
            if np.abs(off[2] - off[t]).max() <= 2 * B0:  # within reach of one search
                assert np.array_equal(pos[t], off[2] - off[t]), (seed, t)


def test_the_sign_is_the_merges():
    """Noise-free crops, positions from the stage, the plain mean of the window (the all-0 table): every member is read where it
    shows what the base shows, so the mean is the base frame; with the positions negated it is not."""
    H, W, levels, radius = 96, 200, 3, 2
    frames, off = scene_frames(5, H, W, levels, radius, 17, noise=0.0)
    pos, sad = R.align(frames, BLACK, levels, radius)
    assert np.array_equal(np.diff(pos.astype(np.int64), axis=0), off[:-1] - off[1:]) and not sad.any()
    zero = np.zeros((4, 64), np.uint16)
    m = int(np.abs(pos.astype(np.int64) - pos[2]).max())
    assert 0 < m < min(H, W) // 2
    out = MR.merge(frames, zero, 10, 2, 2, 2, 1, support=0, pos=pos)[0]
    assert np.array_equal(out[m:H - m, m:W - m], frames[2][m:H - m, m:W - m])
    wrong = MR.merge(frames, zero, 10, 2, 2, 2, 1, support=0, pos=-pos.astype(np.int64))[0]
    assert not np.array_equal(wrong[m:H - m, m:W - m], frames[2][m:H - m, m:W - m])


def test_what_the_python_layer_checks_itself():
    assert M.align_window(2160, 3840) == (1080 - 78, 1920 - 78)
    assert M.align_window(6, 6, 1, 1) == (1, 1) and M.align_window(7, 9, 1, 1) == (1, 2)
    assert M.align_window(256, 256, levels=4, radius=2) == (128 - 46, 128 - 46)
    for kw in (dict(levels=0), dict(levels=7), dict(levels=2.5), dict(levels=True), dict(radius=0), dict(radius=9), dict(radius=-1),
               dict(radius=1.5)):
        with pytest.raises(ValueError):
            M.align_window(2160, 3840, **kw)
    for h, w, levels, radius in ((5, 6, 1, 1), (6, 5, 1, 1), (20, 20, 2, 2), (0, 6, 1, 1), (6, 65537, 1, 1), (150, 4000, 4, 4)):
        with pytest.raises(ValueError):
            M.align_window(h, w, levels, radius)
        assert M.load().mcraw_align_work_bytes(w, h, 2, levels, radius) == 0  # the library agrees
    for (H, W), levels, radius, _ in SCENES:
        wh, ww = M.align_window(H, W, levels, radius)
        B0 = R.bounds(levels, radius)[0]
        assert (wh, ww) == (H // 2 - 2 * B0, W // 2 - 2 * B0)
        R.check_window(H, W, levels, radius)
        assert M.load().mcraw_align_work_bytes(W, H, 2, levels, radius) > 0
