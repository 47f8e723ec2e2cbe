"""The position field (mcraw_align_cells_batch, mcraw_merge_cells_batch) without a GPU: the ABI's symbols and structs, every
rejection through the library itself (the checks come before the first use of the device), the args header under sanitizers, the
numpy statements (_align_cells_ref, _merge_cells_ref) against scalar ones written straight from the header, the recovery of the
two halves' motion of a scene with a seam, the sign against the merge's, and the merge statement's equivalences."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _align_cells_ref as CR
import _align_ref as R
import _merge_cells_ref as MC
import _merge_ref as MR
import motioncam_decoder_amd as M
from _cells_scenes import halves_field, halves_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "motioncam_decoder_amd", "csrc")
BLACK = (64, 64, 64, 64)
SYMS = ("mcraw_align_cells_batch", "mcraw_align_cells_work_bytes", "mcraw_merge_cells_batch")


def _hdr():
    return open(os.path.join(ROOT, "include", "mcraw_hip.h")).read()


def test_symbols_exported_and_listed():
    hdr, lib = _hdr(), M.load()
    for sym in SYMS:
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
        assert sym in M.ABI_SYMBOLS and hasattr(lib, sym), sym
    for name in ("AlignCells", "Cells", "cell_grid"):
        assert name in M.__all__
    block = hdr[hdr.index("a field of local positions"):hdr.index("} mcraw_cells;")]
    for line in ("cell_w a multiple of 256 and cell_h a multiple of 32", "cells_y = ceil(height / cell_h), cells_x = ceil(width / cell_w)",
                 "(n, cells_y, cells_x, 2) int16 as (y, x)", "g = (gpos[t] - gpos[b]) >> 1 per component",
                 "g >> (K - 1) (arithmetic)", "|G_l[t][clamp(y + dy, 0, h(l) - 1)][clamp(x + dx, 0, w(l) - 1)] - G_l[b][y][x]|",
                 "(i * cell_h) >> (l + 1) up to min(((i + 1) * cell_h) >> (l + 1), h(l))", "has SAD 0 for every candidate",
                 "key = (SAD, ddy * ddy + ddx * ddx, ddy, ddx)", "pos[t][i][j] = pos[t - 1][i][j] + 2 * d(t|t - 1)[i][j]",
                 "pos[t][i][j] = 2 * d(t|ref)[i][j]", "clamped to -32768 .. 32767", "drifts between cells over a long chain",
                 "exact for ref = r", "second-order error over a merge window",
                 "sy = (F[t][y / cell_h][x / cell_w].y - F[b][y / cell_h][x / cell_w].y) & ~1", "m->pos must be NULL",
                 "All nine terms of support 1 use the shift of the base pixel's own cell"):
        assert line in block, line
    for word in ("below a quad", "smaller than a merge tile", "regularising", "pairwise", "gyro", "resampling"):  # the steps that follow
        assert word in block, word
    # the global stage no longer calls local motion and rotation out of scope: it points here
    glob = hdr[hdr.index("the frames' global positions"):hdr.index("} mcraw_align;")]
    assert "Out of scope: local or tile-wise" not in glob and "mcraw_align_cells_batch" in glob


def test_struct_layouts():
    names = ("levels", "radius", "ref", "reserved", "cell_h", "cell_w", "black", "gpos", "pos", "sad", "work", "work_bytes")
    assert C.sizeof(M.AlignCells) == 72
    assert [getattr(M.AlignCells, f).offset for f in names] == [0, 4, 8, 12, 16, 20, 24, 32, 40, 48, 56, 64]
    m = re.search(r"\}\s*mcraw_align_cells;\s*/\*\s*sizeof (\d+); radius (\d+), ref (\d+), reserved (\d+), cell_h (\d+), cell_w (\d+), "
                  r"black (\d+), gpos (\d+), pos (\d+), sad (\d+), work (\d+), work_bytes (\d+)", _hdr())
    assert m and [int(v) for v in m.groups()] == [72, 4, 8, 12, 16, 20, 24, 32, 40, 48, 56, 64]
    names = ("cell_h", "cell_w", "cells_y", "cells_x", "reserved", "pos")
    assert C.sizeof(M.Cells) == 32
    assert [getattr(M.Cells, f).offset for f in names] == [0, 4, 8, 12, 16, 24]
    m = re.search(r"\}\s*mcraw_cells;\s*/\*\s*sizeof (\d+); cell_w (\d+), cells_y (\d+), cells_x (\d+), reserved (\d+), pos (\d+)", _hdr())
    assert m and [int(v) for v in m.groups()] == [32, 4, 8, 12, 16, 24]


def test_work_bytes_and_grid():
    wb = M.load().mcraw_align_cells_work_bytes
    uhd = wb(3840, 2160, 240, 3, 2, 64, 256)
    cells = 34 * 15
    assert M.cell_grid(2160, 3840) == (34, 15) and M.cell_grid(100, 600, (32, 256)) == (4, 3) and M.cell_grid(1, 1, (32, 256)) == (1, 1)
    # at least the pyramid (rows of whole 16-byte pieces), the candidates' 64-bit sums and a winner per cell and level
    assert uhd >= 240 * (2 * (1080 * 1920 + 540 * 960 + 270 * 480) + cells * (8 * (25 + 18) + 3 * 16))
    assert 0 < wb(16, 8, 1, 3, 4, 32, 256) <= wb(16, 8, 2, 3, 4, 32, 256) and wb(1, 1, 1, 1, 1, 32, 256) > 0
    for bad in ((600, 100, 4, 0, 2, 32, 256), (600, 100, 4, 4, 2, 32, 256), (600, 100, 4, 3, 0, 32, 256), (600, 100, 4, 3, 5, 32, 256),
                (600, 100, 4, 3, 2, 16, 256), (600, 100, 4, 3, 2, 48, 256), (600, 100, 4, 3, 2, 32, 128), (600, 100, 4, 3, 2, 32, 384),
                (600, 100, 4, 3, 2, 0, 256), (600, 100, 4, 3, 2, 32, 0), (0, 100, 4, 3, 2, 32, 256), (600, 65537, 4, 3, 2, 32, 256),
                (600, 100, 0, 3, 2, 32, 256), (600, 100, -1, 3, 2, 32, 256)):
        assert wb(*bad) == 0, bad
    for cell in ((16, 256), (32, 128), (48, 256), (32, 257), (0, 256), 64, (64,), (32.5, 256), (True, 256)):
        with pytest.raises(ValueError):
            M.cell_grid(100, 600, cell)


def _align_struct(levels=3, radius=2, ref=-1, reserved=0, cell=(32, 256), black=(0, 0, 0, 0), gpos=0, pos=0, sad=0, work=0, work_bytes=0):
    a = M.AlignCells()
    a.levels, a.radius, a.ref, a.reserved, a.cell_h, a.cell_w = levels, radius, ref, reserved, cell[0], cell[1]
    for i in range(4):
        a.black[i] = black[i]
    a.gpos, a.pos, a.sad, a.work, a.work_bytes = gpos or None, pos or None, sad or None, work or None, work_bytes
    return a


def test_every_rejection_through_the_library():
    """The entry points check their arguments before they touch the device or the context, so a host buffer stands for device
    memory and for the context here: every call below must come back < 0 with its prefix, and leave the buffer as it was."""
    lib = M.load()
    w, h, n = 600, 100, 3
    SENT = 0x5A
    buf = np.full(1 << 21, SENT, np.uint8)
    base = (buf.ctypes.data + 255) // 256 * 256
    ctx = C.c_void_p(base)  # never looked into by a rejected call
    ip, gp, pp, sp, op, lp = base + 4096, base + (1 << 19), base + (1 << 19) + 4096, base + (1 << 19) + 8192, base + (1 << 20), base + (1 << 19) + 16384
    kp = base + (1 << 20) + (1 << 19)
    need = lib.mcraw_align_cells_work_bytes(w, h, n, 3, 2, 32, 256)
    assert 0 < need <= (1 << 19) - 512 and 2 * n * w * h <= (1 << 19) - 4096
    S = lambda **kw: _align_struct(**dict(dict(gpos=gp, pos=pp, sad=sp, work=kp, work_bytes=need), **kw))

    def call(st=None, in_ptr=ip, pitch=w, fs=w * h, w_=w, h_=h, n_=n):
        return lib.mcraw_align_cells_batch(ctx, C.byref(st if st is not None else S()), C.c_void_p(in_ptr), pitch, fs, w_, h_, n_, None)

    cases = [
        ("no context", lambda: lib.mcraw_align_cells_batch(None, C.byref(S()), C.c_void_p(ip), w, w * h, w, h, n, None)),
        ("no struct", lambda: lib.mcraw_align_cells_batch(ctx, None, C.c_void_p(ip), w, w * h, w, h, n, None)),
        ("NULL in", lambda: call(in_ptr=0)), ("odd in", lambda: call(in_ptr=ip + 1)),
        ("NULL pos", lambda: call(S(pos=0))), ("odd pos", lambda: call(S(pos=pp + 1))), ("odd gpos", lambda: call(S(gpos=gp + 1))),
        ("sad on the 4-byte grid only", lambda: call(S(sad=sp + 4))),
        ("NULL work", lambda: call(S(work=0))), ("work on the 8-byte grid only", lambda: call(S(work=kp + 8))),
        ("work_bytes one short", lambda: call(S(work_bytes=need - 1))), ("work_bytes 0", lambda: call(S(work_bytes=0))),
        ("levels 0", lambda: call(S(levels=0))), ("levels 4", lambda: call(S(levels=4))),
        ("radius 0", lambda: call(S(radius=0))), ("radius 5", lambda: call(S(radius=5))),
        ("ref -2", lambda: call(S(ref=-2))), ("ref n", lambda: call(S(ref=n))), ("reserved", lambda: call(S(reserved=1))),
        ("cell_h 16", lambda: call(S(cell=(16, 256)))), ("cell_h 48", lambda: call(S(cell=(48, 256)))), ("cell_h 0", lambda: call(S(cell=(0, 256)))),
        ("cell_w 128", lambda: call(S(cell=(32, 128)))), ("cell_w 384", lambda: call(S(cell=(32, 384)))), ("cell_w 0", lambda: call(S(cell=(32, 0)))),
        ("width 0", lambda: call(w_=0)), ("height 65537", lambda: call(h_=65537, n_=1)), ("negative n", lambda: call(n_=-1)),
        ("pitch below width", lambda: call(pitch=w - 1)), ("frame stride too small", lambda: call(fs=w * h - 1)),
        ("pos inside the input", lambda: call(S(pos=ip + 64))), ("sad inside the input", lambda: call(S(sad=ip + 2 * n * w * h - 8))),
        ("work inside the input", lambda: call(S(work=ip + 16))), ("the input ends inside work", lambda: call(in_ptr=kp - 64)),
        ("pos inside work", lambda: call(S(pos=kp + 32))), ("sad inside work", lambda: call(S(sad=kp + need - 8))),
        ("pos and sad overlap", lambda: call(S(sad=pp + 8))), ("gpos inside pos", lambda: call(S(gpos=pp + 2))),
        ("gpos inside sad", lambda: call(S(gpos=sp + 8))), ("gpos inside work", lambda: call(S(gpos=kp + 100))),
    ]
    for name, fn in cases:
        assert fn() < 0, name
        msg = lib.mcraw_last_error().decode()
        assert msg.startswith("mcraw_align_cells_batch: ") and len(msg) > len("mcraw_align_cells_batch: "), (name, msg)
    assert call(n_=0) == 0 and call(_align_struct(), n_=0) == 0  # n == 0: a no-op

    # the merge with a field
    cy, cx = M.cell_grid(h, w, (32, 256))

    def mstruct(before=1, after=1, first=0, count=n, support=1, amount=256, lut_log2=6, shift=6, nluts=1, reserved=0, lut=lp, pos=0):
        m = M.Merge()
        m.before, m.after, m.first, m.count, m.support, m.amount = before, after, first, count, support, amount
        m.lut_log2, m.shift, m.nluts, m.reserved, m.lut, m.pos = lut_log2, shift, nluts, reserved, lut or None, pos or None
        return m

    def cstruct(cell=(32, 256), grid=(cy, cx), reserved=0, pos=pp):
        g = M.Cells()
        g.cell_h, g.cell_w, g.cells_y, g.cells_x, g.reserved, g.pos = cell[0], cell[1], grid[0], grid[1], reserved, pos or None
        return g

    def mcall(m=None, g=None, in_ptr=ip, pitch=w, fs=w * h, w_=w, h_=h, n_=n, out=op, opitch=w, ofs=w * h):
        return lib.mcraw_merge_cells_batch(ctx, C.byref(m if m is not None else mstruct()), C.byref(g if g is not None else cstruct()),
                                           C.c_void_p(in_ptr), pitch, fs, w_, h_, n_, C.c_void_p(out), opitch, ofs, None)

    mcases = [
        ("no context", lambda: lib.mcraw_merge_cells_batch(None, C.byref(mstruct()), C.byref(cstruct()), C.c_void_p(ip), w, w * h, w, h, n,
                                                           C.c_void_p(op), w, w * h, None)),
        ("no merge struct", lambda: lib.mcraw_merge_cells_batch(ctx, None, C.byref(cstruct()), C.c_void_p(ip), w, w * h, w, h, n, C.c_void_p(op),
                                                                w, w * h, None)),
        ("no cells", lambda: lib.mcraw_merge_cells_batch(ctx, C.byref(mstruct()), None, C.c_void_p(ip), w, w * h, w, h, n, C.c_void_p(op), w,
                                                         w * h, None)),
        # what mcraw_merge_batch rejects
        ("NULL in", lambda: mcall(in_ptr=0)), ("NULL out", lambda: mcall(out=0)), ("odd in", lambda: mcall(in_ptr=ip + 1)),
        ("odd out", lambda: mcall(out=op + 1)), ("width 0", lambda: mcall(w_=0)), ("height 65537", lambda: mcall(h_=65537, n_=1, m=mstruct(count=1))),
        ("negative n", lambda: mcall(n_=-1)), ("pitch below width", lambda: mcall(pitch=w - 1)), ("out pitch below width", lambda: mcall(opitch=w - 1)),
        ("frame stride too small", lambda: mcall(fs=w * h - 1)), ("out stride too small", lambda: mcall(ofs=w * h - 1)),
        ("before + after 16", lambda: mcall(mstruct(before=8, after=8))), ("first + count above n", lambda: mcall(mstruct(first=1))),
        ("support 2", lambda: mcall(mstruct(support=2))), ("amount 0", lambda: mcall(mstruct(amount=0))), ("amount 257", lambda: mcall(mstruct(amount=257))),
        ("lut_log2 5", lambda: mcall(mstruct(lut_log2=5))), ("lut_log2 11", lambda: mcall(mstruct(lut_log2=11))), ("shift 16", lambda: mcall(mstruct(shift=16))),
        ("nluts 2", lambda: mcall(mstruct(nluts=2))), ("reserved", lambda: mcall(mstruct(reserved=1))), ("NULL lut", lambda: mcall(mstruct(lut=0))),
        ("lut on the 8-byte grid only", lambda: mcall(mstruct(lut=lp + 8))), ("in and out overlap", lambda: mcall(out=ip + 2 * w * h)),
        # and what the field adds
        ("m->pos given", lambda: mcall(mstruct(pos=gp))), ("odd m->pos", lambda: mcall(mstruct(pos=gp + 1))),
        ("cell_h 16", lambda: mcall(g=cstruct(cell=(16, 256), grid=(7, 3)))), ("cell_h 48", lambda: mcall(g=cstruct(cell=(48, 256), grid=(3, 3)))),
        ("cell_w 128", lambda: mcall(g=cstruct(cell=(32, 128), grid=(4, 5)))), ("cell_w 0", lambda: mcall(g=cstruct(cell=(32, 0)))),
        ("cells_y one more", lambda: mcall(g=cstruct(grid=(cy + 1, cx)))), ("cells_x one fewer", lambda: mcall(g=cstruct(grid=(cy, cx - 1)))),
        ("cells_x the floor", lambda: mcall(g=cstruct(grid=(cy, w // 256)))), ("cells' reserved", lambda: mcall(g=cstruct(reserved=1))),
        ("NULL field", lambda: mcall(g=cstruct(pos=0))), ("odd field", lambda: mcall(g=cstruct(pos=pp + 1))),
        ("field inside the output", lambda: mcall(g=cstruct(pos=op + 64))), ("the field ends inside the output", lambda: mcall(g=cstruct(pos=op - 2))),
    ]
    for name, fn in mcases:
        assert fn() < 0, name
        msg = lib.mcraw_last_error().decode()
        assert msg.startswith("mcraw_merge_cells_batch: ") and len(msg) > len("mcraw_merge_cells_batch: "), (name, msg)
    assert mcall(n_=0) == 0 and mcall(mstruct(count=0)) == 0  # no-ops
    # mcraw_merge_batch itself keeps its prefix
    assert lib.mcraw_merge_batch(ctx, C.byref(mstruct(support=2)), C.c_void_p(ip), w, w * h, w, h, n, C.c_void_p(op), w, w * h, None) < 0
    assert lib.mcraw_last_error().decode().startswith("mcraw_merge_batch: ")
    assert (buf == SENT).all(), "a rejected call wrote"


def test_cells_args_without_hip(tmp_path):
    """csrc/mcraw_cells_args.h alone, under ASan and UBSan, as a program of its own: accept / reject over a sweep of geometries,
    the grid's ceilings, the planes, the sections of the scratch (aligned, in order, none overlapping another), work_bytes
    monotone in n, one defect at a time in pos / sad / gpos / work, and the merge's checks on a field."""
    exe = str(tmp_path / "cells_args_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "cpp", "cells_args_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-3000:], r.stderr[-3000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "wrong 0", r.stdout[-3000:]
    assert int(re.match(r"cases (\d+)", lines[-2]).group(1)) >= 1000, lines[-2]
    acc, rej = (int(v) for v in re.match(r"accepted (\d+) rejected (\d+)", lines[-3]).groups())
    assert acc >= 1000 and rej >= 1000, lines[-3]


def _scalar(imgs, black, cell, levels, radius, ref, gpos):
    """The header's statement, one pixel at a time, in Python integers."""
    n, H, W = imgs.shape
    ch, cw = cell
    Cy, Cx = -(-H // ch), -(-W // cw)

    def plane0(f):
        return [[min((sum(max(int(imgs[f, 2 * y + r, 2 * x + c]) - black[r * 2 + c], 0) for r in (0, 1) for c in (0, 1)) + 2) >> 2, 65535)
                 for x in range(W // 2)] for y in range(H // 2)]

    def half(g):
        wd = len(g[0]) // 2 if g else 0
        return [[(g[2 * y][2 * x] + g[2 * y][2 * x + 1] + g[2 * y + 1][2 * x] + g[2 * y + 1][2 * x + 1] + 2) >> 2 for x in range(wd)]
                for y in range(len(g) // 2)]

    pyr = []
    for f in range(n):
        p = [plane0(f)]
        for _ in range(levels - 1):
            p.append(half(p[-1]))
        pyr.append(p)
    dims = [(H >> (l + 1), W >> (l + 1)) for l in range(levels)]
    clamp = lambda v, hi: max(0, min(v, hi - 1))

    def d_of(t, b, i, j):
        cy = cx = 0
        if gpos is not None:
            cy = ((int(gpos[t][0]) - int(gpos[b][0])) >> 1) >> (levels - 1)
            cx = ((int(gpos[t][1]) - int(gpos[b][1])) >> 1) >> (levels - 1)
        for l in range(levels - 1, -1, -1):
            gb, gt = pyr[b][l], pyr[t][l]
            h, w = dims[l]
            rows = range((i * ch) >> (l + 1), min(((i + 1) * ch) >> (l + 1), h))
            cols = range((j * cw) >> (l + 1), min(((j + 1) * cw) >> (l + 1), w))
            rad = radius if l == levels - 1 else 1
            if l != levels - 1:
                cy, cx = 2 * cy, 2 * cx
            best = None
            for ddy in range(-rad, rad + 1):
                for ddx in range(-rad, rad + 1):
                    s = sum(abs(gt[clamp(y + cy + ddy, h)][clamp(x + cx + ddx, w)] - gb[y][x]) for y in rows for x in cols)
                    key = (s, ddy * ddy + ddx * ddx, ddy, ddx)
                    if best is None or key < best:
                        best = key
            cy, cx = cy + best[2], cx + best[3]
        return cy, cx, best[0]

    pos, sad = np.zeros((n, Cy, Cx, 2), np.int64), np.zeros((n, Cy, Cx), np.uint64)
    for i in range(Cy):
        for j in range(Cx):
            for t in range(n):
                if ref < 0 and t > 0:
                    dy, dx, sad[t, i, j] = d_of(t, t - 1, i, j)
                    pos[t, i, j] = pos[t - 1, i, j] + (2 * dy, 2 * dx)
                elif ref >= 0 and t != ref:
                    dy, dx, sad[t, i, j] = d_of(t, ref, i, j)
                    pos[t, i, j] = (2 * dy, 2 * dx)
    return np.clip(pos, -32768, 32767).astype(np.int16), sad


@pytest.mark.parametrize("levels", (1, 2, 3))
def test_numpy_statement_equals_the_scalar_one(levels):
    """About 70 x 40 grey pixels: 141 x 81 samples under cells of 32 x 256, so three cell rows (the last 17 rows tall) and one
    cell column cut by the frame; every levels x radius, the chain and an anchor, gpos given and NULL."""
    H, W, n, cell = 81, 141, 3, (32, 256)
    rng = np.random.default_rng(100 + levels)
    imgs = (rng.integers(0, 8, size=(n, H, W)) * 100 + rng.integers(0, 3, size=(n, H, W))).astype(np.uint16)  # few values: ties
    gpos = np.array([[0, 0], [5, -7], [-300, 9]], np.int16)  # odd components, and a step larger than the frame
    for radius in (1, 2, 3, 4):
        for ref in (-1, 1):
            for g in (None, gpos):
                got = CR.align_cells(imgs, BLACK, cell, levels, radius, ref, g)
                want = _scalar(imgs, BLACK, cell, levels, radius, ref, g)
                assert got[0].shape == (n,) + M.cell_grid(H, W, cell) + (2,) == (n, 3, 1, 2) and got[0].dtype == np.int16
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (radius, ref, g is None)
    # consequences: identical frames give zeros; a flat pair keeps its centre and sums |difference| over the cell's pixels
    same = CR.align_cells(np.stack([imgs[0]] * 3), BLACK, cell, levels, 2)
    assert not same[0].any() and not same[1].any()
    flat = np.stack([np.full((H, W), v, np.uint16) for v in (1000, 1300)])
    pos, sad = CR.align_cells(flat, (0, 0, 0, 0), cell, levels, 2)
    assert not pos.any() and sad[1, :, 0].tolist() == [300 * 16 * 70, 300 * 16 * 70, 300 * 8 * 70]
    pos, sad = CR.align_cells(flat, (0, 0, 0, 0), cell, levels, 2, -1, gpos[:2])
    c = ((gpos[1].astype(np.int64) - gpos[0]) >> 1) >> (levels - 1)
    assert np.array_equal(pos[1].astype(np.int64), np.broadcast_to(2 * (c << (levels - 1)), (3, 1, 2))) and pos[1].any()
    assert not CR.align_cells(imgs[:1], BLACK, cell, levels, 2)[0].any()  # n = 1


SEEDS = (1, 2, 3)
H3, W3, CELL3, LEVELS3, RADIUS3, BLUR3 = 256, 1536, (64, 256), 3, 2, 35  # blur: 35 samples >= 2^(levels + 1) + 1 = 17 grey pixels
KEEP = [0, 1, 4, 5]  # the cell columns that do not touch the seam at column 768 (2 of 6 do, by the geometry)


_HALVES = {}


def _halves(seed):
    if seed not in _HALVES:
        frames, off = halves_frames(seed, H3, W3, BLUR3, n=4, reach=8)
        _HALVES[seed] = (frames, off, halves_field(off, 4, 6, 3))
    return _HALVES[seed]


@pytest.mark.parametrize("seed", SEEDS)
def test_local_motion_is_recovered(seed):
    assert 2 * (2 ** (LEVELS3 + 1) + 1) <= BLUR3
    frames, off, want = _halves(seed)
    assert M.cell_grid(H3, W3, CELL3) == (4, 6) and (off[:, 0] != off[:, 1]).any()
    glob = R.align(frames, BLACK, LEVELS3, RADIUS3)[0]
    for gpos in (None, glob):
        pos, sad = CR.align_cells(frames, BLACK, CELL3, LEVELS3, RADIUS3, -1, gpos)
        assert np.array_equal(pos[:, :, KEEP].astype(np.int64), want[:, :, KEEP]), (seed, gpos is None)
        assert not sad[0].any()
    # the anchor form, every frame against frame 1
    pos = CR.align_cells(frames, BLACK, CELL3, LEVELS3, RADIUS3, 1, glob)[0]
    assert np.array_equal(pos[:, :, KEEP].astype(np.int64), (want - want[1])[:, :, KEEP])


def _cell_mask(cols):
    m = np.zeros((H3, W3), bool)
    for j in cols:
        m[:, j * CELL3[1]:(j + 1) * CELL3[1]] = True
    return m


def test_the_sign_and_the_point_of_it():
    """The plain mean of the window (the all-0 table) under the field returns the base frame exactly on every cell off the seam,
    whatever `support` is; under the negated field it does not; under one global shift per frame it does not on at least one whole
    half (the last two compared off the edge rows and columns that a member's shift leaves, where the base comes back anyway)."""
    frames, off, want = _halves(1)
    field = CR.align_cells(frames, BLACK, CELL3, LEVELS3, RADIUS3, -1, None)[0]
    zero = np.zeros((4, 64), np.uint16)
    b = 1
    m = int(np.abs(want - want[b]).max())
    assert 0 < m < 32
    inner = np.zeros((H3, W3), bool)
    inner[m:H3 - m, m:W3 - m] = True
    whole = _cell_mask(KEEP)  # every non-seam cell, the frame's edge rows and columns included: a member outside the frame weighs 0
    assert M.cell_grid(H3, W3, CELL3) == field.shape[1:3]
    for support in (0, 1):
        got = MC.merge(frames, zero, 10, field, CELL3, 1, 2, b, 1, support=support)[0]
        assert np.array_equal(got[whole], frames[b][whole]), support
    keep = whole & inner
    wrong = MC.merge(frames, zero, 10, -field.astype(np.int64), CELL3, 1, 2, b, 1, support=0)[0]
    assert not np.array_equal(wrong[keep], frames[b][keep])
    glob = R.align(frames, BLACK, LEVELS3, RADIUS3)[0]
    one = MR.merge(frames, zero, 10, 1, 2, b, 1, support=0, pos=glob)[0]
    left, right = _cell_mask(KEEP[:2]) & inner, _cell_mask(KEEP[2:]) & inner
    assert not np.array_equal(one[left], frames[b][left]) or not np.array_equal(one[right], frames[b][right])


@pytest.mark.parametrize("support", (0, 1))
def test_equivalences_of_the_merge_statement(support):
    H, W, n, cell = 70, 300, 4, (32, 256)
    rng = np.random.default_rng(50 + support)
    imgs = rng.integers(0, 4096, size=(n, H, W), dtype=np.uint16)
    lut, shift = M.noise_lut(S=2e-2, O=2e-3, black=64, white=4095)
    cy, cx = M.cell_grid(H, W, cell)
    # a field that is the same in every cell is merge(pos=)
    pos = rng.integers(-9, 10, size=(n, 2))
    const = np.broadcast_to(pos[:, None, None, :], (n, cy, cx, 2))
    assert np.array_equal(MC.merge(imgs, lut, shift, const, cell, 1, 2, support=support, amount=100),
                          MR.merge(imgs, lut, shift, 1, 2, support=support, amount=100, pos=pos))
    # and one that is not is not, but only in the cells that differ
    field = const.copy()
    field[2, 1, 1] += (4, -6)
    a, b = MC.merge(imgs, lut, shift, field, cell, 1, 2, support=support), MR.merge(imgs, lut, shift, 1, 2, support=support, pos=pos)
    assert not np.array_equal(a[:, 32:64, 256:], b[:, 32:64, 256:])
    a[:, 32:64, 256:] = b[:, 32:64, 256:]
    assert np.array_equal(a, b)
    # before = after = 0 returns the input
    assert np.array_equal(MC.merge(imgs, lut, shift, field, cell, 0, 0, support=support), imgs)
    # per-cell shifts that leave the frame weigh 0: those cells come back as the base, the others are merged
    far = np.zeros((n, cy, cx, 2), np.int64)
    far[1:, 0, 0] = (0, 2 * W)
    far[1:, 1, 1] = (-2 * H, 0)
    out = MC.merge(imgs, lut, shift, far, cell, 0, 3, 0, 1, support=support)[0]
    assert np.array_equal(out[:32, :256], imgs[0, :32, :256]) and np.array_equal(out[32:64, 256:], imgs[0, 32:64, 256:])
    assert np.array_equal(out[64:], MR.merge(imgs, lut, shift, 0, 3, 0, 1, support=support)[0][64:]) and not np.array_equal(out[64:], imgs[0, 64:])
