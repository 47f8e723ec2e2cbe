"""numpy statement of mcraw_align_cells_batch's contract (include/mcraw_hip.h): _align_ref's grey plane and pyramid, the centre
from the global positions, per cell the SAD over the cell's pixels with clamped coordinates, the coarse-to-fine search with the
tie key, the chain / anchor field with the clamp, and `sad`.  int64 throughout."""
import numpy as np

import _align_ref as R


def grid(H, W, cell):
    """(cells_y, cells_x): the ceilings."""
    ch, cw = cell
    assert ch >= 32 and ch % 32 == 0 and cw >= 256 and cw % 256 == 0
    return (H + ch - 1) // ch, (W + cw - 1) // cw


def cell_pixels(i, j, cell, l, h, w):
    """(r0, r1, c0, c1): the pixels of cell (i, j) in the level-l plane of h x w (r0 >= r1 or c0 >= c1: none)."""
    ch, cw = cell
    return (i * ch) >> (l + 1), min(((i + 1) * ch) >> (l + 1), h), (j * cw) >> (l + 1), min(((j + 1) * cw) >> (l + 1), w)


def sads(gb, gt, box, cy, cx, Rr):
    """SAD(cy + ddy, cx + ddx) over the cell's pixels `box` for ddy, ddx in -Rr .. Rr: (2 Rr + 1, 2 Rr + 1) int64; coordinates
    into the member are clamped to its plane."""
    r0, r1, c0, c1 = box
    out = np.zeros((2 * Rr + 1, 2 * Rr + 1), np.int64)
    if r0 >= r1 or c0 >= c1:
        return out
    h, w = gt.shape
    base = gb[r0:r1, c0:c1]
    ys, xs = np.arange(r0, r1), np.arange(c0, c1)
    for a, dy in enumerate(range(cy - Rr, cy + Rr + 1)):
        rows = gt[np.clip(ys + dy, 0, h - 1)]
        for b, dx in enumerate(range(cx - Rr, cx + Rr + 1)):
            out[a, b] = np.abs(rows[:, np.clip(xs + dx, 0, w - 1)] - base).sum()
    return out


def centre(gpos, t, b, levels):
    """(cy, cx) at the coarsest level for the pair (b, t): ((gpos[t] - gpos[b]) >> 1) >> (levels - 1), arithmetic."""
    if gpos is None:
        return 0, 0
    g = np.asarray(gpos).astype(np.int64)
    return tuple(int(((g[t, k] - g[b, k]) >> 1) >> (levels - 1)) for k in (0, 1))


def pair_cell(pb, pt, i, j, cell, radius, c0):
    """(dy, dx, SAD) of the level-0 winner of cell (i, j) for the pyramids of base and member, from the centre c0 at the top."""
    levels = len(pb)
    cy, cx = c0
    for l in range(levels - 1, -1, -1):
        Rr = radius if l == levels - 1 else 1
        s = sads(pb[l], pt[l], cell_pixels(i, j, cell, l, *pb[l].shape), cy, cx, Rr)
        key = min((int(s[dy + Rr, dx + Rr]), dy * dy + dx * dx, dy, dx) for dy in range(-Rr, Rr + 1) for dx in range(-Rr, Rr + 1))
        cy, cx = cy + key[2], cx + key[3]
        if l:
            cy, cx = 2 * cy, 2 * cx
    return cy, cx, key[0]


def positions(d, ref=-1):
    """The field (n, Cy, Cx, 2) int16 from d (n, Cy, Cx, 2) in quads: _align_ref.positions cell by cell."""
    d = np.asarray(d, np.int64)
    n, cy, cx, _ = d.shape
    return np.stack([R.positions(d[:, i, j], ref) for i in range(cy) for j in range(cx)], axis=1).reshape(n, cy, cx, 2)


def align_cells(imgs, black=(0, 0, 0, 0), cell=(64, 256), levels=3, radius=2, ref=-1, gpos=None):
    """(pos (n, Cy, Cx, 2) int16, sad (n, Cy, Cx) uint64) for a batch (n, H, W) of uint16 mosaics."""
    imgs = np.asarray(imgs)
    assert imgs.ndim == 3 and imgs.dtype == np.uint16 and -1 <= ref < max(len(imgs), 1)
    assert 1 <= levels <= 3 and 1 <= radius <= 4
    n, H, W = imgs.shape
    Cy, Cx = grid(H, W, cell)
    pyr = [R.pyramid(f, black, levels) for f in imgs]
    d, sad = np.zeros((n, Cy, Cx, 2), np.int64), np.zeros((n, Cy, Cx), np.uint64)
    for t in range(n):
        b = t - 1 if ref < 0 else (ref if t != ref else -1)
        if b < 0:
            continue
        c0 = centre(gpos, t, b, levels)
        for i in range(Cy):
            for j in range(Cx):
                dy, dx, s = pair_cell(pyr[b], pyr[t], i, j, cell, radius, c0)
                d[t, i, j], sad[t, i, j] = (dy, dx), s
    return positions(d, ref), sad
