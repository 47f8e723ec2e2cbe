"""numpy statement of mcraw_merge_cells_batch's contract (include/mcraw_hip.h): _merge_ref's merge, except that the shift of a
member at a base pixel is that of the pixel's cell in a position field (n, Cy, Cx, 2); every term of the 3x3 measure of a pixel
uses the shift of the pixel's own cell.  int64 throughout."""
import numpy as np

import _merge_ref as MR


def cell_index(H, W, cell):
    """(H, W) arrays of the cell row and the cell column of every pixel."""
    return np.broadcast_to((np.arange(H) // cell[0])[:, None], (H, W)), np.broadcast_to((np.arange(W) // cell[1])[None, :], (H, W))


def shifts_of(field, t, b):
    """(Cy, Cx, 2) of (sy, sx) of member t against base b: the difference of the cells' positions with the low bit dropped."""
    f = np.asarray(field).astype(np.int64)
    return (f[t] - f[b]) & ~1


def measure(base, member, sh, cell, support):
    """(a, inside, D) of _merge_ref.measure with the shift of every pixel's own cell: the whole-frame measure of each distinct
    shift, taken where its cells are."""
    H, W = base.shape
    ci, cj = cell_index(H, W, cell)
    a, inside, D = np.zeros((H, W), np.int64), np.zeros((H, W), bool), np.zeros((H, W), np.int64)
    for sy, sx in sorted({(int(v[0]), int(v[1])) for v in sh.reshape(-1, 2)}):
        a1, in1, D1 = MR.measure(base, member, sy, sx, support)
        m = (sh[ci, cj, 0] == sy) & (sh[ci, cj, 1] == sx)
        a[m], inside[m], D[m] = a1[m], in1[m], D1[m]
    return a, inside, D


def mean(imgs, b, lut, shift, before, after, support, field, cell):
    """m of the contract for the base frame b: _merge_ref.mean with measure() above."""
    n, H, W = imgs.shape
    lut = np.asarray(lut)
    L = lut.shape[1]
    c = imgs[b].astype(np.int64)
    r = lut.astype(np.int64)[MR.positions(H, W), np.minimum(c >> shift, L - 1)]
    num, den = 256 * c, np.full((H, W), 256, np.int64)
    for t in MR.window(b, n, before, after):
        a, inside, D = measure(imgs[b], imgs[t], shifts_of(field, t, b), cell, support)
        x = np.minimum((D * r) >> 8, 16)
        w = np.where(inside, 256 - x * x, 0)
        num += w * a
        den += w
    assert num.max() < 1 << 28 and den.min() >= 256 and den.max() <= 4096
    return (num + (den >> 1)) // den


def merge(imgs, lut, shift, field, cell, before=2, after=2, first=0, count=None, support=1, amount=256):
    """out (count, H, W) uint16 for a batch (n, H, W) and a field (n, Cy, Cx, 2); lut: (4, L) or (n, 4, L)."""
    imgs = np.asarray(imgs)
    assert imgs.ndim == 3 and imgs.dtype == np.uint16
    n, H, W = imgs.shape
    field = np.asarray(field)
    assert field.shape == (n, (H + cell[0] - 1) // cell[0], (W + cell[1] - 1) // cell[1], 2)
    count = n - first if count is None else count
    lut = np.asarray(lut)
    out = np.empty((count, H, W), np.uint16)
    for j in range(count):
        b = first + j
        m = mean(imgs, b, lut if lut.ndim == 2 else lut[b], shift, before, after, support, field, cell)
        out[j] = MR.blend(imgs[b].astype(np.int64), m, amount).astype(np.uint16)
    return out
