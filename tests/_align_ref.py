"""numpy statement of mcraw_align_batch's contract (include/mcraw_hip.h): the grey plane of a mosaic, its pyramid, the levels'
bounds, the coarse-to-fine search of a pair with the tie key, the chain / anchor positions with the clamp, and `sad`.  int64
throughout."""
import numpy as np


def grey(img, black=(0, 0, 0, 0)):
    """G0 of one mosaic (H, W): (H // 2, W // 2) int64."""
    H, W = img.shape
    h, w = H // 2, W // 2
    bl = np.asarray(black, np.int64).reshape(2, 2)
    s = np.maximum(img[:2 * h, :2 * w].astype(np.int64).reshape(h, 2, w, 2) - bl[None, :, None, :], 0)
    return np.minimum((s.sum(axis=(1, 3)) + 2) >> 2, 65535)


def down(g):
    """G(l + 1) of G(l)."""
    h, w = g.shape[0] // 2, g.shape[1] // 2
    return (g[:2 * h, :2 * w].reshape(h, 2, w, 2).sum(axis=(1, 3)) + 2) >> 2


def pyramid(img, black, levels):
    p = [grey(img, black)]
    for _ in range(levels - 1):
        p.append(down(p[-1]))
    return p


def bounds(levels, radius):
    """B(l) for l = 0 .. levels - 1."""
    assert 1 <= levels <= 6 and 1 <= radius <= 8
    B = [radius]
    for _ in range(levels - 1):
        B.insert(0, 2 * B[0] + 1)
    return B


def check_window(H, W, levels, radius):
    """ValueError where the contract rejects the geometry: the window is empty at a level."""
    for l, B in enumerate(bounds(levels, radius)):
        if ((H // 2) >> l) - 2 * B < 1 or ((W // 2) >> l) - 2 * B < 1:
            raise ValueError("empty window at level %d" % l)


def sads(gb, gt, B, cy, cx, R):
    """SAD_l(cy + ddy, cx + ddx) for ddy, ddx in -R .. R: (2R + 1, 2R + 1) int64."""
    h, w = gb.shape
    base = gb[B:h - B, B:w - B]
    if (2 * R + 1) ** 2 * base.size <= 1 << 22:  # every candidate's window at once
        v = np.lib.stride_tricks.sliding_window_view(gt, base.shape)[B + cy - R:B + cy + R + 1, B + cx - R:B + cx + R + 1]
        return np.abs(v - base).sum(axis=(2, 3))
    out = np.empty((2 * R + 1, 2 * R + 1), np.int64)
    for i, dy in enumerate(range(cy - R, cy + R + 1)):
        for j, dx in enumerate(range(cx - R, cx + R + 1)):
            out[i, j] = np.abs(gt[B + dy:h - B + dy, B + dx:w - B + dx] - base).sum()
    return out


def pair(pb, pt, radius):
    """(dy, dx, SAD) of the level-0 winner for the pyramids of base and member."""
    levels = len(pb)
    B = bounds(levels, radius)
    cy = cx = 0
    for l in range(levels - 1, -1, -1):
        R = radius if l == levels - 1 else 1
        s = sads(pb[l], pt[l], B[l], cy, cx, R)
        key = min((int(s[dy + R, dx + R]), dy * dy + dx * dx, dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1))
        cy, cx = cy + key[2], cx + key[3]
        assert abs(cy) <= B[l] and abs(cx) <= B[l]
        if l:
            cy, cx = 2 * cy, 2 * cx
    return cy, cx, key[0]


def positions(d, ref=-1):
    """pos (n, 2) int16 from d (n, 2): d[t] = d(t | base of t) in quads (ignored for the frame without a pair): the chain's sums
    in int32 or the anchor form, clamped."""
    d = np.asarray(d, np.int64).reshape(-1, 2)
    step = 2 * d
    if ref < 0:
        step[:1] = 0
        pos = np.cumsum(step, axis=0)
        assert np.abs(pos).max(initial=0) < 1 << 31
    else:
        step[ref] = 0
        pos = step
    return np.clip(pos, -32768, 32767).astype(np.int16)


def align(imgs, black=(0, 0, 0, 0), levels=4, radius=4, ref=-1):
    """(pos (n, 2) int16, sad (n,) uint64) for a batch (n, H, W) of uint16 mosaics."""
    imgs = np.asarray(imgs)
    assert imgs.ndim == 3 and imgs.dtype == np.uint16 and -1 <= ref < max(len(imgs), 1)
    n, H, W = imgs.shape
    check_window(H, W, levels, radius)
    pyr = [pyramid(f, black, levels) for f in imgs]
    d, sad = np.zeros((n, 2), np.int64), np.zeros(n, np.uint64)
    for t in range(n):
        b = t - 1 if ref < 0 else (ref if t != ref else -1)
        if b >= 0:
            dy, dx, s = pair(pyr[b], pyr[t], radius)
            d[t], sad[t] = (dy, dx), s
    return positions(d, ref), sad
