"""numpy statement of mcraw_denoise_batch's contract (include/mcraw_hip.h): every pixel of a uint16 mosaic becomes the
weighted mean of itself and the 8 (radius 1) or 24 (radius 2) neighbours on its own lattice (distances 2 and 4, reflected at
the frame's edges), the weights falling with the squared difference over a cut-off that a per-level, per-CFA-position table
gives.  int64 throughout: the bounds the contract states are checked, not relied on."""
import numpy as np


def neighbour(c, d, size):
    """c + d; outside [0, size): c - d; that outside too: c.  c: an int array."""
    c = np.asarray(c, dtype=np.int64)
    a, b = c + d, c - d
    return np.where((a >= 0) & (a < size), a, np.where((b >= 0) & (b < size), b, c))


def offsets(radius):
    """(dy, dx) of the neighbours: {-2R .. 2R step 2}^2 without (0, 0)."""
    steps = range(-2 * radius, 2 * radius + 1, 2)
    return tuple((dy, dx) for dy in steps for dx in steps if (dy, dx) != (0, 0))


def positions(H, W):
    return (np.arange(H)[:, None] & 1) * 2 + (np.arange(W)[None, :] & 1)


def neighbours(img, radius):
    """The (H, W) arrays of every pixel's neighbour values, in the order of offsets(radius)."""
    H, W = img.shape
    ys = {d: neighbour(np.arange(H), d, H) if d else np.arange(H) for d in range(-2 * radius, 2 * radius + 1, 2)}
    xs = {d: neighbour(np.arange(W), d, W) if d else np.arange(W) for d in range(-2 * radius, 2 * radius + 1, 2)}
    return [img[ys[dy][:, None], xs[dx][None, :]] for dy, dx in offsets(radius)]


def mean(img, lut, shift, radius):
    """m of the contract for one mosaic: (H, W) int64.  lut: (4, L)."""
    H, W = img.shape
    lut = np.asarray(lut)
    assert lut.ndim == 2 and lut.shape[0] == 4 and lut.dtype == np.uint16
    L = lut.shape[1]
    assert L in (64, 128, 256, 512, 1024) and 0 <= shift <= 15 and radius in (1, 2)
    c = img.astype(np.int64)
    r = lut.astype(np.int64)[positions(H, W), np.minimum(c >> shift, L - 1)]
    num, den = 256 * c, np.full((H, W), 256, np.int64)
    for a in neighbours(img, radius):
        a = a.astype(np.int64)
        prod = np.abs(a - c) * r
        assert prod.size == 0 or prod.max() < 1 << 32
        x = np.minimum(prod >> 8, 16)
        w = 256 - x * x
        num += w * a
        den += w
    assert num.size == 0 or (num.max() < 1 << 29 and den.min() >= 256 and den.max() <= 6400)
    return (num + (den >> 1)) // den


def blend(c, m, amount):
    """out of the contract from c and m (int64 arrays): c + (((m - c) * amount + 128) >> 8), which lies between them."""
    assert 1 <= amount <= 256
    o = c + (((m - c) * amount + 128) >> 8)
    assert o.size == 0 or (np.minimum(c, m) <= o).all() and (o <= np.maximum(c, m)).all()
    return o


def denoise(imgs, lut, shift, radius=2, amount=256):
    """out (N, H, W) uint16 for a batch; lut: (4, L) for the batch or (N, 4, L), one table per frame."""
    imgs = np.asarray(imgs)
    assert imgs.ndim == 3 and imgs.dtype == np.uint16 and 1 <= amount <= 256
    lut = np.asarray(lut)
    assert lut.ndim == 2 or (lut.ndim == 3 and lut.shape[0] == imgs.shape[0])
    out = np.empty(imgs.shape, np.uint16)
    for f in range(imgs.shape[0]):
        m = mean(imgs[f], lut if lut.ndim == 2 else lut[f], shift, radius)
        out[f] = blend(imgs[f].astype(np.int64), m, amount).astype(np.uint16)
    return out
