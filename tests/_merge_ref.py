"""numpy statement of mcraw_merge_batch's contract (include/mcraw_hip.h): output j is the base frame first + j, every pixel
the weighted mean of itself and the samples at its (shifted) position in the other frames of the base's window, the weights
falling with a motion measure (the pixel's own difference, or the 3x3 sum of differences with a per-pixel guard) over the
cut-off that the denoiser's per-level, per-CFA-position table gives.  int64 throughout: the bounds the contract states are
checked, not relied on."""
import numpy as np


def positions(H, W):
    return (np.arange(H)[:, None] & 1) * 2 + (np.arange(W)[None, :] & 1)


def window(b, n, before, after):
    """The members of base b: max(0, b - before) .. min(n - 1, b + after) without b (clipped, not wrapped)."""
    return [t for t in range(max(0, b - before), min(n - 1, b + after) + 1) if t != b]


def shift_of(pos, t, b):
    """(sy, sx) of member t against base b: the difference of the positions with the low bit dropped towards minus infinity."""
    if pos is None:
        return 0, 0
    pos = np.asarray(pos).astype(np.int64)
    return int(pos[t, 0] - pos[b, 0]) & ~1, int(pos[t, 1] - pos[b, 1]) & ~1


def _moved(img, sy, sx, pad):
    """img[y + sy][x + sx] for y in -pad .. H + pad - 1, x likewise, as int64 with 0 outside the frame, and the mask of the
    positions (y, x) whose own position and moved position both lie inside the frame."""
    H, W = img.shape
    ys, xs = np.arange(-pad, H + pad), np.arange(-pad, W + pad)
    oky = (ys >= 0) & (ys < H) & (ys + sy >= 0) & (ys + sy < H)
    okx = (xs >= 0) & (xs < W) & (xs + sx >= 0) & (xs + sx < W)
    ok = oky[:, None] & okx[None, :]
    val = img.astype(np.int64)[np.clip(ys + sy, 0, H - 1)[:, None], np.clip(xs + sx, 0, W - 1)[None, :]]
    return np.where(ok, val, 0), ok


def measure(base, member, sy, sx, support):
    """(a, inside, D) of the contract for one member: the member's samples (int64, 0 where outside), whether the member's
    position is inside the frame, and the motion measure."""
    H, W = base.shape
    a1, ok1 = _moved(member, sy, sx, 1)
    c1 = np.pad(base.astype(np.int64), 1)
    e1 = np.where(ok1, a1 - c1, 0)  # e(dy, dx) where both positions are inside the frame, else 0
    a, inside, e0 = a1[1:-1, 1:-1], ok1[1:-1, 1:-1], e1[1:-1, 1:-1]
    if support == 0:
        return a, inside, np.abs(e0)
    s = np.zeros((H, W), np.int64)
    nv = np.zeros((H, W), np.int64)
    for dy in range(3):
        for dx in range(3):
            s += e1[dy:dy + H, dx:dx + W]
            nv += ok1[dy:dy + H, dx:dx + W]
    s += (9 - nv) * e0  # a term outside counts e0 instead
    return a, inside, np.maximum(np.minimum(np.abs(s) >> 3, 65535), np.abs(e0) >> 1)


def mean(imgs, b, lut, shift, before, after, support=1, pos=None):
    """m of the contract for the base frame b of the batch: (H, W) int64.  lut: (4, L), the base's table."""
    n, H, W = imgs.shape
    lut = np.asarray(lut)
    assert lut.ndim == 2 and lut.shape[0] == 4 and lut.dtype == np.uint16
    L = lut.shape[1]
    assert L in (64, 128, 256, 512, 1024) and 0 <= shift <= 15 and support in (0, 1) and before + after <= 15
    c = imgs[b].astype(np.int64)
    r = lut.astype(np.int64)[positions(H, W), np.minimum(c >> shift, L - 1)]
    num, den = 256 * c, np.full((H, W), 256, np.int64)
    for t in window(b, n, before, after):
        sy, sx = shift_of(pos, t, b)
        a, inside, D = measure(imgs[b], imgs[t], sy, sx, support)
        prod = D * r
        assert prod.size == 0 or prod.max() < 1 << 32
        x = np.minimum(prod >> 8, 16)
        w = np.where(inside, 256 - x * x, 0)
        num += w * a
        den += w
    assert num.size == 0 or (num.max() < 1 << 28 and den.min() >= 256 and den.max() <= 4096)
    return (num + (den >> 1)) // den


def blend(c, m, amount):
    """out of the contract from c and m (int64 arrays): c + (((m - c) * amount + 128) >> 8), which lies between them."""
    assert 1 <= amount <= 256
    o = c + (((m - c) * amount + 128) >> 8)
    assert o.size == 0 or (np.minimum(c, m) <= o).all() and (o <= np.maximum(c, m)).all()
    return o


def merge(imgs, lut, shift, before=2, after=2, first=0, count=None, support=1, amount=256, pos=None):
    """out (count, H, W) uint16 for a batch (n, H, W); lut: (4, L) for the batch or (n, 4, L), one table per base frame."""
    imgs = np.asarray(imgs)
    assert imgs.ndim == 3 and imgs.dtype == np.uint16
    n = imgs.shape[0]
    count = n - first if count is None else count
    assert 0 <= first and first + count <= n
    lut = np.asarray(lut)
    assert lut.ndim == 2 or (lut.ndim == 3 and lut.shape[0] == n)
    out = np.empty((count,) + imgs.shape[1:], np.uint16)
    for j in range(count):
        b = first + j
        m = mean(imgs, b, lut if lut.ndim == 2 else lut[b], shift, before, after, support, pos)
        out[j] = blend(imgs[b].astype(np.int64), m, amount).astype(np.uint16)
    return out
