"""numpy statement of mcraw_fixpix_batch's contract (include/mcraw_hip.h): defective pixels of a uint16 mosaic found against
the eight neighbours on the pixel's own lattice (distance 2, reflected at the frame's edges) and replaced by the mean of
the flattest opposite pair; an optional static list of pixels replaced unconditionally from pairs that are not listed
themselves.  int64 throughout: the bounds the contract states are checked, not relied on."""
import numpy as np

HOT, COLD = 1, 2
# (dy, dx) of the eight neighbours, in the contract's order, and the four opposite pairs as indices into it
NEIGHBOURS = ((-2, -2), (-2, 0), (-2, 2), (0, -2), (0, 2), (2, -2), (2, 0), (2, 2))
PAIRS = ((3, 4), (1, 6), (0, 7), (2, 5))  # (W,E), (N,S), (NW,SE), (NE,SW)


def neighbour(c, d, size):
    """c + d; outside [0, size): c - d; that outside too: c.  c: an int array."""
    c = np.asarray(c, dtype=np.int64)
    a, b = c + d, c - d
    return np.where((a >= 0) & (a < size), a, np.where((b >= 0) & (b < size), b, c))


def positions(H, W):
    return (np.arange(H)[:, None] & 1) * 2 + (np.arange(W)[None, :] & 1)


def neighbours(img):
    """The eight (H, W) uint16 arrays of every pixel's neighbour values, in the contract's order."""
    H, W = img.shape
    ys = {d: neighbour(np.arange(H), d, H) for d in (-2, 2)}
    xs = {d: neighbour(np.arange(W), d, W) for d in (-2, 2)}
    ys[0], xs[0] = np.arange(H), np.arange(W)
    return [img[ys[dy][:, None], xs[dx][None, :]] for dy, dx in NEIGHBOURS]


def threshold(m, p, black, abs_thr, rel_thr, peak=None):
    prod = np.maximum(m.astype(np.int64) - np.asarray(black, np.int64)[p], 0) * int(rel_thr)
    assert prod.size == 0 or prod.max() < 1 << 32
    t = np.asarray(abs_thr, np.int64)[p] + (prod >> 8)
    assert t.size == 0 or t.max() < 1 << 32
    if peak is not None and prod.size:
        peak.append(int(max(prod.max(), t.max())))
    return t


def replacement(nb, eligible=None):
    """(value, any pair eligible) from the neighbour values nb (8, ...): the mean, rounded up, of the opposite pair with
    the smallest |a - b|, the first pair winning ties; `eligible` (4, ...) bool keeps pairs out."""
    diffs = np.stack([np.abs(nb[a] - nb[b]) for a, b in PAIRS])
    means = np.stack([(nb[a] + nb[b] + 1) >> 1 for a, b in PAIRS])
    if eligible is not None:
        diffs = np.where(eligible, diffs, 1 << 20)
    k = np.argmin(diffs, axis=0)  # the first of equal minima
    val = np.take_along_axis(means, k[None], axis=0)[0]
    ok = np.ones(val.shape, bool) if eligible is None else eligible.any(axis=0)
    return val, ok


def member(lst, keys):
    """The contract's lower-bound search, literally, for an array of keys: a list that is not ascending has one defined
    result too."""
    lst = np.asarray(lst, dtype=np.int64)
    keys = np.asarray(keys, dtype=np.int64)
    n = len(lst)
    lo = np.zeros(keys.shape, np.int64)
    hi = np.full(keys.shape, n, np.int64)
    while True:
        act = lo < hi
        if not act.any():
            break
        mid = (lo + hi) >> 1
        less = lst[np.where(act, mid, 0)] < keys
        lo = np.where(act & less, mid + 1, lo)
        hi = np.where(act & ~less, mid, hi)
    return (lo < n) & (lst[np.minimum(lo, max(n - 1, 0))] == keys) if n else np.zeros(keys.shape, bool)


def rank_values(nb, rank):
    """(Hk, Lk): the rank-th largest and the rank-th smallest of the eight arrays, duplicates counting."""
    h1, l1 = nb[0], nb[0]
    h2, l2 = np.zeros_like(h1), np.full_like(l1, 65535)
    for a in nb[1:]:
        h2, h1 = np.maximum(h2, np.minimum(h1, a)), np.maximum(h1, a)
        l2, l1 = np.minimum(l2, np.maximum(l1, a)), np.minimum(l1, a)
    return (h1, l1) if rank == 1 else (h2, l2)


def dynamic(img, flags, rank, rel_thr, black, abs_thr, peak=None):
    """(out int64 (H, W), hot (H, W) bool, cold (H, W) bool) of the dynamic pass for one mosaic."""
    assert rank in (1, 2) and 0 <= rel_thr <= 65535 and not flags & ~(HOT | COLD)
    H, W = img.shape
    nb = neighbours(img)
    Hk, Lk = rank_values(nb, rank)
    p = positions(H, W)
    hot, cold = np.zeros((H, W), bool), np.zeros((H, W), bool)
    for on, flag, side, ref in ((flags & HOT, hot, img > Hk, Hk), (flags & COLD, cold, img < Lk, Lk)):
        if on:  # the thresholds where they can matter: v outside [Lk, Hk]
            cy, cx = np.nonzero(side)
            m, v = ref[cy, cx].astype(np.int64), img[cy, cx].astype(np.int64)
            flag[cy, cx] = np.abs(v - m) > threshold(m, p[cy, cx], black, abs_thr, rel_thr, peak)
    assert not (hot & cold).any()
    out = img.astype(np.int64)
    fy, fx = np.nonzero(hot | cold)
    rep, _ = replacement(np.stack([a[fy, fx] for a in nb]).astype(np.int64))
    out[fy, fx] = rep
    return out, hot, cold


def fixpix(imgs, flags=HOT | COLD, rank=2, rel_thr=0, black=(0, 0, 0, 0), abs_thr=(0, 0, 0, 0), lst=None, peak=None):
    """(out (N, H, W) uint16, counts (N, 2, 4) uint32: hot[4], cold[4] by CFA position) for a batch; lst: the packed
    entries y << 16 | x as the call gets them (any order, entries outside the frame included), or None."""
    imgs = np.asarray(imgs)
    assert imgs.ndim == 3 and imgs.dtype == np.uint16
    N, H, W = imgs.shape
    lst = np.zeros(0, np.uint32) if lst is None else np.asarray(lst, dtype=np.uint32)
    assert lst.ndim == 1 and len(lst) <= 1 << 20
    p = positions(H, W)
    ly, lx = (lst >> 16).astype(np.int64), (lst & 0xFFFF).astype(np.int64)
    keep = (lx < W) & (ly < H)
    ly, lx = ly[keep], lx[keep]
    if len(lst):
        ny = np.stack([neighbour(ly, dy, H) if dy else ly for dy, _ in NEIGHBOURS])
        nx = np.stack([neighbour(lx, dx, W) if dx else lx for _, dx in NEIGHBOURS])
        free = ~member(lst, (ny << 16) | nx)
        eligible = np.stack([free[a] & free[b] for a, b in PAIRS])
    out = np.empty((N, H, W), np.uint16)
    counts = np.zeros((N, 2, 4), np.uint32)
    for f in range(N):
        o, hot, cold = dynamic(imgs[f], flags, rank, rel_thr, black, abs_thr, peak)
        if len(lst):
            fy, fx = np.nonzero(hot | cold)  # a flagged pixel that the search finds in the list is not counted
            found = member(lst, (fy.astype(np.int64) << 16) | fx)
            hot[fy[found], fx[found]] = cold[fy[found], fx[found]] = False
            v = imgs[f].astype(np.int64)
            rep, ok = replacement(v[ny, nx], eligible)
            o[ly[ok], lx[ok]] = rep[ok]
        for q in range(4):
            counts[f, 0, q], counts[f, 1, q] = (hot & (p == q)).sum(), (cold & (p == q)).sum()
        out[f] = o.astype(np.uint16)
    return out, counts
