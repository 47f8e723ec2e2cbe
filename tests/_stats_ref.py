"""The contract of mcraw_stats_batch (include/mcraw_hip.h) in numpy: per frame and CFA position p = (y & 1) * 2 + (x & 1) a
histogram of min(v >> shift, B - 1), the sample count, the saturated count (v >= sat[p]), the int64 sum of the unsaturated
samples, min and max over the window; and the record bytes (uint32 hist[4][B], cnt[4], nsat[4], min[4], max[4], uint64
sum[4]).  Everything is an integer: the GPU result must equal this byte for byte."""
import numpy as np


def record_bytes(bins):
    return 16 * bins + 96


def empty(n, bins):
    """The fields of n records nothing was counted into."""
    return {"hist": np.zeros((n, 4, bins), np.uint32), "cnt": np.zeros((n, 4), np.uint32), "nsat": np.zeros((n, 4), np.uint32),
            "min": np.full((n, 4), 65535, np.uint32), "max": np.zeros((n, 4), np.uint32), "sum": np.zeros((n, 4), np.uint64)}


def stats(imgs, bins=256, shift=0, sat=(65535,) * 4, roi=None, into=None):
    """The fields for frames (N, H, W) uint16; roi = (y0, x0, h, w) in frame pixels.  into: fields to accumulate into
    (MCRAW_STATS_ACCUMULATE: counters modulo 2^32, min / max combined); they are not modified."""
    imgs = np.asarray(imgs)
    assert imgs.dtype == np.uint16 and imgs.ndim == 3
    n, H, W = imgs.shape
    y0, x0, h, w = (0, 0, H, W) if roi is None else roi
    assert 0 <= y0 and 0 <= x0 and h >= 1 and w >= 1 and y0 + h <= H and x0 + w <= W
    out = empty(n, bins) if into is None else {k: v.copy() for k, v in into.items()}
    ys, xs = np.arange(y0, y0 + h), np.arange(x0, x0 + w)
    for p in range(4):
        yy, xx = ys[(ys & 1) == (p >> 1)], xs[(xs & 1) == (p & 1)]  # frame coordinates decide the position
        if yy.size == 0 or xx.size == 0:
            continue
        for f in range(n):
            v = imgs[f][np.ix_(yy, xx)].astype(np.int64).ravel()
            b = np.minimum(v >> shift, bins - 1)
            s = v >= sat[p]
            out["hist"][f, p] += np.bincount(b, minlength=bins).astype(np.uint32)  # (uint32 adds wrap modulo 2^32)
            out["cnt"][f, p] += np.uint32(v.size)
            out["nsat"][f, p] += np.uint32(int(s.sum()))
            out["sum"][f, p] += np.uint64(int(v[~s].sum()))
            out["min"][f, p] = min(int(out["min"][f, p]), int(v.min()))
            out["max"][f, p] = max(int(out["max"][f, p]), int(v.max()))
    return out


def record(fields):
    """(N, 16 * B + 96) uint8: the records of the fields, as the library lays them out."""
    n, _, bins = fields["hist"].shape
    words = np.concatenate([fields[k].reshape(n, -1).astype("<u4") for k in ("hist", "cnt", "nsat", "min", "max")], axis=1)
    return np.concatenate([np.ascontiguousarray(words).view(np.uint8).reshape(n, -1),
                           np.ascontiguousarray(fields["sum"].astype("<u8")).view(np.uint8).reshape(n, -1)], axis=1)


def parse(raw, bins):
    """The fields of record bytes (N, 16 * B + 96) uint8."""
    raw = np.ascontiguousarray(raw)
    n = raw.shape[0]
    assert raw.shape[1] == record_bytes(bins)
    words = raw[:, :16 * bins + 64].copy().view("<u4")
    small = words[:, 4 * bins:]
    return {"hist": words[:, :4 * bins].reshape(n, 4, bins), "cnt": small[:, 0:4], "nsat": small[:, 4:8], "min": small[:, 8:12],
            "max": small[:, 12:16], "sum": raw[:, 16 * bins + 64:].copy().view("<u8")}


def helper_input(fields, bins, shift):
    """What the stats_* helpers take: the arrays on the CPU plus bins and shift."""
    d = dict(fields)
    d["bins"], d["shift"] = bins, shift
    return d
