"""Legacy (type 6) content for the tests: the generators of the parity and fuzz suites, and a compact corpus made of them.

The corpus (corpus(), built on the CPU, deterministic) is what tests/test_gpu_k6_paths.py decodes with every forced-path
build of k6_decode.  k6_decode works on segments of 16 KiB of stream, looks back over windows of 8 (scalar polls) and 16
(vector polls) segments, and chooses its paths by content; so the corpus holds
  * frames of exactly 1, 2, 7, 8, 9, 16, 17, 33 and more than 48 segments, among them streams that end one, three or five
    bytes in front of or behind a segment's start (fit6 / sized: records are given one more bit until the length is the one asked for);
  * natural 12-bit frames, 14-bit noise, a flat and a half-clipped frame, flat and textured bands, one record size per frame
    (nibbles 0, 1, 2, 5, 10 and raw 16-bit), mixed sizes around the list thresholds (352, 736 and 768 records per wave), the stream
    whose 17 chains never meet, one whose chains meet only INSIDE a segment (the late front), a stream cut inside a late
    segment, a width off the 32 grid and a height off the 4 grid;
  * single-byte mutants of two of the frames (the fuzz suite's mutator, fixed seeds).
About 5 MB of stream (310 segments) and 5 MP in 35 frames.  What a frame must decode to is the oracle's business (expectations())."""
import functools

import numpy as np

import _libs as L

SEG6 = 16384      # bytes of stream per k6_decode workgroup (SEG_CHUNKS6 chunks of CHUNK6 bytes, csrc/mcraw_plan.h)
CHUNK6 = 1024


def segments(nbytes):
    """Workgroups k6_decode is launched with for a stream of `nbytes` (csrc/mcraw_submit.hip: whole chunks, then whole segments)."""
    return ((nbytes + CHUNK6 - 1) // CHUNK6 + 15) // 16


def full_segments_with_predecessor(nbytes):
    """Segments other than the first that hold all their 16 chunks: the ones that publish an exit phase or a map for a successor."""
    return max(0, (nbytes + CHUNK6 - 1) // CHUNK6 // 16 - 1)


# ---------------------------------------------------------------- generators (shared with test_gpu_parity.py / test_gpu_fuzz.py)

def one_size_frame(rng, nib, w, h):
    """Every record of the frame has header nibble `nib` (0..10: that many bits per sample; above: raw 16-bit).  -> (img, min_bits)"""
    nb = nib if nib <= 10 else 16
    img = rng.integers(0, 1 << max(nb, 1), size=(h, w), dtype=np.uint16) if nb else np.full((h, w), 321, np.uint16)
    nrec = ((w + 31) // 32) * 2 * h
    return img, np.full(nrec, nib, np.uint8)


def mixed_size_image(rng, nibs, w, h):
    """Records drawn from the sizes `nibs`, changing in runs of 1 .. 400 records (w a multiple of 32)."""
    rpr = w // 32 * 2                                           # records per row
    nrec = rpr * h
    run = rng.integers(1, 400, size=nrec)                      # sizes change in runs of 1 .. 400 records
    idx = np.repeat(np.arange(nrec), run)[:nrec] % len(nibs)
    nib = np.asarray(nibs, np.int64)[rng.permutation(len(nibs))][idx].reshape(h, w // 32, 2)
    # record (y, g, p) holds the samples of columns 32 g + 2 i + p: residuals of nib[y, g, p] bits above a common reference
    bits = np.repeat(nib, 16, axis=1).reshape(h, w // 32, 16, 2).reshape(h, w)
    return (100 + (rng.random((h, w)) * (1 << bits)).astype(np.int64)).astype(np.uint16)


def banded_image(rng, w, h, band):
    """Bands of `band` constant rows between bands of 12-bit noise: runs of 2-byte records between long ones."""
    img = rng.integers(0, 4096, size=(h, w), dtype=np.uint16)
    for y0 in range(0, h, 2 * band):
        img[y0:y0 + band] = 517
    return img


def never_unanimous_image(w, h):
    """Payload bytes that read as headers of the same record size: the constant 0xBFFF is coded with the reference 0xFFF and raw
    residuals 0xB000, so every even byte of the stream -- the headers' 0xFF and the payload's 0xB0 -- has a nibble >= 11 = "raw
    record, 34 bytes": all 17 phases are chains of their own that never meet."""
    return np.full((h, w), 0xBFFF, np.uint16)


def cut_inside_late_segment(good):
    """The stream's first two thirds, ending in the middle of a record."""
    return good[: (good.size * 2 // 3) | 1].copy()


def mutants(buf, rng, n, hot=(), flips=None):
    """`n` copies of `buf` with 1 .. 3 (or `flips`) bytes replaced by random ones, half of them inside the `hot` ranges."""
    out = []
    for i in range(n):
        b = buf.copy()
        k = int(rng.integers(1, 4)) if flips is None else flips
        for _ in range(k):
            if hot and rng.random() < 0.5:
                lo, hi = hot[int(rng.integers(0, len(hot)))]
                pos = int(rng.integers(lo, min(hi, b.size)))
            else:
                pos = int(rng.integers(0, b.size))
            b[pos] = rng.integers(0, 256)
        out.append(b)
    return out


# ---------------------------------------------------------------- streams of a chosen length

def record_nibbles(buf, nrec):
    """Header nibbles of the stream's first `nrec` records, and the byte behind the last of them."""
    b = buf.tobytes()
    nib = np.empty(nrec, np.uint8)
    o = 0
    for i in range(nrec):
        n = b[o] >> 4
        nib[i] = n
        o += 2 * n + 2 if n <= 10 else 34
    return nib, o


def fit6(img, nbytes):
    """encode6(img) made exactly `nbytes` long (odd: the records are even and one byte ends the stream): records of at most 9 bits
    per sample get a bit more, two bytes each, spread evenly over the frame."""
    h, w = img.shape
    nrec = ((w + 31) // 32) * 2 * h
    buf = L.encode6(img)
    nib, end = record_nibbles(buf, nrec)
    assert end + 1 == buf.size and (nbytes - buf.size) % 2 == 0 and nbytes >= buf.size, (buf.size, nbytes)
    k = (nbytes - buf.size) // 2
    while k:
        e = np.flatnonzero(nib <= 9)
        assert e.size, "no record left that can grow"
        take = np.unique(e[np.linspace(0, e.size - 1, min(k, e.size)).astype(np.int64)])
        nib[take] += 1
        k -= take.size
    buf = L.encode6(img, nib)
    assert buf.size == nbytes, (buf.size, nbytes)
    return buf


def sized(big, nbytes, hmod=None):
    """The first rows of `big` -- as many as fit `nbytes` of stream (hmod: a height with h % 4 == hmod) --, then fit6.  -> (img, buf)"""
    H, w = big.shape
    rpr = ((w + 31) // 32) * 2
    nib, _ = record_nibbles(L.encode6(big), rpr * H)
    size = np.where(nib <= 10, 2 * nib.astype(np.int64) + 2, 34).reshape(H, rpr).sum(axis=1)
    cum = np.cumsum(size)
    h = int(np.searchsorted(cum, nbytes - 1, side="right"))
    while hmod is not None and h % 4 != hmod:
        h -= 1
    assert 0 < h < H, (h, H)
    img = np.ascontiguousarray(big[:h])
    return img, fit6(img, nbytes)


# ---------------------------------------------------------------- which way the sure entry of a segment goes (a model of k6_decode's)

def front_kinds(buf):
    """For every segment with a predecessor: 0 -- the 17 chains that can cross into the KiB in front of it are one at its start --,
    the quarter (of 256 bytes) inside it at which they become one, or None when they never do.  Plain Python, for the CPU tests."""
    b = buf.tobytes()
    n = len(b)

    def walk(p, bound):  # -> first record start at or behind `bound`, None for a chain that ends in front of it
        while p < bound:
            nb = (b[p] if p < n else 0) >> 4
            t = 2 * nb + 2 if nb <= 10 else 34
            if p + t >= n:
                return None
            p += t
        return p

    kinds = []
    for s in range(1, segments(n)):
        start = s * SEG6
        cnt = min(16, (n + CHUNK6 - 1) // CHUNK6 - 16 * s)
        ps = [walk(start - CHUNK6 + 2 * i, start) for i in range(17)]
        kind = None
        for kb in range(4 * cnt):
            ps = [None if p is None else walk(p, start + 256 * kb) for p in ps]
            if len({p for p in ps if p is not None}) <= 1:
                kind = kb
                break
        kinds.append(kind)
    return kinds


# ---------------------------------------------------------------- the corpus

def _half_clipped(w, h, seed):
    img = L.natural_image_np(w, h, 12, 12.0, seed)
    img[:, w // 2:] = 4095  # the right half of every row: 2-byte records
    return img


def _late_front(w, rows_apart, rows_noise, seed):
    """Rows of the never-meeting constant, then noise: the chains become one where the noise begins -- `rows_apart` rows of
    w / 16 records of 34 bytes into the stream, chosen to lie INSIDE a segment."""
    img = np.random.default_rng(seed).integers(0, 4096, size=(rows_apart + rows_noise, w), dtype=np.uint16)
    img[:rows_apart] = 0xBFFF
    return img


@functools.lru_cache(maxsize=1)
def corpus():
    """-> list of dicts: name, w, h, buf, img (None for a stream that is not an image's), segs (the count the frame was made for, or
    None), whole (an unmutated, uncut stream: must decode to img with status 0)."""
    out = []

    def add(name, img, buf, segs=None, whole=True):
        h, w = img.shape
        out.append(dict(name=name, w=w, h=h, buf=buf, img=img if whole else None, segs=segs, whole=whole))

    def add_sized(name, big, nbytes, hmod=None):
        img, buf = sized(big, nbytes, hmod)
        add(name, img, buf, segs=segments(nbytes))

    # segment counts around the look-back windows; lengths around segment starts
    add_sized("nat12 w200 1 segment", L.natural_image_np(200, 200, 12, 12.0, 11), 15001)            # a width off the 32 grid
    add_sized("nat12 h%4=3 2 segments", L.natural_image_np(512, 120, 12, 12.0, 12), 2 * SEG6 - 3, hmod=3)
    rng = np.random.default_rng(14)
    img = rng.integers(0, 1 << 14, size=(80, 640), dtype=np.uint16)                                  # 80 rows of 40 raw records: 108 801 bytes
    add("noise14 7 segments", img, L.encode6(img), segs=7)
    add_sized("nat12 8 segments, ends 3 bytes short", L.natural_image_np(1024, 200, 12, 12.0, 13), 8 * SEG6 - 3)
    add_sized("nat12 9 segments, ends 5 bytes in", L.natural_image_np(1024, 200, 12, 12.0, 15), 8 * SEG6 + 5)
    add_sized("half-clipped 16 segments, ends 1 byte short", _half_clipped(1024, 700, 16), 16 * SEG6 - 1)
    add_sized("bands w1000 17 segments, ends 1 byte in", banded_image(np.random.default_rng(17), 1000, 600, 10), 16 * SEG6 + 1)
    add_sized("nat12 33 segments", L.natural_image_np(1024, 700, 12, 12.0, 18), 33 * SEG6 - 4001)
    img = np.random.default_rng(19).integers(0, 1 << 14, size=(512, 1024), dtype=np.uint16)
    add("noise14 1024x512", img, L.encode6(img), segs=69)                                            # 32 768 raw records and the byte that ends the stream: 68 segments + 1 byte
    # one record size per frame, two to three segments each
    rng = np.random.default_rng(66)
    for nib in (0, 1, 2, 5, 10, 15):
        nb = nib if nib <= 10 else 16
        w = 1024 + 32 * nib
        h = int(2.5 * SEG6 / (2 + 2 * nb) * 16 / w) + 1 + nib
        img, mb = one_size_frame(rng, nib, w, h)
        add("records of nibble %d" % nib, img, L.encode6(img, mb))
    img = np.full((37, 1000), 4095, np.uint16)
    add("flat 1000x37", img, L.encode6(img))
    # mixed sizes around the list thresholds
    rng = np.random.default_rng(606)
    for nibs, w in (((4, 5, 6), 1504), ((1, 2, 3), 2016), ((0, 1, 2), 992), ((2, 12), 1184)):
        img = mixed_size_image(rng, nibs, w, 130)
        add("mixed nibbles %s" % (nibs,), img, L.encode6(img))
    # chains that never meet; chains that meet inside segment 1 (5 rows of 120 raw records = 20 400 bytes: 4016 into it)
    img = never_unanimous_image(960, 100)
    add("never unanimous", img, L.encode6(img))
    img = _late_front(1920, 5, 25, 23)
    add("late front", img, L.encode6(img))
    # a stream cut inside a late segment
    img = L.natural_image_np(1920, 160, 12, 12.0, 31)
    add("cut inside a late segment", img, cut_inside_late_segment(L.encode6(img)), whole=False)
    # single-byte mutants of two frames
    for k, seed in ((1, 6601), (3, 6602)):
        f = out[k]
        for j, b in enumerate(mutants(f["buf"], np.random.default_rng(seed), 6, flips=1)):
            out.append(dict(name="%s, mutant %d" % (f["name"], j), w=f["w"], h=f["h"], buf=b, img=None, segs=None, whole=False))
    return out


def expectations():
    """The oracle's word on every frame of the corpus: [(ret, pixels)].  HIP must agree by the fuzz suite's rule: ret == 0 -- a
    nonzero status and nothing written --, else status 0, `ret` written and the first ret // w rows equal."""
    return [L.oracle_decode6(f["buf"], f["w"], f["h"]) for f in corpus()]
