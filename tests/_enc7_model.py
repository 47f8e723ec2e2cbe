"""A model of the type-7 encoder's two kernels (csrc/mcraw_encode7.hip) in numpy, and the corpus of its path tests.

From a batch -- a list of frames as frame() makes them -- it works out, without the library and without the synthesiser, what
k7e_payload and k7e_side must find and count: the geometry (tilesX, ntiles, nseg, R, and the batch's strides smax and rmax), every
block's class and ref with the edge padding of clamp_par, every segment's payload bytes, every side-stream record's header class
and ref, every counter of the kernels' path census that content decides (PATHS gives their order, enum PathE in the kernel
source), and the bytes a frame whose look-back failed may have touched.  tests/test_enc7_model.py holds the model against the
synthesiser on the CPU; tests/test_gpu_enc7_paths.py holds the kernels' census against the model.  TEST INFRASTRUCTURE."""
import numpy as np

from motioncam_decoder_amd.synthlib import natural_image_np, uniform_image_np

E_ARGS, E_CAPACITY, E_DEVICE = 0x1, 0x10, 0x100
LEN7 = np.array([0, 8, 16, 24, 32, 40, 48, 64, 64, 80, 80, 128, 128, 128, 128, 128, 128])
SEG_TILES, SIDE_RECS, WINDOW = 64, 256, 64

# The census, in the order of PathE.  k7e_payload first ...
PATHS = (["live", "idle", "hit", "refetched", "loads16", "loads_edge", "loads_clamped_row", "dead_tiles"]
         + ["class%d" % k for k in range(17)]
         + ["rows", "refs_clamped", "lookbacks", "windows", "words", "polls", "gave_up", "met_fail", "never",
            # ... then k7e_side
            "side_bad", "side_fail", "side_idle", "side_chunks"]
         + ["bits_rec%d" % k for k in range(16)] + ["refs_rec%d" % k for k in range(16)] + ["headers"])
# what timing decides (the parent's bounds hold for them, the model says nothing)
TIMING = ("hit", "refetched", "windows", "words", "polls", "gave_up", "met_fail", "never")
CONTENT = tuple(k for k in PATHS if k not in TIMING)
# content-driven counters that are zero in a batch of good frames
ONLY_BAD = ("side_bad", "side_fail")
# ... and those no input reaches: a bits stream's entries are classes, 0..16, so its records have the classes 0..5
UNREACHABLE = tuple("bits_rec%d" % k for k in range(6, 16))


def clamp_par(x, n):
    """Past the edge: the last index of the same parity (mcraw_synth_encode7's padding rule)."""
    x = np.asarray(x, np.int64)
    c = np.maximum((n - 1) - (((n - 1) ^ x) & 1), 0)
    return np.where(x < n, x, c)


def geometry(w, h):
    tiles_x, tiles_y = (w + 63) // 64, (h + 3) // 4
    ntiles = tiles_x * tiles_y
    return dict(w=w, h=h, tilesX=tiles_x, tilesY=tiles_y, ntiles=ntiles, nseg=(ntiles + SEG_TILES - 1) // SEG_TILES,
                R=(4 * ntiles + 63) // 64)


def bit_length(a):
    a = np.asarray(a, np.int64)
    return np.where(a > 0, np.floor(np.log2(np.maximum(a, 1))).astype(np.int64) + 1, 0)


def frame(img=None, bad=0, w=None, h=None, name=""):
    """One frame of a batch: an image, or a frame the host rejects (bad = E_ARGS / E_CAPACITY; the image is what it is given)."""
    if img is not None:
        img = np.ascontiguousarray(img, dtype=np.uint16)
        h, w = img.shape
    return dict(img=img, bad=bad, w=w, h=h, name=name)


class Frame:
    """What the kernels must make of one good frame."""

    def __init__(self, img):
        img = np.ascontiguousarray(img, dtype=np.uint16)
        h, w = img.shape
        self.__dict__.update(geometry(w, h))
        G = self
        pad = img[clamp_par(np.arange(4 * G.tilesY), h)][:, clamp_par(np.arange(64 * G.tilesX), w)].astype(np.int64)
        # [tile row, upper / lower half of the block, row parity, tile column, 32 sample pairs, column parity]
        a = pad.reshape(G.tilesY, 2, 2, G.tilesX, 32, 2)
        mn = a.min(axis=(1, 4)).transpose(0, 2, 1, 3).reshape(-1)  # block m = 4 tile + 2 row parity + column parity
        mx = a.max(axis=(1, 4)).transpose(0, 2, 1, 3).reshape(-1)
        self.nb = bit_length(mx - mn)  # class of every block
        self.ref = mn
        self.blen = LEN7[self.nb]
        seg_of_block = np.arange(4 * G.ntiles) // (4 * SEG_TILES)
        self.seg_bytes = np.bincount(seg_of_block, weights=self.blen, minlength=G.nseg).astype(np.int64)
        self.payload = int(self.blen.sum())
        # the side streams: entries padded with zeros to whole records
        ent = np.zeros((2, 64 * G.R), np.int64)
        ent[0, :4 * G.ntiles], ent[1, :4 * G.ntiles] = self.nb, self.ref
        ent = ent.reshape(2, G.R, 64)
        self.rec_min = ent.min(axis=2)
        self.rec_ref = np.minimum(self.rec_min, 4095)
        self.rec_hb = np.minimum(15, bit_length(ent.max(axis=2) - self.rec_ref))
        self.rec_len = 2 + LEN7[self.rec_hb]
        self.length = 16 + self.payload + 2 * 4 + int(self.rec_len.sum())
        # what the loads of a tile are, by its column and its row
        x0 = 64 * np.arange(G.tilesX)[:, None] + 8 * np.arange(8)[None, :]
        self.tile16 = 4 * (x0 + 8 <= w).sum(axis=1)  # per tile column: lanes with a 16-byte load (four rows of eight)
        self.tile_clamped = 8 * ((4 * np.arange(G.tilesY)[:, None] + np.arange(4)[None, :]) >= h).sum(axis=1)

    def seg_census(self, seg):
        """The content-driven counters of the workgroup of k7e_payload that takes segment `seg` (but `rows`: the caller knows
        whether the segment's rows are stored)."""
        c = dict.fromkeys(PATHS, 0)
        t = np.arange(seg * SEG_TILES, min((seg + 1) * SEG_TILES, self.ntiles))
        c["loads16"] = int(self.tile16[t % self.tilesX].sum())
        c["loads_edge"] = 32 * len(t) - c["loads16"]
        c["loads_clamped_row"] = int(self.tile_clamped[t // self.tilesX].sum())
        c["dead_tiles"] = SEG_TILES - len(t)
        for k, v in enumerate(np.bincount(self.nb[4 * t[0]: 4 * t[-1] + 4], minlength=17)):
            c["class%d" % k] = int(v)
        c["refs_clamped"] = int((self.rec_min[1, 4 * seg: 4 * seg + 4] > 4095).sum())
        return c

    def failed_range(self, lost_seg=3):
        """The bytes a frame may have touched whose segment `lost_seg` never published: the payload of the segments in front."""
        return 16, 16 + int(self.seg_bytes[:lost_seg].sum())


_frames = {}


def model_of(img):
    key = (img.shape, img.tobytes())
    if key not in _frames:
        _frames[key] = Frame(img)
    return _frames[key]


def strides(batch):
    good = [geometry(f["w"], f["h"]) for f in batch if not f["bad"]]
    return max([g["nseg"] for g in good] + [1]), max([g["R"] for g in good] + [1])


def census(batch, lost=False):
    """The content-driven counters of one encode of `batch`.  lost: a launch of the `lost` build at an odd epoch -- the workgroup
    of frame 0's segment 3 returns behind its ticket, every later segment of the frame gives up or meets a failure and stores
    nothing, and k7e_side writes nothing for the frame."""
    n = len(batch)
    smax, rmax = strides(batch)
    chunks = (rmax + SIDE_RECS - 1) // SIDE_RECS
    c = dict.fromkeys(CONTENT, 0)
    for i, f in enumerate(batch):
        if f["bad"]:
            c["side_bad"] += 2 * chunks
            continue
        F = model_of(f["img"])
        failed = lost and i == 0 and F.nseg > 4
        c["live"] += F.nseg
        for seg in range(F.nseg):
            if failed and seg == 3:
                continue
            for k, v in F.seg_census(seg).items():
                if k in c:
                    c[k] += v
            c["lookbacks"] += seg > 0
            if not (failed and seg > 3):
                c["rows"] += int(F.seg_bytes[seg]) // 8
        if failed:
            c["side_fail"] += 2 * chunks
            continue
        mine = (F.R + SIDE_RECS - 1) // SIDE_RECS
        c["side_idle"] += 2 * (chunks - mine)
        c["side_chunks"] += 2 * (mine - 1)
        c["headers"] += 1
        for s, what in enumerate(("bits_rec%d", "refs_rec%d")):
            for k, v in enumerate(np.bincount(F.rec_hb[s], minlength=16)):
                c[what % k] += int(v)
    c["idle"] = n * smax - c["live"]
    return c


def word_bounds(batch, lost=False):
    """(fewest, most) predecessor words the look-backs of one encode add up: every look-back that ends well adds one at least
    (the word in front of it), none more than the segments in front.  A look-back that gives up may have added none."""
    lo = hi = 0
    for i, f in enumerate(batch):
        if f["bad"]:
            continue
        nseg = geometry(f["w"], f["h"])["nseg"]
        lo += 2 if lost and i == 0 and nseg > 4 else nseg - 1  # (segments 1 and 2 in front of the lost one)
        hi += nseg * (nseg - 1) // 2
    return lo, hi


def windows_aggonly(batch):
    """Fewest windows when no segment ever publishes a prefix: every look-back walks to segment 0, 64 words a window."""
    return sum(sum((seg + WINDOW - 1) // WINDOW for seg in range(1, geometry(f["w"], f["h"])["nseg"])) for f in batch if not f["bad"])


# ---------------------------------------------------------------------------------------------------- the corpus

def set_block(img, ty, tx, b, vals):
    i = np.arange(64)
    img[4 * ty + (b >> 1) + 2 * (i >> 5), 64 * tx + 2 * (i & 31) + (b & 1)] = np.asarray(vals).astype(np.uint16)


def block_of_class(nb, lo, rng):
    """64 samples whose range is exactly 2^nb - 1 above `lo`."""
    span = (1 << nb) - 1
    vals = lo + rng.integers(0, span + 1, size=64)
    if span:
        vals[0], vals[1] = lo, lo + span
    return vals


def classes_image(w=256, h=64, seed=5):
    """Blocks of every class 0..16: block m of the frame (tile order) gets the range 2^(m % 17) - 1 (0 for class 0)."""
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w), dtype=np.uint16)
    tiles_x = (w + 63) // 64
    m = 0
    for ty in range(h // 4):
        for tx in range(tiles_x):
            for b in range(4):
                nb = m % 17
                lo = int(rng.integers(0, 65536 - (1 << nb) + 1)) if nb < 16 else 0
                span = (1 << nb) - 1
                vals = lo + rng.integers(0, span + 1, size=64) if span else np.full(64, lo)
                if span:
                    vals[0], vals[1] = lo, lo + span
                set_block(img, ty, tx, b, vals)
                m += 1
    return img


RECORD_CLASSES = [(3, 0), (3, 1), (2, 3), (1, 7), (0, 15), (0, 16), (16, 0), (11, 5)]  # (lowest block class, spread) of a record


def records_image(seed=7):
    """1024 x 112: 16 tiles = 64 blocks = one record of each side stream per tile row, 28 records.
      0..15   flat blocks whose values span 2^k - 1 above a base (100 up to k = 11, 0 above): refs records of class k
      16..19  flat blocks at 4095 / 4096 / 50000 + 0..7 / 65535: the refs record's 12-bit ref at, one above and far above its clamp
      20..27  blocks of the classes floor .. floor + spread of RECORD_CLASSES: bits records of the classes 0..5"""
    rng = np.random.default_rng(seed)
    img = np.zeros((112, 1024), dtype=np.uint16)

    def record(r, blocks):
        for j, vals in enumerate(blocks):
            set_block(img, r, j // 4, j % 4, vals)

    for k in range(16):
        base, span = (100 if k <= 11 else 0), (1 << k) - 1
        record(k, [np.full(64, base + j * span // 63) for j in range(64)])
    record(16, [np.full(64, 4095)] * 64)
    record(17, [np.full(64, 4096)] * 64)
    record(18, [np.full(64, 50000 + j % 8) for j in range(64)])
    record(19, [np.full(64, 65535)] * 64)
    for r, (floor, spread) in enumerate(RECORD_CLASSES):
        nbs = [floor + j % (spread + 1) for j in range(64)]
        record(20 + r, [block_of_class(nb, 1000 if nb < 16 else 0, rng) for nb in nbs])
    return img


SHAPES = [(1, 1), (2, 2), (3, 5), (63, 3), (64, 4), (65, 5), (127, 7), (200, 100)]
KINDS = ["nat10", "nat12", "nat14", "uni8", "uni12", "uni16", "zero", "max", "highref"]


def content(kind, w, h, seed):
    if kind.startswith("nat"):
        return natural_image_np(w, h, int(kind[3:]), 8.0, seed)
    if kind.startswith("uni"):
        return uniform_image_np(w, h, int(kind[3:]), seed)
    if kind == "zero":
        return np.zeros((h, w), dtype=np.uint16)
    if kind == "max":
        return np.full((h, w), 65535, dtype=np.uint16)
    if kind == "highref":  # refs above 4095 (the side stream's 12-bit ref clamp) with small ranges
        return (np.uint16(50000) + uniform_image_np(w, h, 6, seed)).astype(np.uint16)
    raise ValueError(kind)


BIG65 = ("nat12", 1024, 1028, 31)    # 4112 tiles: nseg 65 (one segment behind the first window), R 257 (one record in chunk 1)
BIG130 = ("uni8", 1024, 2068, 32)    # nseg 130, R 517: three windows, three chunks
NARROW = ("nat12", 4, 4100, 33)      # one tile per tile row, nseg 17: every load is a right-edge load

_corpus = []


def corpus():
    """The frames, made once: [frame()], the names unique."""
    if not _corpus:
        _corpus.append(frame(records_image(), name="records"))
        _corpus.append(frame(classes_image(), name="classes"))
        for kind in KINDS:
            for i, (w, h) in enumerate(SHAPES):
                _corpus.append(frame(content(kind, w, h, 11 + i), name="%s %dx%d" % (kind, w, h)))
        for kind, w, h, seed in (BIG65, BIG130, NARROW):
            _corpus.append(frame(content(kind, w, h, seed), name="%s %dx%d" % (kind, w, h)))
    return list(_corpus)


def by_name(name):
    return next(f for f in corpus() if f["name"] == name)


def batches():
    """[(name, [frame()])] in the order the child encodes them on ONE context: all frames at once (uneven nseg against smax: idle
    workgroups in both kernels), the reverse order, every frame alone, big / 1 x 1 alone / big (the strides shrink and grow over
    stale workspace), and good frames with one the host rejects for its arguments and one for its capacity among them."""
    K = corpus()
    big, tiny = by_name("uni8 1024x2068"), by_name("zero 1x1")
    out = [("all", K), ("reversed", K[::-1])]
    out += [("alone " + f["name"], [f]) for f in K]
    out += [("seq big", [big]), ("seq tiny", [tiny]), ("seq big again", [big])]
    rec, small = by_name("records"), by_name("nat12 200x100")
    out.append(("bad among good", [rec, frame(small["img"], bad=E_ARGS, w=0, h=100, name="E_ARGS"), small,
                                   frame(small["img"], bad=E_CAPACITY, name="E_CAPACITY"), by_name("nat12 4x4100")]))
    return out


def lost_batches():
    """The batches of the `lost` build, on one context: odd, even, odd, even epochs.  Frame 0 is the 1024 x 1028 frame."""
    big, rec, small = by_name("nat12 1024x1028"), by_name("records"), by_name("nat12 200x100")
    b = [big, rec, small, by_name("uni8 1024x2068")]
    return [("lost 1", b), ("lost 2", b), ("lost 3", [big, small]), ("lost 4", [big, small])]


def plan(variant):
    """[(name, batch, host, lost)] that the child of `variant` encodes, in this order, on ONE context.  host: in MCRAW_MEM_HOST
    (the others are device-resident with len_out); lost: a launch in which the `lost` build drops frame 0's segment 3."""
    if variant == "lost":  # the host batch is the context's fifth: an odd epoch again
        lb = lost_batches()
        return [(name, b, False, i % 2 == 0) for i, (name, b) in enumerate(lb)] + [("lost 5 host", lb[0][1], True, True)]
    if variant == "wrap":  # (epochs 0xFFFFFFFE, 0xFFFFFFFF, 1, 2, 3)
        b = [by_name("nat12 1024x1028"), by_name("records"), by_name("nat12 200x100"), by_name("nat12 4x4100")]
        return [("wrap %d" % k, b, False, False) for k in range(1, 6)]
    return [(name, b, False, False) for name, b in batches()] + [("all host", corpus(), True, False)]
