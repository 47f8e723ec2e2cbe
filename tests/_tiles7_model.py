"""k7_tiles for the tests: a plain model of what content and geometry decide in it, and a compact corpus made for its paths.

k7_tiles (csrc/mcraw_type7.hip) gives one wave a decode ITEM -- 32 payload blocks, 8 tiles of 64 x 4 pixels --: the wave reads
the blocks' bit widths and references, stages the item's payload span in its LDS slice, unpacks every block by its storage class
and stores 8-sample pieces of rows in one of several forms.  Nothing in it depends on timing, so census() below predicts every
counter of the kernel's path census (-DMCRAW_PATHST, enum PathT; PATHS has the names in its order) EXACTLY, from the frame buffers
and the call's parameters alone: width, height, the output address modulo 16, the stage behind the decode, the black levels, which
frames share a batch and MCRAW_XCD_CHUNK.  It holds as plain Python what the kernel and the host take for granted of each other:
len7_of / cls7_of, the item / tile / lane geometry, post_fast_align and the `fast_store` rule of csrc/mcraw_submit.hip, the lean
decision of the strip instances, the rule of the merged 14-bit store, and the size-class cut of a batch -- of the latter only what
it guarantees: plans sorted by their group count, a frame joins the class in front while 5 g >= 4 G.  Bit widths and references
come from the side streams as their writer meant them (_side7_corpus.parse_stream); decode_np() decodes a frame from them in
numpy, which tests/test_tiles7_model.py holds against the oracle, so the model's view of a frame is the oracle's.

The corpus (corpus(), built on the CPU, deterministic; 30 frames, 0.26 MP):
  * `pairs`: 640 x 116, 290 tiles: every one of the 17 x 17 pairs of bit widths (0 .. 16) in the sibling pairs (0, 1) and (2, 3)
    of one tile, every block with residuals that use its width to the full (the classes of a pair meet in one lane's two unpacks);
  * geometry: widths 64, 128, 200, 576, 1000 (crop inside a tile, width % 8 == 0), 77 and 1001 (width % 8 != 0: no piece on the
    fast grid, an odd last sample), 66 (the planes layout's cropped end); heights 4, 6, 10, 37 (rows end inside a tile row:
    y >= rows, y + 2 >= rows); one to nine tile columns (and 16) for the merged store's neighbours; a frame coded shorter than asked;
  * lean, one frame per reason an item is not lean, each failing for that reason ALONE in the setting named for it (LEAN_ALONE;
    alone_report() confirms it): 16-bit noise (raw blocks), dark blocks under black levels 64 .. 4000, 14-bit content in 10- and
    12-bit strips, values >= 65400 under black levels >= 50000 (the reference add could wrap, the strip's top holds); and two natural
    frames that are lean throughout, one of them above the black levels of the settings that have them;
  * `wrap`: references re-laid (emit_stream / assemble) so that reference + residual passes 65535: the oracle wraps, RawData.cpp:492;
  * spans: all-zero blocks (no payload at all), 32 raw blocks behind an 8-byte block (a full span at head 8: PAY_CHUNKS chunks),
    frames whose last item holds fewer than 32 blocks;
  * a mixed batch: 320 x 64 (5 groups) with two frames of 256 x 64 (4 groups) in one size class: items beyond a frame.
Every frame is decoded alone, the mixed batch as one batch.  What a frame must decode to is the oracle's business (expectations()).
"""
import functools

import numpy as np

import _float_ref as FR
import _libs as L
import _side7_corpus as K

ITEM_BLOCKS, ITEM_TILES, PAY_CHUNKS = 32, 8, 4096 // 16 + 1

# the order of PathT in csrc/mcraw_type7.hip
PATHS = (["waves", "invalid", "short", "tiles_skipped", "span_empty", "span_full", "head", "wg_remap", "wg_chunked"]
         + ["cls%d" % c for c in range(10)]
         + ["pair_diff", "wrap_lanes", "lean", "notlean", "fail_bits", "fail_ref", "fail_top", "fail_wrap",
            "drop_y", "drop_x", "st_aligned", "st_unaligned", "st_cropped", "st_merged_fwd", "st_merged_back",
            "decl_partial", "decl_notin"])

BLACK = (64, 200, 1000, 4000)
HIGH_BLACK = (50000, 50100, 50200, 50300)
WHITE = 16383.0

# The child's settings, one context each: name -> dict(env, stage, off: output address modulo 16, only / skip: frames by tag).
# stage: None (the plain mosaic), ("post", kwargs of Context.set_post) or ("float", kwargs of Context.set_float_out).
SETTINGS = {
    "plain": dict(),
    "plain off2": dict(off=2),
    "u16 black": dict(stage=("post", dict(black=BLACK))),
    "p12": dict(stage=("post", dict(bits=12))),
    "p12 black": dict(stage=("post", dict(bits=12, black=BLACK))),
    "p12 off2": dict(stage=("post", dict(bits=12)), off=2),
    "p10": dict(stage=("post", dict(bits=10))),
    "p10 black": dict(stage=("post", dict(bits=10, black=BLACK))),
    "p14": dict(stage=("post", dict(bits=14))),
    "p14 black": dict(stage=("post", dict(bits=14, black=BLACK))),
    "p14 off2": dict(stage=("post", dict(bits=14)), off=2),
    "p14 highblack": dict(stage=("post", dict(bits=14, black=HIGH_BLACK)), only="lean"),
    "f32 mosaic": dict(stage=("float", dict(dtype="f32", white=WHITE, layout="mosaic", black=BLACK))),
    "f16 planes clip": dict(stage=("float", dict(dtype="f16", white=WHITE, layout="planes", black=BLACK, clip=True, plane=(2, 0, 3, 1))), even=True),
    "bf16 mosaic clip": dict(stage=("float", dict(dtype="bf16", white=WHITE, layout="mosaic", black=BLACK, clip=True))),
    "f32 planes": dict(stage=("float", dict(dtype="f32", white=WHITE, layout="planes")), even=True),
    "plain xcd0": dict(env={"MCRAW_XCD_CHUNK": "0"}, xcd=0),
    "plain xcd3": dict(env={"MCRAW_XCD_CHUNK": "3"}, xcd=3),
    "plain split22": dict(env={"MCRAW_SIDE_SPLIT": "2,2", "MCRAW_SIDE_LASTC": "1"}),
}
ENV_KEYS = ("MCRAW_XCD_CHUNK", "MCRAW_SIDE_SPLIT", "MCRAW_SIDE_LASTC")

# lean frame -> (the setting in which it is not lean for ONE reason, that reason's counter)
LEAN_ALONE = {"lean raw": ("p14", "fail_bits"), "lean dark": ("p14 black", "fail_ref"), "lean top12": ("p12", "fail_top"),
              "lean top10": ("p10", "fail_top"), "lean high": ("p14 highblack", "fail_wrap")}
FAILS = ("fail_bits", "fail_ref", "fail_top", "fail_wrap")

# counter -> settings in which the corpus must drive it above zero in the `census` build (every counter of PATHS is in here)
STRIPS = ("p12", "p12 black", "p10", "p10 black", "p14", "p14 black")
ALL = tuple(SETTINGS)
WIDE = tuple(s for s in SETTINGS if s != "p14 highblack")  # (the settings that take the whole corpus; the planes: its even frames)
DRIVEN = {
    "waves": ALL, "invalid": WIDE, "short": WIDE, "tiles_skipped": WIDE, "span_empty": WIDE, "span_full": WIDE, "head": WIDE,
    "wg_remap": ("plain xcd0",), "wg_chunked": tuple(s for s in ALL if s != "plain xcd0"),
    **{"cls%d" % c: WIDE for c in range(10)}, "pair_diff": WIDE, "wrap_lanes": WIDE,
    "lean": STRIPS, "notlean": STRIPS + ("p14 highblack",), "fail_bits": STRIPS, "fail_ref": ("p12 black", "p10 black", "p14 black"),
    "fail_top": STRIPS, "fail_wrap": ("p14 highblack",) + STRIPS,
    "drop_y": WIDE, "drop_x": WIDE, "st_aligned": tuple(s for s in WIDE if s not in ("plain off2", "p12 off2")),  # (off their grid by 2 bytes)
    "st_unaligned": WIDE, "st_cropped": WIDE,
    "st_merged_fwd": ("p14", "p14 black", "p14 off2"), "st_merged_back": ("p14", "p14 black", "p14 off2"),
    "decl_partial": ("p14", "p14 black", "p14 off2"), "decl_notin": ("p14", "p14 black", "p14 off2"),
}


def len7_of(b):
    b = np.asarray(b, np.int64)
    return np.where(b <= 6, 8 * b, np.where(b <= 8, 64, np.where(b <= 10, 80, 128)))


def cls7_of(b):
    b = np.asarray(b, np.int64)
    return np.where(b <= 6, b, np.where(b <= 8, 7, np.where(b <= 10, 8, 9)))


def storage_width(b):
    b = np.asarray(b, np.int64)
    return np.where(b <= 6, b, np.where(b <= 8, 8, 10))


def fast_align(kind, planes):
    """post_fast_align (csrc/mcraw_plan.h)."""
    if kind in ("f32", "f16", "bf16"):
        return 8 if planes and kind != "f32" else 16
    return {12: 4, 10: 2, 14: 2}.get(kind, 16)


def stage_of(setting):
    """-> (kind: 0 plain, 16 / 12 / 10 / 14, "f32" / "f16" / "bf16"; black levels or None; planes)"""
    st = SETTINGS[setting].get("stage")
    if st is None:
        return 0, None, False
    if st[0] == "post":
        return int(st[1].get("bits") or 16), st[1].get("black"), False
    return st[1]["dtype"], st[1].get("black", (0, 0, 0, 0)), st[1].get("layout", "planes") == "planes"


# ---------------------------------------------------------------- a frame as its side streams describe it

class Parsed:
    def __init__(self, buf):
        self.encW, self.encH, _, _ = K.header(buf)
        self.nblk = K.geometry(buf)[0]
        self.tilesX = self.encW // 64
        self.bits = K.parse_stream(buf, 0)[1][:self.nblk].astype(np.int64)
        self.refs = K.parse_stream(buf, 1)[1][:self.nblk].astype(np.int64)
        assert self.bits.max() <= 16
        # payload: block after block from byte 16 on (RawData.cpp:562, 576-579)
        ln = len7_of(self.bits)
        self.cum = 16 + np.concatenate([[0], np.cumsum(ln)])
        self.res = np.zeros((self.nblk, 64), np.int64)  # residuals, sample i of a block in the reference's order
        b8 = np.frombuffer(buf.tobytes(), np.uint8)
        layout = np.where(self.bits <= 6, self.bits, np.where(self.bits <= 8, 8, np.where(self.bits <= 10, 10, 15)))  # (7/8, 9/10, 11.. share one)
        for nib in (1, 2, 3, 4, 5, 6, 8, 10, 15):
            idx = np.flatnonzero(layout == nib)
            if not idx.size:
                continue
            n = K.LEN7[nib]
            raw = b8[self.cum[idx][:, None] + np.arange(n)[None, :]]
            bit = np.unpackbits(raw, axis=1, bitorder="little").astype(np.int64)
            self.res[idx] = (bit[:, K._bitmap(nib)] << np.arange(K.WIDTH[nib], dtype=np.int64)).sum(axis=2)


_parsed = {}


def parse(buf):
    key = id(buf)
    if key not in _parsed:
        _parsed[key] = (buf, Parsed(buf))  # (the buffer is kept: its id stays its own)
    return _parsed[key][1]


def block_image(vals, tilesX):
    """[nblk, 64] samples per block -> the coded image (RawData.cpp:581-593: block k of a tile is row parity k >> 1, column parity
    k & 1; sample i sits in row 2 (i >> 5) of that parity, column 2 (i & 31))."""
    nblk = vals.shape[0]
    tilesY = nblk // 4 // tilesX
    img = np.zeros((4 * tilesY, 64 * tilesX), vals.dtype)
    v = vals.reshape(tilesY, tilesX, 4, 2, 32)  # ty, tx, block, row of the parity, column of the parity
    for k in range(4):
        for half in range(2):
            rows = img[(k >> 1) + 2 * half::4, (k & 1)::2]                 # [tilesY, 32 * tilesX]
            rows[:, :] = v[:, :, k, half, :].reshape(tilesY, 32 * tilesX)
    return img


def decode_np(buf, w, h):
    """The frame decoded from the parsed bit widths, references and payload: the rows the decoder keeps, [min(h, encH), w]."""
    P = parse(buf)
    img = block_image(((P.res + P.refs[:, None]) & 0xFFFF).astype(np.uint16), P.tilesX)
    return img[:min(h, P.encH), :w]


# ---------------------------------------------------------------- the census

def ngroups_planned(w, h):
    """Plan7::ngroups: from the caller's width x height (csrc/mcraw_submit.hip)."""
    return (4 * ((w + 63) // 64) * ((h + 3) // 4) + 63) // 64


def size_classes(groups):
    """Frames by their planned groups -> [(frame indices, groups of the class)]: sorted by groups, descending and stable; a frame
    opens a class when 5 g < 4 G for the class in front (and there are fewer than 8)."""
    order = sorted(range(len(groups)), key=lambda i: -groups[i])
    out = []
    for i in order:
        if not out or (groups[i] * 5 < out[-1][1] * 4 and len(out) < 8):
            out.append(([], groups[i]))
        out[-1][0].append(i)
    return out


def lean_conditions(P, kind, black):
    """Per block, the four conditions of the strip instances as integers: -> dict of bool arrays (True: the block FAILS it)."""
    bl = np.asarray(black if black is not None else (0, 0, 0, 0), np.int64)[np.arange(P.nblk) & 3]
    top = (1 << storage_width(P.bits)) - 1
    return bl, dict(fail_bits=P.bits > 10, fail_ref=P.refs < bl, fail_top=P.refs - bl + top > (1 << kind) - 1, fail_wrap=P.refs + top > 65535)


def frame_census(f, kind, black, planes, off, variant):
    """What one valid frame adds to the census beyond its launch (waves, invalid items and workgroups are the batch's)."""
    P = parse(f["buf"])
    c = dict.fromkeys(PATHS, 0)
    w, rows = f["w"], min(f["h"], P.encH)
    nitems = (P.nblk + ITEM_BLOCKS - 1) // ITEM_BLOCKS
    ntiles = P.nblk // 4
    item_of = np.arange(P.nblk) // ITEM_BLOCKS
    # ---- items and their spans
    lo = np.arange(nitems) * ITEM_BLOCKS
    hi = np.minimum(lo + ITEM_BLOCKS, P.nblk)
    start, end = P.cum[lo], P.cum[hi]
    base16 = start & ~15
    n16 = np.minimum((end - np.minimum(end, base16) + 15) >> 4, PAY_CHUNKS)
    c["short"] = int((hi - lo < ITEM_BLOCKS).sum())
    c["tiles_skipped"] = nitems * ITEM_TILES - ntiles
    c["span_empty"] = int((n16 == 0).sum())
    c["span_full"] = int((n16 == PAY_CHUNKS).sum())
    c["head"] = int((start != base16).sum())
    # ---- blocks
    cls = cls7_of(P.bits)
    for k in range(10):
        c["cls%d" % k] = int((cls == k).sum())
    c["pair_diff"] = int((cls[0::2] != cls[1::2]).sum())
    # ---- lean (the strip instances)
    ref_used = P.refs
    if kind in (10, 12, 14):
        bl, fails = lean_conditions(P, kind, black)
        item_fails = {k: np.bincount(item_of, v, nitems) > 0 for k, v in fails.items()}
        lean = ~(item_fails["fail_bits"] | item_fails["fail_ref"] | item_fails["fail_top"] | item_fails["fail_wrap"])
        for k, v in item_fails.items():
            c[k] = int(v.sum())
        if variant == "nolean":
            lean[:] = False
        c["lean"], c["notlean"] = int(lean.sum()), int((~lean).sum())
        ref_used = np.where(lean[item_of], P.refs - bl, P.refs)  # (a lean item's references go into the LDS without their black levels)
    c["wrap_lanes"] = int(((P.res + ref_used[:, None]) > 65535).reshape(P.nblk, 8, 8).any(axis=2).sum())
    # ---- stores: every tile is 4 rows of 8 pieces of 8 samples
    fast = variant != "slowstore" and off % fast_align(kind, planes) == 0 and w % 8 == 0
    tilesY = ntiles // P.tilesX
    merged = np.zeros((tilesY, P.tilesX), bool)
    if kind == 14 and variant != "nomerge":
        ty, tx = np.divmod(np.arange(ntiles), P.tilesX)
        tin = fast & (4 * ty + 4 <= rows) & (64 * tx + 64 <= w)
        for m in range(0, ntiles, 4):  # a round of a wave: four tiles in a row of the stream's order
            if m + 4 > ntiles:
                c["decl_partial"] += 1
            elif not tin[m:m + 4].all():
                c["decl_notin"] += 1
            else:
                merged[ty[m:m + 4], tx[m:m + 4]] = True
                back = 4 * sum(1 for j in range(4) if j == 3 or tx[m + j] + 1 == P.tilesX)  # lane k = 7 of both row pairs, two rows each
                c["st_merged_back"] += back
                c["st_merged_fwd"] += 128 - back
    Y = np.arange(4 * tilesY)[:, None]
    X = 8 * np.arange(8 * P.tilesX)[None, :]
    plain = ~np.repeat(np.repeat(merged, 4, axis=0), 8, axis=1)
    inside = plain & (Y < rows) & (X < w)
    c["drop_y"] = int((plain & (Y >= rows)).sum())
    c["drop_x"] = int((plain & (Y < rows) & (X >= w)).sum())
    whole = inside & (X + 8 <= w)
    c["st_aligned"] = int(whole.sum()) if fast else 0
    c["st_unaligned"] = 0 if fast else int(whole.sum())
    c["st_cropped"] = int((inside & ~whole).sum())
    return c


def census(batches, setting, variant="census"):
    """The census of one context that decodes `batches` (lists of frames) under `setting`, in the build `variant`."""
    kind, black, planes = stage_of(setting)
    S = SETTINGS[setting]
    xcd = S.get("xcd", 128)
    tot = dict.fromkeys(PATHS, 0)
    for frames in batches:
        for members, groups in size_classes([ngroups_planned(f["w"], f["h"]) for f in frames]):
            total = groups * 2 * len(members)
            tot["waves"] += total
            tot["wg_chunked" if xcd else "wg_remap"] += (total + 3) // 4
            for i in members:
                nitems = (parse(frames[i]["buf"]).nblk + ITEM_BLOCKS - 1) // ITEM_BLOCKS
                assert nitems <= 2 * groups
                tot["invalid"] += 2 * groups - nitems
        for f in frames:
            for k, v in frame_census(f, kind, black, planes, S.get("off", 0), variant).items():
                tot[k] += v
    return tot


# ---------------------------------------------------------------- the corpus

def _full_width_blocks(rng, widths, ref=5):
    """[n, 64] samples: block i has residuals of exactly widths[i] bits (0 and 2^b - 1 both occur) above `ref` (0 for 16 bits)."""
    out = np.zeros((len(widths), 64), np.int64)
    for i, b in enumerate(widths):
        if b:
            out[i] = rng.integers(0, 1 << b, 64)
            a, z = rng.choice(64, 2, replace=False)
            out[i, a], out[i, z] = 0, (1 << b) - 1
        out[i] += 0 if b == 16 else ref
    return out.astype(np.uint16)


@functools.lru_cache(maxsize=1)
def corpus():
    """-> list of dicts: name, w, h (what the caller asks for), buf, tags"""
    out = []

    def add(name, img, buf=None, h=None, **tags):
        out.append(dict(name=name, w=img.shape[1], h=h or img.shape[0], buf=np.ascontiguousarray(L.encode7(img) if buf is None else buf),
                        img=img, tags=tags))

    rng = np.random.default_rng(7701)
    # ---- every pair of bit widths in both sibling pairs of a tile
    pairs = [(a, b) for a in range(17) for b in range(17)] + [(16, 0)]  # (290 tiles: 10 x 29)
    widths = [v for a, b in pairs for v in (a, b, a, b)]
    img = block_image(_full_width_blocks(rng, widths), 10)
    add("pairs", img, pairs=1)
    assert list(parse(out[-1]["buf"]).bits) == widths
    # ---- geometry
    for w, h in ((64, 4), (128, 6), (200, 10), (576, 37), (1000, 37), (77, 10), (1001, 6), (66, 6), (66, 10),
                 (192, 4), (320, 8), (384, 10), (448, 6), (512, 8)):
        add("geo %dx%d" % (w, h), L.natural_image_np(w, h, 12, 12.0, 100 + w + h), geo=1)
    img = L.natural_image_np(256, 8, 12, 12.0, 77)
    add("coded shorter than asked", img, h=12, geo=1, short=1)
    # ---- lean, one reason each
    add("lean raw", rng.integers(0, 1 << 16, (16, 256)).astype(np.uint16), lean=1)
    add("lean dark", rng.integers(0, 60, (16, 256)).astype(np.uint16), lean=1)
    ramp = (9000 + 2 * np.arange(256)[None, :] + 100 * np.arange(16)[:, None] + rng.integers(0, 64, (16, 256))).astype(np.uint16)
    add("lean top12", ramp, lean=1)
    add("lean top10", ramp + 16, lean=1)
    add("lean high", rng.integers(65400, 65528, (16, 256)).astype(np.uint16), lean=1)
    add("lean natural", L.natural_image_np(256, 16, 10, 6.0, 78) >> 1, lean=1)
    cfa = (np.arange(16)[:, None] & 1) * 2 + (np.arange(256)[None, :] & 1)
    add("lean natural above black", (np.asarray(BLACK)[cfa] + (L.natural_image_np(256, 16, 10, 6.0, 76) >> 1)).astype(np.uint16), lean=1)
    # ---- the reference add wraps: references of every third block re-laid just below 65536
    img = L.natural_image_np(256, 16, 10, 12.0, 79)
    base = np.ascontiguousarray(L.encode7(img))
    count, vals, nibs, _ = K.parse_stream(base, 1)
    vals = vals.copy()
    vals[0:K.geometry(base)[0]:3] = 65535 - np.arange(len(vals[0:K.geometry(base)[0]:3])) % 7
    buf = K.assemble(base, [K.stream_bytes(base, 0), K.emit_stream(vals, [15] * len(nibs), count)])
    add("wrap", img, buf=buf, wrap=1)
    # ---- spans
    add("span empty", np.full((16, 256), 777, np.uint16), span=1)
    widths = [1] + [16] * 63
    add("span full", block_image(_full_width_blocks(rng, widths), 4), span=1)
    add("span short", L.natural_image_np(192, 4, 12, 12.0, 80), span=1)
    # ---- one size class of 5 groups for frames of 5 and of 4
    for i, w in enumerate((256, 320, 256)):
        add("mixed %d" % i, L.natural_image_np(w, 64, 12, 12.0, 81 + i), mixed=1)
    return out


def batches(setting):
    """The batches of frames (indices into corpus()) that the child decodes under `setting`: every frame alone, the mixed
    frames as one batch.  The planes layout takes frames of even width and height, coded no shorter than asked."""
    S, C = SETTINGS[setting], corpus()
    ok = [i for i, f in enumerate(C) if (not S.get("only") or S["only"] in f["tags"])
          and (not S.get("even") or (f["w"] % 2 == 0 and f["h"] % 2 == 0 and "short" not in f["tags"]))]
    out = [[i] for i in ok if "mixed" not in C[i]["tags"]]
    mixed = [i for i in ok if "mixed" in C[i]["tags"]]
    return out + ([mixed] if mixed else [])


@functools.lru_cache(maxsize=1)
def expectations():
    """The oracle's word on every frame: [(ret, rows)], rows = the first ret // w rows of its output."""
    out = []
    for f in corpus():
        ret, px = L.oracle_decode7(f["buf"], f["w"], f["h"])
        assert ret > 0 and ret % f["w"] == 0
        out.append((ret, px[:ret // f["w"]].copy()))
    return out


def expected_bytes(setting, i):
    """What frame i's output must hold under `setting` (uint8), and the bytes its buffer gets for the height asked."""
    f = corpus()[i]
    rows = expectations()[i][1]
    st = SETTINGS[setting].get("stage")
    if st is None:
        return rows.view(np.uint8).ravel(), 2 * f["w"] * f["h"]
    if st[0] == "post":
        kw = st[1]
        return L.oracle_post(rows, black=kw.get("black"), bits=kw.get("bits")).ravel(), L.post_row_bytes(f["w"], bits=kw.get("bits")) * f["h"]
    kw = st[1]
    es = 4 if kw["dtype"] == "f32" else 2
    return FR.ref_bytes(rows, kw["dtype"], kw["white"], kw.get("layout", "planes"), kw.get("black", (0, 0, 0, 0)), kw.get("clip", False),
                        kw.get("plane")), es * f["w"] * f["h"]


def model(setting, variant="census"):
    C = corpus()
    return census([[C[i] for i in b] for b in batches(setting)], setting, variant)


def alone_report():
    """For every frame of LEAN_ALONE: its four fail counters in its setting -> {frame: {counter: items}}."""
    C = {f["name"]: f for f in corpus()}
    out = {}
    for name, (setting, _) in LEAN_ALONE.items():
        kind, black, planes = stage_of(setting)
        c = frame_census(C[name], kind, black, planes, 0, "census")
        out[name] = {k: c[k] for k in FAILS + ("lean", "notlean")}
    return out
