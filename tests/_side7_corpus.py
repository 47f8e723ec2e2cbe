"""Type-7 side streams for the tests: a tool that codes a side stream again with chosen record sizes, a plain model of what a
stream's content decides in k7_side, and a compact corpus made with both.

A side stream is a 4-byte entry count and a chain of records {nibble << 4 | ref >> 8, ref & 255, LEN[nibble] payload bytes}; a
record holds 64 entries (the bit widths, or the references, of 64 blocks = 4096 pixels).  k7_side (csrc/mcraw_type7.hip) takes a
stream through LDS in pieces of 32 KiB that start at A0 = (offset + 4) & ~15, looks at every second byte as a candidate record
start, follows the chain by runs of equally long records or by segment walkers, in units of at most SIDE_LCAP records, and may
cut a stream into parts by a guess of where it ends.  All of that is decided by record sizes and positions, so the corpus is
mostly images that are FLAT within a record's 4096 pixels (another value per record): no payload at all, and side streams whose records can be given any of the ten sizes (2 .. 130 bytes) by a
wider header nibble than their values need (recode_side).  It holds (corpus(), built on the CPU, deterministic)
  * one record size per stream for every header nibble 0 .. 15 (all ten storage classes), each stream at another offset mod 16
    (every first candidate 0 .. 7, even and odd addresses); sizes that alternate every record (66/82, 2/130); runs of exactly 63,
    64, 65 and 128 equal records; runs that end where a list of 128 / 512 (and 64 / 256) records is full and one record to
    either side;
  * streams of exactly 1, 2, 3, 4, 5, 8 and 9 pieces; a record that ends exactly at a piece's end, one of 130 bytes on the piece's
    last candidate (straddling by 128 bytes), records that straddle by 2 and by 64 bytes -- at the 32 KiB and at the 8 KiB grid;
  * a last record that ends exactly at `len` and one byte past it, a stream cut in its first piece, after one of its three
    pieces and in its last piece (the partition into parts follows `len`, so a cut always falls to the last part), an entry count
    one short, a bits entry of 17 in the first and in the last record, unused entries of the last record above 16;
  * an end guess far too long (refs in front of bits, trailing bytes), one too short (the refs stream is the tail of the bits
    stream, which has extra records: the other stream's offset, the guess, lies inside it), streams shorter than a piece;
  * a refs stream whose payload bytes read as headers of the records' own size (chains off the true one never join it);
  * two natural 12-bit frames, 14-bit noise, a banded frame, and single-byte mutants of two frames' side streams.
64 frames, 86 MP (a product-size piece of the largest records is a megapixel: the frames of 4, 5, 8 and 9 pieces are 25 of them), 15 MB
of streams and payload.  What a frame must decode to is the oracle's business (expectations())."""
import ctypes as C
import functools

import numpy as np

import _libs as L
from _legacy_corpus import banded_image, mutants

PIECE = 32768       # stream bytes per piece of k7_side (16 * SIDE_T * SIDE_LPT)
LCAP = 512          # records per unit (SIDE_LCAP); the first unit of a decode takes a quarter
LEN7 = (0, 8, 16, 24, 32, 40, 48, 64, 64, 80, 80, 128, 128, 128, 128, 128)  # payload bytes of a record by header nibble
SIZE = tuple(2 + n for n in LEN7)
WIDTH = (0, 1, 2, 3, 4, 5, 6, 8, 8, 10, 10, 16, 16, 16, 16, 16)            # bits stored per entry


# ---------------------------------------------------------------- records

def _pack(nib, res):
    out = np.zeros(128, np.uint8)
    n = L.synth().mcraw_synth_pack_block7(out.ctypes.data_as(C.c_void_p), int(nib), np.ascontiguousarray(res, np.uint16).ctypes.data_as(C.c_void_p))
    assert n == LEN7[nib]
    return out[:n]


@functools.lru_cache(maxsize=None)
def _bitmap(nib):
    """[64, WIDTH] payload bit that holds bit b of entry i (found by packing one bit at a time)."""
    m = np.zeros((64, WIDTH[nib]), np.int64)
    for i in range(64):
        for b in range(WIDTH[nib]):
            v = np.zeros(64, np.uint16)
            v[i] = 1 << b
            bits = np.flatnonzero(np.unpackbits(_pack(nib, v), bitorder="little"))
            assert bits.size == 1
            m[i, b] = bits[0]
    return m


def _unpack(nib, payload):
    if WIDTH[nib] == 0:
        return np.zeros(64, np.uint16)
    bits = np.unpackbits(np.frombuffer(payload, np.uint8), bitorder="little").astype(np.uint32)
    return (bits[_bitmap(nib)] << np.arange(WIDTH[nib], dtype=np.uint32)).sum(axis=1).astype(np.uint16)


def emit_stream(values, nibbles, count):
    """count, then one record per 64 entries of `values` with the header nibble given for it."""
    values = np.asarray(values, np.uint16).reshape(-1, 64)
    assert len(values) == len(nibbles)
    out = [np.frombuffer(np.uint32(count).tobytes(), np.uint8)]
    for v, nib in zip(values, nibbles):
        ref = min(int(v.min()), 4095)
        res = (v.astype(np.int64) - ref).astype(np.uint16)
        assert nib >= 11 or int(res.max()) < (1 << WIDTH[nib]), "nibble %d cannot hold %d" % (nib, int(res.max()))
        out += [np.array([(nib << 4) | (ref >> 8), ref & 255], np.uint8), _pack(nib, res)]
    return np.concatenate(out)


def header(buf):
    """-> encW, encH, bitsOff, refsOff"""
    return tuple(int(v) for v in np.frombuffer(buf[:16].tobytes(), np.uint32))


def geometry(buf):
    """-> nblk, R (records of a side stream the frame uses)"""
    encW, encH = header(buf)[:2]
    nblk = encW * encH // 64
    return nblk, (nblk + 63) // 64


def parse_stream(buf, which):
    """The stream as its writer meant it: -> (count, values [nrec * 64], nibbles [nrec], bytes it takes), nrec = ceil(count / 64)."""
    b = buf.tobytes()
    so = header(buf)[2 + which]
    count = int.from_bytes(b[so:so + 4], "little")
    p, vals, nibs = so + 4, [], []
    for _ in range((count + 63) // 64):
        nib, ref = b[p] >> 4, ((b[p] & 15) << 8) | b[p + 1]
        assert p + SIZE[nib] <= len(b)
        vals.append((_unpack(nib, b[p + 2:p + SIZE[nib]]).astype(np.uint32) + ref).astype(np.uint16))
        nibs.append(nib)
        p += SIZE[nib]
    return count, np.concatenate(vals), np.array(nibs), p - so


def assemble(buf, streams, order=(0, 1), so_mod16=(None, None), tail=0, fill=0xEE):
    """The frame `buf` with its side streams replaced by the bytes streams[0] (bits), streams[1] (refs), laid out in `order` behind
    the payload; so_mod16[which]: bytes are put in front of that stream until its offset is that modulo 16; `tail` unused bytes
    behind the last stream.  bitsOff / refsOff are patched."""
    front = min(header(buf)[2:])
    out = [buf[:front]]
    n = front
    offs = [0, 0]
    for which in order:
        pad = 0 if so_mod16[which] is None else (so_mod16[which] - n) % 16
        out.append(np.full(pad, fill, np.uint8))
        offs[which] = n + pad
        out.append(streams[which])
        n += pad + streams[which].size
    out.append(np.full(tail, fill, np.uint8))
    res = np.concatenate(out)
    res[8:16] = np.frombuffer(np.array(offs, np.uint32).tobytes(), np.uint8)
    return res


def stream_bytes(buf, which):
    so = header(buf)[2 + which]
    return buf[so:so + parse_stream(buf, which)[3]]


def recode_side(buf, which, nibbles, extra=0, **layout):
    """`buf` with side stream `which` (0 bits, 1 refs) coded again: record i gets the header nibble nibbles[i] (one number: every
    record) -- at least what its entries need --, `extra` more records than the stream had (entries 0 .. 7, counted in the entry
    count; nibbles covers them).  The other stream is kept byte for byte; layout: see assemble()."""
    count, vals, old, _ = parse_stream(buf, which)
    if extra:
        vals = np.concatenate([vals, np.tile(np.arange(64, dtype=np.uint16) & 7, extra)])
        count = (count + 63) // 64 * 64 + 64 * extra
    nrec = vals.size // 64
    nibbles = [int(nibbles)] * nrec if np.isscalar(nibbles) else [int(v) for v in nibbles]
    assert len(nibbles) == nrec, (len(nibbles), nrec)
    streams = [None, None]
    streams[which] = emit_stream(vals, nibbles, count)
    streams[1 - which] = stream_bytes(buf, 1 - which)
    return assemble(buf, streams, **layout)


# ---------------------------------------------------------------- what the content decides (a model of k7_side)

OUT, DEAD = "out", "dead"


class Stream:
    """Side stream `which` of the frame `buf` as k7_side sees it, for pieces of `piece` bytes."""

    def __init__(self, buf, which, piece=PIECE):
        self.b = buf.tobytes()
        self.len = len(self.b)
        self.which, self.piece = which, piece
        encW, encH, bo, ro = header(buf)
        self.so, self.other = (ro, bo) if which else (bo, ro)
        self.nblk, self.R = geometry(buf)
        self.A0 = (self.so + 4) & ~15
        self.odd = (self.so + 4) & 1                      # candidates are the byte pairs at A0 + 2 u + odd
        self.first_cand = ((self.so + 4) & 15) >> 1
        count = int.from_bytes(self.b[self.so:self.so + 4], "little") if self.so + 4 <= self.len else 0
        self.accepted = self.so + 4 <= self.len and count >= self.nblk   # (the header checks that the corpus can fail)

    def stride(self, p):
        """Bytes of the record that a header at byte p announces; DEAD: it would cross `len`."""
        size = SIZE[(self.b[p] if p < self.len else 0) >> 4]
        return DEAD if p + size > self.len else size

    def piece_of(self, p):
        return (p - self.A0) // self.piece

    def piece_end(self, pc):
        return self.A0 + (pc + 1) * self.piece

    def chain(self, start=None, limit=None, until=None):
        """Record starts from `start` (default: the stream's first record) on: at most `limit` of them, none at or behind `until`.
        -> (starts, what stands behind them: the next start, or DEAD)"""
        p = self.so + 4 if start is None else start
        out = []
        while (limit is None or len(out) < limit) and (until is None or p < until):
            s = self.stride(p)
            if s is DEAD:
                return out, DEAD
            out.append(p)
            p += s
        return out, p

    @functools.cached_property
    def records(self):
        """Starts of the records the frame uses (R, fewer when the chain is dead)."""
        return self.chain(limit=self.R)[0]

    @property
    def dead(self):
        return self.accepted and len(self.records) < self.R

    @property
    def pieces(self):
        """Pieces in which records of the stream start."""
        return self.piece_of(self.records[-1]) + 1 if self.records else 0

    def crossings(self):
        """For every piece boundary the chain crosses: bytes by which the straddling record reaches over it (0: it ends there)."""
        out = []
        for p in self.records:
            e = self.piece_end(self.piece_of(p))
            if p + self.stride(p) >= e:
                out.append(p + self.stride(p) - e)
        return out

    # ---- parts
    def parts(self, nsp):
        """[(m_lo, m_hi)] per part: the pieces it owns by the guess of where the stream ends (the other stream's offset when that
        lies behind this one's, else `len`); the last part's range is open."""
        end_guess = self.other if self.other > self.so else self.len
        npieces = (end_guess - self.A0 + self.piece - 1) // self.piece
        return [(q * npieces // nsp, (q + 1) * npieces // nsp if q + 1 < nsp else None) for q in range(nsp)]

    def asking_parts(self, nsp):
        """Parts that ask the part in front (all but part 0 and the part that owns piece 0) -> dict: `asking` -- how many --,
        `asking_work` -- those of them that own pieces --, `part1`, `part1_work` -- the same for part 1 alone: the part it
        asks is part 0, so in a build whose part 0 never tells it gives up whatever the timing."""
        out = dict(asking=0, asking_work=0, part1=0, part1_work=0)
        for q, (lo, hi) in enumerate(self.parts(nsp)):
            work = hi is None or hi > lo
            if q == 0 or (work and lo == 0):
                continue
            for k in ("asking",) + (("part1",) if q == 1 else ()):
                out[k] += 1
                out[k + "_work"] += work
        return out

    def spec_entry(self, part, nsp, warm):
        """Where the chain that starts `warm` candidates in front of the part's first piece enters that piece, and where the true
        chain does (None: it does not reach it)."""
        lo = self.parts(nsp)[part][0]
        edge = self.A0 + lo * self.piece
        got = self.chain(start=edge - 2 * warm + self.odd, until=edge)[1]
        true = self.chain(until=edge)[1]
        return got, (None if true is DEAD else true)

    def handoff(self, nsp, warm, lastc=True):
        """Which of its outcomes the hand-off of each part takes when every part in front speaks in time: the part that owns
        piece 0 has nobody to ask (its count stands; the last part has none to stand); for the others, the stream is over in
        front of their pieces (R records, or a dead chain), or they own nothing and pass on what they hear, or their speculative
        count entered their first piece where the true chain does, or elsewhere.  -> {outcome: parts}"""
        out = dict(ho_over=0, ho_pass=0, ho_last=0, ho_hit=0, ho_miss=0, lastc_replayed=0)
        for q, (lo, hi) in enumerate(self.parts(nsp)):
            empty, lastp = hi is not None and hi <= lo, q == nsp - 1
            if not empty and lo == 0:
                out["ho_last" if lastp else "ho_hit"] += 1
                continue
            edge = self.A0 + lo * self.piece
            starts, true = self.chain(limit=self.R, until=edge)
            if len(starts) >= self.R or true is DEAD:
                out["ho_over"] += 1
            elif empty:
                out["ho_pass"] += 1
            else:
                hit = self.chain(start=edge - 2 * warm + self.odd, until=edge)[1] == true
                if lastp:
                    out["ho_last"] += 1
                    out["lastc_replayed"] += lastc and hit
                else:
                    out["ho_hit" if hit else "ho_miss"] += 1
        return out

    # ---- one workgroup per stream: the walk
    def walk(self, lcap=LCAP, ratio=3, force_segw=False):
        """Units and passes of the walk of one workgroup over the whole stream.  (Unlike the chain, the pieces, the parts and the
        hand-off above, which follow from the format, passes and units are no property of the stream: they are what the kernel's
        run rule makes of it, and this is that rule in Python, step for step.  Counts compared with it show that the kernel
        still takes the ways it took, not that the rule is right; that is the pixels' business, against the oracle.)  The run rule: a pass looks at the 64 candidates
        p, p + S, p + 2S ... for the stride S of the record at p (a first pass of a unit that does not know S finds it and lists
        nothing) and lists those up to the first that announces another stride, lies behind the piece or would cross `len`; a
        unit ends when its list is full or the stream complete (why 1), behind the piece (2) or where the chain is dead (3).  From
        its 8th pass on a unit that has listed fewer than `ratio` records per pass hands the rest of the stream to the segment
        walkers, which list a piece from where the chain stands to its end and hand it out unit by unit."""
        c = dict(records=0, units=0, units_full=0, piece_steps=0, units_dead=0, run_passes=0, run_passes64=0, segw_switch=0,
                 segw_pieces=0, segw_resumed=0, dead=0, max_passes=0, early=0)
        if not self.accepted:
            return c
        R, p, S, n = self.R, self.so + 4, 0, 0
        pc = self.piece_of(p)
        segw, seg, fresh = force_segw, None, True  # seg: [records of the piece not handed out yet, what stands behind them]
        room = min(R, lcap // 4)
        while True:
            cnt, why, end = 0, 2, self.piece_end(pc)
            if not segw and p < end:
                passes = 0
                while True:
                    codes = [OUT if p + j * S >= end else self.stride(p + j * S) for j in range(64 if S else 1)]
                    nb = next((j for j, v in enumerate(codes) if v != S), 64) if S else 0
                    take = min(nb, room - cnt)
                    nxt = codes[nb & 63] if S else codes[0]
                    cnt, p = cnt + take, p + take * S
                    go = take == nb and cnt < room and (nb == 64 or nxt not in (OUT, DEAD))
                    if go and nb != 64:
                        S = nxt
                    passes += 1
                    c["run_passes"] += 1
                    c["run_passes64"] += nb == 64
                    c["early"] |= go and passes >= 8
                    segw = go and passes >= 8 and passes * ratio > cnt
                    if not go or segw:
                        break
                c["max_passes"] = max(c["max_passes"], passes)
                if segw:
                    c["segw_switch"] += 1
                    seg = None
                elif take < nb:
                    why = 1
                elif cnt >= room:
                    why, S = 1, (nxt if nb != 64 and nxt not in (OUT, DEAD) else 0)
                else:
                    why, S = (2 if nxt is OUT else 3), 0
            elif not segw:
                S = 0
            if segw and p < end:
                if fresh or seg is None:
                    seg = list(self.chain(start=p, until=end))
                    c["segw_pieces"] += 1
                else:
                    c["segw_resumed"] += 1
                take = min(room - cnt, len(seg[0]))
                seg[0] = seg[0][take:]
                cnt, S = cnt + take, 0
                if not seg[0]:
                    why, p, seg = (3 if seg[1] is DEAD else 2), seg[1], None
                else:
                    why, p = 1, seg[0][0]
            c["units"] += 1
            c["units_full"] += why == 1
            c["piece_steps"] += why == 2
            c["units_dead"] += why == 3
            n += cnt
            if n >= R or why == 3:
                c["dead"] = int(why == 3 and n < R)
                break
            fresh = why == 2
            pc += fresh
            room = min(R - n, lcap)
        c["records"] = n
        assert n == len(self.records)
        return c


def model(buf, which, piece=PIECE):
    return Stream(buf, which, piece)


# ---------------------------------------------------------------- the corpus

def flat_frame(R, w=1024):
    """An image of R records per side stream (4096 pixels each) that is flat within each record's 16 tiles and differs from
    record to record: no payload, bits entries 0, and the 64 refs entries of record r are all 1000 + 37 r mod 2000 -- any header
    nibble holds them, and a record listed twice or left out changes the pixels."""
    assert (4 * R * 1024) % w == 0 and w % 64 == 0
    h = 4 * R * 1024 // w
    tile = np.arange(h // 4)[:, None] * (w // 64) + np.arange(w // 64)[None, :]   # tiles in the order of the streams' entries
    vals = (1000 + (tile // 16) * 37 % 2000).astype(np.uint16)
    img = np.repeat(np.repeat(vals, 4, axis=0), 64, axis=1)
    return img, L.encode7(img)


def sizes_to(total):
    """Header nibbles of the fewest records whose sizes add up to `total` bytes (even)."""
    assert total >= 0 and total % 2 == 0
    big = max(0, (total - 400) // 130)
    rest = total - 130 * big
    best = {0: []}
    for t in range(2, rest + 1, 2):
        cands = [(best[t - SIZE[nib]] + [nib]) for nib in (0, 1, 2, 3, 4, 5, 6, 8, 10, 15) if t - SIZE[nib] in best]
        best[t] = min(cands, key=len)
    return [15] * big + best[rest]


def _land(buf, which, R, offset, then, piece=PIECE, so_mod16=6):
    """Stream `which` coded so that a record starts exactly `offset` bytes from the end of piece 0 (a negative offset: in front
    of it) with the header nibble `then`; records of 130 bytes behind it."""
    layout = dict(so_mod16=(None, so_mod16) if which else (so_mod16, None))
    so = header(recode_side(buf, which, 0, **layout))[2 + which]
    A0 = (so + 4) & ~15
    pre = sizes_to(A0 + piece + offset - (so + 4))
    return recode_side(buf, which, (pre + [then] + [15] * R)[:R], **layout)


def _side_mutants(buf, seed, n):
    """`n` single-byte mutants of the frame's side streams (the fuzz suite's mutator; header and payload stay)."""
    s0 = min(header(buf)[2:])
    return [np.concatenate([buf[:s0], m]) for m in mutants(buf[s0:].copy(), np.random.default_rng(seed), n, flips=1)]


def _overlapped(R, E, seed):
    """A frame whose refs stream is the tail of its bits stream: every block has 2-bit residuals above the reference 2, so bits
    entries and refs entries are all 2 and a record of the one is a record of the other.  The bits stream has E more records
    than the frame uses, of 130 bytes, but for records E - 2 and E - 1: two headers of 2-byte records, {0x00, 0x02} twice, which
    read as an entry count of 0x02000200.  refsOff points at them.  The guess of where the bits stream ends -- the other
    stream's offset -- then falls E - 2 records into it."""
    rng = np.random.default_rng(seed)
    img = (2 + rng.integers(0, 4, size=(4 * R, 1024))).astype(np.uint16)
    col = np.arange(1024) % 64  # (every block's minimum is 2 and its maximum 5: a block is the samples of one column parity in rows y, y + 2 of a tile)
    img[:, col < 4] = 2
    img[:, (col >= 4) & (col < 8)] = 5
    buf = L.encode7(img)
    assert set(parse_stream(buf, 0)[1]) == {2} and set(parse_stream(buf, 1)[1]) == {2}
    nib = [15] * (R + E)
    nib[E - 2] = nib[E - 1] = 0
    s0 = emit_stream(np.full(64 * (R + E), 2, np.uint16), nib, (R + E) * 64)
    buf = assemble(buf, [s0, np.zeros(0, np.uint8)], so_mod16=(3, None))
    bo = header(buf)[2]
    ro = bo + 4 + sum(SIZE[v] for v in nib[:E - 2])
    buf[12:16] = np.frombuffer(np.uint32(ro).tobytes(), np.uint8)
    return img, buf


@functools.lru_cache(maxsize=1)
def corpus():
    """-> list of dicts: name, w, h, buf, img (None for a stream that is not an image's), whole (must decode to img, status 0),
    tags (what the frame was made for: test_side7_corpus.py checks each with the model)."""
    out = []

    def add(name, img, buf, whole=True, **tags):
        h, w = img.shape
        out.append(dict(name=name, w=w, h=h, buf=np.ascontiguousarray(buf), img=img if whole else None, whole=whole, tags=tags))

    # ---- record sizes: one size per stream, every nibble, every offset mod 16
    img, base = flat_frame(40)
    for nib in range(16):
        buf = recode_side(recode_side(base, 0, 15 - nib, so_mod16=((5 * nib + 3) % 16, None)), 1, nib, so_mod16=(None, nib))
        add("records of nibble %d" % nib, img, buf, nibble=nib)
    img, base = flat_frame(600)
    add("66/82 alternating", img, recode_side(base, 1, [7, 9] * 300), alternating=(66, 82))
    add("2/130 alternating", img, recode_side(base, 0, [0, 15] * 300), alternating=(2, 130))
    img, base = flat_frame(264)
    for run in (63, 64, 65, 128):
        add("runs of %d" % run, img, recode_side(base, 1, (([4] * run + [6] * run) * 5)[:264]), run=run)
    img, base = flat_frame(700)
    for d in (-1, 0, 1):  # sizes change where the lists of 128 and 512 records (64 and 256: the short-unit build) are full, and next to it
        at = (64 + d, 128 - d, 320 + d, 640 - d)
        nib = [3 + 2 * sum(i >= a for a in at) for i in range(700)]
        add("runs end at lists %+d" % d, img, recode_side(base, 1, nib), list_ends=at)
    # ---- boundaries
    for k, R in ((1, 240), (2, 490), (3, 740), (4, 1000), (5, 1250), (8, 2000), (9, 2250)):
        img, base = flat_frame(R, w=2048 if R % 2 == 0 else 1024)
        add("%d pieces" % k, img, recode_side(base, 1, 15), pieces=k)
    for piece, R, grid in ((PIECE, 520, "32 KiB"), (8192, 200, "8 KiB")):
        img, base = flat_frame(R)
        for off, then, reach in ((-66, 8, 0), (-2, 15, 128), (-128, 15, 2), (-66, 15, 64)):
            add("straddles by %d at %s" % (reach, grid), img, _land(base, 1, R, off, then, piece), straddle=(piece, reach))
    # ---- ends
    img, base = flat_frame(40)
    full = recode_side(base, 1, 10)
    add("ends one byte past len", img, full[:-1], whole=False, dead=1)
    add("count one short", img, np.concatenate([full[:header(full)[3]], np.frombuffer(np.uint32(geometry(full)[0] - 1).tobytes(), np.uint8), full[header(full)[3] + 4:]]),
        whole=False, rejected=1)
    img, base = flat_frame(740)
    full = recode_side(base, 1, 15)
    ro = header(full)[3]
    add("cut in its first piece", img, full[:ro + 4 + 130 * 100 + 7], whole=False, dead=1, cut_piece=0)
    add("cut after one of three pieces", img, full[:ro + 4 + 130 * 400 + 64], whole=False, dead=1, cut_piece=1)
    add("cut in its last piece", img, full[:ro + 4 + 130 * 730 + 1], whole=False, dead=1, cut_piece=2)
    for name, w, h, at, val, whole in (("bits entry 17 in the first record", 256, 64, 0, 17, False),
                                       ("bits entry 17 in the last record", 256, 64, 255, 17, False),
                                       ("unused bits entries above 16", 192, 20, 61, 200, True)):  # (60 blocks: the record has four entries the frame does not use)
        img = L.natural_image_np(w, h, 12, 12.0, 41)
        base = L.encode7(img)
        count, vals, nibs, _ = parse_stream(base, 0)
        vals[at:at + (3 if whole else 1)] = val
        add(name, img, assemble(base, [emit_stream(vals, [15] * len(nibs), count), stream_bytes(base, 1)]), whole=whole, entry=at)
    # ---- parts
    img, base = flat_frame(300)
    add("end guess far too long", img, recode_side(recode_side(base, 1, 15, order=(1, 0)), 0, 1, order=(1, 0), tail=5 * PIECE + 77), guess="long")
    img, buf = _overlapped(600, 300, 43)
    add("end guess too short", img, buf, guess="short")
    # ---- adversarial: payload bytes that read as headers of the records' own size (0xC0AF = reference 0xFFF + raw residual 0xB0B0)
    img = np.full((1024, 2048), 0xC0AF, np.uint16)
    add("chains never join", img, L.encode7(img), never_join=1)
    # ---- natural content
    for seed in (51, 52):
        img = L.natural_image_np(2048, 1536, 12, 12.0 * (seed - 50), seed)
        add("nat12 %d" % seed, img, L.encode7(img), natural=1)
    img = np.random.default_rng(53).integers(0, 1 << 14, size=(1024, 1024), dtype=np.uint16)
    add("noise14", img, L.encode7(img), noise=1)
    img = banded_image(np.random.default_rng(54), 1024, 1024, 10)
    add("bands", img, L.encode7(img))
    img = banded_image(np.random.default_rng(56), 512, 256, 6)
    add("bands small", img, L.encode7(img))
    img = L.natural_image_np(512, 256, 12, 12.0, 55)
    add("nat12 small", img, L.encode7(img, flags=4))
    for k, seed in ((len(out) - 1, 7701), (len(out) - 2, 7702)):
        f = out[k]
        for j, b in enumerate(_side_mutants(f["buf"], seed, 3)):
            out.append(dict(name="%s, mutant %d" % (f["name"], j), w=f["w"], h=f["h"], buf=b, img=None, whole=False, tags=dict(mutant=1)))
    f = out[3]  # (more rows asked for than the frame codes: the rows below stay untouched)
    out.append(dict(name="coded shorter than asked", w=f["w"], h=f["h"] + 8, buf=f["buf"], img=None, whole=False, tags=dict(short=1)))
    return out


def expectations():
    """The oracle's word on every frame of the corpus: [(ret, pixels)].  HIP must agree by the fuzz suite's rule: ret == 0 -- a
    nonzero status and nothing written --, else status 0, `ret` written and the first ret // w rows equal."""
    return [L.oracle_decode7(f["buf"], f["w"], f["h"]) for f in corpus()]


def census_model(frames, piece=PIECE, **walk):
    """What one decode of `frames`, one workgroup per stream, adds to the census: the sum of Stream.walk() over their streams,
    and the workgroups accepted and rejected."""
    tot = {}
    for f in frames:
        for which in (0, 1):
            s = Stream(f["buf"], which, piece)
            c = s.walk(**walk)
            c["streams"], c["rejected"] = int(s.accepted), int(not s.accepted)
            c["early_streams"] = int(c.pop("early"))
            c.pop("max_passes")
            for k, v in c.items():
                tot[k] = tot.get(k, 0) + int(v)
    return tot
