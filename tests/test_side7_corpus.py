"""The type-7 side-stream corpus of tests/_side7_corpus.py is what it says it is (CPU): every whole frame decodes to its image
through the oracle, the oracle accepts or rejects the others as listed, and every frame made for a way of k7_side's chain walk
has the property it is named for, by the plain model of tests/_side7_corpus.py."""
import numpy as np

import _side7_corpus as K
from motioncam_decoder_amd import build as B


def _by_name():
    return {f["name"]: f for f in K.corpus()}


def _tagged(tag):
    return [f for f in K.corpus() if tag in f["tags"]]


def _flag(variant, name):
    return next(int(v.split("=")[1].rstrip("u")) for v in B.K7_PATH_VARIANTS[variant] if v.startswith("-D" + name + "="))


def test_the_oracle_accepts_or_rejects_every_frame_as_listed():
    frames, expect = K.corpus(), K.expectations()
    rets = {}
    for f, (ret, out) in zip(frames, expect):
        rets[f["name"]] = ret
        if f["whole"]:
            assert ret == f["w"] * f["h"] and np.array_equal(out, f["img"]), f["name"]
    for name in ("ends one byte past len", "count one short", "cut in its first piece", "cut after one of three pieces",
                 "cut in its last piece", "bits entry 17 in the first record", "bits entry 17 in the last record"):
        assert rets[name] == 0, name
    mut = [r for n, r in rets.items() if "mutant" in n]
    assert len(mut) == 6 and any(r == 0 for r in mut) and any(r != 0 for r in mut)  # both sides of the status rule


def test_the_corpus_stays_compact():
    frames = K.corpus()
    assert sum(f["buf"].size for f in frames) <= 16 << 20
    big = [f["name"] for f in frames if f["w"] * f["h"] > 3 << 20]  # (a product-size piece of the largest records is a megapixel)
    assert sorted(big) == sorted(["4 pieces", "5 pieces", "8 pieces", "9 pieces"]), big
    assert len(frames) <= 64  # 4,4 parts: 8 workgroups a frame, 512 are resident at once
    assert max(f["w"] * f["h"] for f in frames) <= 9.5 * (1 << 20)


def test_record_sizes_offsets_and_runs():
    firsts, odds = set(), set()
    for f in _tagged("nibble"):
        nib = f["tags"]["nibble"]
        for which, want in ((1, nib), (0, 15 - nib)):
            s = K.model(f["buf"], which)
            sizes = {s.stride(p) for p in s.records}
            assert sizes == {K.SIZE[want]} and len(s.records) == s.R == 40, (f["name"], which, sizes)
            firsts.add(s.first_cand)
            odds.add(s.odd)
    assert firsts == set(range(8)) and odds == {0, 1}
    assert {K.SIZE[n] for n in range(16)} == {2, 10, 18, 26, 34, 42, 50, 66, 82, 130}  # the ten storage classes
    for f in _tagged("alternating"):
        which = 0 if f["tags"]["alternating"] == (2, 130) else 1
        s = K.model(f["buf"], which)
        assert [s.stride(p) for p in s.records] == list(f["tags"]["alternating"]) * (s.R // 2), f["name"]
    for f in _tagged("run"):
        s = K.model(f["buf"], 1)
        sizes = [s.stride(p) for p in s.records]
        change = [i for i in range(1, len(sizes)) if sizes[i] != sizes[i - 1]]
        assert change[0] == f["tags"]["run"] and change[1] == 2 * f["tags"]["run"], (f["name"], change)
    ends = set()
    for f in _tagged("list_ends"):
        s = K.model(f["buf"], 1)
        sizes = [s.stride(p) for p in s.records]
        change = tuple(i for i in range(1, len(sizes)) if sizes[i] != sizes[i - 1])
        assert change == tuple(sorted(f["tags"]["list_ends"])), (f["name"], change)
        ends |= set(change)
    # the first list of a decode holds SIDE_LCAP / 4 records, the next SIDE_LCAP more
    for lcap in (K.LCAP, _flag("shortunits", "MCRAW_SIDE_LCAP")):
        for full in (lcap // 4, lcap // 4 + lcap):
            assert {full - 1, full, full + 1} <= ends, (lcap, full, sorted(ends))


def test_pieces_and_boundaries():
    assert sorted(f["tags"]["pieces"] for f in _tagged("pieces")) == [1, 2, 3, 4, 5, 8, 9]
    for f in _tagged("pieces"):
        s = K.model(f["buf"], 1)
        assert s.pieces == f["tags"]["pieces"] and not s.dead, (f["name"], s.pieces)
    seen = set()
    for f in _tagged("straddle"):
        piece, reach = f["tags"]["straddle"]
        s = K.model(f["buf"], 1, piece)
        assert s.crossings()[0] == reach and not s.dead, (f["name"], s.crossings()[:3])
        if reach == 128:  # the record sits on the piece's last candidate
            p = [p for p in s.records if s.piece_of(p) == 0][-1]
            assert s.piece_end(0) - p == 2 and s.stride(p) == 130
        seen.add((piece, reach))
    assert seen == {(p, r) for p in (K.PIECE, 8192) for r in (0, 2, 64, 128)}


def test_ends():
    N = _by_name()
    for f in K.corpus():  # a whole frame's last stream ends exactly at `len`
        if f["whole"] and "guess" not in f["tags"] and f["name"] != "nat12 small":
            bo, ro = K.header(f["buf"])[2:]
            s = K.model(f["buf"], int(ro > bo))
            assert s.records[-1] + s.stride(s.records[-1]) == s.len and not s.dead, f["name"]
    s = K.model(N["ends one byte past len"]["buf"], 1)
    assert s.dead and len(s.records) == s.R - 1 and s.records[-1] + 82 + 82 == s.len + 1
    assert not K.model(N["count one short"]["buf"], 1).accepted and K.model(N["count one short"]["buf"], 0).accepted
    for f in _tagged("cut_piece"):
        s = K.model(f["buf"], 1)
        assert s.dead and s.pieces == f["tags"]["cut_piece"] + 1, (f["name"], s.pieces)
        lo, hi = s.parts(4)[-1]  # the partition follows `len`: the piece in which the chain ends is the last part's
        assert hi is None and lo <= f["tags"]["cut_piece"]
    for name in ("bits entry 17 in the first record", "bits entry 17 in the last record", "unused bits entries above 16"):
        f = N[name]
        vals = K.parse_stream(f["buf"], 0)[1]
        nblk = K.geometry(f["buf"])[0]
        at = f["tags"]["entry"]
        assert vals[at] > 16 and (at < nblk) == (not f["whole"]) and (vals[:nblk] > 16).sum() == (0 if f["whole"] else 1), name


def test_end_guesses():
    N = _by_name()
    f = N["end guess far too long"]
    s = K.model(f["buf"], 0)
    assert s.pieces == 1 and not s.dead
    for nsp in (2, 3, 4):  # every part but the first owns pieces behind the stream's end
        parts = s.parts(nsp)
        assert parts[0] == (0, parts[0][1]) and parts[0][1] >= 1 and all(lo >= 1 for lo, hi in parts[1:]), parts
    f = N["end guess too short"]
    s = K.model(f["buf"], 0)
    lo, hi = s.parts(2)[1]
    guess = (s.other - s.A0 + K.PIECE - 1) // K.PIECE
    assert s.other > s.so and hi is None and 0 < lo < guess < s.pieces and not s.dead, (lo, guess, s.pieces)  # records behind the last part's count
    r = K.model(f["buf"], 1)
    assert r.records == s.chain()[0][300:900] and not r.dead  # the refs stream is the bits stream from its record 300 on


def test_chains_that_never_join():
    f = _by_name()["chains never join"]
    s = K.model(f["buf"], 1)
    assert {s.stride(p) for p in s.records} == {130} and s.pieces == 3
    parts = s.parts(4)
    assert parts[2] == (1, 2)  # the middle part that counts from a speculative start
    got, true = s.spec_entry(2, 4, 8192)
    assert got != true and (got - true) % 130 != 0, (got, true)
    # ... and does not meet the true chain anywhere within the part's piece
    mine, _ = s.chain(start=got, until=s.piece_end(1))
    assert not set(mine) & set(s.records)


def test_natural_frames_miss_from_a_cold_start_and_hit_from_the_products():
    warm = _flag("coldspec", "MCRAW_SPEC_WARM")
    for f in _tagged("natural"):
        s = K.model(f["buf"], 1)
        parts = s.parts(4)
        mid = [q for q in (1, 2) if parts[q][0] > 0 and parts[q][1] > parts[q][0]]
        assert mid, (f["name"], parts)
        cold = [s.spec_entry(q, 4, warm) for q in mid]
        assert any(got != true for got, true in cold), (f["name"], cold)
        assert all(got == true for got, true in (s.spec_entry(q, 4, 8192) for q in mid)), f["name"]


def test_the_walk_model_on_the_corpus():
    frames = K.corpus()
    ratio = _flag("earlyswitch", "MCRAW_SEGW_RATIO")
    assert 8 * ratio > K.LCAP  # from the 8th pass on a unit is below `ratio` records per pass whatever it listed
    N = _by_name()
    for name, which in (("noise14", 1), ("66/82 alternating", 1)):
        assert K.model(N[name]["buf"], which).walk()["segw_switch"] == 1, name
    assert K.model(N["runs of 64"]["buf"], 1).walk()["run_passes64"] > 0
    prod, early, never = K.census_model(frames), K.census_model(frames, ratio=ratio), K.census_model(frames, ratio=0)
    # (the streams of eight and more passes, found where nothing switches: a unit whose 8th pass still has the chain in the piece)
    assert early["segw_switch"] == never["early_streams"] > prod["segw_switch"] > 0 == never["segw_switch"]
    assert prod["records"] == early["records"] == never["records"] == K.census_model(frames, force_segw=True)["records"]
    short = K.census_model(frames, lcap=_flag("shortunits", "MCRAW_SIDE_LCAP"))
    assert short["units_full"] > prod["units_full"] and short["segw_resumed"] > prod["segw_resumed"]
    small = K.census_model(frames, piece=8192)
    assert small["piece_steps"] > 3 * prod["piece_steps"]
    assert prod["dead"] == sum(K.model(f["buf"], w).dead for f in frames for w in (0, 1)) >= 4
