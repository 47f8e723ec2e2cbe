"""The legacy corpus of tests/_legacy_corpus.py is what it says it is (CPU): every unmutated frame decodes to its image through
the oracle, has the number of segments it was made for, and the frames made for a rare path of k6_decode's sure entry reach
that path by a plain model of it."""
import numpy as np

import _legacy_corpus as K


def test_every_whole_frame_round_trips_and_has_its_segment_count():
    frames, expect = K.corpus(), K.expectations()
    assert len(frames) == len(expect)
    for f, (ret, out) in zip(frames, expect):
        if f["segs"] is not None:
            assert K.segments(f["buf"].size) == f["segs"], (f["name"], f["buf"].size)
        if f["whole"]:
            assert ret == f["w"] * f["h"] and np.array_equal(out, f["img"]), f["name"]
    assert sorted({f["segs"] for f in frames if f["segs"]}) == [1, 2, 7, 8, 9, 16, 17, 33, 69]
    assert max(K.segments(f["buf"].size) for f in frames) >= 48
    # streams that end a few bytes into a segment and just short of one
    tails = {f["buf"].size % K.SEG6 for f in frames if f["segs"]}
    assert {1, 5, K.SEG6 - 1, K.SEG6 - 3} <= tails
    assert any(f["w"] % 32 for f in frames) and any(f["h"] % 4 for f in frames)


def test_the_corpus_stays_compact():
    frames = K.corpus()
    assert sum(f["buf"].size for f in frames) <= 20 << 20
    assert all(f["w"] * f["h"] <= 1 << 20 for f in frames)
    assert sum(1 for f in frames if not f["whole"] and f["img"] is None and "mutant" in f["name"]) == 12


def test_the_cut_stream_and_some_mutants_are_rejected_by_the_oracle():
    frames, expect = K.corpus(), K.expectations()
    rets = {f["name"]: ret for f, (ret, _) in zip(frames, expect)}
    assert rets["cut inside a late segment"] == 0
    mut = [ret for f, (ret, _) in zip(frames, expect) if "mutant" in f["name"]]
    assert any(r == 0 for r in mut) and any(r != 0 for r in mut)  # both sides of the status rule


def test_the_frames_made_for_the_sure_entrys_rare_ways_reach_them():
    by_name = {f["name"]: f for f in K.corpus()}
    late = K.front_kinds(by_name["late front"]["buf"])
    assert late[0] is not None and late[0] > 0, late       # segment 1: its chains become one inside it
    assert all(k == 0 for k in late[1:])
    never = K.front_kinds(by_name["never unanimous"]["buf"])
    assert never and all(k is None for k in never[:-1])    # (the last segment ends with the stream)
    assert all(k == 0 for k in K.front_kinds(by_name["nat12 9 segments, ends 5 bytes in"]["buf"])[:-1])
