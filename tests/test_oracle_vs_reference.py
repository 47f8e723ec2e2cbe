"""CPU: oracle == real reference on randomized frames.  Where the reference build is present (oracle/_ref) every frame is
decoded by it too; elsewhere the oracle is compared with the answers the reference gave for the same bytes when
tests/golden/ref_answers.json was written (return value and SHA-1 of the decoded mosaic per frame:
`python tests/test_oracle_vs_reference.py --record`, where the reference is built)."""
import hashlib
import json
import os

import numpy as np
import pytest

import _libs as L

ANSWERS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_answers.json")
_record = None  # {key: [ret, sha1]} while --record runs


def _answers():
    with open(ANSWERS) as f:
        return json.load(f)


def _reference(key, typ, buf, w, h):
    """The reference's (return value, SHA-1 of its first h rows) for these bytes: computed where the reference was built (and
    checked against the stored answer), else the stored answer."""
    got = None
    if L.ref() is not None:
        rr, orr = (L.ref_decode7 if typ == 7 else L.ref_decode6)(buf, w, h)
        got = [int(rr), hashlib.sha1(np.ascontiguousarray(orr[:h]).tobytes()).hexdigest()]
        if _record is not None:
            _record[key] = got
            return got
    want = _answers()[key]
    assert got is None or got == want, (key, got, want)
    return want


def _check(key, typ, buf, w, h, ro, oo, ret):
    rr, digest = _reference(key, typ, buf, w, h)
    assert ro == rr == ret, (key, ro, rr, ret)
    assert hashlib.sha1(np.ascontiguousarray(oo).tobytes()).hexdigest() == digest, key


T7_RANDOM = [(128, 8), (256, 64), (192, 12), (100, 8), (77, 4), (64, 4), (4032 // 4, 3024 // 4)]
T6_RANDOM = [(96, 4), (80, 6), (75, 5), (256, 16), (33, 3), (1920 // 2, 1080 // 4)]
T7_FULL = [
    (1920, 1080, 10, 0, 0), (1920, 1080, 10, 1, 4),          # BASELINE config 1, both distributions
    (4032, 3024, 12, 1, 12), (4032, 3024, 12, 0, 0),         # config 2: Nat and U
    (3840, 2160, 12, 1, 12), (3840, 2160, 12, 0, 0),         # config 3's frame (the bench line's): Nat and U
    (4032, 3024, 14, 0, 0),                                  # config 4's 14-bit frames
    (7680, 4320, 12, 1, 12),                                 # config 5's frame
]
T6_FULL = [
    (4000, 3000, 12, 1, 12, 0),                              # the bench's legacy leg; width % 32 == 0
    (4000, 3000, 14, 0, 0, 1),                               # config 4's 14-bit legacy frames, with a trailer
    (1920, 1080, 10, 1, 4, 0), (1920, 1080, 10, 0, 0, 1),    # config 1's frame as legacy
    (4032 - 5, 3024 // 4, 12, 1, 12, 1),                     # a padded width at full row length
]


@pytest.mark.parametrize("w,h", T7_RANDOM)
def test_type7_random(w, h):
    rng = np.random.default_rng(w * 131 + h)
    encW, encH = (w + 63) // 64 * 64, (h + 3) // 4 * 4
    for trial in range(6):
        nb = int(rng.integers(1, 17))
        img = rng.integers(0, 1 << nb, size=(h, w), dtype=np.uint16)
        mb = rng.integers(0, 17, size=encW * encH // 64).astype(np.uint8) if trial % 2 else None
        buf = L.encode7(img, mb)
        ro, oo = L.oracle_decode7(buf, w, h)
        _check("t7_random/%dx%d/%d" % (w, h, trial), 7, buf, w, h, ro, oo, w * encH)
        assert np.array_equal(oo, img)


@pytest.mark.parametrize("w,h", T6_RANDOM)
def test_type6_random(w, h):
    rng = np.random.default_rng(w * 17 + h)
    for trial in range(6):
        nb = int(rng.integers(1, 17))
        img = rng.integers(0, 1 << nb, size=(h, w), dtype=np.uint16)
        nrec = ((w + 31) // 32) * 2 * h
        mb = rng.integers(0, 16, size=nrec).astype(np.uint8) if trial % 2 else None
        buf = L.encode6(img, mb, flags=trial & 1)
        ro, oo = L.oracle_decode6(buf, w, h)
        _check("t6_random/%dx%d/%d" % (w, h, trial), 6, buf, w, h, ro, oo, w * h)
        assert np.array_equal(oo, img)


@pytest.mark.parametrize("w,h,nb,dist,sig", T7_FULL)
def test_full_size_type7(w, h, nb, dist, sig):
    img = L.synth_image(w, h, nb, dist, sig, 1000 + dist)
    buf = L.encode7(img)
    ro, oo = L.oracle_decode7(buf, w, h)
    _check("t7_full/%dx%d/%d/%d/%g" % (w, h, nb, dist, sig), 7, buf, w, h, ro, oo, w * h)
    assert np.array_equal(oo, img)


@pytest.mark.parametrize("w,h,nb,dist,sig,flags", T6_FULL)
def test_full_size_legacy(w, h, nb, dist, sig, flags):
    img = L.synth_image(w, h, nb, dist, sig, 2000 + dist)
    buf = L.encode6(img, None, flags)
    ro, oo = L.oracle_decode6(buf, w, h)
    _check("t6_full/%dx%d/%d/%d/%g/%d" % (w, h, nb, dist, sig, flags), 6, buf, w, h, ro, oo, w * h)
    assert np.array_equal(oo, img)


if __name__ == "__main__":  # python tests/test_oracle_vs_reference.py --record: the reference's answers, where it is built
    import sys
    if sys.argv[1:] != ["--record"] or L.ref() is None:
        sys.exit("usage: python tests/test_oracle_vs_reference.py --record  (needs the reference build: make -C oracle ref)")
    _record = {}
    for a in T7_RANDOM:
        test_type7_random(*a)
    for a in T6_RANDOM:
        test_type6_random(*a)
    for a in T7_FULL:
        test_full_size_type7(*a)
    for a in T6_FULL:
        test_full_size_legacy(*a)
    with open(ANSWERS, "w") as f:
        json.dump(_record, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d frames" % (ANSWERS, len(_record)))
