"""GPU (-m gpu): every rare path of k6_decode, forced and counted, against the oracle.

Which of its paths a segment of a legacy stream takes in k6_decode (csrc/mcraw_type6.hip) is decided by the stream's content
and, for the look-back, by timing: the parity suite compares pixels on a good set of contents but neither makes the kernel take
a chosen path nor checks which one it took.  Here eleven builds of the same sources -- the product's code with the path census
(-DMCRAW_PATHS6), and ten that also force one path each (build.K6_PATH_VARIANTS; every switch chooses among paths that are
valid for every input, see the kernel source) -- decode the corpus of tests/_legacy_corpus.py in a child process each
(tests/_k6_paths_child.py: one batch, frame by frame, reversed batch; a few frames through the 12-bit-strip and f16-plane
stages that share the unpack loop).  The child compares every frame with the oracle (pixels, return value, status rule of the
fuzz suite); this module compares the census with what the corpus and the switch determine -- exact counts where content or
the switch decides, nothing where timing alone does:

  census      every content-driven counter is above zero: careful segments, repair rounds, late front (the corpus frame "late
              front" reaches it by construction, tests/test_legacy_corpus.py), no front and its maps, the three ways to build
              the lists, both list layouts, waves of several rounds
  polls0      no look-back resolved by scalar polls or handed over: all of them by vector polls
  polls1      one scalar window, then the hand-over of `base` / `jn`: pixels, and the look-backs add up
  slowprefix  prefix words come late, look-backs run window by window to the frame's front: hand-overs with a sum on the
              frames of 16 and more segments
  careful     every segment walks the careful way, no list comes from notes
  latefront   no segment with a predecessor is entered from its own front
  nofront     every segment with a predecessor is entered through maps; every full one publishes its own
  nolean      no list is built by the resolving wave
  pairmode    every live wave unpacks from the layout by pairs
  warm64      walkers start 64 bytes in front of their quarters: at least as many repaired segments as the product
  poison      the staged front is overwritten behind the resolve: pixels only.  (One store of the whole front, list 0's place
              and the rest, before any list is written -- not list 0's place before and the rest after the resolver's entries:
              list 0 is written over its part afterwards, and the wave of the sure entry, the front's last reader, is by then
              held at the next barrier; no barrier is added)
  every one   nothing lost, every segment counted once, the look-backs add up to the segments that have a predecessor

A child that ends by a signal or runs into its time limit is followed by no more GPU work from this module or any other (tests/_paths_harness.py): the remaining
variants fail at once.  Nothing is tried twice.

Wall times on an MI355X, one run of the module (11 passed in 26.0 s).  Per variant: the child's own `seconds` (from its first
line to its result: corpus, decodes, comparisons) / the whole test (link of the variant, start of the child with its imports, child):
  census 0.22 / 2.37   polls0 0.23 / 2.37   polls1 0.23 / 2.40   slowprefix 0.22 / 2.35   careful 0.22 / 2.22   latefront 0.22 / 2.17
  nofront 0.23 / 2.25  nolean 0.24 / 2.22   pairmode 0.22 / 2.10  warm64 0.23 / 2.41      poison 0.24 / 2.57
The child process is what the time limit is on; it is no slower than the test around it, 2.57 s at the most.  CHILD_TIMEOUT is
ten times that."""
import json
import os

import numpy as np
import pytest

import _paths_harness as PH
from motioncam_decoder_amd import build as B

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "_k6_paths_child.py")
CHILD_TIMEOUT = 25   # seconds: ten times the slowest measured child (see above)
PASSES = 3           # one batch, frame by frame, reversed batch


POST_FRAMES = ("nat12 w200 1 segment", "nat12 8 segments, ends 3 bytes short", "mixed nibbles (1, 2, 3)", "late front")
POST_BLACK, POST_WHITE = (60, 64, 68, 1000), 4095.0


def make_npz(path):
    """The corpus and what the oracle makes of it, as a file for the children.  -> the corpus' segment totals"""
    import _float_ref as R
    import _legacy_corpus as K
    import _libs as L
    import motioncam_decoder_amd as M
    frames, expect = K.corpus(), K.expectations()
    arrays = {"meta": np.array([[f["w"], f["h"], ret, K.segments(f["buf"].size)] for f, (ret, _) in zip(frames, expect)], np.int64)}
    for i, (f, (ret, out)) in enumerate(zip(frames, expect)):
        arrays["buf%d" % i] = f["buf"]
        arrays["out%d" % i] = out
    plane = M.cfa_planes("grbg")
    sub = [i for i, f in enumerate(frames) if f["name"] in POST_FRAMES]
    assert len(sub) == len(POST_FRAMES)
    for i in sub:
        img = frames[i]["img"]
        arrays["strip%d" % i] = L.oracle_post(img, list(POST_BLACK), bits=12)
        arrays["planes%d" % i] = R.ref_bytes(img, "f16", POST_WHITE, "planes", POST_BLACK, False, plane)
    arrays.update(post_frames=np.array(sub), post_black=np.array(POST_BLACK), post_white=np.array(POST_WHITE), post_plane=np.array(plane))
    np.savez(path, **arrays)
    sizes = [f["buf"].size for f in frames]
    return dict(segments=sum(K.segments(s) for s in sizes), with_pred=sum(K.segments(s) - 1 for s in sizes),
                full_with_pred=sum(K.full_segments_with_predecessor(s) for s in sizes),
                big_with_pred=sum(K.segments(s) - 1 for s in sizes if K.segments(s) >= 16))


@pytest.fixture(scope="module")
def corpus_npz(tmp_path_factory):
    """Computed once for the module: (the file, the totals)."""
    path = str(tmp_path_factory.mktemp("k6_paths") / "corpus.npz")
    return path, make_npz(path)


def _child(variant, corpus_npz, tmp_path_factory):
    """The census of `variant`'s child, which is run once whatever becomes of it (tests/_paths_harness.py)."""
    res = PH.run_child(__name__, variant, CHILD, [corpus_npz[0]], B.K6_PATH_VARIANTS[variant], "libmcraw_k6_%s.so" % variant, CHILD_TIMEOUT,
                      tmp_path_factory, PH.no_errors("frames differ from the oracle"))
    print(variant, json.dumps(res))
    return res


@pytest.mark.parametrize("variant", list(B.K6_PATH_VARIANTS))
def test_k6_decode_paths(variant, corpus_npz, tmp_path_factory):
    res = _child(variant, corpus_npz, tmp_path_factory)
    T = corpus_npz[1]
    c, big = res["plain"], res["big"]
    # ---- every variant
    for part, segs, pred in ((c, PASSES * T["segments"], PASSES * T["with_pred"]), (big, None, T["big_with_pred"])):
        assert part["lost"] == 0, part
        assert segs is None or part["segments"] == segs, (part, segs)
        assert part["lb_scalar"] + part["lb_vector"] + part["lb_handed"] == pred, (part, pred)
        assert part["front0"] + part["latefront"] + part["nofront"] == pred, (part, pred)
        assert part["noted"] + part["coop"] + part["noncoop"] == part["segments"], part
        assert part["waves_pair"] <= part["waves"] and part["maps"] <= part["nofront"], part
    assert res["post"]["lost"] == 0 and res["post"]["segments"] > 0
    # ---- what the variant is about
    if variant == "census":
        for k in ("careful", "repaired", "latefront", "nofront", "maps", "noted", "coop", "noncoop", "waves_pair", "waves_multi"):
            assert c[k] > 0, (k, c)
        assert c["waves_pair"] < c["waves"], c  # (and the layout by records)
    elif variant == "polls0":
        for part, pred in ((c, PASSES * T["with_pred"]), (big, T["big_with_pred"])):
            assert part["lb_scalar"] == 0 and part["lb_handed"] == 0 and part["lb_vector"] == pred, (part, pred)
    elif variant == "slowprefix":
        assert big["lb_handed"] > 0, big
    elif variant == "careful":
        assert c["careful"] == c["segments"] and c["noted"] == 0, c
    elif variant == "latefront":
        assert c["front0"] == 0 and big["front0"] == 0, (c, big)
        assert c["latefront"] > 0, c
    elif variant == "nofront":
        assert c["nofront"] == PASSES * T["with_pred"] and c["maps"] == PASSES * T["full_with_pred"], (c, T)
    elif variant == "nolean":
        assert c["noted"] == 0 and c["coop"] == 0 and c["noncoop"] == c["segments"], c
    elif variant == "pairmode":
        assert c["waves_pair"] == c["waves"] and c["waves"] > 0, c
    elif variant == "warm64":
        product = _child("census", corpus_npz, tmp_path_factory)["plain"]
        assert c["repaired"] >= product["repaired"], (c["repaired"], product["repaired"])
    else:
        assert variant in ("polls1", "poison")  # pixels, and the sums above
