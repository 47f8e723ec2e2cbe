"""GPU (-m gpu): every way of k7_side's chain walk, forced and counted, against the oracle.

Which way a side stream goes in k7_side (csrc/mcraw_type7.hip) -- runs or segment walkers and the switch between them, repair
rounds, how its units end, and for streams in parts the count, the hand-off and the replay -- is decided by the stream's content
and, for the hand-off, by timing.  The other suites compare pixels on contents chosen for other reasons; here ten builds of the
same sources -- the product's code with the path census (-DMCRAW_PATHS7), and nine that also force one way each
(build.K7_PATH_VARIANTS; every switch chooses among ways that are valid for every input, see the kernel source) -- decode the
corpus of tests/_side7_corpus.py in a child process each (tests/_k7_paths_child.py: the library's own choice and one workgroup
per stream as one batch, frame by frame and as a reversed batch; every stream in 2,2 / 4,4 / 3,2 parts, the last also without the
last part's count).  The child compares every frame with the oracle (pixels, return value, status rule of the fuzz suite, rows
below a short frame and a guard band behind every output); this module compares the census with what the model of
tests/_side7_corpus.py and the switch determine -- exact counts where content or the switch decides, nothing where timing alone does:

  every one    workgroups = two per frame times the parts; records decoded and dead chains reported are the model's in every
               setting; the six outcomes of the hand-off add up to the parts; no part gives up waiting (but `mute`), and then
               each outcome's count is the model's, as are the last parts whose count stood; with one workgroup per stream
               the units, how they end, the run passes, the switches and the walkers' pieces are the model's
  census       every content-driven counter is above zero somewhere (see CENSUS_DRIVEN and NOT_DRIVEN)
  segw         no run pass at all            noswitch     no call of the walkers
  earlyswitch  the streams that hand over are the model's streams of eight and more passes
  warm1        at least as many repaired calls of the walkers as `segw`
  coldspec     at least as many speculative counts miss as in `census`, some of them (more than the adversarial stream's)
  mute         every part 1 that asks gives up waiting (part 0 never tells): their number, and that of those with pieces of their
               own, is the model's; parts 2 and 3 may hear their predecessor in time -- timing --, so for all parts together only
               the bounds hold: no fewer give up than the parts 1, no more than ask; units are walked and skipped
  shortunits   more full lists and more resumed pieces than `census`
  smallpieces  the piece steps are the model's at 8 KiB
  poison       pixels, and the sums above

A child that ends by a signal, at its time limit or without its result stops every further child, of this module and of every other (tests/_paths_harness.py): the remaining variants fail at
once.  Nothing is tried twice.

Wall times on an MI355X, one run of the module (10 passed in 26.5 s; the corpus and the oracle's answers, made once: 0.55 s).  Per
variant: the child's own `seconds` (from its first line to its result: 136 decode calls and their comparisons) / the whole test
(link of the variant, start of the child with its imports, child, the model):
  census 0.82 / 3.07   segw 0.44 / 2.53        noswitch 0.44 / 2.64     earlyswitch 0.49 / 2.70  warm1 0.43 / 2.34
  coldspec 0.43 / 2.58 mute 0.41 / 2.31        shortunits 0.42 / 2.57   smallpieces 0.40 / 2.32  poison 0.43 / 2.42
The child process is what the time limit is on; it is no slower than the test around it, 3.07 s at the most.  CHILD_TIMEOUT is
ten times that."""
import json
import os

import numpy as np
import pytest

import _paths_harness as PH
from motioncam_decoder_amd import build as B

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "_k7_paths_child.py")
CHILD_TIMEOUT = 31  # seconds: ten times the slowest measured whole test (see above)

# setting of the child -> (passes over the corpus, parts of the bits stream, parts of the refs stream)
SETTINGS = {"default": (3, 1, 1), "one": (3, 1, 1), "2,2": (1, 2, 2), "4,4": (1, 4, 4), "3,2": (1, 3, 2), "3,2 lastc0": (1, 3, 2)}
# how the model walks for a variant (Stream.walk's arguments, the piece size)
WALK = {"segw": dict(force_segw=True), "warm1": dict(force_segw=True), "noswitch": dict(ratio=0), "earlyswitch": dict(ratio=65),
        "shortunits": dict(lcap=256), "smallpieces": dict(piece=8192)}
EXACT_UNSPLIT = ("units", "units_full", "piece_steps", "units_dead", "run_passes", "run_passes64", "segw_switch", "segw_pieces", "segw_resumed")
# counters that content drives and the corpus reaches in the product's build, summed over the settings
CENSUS_DRIVEN = ("streams", "rejected", "records", "units", "units_full", "piece_steps", "units_dead", "dead", "run_passes", "run_passes64",
                 "segw_switch", "segw_pieces", "segw_repaired", "segw_rounds2", "segw_resumed", "parts", "part_empty", "counted", "spec", "ho_over",
                 "ho_pass", "ho_last", "ho_hit", "ho_miss", "lastc_replayed", "replay_units", "replay_pieceflag", "replay_tail",
                 "told_late", "items_behind_part0", "truncated_by_tiles")
# ... and those it cannot: a unit is skipped only by a part whose predecessor never spoke (every other part starts in its own
# first piece), and no part of these batches gives up waiting: both are what the `mute` build is for
NOT_DRIVEN = ("ho_mute", "ho_mute_work", "ho_mute_part1", "skipped_units")

_models = {}


def make_npz(path):
    """The corpus and what the oracle makes of it, as a file for the children."""
    import _side7_corpus as K
    frames, expect = K.corpus(), K.expectations()
    arrays = {"meta": np.array([[f["w"], f["h"], ret] for f, (ret, _) in zip(frames, expect)], np.int64)}
    for i, (f, (ret, out)) in enumerate(zip(frames, expect)):
        rows = out[: ret // f["w"]]
        arrays["buf%d" % i] = f["buf"]
        # (most frames are flat within every tile of 64 x 4 pixels: one value per tile then, which the child spreads out again)
        tiles = rows[::4, ::64]
        flat = rows.size and rows.shape[0] % 4 == 0 and f["w"] % 64 == 0 and np.array_equal(np.repeat(np.repeat(tiles, 4, 0), 64, 1), rows)
        arrays["out%d" % i] = tiles if flat else rows
        arrays["tiled%d" % i] = np.array(bool(flat))
    np.savez(path, **arrays)


def model(variant):
    """What the model says of the corpus for `variant`'s way to walk: the census of one pass with one workgroup per stream, and
    per split setting the parts that ask a predecessor and the outcomes of the hand-off."""
    import _side7_corpus as K
    kw = dict(WALK.get(variant, {}))
    key = json.dumps(kw, sort_keys=True) + (variant if variant in ("coldspec", "smallpieces") else "")
    if key not in _models:
        piece = kw.get("piece", K.PIECE)
        frames = K.corpus()
        m = K.census_model(frames, **kw)
        streams = [K.Stream(f["buf"], which, piece) for f in frames for which in (0, 1)]
        warm = next((int(f.split("=")[1]) for f in B.K7_PATH_VARIANTS[variant] if f.startswith("-DMCRAW_SPEC_WARM=")), 8192)
        for name, (_, nb, nr) in SETTINGS.items():
            if nb + nr > 2:
                live = [s for s in streams if s.accepted]
                ask = [s.asking_parts(nr if s.which else nb) for s in live]
                m["asking " + name] = {k: sum(a[k] for a in ask) for k in ask[0]}
                ho = [s.handoff(nr if s.which else nb, warm, lastc="lastc0" not in name) for s in live]
                m["handoff " + name] = {k: sum(h[k] for h in ho) for k in ho[0]}
        m["frames"] = len(frames)
        _models[key] = m
    return _models[key]


@pytest.fixture(scope="module")
def corpus_npz(tmp_path_factory):
    """Computed once for the module."""
    path = str(tmp_path_factory.mktemp("k7_paths") / "corpus.npz")
    make_npz(path)
    return path


def _child(variant, corpus_npz, tmp_path_factory):
    """The census of `variant`'s child, which is run once whatever becomes of it (tests/_paths_harness.py)."""
    res = PH.run_child(__name__, variant, CHILD, [corpus_npz], B.K7_PATH_VARIANTS[variant], "libmcraw_k7_%s.so" % variant, CHILD_TIMEOUT,
                      tmp_path_factory, PH.no_errors("frames differ from the oracle"))
    print(variant, json.dumps(res))
    return res


def check(variant, res, others):
    """The census `res` of `variant`'s child against the model; others(name): another variant's census."""
    T = model(variant)
    for name, (passes, nb, nr) in SETTINGS.items():
        c = res[name]
        # ---- every variant and setting
        assert c["streams"] + c["rejected"] == T["frames"] * (nb + nr) * passes, (name, c)
        assert c["records"] == passes * T["records"], (name, c["records"], T["records"])
        assert c["dead"] == passes * T["dead"], (name, c["dead"], T["dead"])
        assert c["parts"] == (0 if nb + nr == 2 else c["streams"]), (name, c)
        assert sum(c[k] for k in ("ho_mute", "ho_over", "ho_pass", "ho_last", "ho_hit", "ho_miss")) == c["parts"], (name, c)
        # (a batch is 128 to 512 workgroups, two per CU on 256 CUs: every one is resident, and a part waits 2^19 polls for the one it asks)
        if variant != "mute":
            assert c["ho_mute"] == 0 and c["skipped_units"] == 0, (name, c)
        assert c["counted"] > 0 or c["replay_units"] == 0, (name, c)
        assert c["units_full"] + c["piece_steps"] + c["units_dead"] == c["units"] and c["run_passes64"] <= c["run_passes"], (name, c)
        assert c["segw_rounds2"] <= c["segw_repaired"] <= c["segw_pieces"] and c["lastc_replayed"] <= c["ho_last"], (name, c)
        if nb + nr > 2 and variant != "mute":  # (every part in front speaks in time: which outcome a part takes is decided by content)
            for k, v in T["handoff " + name].items():
                assert c[k] == v, (name, k, c[k], T["handoff " + name])
        # ---- one workgroup per stream: the walk is the model's
        if nb + nr == 2:
            assert c["streams"] == passes * T["streams"] and c["rejected"] == passes * T["rejected"], (name, c)
            for k in EXACT_UNSPLIT:
                assert c[k] == passes * T[k], (name, k, c[k], passes * T[k])
    total = {k: sum(res[name][k] for name in SETTINGS) for k in res["default"]}
    split = [name for name, (_, nb, nr) in SETTINGS.items() if nb + nr > 2]
    # ---- what the variant is about
    if variant == "census":
        for k in CENSUS_DRIVEN:
            assert total[k] > 0, (k, total)
        for k in NOT_DRIVEN:
            assert total[k] == 0, (k, total)
    elif variant in ("segw", "warm1"):
        assert total["run_passes"] == 0 and total["segw_switch"] == 0 and total["segw_pieces"] > 0, total
        if variant == "warm1":
            assert total["segw_repaired"] >= sum(others("segw")[name]["segw_repaired"] for name in SETTINGS), total
    elif variant == "noswitch":
        assert total["segw_pieces"] == 0 and total["segw_switch"] == 0, total
    elif variant == "earlyswitch":
        for name in ("default", "one"):
            # (the model's streams of eight and more passes are found where nothing switches: the walk with ratio 0)
            assert res[name]["segw_switch"] == 3 * model("noswitch")["early_streams"] > 3 * model("census")["segw_switch"], (name, res[name])
    elif variant == "coldspec":
        product = others("census")
        for name in split:
            assert res[name]["ho_miss"] >= product[name]["ho_miss"], (name, res[name], product[name])
        # (the adversarial stream misses in both builds; what coldspec adds is the natural frames' middle parts, tests/test_side7_corpus.py)
        assert res["4,4"]["ho_miss"] >= product["4,4"]["ho_miss"] + 2, (res["4,4"], product["4,4"])
    elif variant == "mute":
        # Part 0 never tells, so every part 1 that asks gives up: content alone decides how many those are, and how many of them own
        # pieces.  Parts 2 and 3 ask a part that does tell, behind its own decode: whether they hear it in time is timing, and all
        # that holds for them is that no more parts give up than ask.  (With two parts per stream every asking part is part 1.)
        for name in split:
            c, A = res[name], T["asking " + name]
            assert c["ho_mute_part1"] == A["part1"] > 0, (name, c, A)
            assert A["part1_work"] <= c["ho_mute_work"] <= A["asking_work"] and A["part1_work"] > 0, (name, c, A)
            assert A["part1"] <= c["ho_mute"] <= A["asking"], (name, c, A)
        assert res["2,2"]["ho_mute_work"] == T["asking 2,2"]["asking_work"] == T["asking 2,2"]["part1_work"], (res["2,2"], T["asking 2,2"])
        assert total["skipped_units"] > 0, total
    elif variant == "shortunits":
        product = others("census")
        for k in ("units_full", "segw_resumed"):
            assert total[k] > sum(product[name][k] for name in SETTINGS), (k, total)
    elif variant == "smallpieces":
        assert res["one"]["piece_steps"] == 3 * T["piece_steps"] > 3 * model("census")["piece_steps"], (res["one"], T)
    else:
        assert variant == "poison" and total["replay_units"] > 0, total  # pixels, and the sums above


@pytest.mark.parametrize("variant", list(B.K7_PATH_VARIANTS))
def test_k7_side_paths(variant, corpus_npz, tmp_path_factory):
    res = _child(variant, corpus_npz, tmp_path_factory)
    check(variant, res, lambda name: _child(name, corpus_npz, tmp_path_factory))
