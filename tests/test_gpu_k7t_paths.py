"""GPU (-m gpu): every item, block, lean and store path of k7_tiles, counted and forced, against the oracle and an exact model.

k7_tiles (csrc/mcraw_type7.hip) turns the payload of every type-7 frame into pixels, in seven instances (the plain mosaic / uint16
with black levels, 10-, 12- and 14-bit strips, f32 / f16 / bf16 rows or planes).  Which of its ways an item goes -- valid, short,
empty or full span, lean or not and why not, which store form a row piece takes, whether the merged 14-bit store is taken, stores
forward or back, or declines -- is decided by content and geometry alone.  The other suites compare pixels on contents chosen by
hand; here five builds of the same sources -- the product's code with the path census (-DMCRAW_PATHST), and four that also force
one way each (build.K7T_PATH_VARIANTS; every switch chooses among ways that are valid for every input, see the head of the kernel
source) -- decode the corpus of tests/_tiles7_model.py in a child process each (tests/_k7t_paths_child.py) under the 19 settings of
its SETTINGS, which reach every instance and both float layouts.  The child compares every frame byte for byte with what this
module worked out from the oracle (L.oracle_decode7, L.oracle_post, tests/_float_ref.py), the bytes around every output included;
this module compares the census of every setting with the model, EVERY counter, EXACTLY: none depends on timing.

  every one    census == model(setting, variant), counter by counter
  census       every counter is above zero in the settings named for it (DRIVEN names every counter: none is left undriven)
  nolean       no lean item; the items that are not lean are the product's lean and not lean ones
  slowstore    no piece on the fast grid, no merged store; the whole pieces off the grid are all the product's whole pieces
  nomerge      no merged store and no decline; the plain 14-bit forms take the merged pieces
  poison       pixels, and every count as in `census` (a pixel that changes proves a dependence on LDS the item never staged)

A child that ends by a signal, at its time limit or without its result stops every further child, of this module and of every other (tests/_paths_harness.py): the remaining variants fail at
once.  Nothing is tried twice.

Wall times on an MI355X, one run of the module (5 passed in 32.5 s).  Per variant: the child's own `seconds` (from its first line
to its result: 19 contexts, 501 decode calls and their comparisons) / the whole test (the variant's object compiled where none
came with the tree, the link, start of the child with its imports, child, the models; `census` also makes the corpus, the oracle's
answers and the file for the children):
  census 0.89 / 10.94   nolean 0.78 / 5.36   slowstore 0.76 / 5.28   nomerge 0.76 / 5.17   poison 0.75 / 5.29
CHILD_TIMEOUT is ten times the slowest whole test; it guards against a hang, not against performance."""
import json
import os

import numpy as np
import pytest

import _paths_harness as PH
from motioncam_decoder_amd import build as B

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "_k7t_paths_child.py")
CHILD_TIMEOUT = 110  # seconds: ten times the slowest measured whole test (see above)

MERGED = ("st_merged_fwd", "st_merged_back")


def make_npz(path):
    """The corpus, the plan of the settings and what the oracle makes of every frame under each, as a file for the children."""
    import _tiles7_model as T
    frames, expect = T.corpus(), T.expectations()
    arrays = {"meta": np.array([[f["w"], f["h"], ret] for f, (ret, _) in zip(frames, expect)], np.int64)}
    for i, f in enumerate(frames):
        arrays["buf%d" % i] = f["buf"]
    plan = []
    for s, (name, S) in enumerate(T.SETTINGS.items()):
        bat = T.batches(name)
        alloc = {}
        for i in sorted({i for b in bat for i in b}):
            arrays["exp_%d_%d" % (s, i)], alloc[str(i)] = T.expected_bytes(name, i)
            assert arrays["exp_%d_%d" % (s, i)].dtype == np.uint8 and arrays["exp_%d_%d" % (s, i)].size <= alloc[str(i)]
        plan.append(dict(name=name, env=S.get("env", {}), stage=S.get("stage"), off=S.get("off", 0), batches=bat, alloc=alloc))
    arrays["plan"] = np.array(json.dumps(plan))
    np.savez(path, **arrays)


@pytest.fixture(scope="module")
def corpus_npz(tmp_path_factory):
    """Computed once for the module."""
    path = str(tmp_path_factory.mktemp("k7t_paths") / "corpus.npz")
    make_npz(path)
    return path


def _child(variant, corpus_npz, tmp_path_factory):
    """The census of `variant`'s child, which is run once whatever becomes of it (tests/_paths_harness.py)."""
    res = PH.run_child(__name__, variant, CHILD, [corpus_npz], B.K7T_PATH_VARIANTS[variant], "libmcraw_k7t_%s.so" % variant, CHILD_TIMEOUT,
                      tmp_path_factory, PH.no_errors("frames differ from the oracle"))
    print(variant, json.dumps(res))
    return res


def check(variant, res):
    """The census `res` of `variant`'s child against the model."""
    import _tiles7_model as T
    assert res["paths"] == T.PATHS, "the child's counters are not the model's"
    for setting in T.SETTINGS:
        got, want = res[setting], T.model(setting, variant)
        product = T.model(setting)
        print(variant, setting, "census", json.dumps(got), "model", json.dumps(want))
        # ---- every variant and setting: the model, exactly
        for k in T.PATHS:
            assert got[k] == want[k], (variant, setting, k, got[k], want[k])
        # ---- what the variant is about
        if variant in ("census", "poison"):
            for k, settings in T.DRIVEN.items():
                assert got[k] > 0 or setting not in settings, (variant, setting, k)
            assert got == product
        elif variant == "nolean":
            assert got["lean"] == 0 and got["notlean"] == product["lean"] + product["notlean"], (setting, got)
        elif variant == "slowstore":
            assert got["st_aligned"] == 0 and got["st_merged_fwd"] == got["st_merged_back"] == 0, (setting, got)
            assert got["st_unaligned"] == product["st_aligned"] + product["st_unaligned"] + sum(product[k] for k in MERGED), (setting, got)
        else:
            assert variant == "nomerge"
            assert all(got[k] == 0 for k in MERGED + ("decl_partial", "decl_notin")), (setting, got)
            assert got["st_aligned"] == product["st_aligned"] + sum(product[k] for k in MERGED), (setting, got)
            assert all(got[k] == product[k] for k in ("st_unaligned", "st_cropped", "drop_y", "drop_x")), (setting, got)


@pytest.mark.parametrize("variant", list(B.K7T_PATH_VARIANTS))
def test_k7_tiles_paths(variant, corpus_npz, tmp_path_factory):
    check(variant, _child(variant, corpus_npz, tmp_path_factory))
