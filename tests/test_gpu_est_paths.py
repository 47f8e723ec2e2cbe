"""GPU (-m gpu): every path of the estimators counted, the launch loops split, the guarded paths forced and the scratch poisoned,
against the numpy statements and an exact model.

mcraw_align_batch, mcraw_align_cells_batch and mcraw_noise_batch steer everything behind them: `pos` decides which samples the
merge averages, the noise profile how hard the denoiser and the merge weigh.  Their own suites compare outputs bit for bit;
nothing there shows which branch a case entered, and no launch loop of theirs had run a second iteration on any machine.  Here six
builds of the three sources (build.EST_PATH_VARIANTS; why each is valid: the head of csrc/mcraw_est_paths.h) run the corpus of
tests/_est_paths_model.py in a child process each (tests/_est_paths_child.py): 5 frames a call (launches of 2, 2, 1 in `frames2`),
a chain and an anchor in the middle, every shape as three views (on the 16-byte grid, a base 2 bytes off it, a pitch of W + 3),
scenes, full-range noise, flat and identical frames, centres from nothing, by hand and from align(), one chain of 2056 frames
that the clamp cuts.  The child calls align and cells through the raw ABI twice, with a scratch of 0xFF bytes and one of 0x00
bytes, and compares pos, sad and the records with the numpy statements; this module compares the census of every call with the
model, EVERY counter, EXACTLY.

  every one          outputs; census == model(setting, variant), counter by counter, for both scratch fills
  census             every counter is above zero in the settings DRIVEN names for it, in one of those DRIVEN_ANY names; the
                     counters of NEVER are zero (the model's parity argument: kalign_sad<1> only ever sees (ob, om) = (1, 0))
  slow, poisonslow   no wave in al_refine<true>, no sum stored, kcells_zero in every call of cells
  poison*            every counter equals the unpoisoned twin's, call by call
  frames2            launches of the SAD kernels and of kalign_down = ceil(n / 2) times `census`'s; every other counter outside
                     knoise equals `census`'s; knoise's workgroups follow noise_plan per launch
  strips1            knoise with one strip per workgroup: as many workgroups as strips

A child that ends by a signal, at its time limit or without its result stops every further child, of this module and of every other (tests/_paths_harness.py): the remaining tests fail at
once.  Nothing is tried twice.

Measured on an MI355X, one run of the module (7 passed in 34.28 s with the new test of test_gpu_align_cells.py).  Per variant: the
child's own `seconds` (from its first line to its result: 237 calls, their comparisons and census reads) / the whole test (the
link of the variant, whose objects came with the build; start of the child with its imports, child, the 126 models -- `census`
makes the replays that the later variants reuse; the numpy statements' answers for the children are made once, in 0.7 s, in front
of `census`):
  census 0.82 / 11.54   frames2 1.11 / 4.78   slow 0.64 / 4.32   poison 0.64 / 3.61   poisonslow 0.62 / 3.51   strips1 0.67 / 3.59
CHILD_TIMEOUT is ten times the slowest whole test; it guards against a hang, not against performance."""
import json
import os

import numpy as np
import pytest

import _paths_harness as PH
from motioncam_decoder_amd import build as B

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "_est_paths_child.py")
CHILD_TIMEOUT = 115  # seconds: ten times the slowest measured whole test (see above)



def make_npz(path):
    """What the numpy statements give for every setting: pos_<i> and sad_<i>, or rec_<i>."""
    import _est_paths_model as T
    arrays = {}
    for i, name in enumerate(T.SETTINGS):
        want = T.statement(name)
        if len(want) == 2:
            arrays["pos_%d" % i], arrays["sad_%d" % i] = np.asarray(want[0], np.int16), np.asarray(want[1], np.uint64)
        else:
            arrays["rec_%d" % i] = np.asarray(want[0], np.uint8)
    np.savez(path, **arrays)


@pytest.fixture(scope="module")
def corpus_npz(tmp_path_factory):
    """Computed once for the module."""
    path = str(tmp_path_factory.mktemp("est_paths") / "corpus.npz")
    make_npz(path)
    return path


def _child(variant, corpus_npz, tmp_path_factory):
    """The result of `variant`'s child, which is run once whatever becomes of it (tests/_paths_harness.py)."""
    return PH.run_child(__name__, variant, CHILD, [corpus_npz, variant], B.EST_PATH_VARIANTS[variant], "libmcraw_estp_%s.so" % variant,
                       CHILD_TIMEOUT, tmp_path_factory, PH.no_errors("outputs differ from the numpy statements"))


def _seen(variant):
    """What `variant`'s child left, if it has run: its result or the failure."""
    return PH.outcome(__name__, variant)


def check(variant, res):
    """The census `res` of `variant`'s child against the model."""
    import _est_paths_model as T
    assert res["paths"] == T.PATHS, "the child's counters are not the model's"
    assert list(res["census"]) == list(T.SETTINGS)
    total = dict.fromkeys(T.PATHS, 0)
    twin = _seen({"poison": "census", "poisonslow": "slow"}.get(variant))
    plain = _seen("census") if variant == "frames2" else None
    bad = []
    for name, rows in res["census"].items():
        S, want = T.SETTINGS[name], T.model(name, variant)
        assert len(rows) == (1 if S["family"] == "noise" else 2), name
        for fill, row in enumerate(rows):
            got = dict(zip(T.PATHS, row))
            if fill == 0:
                print(variant, name, json.dumps({k: v for k, v in got.items() if v}))
                for k in T.PATHS:
                    total[k] += got[k]
            bad += [(name, fill, k, got[k], want[k]) for k in T.PATHS if got[k] != want[k]]
            if isinstance(twin, dict):
                assert row == twin["census"][name][fill], (variant, name, fill, "differs from the unpoisoned build")
        got = dict(zip(T.PATHS, rows[0]))
        if variant == "census":
            for k, names in T.DRIVEN.items():
                assert got[k] > 0 or name not in names, (name, k)
            assert all(got[k] == 0 for k in T.NEVER), name
        if variant in ("slow", "poisonslow"):
            assert got["as1_ref_full"] == got["cs1_ref_full"] == got["cs0_store"] == got["cs1_store"] == 0, name
            assert got["cz_launch"] == (1 if S["family"] == "cells" else 0), name
        if isinstance(plain, dict):  # frames2 against the census build's own counts
            was, k2 = dict(zip(T.PATHS, plain["census"][name][0])), -(-S["n"] // 2)
            for k in T.PATHS:
                if k.startswith("ns_"):
                    continue
                assert got[k] == (k2 * was[k] if k.endswith("_launch") and k[:2] in ("as", "cs", "dn") else was[k]), (name, k)
        if variant in ("frames2", "strips1") and S["family"] == "noise":
            y0, x0, h, w = S["roi"]
            wgs = sum(nf * T.noise_plan(w, h, nf, 1 if variant == "strips1" else T.NS_MAXSTRIPS)["wgs"] for nf in T._launches(S["n"], variant))
            assert got["ns_wg"] == S["calls"] * wgs, name
            if variant == "strips1":
                assert got["ns_wg"] == S["calls"] * S["n"] * (h // 16) * -(-(w // 16) // T.NS_SB), name
    print(variant, "totals", json.dumps(total))
    assert not bad, "%d counters differ from the model (setting, scratch fill, counter, got, want): %r" % (len(bad), bad[:40] + sorted({(n[:12], k) for n, _, k, _, _ in bad}))
    if variant == "census":
        for k, names in T.DRIVEN_ANY.items():
            assert sum(dict(zip(T.PATHS, res["census"][n][0]))[k] for n in names) > 0, k
        assert all(total[k] > 0 for k in T.PATHS if k not in T.NEVER)
    if variant in ("slow", "poisonslow"):
        assert total["as1_ref_mask"] > 0 and total["cs1_ref_mask"] > 0 and total["cs1_glob_add"] > 0 and total["cs0_glob_add"] > 0


@pytest.mark.parametrize("variant", list(B.EST_PATH_VARIANTS))
def test_est_paths(variant, corpus_npz, tmp_path_factory):
    import _est_paths_model as T
    assert tuple(B.EST_PATH_VARIANTS) == T.VARIANTS
    check(variant, _child(variant, corpus_npz, tmp_path_factory))
