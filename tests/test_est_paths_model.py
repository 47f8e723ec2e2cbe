"""CPU: the model of the estimators' path census (tests/_est_paths_model.py) against the numpy statements and its own identities,
before any GPU sees the corpus: the replay of the search ends where _align_ref / _align_cells_ref end; the counters of every
setting add up the way the kernels' structure says; every counter is driven by the corpus where DRIVEN says, and the only counters
that nothing drives are those that no input can (NEVER)."""
import numpy as np
import pytest

import _est_paths_model as T
from motioncam_decoder_amd import build as B

NAMES = list(T.SETTINGS)


def test_variants_and_names():
    assert tuple(B.EST_PATH_VARIANTS) == T.VARIANTS
    assert all(f in B.TEST_VARIANTS for f in B.EST_PATH_VARIANTS.values())
    assert len(set(T.PATHS)) == len(T.PATHS)
    claimed = set(T.DRIVEN) | set(T.DRIVEN_ANY) | set(T.NEVER)
    assert claimed == set(T.PATHS), (sorted(set(T.PATHS) - claimed), sorted(claimed - set(T.PATHS)))
    assert not (set(T.DRIVEN) | set(T.DRIVEN_ANY)) & set(T.NEVER)
    for views in ([S["view"] for S in T.SETTINGS.values() if S["family"] == f] for f in ("align", "cells", "noise")):
        assert set(views) == set(T.VIEWS)


@pytest.mark.parametrize("name", NAMES)
def test_replay_is_the_statement(name):
    for got, want in zip(T.answers(name), T.statement(name)):
        assert np.array_equal(np.asarray(got), np.asarray(want)), name


def _sad_identities(name, c, S, variant):
    n = S["n"]
    pairs = n - 1
    for fam in ("as", "cs"):
        for rt in (0, 1):
            g = lambda k: c["%s%d_%s" % (fam, rt, k)]  # noqa: E731
            live = g("wg") - g("nopair") - g("empty")  # workgroups with pixels
            assert g("om0") + g("om1") + g("ob1om0") + g("ob1om1") == live, (name, fam, rt)
            assert g("wave_add") + g("wave_skip") == 4 * live * (9 if rt else (2 * S.get("radius", 0) + 1) ** 2), (name, fam, rt)
            if rt:
                assert g("ref_full") + g("ref_mask") == 4 * live, (name, fam, rt)
            if variant in ("slow", "poisonslow"):
                assert g("ref_full") == 0 and g("store") == 0
            ncand = 9 if rt else (2 * S.get("radius", 0) + 1) ** 2
            assert g("store") + g("glob_add") + g("glob_skip") == ncand * (g("wg") - g("nopair")), (name, fam, rt)
            assert g("nopair") * pairs == (g("wg") - g("nopair")) * (n - pairs), (name, fam, rt)
            staged = g("stg_load") + g("stg_zero_y") + g("stg_zero_col") + g("stg_left") + g("stg_right")
            if fam == "as":  # rows * ndw of both tiles, per workgroup
                R = 1 if rt else S["radius"]
                assert staged == live * (32 * 65 + (32 + 2 * R) * (64 + R + 1)), (name, rt)
                assert g("stg_pad") <= g("stg_load")
            else:
                assert staged <= live * (32 * 64 + 40 * 69)


@pytest.mark.parametrize("variant", ("census", "frames2", "slow", "strips1"))
@pytest.mark.parametrize("name", NAMES)
def test_identities(name, variant):
    S, c = T.SETTINGS[name], T.model(name, variant)
    assert list(c) == T.PATHS and all(isinstance(v, int) and v >= 0 for v in c.values())
    assert all(c[k] == 0 for k in T.NEVER), name
    n = S["n"]
    if S["family"] == "noise":
        by, bx = S["roi"][2] // 16, S["roi"][3] // 16
        assert c["ns_accept"] + c["ns_rej_sat"] + c["ns_rej_lo"] == S["calls"] * n * by * bx * 4
        assert c["ns_block"] == S["calls"] * n * by * bx * 2
        assert c["ns_ld_vec"] + c["ns_ld_unal"] == 16 * c["ns_block"]
        assert (c["ns_skip_t1"] + c["ns_skip_inactive"] + c["ns_block"]) % 128 == 0
        assert c["ns_hist_flush"] <= c["ns_accept"] and c["ns_reg_flush"] <= 16 * c["ns_wg"]
        launches = T._launches(n, variant)
        assert c["ns_wg"] == S["calls"] * sum(nf * T.noise_plan(S["roi"][3], S["roi"][2], nf, 1 if variant == "strips1" else T.NS_MAXSTRIPS)["wgs"]
                                             for nf in launches)
        assert all(c[k] == 0 for k in T.PATHS if not k.startswith("ns_"))
        return
    assert all(c[k] == 0 for k in T.PATHS if k.startswith("ns_"))
    # the pyramid: every lane returns or works; G0 rows by form sum to the lanes' rows; loads + zero-filled rows are 8 per lane
    lanes = 256 * c["py_wg"] - c["py_ret"]
    assert c["py_g0_vec"] + c["py_g0_elem"] + c["py_g0_left"] == 4 * lanes
    assert c["py_ld_vec"] + c["py_ld_unal"] + c["py_ld_elem"] + c["py_zero_row"] == 8 * lanes
    if S["levels"] >= 2:
        assert c["py_g1_dword"] + c["py_g1_elem"] + c["py_g1_none"] + c["py_g1_left"] == 2 * lanes and c["py_ret_l2"] == 0
    else:
        assert c["py_ret_l2"] == lanes
    assert c["py_g2_store"] + c["py_g2_none"] == (lanes if S["levels"] >= 3 else 0)
    assert c["py_ret_l3"] == (lanes if S["levels"] == 2 else 0)
    _sad_identities(name, c, S, variant)
    if variant == "frames2":
        plain = T.model(name, "census")
        k = -(-n // 2)
        for key in T.PATHS:
            if key.endswith("_launch") and key[:2] in ("as", "cs", "dn"):
                assert c[key] == k * plain[key], (name, key)
            else:
                assert c[key] == plain[key], (name, key)


def test_every_counter_is_driven():
    """DRIVEN: above zero in every setting named; DRIVEN_ANY: in one of those named."""
    for k, names in T.DRIVEN.items():
        assert names, k
        for name in names:
            assert T.model(name)[k] > 0, (k, name)
    for k, names in T.DRIVEN_ANY.items():
        assert sum(T.model(name)[k] for name in names) > 0, k
