"""The rules of tests/_paths_harness.run_child, on throw-away children: no GPU, no library, no build (flags None).  Each child is
a few lines of Python that leave a mark in a file and end the way the case needs.  The one wait is the 1-second time limit."""
import contextlib

import pytest

import _paths_harness as PH

PROLOGUE = "import os, signal, sys, time\nopen(sys.argv[1], 'a').write('started\\n')\n"
RESULT = "print('RESULT {\"errors\": [], \"answer\": 42}')\n"


@contextlib.contextmanager
def fresh():
    """The harness with an empty stop list and memo; what the process had is put back afterwards."""
    stop, memo = list(PH.STOP), dict(PH.MEMO)
    PH.STOP.clear()
    PH.MEMO.clear()
    try:
        yield PH
    finally:
        PH.STOP[:] = stop
        PH.MEMO.clear()
        PH.MEMO.update(memo)


@pytest.fixture
def harness():
    with fresh() as h:
        yield h


def run(tmp_path, module, key, body, timeout=30):
    """run_child for a child with `body`; -> (its result, its marker file)"""
    script, mark = tmp_path / ("%s_%s.py" % (module, key)), tmp_path / ("%s_%s.mark" % (module, key))
    script.write_text(PROLOGUE + body)
    return PH.run_child(module, key, str(script), [mark], None, None, timeout), mark


def test_result_is_memoised(harness, tmp_path):
    res, mark = run(tmp_path, "mod_a", "census", RESULT)
    assert res == {"errors": [], "answer": 42}
    again, _ = run(tmp_path, "mod_a", "census", RESULT)
    assert again is res and mark.read_text() == "started\n"  # (started once)
    assert harness.outcome("mod_a", "census") is res and harness.outcome("mod_a", "other") is None and not harness.STOP


def test_ordinary_failure_stops_nothing(harness, tmp_path):
    body = "print('RESULT {\"errors\": [\"pixel 3 differs\"]}')\nsys.exit(1)\n"
    with pytest.raises(AssertionError, match="pixel 3 differs"):
        run(tmp_path, "mod_a", "slow", body)
    assert not harness.STOP
    with pytest.raises(AssertionError, match="pixel 3 differs"):  # the memoised failure, raised again
        run(tmp_path, "mod_a", "slow", body)
    assert (tmp_path / "mod_a_slow.mark").read_text() == "started\n"
    res, mark = run(tmp_path, "mod_b", "census", RESULT)  # the next child runs
    assert res["answer"] == 42 and mark.exists()


@pytest.mark.parametrize("case,body,timeout,reason", [
    ("noresult", "print('nothing to say')\n", 30, "noresult ended with status 0 and no result"),
    ("status139", RESULT + "sys.exit(139)\n", 30, "status139 ended with status 139"),
    ("sigterm", RESULT + "sys.stdout.flush()\nos.kill(os.getpid(), signal.SIGTERM)\n", 30, "sigterm ended with status -15"),
    ("sleeper", "time.sleep(30)\n", 1, "sleeper ran into its time limit"),
])
def test_out_of_order_ending_stops_every_module(harness, tmp_path, case, body, timeout, reason):
    with pytest.raises(pytest.fail.Exception, match=reason):
        run(tmp_path, "mod_a", case, body, timeout)
    assert harness.STOP == [reason]
    with pytest.raises(pytest.fail.Exception, match="no GPU work after a child that did not end in order: " + reason):
        run(tmp_path, "mod_b", "census", RESULT)  # another module: fails at once, with the first reason
    assert not (tmp_path / "mod_b_census.mark").exists() and harness.STOP == [reason]  # (and its child never started)
    with pytest.raises(pytest.fail.Exception, match=reason):  # the memoised failure, raised again
        run(tmp_path, "mod_a", case, body, timeout)
    assert (tmp_path / ("mod_a_%s.mark" % case)).read_text() == "started\n"


def test_what_the_process_had_is_put_back():
    with fresh():  # (whatever the modules that ran before left stays out of this test, too)
        PH.STOP.append("kept")
        PH.MEMO["m", "k"] = {"kept": 1}
        with fresh():
            assert PH.STOP == [] and PH.MEMO == {}
            PH.STOP.append("from a test")
            PH.MEMO["x", "y"] = 1
        assert PH.STOP == ["kept"] and PH.MEMO == {("m", "k"): {"kept": 1}}
