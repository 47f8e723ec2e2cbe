"""What the path-census tests share (tests/test_gpu_*_paths.py, their children tests/_*_paths_child.py; DESIGN.md "The census
layer").  A plain module: no fixture, no plugin.

Parent side: run_child() links one -D build of the library (build.build_variant) and runs one child process on it, once.  A child
that ends by a signal, at its time limit, with status 124 / 134 / 137 / 139 or without its  RESULT {json}  line (an exception
on the way: a HIP error is one) may have left the GPU faulted: the reason goes into STOP, and from then on every run_child() of
every module of this pytest process fails at once, with that first reason, before it builds or starts anything.  Only "compared
everything, something differs" (status 1 WITH the line) lets the others run.  Nothing is tried twice: what became of a child --
its result or the failure raised -- is kept per (module, key) and handed to every later caller.

Child side: census_reader() for the library's mcraw_diag_*_paths, finish() for the result line.  (pytest is imported where the
parent needs it, so that a child does not pay for it.)"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

STOP = []   # why no further child may be started, one list for the process
MEMO = {}   # (module, key) -> what the child printed, or the failure that was raised


def no_errors(what, also=lambda res: True):
    """The usual verdict on a child that ended in order: status 0, no errors listed (and also(res))."""
    def judge(key, res, returncode):
        assert returncode == 0 and not res["errors"] and also(res), "%s: %s:\n%s" % (key, what, "\n".join(res["errors"]))
    return judge


def outcome(module, key):
    """What run_child(module, key, ..) left, without running anything: the result, the failure, or None."""
    return MEMO.get((module, key))


def run_child(module, key, child, args, flags, libname, timeout, tmp_path_factory=None, judge=no_errors("the child found differences")):
    """The result of  python child *args  with MCRAW_LIB_PATH = the build of the library with `flags` (None: nothing is built, the
    environment stays), for the caller `module` (its __name__) and its variant `key`; judge(key, res, returncode) has the last word
    on a child that ended in order."""
    import pytest
    if (module, key) not in MEMO:
        if STOP:
            pytest.fail("no GPU work after a child that did not end in order: " + STOP[0])
        try:
            MEMO[module, key] = _run(key, child, args, flags, libname, timeout, tmp_path_factory, judge)
        except BaseException as e:  # (pytest.fail's outcome is no Exception)
            MEMO[module, key] = e
    if isinstance(MEMO[module, key], BaseException):
        raise MEMO[module, key]
    return MEMO[module, key]


def _run(key, child, args, flags, libname, timeout, tmp_path_factory, judge):
    import pytest
    env = dict(os.environ)
    if flags is not None:
        from motioncam_decoder_amd import build as B
        env["MCRAW_LIB_PATH"] = B.build_variant(str(tmp_path_factory.mktemp("lib_" + key) / libname), flags)
    try:
        r = subprocess.run([sys.executable, child] + [str(a) for a in args], env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        STOP.append("%s ran into its time limit" % key)
        pytest.fail(STOP[-1])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or not line:
        STOP.append("%s ended with status %d%s" % (key, r.returncode, "" if line else " and no result"))
        pytest.fail(STOP[-1] + "\n" + r.stdout[-2000:] + r.stderr[-3000:])
    res = json.loads(line[-1][7:])
    print(key, "child seconds", res.get("seconds"))
    judge(key, res, r.returncode)
    return res


def census_reader(lib, symbol, paths, as_dict=True):
    """-> census(): the counters of the library's `symbol` (int mcraw_diag_*_paths(uint64_t *out, int n, int reset)) since the last
    call, as a dict over `paths` or as a list, and the census started over."""
    fn = getattr(lib, symbol)
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(C.c_uint64), C.c_int, C.c_int]

    def census():
        a = (C.c_uint64 * len(paths))()
        got = fn(a, len(paths), 1)
        assert got == len(paths), "the census has %d counters, this script knows %d" % (got, len(paths))
        return dict(zip(paths, (int(v) for v in a))) if as_dict else [int(v) for v in a]
    return census


def finish(res, errors, t0):
    """The end of a child's main(): prints the result line, -> the exit status (1 when there are errors)."""
    res["seconds"] = round(time.time() - t0, 2)
    res["errors"] = errors[:20]
    print("RESULT " + json.dumps(res))
    return 1 if errors else 0
