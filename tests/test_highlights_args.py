"""CPU: the host side of the highlight stage (csrc/mcraw_highlights_args.h: the struct's checks, inv, m, cap, the green positions,
the records against the extents) is plain C++ and needs neither a GPU nor HIP.  tests/cpp/highlights_args_check.cpp includes that
header alone."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "motioncam_decoder_amd", "csrc")


def test_highlights_args_without_hip(tmp_path):
    """inv over the whole range of the gain, inv, m and cap at gains 256 and 65535 with sat = 65535, the overflow bounds that the
    contract claims, and every check with its neighbours that pass.  Host code only, under ASan and UBSan."""
    exe = str(tmp_path / "highlights_args_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "cpp", "highlights_args_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-3000:], r.stderr[-3000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "wrong 0", r.stdout[-3000:]
    assert int(re.match(r"checks (\d+)", lines[-2]).group(1)) >= 200, lines[-2]
