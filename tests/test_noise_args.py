"""CPU: the host side of the noise measurement (csrc/mcraw_noise_args.h: the struct's checks, the bin formulas, the record's
indices, the launch plan and the lane mapping that the kernel itself uses) is plain C++ and needs neither a GPU nor HIP.
tests/cpp/noise_args_check.cpp includes that header alone."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "motioncam_decoder_amd", "csrc")


def test_noise_args_without_hip(tmp_path):
    """Both sides of every bin edge, every index, every check with its neighbours that pass, and the walk of strips, workgroups,
    rounds, halves and lanes for widths 16 .. 4112 and heights 16 .. 80: every block once, nothing outside the window.  Host code
    only, under ASan and UBSan, as its own executable."""
    exe = str(tmp_path / "noise_args_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "cpp", "noise_args_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-3000:], r.stderr[-3000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "wrong 0", r.stdout[-3000:]
    assert int(re.match(r"checks (\d+)", lines[-2]).group(1)) >= 70000, lines[-2]
