"""CPU: the rule of the context's run-time races (csrc/mcraw_race.h: which XCD mapping k7_tiles runs with, how many parts resolve a
long side stream) is a function of (candidate, milliseconds) samples and needs neither a GPU nor HIP.  tests/cpp/race_check.cpp
includes that header alone and checks the rule case by case and against transcriptions of the two functions it replaced."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "motioncam_decoder_amd", "csrc")


def test_race_rule_without_hip(tmp_path):
    """Hand-out order and the cap of three issues, the decision at the last second sample (smallest minimum, ties to the lower
    index), -1 while results are under way, the lost-sample fallback, one timed launch in 64 in the order (decided + q) % nc, the
    moving average and the margins 0.99 / 0.97, reset; 320 seeded scripts of 2 000 launches against tune_pick (pick for pick),
    320 each for 3 and 8 candidates against side_pick up to the decision.  Host code only, under ASan and UBSan."""
    exe = str(tmp_path / "race_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "cpp", "race_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-3000:], r.stderr[-3000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "wrong 0", r.stdout[-3000:]
    assert int(re.match(r"scripts (\d+)", lines[-2]).group(1)) >= 300, lines[-2]


def test_measurement_state_has_one_owner():
    """The state of the four measurements is declared once (mcraw_host.h) and touched by mcraw_tune.hip alone."""
    names = re.compile(r"\bentries\[|send_home|trial_rate|big_seen|sent_trials|TicketTrial|\.tt\.|TRIAL_TICKETS|\.race\b")
    for root in (CSRC, os.path.join(ROOT, "include")):
        for f in sorted(os.listdir(root)):
            if f in ("mcraw_tune.hip", "mcraw_host.h"):
                continue
            hits = [ln for ln in open(os.path.join(root, f), errors="replace") if names.search(ln)]
            assert not hits, (f, hits[:3])
    assert open(os.path.join(CSRC, "mcraw_tune.hip")).read().count("TRIAL_TICKETS = ") == 1
    assert "TRIAL_TICKETS" not in open(os.path.join(CSRC, "mcraw_host.h")).read()
