"""CPU: the host layer's planners (jieba-go_amd/csrc/jb_plan.cpp: plan_pieces, plan_units, han_run_start,
jb_split_points) in tests/host/plan_check.cpp, a program of its own built with jb_plan.cpp and jb_err.cpp
alone under AddressSanitizer + UndefinedBehaviorSanitizer.  It checks the piece layout and the unit cuts
property by property; its unit lists for the fixed inputs must also equal tests/golden/plan_units.json,
recorded from the code as it was inside jb_capi.cpp's cut_sharded before the planners were split out."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("plan") / "plan_check")
    src = os.path.join(ROOT, "jieba-go_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *SAN, "-I", os.path.join(ROOT, "include"), "-I", src,
                    "-o", exe, os.path.join(ROOT, "tests", "host", "plan_check.cpp"),
                    os.path.join(src, "jb_plan.cpp"), os.path.join(src, "jb_err.cpp")], check=True)
    return exe


def test_planner_properties_under_asan_ubsan(plan_check):
    r = subprocess.run([plan_check], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-4000:]


def test_plan_units_equal_recorded_lists(plan_check):
    r = subprocess.run([plan_check, "--dump"], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0, r.stderr[-4000:]
    got = json.loads(r.stdout)
    with open(os.path.join(ROOT, "tests", "golden", "plan_units.json")) as f:
        want = json.load(f)
    assert [c["name"] for c in got] == [c["name"] for c in want]
    for g, w in zip(got, want):
        assert g == w, g["name"]
    assert sum(c["split"] for c in want) >= 30  # (the fixture does exercise the split)
