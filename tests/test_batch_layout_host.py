"""CPU: the layout of the host-text calls' first device buffer (jieba-go_amd/csrc/jb_batch.h: batch_layout,
batch_chain_extra, Arena) in tests/host/batch_layout_check.cpp, a program of its own built from the header's
HIP-free part alone under AddressSanitizer + UndefinedBehaviorSanitizer.  Every host-text entry point sizes and
cuts that buffer through this one function; the program checks alignment, disjointness and bounds over a grid, and
that the total equals the sums the entry points wrote out for themselves before they shared a front."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


@pytest.fixture(scope="module")
def batch_layout_check(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("batch_layout") / "batch_layout_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *SAN, "-I", os.path.join(ROOT, "jieba-go_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "host", "batch_layout_check.cpp")], check=True)
    return exe


def test_batch_layout_under_asan_ubsan(batch_layout_check):
    r = subprocess.run([batch_layout_check], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-4000:]
