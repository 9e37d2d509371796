"""CPU: the collocation rule's host code (jieba-go_amd/csrc/jb_colloc.cpp) and the code jb_colloc.h shares between
host and kernels under AddressSanitizer + UndefinedBehaviorSanitizer: tests/host/colloc_fuzz.cpp, a program of its
own built with the flags tests/test_neardup_sanitize.py uses.  Seeded ids, doc_tok, spans and uni of arbitrary bit
patterns, outputs in heap blocks of exactly the lengths the call is told.  A report fails the run."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


@pytest.mark.skipif(not shutil.which("g++"), reason="no g++")
def test_colloc_code_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "colloc_fuzz")
    src = os.path.join(ROOT, "jieba-go_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *SAN, "-I", os.path.join(ROOT, "include"), "-I", src, "-o",
                    exe, os.path.join(ROOT, "tests", "host", "colloc_fuzz.cpp"), os.path.join(src, "jb_colloc.cpp"),
                    os.path.join(src, "jb_err.cpp")], check=True)
    r = subprocess.run([exe, "400", "41"], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-4000:]
