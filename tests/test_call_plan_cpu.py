"""The plan of a pose call and the routing rules of the refine calls (csrc/call_plan.h), without a GPU: tests/asan/call_plan_host.cpp,
built with AddressSanitizer and UBSan by the recipe in its header and run as a child process, plays the queue of the *_queued entries,
the lane rotation of merged sequences and the graph cache over every script of its small alphabets against the invariants at the top
of the header (every admitted call launched once, in order; what one flush may hold; what is captured, replayed, evicted, and that every
executable handed in comes back once), and checks the pose call's schedule and extents against the rules and a hand-made table."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_call_plan_invariants_under_sanitizers(tmp_path):
    exe = str(tmp_path / "call_plan_host")
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "tightly_coupled_sfm_amd", "csrc"), os.path.join(ROOT, "tests", "asan", "call_plan_host.cpp"),
                    "-o", exe], check=True, cwd=ROOT)
    r = subprocess.run([exe], capture_output=True, text=True)      # (the sanitizers are linked into the program itself)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("call_plan_host ok"), r.stdout
