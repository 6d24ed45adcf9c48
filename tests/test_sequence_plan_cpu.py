"""The ring plan and the schedule of the sequence calls (csrc/sequence_plan.h), without a GPU: tests/asan/sequence_plan_host.cpp, built
with AddressSanitizer and UBSan by the recipe in its header and run as a child process, plays every accepted plan of its grid against a
model of the slots and checks the invariants that keep the pipeline free of races; it also pins the plans of the tested parameters."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_sequence_plan_invariants_under_sanitizers(tmp_path):
    exe = str(tmp_path / "sequence_plan_host")
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "tightly_coupled_sfm_amd", "csrc"), os.path.join(ROOT, "tests", "asan", "sequence_plan_host.cpp"),
                    "-o", exe], check=True, cwd=ROOT)
    r = subprocess.run([exe], capture_output=True, text=True)      # (the sanitizers are linked into the program itself)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("sequence_plan_host ok"), r.stdout
