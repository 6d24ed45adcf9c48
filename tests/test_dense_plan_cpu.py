"""The scratch plan of the dense modes (csrc/dense_plan.h), without a GPU: tests/asan/dense_plan_host.cpp, built with AddressSanitizer
and UBSan by the recipe in its header and run as a child process, plans every admissible call of its grid of handles and checks that
every view lies inside its buffer's capacity, that views written side by side are disjoint, that a plan is refused exactly where the
drivers' own checks refused, and a hand-made table of capacities and offsets; the same build runs the host closed form of the
pose-consistency term (csrc/se3_math.h) on a hand-made input."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_dense_plan_invariants_under_sanitizers(tmp_path):
    exe = str(tmp_path / "dense_plan_host")
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "tightly_coupled_sfm_amd", "csrc"), os.path.join(ROOT, "tests", "asan", "dense_plan_host.cpp"),
                    "-o", exe], check=True, cwd=ROOT)
    r = subprocess.run([exe], capture_output=True, text=True)      # (the sanitizers are linked into the program itself)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("dense_plan_host ok"), r.stdout
