"""The decisions of the drop-in operators (csrc/operator_plan.h), without a GPU: tests/asan/operator_plan_host.cpp, built with
AddressSanitizer and UBSan by the recipe in its header and run as a child process, plays every NULL / wanted combination of the three
backward plans (16, 32 and 16 cases) against truth tables written from what each output needs, and the launch and scratch geometry at
its edges.  Built three more times with one wrong decision planted behind the plan (-DPLANT=1..3), the program must fail each time:
the tables do catch a d_depth_s that is never zeroed, depth cotangents computed without g_weight and a block count rounded down."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, plant):
    exe = str(tmp_path / f"operator_plan_host_{plant}")
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    f"-DPLANT={plant}", "-I", os.path.join(ROOT, "tightly_coupled_sfm_amd", "csrc"),
                    os.path.join(ROOT, "tests", "asan", "operator_plan_host.cpp"), "-o", exe], check=True, cwd=ROOT)
    return subprocess.run([exe], capture_output=True, text=True)      # (the sanitizers are linked into the program itself)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_operator_plan_truth_tables_under_sanitizers(tmp_path):
    r = _build(tmp_path, 0)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("operator_plan_host ok"), r.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("plant, where", [(1, "warp backward case 2"), (2, "a cotangent read that was not given"), (3, "hw 16: 0 blocks")])
def test_planted_wrong_decisions_are_caught(tmp_path, plant, where):
    r = _build(tmp_path, plant)
    assert r.returncode == 1, r.stdout + r.stderr
    assert "FAILED" in r.stdout and where in r.stdout and f"checks failed (PLANT={plant})" in r.stdout, r.stdout
