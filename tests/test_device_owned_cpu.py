"""The owners of every device allocation, stream and event of the library (csrc/device_owned.h), without a GPU:
tests/asan/device_owned_host.cpp, built with AddressSanitizer and UBSan by the recipe in its header and run as a child process, puts
counting stand-ins under the HIP calls the header makes and checks that a vector of buffers that grows from 1 to 9 while they are live
frees each allocation exactly once, that a failed reserve leaves the buffer empty and the next one allocates, that a sufficient reserve
keeps the pointer, that a moved-from buffer frees nothing, that a struct which only points at another's weights frees none of them in
either destruction order, and that the stream, event and pinned-memory owners destroy once."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_device_owners_release_once_under_sanitizers(tmp_path):
    exe = str(tmp_path / "device_owned_host")
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "tightly_coupled_sfm_amd", "csrc"), os.path.join(ROOT, "tests", "asan", "device_owned_host.cpp"),
                    "-o", exe], check=True, cwd=ROOT)
    r = subprocess.run([exe], capture_output=True, text=True)      # (the sanitizers are linked into the program itself)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("device_owned_host ok"), r.stdout
