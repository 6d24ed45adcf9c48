"""Build libtcsfm_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "tcsfm_api.hip")
DEPS = [SRC] + sorted(os.path.join(HERE, "csrc", f) for f in os.listdir(os.path.join(HERE, "csrc")) if f.endswith(".h")) + \
       [os.path.join(os.path.dirname(HERE), "include", "tcsfm.h")]          # every header of csrc/ (a fixed list once missed joint_kernel.h)
OUT = os.path.join(HERE, "libtcsfm_hip.so")
# -ffp-contract=on: a*b+c is fused only where the source writes it in one expression (hipcc's default, "fast", lets the backend fuse
# across statements depending on how many uses a product has -- which made the decision-recording instantiations of the kernels
# (TRACE=true: same arithmetic, a few extra stores) round differently from the production ones by an ulp here and there).  With
# "on" every instantiation of a template performs bit-identical arithmetic, so the parity tests that run the recording build
# vouch for the production build.  tests/parity_util.py traced_and_production asserts the two agree bit for bit wherever the oracle
# replays a trace: in replay_pairs / replay_window / replay_dense_pairs (pose, dense and joint dense modes) and at every replay of
# tests/test_gpu_dense_reference.py and tests/test_gpu_dense_shapes.py (the reference-loss modes); test_gpu_four_sources.py for S = 4.
FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=on", "-fPIC", "-shared"]


def needs_build() -> bool:
    return not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in DEPS)


def build(force: bool = False, verbose: bool = False) -> str:
    if not force and not needs_build():
        return OUT
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + FLAGS + [SRC, "-o", OUT]
    if verbose:
        cmd.insert(1, "-Rpass-analysis=kernel-resource-usage")
    subprocess.check_call(cmd)
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose="--verbose" in sys.argv))
