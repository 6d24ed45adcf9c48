#!/usr/bin/env python3
"""Write tests/golden/golden_resize.npz: the inputs of tests/resize_inputs.py and PILLOW's bytes for them.

    python tests/golden/make_golden_resize.py            (needs Pillow; the tests do not)

The reference resizes every camera frame with PIL's Image.resize((W, H), resample=Image.ANTIALIAS) (data/scannet_test_loader.py:157-170,
data/create_kitti_odometry_data.py:56-65); Image.LANCZOS is the filter ANTIALIAS named.  Per case and per sequence of resize_inputs the
file holds `in_<name>` uint8 [N,h,w,3] and `out_<name>` uint8 [N,H,W,3] = what Pillow returns, frame by frame.  Data only."""
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import resize_inputs as R  # noqa: E402


def pillow(frames, H, W):
    return np.stack([np.asarray(Image.fromarray(f, "RGB").resize((W, H), resample=Image.LANCZOS)) for f in frames])


def main():
    out = {}
    for name, _, (H, W), _ in R.CASES:
        out["in_" + name] = R.make_input(name)
        out["out_" + name] = pillow(out["in_" + name], H, W)
    for name, _, (H, W), _ in R.SEQUENCES:
        out["in_" + name] = R.make_sequence_input(name)
        out["out_" + name] = pillow(out["in_" + name], H, W)
    np.savez_compressed(R.GOLDEN, **out)
    print(R.GOLDEN, os.path.getsize(R.GOLDEN), "bytes; Pillow", Image.__version__)


if __name__ == "__main__":
    main()
