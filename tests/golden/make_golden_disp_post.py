"""Generate tests/golden/golden_disp_post.npz: the reference's own utils.learning_helpers.batch_post_process_disparity on float32 planes.

Run on the build box (needs /root/reference, imported as make_golden.py imports it):  python tests/golden/make_golden_disp_post.py
Inputs: rng.uniform(1 / 2.67, 1 / 0.06) cast to float32 -- the range of disp_to_depth's scaled_disp at the reference's min / max depth
-- at (2, 8, 64), (1, 4, 96) and (1, 3, 33): an even width, a second one, and an odd one.  `r` is the second argument as the reference
passes it, i.e. the mirrored pass's result already un-flipped.  Stored: l, r (float32) and the float64 result.  Data only."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

SHAPES = [(2, 8, 64), (1, 4, 96), (1, 3, 33)]


def main():
    import make_golden
    lh = make_golden.import_reference()["learning_helpers"]
    rng = np.random.default_rng(19)
    out = {}
    for k, shape in enumerate(SHAPES):
        l = rng.uniform(1 / 2.67, 1 / 0.06, size=shape).astype(np.float32)
        r = rng.uniform(1 / 2.67, 1 / 0.06, size=shape).astype(np.float32)
        post = lh.batch_post_process_disparity(l, r)
        assert post.dtype == np.float64 and post.shape == shape
        out[f"l{k}"], out[f"r{k}"], out[f"post{k}"] = l, r, post
    path = os.path.join(HERE, "golden_disp_post.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
