"""CPU: the mask-pinned float64 reference of tests/depthnet_twin.py (forward_pinned, maxpool_argmax, encoder_tape_entries) against
the plain float64 twin and torch's own max pool: pinned to the twin's own ReLU and max-pool decisions it is the twin, gradients
included, so the GPU tests that pin it to the HIP forward's decisions compare with the twin's network."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import depthnet_twin as dt  # noqa: E402


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def test_pinned_forward_reproduces_twin_gradients():
    N, H, W = 2, 64, 96
    sd = {k: v.double() for k, v in dt.depthnet_params(0).items()}
    x = torch.from_numpy(dt.sample_images(5, N, H, W))
    entries = dt.twin_tape_entries(sd, x)
    assert [tuple(e.shape[1:]) for e in entries] == dt.encoder_tape_shapes(H, W)
    g = torch.Generator().manual_seed(3)
    R = torch.randn((N, 1, H, W), generator=g, dtype=torch.float64)
    Rs = [torch.randn((N, c, H >> (k + 1), W >> (k + 1)), generator=g, dtype=torch.float64)
          for k, c in enumerate((64, 64, 128, 256, 512))]

    def grads(fwd):
        p = {k: v.clone().requires_grad_(not k.endswith(("running_mean", "running_var"))) for k, v in sd.items()}
        disp, skips = fwd(p)
        ((disp * R).sum() + sum((s * r).sum() for s, r in zip(skips, Rs))).backward()
        return disp.detach(), [s.detach() for s in skips], {k: v.grad for k, v in p.items() if v.grad is not None}

    d0, s0, g0 = grads(lambda p: dt.forward(p, x.double(), return_skips=True))
    d1, s1, g1 = grads(lambda p: dt.forward_pinned(p, x, entries))
    assert torch.equal(d0, d1)
    for a, b in zip(s0, s1):
        assert torch.equal(a, b)
    assert sorted(g0) == sorted(g1) and len(g0) == 84 and sum(k.startswith(dt.ENC) for k in g0) == 60
    bad = {k: e for k in g0 if (e := _rel(g1[k], g0[k])) > 1e-12}
    assert not bad, bad
    # the pinning is live: other masks give other gradients
    flipped = list(entries)
    flipped[9] = torch.where(entries[9] > 0, torch.zeros_like(entries[9]), torch.ones_like(entries[9]))
    _, _, g2 = grads(lambda p: dt.forward_pinned(p, x, flipped))
    assert _rel(g2[f"{dt.ENC}layer3.0.conv1.weight"], g0[f"{dt.ENC}layer3.0.conv1.weight"]) > 0.1


@pytest.mark.parametrize("h,w", [(8, 8), (9, 12), (16, 10)])
def test_maxpool_argmax_matches_torch_with_ties(h, w):
    rs = np.random.RandomState(h * 100 + w)
    a = rs.randint(0, 3, size=(2, 5, h, w)).astype(np.float64)     # values in {0, 1, 2}: ties in almost every window
    a[0, 0] = 0.0                                                   # a channel of all-zero windows
    a[0, 1, :3, :] = 2.0                                            # ties along the top border (a padded row above)
    a[0, 2, :, -3:] = 2.0                                           # and the right border (odd w: a padded column)
    a[1, 3] = -1.0                                                  # all-negative, all equal
    a[1, 4, ::2, ::2] = 5.0                                         # window corners tie with each other
    t = torch.from_numpy(a)
    vals, ref = torch.nn.functional.max_pool2d(t, 3, 2, 1, return_indices=True)
    idx = dt.maxpool_argmax(t)
    assert torch.equal(idx, ref)
    assert torch.equal(t.flatten(2).gather(2, idx.flatten(2)).view(idx.shape), vals)


def test_encoder_tape_entries_reads_entry_major_layout():
    N, H, W = 3, 32, 64
    shp = dt.encoder_tape_shapes(H, W)
    assert len(shp) == 19 and shp[1] == (16, 32, 64) and shp[2] == (8, 16, 64) and shp[-1] == (1, 2, 512)
    # per image: 6.5 M floats at 640 x 192
    assert sum(int(np.prod(s)) for s in dt.encoder_tape_shapes(192, 640)) == 6512640
    parts = [torch.arange(N * int(np.prod(s)), dtype=torch.float32) + 1000.0 * e for e, s in enumerate(shp)]
    tape = torch.cat(parts)
    ent = dt.encoder_tape_entries(tape, N, H, W)
    for e, (t, p, s) in enumerate(zip(ent, parts, shp)):
        assert tuple(t.shape) == (N, *s)
        assert torch.equal(t.reshape(-1), p), e
    with pytest.raises(ValueError, match="encoder tape"):
        dt.encoder_tape_entries(tape[:-1], N, H, W)
