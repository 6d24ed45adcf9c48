"""GPU: the depth network's backward pass (csrc/depthnet_grad_kernel.h, tcsfm_depthnet_*_train / *_backward) behind
depthnet_train.DepthNetModule, against the float64 twin of tests/depthnet_twin.py under torch autograd, its determinism and
memory contracts, its refusals, and the mechanics of the reference's weight-tuning loop (deep copy, optimiser on encoder weights)."""
import copy
import os
import sys

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import depthnet_twin as dt  # noqa: E402


def _module(seed=0, max_images=6):
    from tightly_coupled_sfm_amd.depthnet_train import DepthNetModule
    return DepthNetModule(dt.depthnet_params(seed), max_images=max_images).cuda()


def _imgs(seed, N, H, W):
    return torch.from_numpy(dt.sample_images(seed, N, H, W)).cuda()


def _cot(seed, shape):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64)


def _twin_grads(x, R, Rs=None, seed=0):
    """float64 twin: gradients of (disp R).sum() (+ sum_k (skip_k Rs_k).sum()) with respect to every parameter"""
    sd = {k: v.double().cuda() for k, v in dt.depthnet_params(seed).items()}
    for k, v in sd.items():
        if not (k.endswith("running_mean") or k.endswith("running_var")):
            v.requires_grad_(True)
    disp, skips = dt.forward(sd, x.double(), return_skips=True)
    loss = (disp * R.cuda()).sum()
    if Rs is not None:
        loss = loss + sum((s * r.cuda()).sum() for s, r in zip(skips, Rs))
    loss.backward()
    return {k: v.grad for k, v in sd.items() if v.grad is not None}


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


@pytest.mark.parametrize("N,H,W", [(3, 64, 192), (5, 96, 320), (2, 192, 640)])
@pytest.mark.parametrize("with_skips", [False, True])
def test_gradient_parity_with_float64_twin(N, H, W, with_skips):
    """Decoder and head parameters (smooth ELU / sigmoid path) within 1e-4 relative L2 of the float64 twin.  Encoder parameters within
    1e-2: a ReLU whose pre-activation lies within fp32 rounding of zero can switch between fp32 and fp64, and with a zero-mean
    cotangent one such pixel moves a cancelling pixel sum by ~1e-3 (measured: 1 of 294 912 skip-2 pixels at 128 x 384 -> 2.0e-3 on
    layer2.1.bn2.bias; the fp32 MIOpen twin's own error reaches 4.7e-3 at 640 x 192).  The exactness of the backward itself is
    test_encoder_gradient_exact_on_own_relu_masks."""
    mod = _module(0, max_images=4)              # (5, ...) runs in two groups
    x = _imgs(11 + N, N, H, W)
    R = _cot(1, (N, 1, H, W))
    Rs = [_cot(2 + k, (N, c, H >> (k + 1), W >> (k + 1))) for k, c in enumerate((64, 64, 128, 256, 512))] if with_skips else None
    disps, skips = mod(x)
    loss = (disps[0] * R.float().cuda()).sum()
    if with_skips:
        loss = loss + sum((s * r.float().cuda()).sum() for s, r in zip(skips, Rs))
    loss.backward()
    ref = _twin_grads(x, R, Rs)
    bad = {}
    for k, p in mod.named_parameters():
        assert p.grad is not None, k
        e = _rel(p.grad, ref[k])
        if e > (1e-2 if k.startswith("encoder.") else 1e-4):
            bad[k] = e
    assert not bad, bad


def test_encoder_gradient_exact_on_own_relu_masks():
    """loss on skip 2 only: layer2.1.bn2's beta gradient is the channel sum of r * [skip2 > 0] over the module's own skip 2"""
    N, H, W = 3, 128, 384
    mod = _module(0, max_images=4)
    x = _imgs(14, N, H, W)
    _, sk = mod(x, return_disp=False)
    r = _cot(52, tuple(sk[2].shape)).float().cuda()
    (sk[2] * r).sum().backward()
    g = mod.get_parameter("encoder.encoder.layer2.1.bn2.bias").grad.double()
    own = (r.double() * (sk[2].detach() > 0).double()).sum((0, 2, 3))
    assert _rel(g, own) <= 1e-5


def test_requires_grad_false_and_encoder_bits_independent_of_decoder_requests():
    N, H, W = 2, 64, 192
    x = _imgs(3, N, H, W)
    R = _cot(5, (N, 1, H, W)).float().cuda()
    grads = []
    for dec_on in (True, False):
        mod = _module(1)
        for k, p in mod.named_parameters():
            if not k.startswith("encoder."):
                p.requires_grad_(dec_on)
        mod.get_parameter("encoder.encoder.layer2.0.conv1.weight").requires_grad_(False)
        (mod(x)[0][0] * R).sum().backward()
        assert mod.get_parameter("encoder.encoder.layer2.0.conv1.weight").grad is None
        if not dec_on:
            assert all(p.grad is None for k, p in mod.named_parameters() if not k.startswith("encoder."))
        grads.append({k: p.grad.clone() for k, p in mod.named_parameters() if k.startswith("encoder.") and p.grad is not None})
    assert sorted(grads[0]) == sorted(grads[1])
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k


def test_backward_is_bit_reproducible_and_batch_independent():
    H, W = 96, 320
    mod = _module(2, max_images=5)
    x = _imgs(21, 5, H, W)
    R = _cot(7, (5, 1, H, W)).float().cuda()
    runs = []
    for _ in range(2):
        mod.zero_grad(set_to_none=True)
        (mod(x)[0][0] * R).sum().backward()
        runs.append({k: p.grad.clone() for k, p in mod.named_parameters()})
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
    # one image's skip gradients alone == inside the batch of 5 (bottleneck leaves, decoder frozen)
    for p in mod.parameters():
        p.requires_grad_(False)
    with torch.no_grad():
        _, sk = mod(x, return_disp=False)

    def skip_grads(idx):
        leaves = [s[idx].clone().requires_grad_(True) for s in sk]
        (mod(None, skips=leaves)[0][0] * R[idx]).sum().backward()
        return [leaf.grad for leaf in leaves]
    batch, one = skip_grads(slice(0, 5)), skip_grads(slice(3, 4))
    for a, b in zip(batch, one):
        assert torch.equal(a[3:4], b)


def test_training_forward_bits_and_refold_after_update():
    from tightly_coupled_sfm_amd.depthnet import DepthNetHIP
    from tightly_coupled_sfm_amd.engine import Engine
    H, W, N = 64, 192, 3
    mod = _module(3)
    x = _imgs(31, N, H, W)
    disps, skips = mod(x)
    assert disps[0].requires_grad
    hip = DepthNetHIP(Engine(H, W, 2), N, dt.depthnet_params(3))
    rd, rs = hip(x=x)
    assert torch.equal(disps[0].detach(), rd[0])
    for a, b in zip(skips, rs):
        assert torch.equal(a.detach(), b)
    with torch.no_grad():
        for p in mod.parameters():
            p.mul_(1.01).add_(1e-3)
    d2 = mod(x)[0][0].detach()
    hip.load({k: v.detach().cpu() for k, v in mod.state_dict().items()})
    r2 = hip.forward(x)
    assert float((d2 - r2).abs().max()) <= 2e-6
    assert not torch.equal(d2, rd[0])
    with torch.no_grad():
        assert torch.equal(mod(x)[0][0], r2)                 # the no-tape path on the device fold


def test_refusals():
    mod = _module(0)
    x = _imgs(1, 1, 64, 192)
    mod.train()
    with pytest.raises(RuntimeError, match="training-mode BatchNorm"):
        mod(x)
    mod.eval()
    with pytest.raises(RuntimeError, match="images"):
        mod(x.clone().requires_grad_(True))
    bad = dict(dt.depthnet_params(0))
    bad["feature_convs.1.0.conv.weight"] = torch.zeros(8, 64, 3, 3)
    from tightly_coupled_sfm_amd.depthnet_train import DepthNetModule
    with pytest.raises(ValueError, match="num_scales"):
        DepthNetModule(bad)


def test_tape_memory_returns_to_baseline():
    mod = _module(4)
    x = _imgs(2, 2, 64, 192)
    R = _cot(9, (2, 1, 64, 192)).float().cuda()
    (mod(x)[0][0] * R).sum().backward()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    for _ in range(20):
        (mod(x)[0][0] * R).sum().backward()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == base


def test_reference_loop_mechanics():
    """a fresh restatement of the reference's weight tuning: deep copy, the copy's encoder parameters in an optimiser, a few epochs"""
    N, H, W, epochs = 2, 64, 192, 3
    x = _imgs(41, N, H, W)
    target = torch.full((N, 1, H, W), 0.3, device="cuda")

    def loop(model, opt_cls, lr, params_of, **call):
        opt = opt_cls(params_of(model), lr=lr)
        losses = []
        for _ in range(epochs):
            opt.zero_grad()
            disp = model(**call)[0][0]
            loss = ((disp.float() - target) ** 2).mean()
            loss.backward()
            opt.step()
            losses.append(float(loss))
        return losses

    orig = _module(5)
    before = {k: v.clone() for k, v in orig.state_dict().items()}
    # SGD on the encoder against the float64 twin
    cp = copy.deepcopy(orig)
    loop(cp, torch.optim.SGD, 0.05, lambda m: m.encoder.parameters(), x=x)
    twin = dt.DepthNetTwin(dt.depthnet_params(5), dtype=torch.float64, device="cuda")
    enc = {k: v.requires_grad_(True) for k, v in twin.p.items() if k.startswith("encoder.") and not k.endswith(("running_mean", "running_var"))}
    opt = torch.optim.SGD(list(enc.values()), lr=0.05)
    for _ in range(epochs):
        opt.zero_grad()
        loss = ((dt.forward(twin.p, x.double()) - target.double()) ** 2).mean()
        loss.backward()
        opt.step()
    for k, v in enc.items():
        assert _rel(cp.get_parameter(k).detach(), v.detach()) <= 1e-4, k
    # Adam: the copy changes and its loss goes down, the original is untouched
    cp = copy.deepcopy(orig)
    losses = loop(cp, torch.optim.Adam, 1e-5, lambda m: m.encoder.parameters(), x=x)
    assert losses[-1] < losses[0]
    assert any(not torch.equal(cp.state_dict()[k], before[k]) for k in before)
    for k, v in orig.state_dict().items():
        assert torch.equal(v, before[k]), k
    # bottleneck values: skips 3 and 4 as leaves
    with torch.no_grad():
        _, sk = orig(x, return_disp=False)
    cp = copy.deepcopy(orig)
    for p in cp.parameters():
        p.requires_grad_(False)
    leaves = [s.clone().requires_grad_(k >= 3) for k, s in enumerate(sk)]
    losses = loop(cp, torch.optim.Adam, 1e-3, lambda m: [leaves[3], leaves[4]], x=None, skips=leaves)
    assert losses[-1] < losses[0] and leaves[0].grad is None
    # decoder weights with fixed skips
    cp = copy.deepcopy(orig)
    dec = [p for k, p in cp.named_parameters() if not k.startswith("encoder.")]
    losses = loop(cp, torch.optim.Adam, 1e-4, lambda m: dec, x=None, skips=[s.clone() for s in sk])
    assert losses[-1] < losses[0]
    for k, v in orig.state_dict().items():
        assert torch.equal(v, before[k]), k


def test_gradients_against_reference_golden():
    """the HIP gradients against the reference module's own (fixture golden_depthnet_grad.npz); tolerances as in the twin parity
    test (encoder: fp32 ReLU / max-pool decisions that differ from float64)"""
    from conftest import load_golden
    from test_depthnet_grad_golden_cpu import check_against_golden, golden_grad_inputs
    g = load_golden("depthnet_grad")
    x, R = golden_grad_inputs(g)
    mod = _module(int(g["seed"]))
    (mod(x.cuda())[0][0] * R.float().cuda()).sum().backward()
    bad = check_against_golden(g, dict((k, p.grad) for k, p in mod.named_parameters()),
                               lambda k: 1e-2 if k.startswith("encoder.") else 1e-4)
    assert not bad, bad


def test_refuses_stale_backward_and_bad_images():
    mod = _module(6)
    x = _imgs(4, 1, 64, 192)
    disp = mod(x)[0][0]
    with torch.no_grad():
        mod.get_parameter("iconvs.0.0.conv.bias").add_(0.1)
    mod(x)                                                   # re-folds the changed parameters into the native state
    with pytest.raises(RuntimeError, match="changed in place"):
        disp.sum().backward()
    with pytest.raises(ValueError, match=r"expected images \[N,3,H,W\]"):
        mod(x[:, :1].contiguous())
