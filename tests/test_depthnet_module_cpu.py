"""CPU: depthnet_train.DepthNetModule's parameter tree reproduces the reference depth_model's names (what the reference's weight
tuning reads: state_dict(), encoder.parameters(), deep copies), without touching a GPU."""
import copy
import os
import sys

import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def test_module_tree_matches_reference_names():
    import depthnet_twin as dt
    from tightly_coupled_sfm_amd.depthnet_train import DepthNetModule
    sd = dict(dt.depthnet_params(0))
    sd["fc.weight"] = torch.zeros(1000, 512)                        # accepted and ignored
    mod = DepthNetModule(sd)
    assert not mod.training
    assert list(mod.state_dict()) == list(dt.param_shapes())
    for k, v in dt.depthnet_params(0).items():
        assert torch.equal(mod.state_dict()[k], v), k
    assert "encoder.encoder.layer1.0.conv1.weight" in dict(mod.named_parameters())
    assert "depth_upconvs.0.1.conv.weight" in dict(mod.named_parameters())
    assert "encoder.encoder.bn1.running_mean" in dict(mod.named_buffers())
    enc = {id(p) for p in mod.encoder.parameters()}
    want = {id(p) for k, p in mod.named_parameters() if k.startswith("encoder.encoder.")}
    assert enc == want and len(enc) == 60
    cp = copy.deepcopy(mod)
    with torch.no_grad():
        cp.get_parameter("encoder.encoder.conv1.weight").add_(1.0)
    assert not torch.equal(cp.state_dict()["encoder.encoder.conv1.weight"], mod.state_dict()["encoder.encoder.conv1.weight"])
    bad = dict(dt.depthnet_params(0))
    del bad["iconvs.2.0.conv.bias"]
    with pytest.raises(KeyError, match="iconvs.2.0.conv.bias"):
        DepthNetModule(bad)
