#!/usr/bin/env python3
"""Generate the depth-network fixture G14 by running the reference's own module (build container only; see make_golden.py).

    python tests/golden/make_golden_depthnet.py        # writes tests/golden/golden_depthnet.npz

models.depth_w_access.depth_model (num_scales = 1) in float64 with the seeded parameters of tests/depthnet_twin.depthnet_params, on
the seeded images of depthnet_twin.sample_images: the disparity at 64x192 (N = 3, full) and 192x640 (N = 1, every second row and
column), per-skip statistics (max |skip|, mean, std) and a fixed strided subsample of every skip, input checksums, and the list of
state_dict names and shapes of the reference module (without fc.* and num_batches_tracked).  torchvision is not a dependency of
this project: a local stand-in of torchvision.models provides a ResNet18 built from BasicBlocks whose resnet18(pretrained) ignores
`pretrained` (nothing is downloaded).  Data only: nothing from the reference's source text is copied.
"""
import os
import sys
import types

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REPO, REF  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "tests"))
from depthnet_twin import depthnet_params, sample_images  # noqa: E402

SEED = 0
SKIP_SAMPLES = 2048


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample

    def forward(self, x):
        idn = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        return self.relu(self.bn2(self.conv2(out)) + idn)


class ResNet(nn.Module):
    def __init__(self, block, layers, num_classes=1000):
        super().__init__()
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], 2)
        self.layer3 = self._make_layer(block, 256, layers[2], 2)
        self.layer4 = self._make_layer(block, 512, layers[3], 2)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512, num_classes)

    def _make_layer(self, block, planes, blocks, stride=1):
        ds = None
        if stride != 1 or self.inplanes != planes:
            ds = nn.Sequential(nn.Conv2d(self.inplanes, planes, 1, stride, bias=False), nn.BatchNorm2d(planes))
        layers = [block(self.inplanes, planes, stride, ds)]
        self.inplanes = planes
        layers += [block(planes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*layers)


def resnet18(pretrained=False, **kw):
    return ResNet(BasicBlock, [2, 2, 2, 2])       # `pretrained` is ignored: no weights are downloaded


def _unsupported(*a, **k):
    raise NotImplementedError("only resnet18 is provided by the stand-in")


def install_torchvision_standin():
    tv = types.ModuleType("torchvision")
    models = types.ModuleType("torchvision.models")
    resnet = types.ModuleType("torchvision.models.resnet")
    resnet.BasicBlock, resnet.Bottleneck, resnet.ResNet, resnet.model_urls = BasicBlock, BasicBlock, ResNet, {}
    models.resnet, models.ResNet = resnet, ResNet
    models.resnet18 = resnet18
    models.resnet34 = models.resnet50 = models.resnet101 = models.resnet152 = _unsupported
    tv.models = models
    sys.modules.update({"torchvision": tv, "torchvision.models": models, "torchvision.models.resnet": resnet})


def main():
    install_torchvision_standin()
    sys.path.insert(0, REF)
    from models.depth_w_access import depth_model
    net = depth_model({"num_scales": 1}).double().eval()
    sd_ref = net.state_dict()
    names = [k for k in sd_ref if not k.endswith("num_batches_tracked") and ".fc." not in k]
    params = depthnet_params(SEED)
    missing = set(names) ^ set(params)
    assert not missing, f"parameter names differ from the reference module: {sorted(missing)}"
    net.load_state_dict({k: v.double() for k, v in params.items()}, strict=False)
    out = {"seed": np.int64(SEED), "names": np.array(names), "shapes": np.array([list(sd_ref[k].shape) + [0] * (4 - sd_ref[k].dim()) for k in names])}
    rs = np.random.RandomState(77)
    for tag, (img_seed, N, H, W, step) in {"s64x192": (11, 3, 64, 192, 1), "s192x640": (12, 1, 192, 640, 2)}.items():
        x = sample_images(img_seed, N, H, W)
        with torch.no_grad():
            disps, skips = net(x=torch.from_numpy(x).double())
        d = disps[0].numpy()
        out[f"{tag}_img_seed"] = np.int64(img_seed)
        out[f"{tag}_img_sum"] = np.float64(x.astype(np.float64).sum())
        out[f"{tag}_img_sumsq"] = np.float64((x.astype(np.float64) ** 2).sum())
        out[f"{tag}_disp_step"] = np.int64(step)
        out[f"{tag}_disp"] = d[:, :, ::step, ::step].astype(np.float32)
        out[f"{tag}_disp_stats"] = np.array([d.mean(), d.std(), d.std(axis=(1, 2, 3)).min()])
        for k, s in enumerate(skips):
            s = s.numpy()
            idx = np.sort(rs.choice(s.size, size=min(SKIP_SAMPLES, s.size), replace=False))
            out[f"{tag}_skip{k}_idx"] = idx.astype(np.int64)
            out[f"{tag}_skip{k}_val"] = s.reshape(-1)[idx].astype(np.float32)
            out[f"{tag}_skip{k}_stats"] = np.array([np.abs(s).max(), s.mean(), s.std()])
        print(tag, "disp mean / std / min per-image std", out[f"{tag}_disp_stats"], "skip max", [float(np.abs(s).max()) for s in skips])
    path = os.path.join(HERE, "golden_depthnet.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
