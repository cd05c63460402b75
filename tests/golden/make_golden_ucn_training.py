"""tests/golden/ucn_backbone_train.npz: the reference's own Resnet34_8s towers in TRAINING mode (batch statistics, running
statistics updated) with the SEGNET glue of lib/networks/SEG.py:104-114, in float64.

    python tests/golden/make_golden_ucn_training.py <reference>/lib/networks

Needs only torch: resnet.py and resnet_dilated.py are loaded by file path, as make_golden.py::g_ucn_backbone does, take the
synthetic parameters ``synthetic.ucn_backbone_state_dict(salt=6)`` and the seeded (2, 3, 64, 96) inputs of that fixture, and run
ONE forward in ``.train()`` mode on the CPU.  Stored: feats[:, :, ::3, ::3] (both towers, add fusion, F.normalize) and
rgb_only[:, :, ::6, ::6] (the colour tower alone, normalised) from that forward, and every BatchNorm's running_mean, running_var
and num_batches_tracked after it, under the package's state-dict names ("fcn.resnet34_8s.bn1.running_mean", ...).  Gradients are
not stored: at network level torch's own fp32 backward is up to 8.6e-2 of a parameter tensor's maximum away from float64 (ReLU
and max-pool decisions flip between the precisions), so tests/test_gpu_ucn_training.py pins the backward against torch autograd
of the same graph instead."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from unseenobjectswithmeanshift_amd import synthetic as syn  # noqa: E402


def load_reference(networks_dir):
    pkg = types.ModuleType("refnetworks")
    pkg.__path__ = [networks_dir]
    sys.modules["refnetworks"] = pkg
    for name in ("resnet", "resnet_dilated"):
        spec = importlib.util.spec_from_file_location(f"refnetworks.{name}", os.path.join(networks_dir, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[f"refnetworks.{name}"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["refnetworks.resnet_dilated"]


def main(networks_dir):
    RD = load_reference(networks_dir)
    shapes = syn.ucn_backbone_param_shapes()
    sd = syn.ucn_backbone_state_dict(shapes, salt=6)
    towers = {}
    for t in ("fcn", "fcn_depth"):
        net = RD.Resnet34_8s(num_classes=64, input_channels=3, pretrained=False)
        assert list(net.state_dict()) == [k[len(t) + 1:] for k in shapes if k.startswith(t + ".")], "backbone state-dict layout drifted"
        net.load_state_dict({k[len(t) + 1:]: v for k, v in sd.items() if k.startswith(t + ".")}, strict=True)
        towers[t] = net.double().train()
    g = torch.Generator().manual_seed(31)
    img = torch.randn(2, 3, 64, 96, generator=g).double()
    depth = (torch.randn(2, 3, 64, 96, generator=g) * 0.5).double()
    with torch.no_grad():                                                         # one forward: every running statistic moves once
        rgb = towers["fcn"](img)
        feats = F.normalize(rgb + towers["fcn_depth"](depth), p=2, dim=1)        # SEG.py:104-114
        rgb_only = F.normalize(rgb, p=2, dim=1)                                   # INPUT 'COLOR' (SEG.py:99-100)
    # float64 results rounded once to float32 (6e-8 relative, against a 1e-4 contract): the file stays below 1 MB
    out = {"feats": feats[:, :, ::3, ::3].float().contiguous().numpy(), "rgb_only": rgb_only[:, :, ::6, ::6].float().contiguous().numpy()}
    for t, net in towers.items():
        for k, v in net.state_dict().items():
            if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
                out[f"{t}.{k}"] = (v.float() if v.is_floating_point() else v).numpy()
    path = os.path.join(HERE, "ucn_backbone_train.npz")
    np.savez_compressed(path, **out)
    print(f"ucn_backbone_train: {len(out)} arrays, {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main(sys.argv[1])
