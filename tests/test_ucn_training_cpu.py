"""The UCN backbone under autograd on the CPU (torch's tail): training-mode semantics against the reference's own towers in
training mode (tests/golden/ucn_backbone_train.npz), eval-mode BatchNorm against the inference module, and the inference
module's refusal of training mode, which stays."""
import pytest
import torch

import ucn_training_cases as uc
from test_backbone_cpu import backbone_inputs, make_backbone


def test_train_mode_matches_the_reference_towers(golden):
    uc.check_train_mode(golden, "cpu", fused_tail=False)


def test_eval_mode_batchnorm_matches_inference(golden):
    uc.check_eval_batchnorm(golden, "cpu", fused_tail=False)


def test_gradients_reach_every_parameter_and_input():
    from unseenobjectswithmeanshift_amd import training as tr
    net = make_backbone().train()
    img, depth = (t.requires_grad_(True) for t in backbone_inputs())
    lo_a, lo_b = tr.ucn_towers_forward_train(net, img, depth)
    assert lo_a.shape == lo_b.shape == (2, 64, 8, 12)
    y = tr.ucn_embedding_tail(lo_a, lo_b, img.shape[2:], norms=1, fused=False)
    g = torch.randn(y.shape, generator=torch.Generator().manual_seed(3))
    y.backward(g)
    for name, p in list(net.named_parameters()) + [("img", img), ("depth", depth)]:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name


def test_inference_module_still_rejects_training_mode():
    net = make_backbone().train()
    img, depth = backbone_inputs()
    with pytest.raises(NotImplementedError):
        net(img, None, depth)


def test_unsupported_configurations_raise():
    from unseenobjectswithmeanshift_amd import training as tr
    from unseenobjectswithmeanshift_amd.ucn_backbone import UCNBackbone
    img, depth = backbone_inputs()
    net = make_backbone()
    net.backbone_dtype = "bf16"
    with pytest.raises(NotImplementedError, match="fp32"):
        tr.ucn_towers_forward_train(net, img, depth)
    with pytest.raises(RuntimeError, match="depth tower"):
        tr.ucn_towers_forward_train(UCNBackbone(use_depth=False), img, depth)
