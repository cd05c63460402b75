"""Shared checks of the UCN backbone under autograd (training.ucn_backbone_forward_train) against tests/golden/ucn_backbone_train.npz
(the reference's towers in training mode, float64; tests/golden/make_golden_ucn_training.py) and against the inference module --
helper, not collected.  tests/test_ucn_training_cpu.py runs them on the CPU with torch's tail, tests/test_gpu_ucn_training.py on the
GPU with the fused one."""
import torch

from test_backbone_cpu import backbone_inputs, make_backbone

RTOL = 1e-4                                      # the fp32 contract: max|got - ref64| <= RTOL * max|ref64| per tensor


def within(what, got, ref, rtol=RTOL):
    ref = ref.double()
    scale = float(ref.abs().max())
    err = float((got.detach().cpu().double() - ref).abs().max())
    print(f"ucn training: {what} max|d| {err:.3e} of max|ref| {scale:.3e} -> {err / scale if scale else err:.2e}")
    return err <= rtol * scale


def batchnorms(net):
    return [(n, m) for n, m in net.named_modules() if isinstance(m, torch.nn.BatchNorm2d)]


def check_train_mode(golden, device, fused_tail):
    """One forward of a backbone in training mode: the golden outputs and the golden buffers after it, within the contract."""
    from unseenobjectswithmeanshift_amd import training as tr
    g = golden("ucn_backbone_train")
    img, depth = (t.to(device) for t in backbone_inputs())
    net = make_backbone(device).train()
    net.miopen_find = False
    feats = tr.ucn_backbone_forward_train(net, img, depth, fused_tail=fused_tail)
    assert feats.shape == (2, 64, 64, 96) and feats.requires_grad
    assert within("train-mode feats", feats[:, :, ::3, ::3], torch.from_numpy(g["feats"]))
    sd = net.state_dict()
    keys = [k for k in sd if k.endswith(("running_mean", "running_var", "num_batches_tracked"))]
    assert sorted(keys) == sorted(k for k in g.files if k not in ("feats", "rgb_only")) and len(keys) == 3 * len(batchnorms(net))
    bad = []
    for k in keys:
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(g[k]) == 1, k
        elif not within(k, sd[k], torch.from_numpy(g[k])):
            bad.append(k)
    assert not bad, bad
    # colour only, on a backbone of its own (batch statistics do not depend on the running ones, but each call moves them)
    net = make_backbone(device).train()
    net.miopen_find = False
    rgb = tr.ucn_backbone_forward_train(net, img, fused_tail=fused_tail)
    assert within("train-mode rgb_only", rgb[:, :, ::6, ::6], torch.from_numpy(g["rgb_only"]))
    assert int(net.fcn.resnet34_8s.bn1.num_batches_tracked) == 1 and int(net.fcn_depth.resnet34_8s.bn1.num_batches_tracked) == 0


def check_eval_batchnorm(golden, device, fused_tail):
    """Every BatchNorm in eval(): UCNBackbone.forward and the existing ucn_backbone.npz, at test_backbone_cpu.check_backbone's
    tolerances, for renormalize False and True; no buffer moves."""
    from unseenobjectswithmeanshift_amd import training as tr
    g = golden("ucn_backbone")
    img, depth = (t.to(device) for t in backbone_inputs())
    net = make_backbone(device)
    net.miopen_find = False
    before = {k: v.clone() for k, v in net.state_dict().items()}
    for mode in (False, True):                                                  # backbone.training does not matter: the BatchNorms decide
        net.train(mode)
        for _, m in batchnorms(net):
            m.eval()
        for renorm in (False, True):
            got = tr.ucn_backbone_forward_train(net, img, depth, renormalize=renorm, fused_tail=fused_tail)
            ref = net.eval()(img, None, depth, renormalize=renorm)
            torch.testing.assert_close(got.detach(), ref, rtol=2e-4, atol=2e-5)
            torch.testing.assert_close(got.detach()[:, :, ::3, ::3].cpu(), torch.from_numpy(g["feats"]), rtol=2e-4, atol=2e-5)
            net.train(mode)
            for _, m in batchnorms(net):
                m.eval()
        rgb = tr.ucn_backbone_forward_train(net, img, fused_tail=fused_tail)
        torch.testing.assert_close(rgb.detach()[:, :, ::6, ::6].cpu(), torch.from_numpy(g["rgb_only"]), rtol=2e-4, atol=2e-5)
    after = net.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
