"""Training the UCN RGB-D backbone from images on the GPU (training.ucn_towers_forward_train / ucn_backbone_forward_train /
ucn_model_losses; pytest -m gpu), B = 2 at 64 x 96 with MIOpen's find mode off.

The backward of the towers is torch autograd of stock modules on both routes; what is the package's own is the tail, so the wiring
test backpropagates the fused tail and torch's tail through ONE retained tower graph: every ReLU and max-pool decision is shared
and no element is excused from the fp32 contract."""
import pytest
import torch

import ucn_training_cases as uc
from test_backbone_cpu import backbone_inputs, make_backbone

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Q, LAYERS = 8, 2                                 # the smallest decoder of tests/test_gpu_head_training.py


def _backbone(train=True, use_depth=True):
    from unseenobjectswithmeanshift_amd.ucn_backbone import UCNBackbone
    if use_depth:
        net = make_backbone(DEV)
    else:
        from unseenobjectswithmeanshift_amd import synthetic as syn
        net = UCNBackbone(num_units=64, in_channels=3, use_depth=False)
        sd = syn.ucn_backbone_state_dict(syn.ucn_backbone_param_shapes(), salt=6)
        net.load_state_dict({k: v for k, v in sd.items() if k.startswith("fcn.")}, strict=True)
        net = net.to(DEV)
    net.miopen_find = False
    return net.train(train)


@pytest.mark.parametrize("norms", [1, 2])
def test_fused_and_torch_tail_through_one_tower_graph(norms):
    from unseenobjectswithmeanshift_amd import training as tr
    net = _backbone()
    img, depth = (t.to(DEV).requires_grad_(True) for t in backbone_inputs())
    lo_a, lo_b = tr.ucn_towers_forward_train(net, img, depth)
    assert lo_a.shape == lo_b.shape == (2, 64, 8, 12) and lo_a.dtype == torch.float32
    size = img.shape[2:]
    y_fused = tr.ucn_embedding_tail(lo_a, lo_b, size, norms=norms)
    y_torch = tr.ucn_embedding_tail(lo_a, lo_b, size, norms=norms, fused=False)
    assert uc.within(f"norms {norms}: y fused vs torch", y_fused, y_torch.detach().cpu())
    gout = torch.randn(y_fused.shape, generator=torch.Generator().manual_seed(17)).to(DEV)
    named = list(net.named_parameters()) + [("img", img), ("depth", depth)]
    leaves = [p for _, p in named]
    got = torch.autograd.grad(y_fused, leaves, gout, retain_graph=True)
    ref = torch.autograd.grad(y_torch, leaves, gout)
    bad = []
    for (name, _), a, r in zip(named, got, ref):
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0, name
        if not uc.within(f"norms {norms}: grad {name}", a, r.cpu()):
            bad.append(name)
    assert not bad, bad


def test_forward_train_is_the_composition(monkeypatch):
    """Bit for bit on the maps the call itself computed (two runs of the library convolutions and batch statistics are not the same
    bits on this GPU, so a second run of the towers is held to the contract instead), one update of the running statistics per call."""
    from unseenobjectswithmeanshift_amd import training as tr
    img, depth = (t.to(DEV) for t in backbone_inputs())
    towers, seen = tr.ucn_towers_forward_train, []

    def spy(*args, **kw):
        seen.append(towers(*args, **kw))
        return seen[-1]

    for renorm in (False, True):
        net = _backbone()
        bns = uc.batchnorms(net)
        monkeypatch.setattr(tr, "ucn_towers_forward_train", spy)
        whole = tr.ucn_backbone_forward_train(net, img, depth, renormalize=renorm)
        monkeypatch.setattr(tr, "ucn_towers_forward_train", towers)
        assert all(int(m.num_batches_tracked) == 1 for _, m in bns)              # one update per call, both towers
        lo_a, lo_b = seen.pop()
        assert not seen and torch.equal(whole, tr.ucn_embedding_tail(lo_a, lo_b, img.shape[2:], norms=1 + renorm))
        first = {n: m.running_mean.clone() for n, m in bns}
        lo_a, lo_b = tr.ucn_towers_forward_train(net, img, depth)
        parts = tr.ucn_embedding_tail(lo_a, lo_b, img.shape[2:], norms=1 + renorm)
        assert all(int(m.num_batches_tracked) == 2 for _, m in bns)
        assert uc.within("second run of the towers", parts, whole.detach().cpu())   # batch statistics do not depend on the running ones
        # the second update moved every running mean by momentum * (batch mean - running mean) again: not equal to the first
        assert all(not torch.equal(first[n], m.running_mean) for n, m in bns)
        torch.testing.assert_close(whole.detach().norm(dim=1), torch.ones(2, 64, 96, device=DEV), rtol=1e-5, atol=1e-5)


def test_train_mode_matches_the_reference_towers(golden):
    uc.check_train_mode(golden, DEV, fused_tail=True)


def test_eval_mode_batchnorm_matches_inference(golden):
    uc.check_eval_batchnorm(golden, DEV, fused_tail=True)


def test_colour_only_with_and_without_a_depth_tower():
    from unseenobjectswithmeanshift_amd import training as tr
    img, depth = (t.to(DEV) for t in backbone_inputs())
    both, single = _backbone(), _backbone(use_depth=False)
    a = tr.ucn_backbone_forward_train(both, img)
    b = tr.ucn_backbone_forward_train(single, img)
    assert a.shape == b.shape == (2, 64, 64, 96) and uc.within("colour only, with vs without a depth tower", a, b.detach().cpu())
    a.sum().backward()
    assert all(p.grad is None for p in both.fcn_depth.parameters())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in both.fcn.parameters())
    with pytest.raises(RuntimeError, match="depth tower"):
        tr.ucn_backbone_forward_train(single, img, depth)
    both.backbone_dtype = "f16"
    with pytest.raises(NotImplementedError):
        tr.ucn_backbone_forward_train(both, img, depth)


def _model_and_batch():
    from unseenobjectswithmeanshift_amd import criterion as cr
    from unseenobjectswithmeanshift_amd import synthetic as syn
    from unseenobjectswithmeanshift_amd.embedding_loss import EmbeddingLoss
    from unseenobjectswithmeanshift_amd.meta_arch import build_ucn_model
    torch.manual_seed(3)
    model = build_ucn_model(num_queries=Q, dec_layers=LAYERS)
    with torch.no_grad():                                # synthetic initialisation: mask logits of order 1 (as test_gpu_head_training)
        for name, p in model.sem_seg_head.named_parameters():
            p.copy_(syn.synth_param(name, p.shape, salt=3))
    model.backbone.load_state_dict(syn.ucn_backbone_state_dict(syn.ucn_backbone_param_shapes(), salt=6), strict=True)
    model = model.to(DEV).train()
    model.backbone.miopen_find = False
    img, depth = (t.to(DEV) for t in backbone_inputs())
    H, W = img.shape[2:]
    targets, labels = [], torch.full((2, 1, H, W), -1.0)
    for b in range(2):
        masks = torch.zeros(3, H, W, dtype=torch.uint8)
        for t in range(3):
            masks[t, 4 + 16 * t:18 + 16 * t, 8 + 4 * b:70 + 4 * b] = 1
            labels[b, 0, 4 + 16 * t:18 + 16 * t, 8 + 4 * b:70 + 4 * b] = t + 1
        labels[b, 0, 54:, :] = 0
        targets.append({"labels": torch.tensor([0, 1, 0]).to(DEV), "masks": masks.to(DEV)})

    def criterion():
        return cr.build_criterion(2, class_weight=2.0, mask_weight=5.0, dice_weight=5.0, no_object_weight=0.1, dec_layers=LAYERS + 1,
                                  train_num_points=112, generator=torch.Generator().manual_seed(9), solver="host")
    return model, img, depth, targets, labels.to(DEV), criterion, EmbeddingLoss(0.02, 0.5, 1.0, 1.0)


def test_model_losses_end_to_end():
    from unseenobjectswithmeanshift_amd import training as tr
    from unseenobjectswithmeanshift_amd.optim import build_optimizer
    model, img, depth, targets, labels, criterion, el = _model_and_batch()
    opt = build_optimizer(model, base_lr=1e-3)
    losses = tr.ucn_model_losses(model, img, depth, targets, criterion(), labels=labels, embedding_loss=el, embedding_weight=0.5)
    assert len(losses) == 3 * (LAYERS + 1) + 1 and "embedding_loss" in losses
    # the same step from the backbone's own (once-normalised) embedding through head_losses, which normalises once more
    emb = tr.ucn_backbone_forward_train(model.backbone, img, depth, renormalize=False).detach()
    ref = tr.head_losses(model.sem_seg_head, emb, targets, criterion(), labels=labels, embedding_loss=el, embedding_weight=0.5)
    assert set(ref) == set(losses)
    for k in ref:
        a, r = float(losses[k].detach()), float(ref[k].detach())
        print(f"ucn_model_losses {k}: {a:.9g} head_losses {r:.9g}")
        assert a == a and abs(a) != float("inf") and abs(a - r) <= 1e-5 * abs(r), k
    sum(losses.values()).backward()
    params = dict(model.named_parameters())
    assert any(k.startswith("backbone.fcn_depth.") for k in params) and any(k.startswith("sem_seg_head.") for k in params)
    for name, p in params.items():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    before = {k: p.detach().clone() for k, p in params.items()}
    opt.step()
    torch.cuda.synchronize()
    moved = [k for k, p in params.items() if not torch.equal(before[k], p.detach())]
    still = [k for k in params if k not in moved and float(params[k].grad.abs().max()) > 0]
    assert not still, still
    assert any(k.startswith("backbone.fcn.") for k in moved) and any(k.startswith("sem_seg_head.predictor.") for k in moved)
    with pytest.raises(ValueError, match="labels"):
        tr.ucn_model_losses(model, img, depth, targets, criterion(), embedding_loss=el)
