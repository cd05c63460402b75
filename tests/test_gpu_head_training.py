"""Training the RGB-D head end to end on the GPU (training.head_forward_train / head_losses; pytest -m gpu).

head_forward_train against a restatement on the same device -- torch's own F.conv2d (and its autograd) for mask_features, then the
same decoder_forward_train -- on a fixed seeded random weighting of all predictions: the gradients with respect to the embedding,
the convolution and every decoder parameter, per tensor within the fp32 contract: max|got - ref| <= 1e-4 max|ref|.
The attention-mask bits are thresholds of the intermediate mask logits, so the head takes the synthetic parameters
(synthetic.synth_param: mask logits of order 1; under torch's default initialisation every one of the five seeds had some of the
7680 logits within 1e-4 of the threshold) salted by the first seed of (0, 1, 2, 3, 4) whose restatement keeps every intermediate
mask logit at least 1e-4 away from 0 (none: the test fails).
head_losses against the hand-composed weighted_losses of the same pieces."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 1e-4
B, H, W, Q, LAYERS = 2, 12, 20, 8, 2


def _head(seed, **kw):
    from unseenobjectswithmeanshift_amd.meta_arch import build_ucn_head
    from unseenobjectswithmeanshift_amd import synthetic as syn
    torch.manual_seed(seed)
    head = build_ucn_head(num_queries=Q, dec_layers=LAYERS, **kw)
    with torch.no_grad():                                # synthetic initialisation, salted by the seed: mask logits of order 1
        for name, p in head.named_parameters():
            p.copy_(syn.synth_param(name, p.shape, salt=seed))
    return head.to(DEV)


def _embedding(seed):
    g = torch.Generator().manual_seed(100 + seed)
    return F.normalize(torch.randn(B, 64, H, W, generator=g), dim=1).to(DEV)


def _functional(out):
    """A fixed seeded random weighting of all predictions (as tests/golden/make_golden.py's decoder_backward_loss)."""
    g = torch.Generator().manual_seed(5)
    preds = out["aux_outputs"] + [{"pred_logits": out["pred_logits"], "pred_masks": out["pred_masks"]}]
    loss = 0.0
    for p in preds:
        wl = torch.randn(tuple(p["pred_logits"].shape), generator=g, dtype=torch.float64)
        wm = torch.randn(tuple(p["pred_masks"].shape), generator=g, dtype=torch.float64) / (H * W) ** 0.5
        loss = loss + (p["pred_logits"] * wl.float().to(DEV)).sum() + (p["pred_masks"] * wm.float().to(DEV)).sum()
    return loss


def _restatement(head, f):
    from unseenobjectswithmeanshift_amd import training as tr
    conv = head.pixel_decoder.mask_features
    mf = F.conv2d(f, conv.weight, conv.bias, padding=1)                                       # torch's own convolution and autograd
    return tr.decoder_forward_train(head.predictor, [f], mf)


@functools.lru_cache(maxsize=None)
def _setup():
    """(seed, head, names, parameters, restatement outputs, restatement gradients): the first seed whose restatement has no
    intermediate mask logit within 1e-4 of the threshold."""
    for seed in (0, 1, 2, 3, 4):
        head = _head(seed)
        f = _embedding(seed).requires_grad_(True)
        out = _restatement(head, f)
        margin = min(float(a["pred_masks"].detach().abs().min()) for a in out["aux_outputs"])
        print(f"head training seed {seed}: smallest intermediate |mask logit| {margin:.3e}")
        if margin < 1e-4:
            continue
        conv = head.pixel_decoder.mask_features
        named = [("mask_features.weight", conv.weight), ("mask_features.bias", conv.bias)]
        named += [("predictor." + n, p) for n, p in head.predictor.named_parameters()]
        names, params = [n for n, _ in named], [p for _, p in named]
        grads = torch.autograd.grad(_functional(out), [f] + params, allow_unused=True)
        return seed, head, names, params, {k: v for k, v in out.items()}, grads
    pytest.fail("no seed of (0, 1, 2, 3, 4) keeps the intermediate mask logits 1e-4 away from the threshold")


def _within(name, got, ref):
    scale = float(ref.abs().max())
    err = float((got.double() - ref.double()).abs().max())
    print(f"head training: {name} max|d| {err:.3e} of max|ref| {scale:.3e} -> {err / scale if scale else err:.2e}")
    return err <= RTOL * scale


def test_head_forward_train_gradients_vs_torch_conv():
    from unseenobjectswithmeanshift_amd import training as tr
    seed, head, names, params, ref_out, ref_grads = _setup()
    f = _embedding(seed).requires_grad_(True)
    out = tr.head_forward_train(head, {"res5": f})
    assert len(out["aux_outputs"]) == LAYERS
    assert tuple(out["pred_masks"].shape) == (B, Q, H, W) and tuple(out["pred_logits"].shape) == (B, Q, 3)
    grads = torch.autograd.grad(_functional(out), [f] + params, allow_unused=True)
    bad = []
    for name, got, ref in zip(["embedding"] + names, grads, ref_grads):
        assert (got is None) == (ref is None), name
        if ref is not None and not _within("grad " + name, got, ref):
            bad.append(name)
    assert grads[0] is not None and grads[1] is not None and grads[2] is not None
    assert not bad, bad


def test_head_forward_train_matches_inference():
    from unseenobjectswithmeanshift_amd import training as tr
    seed, head, _, _, _, _ = _setup()
    f = _embedding(seed)
    with torch.no_grad():
        out = tr.head_forward_train(head, {"res5": f})
    was_training = head.training
    pred, _ = head.eval()({"res5": f})
    head.train(was_training)
    for k in ("pred_logits", "pred_masks"):
        assert _within(k + " vs eval-mode head", out[k], pred[k]), k


def _loss_setup(seed=3, **head_kw):
    from unseenobjectswithmeanshift_amd import criterion as cr
    from unseenobjectswithmeanshift_amd.embedding_loss import EmbeddingLoss
    head = _head(seed, **head_kw)
    g = torch.Generator().manual_seed(200 + seed)
    emb = (torch.randn(B, 64, H, W, generator=g) * 2).to(DEV).requires_grad_(True)            # not normalised: head_losses does it
    targets, labels = [], torch.full((B, 1, H, W), -1.0)
    for b in range(B):
        masks = torch.zeros(3, H, W, dtype=torch.uint8)
        for t in range(3):
            masks[t, 1 + 3 * t:4 + 3 * t, 2 + b:14 + b] = 1
            labels[b, 0, 1 + 3 * t:4 + 3 * t, 2 + b:14 + b] = t + 1
        labels[b, 0, 10:, :] = 0
        targets.append({"labels": torch.tensor([0, 1, 0]).to(DEV), "masks": masks.to(DEV)})

    def criterion():
        return cr.build_criterion(2, class_weight=2.0, mask_weight=5.0, dice_weight=5.0, no_object_weight=0.1, dec_layers=LAYERS + 1,
                                  train_num_points=112, generator=torch.Generator().manual_seed(9), solver="host")
    return head, emb, targets, labels.to(DEV), criterion, EmbeddingLoss(0.02, 0.5, 1.0, 1.0)


def test_head_losses_vs_hand_composed():
    from unseenobjectswithmeanshift_amd import training as tr
    head, emb, targets, labels, criterion, el = _loss_setup()
    crit = criterion()
    before = dict(crit.weight_dict)
    losses = tr.head_losses(head, emb, targets, crit, labels=labels, embedding_loss=el, embedding_weight=0.5)
    assert crit.weight_dict == before and "embedding_loss" not in crit.weight_dict
    assert set(losses) == set(before) | {"embedding_loss"} and len(losses) == 3 * (LAYERS + 1) + 1
    # the same pieces by hand
    crit2 = criterion()
    norm = F.normalize(emb.detach(), p=2, dim=1)
    raw = crit2(tr.head_forward_train(head, {"res5": norm}), targets)
    raw["embedding_loss"] = el(norm, labels)[0]
    ref = tr.weighted_losses(raw, {**crit2.weight_dict, "embedding_loss": 0.5})
    assert set(ref) == set(losses)
    for k in ref:
        a, r = float(losses[k].detach()), float(ref[k].detach())
        print(f"head_losses {k}: {a:.9g} hand-composed {r:.9g}")
        assert abs(a - r) <= RTOL * abs(r), k
    sum(losses.values()).backward()
    conv = head.pixel_decoder.mask_features
    assert emb.grad is not None and bool(torch.isfinite(emb.grad).all()) and float(emb.grad.abs().max()) > 0
    for p in (conv.weight, conv.bias, head.predictor.query_feat.weight, head.predictor.class_embed.weight):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
    assert all(bool(torch.isfinite(p.grad).all()) for p in head.parameters() if p.grad is not None)
    # without an embedding loss: the criterion's keys only; with one, labels and a weight are required
    plain = tr.head_losses(head, emb, targets, criterion())
    assert set(plain) == set(before)
    with pytest.raises(ValueError, match="labels"):
        tr.head_losses(head, emb, targets, criterion(), embedding_loss=el)


def test_head_losses_mask_dim_64_has_no_convolution():
    from unseenobjectswithmeanshift_amd import training as tr
    head, emb, targets, labels, criterion, el = _loss_setup(mask_dim=64)
    assert not hasattr(head.pixel_decoder, "mask_features")
    losses = tr.head_losses(head, emb, targets, criterion(), labels=labels, embedding_loss=el, embedding_weight=0.5)
    sum(losses.values()).backward()
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    assert emb.grad is not None and bool(torch.isfinite(emb.grad).all()) and float(emb.grad.abs().max()) > 0
