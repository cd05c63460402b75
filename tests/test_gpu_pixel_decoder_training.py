"""Training the ResNet-50 head's pixel decoder on the GPU (training.pixel_decoder_forward_train / segmentation_head_forward_train;
pytest -m gpu).

Golden case tests/golden/pixel_decoder_backward.npz (made by tests/golden/make_golden_pixel_decoder_backward.py from the imported
reference in float64; tests/test_pd_bwd_cases_cpu.py checks the file): the outputs of pixel_decoder_forward_train and the gradients of
the stored functional for the four feature maps and every parameter, per tensor within the fp32 contract:
max|got - ref64| <= 1e-4 max|ref64| -- four times the reference's own stored fp32 error for a tensor where that error exceeds a quarter
of the contract (none does: the generator's seed search, re-asserted on the CPU).  The figures are printed (pytest -s) and recorded
in DESIGN.md section 5t."""
import functools
import os

import numpy as np
import pytest
import torch

import pd_bwd_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pixel_decoder_backward.npz")


@functools.lru_cache(maxsize=None)
def _golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def _pixel_decoder(seed):
    from unseenobjectswithmeanshift_amd.modeling import MSDeformAttnPixelDecoder, ShapeSpec
    shape = {k: ShapeSpec(channels=c, stride=s) for k, c, s in zip(("res2", "res3", "res4", "res5"), K.PD_IN_CHANNELS, (4, 8, 16, 32))}
    pd = MSDeformAttnPixelDecoder(shape, transformer_dropout=0.0, transformer_nheads=8, transformer_dim_feedforward=K.PD_FFN,
                                  transformer_enc_layers=K.PD_ENC_LAYERS, conv_dim=K.PD_CONV_DIM, mask_dim=K.PD_MASK_DIM, norm="GN",
                                  transformer_in_features=["res3", "res4", "res5"], common_stride=4)
    pd.load_state_dict(K.pd_state_dict(seed), strict=True)
    return pd.to(DEV)


@functools.lru_cache(maxsize=None)
def _trained():
    """One forward + backward of the golden case: (pd, outputs, gradients by the fixture's keys)."""
    from unseenobjectswithmeanshift_amd import training as tr
    seed = int(_golden()["seed"])
    pd = _pixel_decoder(seed)
    feats = {k: v.to(DEV).requires_grad_(True) for k, v in K.pd_features(seed).items()}
    mf, enc, ms = tr.pixel_decoder_forward_train(pd, feats)
    K.pd_functional(mf, enc, ms, seed).backward()
    torch.cuda.synchronize()
    got = {"out__mask_features": mf.detach()[:, ::K.PD_MF_STRIDE]}
    got.update({f"out__ms{i}": t.detach() for i, t in enumerate(ms)})
    got.update({"g_in__" + k: v.grad for k, v in feats.items()})
    got.update({"g__" + n: p.grad for n, p in pd.named_parameters()})
    return pd, (mf.detach(), enc.detach(), [t.detach() for t in ms]), got


def test_outputs_and_gradients_match_the_float64_reference():
    z = _golden()
    _, (mf, enc, ms), got = _trained()
    assert tuple(mf.shape) == (K.PD_BATCH, K.PD_MASK_DIM, 12, 20) and len(ms) == 3 and torch.equal(enc, ms[0])
    keys = [k for k in z if k.startswith(("out__", "g_in__", "g__"))]
    assert sorted(keys) == sorted(got) and len(keys) == 4 + 4 + len(K.pd_param_shapes())
    bad, worst = [], {}
    for k in keys:
        assert got[k] is not None, k                                                       # every input and parameter is reached
        ref = torch.from_numpy(z[k]).double()
        assert tuple(got[k].shape) == tuple(ref.shape), k
        scale = float(ref.abs().max())
        err = float((got[k].detach().cpu().double() - ref).abs().max())
        err32 = float(z["err32__" + k])
        bound = K.RTOL * scale if err32 <= 0.25 * K.RTOL * scale else 4.0 * err32
        group = k.split("__")[0] if not k.startswith("g__") else "g__" + ("encoder" if "transformer" in k else "convolutions")
        worst[group] = max(worst.get(group, (0.0, 0.0)), (err / scale, err32 / scale))
        print(f"pixel decoder training: {k} max|d| {err:.3e} of max|ref| {scale:.3e} -> {err / scale:.2e} (reference fp32 {err32 / scale:.2e})")
        if not err <= bound:
            bad.append(k)
    for group, (frac, frac32) in worst.items():
        print(f"pixel decoder training: worst of {group}: {frac:.2e} of max|ref| (reference fp32, same tensor: {frac32:.2e})")
    assert not bad, bad


def test_outputs_match_eval_mode_forward_features():
    pd, (mf, enc, ms), _ = _trained()
    seed = int(_golden()["seed"])
    feats = {k: v.to(DEV) for k, v in K.pd_features(seed).items()}
    was_training = pd.training
    ref_mf, ref_enc, ref_ms = pd.eval().forward_features(feats)
    pd.train(was_training)
    for name, a, b in [("mask_features", mf, ref_mf), ("encoder features", enc, ref_enc)] + [(f"ms{i}", x, y) for i, (x, y) in enumerate(zip(ms, ref_ms))]:
        assert tuple(a.shape) == tuple(b.shape), name
        K.check("pixel decoder training", "golden", name + " vs eval-mode forward_features", a, b.detach().cpu().double())


def test_segmentation_head_trains_every_parameter():
    from unseenobjectswithmeanshift_amd import criterion as cr
    from unseenobjectswithmeanshift_amd import synthetic as syn
    from unseenobjectswithmeanshift_amd import training as tr
    from unseenobjectswithmeanshift_amd.meta_arch import build_resnet50_head
    head = build_resnet50_head(num_queries=4, dec_layers=1, enc_layers=1)
    with torch.no_grad():
        for name, p in head.named_parameters():
            p.copy_(syn.synth_param(name, p.shape, salt=1))
    head = head.to(DEV)
    gen = torch.Generator().manual_seed(11)
    # a 64 x 96 frame: the decoder's attention masks need the levels to divide the mask resolution (msm_mask_logits_fwd)
    sizes = {"res2": (16, 24), "res3": (8, 12), "res4": (4, 6), "res5": (2, 3)}
    feats = {k: torch.randn(2, c, *sizes[k], generator=gen).to(DEV).requires_grad_(True)
             for k, c in zip(("res2", "res3", "res4", "res5"), (256, 512, 1024, 2048))}
    targets = []
    for b in range(2):
        masks = torch.zeros(2, 64, 96, dtype=torch.uint8)
        masks[0, 4:28, 8 + 4 * b:48] = 1
        masks[1, 36:60, 40:88 - 4 * b] = 1
        targets.append({"labels": torch.tensor([0, 1]).to(DEV), "masks": masks.to(DEV)})
    crit = cr.build_criterion(2, class_weight=2.0, mask_weight=5.0, dice_weight=5.0, no_object_weight=0.1, dec_layers=2,
                              train_num_points=112, generator=torch.Generator().manual_seed(9), solver="host")
    out = tr.segmentation_head_forward_train(head, feats)
    assert len(out["aux_outputs"]) == 1 and tuple(out["pred_masks"].shape) == (2, 4, 16, 24) and tuple(out["pred_logits"].shape) == (2, 4, 3)
    losses = tr.weighted_losses(crit(out, targets), crit.weight_dict)
    assert any(k.endswith("_0") for k in losses)                                           # the auxiliary prediction is supervised
    total = sum(losses.values())
    assert torch.isfinite(total)
    total.backward()
    # one decoder layer attends level 0 only (DEC:608): the decoder's input projections of levels 1 and 2 cannot reach the loss
    unreachable = {f"predictor.input_proj.{i}.{leaf}" for i in (1, 2) for leaf in ("weight", "bias")}
    names = [n for n, _ in head.named_parameters()]
    assert unreachable <= set(names)
    for n, p in head.named_parameters():
        if n in unreachable:
            assert p.grad is None, n
        else:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    for k, v in feats.items():
        assert v.grad is not None and bool(torch.isfinite(v.grad).all()) and float(v.grad.abs().max()) > 0, k
    # the same dict through the one-call entry point (a fresh criterion: the same point-sampling seed)
    crit2 = cr.build_criterion(2, class_weight=2.0, mask_weight=5.0, dice_weight=5.0, no_object_weight=0.1, dec_layers=2,
                               train_num_points=112, generator=torch.Generator().manual_seed(9), solver="host")
    again = tr.segmentation_head_losses(head, feats, targets, crit2)
    assert set(again) == set(losses)
    for k in losses:                                                                       # the forward's moments are atomic sums: equal up to the last bits
        assert abs(float(again[k]) - float(losses[k])) <= 1e-5 * abs(float(losses[k])), k


def test_head_forward_train_still_rejects_this_head():
    from unseenobjectswithmeanshift_amd import training as tr
    from unseenobjectswithmeanshift_amd.meta_arch import build_resnet50_head
    head = build_resnet50_head(num_queries=4, dec_layers=1, enc_layers=1).to(DEV)
    with pytest.raises(NotImplementedError, match="MSDeformAttnPixelDecoder"):
        tr.head_forward_train(head, {"res5": torch.zeros(1, 64, 4, 4, device=DEV)})
    assert callable(tr.segmentation_head_forward_train)


@pytest.mark.parametrize("rows", [4095, 4096, 8200])
def test_linear_over_long_token_maps(rows):
    """training.linear's weight and bias gradients reduce over the rows of the token map: one GEMM below 4096 rows, from there on
    up to 64 split-K parts added in index order (4096: two parts of 2048; 8200: four parts, the last one short).  Against float64
    CPU autograd, the fp32 contract per tensor."""
    import torch.nn.functional as F
    from unseenobjectswithmeanshift_amd import training as tr
    assert callable(tr.pixel_decoder_forward_train)
    gen = torch.Generator().manual_seed(rows)
    x, w, b = torch.randn(2, rows // 2, 64, generator=gen), torch.randn(96, 64, generator=gen) / 8, torch.randn(96, generator=gen)
    g = torch.randn(2, rows // 2, 96, generator=gen)
    ref = [t.double().requires_grad_(True) for t in (x, w, b)]
    F.linear(*ref).backward(g.double())
    got = [t.to(DEV).requires_grad_(True) for t in (x, w, b)]
    y = tr.linear(*got)
    y.backward(g.to(DEV))
    K.check("linear", f"rows={2 * (rows // 2)}", "y", y, F.linear(*ref).detach())
    for name, a, r in zip(("dx", "dw", "db"), got, ref):
        K.check("linear", f"rows={2 * (rows // 2)}", name, a.grad, r.grad)
