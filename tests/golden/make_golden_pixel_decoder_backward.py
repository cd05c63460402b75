"""Generate tests/golden/pixel_decoder_backward.npz: outputs and gradients of the REFERENCE pixel decoder
(MSMFormer/meanshiftformer/modeling/pixel_decoder/msdeformattn.py, imported through _ref_import.py with its pure-torch core
ms_deform_attn_core_pytorch) in float64 on a small seeded case, for training.pixel_decoder_forward_train.

Run in the build container only:   python tests/golden/make_golden_pixel_decoder_backward.py

Case (tests/pd_bwd_cases.py): conv_dim 64, mask_dim 256, 2 encoder layers, dim_feedforward 128, in-channels (16, 24, 32, 48); feature
maps res2 (2, 16, 12, 20), res3 (.., 6, 10), res4 (.., 3, 5), res5 (.., 2, 3); weights synthetic.synth_state_dict(salt = seed), inputs
and the linear functional of the three outputs regenerated from the same seed.  Only data is stored:
    seed, margins (sampling-coordinate distance to an integer in pixels, smallest |pre-ReLU value|, largest fp32 fraction of the contract)
    out__mask_features (every 4th channel: the full map would take the file past the size limit for committed files), out__ms0..2
    g_in__res2..res5, g__<parameter name>      float64 autograd results, stored rounded to fp32
    err32__<the same keys>                     max |reference fp32 CPU run - float64| per tensor
The seed is searched until (1) no sampling coordinate of any encoder layer lies within 1e-4 px of an integer (the kinks of the
bilinear gradient; counted for the samples that can touch the map, both coordinates inside [-1, size]: the others read zero padding in a
whole neighbourhood, and with them ~60 000 coordinates per case leave no seed), (2) no pre-ReLU value (the FFN's linear1, layer_1's GroupNorm) lies within 1e-5 of zero, (3) the reference's own
fp32 run stays within a quarter of the contract 1e-4 * max|ref64| on every tensor.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _ref_import as R  # noqa: E402
import pd_bwd_cases as K  # noqa: E402

torch.set_num_threads(8)
COORD_MARGIN, RELU_MARGIN = 1e-4, 1e-5


class _KeepDtype:
    """forward_features reads every feature map as ``features[f].float()`` (msdeformattn.py:320,344); the float64 run hands it this
    stand-in, whose float() is the double tensor itself."""

    def __init__(self, t):
        self.t = t

    def float(self):
        return self.t


def build(seed, dtype):
    MSD = R.ref("modeling.pixel_decoder.msdeformattn")
    SS = R._ShapeSpec
    shape = {k: SS(channels=c, stride=s) for k, c, s in zip(("res2", "res3", "res4", "res5"), K.PD_IN_CHANNELS, (4, 8, 16, 32))}
    pd = MSD.MSDeformAttnPixelDecoder(
        shape, transformer_dropout=0.0, transformer_nheads=8, transformer_dim_feedforward=K.PD_FFN,
        transformer_enc_layers=K.PD_ENC_LAYERS, conv_dim=K.PD_CONV_DIM, mask_dim=K.PD_MASK_DIM, norm="GN",
        transformer_in_features=["res3", "res4", "res5"], common_stride=4).eval()
    sd = K.pd_state_dict(seed)
    assert {k: tuple(v.shape) for k, v in pd.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    pd.load_state_dict(sd, strict=True)
    return pd.to(dtype)


def run(seed, dtype):
    """Outputs, gradients and the two margins of one run of the reference in ``dtype``."""
    pd = build(seed, dtype)
    mod = R.ref("modeling.pixel_decoder.ops.modules.ms_deform_attn")
    core = mod.ms_deform_attn_core_pytorch
    margins = {"coord": float("inf"), "relu": float("inf")}

    def recording_core(value, shapes, loc, aw):
        wh = torch.stack([shapes[:, 1], shapes[:, 0]], -1).to(loc.dtype)
        px = loc.detach() * wh[None, None, None, :, None, :] - 0.5                         # grid_sample, align_corners=False
        size = wh[None, None, None, :, None, :]
        # a sample outside (-1, W) x (-1, H) reads only padding, also everywhere near it: no kink there
        live = ((px >= -1 - COORD_MARGIN) & (px <= size + COORD_MARGIN)).all(-1, keepdim=True).expand_as(px)
        if live.any():
            margins["coord"] = min(margins["coord"], float((px - px.round()).abs()[live].min()))
        return core(value, shapes, loc, aw)

    def pre_relu(_m, _i, out):
        margins["relu"] = min(margins["relu"], float(out.detach().abs().min()))

    hooks = [layer.linear1.register_forward_hook(pre_relu) for layer in pd.transformer.encoder.layers]
    hooks.append(pd.layer_1.norm.register_forward_hook(pre_relu))
    mod.ms_deform_attn_core_pytorch = recording_core
    try:
        feats = {k: v.to(dtype).requires_grad_(True) for k, v in K.pd_features(seed).items()}
        mf, enc, ms = pd.forward_features({k: _KeepDtype(v) for k, v in feats.items()})
        K.pd_functional(mf, enc, ms, seed).backward()
    finally:
        mod.ms_deform_attn_core_pytorch = core
        for h in hooks:
            h.remove()
    arrs = {"out__mask_features": mf.detach()[:, ::K.PD_MF_STRIDE].contiguous()}
    arrs.update({f"out__ms{i}": t.detach() for i, t in enumerate(ms)})
    arrs.update({"g_in__" + k: v.grad for k, v in feats.items()})
    arrs.update({"g__" + n: p.grad for n, p in pd.named_parameters()})
    assert all(v is not None for v in arrs.values())
    return arrs, margins


def main():
    for seed in range(1, 100000):
        ref, margins = run(seed, torch.float64)
        if margins["coord"] <= COORD_MARGIN or margins["relu"] <= RELU_MARGIN:
            continue
        f32, _ = run(seed, torch.float32)
        err = {k: float((f32[k].double() - ref[k]).abs().max()) for k in ref}
        frac = {k: err[k] / (K.RTOL * float(ref[k].abs().max())) for k in ref}
        worst = max(frac, key=frac.get)
        print(f"seed {seed}: margins {margins}, worst fp32 fraction of the contract {frac[worst]:.3f} ({worst})")
        if frac[worst] > 0.25:
            continue
        out = {"seed": np.int64(seed),
               "margins": np.array([margins["coord"], margins["relu"], frac[worst]], dtype=np.float64)}
        for k, v in ref.items():
            out[k] = v.float().numpy()
            out["err32__" + k] = np.float64(err[k])
        path = os.path.join(HERE, "pixel_decoder_backward.npz")
        np.savez_compressed(path, **out)
        print(f"pixel_decoder_backward: seed {seed}, {len(ref)} tensors, {os.path.getsize(path) / 1024:.1f} KiB")
        return
    raise SystemExit("no seed met the three conditions")


if __name__ == "__main__":
    main()
