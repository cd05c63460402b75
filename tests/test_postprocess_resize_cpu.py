"""Instance masks at a requested output size (msm_instance_postprocess_resized): the host side, and the yardstick the GPU
tests of tests/test_gpu_postprocess_resize.py share -- the reference's own chain in torch on the CPU.

The reference brings the low-res mask logits to an image in two interpolations (pretrained_meanshiftformer_model.py:337-343,
then detectron2's sem_seg_postprocess, :354-357, which is a crop plus ``F.interpolate(size=(height, width), mode="bilinear",
align_corners=False)``); detectron2 is not a dependency, so ``chain`` restates those two lines.

Acceptance rule for masks.  r32 = chain in float32, r64 = chain in float64, tau = 16 * max|r32 - r64| per case: the distance the
reference keeps from its own definition, times 16 for a kernel that contracts the same formulas into FMAs and rounds its tap weights
on its own.  tau is measured on the reference alone.  A pixel is uncertain when |r64| < tau; everywhere else a mask must equal
r64 > 0 exactly, and at most 1e-3 of a case's pixels may be uncertain (checked here, before any kernel is looked at)."""
import ctypes
import functools
import re

import torch
import torch.nn.functional as F

from oracle import msm_oracle as O
from unseenobjectswithmeanshift_amd import _lib

B, Q, T = 2, 100, 20
UNCERTAIN_CAP = 1e-3

# low-res map -> padded frame -> image (the crop) -> output
CASES = {
    "down1.5_crop_oddw": ((30, 40), (120, 160), (113, 153), (75, 101)),      # scalar stores
    "up2_crop": ((30, 40), (120, 160), (113, 153), (226, 306)),
    "up3.3_crop": ((30, 40), (120, 160), (113, 153), (374, 505)),            # last rows / columns clamp at the crop edge; two column tiles
    "down3_vec": ((30, 40), (120, 160), (120, 160), (40, 52)),               # OW % 4 == 0
    "down17": ((30, 40), (120, 160), (120, 160), (7, 9)),
    "to1x1": ((30, 40), (120, 160), (113, 153), (1, 1)),
    "frame_not_4x": ((25, 33), (96, 128), (90, 125), (61, 84)),
    "up4_tiles": ((30, 40), (120, 160), (120, 160), (480, 640)),             # 30 strips of 160 four-pixel threads
    # one strip whose cropped-image tile (the whole 256 x 640 image) is beyond the kernel's LDS budget of 12288 floats: every tap loaded directly
    "down32_direct": ((64, 160), (256, 640), (256, 640), (8, 20)),
}


def chain(low, frame, image, out, dtype):
    u = F.interpolate(low.to(dtype)[None], size=frame, mode="bilinear", align_corners=False)[..., :image[0], :image[1]]
    return F.interpolate(u, size=out, mode="bilinear", align_corners=False)[0]


def mask_rule(r32, r64):
    """(tau, uncertain) of the acceptance rule; r32 / r64 any shape."""
    tau = 16.0 * float((r32.double() - r64).abs().max())
    return tau, r64.abs() < tau


def reference_scores(r32):
    """(N, OH, OW) fp32 logits -> the reference's mask score (PM:494)."""
    binm = (r32 > 0).float()
    return (r32.sigmoid().flatten(1) * binm.flatten(1)).sum(1) / (binm.flatten(1).sum(1) + 1e-6)


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """Seeded inputs of a case and the chain on them, computed once per session: low (B,Q,h,w) = 2 * randn with map (0, 5) set
    to -1 (an empty mask), qidx (B,T) int32 (T distinct queries per image, (0, 0) = 5), r32 / r64 (B,T,OH,OW), tau, uncertain."""
    (h, w), frame, image, out = CASES[name]
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    low = 2.0 * torch.randn(B, Q, h, w, generator=g)
    low[0, 5] = -1.0
    qidx = torch.stack([torch.randperm(Q, generator=g)[:T] for _ in range(B)]).to(torch.int32)
    qidx[0, 0] = 5
    sel = torch.stack([low[b][qidx[b].long()] for b in range(B)])
    r32 = torch.stack([chain(sel[b], frame, image, out, torch.float32) for b in range(B)])
    r64 = torch.stack([chain(sel[b], frame, image, out, torch.float64) for b in range(B)])
    tau, uncertain = mask_rule(r32, r64)
    return {"low": low, "qidx": qidx, "sel": sel, "r32": r32, "r64": r64, "tau": tau, "uncertain": uncertain,
            "frame": frame, "image": image, "out": out}


def test_header_declares_and_bindings_bind_the_entry():
    assert "msm_instance_postprocess_resized" in _lib.declared_symbols()
    res, args = _lib._SIGNATURES["msm_instance_postprocess_resized"]
    assert res is ctypes.c_int and len(args) == 19          # 6 pointers, B Q T h w H W Hs Ws OH OW, workspace, stream
    assert len(args) == len(_lib._SIGNATURES["msm_instance_postprocess"][1]) + 2
    with open(_lib.HEADER_PATH) as f:
        src = f.read()
    assert int(re.search(r"#define\s+MSM_ABI_VERSION\s+(\d+)", src).group(1)) == _lib.ABI_VERSION
    assert re.search(r"int\s+msm_instance_postprocess_resized\([^;]*int OH, int OW,\s*float\* workspace, void\* stream\);", src)
    assert "POST_RESIZE_DIRECT" in _lib.OPTIONS and src.count("MSM_OPT_POST_RESIZE_DIRECT") >= 1


def test_entry_checks_its_arguments_without_a_gpu():
    L = _lib.lib()
    p = ctypes.c_void_p(16)
    ok = (2, 100, 20, 30, 40, 113, 153, 120, 160)
    assert L.msm_instance_postprocess_resized(p, p, None, p, p, p, *ok, 0, 5, p, None) == -1
    assert b"bad output size" in L.msm_last_error_string()
    assert L.msm_instance_postprocess_resized(p, p, None, p, p, p, *ok, 5, -1, p, None) == -1
    assert L.msm_instance_postprocess_resized(p, p, None, p, p, p, 2, 100, 20, 30, 40, 121, 153, 120, 160, 5, 5, p, None) == -1
    assert b"smaller than the image" in L.msm_last_error_string()
    assert L.msm_instance_postprocess_resized(p, p, None, None, p, p, *ok, 5, 5, p, None) == -1
    assert b"null pointer" in L.msm_last_error_string()


def test_chain_at_the_image_size_is_the_oracles_upsample_and_crop():
    """The second interpolation at out == image is the identity (scale 1: every source coordinate is its own index, the upper
    tap's weight 0), so the chain reduces to what oracle.instance_inference thresholds."""
    g = torch.Generator().manual_seed(7)
    logits, low = torch.randn(Q, 3, generator=g), 2.0 * torch.randn(Q, 30, 40, generator=g)
    for frame, image in (((120, 160), (120, 160)), ((120, 160), (113, 153))):
        ref = O.instance_inference(logits, low, image, topk=T, padded_size=frame)
        r = chain(low[ref["query_index"]], frame, image, image, torch.float32)
        up = F.interpolate(low[None], size=frame, mode="bilinear", align_corners=False)[0][:, :image[0], :image[1]]
        assert torch.equal(r, up[ref["query_index"]])
        assert torch.equal((r > 0).float(), ref["pred_masks"])
        cls = torch.softmax(logits, -1)[:, :-1].flatten()[O.canonical_topk(torch.softmax(logits, -1)[:, :-1].flatten(), T)]
        assert torch.equal(cls * reference_scores(r), ref["scores"])


def test_uncertain_share_of_the_reference_is_capped_on_every_gpu_case():
    for name in CASES:
        c = case_reference(name)
        share = float(c["uncertain"].float().mean())
        print(f"{name}: tau = {c['tau']:.3e}, uncertain share = {share:.3e}")
        assert 0.0 < c["tau"] < 1e-3, (name, c["tau"])
        assert share <= UNCERTAIN_CAP, f"{name}: tau = {c['tau']:.3e}, uncertain share {share:.3e}"
        assert not bool(c["uncertain"][0, 0].any()) and bool((c["r64"][0, 0] < -0.5).all())      # the empty mask


def test_two_stages_are_not_one_resize():
    """A single (h, w) -> (OH, OW) interpolation is another function: its sign differs from the chain's on a large share of pixels."""
    c = case_reference("down1.5_crop_oddw")
    single = torch.stack([F.interpolate(c["sel"][b][None], size=c["out"], mode="bilinear", align_corners=False)[0] for b in range(B)])
    assert float(((single > 0) != (c["r64"] > 0)).float().mean()) > 0.10


def test_group_by_size_groups_in_order_and_inverts():
    from unseenobjectswithmeanshift_amd.meta_arch import group_by_size
    a, b, c = ((60, 90), (120, 180)), ((64, 96), (64, 96)), ((50, 70), (30, 42))
    sizes = [a, b, a, c, b, a]
    groups, inverse = group_by_size(sizes)
    assert groups == [(a, [0, 2, 5]), (b, [1, 4]), (c, [3])]
    flat = [i for _, members in groups for i in members]
    assert [flat[j] for j in inverse] == list(range(len(sizes)))
    assert inverse == [0, 3, 1, 5, 4, 2]
    assert group_by_size([a]) == ([(a, [0])], [0])
    assert group_by_size([]) == ([], [])
