"""The branch from the res2 lateral to the mask features and the final mask step that reads them: the two-block form of
msm_mask_logits_fwd (launches that write the logits of <= 32 queries) and msm_groupnorm_nchw_pool_f32 (GroupNorm to NCHW planes
with the decoder's pooled centre-tap maps from the same pass).  Both must be bit-equal to what they replace -- the seven-block
mask kernel, and msm_groupnorm_apply_nchw_f32 followed by msm_pool_mask_taps -- which the library's options still select
(MASK_KERNEL = 7, GN_POOL = 0).  Float64 comparisons use the tolerances of the existing tests of the same ops
(test_gpu_ops.test_mask_logits_folded_form, the ``rule`` of test_gpu_norm).  Needs a real MI355X (pytest -m gpu)."""
import ctypes

import pytest
import torch

from oracle import msm_oracle as O
from unseenobjectswithmeanshift_amd import synthetic as syn

from test_gpu_norm import gn_t32, rule

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -12345.5


def ops():
    from unseenobjectswithmeanshift_amd import ops as _ops
    return _ops


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


# =============================================================================================
# A: the final mask step sized to its queries
# =============================================================================================
def mask_step_into(wide, f, rows_alloc):
    """msm_mask_logits_fwd as the decoder calls its final step -- embedding = the leading 64 columns of the 68-wide rows of
    ``wide`` (B, Q, 68), qbias = column 64, logits only -- writing into a flat buffer of B * Q + rows_alloc rows of H * W that was
    pre-filled with a sentinel.  Returns the whole buffer (B * Q + rows_alloc, H * W)."""
    from unseenobjectswithmeanshift_amd._lib import check, lib
    B, Q, ld = wide.shape
    _, C, H, W = f.shape
    buf = torch.full((B * Q + rows_alloc, H * W), SENTINEL, device=DEV)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + 4 * off)
    rc = lib().msm_mask_logits_fwd(p(wide), p(f), p(buf), None, None, B, Q, C, H, W, 0, 0, 0, ld, p(wide, 64), ld,
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    check(rc, "msm_mask_logits_fwd")
    return buf


MASK_MAPS = [(2, 16), (6, 32), (10, 48)]


@pytest.fixture(scope="module")
def mask_inputs():
    """Per map: features (2, 64, H, W), 33 embedding rows (2, 33, 68) and the float64 logits of all 33 -- computed once."""
    out = {}
    for H, W in MASK_MAPS:
        wide = rnd(2, 33, 68, seed=1, scale=0.3)
        f = rnd(2, 64, H, W, seed=2)
        ref = torch.einsum("bqc,bchw->bqhw", wide[..., :64].double(), f.double()) + wide[..., 64].double()[..., None, None]
        out[(H, W)] = (wide.to(DEV), f.to(DEV), ref)
    return out


@pytest.mark.parametrize("Q", [1, 15, 16, 17, 20, 32, 33])
@pytest.mark.parametrize("H,W", MASK_MAPS)
def test_final_mask_step_short_form(H, W, Q, mask_inputs, lib_option):
    """Q <= 32 takes the two-block kernel, Q = 33 the seven-block one.  (i) the rows are bit-equal to the first Q rows of the
    seven-block kernel's result for the same embeddings padded to 33 rows; (ii) they are the float64 einsum + bias within the
    tolerance of test_mask_logits_folded_form; (iii) the row after the last one keeps its sentinel."""
    B = 2
    wide33, f, ref33 = mask_inputs[(H, W)]
    wide = wide33[:, :Q].contiguous()                       # (B, Q, 68): rows as topk_class_scores gathers them
    seven = mask_step_into(wide33, f, 0).view(B, 33, H * W)[:, :Q]
    buf = mask_step_into(wide, f, 1)
    assert bool((buf[B * Q:] == SENTINEL).all()), "wrote past row Q"
    got = buf[:B * Q].view(B, Q, H * W)
    assert not bool((got == SENTINEL).any())
    assert torch.equal(got, seven)
    torch.testing.assert_close(got.cpu().view(B, Q, H, W), ref33[:, :Q].float(), rtol=1e-4, atol=1e-4)
    # the option keeps the seven-block kernel for every Q: the same bits
    lib_option("MASK_KERNEL", 7)
    assert torch.equal(mask_step_into(wide, f, 1), buf)


# =============================================================================================
# B: GroupNorm to NCHW planes + pooled centre taps in one launch
# =============================================================================================
POOL_CASES = [((8, 8), [(4, 4), (2, 2), (1, 1)]),
              ((16, 32), [(8, 16), (4, 8), (2, 4)]),
              ((24, 40), [(12, 20), (6, 10), (3, 5)]),         # 40 columns: a partial 16-column tile
              ((24, 40), [(12, 20)])]


@pytest.fixture(scope="module")
def gn_inputs():
    """Per map and ReLU: tokens, affine, moments on the device; the two-launch results; float64 and torch-fp32 definitions."""
    out = {}
    for H, W in sorted({hw for hw, _ in POOL_CASES}):
        x, g, b = rnd(2, H * W, 64, seed=1), 1 + 0.1 * rnd(64, seed=2), rnd(64, seed=3)
        xd, gd, bd = x.to(DEV), g.to(DEV), b.to(DEV)
        st = ops().groupnorm_stats(xd)
        for relu in (False, True):
            act = ops().groupnorm_nchw(xd, st, gd, bd, groups=32, relu=relu)
            ref = O.groupnorm_tokens(x, g, b, H, W, 32, relu=relu).transpose(1, 2)
            t32 = gn_t32(x, g, b, H, W, 32, relu=relu).transpose(1, 2)
            out[(H, W, relu)] = (xd, gd, bd, st, act, ref, t32)
    return out


@pytest.mark.parametrize("zero_rows", [0, 5, 100])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("hw,sizes", POOL_CASES)
def test_groupnorm_nchw_pool_equals_two_launches(hw, sizes, relu, zero_rows, gn_inputs):
    from unseenobjectswithmeanshift_amd._lib import check, lib
    H, W = hw
    B = 2
    xd, gd, bd, st, act2, ref, t32 = gn_inputs[(H, W, relu)]
    pooled2 = ops().pool_mask_taps(act2.view(B, 64, H, W), sizes)
    # the wrapper allocates its flag buffer: the raw entry point takes one pre-filled with ones
    y = torch.full((B, 64, H, W), SENTINEL, device=DEV)
    outs = [torch.full((B, th * tw, 64), SENTINEL, device=DEV) for th, tw in sizes]
    flags = torch.ones((B, max(zero_rows, 1)), device=DEV, dtype=torch.int32)
    n = len(sizes)
    ths = (ctypes.c_int32 * n)(*[s[0] for s in sizes])
    tws = (ctypes.c_int32 * n)(*[s[1] for s in sizes])
    ptrs = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib().msm_groupnorm_nchw_pool_f32(p(xd), p(st), p(gd), p(bd), p(y), B, H, W, 64, 32, 1e-5, 1 if relu else 0, n,
                                           ctypes.cast(ths, ctypes.c_void_p), ctypes.cast(tws, ctypes.c_void_p), ctypes.cast(ptrs, ctypes.c_void_p),
                                           p(flags) if zero_rows else None, B * zero_rows, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    check(rc, "msm_groupnorm_nchw_pool_f32")
    assert torch.equal(y.view(B, 64, H * W), act2)
    for o, o2 in zip(outs, pooled2):
        assert torch.equal(o, o2)
    if zero_rows:
        assert not bool(flags.any())
    else:
        assert bool((flags == 1).all())
    rule("groupnorm_nchw_pool", f"{H}x{W} sizes={sizes} relu={relu}", y.view(B, 64, H * W), ref, t32)
    # the wrapper: same results, a cleared (B, zero_rows) buffer
    ya, outs_a, fl = ops().groupnorm_nchw_pool(xd, st, gd, bd, H, W, sizes, groups=32, relu=relu, zero_rows=zero_rows)
    assert torch.equal(ya, y) and all(torch.equal(a, o) for a, o in zip(outs_a, outs))
    assert (fl is None) if not zero_rows else (tuple(fl.shape) == (B, zero_rows) and not bool(fl.any()))


def test_groupnorm_nchw_pool_rejects_bad_arguments():
    z = lambda *s, dt=torch.float32: torch.zeros(*s, device=DEV, dtype=dt)
    st = z(1, 64, 2, dt=torch.float64)
    with pytest.raises(RuntimeError):
        ops().groupnorm_nchw_pool(z(1, 36, 64), st, z(64), z(64), 6, 6, [(3, 3)])            # W % 4 != 0
    with pytest.raises(RuntimeError):
        ops().groupnorm_nchw_pool(z(1, 64, 64), st, z(64), z(64), 8, 8, [(8, 8)])            # reduction 1
    with pytest.raises(RuntimeError):
        ops().groupnorm_nchw_pool(z(1, 64, 32), z(1, 32, 2, dt=torch.float64), z(32), z(32), 8, 8, [(4, 4)])   # C != 64


# =============================================================================================
# The whole plan
# =============================================================================================
def test_inference_with_and_without_the_new_launches(lib_option):
    """model.inference (B = 1, the 64 x 96 frame of the suite's small cases: a 16 x 24 mask-feature map, levels 8 x 12, 4 x 6,
    2 x 3) with the fused pooling launch and the two-block final step is bit-equal to the same model with both switched off by
    their options, and graphs.GraphedInference on it is bit-equal to eager."""
    from unseenobjectswithmeanshift_amd.meta_arch import MeanShiftMaskFormer, build_resnet50_head
    from unseenobjectswithmeanshift_amd.modeling import FoldedMaskFeatures
    head = build_resnet50_head()
    head.pixel_decoder.load_state_dict(syn.synth_state_dict(syn.pixel_decoder_param_shapes()), strict=True)
    head.predictor.load_state_dict(syn.synth_state_dict(syn.decoder_param_shapes()), strict=True)
    model = MeanShiftMaskFormer(backbone=None, sem_seg_head=head.to(DEV).eval(), num_queries=100)
    feats = {k: v.to(DEV) for k, v in syn.synth_backbone_features(1, 64, 96, seed=3).items()}
    # the pixel decoder hands the pooled maps over when the predictor asks for them
    mf, _, ms = head.pixel_decoder.forward_features(feats, folded=True, pool_request=head.predictor.pool_request)
    assert isinstance(mf, FoldedMaskFeatures) and mf.pooled is not None
    assert mf.pooled[0] == [tuple(int(s) for s in m.shape[-2:]) for m in ms] and tuple(mf.pooled[2].shape) == (1, 100)
    assert head.pixel_decoder.forward_features(feats, folded=True)[0].pooled is None
    new = model.inference(feats, (64, 96))
    g = model.graphed()
    for a, b in zip(g(feats, (64, 96)), new):
        assert torch.equal(a, b)
    lib_option("GN_POOL", 0)
    lib_option("MASK_KERNEL", 7)
    old = model.inference(feats, (64, 96))
    assert len(old) == len(new)
    for a, b in zip(old, new):
        assert torch.equal(a, b)
