"""Cases, seeded planted inputs and float64 definitions for the two pixel-decoder backward kernels (csrc/norm_bwd.hip:
msm_groupnorm_bwd_f32, msm_upsample_bilinear_bwd_tokens_f32) and the fixed functional of the pixel-decoder golden case (helper,
not collected).

Definitions: CPU torch autograd in float64 -- F.group_norm (+ ReLU) on the planes form of the token map, F.interpolate(mode="bilinear",
align_corners=False).  tests/test_pd_bwd_cases_cpu.py pins them to independent restatements (the closed GroupNorm-backward formula
written out with sums; the upsampling matrix built entry by entry and transposed); tests/test_gpu_groupnorm_bwd.py and
tests/test_gpu_upsample_bwd.py hold the HIP path to them.

Planted GroupNorm inputs: x = N(0, 1) + 0.5, gamma = 1 + 0.1 N, beta = 0.1 N, g = N(0, 1); the seeds are chosen so that no pre-ReLU
value lies within 1e-5 of zero (asserted in ``gn_reference64``), so the ReLU mask of an fp32 forward cannot differ from the float64 one.
"""
import collections
import functools

import torch
import torch.nn.functional as F

GnCase = collections.namedtuple("GnCase", "B HW C groups relu seed")

GN_CASES = {
    "px1": GnCase(1, 1, 64, 32, False, 21),      # a group's two channels are all the data: dx is what eps leaves of a full cancellation
    "row": GnCase(2, 7, 64, 32, True, 22),
    "odd": GnCase(3, 65, 64, 32, True, 23),      # 65 pixels per image: ranges of unequal length, the last one short
    "wide4": GnCase(2, 36, 128, 32, False, 24),  # four channels per group
    "c256": GnCase(1, 33, 256, 32, True, 25),    # the widest map: a pixel is a whole 256-thread row
    "tall": GnCase(1, 660, 64, 32, True, 26),    # three ranges by the library's own choice
}
GN_SPLIT_CASES = ("odd", "tall")
GN_SPLITS = (1, 3, 7)
EPS = 1e-5
RELU_MARGIN = 1e-5

UpCase = collections.namedtuple("UpCase", "h w H W seed")
UP_B, UP_C = 2, 64
UP_CASES = {
    "x2": UpCase(2, 3, 4, 6, 31),
    "odd": UpCase(2, 3, 5, 7, 32),               # not an integer ratio
    "one": UpCase(1, 1, 3, 4, 33),               # every tap clamps to the single source pixel
    "row": UpCase(1, 5, 1, 10, 34),
    "res3": UpCase(15, 20, 30, 40, 35),          # the FPN step of a 120 x 160 frame
    "same": UpCase(3, 4, 3, 4, 36),              # identity
}

RTOL = 1e-4                                      # the fp32 contract: max|got - ref64| <= RTOL * max|ref64| per tensor


@functools.lru_cache(maxsize=None)
def gn_planted(name):
    """(x (B, HW, C), gamma (C,), beta (C,), g (B, HW, C)) fp32, seeded.  Shared: do not modify."""
    c = GN_CASES[name]
    gen = torch.Generator().manual_seed(c.seed)
    x = (torch.randn(c.B, c.HW, c.C, generator=gen, dtype=torch.float64) + 0.5).float()
    gamma = (1.0 + 0.1 * torch.randn(c.C, generator=gen, dtype=torch.float64)).float()
    beta = (0.1 * torch.randn(c.C, generator=gen, dtype=torch.float64)).float()
    g = torch.randn(c.B, c.HW, c.C, generator=gen, dtype=torch.float64).float()
    return x, gamma, beta, g


@functools.lru_cache(maxsize=None)
def gn_reference64(name):
    """{"y", "dx", "dgamma", "dbeta"} float64 (token layout) from CPU F.group_norm autograd on the planted inputs, and "margin": the
    smallest |pre-ReLU value|.  Shared: do not modify."""
    c = GN_CASES[name]
    x, gamma, beta, g = (t.double() for t in gn_planted(name))
    x.requires_grad_(True), gamma.requires_grad_(True), beta.requires_grad_(True)
    pre = F.group_norm(x.transpose(1, 2), c.groups, gamma, beta, EPS).transpose(1, 2)
    margin = float(pre.detach().abs().min())
    if c.relu:
        assert margin > RELU_MARGIN, (name, margin)
    y = F.relu(pre) if c.relu else pre
    y.backward(g)
    return {"y": y.detach(), "dx": x.grad, "dgamma": gamma.grad, "dbeta": beta.grad, "margin": margin}


def gn_restatement64(name):
    """The same four tensors from the closed formula written out with sums (no normalisation routine, no autograd):
    dx = rstd * (gamma g - (a + xh b) / n), a = sum_group gamma sum_p g, b = sum_group gamma sum_p g xh."""
    c = GN_CASES[name]
    x, gamma, beta, g = (t.double() for t in gn_planted(name))
    cpg = c.C // c.groups
    n = cpg * c.HW
    xg = x.view(c.B, c.HW, c.groups, cpg)
    mean = xg.sum((1, 3), keepdim=True) / n
    var = ((xg - mean) ** 2).sum((1, 3), keepdim=True) / n
    rstd = 1.0 / torch.sqrt(var + EPS)
    xh = ((xg - mean) * rstd).view(c.B, c.HW, c.C)
    y = xh * gamma + beta
    if c.relu:
        g = g * (y > 0)
        y = y.clamp_min(0)
    s1, s2 = g.sum(1), (g * xh).sum(1)                                       # (B, C)
    a = (gamma * s1).view(c.B, c.groups, cpg).sum(2, keepdim=True).expand(-1, -1, cpg).reshape(c.B, 1, c.C)
    b = (gamma * s2).view(c.B, c.groups, cpg).sum(2, keepdim=True).expand(-1, -1, cpg).reshape(c.B, 1, c.C)
    rs = rstd.expand(-1, 1, -1, cpg).reshape(c.B, 1, c.C)
    dx = rs * (gamma * g - (a + xh * b) / n)
    return {"y": y, "dx": dx, "dgamma": s2.sum(0), "dbeta": s1.sum(0)}


@functools.lru_cache(maxsize=None)
def up_planted(name):
    """(x (B, h*w, C), g (B, H*W, C)) fp32, seeded.  Shared: do not modify."""
    c = UP_CASES[name]
    gen = torch.Generator().manual_seed(c.seed)
    x = torch.randn(UP_B, c.h * c.w, UP_C, generator=gen, dtype=torch.float64).float()
    g = torch.randn(UP_B, c.H * c.W, UP_C, generator=gen, dtype=torch.float64).float()
    return x, g


@functools.lru_cache(maxsize=None)
def up_reference64(name):
    """{"y" (B, H*W, C), "dx" (B, h*w, C)} float64 from CPU F.interpolate autograd.  Shared: do not modify."""
    c = UP_CASES[name]
    x, g = (t.double() for t in up_planted(name))
    x.requires_grad_(True)
    planes = x.transpose(1, 2).reshape(UP_B, UP_C, c.h, c.w)
    y = F.interpolate(planes, size=(c.H, c.W), mode="bilinear", align_corners=False).reshape(UP_B, UP_C, c.H * c.W).transpose(1, 2)
    y.backward(g)
    return {"y": y.detach(), "dx": x.grad}


def up_matrix64(n_in, n_out):
    """(n_out, n_in) float64: one axis of the resize, entry by entry (source index scale * (dst + 0.5) - 0.5 clamped at 0, the upper
    neighbour clamped at the border)."""
    m = torch.zeros(n_out, n_in, dtype=torch.float64)
    for d in range(n_out):
        src = max(n_in / n_out * (d + 0.5) - 0.5, 0.0)
        i0 = int(src)
        i1 = min(i0 + 1, n_in - 1)
        m[d, i0] += 1.0 - (src - i0)
        m[d, i1] += src - i0
    return m


def up_restatement64(name):
    """The same two tensors from the explicit (H*W, h*w) matrix and its transpose."""
    c = UP_CASES[name]
    x, g = (t.double() for t in up_planted(name))
    m = torch.kron(up_matrix64(c.h, c.H), up_matrix64(c.w, c.W))             # row Y*W + X, column y*w + x
    return {"y": torch.einsum("pq,bqc->bpc", m, x), "dx": torch.einsum("pq,bpc->bqc", m, g)}


def check(kind, name, what, got, ref, rtol=RTOL):
    """Print the figure, then assert the contract.  Returns the fraction err / max|ref|."""
    scale = float(ref.abs().max())
    err = float((got.detach().cpu().double() - ref).abs().max())
    frac = err / scale if scale else err
    print(f"{kind} case {name}: {what} max|d| {err:.3e} of max|ref| {scale:.3e} -> {frac:.2e}")
    assert err <= rtol * scale, (kind, name, what, err, scale)
    return frac


# ---------------------------------------------------------------------------------------------------------------------------
# the pixel-decoder golden case (tests/golden/pixel_decoder_backward.npz, made by tests/golden/make_golden_pixel_decoder_backward.py)
PD_IN_CHANNELS = (16, 24, 32, 48)
PD_SIZES = {"res2": (12, 20), "res3": (6, 10), "res4": (3, 5), "res5": (2, 3)}     # no exact 2x everywhere, odd sizes
PD_BATCH = 2
PD_CONV_DIM, PD_MASK_DIM, PD_ENC_LAYERS, PD_FFN = 64, 256, 2, 128
PD_MF_STRIDE = 4                                 # mask_features is stored at every 4th channel (the file's size)


def pd_param_shapes():
    from unseenobjectswithmeanshift_amd import synthetic as syn
    return syn.pixel_decoder_param_shapes(in_channels=PD_IN_CHANNELS, conv_dim=PD_CONV_DIM, mask_dim=PD_MASK_DIM,
                                          enc_layers=PD_ENC_LAYERS, d_ffn=PD_FFN)


def pd_state_dict(seed):
    from unseenobjectswithmeanshift_amd import synthetic as syn
    return syn.synth_state_dict(pd_param_shapes(), salt=int(seed))


def pd_features(seed):
    """{"res2".."res5": (2, C_l, H_l, W_l)} fp32: N(0, 1), seeded."""
    gen = torch.Generator().manual_seed(7000 + int(seed))
    return {k: torch.randn(PD_BATCH, c, *PD_SIZES[k], generator=gen) for k, c in zip(("res2", "res3", "res4", "res5"), PD_IN_CHANNELS)}


def pd_functional(mask_features, enc_features, multi_scale, seed):
    """A fixed random linear functional of the three outputs of forward_features (float64 weights N(0, 1) / sqrt(H W), regenerated from
    the seed): the scalar whose gradients the fixture holds."""
    gen = torch.Generator().manual_seed(9000 + int(seed))
    loss = 0.0
    for t in [mask_features, enc_features] + list(multi_scale):
        wgt = torch.randn(tuple(t.shape), generator=gen, dtype=torch.float64) / (t.shape[-2] * t.shape[-1]) ** 0.5
        loss = loss + (t.double() * wgt.to(t.device)).sum()
    return loss
