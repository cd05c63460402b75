"""Cases, seeded planted inputs and the float64 definition for the 3x3 convolution backward (training.conv3x3, csrc/conv3x3_bwd.hip;
helper, not collected).

Definition: torch.nn.functional.conv2d(x, w, bias, padding=1) on the CPU in float64 with ``.backward(g)``: y, dx, dw, db.
tests/test_conv_bwd_cases_cpu.py pins it to an independent nine-term restatement (shifted zero-padded slices + einsum) and checks
the structural zeros below; tests/test_gpu_conv_bwd.py holds the HIP path to it.

Planted inputs: x unit-normalised over its 64 channels (the embedding the head sees), w ~ N(0, 2/576), bias ~ 0.1 N(0, 1),
g ~ N(0, 1).  Case ``edges`` keeps x and g only in columns 0 and W - 1: every tap with dx != 1 is then structurally zero in dw, and a
kernel that lets the flattened pixel axis wrap from (y, W-1) to (y+1, 0) makes them non-zero.
"""
import collections
import functools

import torch
import torch.nn.functional as F

Case = collections.namedtuple("Case", "B H W Cout seed")

CASES = {
    "px1": Case(1, 1, 1, 64, 11),        # only the centre tap sees data
    "row": Case(1, 1, 7, 64, 12),        # no vertical neighbour, W % 4 != 0
    "col": Case(2, 9, 1, 64, 13),        # W = 1: every horizontal neighbour is padding; a row wrap reads the next row
    "edges": Case(2, 4, 8, 64, 14),      # data in columns 0 and W-1 only
    "odd": Case(3, 5, 13, 128, 15),      # 65 pixels per image: pixel ranges cross image boundaries
    "wide": Case(2, 6, 36, 256, 16),     # W % 4 == 0 (weight-stationary forward), a partial 16-pixel tile per row
    "tall": Case(1, 33, 20, 320, 17),    # Cout a multiple of 64, not a power of two; 660 pixels
}

SPLIT_CASES = ("odd", "wide", "tall")
RTOL = 1e-4                              # the fp32 contract: max|got - ref64| <= RTOL * max|ref64| per tensor


@functools.lru_cache(maxsize=None)
def planted(name):
    """(x (B, 64, H, W), w (Cout, 64, 3, 3), bias (Cout,), g (B, Cout, H, W)) fp32, seeded.  Shared: do not modify."""
    c = CASES[name]
    gen = torch.Generator().manual_seed(c.seed)
    x = F.normalize(torch.randn(c.B, 64, c.H, c.W, generator=gen, dtype=torch.float64), dim=1).float()
    w = (torch.randn(c.Cout, 64, 3, 3, generator=gen, dtype=torch.float64) * (2.0 / 576) ** 0.5).float()
    bias = (0.1 * torch.randn(c.Cout, generator=gen, dtype=torch.float64)).float()
    g = torch.randn(c.B, c.Cout, c.H, c.W, generator=gen, dtype=torch.float64).float()
    if name == "edges":
        keep = torch.zeros(c.W, dtype=torch.bool)
        keep[0] = keep[-1] = True
        x = x * keep
        g = g * keep
    return x, w, bias, g


@functools.lru_cache(maxsize=None)
def reference64(name):
    """{"y", "dx", "dw", "db"} float64 from CPU F.conv2d autograd on the planted inputs.  Shared: do not modify."""
    x, w, bias, g = (t.double() for t in planted(name))
    x.requires_grad_(True), w.requires_grad_(True), bias.requires_grad_(True)
    y = F.conv2d(x, w, bias, padding=1)
    y.backward(g)
    return {"y": y.detach(), "dx": x.grad, "dw": w.grad, "db": bias.grad}


def restatement64(name):
    """The same four tensors from nine shifted, zero-padded slices and einsum (no convolution routine, no autograd)."""
    x, w, bias, g = (t.double() for t in planted(name))
    B, _, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    gp = F.pad(g, (1, 1, 1, 1))
    y = bias.view(1, -1, 1, 1).expand(B, -1, H, W).clone()
    dx = torch.zeros_like(x)
    dw = torch.zeros_like(w)
    for dy in range(3):
        for dxx in range(3):
            xs = xp[:, :, dy:dy + H, dxx:dxx + W]                           # x[p + (dy-1, dx-1)]
            y += torch.einsum("oc,bchw->bohw", w[:, :, dy, dxx], xs)
            dw[:, :, dy, dxx] = torch.einsum("bohw,bchw->oc", g, xs)
            gs = gp[:, :, 2 - dy:2 - dy + H, 2 - dxx:2 - dxx + W]           # g[p - (dy-1, dx-1)]
            dx += torch.einsum("oc,bohw->bchw", w[:, :, dy, dxx], gs)
    return {"y": y, "dx": dx, "dw": dw, "db": g.sum((0, 2, 3))}


def structural_zero_taps(name):
    """Bool (3, 3): taps (dy, dx) of dw no pixel of the case can reach."""
    c = CASES[name]
    z = torch.zeros(3, 3, dtype=torch.bool)
    if c.H == 1:
        z[0] = z[2] = True
    if c.W == 1 or name == "edges":
        z[:, 0] = z[:, 2] = True
    return z


def tap_major(dw):
    """(Cout, 64, 3, 3) -> (Cout, 576), column (dy*3 + dx)*64 + c: the layout of the C entry points."""
    return dw.permute(0, 2, 3, 1).reshape(dw.shape[0], 576)


def check(name, what, got, ref, rtol=RTOL):
    """Print the figure, then assert the contract."""
    scale = float(ref.abs().max())
    err = float((got.detach().cpu().double() - ref).abs().max())
    print(f"conv3x3 backward case {name}: {what} max|d| {err:.3e} of max|ref| {scale:.3e} -> {err / scale if scale else err:.2e}")
    assert err <= rtol * scale, (name, what, err, scale)
