"""Cases, seeded planted inputs and the float64 definition for the backward of the UCN embedding tail (csrc/backbone_bwd.hip:
msm_ucn_embedding_tail_bwd; training.ucn_embedding_tail) -- helper, not collected.

Definition: CPU torch autograd in float64 of the literal expression -- F.interpolate(mode="bilinear", align_corners=True) of each
tower, +, F.normalize(p=2, dim=1, eps) applied ``norms`` times.  tests/test_ucn_tail_cases_cpu.py pins it to an independent
restatement (explicit interpolation matrices, the normalisation's adjoint written out); tests/test_gpu_ucn_tail_bwd.py holds the
HIP path to it.

Planted inputs: a = N(0, 1), b = 0.5 N(0, 1) as (B, 64, h, w) maps, gout = N(0, 1) as (B, 64, H, W).  ``dead`` zeroes both towers on
low-resolution rows and columns 1..2, so the output pixels between them have u = 0 exactly and take the g / eps branch.
"""
import collections
import functools

import torch
import torch.nn.functional as F

Case = collections.namedtuple("Case", "B h w H W towers norms")

CASES = {
    "x8": Case(2, 8, 12, 64, 96, 2, 1),         # two towers, one normalisation
    "x8n2": Case(2, 8, 12, 64, 96, 2, 2),       # two normalisations
    "odd": Case(3, 5, 7, 37, 51, 2, 2),         # odd sizes, B = 3
    "wide": Case(1, 3, 17, 9, 130, 1, 1),       # W not a multiple of 64, one tower
    "same": Case(1, 6, 5, 6, 5, 2, 0),          # identity size, no normalisation: gout transposed, bit for bit
    "row": Case(1, 1, 4, 8, 29, 2, 1),          # h == 1
    "col": Case(1, 4, 1, 29, 8, 1, 2),          # w == 1, one tower
    "down": Case(1, 9, 9, 4, 5, 2, 1),          # downsampling: some low-resolution pixels receive exactly zero
    "px1": Case(1, 2, 2, 1, 1, 2, 1),           # a single output pixel
    "up0": Case(2, 4, 6, 25, 41, 2, 0),         # upsampling without normalisation
    "dead": Case(1, 4, 5, 25, 33, 2, 1),        # u = 0 on a patch of output pixels: the clamp branch
}
C = 64
EPS = 1e-12
RTOL = 1e-4                                      # the fp32 contract: max|got - ref64| <= RTOL * max|ref64| per tensor


@functools.lru_cache(maxsize=None)
def planted(name):
    """(a, b or None, gout) fp32, seeded by the case's position.  Shared: do not modify."""
    c = CASES[name]
    gen = torch.Generator().manual_seed(4100 + list(CASES).index(name))
    a = torch.randn(c.B, C, c.h, c.w, generator=gen, dtype=torch.float64).float()
    b = (0.5 * torch.randn(c.B, C, c.h, c.w, generator=gen, dtype=torch.float64)).float()
    g = torch.randn(c.B, C, c.H, c.W, generator=gen, dtype=torch.float64).float()
    if name == "dead":
        for t in (a, b):
            t[:, :, 1:3, :] = 0
            t[:, :, :, 1:3] = 0
    return a, (b if c.towers == 2 else None), g


def expression(a, b, size, norms, eps=EPS):
    """The literal expression, in the dtype of its inputs."""
    u = F.interpolate(a, size=size, mode="bilinear", align_corners=True)
    if b is not None:
        u = u + F.interpolate(b, size=size, mode="bilinear", align_corners=True)
    for _ in range(norms):
        u = F.normalize(u, p=2, dim=1, eps=eps)
    return u


def _autograd(name, dtype):
    c = CASES[name]
    a, b, g = planted(name)
    a = a.to(dtype, copy=True).requires_grad_(True)                            # copies: the planted tensors stay leaves without grad
    b = None if b is None else b.to(dtype, copy=True).requires_grad_(True)
    y = expression(a, b, (c.H, c.W), c.norms)
    y.backward(g.to(dtype))
    return {"y": y.detach(), "ga": a.grad, "gb": None if b is None else b.grad}


@functools.lru_cache(maxsize=None)
def reference64(name):
    """{"y" (B, 64, H, W), "ga", "gb" (B, 64, h, w; gb None for one tower)} float64 from CPU autograd.  Shared: do not modify."""
    return _autograd(name, torch.float64)


def torch32(name):
    """The same from torch's own fp32 run on the CPU."""
    return _autograd(name, torch.float32)


def axis_matrix64(n_in, n_out):
    """(n_out, n_in) float64: one axis of the align_corners=True resize, entry by entry (source = dst (in - 1) / (out - 1), the upper
    neighbour clamped at the border)."""
    m = torch.zeros(n_out, n_in, dtype=torch.float64)
    scale = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
    for d in range(n_out):
        src = scale * d
        i0 = min(int(src), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        m[d, i0] += 1.0 - (src - i0)
        m[d, i1] += src - i0
    return m


def restatement64(name):
    """The same three tensors without F.interpolate, F.normalize or autograd: up(a) = Uy a Ux^T, the adjoint of
    N(v) = v / max(|v|, eps) written out ((g - y <y, g>) / |v| from eps on, g / eps below), gin = Uy^T g_u Ux."""
    c = CASES[name]
    a, b, g = (None if t is None else t.double() for t in planted(name))
    Uy, Ux = axis_matrix64(c.h, c.H), axis_matrix64(c.w, c.W)
    up = lambda t: torch.einsum("Yi,bcij,Xj->bcYX", Uy, t, Ux)
    v = up(a) if b is None else up(a) + up(b)
    chain = []
    for _ in range(c.norms):
        n = v.pow(2).sum(1, keepdim=True).sqrt()
        chain.append((v, n))
        v = v / n.clamp_min(EPS)
    y = v
    for v, n in reversed(chain):
        unit = v / n.clamp_min(EPS)
        g = torch.where(n >= EPS, (g - unit * (unit * g).sum(1, keepdim=True)) / n.clamp_min(EPS), g / EPS)
    gin = torch.einsum("Yi,bcYX,Xj->bcij", Uy, g, Ux)
    return {"y": y, "ga": gin, "gb": None if b is None else gin}


def zero_gradient_pixels(name):
    """Boolean (h, w): the low-resolution pixels that no output pixel's taps reach with a non-zero weight."""
    c = CASES[name]
    Uy, Ux = axis_matrix64(c.h, c.H), axis_matrix64(c.w, c.W)
    return ~((Uy > 0).any(0)[:, None] & (Ux > 0).any(0)[None, :])


def check(name, what, got, ref, rtol=RTOL):
    """Print the figure, then assert the contract.  Returns the fraction err / max|ref|."""
    scale = float(ref.abs().max())
    err = float((got.detach().cpu().double() - ref).abs().max())
    frac = err / scale if scale else err
    print(f"ucn tail case {name}: {what} max|d| {err:.3e} of max|ref| {scale:.3e} -> {frac:.2e}")
    assert err <= rtol * scale, (name, what, err, scale)
    return frac
