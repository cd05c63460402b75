"""csrc/norm.hip against float64 definitions (oracle/msm_oracle.py: layernorm_chain, groupnorm_tokens, position_embedding_sine).

THE RULE of every fp32 comparison in this file (``rule`` below): on one input compute the float64 definition ``ref``,
torch's own fp32 implementation of the operation on the CPU ``t32`` (the arithmetic the reference model runs) and the kernel
result ``got``, and assert

    max|got - ref| <= max(4 * max|t32 - ref|, 4 * eps_fp32 * max|ref|)

over ALL elements.  The yardstick is torch's error, never the kernel's: the factor 4 covers a different fp32 summation order
(wave butterfly against torch's sequential / vectorised sums) and one more rounding (rstd * gamma); the second term is a floor
for inputs on which torch happens to be exact (constant rows).  No tolerance is chosen per case.  Every case prints both errors
(pytest -s); the worst ratios are recorded in DESIGN.md section 4b.  Needs a real MI355X (pytest -m gpu)."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import msm_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS32 = float(torch.finfo(torch.float32).eps)
SENTINEL = -12345.5


def ops():
    from unseenobjectswithmeanshift_amd import ops as _ops
    return _ops


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def dev(t):
    return None if t is None else t.to(DEV)


def rule(kernel, case, got, ref, t32):
    got = got.detach().cpu().double()
    assert got.shape == ref.shape == t32.shape, (got.shape, ref.shape, t32.shape)
    assert bool(torch.isfinite(got).all())
    e_k = float((got - ref).abs().max())
    e_t = float((t32.double() - ref).abs().max())
    bound = max(4.0 * e_t, 4.0 * EPS32 * float(ref.abs().max()))
    ratio = e_k / e_t if e_t > 0 else (0.0 if e_k == 0 else float("inf"))
    print(f"RULE [{kernel}] {case}: kernel {e_k:.3e} torch-fp32 {e_t:.3e} ratio {ratio:.2f} bound {bound:.3e}")
    assert e_k <= bound, f"{kernel} {case}: max|got - ref| = {e_k:.3e} > {bound:.3e} (torch fp32: {e_t:.3e})"


# =============================================================================================
# LayerNorm
# =============================================================================================
def ln_params(E, seed=10):
    return 1 + 0.1 * rnd(E, seed=seed), rnd(E, seed=seed + 1), 1 + 0.1 * rnd(E, seed=seed + 2), rnd(E, seed=seed + 3)


def ln_t32(x, parts, bias, g1, b1, l2norm, g2, b2, eps):
    """torch's fp32 arithmetic for the chain."""
    v = x if x is not None else torch.zeros_like(parts[0])
    if parts is not None:
        v = v + parts.sum(0)
    if bias is not None:
        v = v + bias
    y = F.layer_norm(v, (v.shape[-1],), g1, b1, eps)
    if l2norm:
        y = F.normalize(y, p=2, dim=-1, eps=1e-12)
    return y, (F.layer_norm(y, (y.shape[-1],), g2, b2, eps) if g2 is not None else None)


def ln_check(case, x, parts, bias, g1, b1, l2norm=False, g2=None, b2=None, eps=1e-5):
    ref, ref2 = O.layernorm_chain(x, parts, bias, g1, b1, l2norm, g2, b2, eps)
    t, t2 = ln_t32(x, parts, bias, g1, b1, l2norm, g2, b2, eps)
    got = ops().layernorm(dev(x), dev(g1), dev(b1), parts=dev(parts), bias=dev(bias), l2norm=l2norm, g2=dev(g2), b2=dev(b2), eps=eps)
    got, got2 = got if g2 is not None else (got, None)
    rule("layernorm", case, got, ref, t)
    if g2 is not None:
        rule("layernorm", case + " second norm", got2, ref2, t2)
    return got, got2


@pytest.mark.parametrize("rows", [1, 3, 37, 300, 1001])
@pytest.mark.parametrize("E", [64, 128, 256, 512])
def test_layernorm_plain(E, rows):
    g1, b1, _, _ = ln_params(E)
    ln_check(f"plain E={E} rows={rows}", rnd(rows, E, seed=1), None, None, g1, b1)


@pytest.mark.parametrize("rows", [37, 1001])
@pytest.mark.parametrize("E", [128, 512])
@pytest.mark.parametrize("form", ["parts1", "parts8", "xnone", "l2", "l2_second", "eps1e-3"])
def test_layernorm_forms(form, E, rows):
    g1, b1, g2, b2 = ln_params(E)
    x, bias = rnd(rows, E, seed=1), rnd(E, seed=2)
    case = f"{form} E={E} rows={rows}"
    if form == "parts1":
        ln_check(case, x, rnd(1, rows, E, seed=3), bias, g1, b1)
    elif form == "parts8":
        ln_check(case, x, rnd(8, rows, E, seed=3), bias, g1, b1)
    elif form == "xnone":
        ln_check(case, None, rnd(3, rows, E, seed=3), None, g1, b1)
    elif form == "eps1e-3":
        ln_check(case, x, None, None, g1, b1, eps=1e-3)
    else:
        second = form == "l2_second"
        y, _ = ln_check(case, x, rnd(2, rows, E, seed=3), bias, g1, b1, True, g2 if second else None, b2 if second else None)
        # the definition: every output row is an fp32 unit vector
        assert float((y.double().norm(dim=-1) - 1).abs().max()) <= 1e-6


@pytest.mark.parametrize("E", [64, 128, 256, 512])
def test_layernorm_value_cases(E):
    g1, b1, g2, b2 = ln_params(E)
    # rows far from zero: mean 1e3, unit spread
    ln_check(f"shifted E={E}", rnd(37, E, seed=1) + 1e3, None, None, g1, b1)
    # constant rows: zero variance, the result is b1
    consts = torch.tensor([0.7, -3.25, 1000.0, 1.0 / 3.0, 0.0])
    x = consts[:, None].expand(5, E).contiguous()
    y, _ = ln_check(f"constant rows E={E}", x, None, None, g1, b1)
    print(f"constant rows E={E}: max|y - b1| = {float((y.cpu().double() - b1.double()).abs().max()):.3e}")
    # g1 = 0, b1 = 0 -> a zero vector into the L2 step: exactly 0 (0 / max(0, 1e-12)), never NaN
    z = torch.zeros(E)
    y, y2 = ln_check(f"zero vector into l2 E={E}", rnd(37, E, seed=2), None, None, z, z, True, g2, b2)
    assert torch.equal(y.cpu(), torch.zeros(37, E)) and bool(torch.isfinite(y2).all())
    # the max(norm, 1e-12) clamp active: |LN| ~ 1e-14, so the norm (~1e-13) is below the clamp and y = LN / 1e-12
    y, _ = ln_check(f"l2 clamp E={E}", rnd(37, E, seed=3), None, None, 1e-14 * g1, z, True)
    assert 1e-3 < float(y.abs().max()) < 0.2


@pytest.mark.parametrize("rows", [1, 3, 37, 1001])
@pytest.mark.parametrize("E", [64, 512])
def test_layernorm_writes_only_its_rows(E, rows):
    """Four rows share a workgroup and ``row >= rows`` is the only guard: y and y2 sit inside sentinel-filled buffers."""
    from unseenobjectswithmeanshift_amd._lib import check, lib
    g1, b1, g2, b2 = [dev(t) for t in ln_params(E)]
    x = dev(rnd(rows, E, seed=1))
    pad = 8 * E
    bufs = [torch.full((rows * E + 2 * pad,), SENTINEL, device=DEV) for _ in range(2)]
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + 4 * off)
    rc = lib().msm_layernorm_f32(p(x), None, 0, rows * E, None, p(g1), p(b1), 1, p(g2), p(b2), p(bufs[0], pad), p(bufs[1], pad),
                                 rows, E, 1e-5, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    check(rc, "msm_layernorm_f32")
    y, y2 = ops().layernorm(x, g1, b1, l2norm=True, g2=g2, b2=b2)
    for buf, want in zip(bufs, (y, y2)):
        assert torch.equal(buf[pad:pad + rows * E].view(rows, E), want)
        assert bool((buf[:pad] == SENTINEL).all()) and bool((buf[pad + rows * E:] == SENTINEL).all())


def test_layernorm_rejects_other_widths():
    with pytest.raises(RuntimeError):
        ops().layernorm(torch.zeros(4, 96, device=DEV), torch.ones(96, device=DEV), torch.zeros(96, device=DEV))


# =============================================================================================
# GroupNorm: moments + token-major apply
# =============================================================================================
def to_nchw(tok, H, W):
    # contiguous NCHW, the layout the reference model normalises (a strided view would send torch down its channels-last path)
    return tok.transpose(1, 2).reshape(tok.shape[0], tok.shape[2], H, W).contiguous()


def to_tok(x):
    return x.flatten(2).transpose(1, 2)


def gn_t32(x, g, b, H, W, groups, eps=1e-5, up=None, up_hw=None, relu=False):
    """torch's fp32 arithmetic: F.group_norm [+ F.interpolate] [relu] on the NCHW form.  torch.group_norm is the function
    F.group_norm ends in; the wrapper only adds a training-time refusal of one value per group, which the 1x1 maps would meet."""
    y = torch.group_norm(to_nchw(x, H, W), groups, g, b, eps, False)
    if up is not None:
        y = y + F.interpolate(to_nchw(up, *up_hw), size=(H, W), mode="bilinear", align_corners=False)
    return to_tok(F.relu(y) if relu else y)


def gn_check(case, x, g, b, H, W, groups, up=None, up_hw=None, relu=False, up_dev=None, eps=1e-5, **kw):
    ref = O.groupnorm_tokens(x, g, b, H, W, groups, eps, up, up_hw, relu)
    t32 = gn_t32(x, g, b, H, W, groups, eps, up, up_hw, relu)
    if up is not None and up_dev is None:
        up_dev = dev(up)
    got = ops().groupnorm_tokens(dev(x), dev(g), dev(b), H, W, groups, up=up_dev, up_hw=up_hw, relu=relu, eps=eps, **kw)
    rule("groupnorm_tokens", case, got, ref, t32)
    return got


def moments_check(case, x, stats):
    """Raw moments against float64 sums.  Derivation of the bound: the kernel widens every value to double before it is added or
    squared, so its own error is n * 2^-53 * sum|x| -- far below anything fp32.  The bound 4 * eps_fp32 * sum|x| is the worst case
    (n - 1) * eps/2 * sum|x| of a recursive fp32 sum of n <= 9 terms: it admits an implementation that adds a handful of values in
    fp32 before widening and nothing longer (a 64-term fp32 run, the parent's for C = 256, has a worst case of 31.5 eps)."""
    xd = x.double()
    st = stats.cpu()
    for k, (name, v) in enumerate((("sum x", xd), ("sum x^2", xd * xd))):
        err = (st[..., k] - v.sum(1)).abs()
        bound = 4 * EPS32 * v.abs().sum(1)
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"MOMENTS [groupnorm_stats] {case} {name}: worst err / (4 eps sum|.|) = {worst:.3e}")
        assert bool((err <= bound).all()), f"{case} {name}: {worst:.3e} of the bound"


def groups_of(C):
    return sorted({1, C} | ({32} if C % 32 == 0 else set()))


GN_SHAPES = [  # every C at two sizes, every size at C = 64, B in {1, 3}
    (3, 4, 3, 5), (1, 4, 61, 67), (3, 32, 1, 1), (1, 32, 15, 20),
    (1, 64, 1, 1), (3, 64, 3, 5), (1, 64, 16, 24), (3, 64, 15, 20), (3, 64, 61, 67), (1, 64, 120, 160),
    (3, 128, 16, 24), (1, 128, 61, 67), (3, 256, 15, 20), (1, 256, 3, 5),
]


@pytest.mark.parametrize("B,C,H,W,groups", [s + (g,) for s in GN_SHAPES for g in groups_of(s[1])])
def test_groupnorm_shapes(B, C, H, W, groups):
    """(61, 67) leaves a ragged last 256-pixel run in the moments kernel; 120x160 at C = 64 is more than 1024 * 256 float4, so the
    grid-stride loop of the apply kernel takes a second step."""
    x, g, b = rnd(B, H * W, C, seed=1), 1 + 0.1 * rnd(C, seed=2), rnd(C, seed=3)
    case = f"B={B} C={C} {H}x{W} groups={groups}"
    moments_check(case, x, ops().groupnorm_stats(dev(x)))
    gn_check(case, x, g, b, H, W, groups)
    gn_check(case + " relu eps=1e-3", x, g, b, H, W, groups, relu=True, eps=1e-3)


def up_sources(H, W):
    return [((H + 1) // 2, (W + 1) // 2), (1, 1), (H, W), (H // 3, W // 3)]


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("H,W,uh,uw", [(H, W) + s for (H, W) in [(15, 20), (61, 67), (16, 24)] for s in up_sources(H, W)])
def test_groupnorm_upsample_add(H, W, uh, uw, relu):
    B, C = 2, 64
    x, g, b, up = rnd(B, H * W, C, seed=1), 1 + 0.1 * rnd(C, seed=2), rnd(C, seed=3), rnd(B, uh * uw, C, seed=4)
    gn_check(f"{H}x{W} up {uh}x{uw} relu={relu}", x, g, b, H, W, 32, up, (uh, uw), relu)


@pytest.mark.parametrize("H,W,uh,uw,C", [(15, 20, 8, 10, 64), (61, 67, 20, 22, 128), (3, 5, 1, 1, 4)])
def test_groupnorm_upsample_source_is_a_slice(H, W, uh, uw, C):
    """``up`` as a token range of a wider buffer: the batch stride exceeds uh * uw * C."""
    B = 3
    x, g, b, up = rnd(B, H * W, C, seed=1), 1 + 0.1 * rnd(C, seed=2), rnd(C, seed=3), rnd(B, uh * uw, C, seed=4)
    wide = torch.full((B, uh * uw + 7, C), float("nan"), device=DEV)
    wide[:, 3:3 + uh * uw] = dev(up)
    view = wide[:, 3:3 + uh * uw]
    assert view.stride(0) > uh * uw * C
    gn_check(f"{H}x{W} up {uh}x{uw} slice", x, g, b, H, W, groups_of(C)[-2] if C > 4 else 1, up, (uh, uw), True, up_dev=view)


COND = [(0.0, 2, 64, 16, 24), (30.0, 2, 64, 60, 80), (100.0, 2, 64, 60, 80), (300.0, 2, 64, 60, 80), (300.0, 1, 64, 120, 160),
        (30.0, 1, 256, 15, 20), (100.0, 1, 256, 15, 20), (300.0, 1, 256, 15, 20)]


@pytest.mark.parametrize("off,B,C,H,W", COND)
def test_groupnorm_conditioning(off, B, C, H, W):
    """Unit-variance maps shifted by ``off``: the mean is large against the spread, which is what a biased 1x1 convolution in
    front of a GroupNorm produces.  E[x^2] - E[x]^2 needs every bit of the raw moments: with fp32 per-thread sums in
    gn_stats_kernel (before it accumulated in double) every case with off >= 30 failed, at 8 to 326 times torch's fp32 error
    (measured on an MI355X); with double sums the same cases are at 0.24 to 0.45 times torch's error."""
    x, g, b = rnd(B, H * W, C, seed=1) + off, 1 + 0.1 * rnd(C, seed=2), rnd(C, seed=3)
    case = f"off={off:g} B={B} C={C} {H}x{W}"
    moments_check(case, x, ops().groupnorm_stats(dev(x)))
    gn_check(case, x, g, b, H, W, 32)


def test_groupnorm_moment_call_forms():
    g, b = dev(1 + 0.1 * rnd(64, seed=2)), dev(rnd(64, seed=3))
    # one moments workgroup per image (H*W <= 256): the order of the double additions is fixed, so bits are comparable
    for (B, H, W) in [(3, 3, 5), (2, 16, 16)]:
        x = dev(rnd(B, H * W, 64, seed=1))
        st = ops().groupnorm_stats(x)
        st0 = torch.zeros(B, 64, 2, device=DEV, dtype=torch.float64)
        st1 = ops().groupnorm_stats(x, st0)
        assert st1.data_ptr() == st0.data_ptr() and torch.equal(st1, st)
        y = ops().groupnorm_tokens(x, g, b, H, W)
        assert torch.equal(ops().groupnorm_tokens(x, g, b, H, W, stats=st, stats_ready=True), y)
        assert torch.equal(ops().groupnorm_tokens(x, g, b, H, W, stats=torch.zeros_like(st)), y)
    # several workgroups per image add their doubles atomically in any order: equal to the last bits of a double, not bit for bit
    B, H, W = 2, 61, 67
    x = dev(rnd(B, H * W, 64, seed=1))
    st, st1 = ops().groupnorm_stats(x), ops().groupnorm_stats(x, torch.zeros(B, 64, 2, device=DEV, dtype=torch.float64))
    assert float(((st1 - st).abs() / st.abs().clamp_min(1.0)).max()) <= 1e-13
    y, y1 = ops().groupnorm_tokens(x, g, b, H, W), ops().groupnorm_tokens(x, g, b, H, W, stats=st, stats_ready=True)
    assert float((y - y1).abs().max()) <= 2 * EPS32 * float(y.abs().max())
    with pytest.raises(RuntimeError):
        ops().groupnorm_stats(torch.zeros(1, 16, 96, device=DEV))
    with pytest.raises(RuntimeError):
        ops().groupnorm_tokens(x, g, b, H, W, stats=torch.zeros(B, 32, 2, device=DEV, dtype=torch.float64), stats_ready=True)


@pytest.mark.parametrize("H,W,uh,uw,big", [(15, 20, 8, 10, False), (61, 67, 1, 1, False), (16, 24, 5, 8, False), (61, 67, 31, 34, True),
                                           (15, 20, 0, 0, True)])
def test_groupnorm_split_and_half_forms(H, W, uh, uw, big):
    """The three-bf16-plane form sums to the fp32 form bit for bit and the half form is its clamped rounding, with the upsample add,
    at ragged sizes and beyond the half range (the moments are computed once and shared, so all three see the same bits)."""
    B, C = 2, 64
    x, g, b = dev(rnd(B, H * W, C, seed=1)), 1 + 0.1 * rnd(C, seed=2), dev(rnd(C, seed=3))
    if big:
        g[0], g[5] = 3e5, -2e5
    g = dev(g)
    kw = dict(up=dev(rnd(B, uh * uw, C, seed=4)), up_hw=(uh, uw)) if uh else {}
    st = ops().groupnorm_stats(x)
    for relu in (False, True):
        y32 = ops().groupnorm_tokens(x, g, b, H, W, relu=relu, stats=st, stats_ready=True, **kw)
        planes = ops().groupnorm_tokens(x, g, b, H, W, relu=relu, stats=st, stats_ready=True, split_planes=True, **kw)
        y16 = ops().groupnorm_tokens(x, g, b, H, W, relu=relu, stats=st, stats_ready=True, out_f16=True, **kw)
        assert planes.shape == (3, B, H * W, C) and planes.dtype == torch.bfloat16
        assert torch.equal((planes[0].float() + planes[1].float()) + planes[2].float(), y32)
        assert y16.dtype == torch.float16 and torch.equal(y16, y32.clamp(-65504.0, 65504.0).half()) and bool(torch.isfinite(y16).all())
        assert not big or float(y32.abs().max()) > 65504.0
    with pytest.raises(RuntimeError):
        ops().groupnorm_tokens(x, g, b, H, W, split_planes=True, out_f16=True)


# =============================================================================================
# GroupNorm written as NCHW planes
# =============================================================================================
NCHW_SHAPES = [(1, 64, 4), (3, 64, 60), (1, 64, 64), (3, 64, 68), (3, 64, 4800), (1, 64, 19200),
               (3, 4, 60), (1, 4, 4800), (1, 128, 68), (3, 128, 19200), (3, 128, 4)]


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("B,C,HW,groups", [s + (g,) for s in NCHW_SHAPES for g in groups_of(s[1])])
def test_groupnorm_nchw(B, C, HW, groups, relu):
    """HW = 4, 60, 68: a ragged last 64-token tile (clamped loads, guarded float4 stores).  The planes of the output are dense
    (plane stride HW), so a margin per plane is not expressible; the output sits inside a sentinel-filled flat buffer, which
    catches a write past the last plane or before the first, and a write past HW inside lands in the next plane, which the
    comparison over all elements sees."""
    from unseenobjectswithmeanshift_amd._lib import check, lib
    x, g, b = rnd(B, HW, C, seed=1), 1 + 0.1 * rnd(C, seed=2), rnd(C, seed=3)
    H, W = (HW // 4, 4)
    xd, gd, bd = dev(x), dev(g), dev(b)
    st = ops().groupnorm_stats(xd)
    n, pad = B * C * HW, 64
    buf = torch.full((n + 2 * pad,), SENTINEL, device=DEV)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + 4 * off)
    rc = lib().msm_groupnorm_apply_nchw_f32(p(xd), p(st), p(gd), p(bd), p(buf, pad), B, HW, C, groups, 1e-5, 1 if relu else 0,
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    check(rc, "msm_groupnorm_apply_nchw_f32")
    assert bool((buf[:pad] == SENTINEL).all()) and bool((buf[pad + n:] == SENTINEL).all())
    got = buf[pad:pad + n].view(B, C, HW)
    assert torch.equal(ops().groupnorm_nchw(xd, st, gd, bd, groups=groups, relu=relu), got)
    ref = O.groupnorm_tokens(x, g, b, H, W, groups, relu=relu).transpose(1, 2)
    t32 = gn_t32(x, g, b, H, W, groups, relu=relu).transpose(1, 2)
    rule("groupnorm_nchw", f"B={B} C={C} HW={HW} groups={groups} relu={relu}", got, ref, t32)
    # the same arithmetic per element as the token-major kernel, from the same moments
    tok = ops().groupnorm_tokens(xd, gd, bd, H, W, groups, relu=relu, stats=st, stats_ready=True)
    assert torch.equal(tok.transpose(1, 2), got)


def test_groupnorm_nchw_rejects_bad_arguments():
    from unseenobjectswithmeanshift_amd._lib import lib
    z = lambda *s, dt=torch.float32: torch.zeros(*s, device=DEV, dtype=dt)
    with pytest.raises(RuntimeError):
        ops().groupnorm_nchw(z(1, 6, 64), z(1, 64, 2, dt=torch.float64), z(64), z(64))               # HW % 4 != 0
    with pytest.raises(RuntimeError):
        ops().groupnorm_nchw(z(1, 8, 132), z(1, 132, 2, dt=torch.float64), z(132), z(132), groups=1)  # C > 128
    x, st, g = z(1, 64, 64), z(1, 64, 2, dt=torch.float64), z(64)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib().msm_groupnorm_apply_nchw_f32(p(x), p(st), p(g), p(g), p(x), 1, 64, 64, 32, 1e-5, 0,
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc != 0                                                                                  # x aliased with y


# =============================================================================================
# transpose, position encoding, L2 normalise
# =============================================================================================
@pytest.mark.parametrize("B,R,C", [(1, 1, 1), (3, 33, 31), (2, 100, 256), (2, 6300, 64)])
def test_transpose_last2(B, R, C):
    x = dev(rnd(B, R, C, seed=1))
    y = ops().transpose_last2(x)
    assert y.shape == (B, C, R) and y.is_contiguous() and torch.equal(y, x.transpose(1, 2))


@pytest.mark.parametrize("temperature,scale", [(10000.0, 2.0 * math.pi), (20.0, 1.0)])
@pytest.mark.parametrize("npf", [32, 128])
@pytest.mark.parametrize("H,W", [(1, 1), (7, 33), (30, 40)])
def test_pos_embed_sine(H, W, npf, temperature, scale):
    """Tolerance per element: 4 * eps_fp32 * max(1, |a|) + max|t32 - ref|, a the sine argument.  Derivation: a = e / dim_t is
    built from (pos / (size + 1e-6)) * scale -- the denominator, the quotient, scale itself and the product each round once --
    divided by powf(temperature, k / npf) (k / npf is exact for npf a power of two; powf is good to about an ulp) and the quotient
    rounds again: about 3.5 eps relative, so sinf / cosf see an argument that is off by 3.5 eps |a| and pass that on with slope
    <= 1, plus their own ulp of a result <= 1.  For |a| < 1 the result rounding dominates, hence max(1, |a|).  torch's fp32 run of
    the same formula differs from float64 for the same reasons, which is the additive term."""
    ref = O.position_embedding_sine(1, H, W, npf, temperature, scale, dtype=torch.float64)[0]
    t32 = O.position_embedding_sine(1, H, W, npf, temperature, scale)[0]
    i = torch.arange(npf, dtype=torch.float64)
    dim_t = temperature ** (2 * torch.div(i, 2, rounding_mode="floor") / npf)
    ay = (torch.arange(1, H + 1, dtype=torch.float64) / (H + 1e-6) * scale)[None, :] / dim_t[:, None]      # (npf, H)
    ax = (torch.arange(1, W + 1, dtype=torch.float64) / (W + 1e-6) * scale)[None, :] / dim_t[:, None]      # (npf, W)
    a = torch.cat([ay[:, :, None].expand(npf, H, W), ax[:, None, :].expand(npf, H, W)])
    add = rnd(2 * npf, seed=1)
    e_t = float((t32.double() - ref).abs().max())
    e_ta = float(((t32 + add[:, None, None]).double() - (ref + add.double()[:, None, None])).abs().max())
    kw = dict(temperature=temperature, scale=scale)
    cases = [
        ("nchw", ops().pos_embed_sine(H, W, npf, DEV, **kw), ref, e_t),
        ("tokens", ops().pos_embed_sine(H, W, npf, DEV, layout="tokens", **kw).t().reshape(2 * npf, H, W), ref, e_t),
        ("nchw+add_c", ops().pos_embed_sine(H, W, npf, DEV, add_c=dev(add), **kw), ref + add.double()[:, None, None], e_ta),
        ("tokens+add_c", ops().pos_embed_sine(H, W, npf, DEV, layout="tokens", add_c=dev(add), **kw).t().reshape(2 * npf, H, W),
         ref + add.double()[:, None, None], e_ta),
    ]
    for name, got, want, et in cases:
        err = (got.cpu().double() - want).abs()
        tol = 4 * EPS32 * a.abs().clamp_min(1.0) + et
        print(f"POS [pos_embed_sine] {H}x{W} npf={npf} T={temperature:g} {name}: kernel {float(err.max()):.3e} torch-fp32 {et:.3e} "
              f"worst err/tol {float((err / tol).max()):.2f}")
        assert bool((err <= tol).all())


@pytest.mark.parametrize("B,C,H,W", [(2, 64, 7, 9), (1, 65, 10, 12), (2, 33, 1, 5), (1, 130, 16, 16)])
def test_l2_normalize_nchw_edges(B, C, H, W):
    """An all-zero pixel gives 0 (never NaN); a pixel of norm 1e-20 is divided by the default eps 1e-12, not by its norm; C = 65 is
    the first channel count on the two-pass path."""
    x = rnd(B, C, H, W, seed=1)
    x[0, :, 0, 0] = 0
    tiny = rnd(C, seed=2)
    tiny = tiny / tiny.norm() * 1e-20
    x[0, :, 0, 1] = tiny
    y = ops().l2_normalize_nchw(dev(x))
    ref = x.double() / x.double().norm(dim=1, keepdim=True).clamp_min(1e-12)
    rule("l2_normalize_nchw", f"B={B} C={C} {H}x{W}", y, ref, F.normalize(x, p=2, dim=1))
    yc = y.cpu()
    assert torch.equal(yc[0, :, 0, 0], torch.zeros(C))
    want = x[0, :, 0, 1].double() / 1e-12
    assert float((yc[0, :, 0, 1].double() - want).abs().max()) <= 4 * EPS32 * float(want.abs().max())
    assert float((yc.double().norm(dim=1).flatten()[2:] - 1).abs().max()) <= 1e-6


# =============================================================================================
# the moments conv1x1_in produces as a by-product (fp32 per-tile sums; not part of the gn_stats_kernel change)
# =============================================================================================
@pytest.mark.xfail(strict=True, reason="known: conv_in_kernel sums its moments in fp32 per 16..64-pixel tile; measured on an MI355X max|err| "
                   "2.5e-4 against torch fp32 1.4e-5 (ratio 17.5, the rule allows 4).  DESIGN.md section 4b")
def test_conv1x1_in_moments_conditioning():
    """A bias of 100 on a unit-variance projection, normalised from the moments the projection kernel produced itself."""
    B, Cin, H, W = 2, 256, 60, 80
    x, w = rnd(B, Cin, H, W, seed=1), rnd(64, Cin, seed=2, scale=Cin ** -0.5)
    bias = torch.full((64,), 100.0)
    g, b = 1 + 0.1 * rnd(64, seed=3), rnd(64, seed=4)
    out, st = ops().conv1x1_in(dev(x), ops().pack_conv_in_weight(dev(w)), dev(bias))
    o = out.cpu()                                      # the GroupNorm input is the convolution's own fp32 output
    assert 99.0 < float(o.mean()) < 101.0 and 0.8 < float(o.std()) < 1.2
    got = ops().groupnorm_tokens(out, dev(g), dev(b), H, W, stats=st, stats_ready=True)
    rule("conv1x1_in moments -> groupnorm_tokens", "bias 100, unit variance", got, O.groupnorm_tokens(o, g, b, H, W, 32),
         gn_t32(o, g, b, H, W, 32))
