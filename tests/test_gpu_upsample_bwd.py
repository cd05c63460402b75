"""Bilinear token-map upsampling on the GPU, forward and adjoint (training.upsample_bilinear_tokens = csrc/norm_bwd.hip:
msm_upsample_bilinear_tokens_f32 / msm_upsample_bilinear_bwd_tokens_f32) against the float64 definition of tests/pd_bwd_cases.py
(F.interpolate autograd), which tests/test_pd_bwd_cases_cpu.py pins to the explicit matrix and its transpose.

Bound: the project's fp32 contract: max|got - ref64| <= 1e-4 max|ref64| per tensor, every element.  The figures are printed
(pytest -s) and recorded in DESIGN.md section 5t.  Needs a real MI355X (pytest -m gpu)."""
import functools

import pytest
import torch

import pd_bwd_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(name, g=None):
    from unseenobjectswithmeanshift_amd import training as tr
    c = K.UP_CASES[name]
    x, g0 = K.up_planted(name)
    xd = x.to(DEV).requires_grad_(True)
    y = tr.upsample_bilinear_tokens(xd, (c.h, c.w), (c.H, c.W))
    y.backward(g0.to(DEV) if g is None else g)
    torch.cuda.synchronize()
    return {"y": y.detach().cpu(), "dx": xd.grad.cpu()}


@functools.lru_cache(maxsize=None)
def _full(name):
    return _run(name)


@pytest.mark.parametrize("name", list(K.UP_CASES))
def test_matches_definition(name):
    ref, out = K.up_reference64(name), _full(name)
    for k in ("y", "dx"):
        assert out[k].shape == ref[k].shape and out[k].dtype == torch.float32
        K.check("upsample", name, k, out[k], ref[k])
    if name == "same":
        x, g = K.up_planted(name)
        assert torch.equal(out["y"], x) and torch.equal(out["dx"], g)                       # the identity, exactly


@pytest.mark.parametrize("name", list(K.UP_CASES))
def test_adjoint_identity(name):
    """<up(x), g> = <x, up^T(g)> with the package's own forward, both sums in float64 over the fp32 results, to the contract's
    bound on the value itself."""
    from unseenobjectswithmeanshift_amd import ops
    c = K.UP_CASES[name]
    x, g = (t.to(DEV) for t in K.up_planted(name))
    y = ops.upsample_bilinear(x, (c.h, c.w), (c.H, c.W))
    gx = ops.upsample_bilinear_backward(g, (c.h, c.w), (c.H, c.W))
    lhs, rhs = float((y.double() * g.double()).sum()), float((x.double() * gx.double()).sum())
    print(f"upsample case {name}: <up x, g> {lhs:.9e}  <x, up^T g> {rhs:.9e}  |difference| / |value| {abs(lhs - rhs) / abs(lhs):.2e}")
    assert abs(lhs - rhs) <= K.RTOL * abs(lhs)
    # the inference path's fused form of the same forward (GroupNorm output + upsample), here on a zero map: the same four-tap fp32
    # expression, so at most a few roundings apart (how the compiler contracts it): 1e-6 of the largest value
    zero = torch.zeros(K.UP_B, c.H * c.W, K.UP_C, device=DEV)
    fused = ops.groupnorm_tokens(zero, torch.ones(K.UP_C, device=DEV), torch.zeros(K.UP_C, device=DEV), c.H, c.W, up=x, up_hw=(c.h, c.w))
    assert float((fused - y).abs().max()) <= 1e-6 * float(y.abs().max())


@pytest.mark.parametrize("name", ["odd", "res3"])
def test_second_call_is_bit_identical(name):
    a, b = _full(name), _run(name)
    assert all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("name", ["odd", "res3"])
def test_non_contiguous_tensors(name):
    c = K.UP_CASES[name]
    x, g = K.up_planted(name)
    big = torch.zeros(K.UP_B, c.H * c.W, K.UP_C + 8)
    big[:, :, 4:4 + K.UP_C] = g
    view = big.to(DEV)[:, :, 4:4 + K.UP_C]                                                   # a channel-sliced gradient
    assert not view.is_contiguous()
    a, b = _full(name), _run(name, g=view)
    assert all(torch.equal(a[k], b[k]) for k in a)
    # the source as a token range of a longer buffer (the finest encoder level): read in place
    from unseenobjectswithmeanshift_amd import training as tr
    buf = torch.zeros(K.UP_B, c.h * c.w + 5, K.UP_C)
    buf[:, 5:] = x
    src = buf.to(DEV).requires_grad_(True)
    y = tr.upsample_bilinear_tokens(src[:, 5:], (c.h, c.w), (c.H, c.W))
    y.backward(g.to(DEV))
    assert torch.equal(y.detach().cpu(), a["y"]) and torch.equal(src.grad[:, 5:].cpu(), a["dx"])
    assert float(src.grad[:, :5].abs().max()) == 0.0


def test_no_host_synchronisation():
    from unseenobjectswithmeanshift_amd import training as tr
    c = K.UP_CASES["odd"]
    x, g = (t.to(DEV) for t in K.up_planted("odd"))
    x.requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        tr.upsample_bilinear_tokens(x, (c.h, c.w), (c.H, c.W)).backward(g)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.equal(x.grad.cpu(), _full("odd")["dx"])


def test_downsampling_and_unsupported_shapes():
    from unseenobjectswithmeanshift_amd import ops
    # outside the required range (H < h), still the adjoint of the forward
    gen = torch.Generator().manual_seed(3)
    x, g = torch.randn(1, 5 * 7, 8, generator=gen).to(DEV), torch.randn(1, 2 * 3, 8, generator=gen).to(DEV)
    y, gx = ops.upsample_bilinear(x, (5, 7), (2, 3)), ops.upsample_bilinear_backward(g, (5, 7), (2, 3))
    lhs, rhs = float((y.double() * g.double()).sum()), float((x.double() * gx.double()).sum())
    assert abs(lhs - rhs) <= K.RTOL * abs(lhs)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.upsample_bilinear_backward(torch.zeros(1, 6, 6, device=DEV), (1, 3), (2, 3))
    with pytest.raises(RuntimeError, match="upsample_bilinear_backward"):
        ops.upsample_bilinear_backward(torch.zeros(1, 7, 8, device=DEV), (1, 3), (2, 3))
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.upsample_bilinear_backward(torch.zeros(1, 6, 16, device=DEV)[:, :, ::2], (1, 3), (2, 3))
