"""3x3 convolution backward on the GPU (training.conv3x3 = csrc/conv3x3_bwd.hip for weight and bias, the implicit GEMM for the input)
against the float64 definition of tests/conv_bwd_cases.py, which tests/test_conv_bwd_cases_cpu.py pins to a nine-term restatement.

Bound: the project's fp32 contract: max|got - ref64| <= 1e-4 max|ref64| per tensor.  Plain fp32 F.conv2d autograd on the
CPU sits between 2e-8 and 1e-6 of float64 on these cases; the kernels' figures are printed (pytest -s) and recorded in DESIGN.md
section 5s.  Needs a real MI355X (pytest -m gpu)."""
import functools

import pytest
import torch

import conv_bwd_cases as CC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(name, x_grad=True, w_grad=True, g=None):
    from unseenobjectswithmeanshift_amd import training as tr
    x, w, bias, g0 = CC.planted(name)
    xd = x.to(DEV).requires_grad_(x_grad)
    wd, bd = w.to(DEV).requires_grad_(w_grad), bias.to(DEV).requires_grad_(w_grad)
    y = tr.conv3x3(xd, wd, bd)
    y.backward(g0.to(DEV) if g is None else g)
    torch.cuda.synchronize()
    return {"y": y.detach().cpu(), "dx": None if xd.grad is None else xd.grad.cpu(), "dw": None if wd.grad is None else wd.grad.cpu(),
            "db": None if bd.grad is None else bd.grad.cpu()}


@functools.lru_cache(maxsize=None)
def _full(name):
    return _run(name)


@pytest.mark.parametrize("name", list(CC.CASES))
def test_matches_definition(name):
    ref, out = CC.reference64(name), _full(name)
    for k in ("y", "dx", "dw", "db"):
        assert out[k].shape == ref[k].shape and out[k].dtype == torch.float32
        CC.check(name, k, out[k], ref[k])
    z = CC.structural_zero_taps(name)
    if z.any():
        assert float(out["dw"][:, :, z].abs().max()) == 0.0                                  # exactly: a padded tap contributes nothing


@pytest.mark.parametrize("name", CC.SPLIT_CASES)
@pytest.mark.parametrize("splits", [1, 3, None])
def test_weight_grad_splits(name, splits):
    from unseenobjectswithmeanshift_amd import ops
    c = CC.CASES[name]
    x, _, _, g = CC.planted(name)
    ref = CC.reference64(name)
    tok = x.flatten(2).transpose(1, 2).contiguous().to(DEV)
    gd = g.to(DEV)
    dw, db = ops.conv3x3_weight_grad(tok, gd, c.H, c.W, splits=splits)
    assert tuple(dw.shape) == (c.Cout, 576) and tuple(db.shape) == (c.Cout,)
    CC.check(name, f"dw splits={splits}", dw, CC.tap_major(ref["dw"]))
    CC.check(name, f"db splits={splits}", db, ref["db"])
    dw2, db2 = ops.conv3x3_weight_grad(tok, gd, c.H, c.W, splits=splits)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)                                     # bit-identical from call to call
    dw3, none = ops.conv3x3_weight_grad(tok, gd, c.H, c.W, splits=splits, want_bias=False)
    assert none is None and torch.equal(dw, dw3)


@pytest.mark.parametrize("name", ["odd", "wide"])
def test_second_call_is_bit_identical(name):
    a, b = _full(name), _run(name)
    assert all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("name", ["odd", "wide"])
def test_needs_input_grad(name):
    full = _full(name)
    frozen_x = _run(name, x_grad=False)
    assert frozen_x["dx"] is None
    assert torch.equal(frozen_x["dw"], full["dw"]) and torch.equal(frozen_x["db"], full["db"])
    frozen_w = _run(name, w_grad=False)
    assert frozen_w["dw"] is None and frozen_w["db"] is None
    assert torch.equal(frozen_w["dx"], full["dx"])


@pytest.mark.parametrize("name", ["odd", "wide"])
def test_non_contiguous_grad_output(name):
    c = CC.CASES[name]
    g = CC.planted(name)[3]
    big = torch.zeros(c.B, c.Cout + 5, c.H, c.W)
    big[:, 3:3 + c.Cout] = g
    view = big.to(DEV)[:, 3:3 + c.Cout]                                                      # a channel-sliced view of a larger tensor
    assert not view.is_contiguous()
    a, b = _full(name), _run(name, g=view)
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_unsupported_shapes_raise():
    from unseenobjectswithmeanshift_amd import ops
    tok = torch.zeros(1, 16, 64, device=DEV)
    with pytest.raises(RuntimeError, match="msm_conv3x3_c64_wgrad"):
        ops.conv3x3_weight_grad(tok, torch.zeros(1, 96, 4, 4, device=DEV), 4, 4)              # Cout not a multiple of 64
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.conv3x3_weight_grad(tok, torch.zeros(1, 128, 4, 4, device=DEV)[:, ::2], 4, 4)
    with pytest.raises(RuntimeError, match="tok"):
        ops.conv3x3_weight_grad(torch.zeros(1, 16, 32, device=DEV), torch.zeros(1, 64, 4, 4, device=DEV), 4, 4)
