"""Backward of the UCN embedding tail on the GPU (csrc/backbone_bwd.hip through training.ucn_embedding_tail and
ops.ucn_embedding_tail_bwd; pytest -m gpu) against the float64 definition of tests/ucn_tail_cases.py, per tensor within the fp32
contract with every element counted; run with -s for the measured fractions."""
import pytest
import torch

import ucn_tail_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = list(tc.CASES)


def _run(name, *, grad_a=True, grad_b=True, gout=None):
    """(y, grad of a, grad of b) of the fused route on the planted inputs (channels_last a, NCHW b: both layouts are accepted)."""
    from unseenobjectswithmeanshift_amd import training as tr
    c = tc.CASES[name]
    a, b, g = tc.planted(name)
    x = a.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(grad_a)
    z = None if b is None else b.to(DEV).requires_grad_(grad_b)
    y = tr.ucn_embedding_tail(x, z, (c.H, c.W), norms=c.norms, eps=tc.EPS)
    assert y.shape == (c.B, 64, c.H, c.W) and y.is_contiguous()
    y.backward(g.to(DEV) if gout is None else gout)
    return y.detach(), x.grad, None if z is None else z.grad


@pytest.mark.parametrize("name", NAMES)
def test_fused_tail_vs_float64(name):
    ref = tc.reference64(name)
    y, ga, gb = _run(name)
    tc.check(name, "y", y, ref["y"])
    tc.check(name, "grad a", ga, ref["ga"])
    assert ga.shape == ref["ga"].shape and (gb is None) == (ref["gb"] is None)
    if gb is not None:
        tc.check(name, "grad b", gb, ref["gb"])
        assert torch.equal(ga, gb)                                               # add fusion: one tensor for both towers
    if name == "same":
        assert torch.equal(ga.cpu(), tc.planted(name)[2])                        # weights exactly 1 and 0: gout, bit for bit
    if name in ("down", "px1"):
        assert bool((ga.cpu()[:, :, tc.zero_gradient_pixels(name)] == 0).all())
    assert bool(torch.isfinite(ga).all())


@pytest.mark.parametrize("name", NAMES)
def test_two_calls_same_bits(name):
    from unseenobjectswithmeanshift_amd import ops
    c = tc.CASES[name]
    a, b, g = (None if t is None else t.to(DEV) for t in tc.planted(name))
    first = ops.ucn_embedding_tail_bwd(a, b, g, norms=c.norms, eps=tc.EPS)
    second = ops.ucn_embedding_tail_bwd(a, b, g, norms=c.norms, eps=tc.EPS)
    assert first.shape == a.shape and first.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))
    assert torch.equal(first, _run(name)[1])                                     # the autograd route calls the same kernels


@pytest.mark.parametrize("name", ["x8n2", "odd", "wide"])
def test_stride0_gradient_and_single_tower_grad(name):
    c = tc.CASES[name]
    ones = torch.ones(c.B, 64, c.H, c.W, device=DEV)
    _, ga, gb = _run(name, gout=ones)
    # y.sum().backward() hands the Function an expanded scalar (every stride 0)
    from unseenobjectswithmeanshift_amd import training as tr
    a, b, _ = tc.planted(name)
    x = a.to(DEV).requires_grad_(True)
    z = None if b is None else b.to(DEV).requires_grad_(True)
    tr.ucn_embedding_tail(x, z, (c.H, c.W), norms=c.norms, eps=tc.EPS).sum().backward()
    assert torch.equal(x.grad, ga)
    if z is not None:
        assert torch.equal(z.grad, gb)
        # only one tower requires grad: the same bits, and nothing for the other
        _, only_a, none_b = _run(name, grad_b=False)
        none_a, only_b, = _run(name, grad_a=False)[1:]
        full = _run(name)[1]
        assert none_b is None and none_a is None and torch.equal(only_a, full) and torch.equal(only_b, full)


@pytest.mark.parametrize("name", ["same", "up0"])
def test_adjoint_identity_without_normalisation(name):
    """norms = 0: the backward is the transpose of the upsampling, <up(a) + up(b), g> = <a + b, gin> (relative 1e-5, sums in float64)."""
    c = tc.CASES[name]
    assert c.norms == 0
    y, ga, _ = _run(name)
    a, b, g = tc.planted(name)
    lhs = float((y.cpu().double() * g.double()).sum())
    rhs = float(((a + b).double() * ga.cpu().double()).sum())
    print(f"ucn tail case {name}: <up(a)+up(b), g> {lhs:.9g}  <a+b, gin> {rhs:.9g}")
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs)


def test_bad_arguments_raise():
    from unseenobjectswithmeanshift_amd import ops
    a, b, g = (t.to(DEV) for t in tc.planted("x8"))
    with pytest.raises(RuntimeError):
        ops.ucn_embedding_tail_bwd(a.cpu(), b.cpu(), g.cpu())                    # host tensors
    with pytest.raises(RuntimeError):
        ops.ucn_embedding_tail_bwd(a[:, :32], None, g)                           # wrong channel count
    with pytest.raises(RuntimeError):
        ops.ucn_embedding_tail_bwd(a, b[:1], g)                                  # mismatched towers
    with pytest.raises(RuntimeError):
        ops.ucn_embedding_tail_bwd(a, b, g[:, :32])                              # gout channels
    with pytest.raises(RuntimeError):
        ops.ucn_embedding_tail_bwd(a, b, g.double())
    with pytest.raises(RuntimeError):
        ops.ucn_embedding_tail_bwd(a, b, g.transpose(2, 3))                      # not contiguous
    with pytest.raises(RuntimeError, match="norms"):
        ops.ucn_embedding_tail_bwd(a, b, g, norms=3)                             # MSM_REQUIRE in the library
