"""GroupNorm backward on the GPU (training.group_norm_tokens = csrc/norm_bwd.hip: msm_groupnorm_bwd_f32) against the float64 definition of
tests/pd_bwd_cases.py, which tests/test_pd_bwd_cases_cpu.py pins to the closed formula written out with sums.

Bound: the project's fp32 contract: max|got - ref64| <= 1e-4 max|ref64| per tensor, every element.  The figures are printed
(pytest -s) and recorded in DESIGN.md section 5t.  Needs a real MI355X (pytest -m gpu)."""
import functools

import pytest
import torch

import pd_bwd_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(name, x_grad=True, gamma_grad=True, beta_grad=True, g=None):
    from unseenobjectswithmeanshift_amd import training as tr
    c = K.GN_CASES[name]
    x, gamma, beta, g0 = K.gn_planted(name)
    xd = x.to(DEV).requires_grad_(x_grad)
    gd, bd = gamma.to(DEV).requires_grad_(gamma_grad), beta.to(DEV).requires_grad_(beta_grad)
    y = tr.group_norm_tokens(xd, gd, bd, c.groups, K.EPS, relu=c.relu)
    y.backward(g0.to(DEV) if g is None else g)
    torch.cuda.synchronize()
    return {"y": y.detach().cpu(), "dx": None if xd.grad is None else xd.grad.cpu(), "dgamma": None if gd.grad is None else gd.grad.cpu(),
            "dbeta": None if bd.grad is None else bd.grad.cpu()}


@functools.lru_cache(maxsize=None)
def _full(name):
    return _run(name)


@pytest.mark.parametrize("name", list(K.GN_CASES))
def test_matches_definition(name):
    ref, out = K.gn_reference64(name), _full(name)
    for k in ("y", "dx", "dgamma", "dbeta"):
        assert out[k].shape == ref[k].shape and out[k].dtype == torch.float32
        K.check("groupnorm backward", name, k, out[k], ref[k])
    if K.GN_CASES[name].relu:
        assert torch.equal(out["y"] == 0, ref["y"] == 0)                                     # the same ReLU mask as float64
        assert float(out["dx"][ref["y"] == 0].abs().max()) > 0                               # dx is dense: the group terms reach masked pixels


@pytest.mark.parametrize("name", K.GN_SPLIT_CASES)
@pytest.mark.parametrize("splits", K.GN_SPLITS)
def test_forced_splits(name, splits):
    from unseenobjectswithmeanshift_amd import ops
    c = K.GN_CASES[name]
    x, gamma, beta, g = (t.to(DEV) for t in K.gn_planted(name))
    ref = K.gn_reference64(name)
    stats = ops.groupnorm_stats(x)
    out = ops.groupnorm_backward(x, g, stats, gamma, beta, c.groups, eps=K.EPS, relu=c.relu, splits=splits)
    for k, t in zip(("dx", "dgamma", "dbeta"), out):
        K.check("groupnorm backward", name, f"{k} splits={splits}", t, ref[k])
    again = ops.groupnorm_backward(x, g, stats, gamma, beta, c.groups, eps=K.EPS, relu=c.relu, splits=splits)
    assert all(torch.equal(a, b) for a, b in zip(out, again))                                # bit-identical from call to call
    dx, dg, db = ops.groupnorm_backward(x, g, stats, gamma, beta, c.groups, eps=K.EPS, relu=c.relu, splits=splits, want_dx=False)
    assert dx is None and torch.equal(dg, out[1]) and torch.equal(db, out[2])
    dx, dg, db = ops.groupnorm_backward(x, g, stats, gamma, beta, c.groups, eps=K.EPS, relu=c.relu, splits=splits, want_dgamma=False,
                                        want_dbeta=False)
    assert dg is None and db is None and torch.equal(dx, out[0])


@pytest.mark.parametrize("name", ["odd", "wide4"])
def test_second_call_is_bit_identical(name):
    a, b = _full(name), _run(name)
    assert all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("name", ["odd", "c256"])
def test_needs_input_grad(name):
    full = _full(name)
    frozen_x = _run(name, x_grad=False)
    assert frozen_x["dx"] is None and torch.equal(frozen_x["dgamma"], full["dgamma"]) and torch.equal(frozen_x["dbeta"], full["dbeta"])
    frozen_gamma = _run(name, gamma_grad=False)
    assert frozen_gamma["dgamma"] is None and torch.equal(frozen_gamma["dx"], full["dx"]) and torch.equal(frozen_gamma["dbeta"], full["dbeta"])
    frozen_beta = _run(name, beta_grad=False)
    assert frozen_beta["dbeta"] is None and torch.equal(frozen_beta["dx"], full["dx"]) and torch.equal(frozen_beta["dgamma"], full["dgamma"])


@pytest.mark.parametrize("name", ["odd", "wide4"])
def test_non_contiguous_grad_output(name):
    c = K.GN_CASES[name]
    g = K.gn_planted(name)[3]
    big = torch.zeros(c.B, c.HW, c.C + 8)
    big[:, :, 4:4 + c.C] = g
    view = big.to(DEV)[:, :, 4:4 + c.C]                                                      # a channel-sliced view of a larger tensor
    assert not view.is_contiguous()
    a, b = _full(name), _run(name, g=view)
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_no_host_synchronisation():
    from unseenobjectswithmeanshift_amd import training as tr
    c = K.GN_CASES["odd"]
    x, gamma, beta, g = (t.to(DEV) for t in K.gn_planted("odd"))
    x.requires_grad_(True), gamma.requires_grad_(True), beta.requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        y = tr.group_norm_tokens(x, gamma, beta, c.groups, K.EPS, relu=True)
        y.backward(g)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    full = _full("odd")
    assert torch.equal(x.grad.cpu(), full["dx"]) and torch.equal(gamma.grad.cpu(), full["dgamma"])


def test_unsupported_shapes_raise():
    from unseenobjectswithmeanshift_amd import ops
    x = torch.zeros(1, 4, 64, device=DEV)
    v = torch.zeros(64, device=DEV)
    stats = torch.zeros(1, 64, 2, device=DEV, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="groups"):
        ops.groupnorm_backward(x, x, stats, v, v, 48)
    with pytest.raises(RuntimeError, match="msm_groupnorm_bwd"):
        ops.groupnorm_backward(x, x, stats, v, v, 32, splits=5000)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.groupnorm_backward(x, torch.zeros(1, 4, 128, device=DEV)[:, :, ::2], stats, v, v, 32)
    with pytest.raises(RuntimeError, match="stats"):
        ops.groupnorm_backward(x, x, stats[:, :32].contiguous(), v, v, 32)
