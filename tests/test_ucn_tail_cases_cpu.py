"""The case table of the UCN embedding-tail backward (tests/ucn_tail_cases.py) on the CPU: its float64 definition against an
independent restatement, torch's own fp32 run inside the contract, and the torch route of training.ucn_embedding_tail."""
import pytest
import torch

import ucn_tail_cases as tc

NAMES = list(tc.CASES)


@pytest.mark.parametrize("name", NAMES)
def test_reference64_is_the_closed_form(name):
    ref, re = tc.reference64(name), tc.restatement64(name)
    for k in ("y", "ga", "gb"):
        assert (ref[k] is None) == (re[k] is None), k
        if ref[k] is not None:
            tc.check(name, k + " restatement vs autograd", re[k], ref[k], rtol=1e-12)


@pytest.mark.parametrize("name", NAMES)
def test_torch_fp32_is_inside_the_contract(name):
    ref, got = tc.reference64(name), tc.torch32(name)
    for k in ("y", "ga", "gb"):
        if ref[k] is not None:
            tc.check(name, k + " torch fp32", got[k], ref[k])


@pytest.mark.parametrize("name", NAMES)
def test_both_towers_get_the_same_gradient(name):
    ref = tc.reference64(name)
    assert (ref["gb"] is None) == (tc.CASES[name].towers == 1)
    if ref["gb"] is not None:
        assert torch.equal(ref["ga"], ref["gb"])
    assert bool(torch.isfinite(ref["ga"]).all())


def test_what_the_cases_exercise():
    same = tc.reference64("same")
    _, _, g = tc.planted("same")
    assert torch.equal(same["ga"], g.double())                                   # identity size, no normalisation: weights 1 and 0
    for name, count in (("down", 51), ("px1", 3)):
        dead = tc.zero_gradient_pixels(name)
        assert int(dead.sum()) == count
        ga = tc.reference64(name)["ga"]
        assert bool((ga[:, :, dead] == 0).all()) and bool((ga[:, :, ~dead].abs().amax(dim=(0, 1)) > 0).all())
    # dead: some output pixels have u = 0 exactly, and their g / eps dominates the gradient
    a, b, _ = tc.planted("dead")
    c = tc.CASES["dead"]
    u = tc.expression(a.double(), b.double(), (c.H, c.W), 0)
    assert int((u.abs().amax(1) == 0).sum()) > 0
    assert 1e12 < float(tc.reference64("dead")["ga"].abs().max()) < 1e14


@pytest.mark.parametrize("name", NAMES)
def test_training_tail_torch_route(name):
    """training.ucn_embedding_tail(fused=False) -- and any call on host tensors -- is the literal expression."""
    from unseenobjectswithmeanshift_amd import training as tr
    c = tc.CASES[name]
    ref = tc.reference64(name)
    a, b, g = tc.planted(name)
    for fused in (False, True):                                                  # host tensors: the torch route either way
        x = a.clone().contiguous(memory_format=torch.channels_last).requires_grad_(True)
        z = None if b is None else b.clone().requires_grad_(True)
        y = tr.ucn_embedding_tail(x, z, (c.H, c.W), norms=c.norms, eps=tc.EPS, fused=fused)
        y.backward(g)
        tc.check(name, "y training route", y, ref["y"])
        tc.check(name, "ga training route", x.grad, ref["ga"])
        if z is not None:
            tc.check(name, "gb training route", z.grad, ref["gb"])
    if name == "down":
        dead = tc.zero_gradient_pixels(name)
        assert bool((x.grad[:, :, dead] == 0).all())


def test_training_tail_rejects_bad_norms():
    from unseenobjectswithmeanshift_amd import training as tr
    a, b, _ = tc.planted("px1")
    with pytest.raises(ValueError, match="norms"):
        tr.ucn_embedding_tail(a, b, (1, 1), norms=3)
