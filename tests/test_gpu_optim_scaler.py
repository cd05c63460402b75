"""GradScaler's protocol for fused optimizers (torch/amp/grad_scaler.py:403-454: the scaler sets ``grad_scale`` and ``found_inf`` on the
optimizer and calls ``step()``) in optim.FullModelClipAdamW, optim.Adam and optim.SGD: the kernels unscale the gradient, skip the step on
found_inf and count the steps of every tensor on the device; nothing waits for the GPU.

Bits are compared where two runs of the same kernels must agree (a power-of-two scale is exact, a skipped step changes nothing) and
where AdamW must stay what it was (the recorded fixture tests/golden/optim_adamw_bits.json); the float64 references of tests/optim_cases.py / tests/optim_rule_cases.py are held to
their contract, max|got - ref64| <= 1e-4 max|ref64| per tensor.  Needs a real MI355X (pytest -m gpu)."""
import json
import math
import os
import sys

import pytest
import torch

import optim_cases as OC
import optim_rule_cases as RC

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import record_optim_bits as RB  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KW = dict(device=DEV, dtype=torch.float32)
SCALE = 65536.0
RULES = ("adamw", "adam", "sgd")


def _chunk():
    from unseenobjectswithmeanshift_amd import ops
    return ops.optim_chunk()


def _setup(rule, case_name):
    """(case, make_opt, torch's make_opt, groups, state keys, float64 reference(grad_steps)) of a rule on a case of optim_cases; SGD
    takes the rows of its own clipped or unclipped case (see optim_rule_cases) and the dampened variant."""
    from unseenobjectswithmeanshift_amd.optim import SGD, Adam, FullModelClipAdamW
    case = OC.CASES[case_name]._replace(steps=3)
    tensors = OC.edge_tensors(_chunk())
    if rule == "sgd":
        groups = RC.sgd_groups("sgd_clip" if case.max_norm > 0 else "sgd_no_clip", "dampened")
        make, make_t, keys = (lambda g: SGD(g, 1e-3, max_norm=case.max_norm)), RC.torch_sgd(case.max_norm), RC.SGD_KEYS
    elif rule == "adam":
        groups, keys = OC.groups_of, RC.ADAM_KEYS
        make, make_t = (lambda g: Adam(g, max_norm=case.max_norm)), RC.torch_adam(case.max_norm)
    else:
        groups, keys = OC.groups_of, RC.ADAM_KEYS
        make = lambda g: FullModelClipAdamW(g, max_norm=case.max_norm)
        make_t = lambda g: OC.ClippedTorchAdamW(g, case.max_norm, foreach=False)
    reference = lambda grad_steps: RC.run(tensors, case, make_t, groups, keys, grad_steps=grad_steps)[2]
    return tensors, case, make, groups, keys, reference


def _trace(tensors, case, make, groups, keys, grad_steps, pre_step=None, post_step=None):
    """Step through grad_steps; after every step the bits of p, .grad and the state of every tensor."""
    params = OC.make_params(tensors, DEV, torch.float32)
    opt = make(groups(tensors, params))
    trace = []
    for i, step in enumerate(grad_steps):
        OC.set_grads(params, OC.gradients(tensors, case, step), DEV)
        if pre_step is not None:
            pre_step(i, params, opt)
        opt.step()
        if post_step is not None:
            post_step(i, params, opt)
        shot = {}
        for name, p in params.items():
            st = opt.state.get(p, {})
            shot[name] = dict(p=p.detach().clone(), grad=None if p.grad is None else p.grad.clone(),
                              **{k: st[k].clone() if st.get(k) is not None else None for k in keys})
        shot["norm"], shot["coef"] = opt.last_grad_norm.clone(), opt.last_clip_coef.clone()
        trace.append(shot)
    torch.cuda.synchronize()
    return params, opt, trace


def _same(a, b, what, skip=()):
    for name, x in a.items():
        if name in ("norm", "coef"):
            assert torch.equal(x, b[name]), (what, name)
            continue
        for k, v in x.items():
            if k in skip:
                continue
            w = b[name][k]
            assert (v is None and w is None) or (v is not None and w is not None and torch.equal(v, w)), (what, name, k)


def _scalars(opt, scale, found):
    opt.grad_scale = None if scale is None else torch.full((), scale, dtype=torch.float32, device=DEV)
    opt.found_inf = torch.full((), found, dtype=torch.float32, device=DEV)


def test_adamw_reproduces_the_recorded_bits():
    """FullModelClipAdamW against tests/golden/optim_adamw_bits.json, recorded by tools/record_optim_bits.py on the last commit that
    stepped AdamW through host-counted kernels of its own: every case of optim_cases on the edge table, three steps, without a
    scaler and with grad_scale = 1, found_inf = 0 set before every step.  Every hash (p, .grad, exp_avg, exp_avg_sq of every
    tensor) and bit pattern (last_grad_norm, last_clip_coef) of every step is the recorded one, and the step counts are the steps
    a tensor had a gradient in.  One test over all twelve runs (about a second): a failure names run, step, tensor and quantity.

    The fixture pins the compiler's sqrtf, division and double pow along with the kernels' own arithmetic.  A toolchain change
    that moves it is answered by recording again on the last commit that passed, with the new toolchain, never by loosening this
    test."""
    with open(RB.DEFAULT_OUT) as f:
        fixture = json.load(f)
    chunk = _chunk()
    assert fixture["header"]["chunk"] == chunk and fixture["header"]["steps"] == RB.STEPS
    assert set(fixture["cases"]) == set(OC.CASES)
    fed = RB.inputs(chunk)
    tensors = OC.edge_tensors(chunk)
    for case_name, case in RB.cases().items():
        assert fed["values"] == fixture["inputs"]["values"] and fed["gradients"][case_name] == fixture["inputs"]["gradients"][case_name], (
            f"{case_name}: the start values or gradients are not the recorded ones (a mismatch on inputs: re-record on the parent)")
        recorded = fixture["cases"][case_name]
        taken = [float(sum(t.name not in case.skip.get(step, ()) for step in range(1, RB.STEPS + 1))) for t in tensors]
        if case_name == "clip_active":
            assert taken == [2.0 if t.name == "skip" else 3.0 for t in tensors]
        for run, pre in (("no scaler", None), ("grad_scale 1, found_inf 0", lambda opt: _scalars(opt, 1.0, 0.0))):
            opt, shots = RB.run_case(case, chunk, DEV, pre_step=pre)
            torch.cuda.synchronize()
            assert len(recorded) == len(shots) == RB.STEPS
            for step, (got, ref) in enumerate(zip(shots, recorded), 1):
                where = f"{case_name}, {run}, step {step}"
                for q in ("last_grad_norm", "last_clip_coef"):
                    assert got[q] == ref[q], f"{where} {q}: {got[q]:#010x}, recorded {ref[q]:#010x} (the arithmetic changed)"
                for t in tensors:
                    for q in RB.QUANTITIES:
                        assert got["tensors"][t.name][q] == ref["tensors"][t.name][q], (
                            f"{where} {t.name} {q}: not the recorded bits (the arithmetic changed)")
            sd = opt.state_dict()["state"]
            assert [float(sd[i]["step"]) for i in range(len(tensors))] == taken, (case_name, run)


def test_a_scaler_that_appears_in_mid_run_changes_no_bit():
    """Two steps without a scaler, then one appears: step 3 is the step 3 of a run without one, and the counts are 2 and 3."""
    tensors, case, make, groups, keys, _ = _setup("adamw", "clip_active")
    _, _, plain = _trace(tensors, case, make, groups, keys, (1, 2, 3))
    _, opt, late = _trace(tensors, case, make, groups, keys, (1, 2, 3),
                          pre_step=lambda i, params, opt: _scalars(opt, 1.0, 0.0) if i == 2 else None)
    _same(plain[2], late[2], "step 3")
    sd = opt.state_dict()["state"]
    assert [float(sd[i]["step"]) for i in range(len(tensors))] == [2.0 if t.name == "skip" else 3.0 for t in tensors]


@pytest.mark.parametrize("rule", ["adamw", "adam"])
def test_fresh_state_restarts_the_count(rule):
    """Two steps, the state of n5 dropped, a third step: n5 gets fresh state and steps as at step 1 from zero moments (the float64
    formula, held to the contract), the others go on to step 3, and the step that notices waits for nothing."""
    tensors, case, make, groups, keys, _ = _setup(rule, "clip_active")
    case = case._replace(skip={})
    params = OC.make_params(tensors, DEV, torch.float32)
    opt = make(groups(tensors, params))
    for step in (1, 2):
        OC.set_grads(params, OC.gradients(tensors, case, step), DEV)
        opt.step()
    given = OC.gradients(tensors, case, 3)
    OC.set_grads(params, given, DEV)
    p = params["n5"]
    del opt.state[p]
    before = p.detach().double().clone()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    sd = opt.state_dict()["state"]
    assert [float(sd[i]["step"]) for i in range(len(tensors))] == [1.0 if t.name == "n5" else 3.0 for t in tensors]
    i = [t.name for t in tensors].index("n5")
    total = math.sqrt(sum(float(g.double().pow(2).sum()) for g in given.values()))
    g = given["n5"].double() * min(1.0, case.max_norm / (total + 1e-6))           # clip_grad_norm_ over the whole table
    z = torch.zeros_like(g)
    ref_p, ref_m, ref_v = (OC.adamw64 if rule == "adamw" else RC.adam64)(before.cpu(), g, z, z, 1, **RC.adam_hyper(i))
    st = opt.state[p]
    for what, got, ref in (("update", p.detach().double() - before, ref_p - before.cpu()), ("exp_avg", st["exp_avg"].double(), ref_m),
                           ("exp_avg_sq", st["exp_avg_sq"].double(), ref_v)):
        err, scale = float((got.cpu() - ref).abs().max()), float(ref.abs().max())
        print(f"{rule} fresh state, n5 {what}: {err / scale:.2e}")
        assert err <= OC.RTOL * scale, (rule, what, err, scale)


@pytest.mark.parametrize("case_name", ["clip_active", "no_clip", "eps_decides"])
@pytest.mark.parametrize("rule", RULES)
def test_unscaling_by_a_power_of_two_is_exact(rule, case_name):
    tensors, case, make, groups, keys, _ = _setup(rule, case_name)

    def scaled(i, params, opt):
        for p in params.values():
            if p.grad is not None:
                p.grad.mul_(SCALE)
        _scalars(opt, SCALE, 0.0)

    _, _, plain = _trace(tensors, case, make, groups, keys, (1, 2, 3))
    _, _, unscaled = _trace(tensors, case, make, groups, keys, (1, 2, 3), pre_step=scaled)
    for step, (a, b) in enumerate(zip(plain, unscaled), 1):
        _same(a, b, f"{rule} {case_name} step {step}")             # .grad too: the unscaled, clipped gradient
    if case.max_norm <= 0:                                          # nothing clipped: .grad is the gradient that was given, unscaled
        given = OC.gradients(tensors, case, 3)
        assert all(torch.equal(unscaled[2][t.name]["grad"].cpu(), given[t.name]) for t in tensors)


@pytest.mark.parametrize("rule,scale", [(r, 1.0) for r in RULES] + [("adam", None)])
def test_a_skipped_step_changes_nothing_and_is_not_counted(rule, scale):
    tensors, case, make, groups, keys, reference = _setup(rule, "clip_active")
    kept = {}

    def pre(i, params, opt):
        _scalars(opt, scale, 1.0 if i == 1 else 0.0)
        if i == 1:
            params["n5"].grad[2] = float("inf")
            kept["grads"] = {name: None if p.grad is None else p.grad.clone() for name, p in params.items()}

    def post(i, params, opt):
        kept[i] = opt._steps_dev.clone()

    params, opt, trace = _trace(tensors, case, make, groups, keys, (1, 2, 3), pre_step=pre, post_step=post)
    _same(trace[0], trace[1], f"{rule}: after the skipped step", skip=("grad",))        # p, state, last_grad_norm, last_clip_coef
    assert torch.equal(kept[0], kept[1]) and int(kept[0].min()) == 1                    # every step count
    for name, g in kept["grads"].items():                                               # .grad untouched, the inf included
        got = trace[1][name]["grad"]
        assert (g is None and got is None) or torch.equal(g, got), name
    assert bool(torch.isinf(trace[1]["n5"]["grad"][2]))
    # the same optimizer over the gradients of steps 1 and 3: bias correction at step 2, SGD's dampened update
    _, opt_2, two = _trace(tensors, case, make, groups, keys, (1, 3), pre_step=lambda i, params, opt: _scalars(opt, scale, 0.0))
    _same(trace[2], two[1], f"{rule}: steps 1, skipped, 3 against steps 1, 3")
    assert torch.equal(kept[2], opt_2._steps_dev) and int(kept[2].max()) == 2
    if rule != "sgd":
        sd = opt.state_dict()["state"]
        assert [float(sd[i]["step"]) for i in range(len(tensors))] == [2.0] * len(tensors)
    # and the float64 run of those two steps
    params, opt, shots = RC.run(tensors, case, make, groups, keys, grad_steps=(1, 2, 3), pre_step=pre, **KW)
    torch.cuda.synchronize()
    ref = reference((1, 3))
    quantities = ("update", "grad") + keys
    OC.compare(shots[0], ref[0], f"{rule} with a skipped step: step 1", quantities=quantities)
    assert all(float(shots[1][t.name]["update"].abs().max()) == 0.0 for t in tensors)
    OC.compare(shots[2], ref[1], f"{rule} with a skipped step: step 3", quantities=quantities)


@pytest.mark.parametrize("rule", RULES)
def test_the_reference_step_through_a_grad_scaler_does_not_wait(rule):
    """AMPTrainer.run_step: scaler.scale(losses).backward(); scaler.step(optimizer); scaler.update(), three iterations, the second
    overflows.  Only scaler.step() runs under the sync-debug mode: with an optimizer outside the protocol it raises there, on the
    .item() of GradScaler._maybe_opt_step."""
    tensors, _, make, groups, keys, _ = _setup(rule, "clip_active")
    case = OC.Case("scaler", 0.01, 3, ("randn", 1.0), {})
    make_t = {"sgd": RC.torch_sgd(0.01), "adam": RC.torch_adam(0.01), "adamw": lambda g: OC.ClippedTorchAdamW(g, 0.01, foreach=False)}[rule]
    ref = RC.run(tensors, case, make_t, groups, keys, grad_steps=(1, 3))[2]
    params = OC.make_params(tensors, DEV, torch.float32)
    opt = make(groups(tensors, params))
    scaler = torch.amp.GradScaler("cuda", init_scale=SCALE)
    shots = []
    for it in (1, 2, 3):
        weights = {name: g.to(DEV) for name, g in OC.gradients(tensors, case, it).items()}
        loss = sum((p * weights[name]).sum() for name, p in params.items())
        if it == 2:
            loss = loss * 3e38                                       # times the scale: every gradient overflows
        opt.zero_grad()
        scaler.scale(loss).backward()
        before = {name: p.detach().double().clone() for name, p in params.items()}
        torch.cuda.set_sync_debug_mode("error")
        try:
            scaler.step(opt)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        scaler.update()
        shots.append(RC.snapshot(params, opt, before, keys))
    torch.cuda.synchronize()
    assert not hasattr(opt, "grad_scale") and not hasattr(opt, "found_inf")
    quantities = ("update", "grad") + keys
    OC.compare(shots[0], ref[0], f"{rule} under GradScaler: iteration 1", quantities=quantities)
    assert all(float(shots[1][t.name]["update"].abs().max()) == 0.0 for t in tensors)
    OC.compare(shots[2], ref[1], f"{rule} under GradScaler: iteration 3", quantities=quantities)
    assert scaler.get_scale() == SCALE / 2                          # halved once, by the overflowing iteration
    assert opt._steps_dev.tolist() == [2] * len(tensors)
