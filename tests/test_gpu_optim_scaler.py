"""GradScaler's protocol for fused optimizers (torch/amp/grad_scaler.py:403-454: the scaler sets ``grad_scale`` and ``found_inf`` on the
optimizer and calls ``step()``) in optim.FullModelClipAdamW, optim.Adam and optim.SGD: the kernels unscale the gradient, skip the step on
found_inf and count the steps of every tensor on the device; nothing waits for the GPU.

Bits are compared where two runs of the same kernels must agree (a power-of-two scale is exact, a skipped step changes nothing, the
device-counted AdamW is the host-counted one); the float64 references of tests/optim_cases.py / tests/optim_rule_cases.py are held to
their contract, max|got - ref64| <= 1e-4 max|ref64| per tensor.  Needs a real MI355X (pytest -m gpu)."""
import pytest
import torch

import optim_cases as OC
import optim_rule_cases as RC

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


def test_device_counted_adamw_is_the_host_counted_one():
    tensors, case, make, groups, keys, _ = _setup("adamw", "clip_active")
    _, opt_a, host = _trace(tensors, case, make, groups, keys, (1, 2, 3))
    _, opt_b, dev = _trace(tensors, case, make, groups, keys, (1, 2, 3), pre_step=lambda i, params, opt: _scalars(opt, 1.0, 0.0))
    assert not opt_a._device_counts and opt_b._device_counts
    for step, (a, b) in enumerate(zip(host, dev), 1):
        _same(a, b, f"step {step}")
    sd_a, sd_b = opt_a.state_dict()["state"], opt_b.state_dict()["state"]
    steps = [float(sd_b[i]["step"]) for i in range(len(tensors))]
    assert steps == [float(sd_a[i]["step"]) for i in range(len(tensors))] == [2.0 if t.name == "skip" else 3.0 for t in tensors]


def test_adamw_switches_to_device_counts_in_mid_run():
    """Two host-counted steps, then a scaler appears: the counts go up once and step 3 is the step 3 of a run without one."""
    tensors, case, make, groups, keys, _ = _setup("adamw", "clip_active")
    _, _, host = _trace(tensors, case, make, groups, keys, (1, 2, 3))
    _, opt, late = _trace(tensors, case, make, groups, keys, (1, 2, 3),
                          pre_step=lambda i, params, opt: _scalars(opt, 1.0, 0.0) if i == 2 else None)
    _same(host[2], late[2], "step 3")
    sd = opt.state_dict()["state"]
    assert [float(sd[i]["step"]) for i in range(len(tensors))] == [2.0 if t.name == "skip" else 3.0 for t in tensors]


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
