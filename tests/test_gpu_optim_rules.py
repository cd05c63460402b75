"""optim.SGD and optim.Adam on the GPU (the rule entries of csrc/optimizer.hip) against the float64 references of
tests/optim_rule_cases.py: clip_grad_norm_ + torch.optim.SGD / torch.optim.Adam (foreach=False) over the same groups on the CPU.

Bound: the contract of tests/optim_cases.py per tensor, max|got - ref64| <= 1e-4 max|ref64| with no element left out, for the update
p_after - p_before, the state tensors, the written-back .grad, total_norm and coef.  torch's own fp32 CPU run of the same cases is held
to the same bound in tests/test_optim_rules_cpu.py; the kernels' figures are printed (pytest -s) and recorded in DESIGN.md section
5za.  Needs a real MI355X (pytest -m gpu)."""
import functools

import pytest
import torch

import optim_cases as OC
import optim_rule_cases as RC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KW = dict(device=DEV, dtype=torch.float32)
SGD_Q = ("update", "grad") + RC.SGD_KEYS
ADAM_Q = ("update", "grad") + RC.ADAM_KEYS


def _chunk():
    from unseenobjectswithmeanshift_amd import ops
    return ops.optim_chunk()


def _sgd(max_norm):
    from unseenobjectswithmeanshift_amd.optim import SGD
    return lambda groups: SGD(groups, 1e-3, max_norm=max_norm)              # every group carries its own hyper-parameters


def _adam(max_norm):
    from unseenobjectswithmeanshift_amd.optim import Adam
    return lambda groups: Adam(groups, max_norm=max_norm)


def _run_sgd(case_name, variant, **kw):
    case = RC.SGD_CASES[case_name]
    out = RC.run(OC.edge_tensors(_chunk()), case, _sgd(case.max_norm), RC.sgd_groups(case_name, variant), RC.SGD_KEYS, **KW, **kw)
    torch.cuda.synchronize()
    return out


def _run_adam(case_name, **kw):
    case = OC.CASES[case_name]
    out = RC.run(OC.edge_tensors(_chunk()), case, _adam(case.max_norm), OC.groups_of, RC.ADAM_KEYS, **KW, **kw)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _first_sgd(case_name, variant):
    return _run_sgd(case_name, variant)


@functools.lru_cache(maxsize=None)
def _first_adam(case_name):
    return _run_adam(case_name)


@pytest.mark.parametrize("case_name", list(RC.SGD_CASES))
@pytest.mark.parametrize("variant", list(RC.SGD_VARIANTS))
def test_sgd_matches_reference(variant, case_name):
    params, opt, shots = _first_sgd(case_name, variant)
    ref = RC.sgd_reference64(case_name, variant, _chunk())
    assert len(shots) == len(ref) == 3
    for step, (got, r) in enumerate(zip(shots, ref), 1):
        OC.compare(got, r, f"sgd {case_name} {variant} step {step}", quantities=SGD_Q)
    assert float(shots[1]["skip"]["update"].abs().max()) == 0.0                         # left out of step 2
    assert params["view_pg"].data_ptr() % 16 == 4 and params["view_pg"].grad.data_ptr() % 16 == 4        # the scalar path ran
    assert opt._n_chunks == 4 + 1 + 1 + 2 + 3 + 1 + 2 + 1
    if case_name == "sgd_clip":
        assert float(shots[0]["coef"]) < 1e-3
    else:
        assert float(shots[0]["coef"]) == 1.0 and float(shots[0]["total_norm"]) == 0.0  # not computed
        given = OC.gradients(OC.edge_tensors(_chunk()), RC.SGD_CASES[case_name], 3)
        for name, p in params.items():                                                  # g + wd p is not written back
            assert torch.equal(p.grad.cpu(), given[name]), name
    if variant == "plain":
        assert all("momentum_buffer" not in opt.state.get(p, {}) for p in params.values())


@pytest.mark.parametrize("case_name", list(OC.CASES))
def test_adam_matches_reference(case_name):
    case = OC.CASES[case_name]
    _, opt, shots = _first_adam(case_name)
    ref = RC.adam_reference64(case_name, _chunk())
    assert len(shots) == len(ref) == case.steps
    for step, (got, r) in enumerate(zip(shots, ref), 1):
        OC.compare(got, r, f"adam {case_name} step {step}", quantities=ADAM_Q)
    tensors = OC.edge_tensors(_chunk())
    if case_name in ("clip_idle", "no_clip", "zero_grads", "eps_decides"):          # coef is exactly 1 and .grad keeps its values
        assert float(shots[0]["coef"]) == 1.0
        given = OC.gradients(tensors, case, 1)
        for t in tensors:
            assert torch.equal(shots[0][t.name]["grad"].float().cpu(), given[t.name]), t.name
    if case_name == "clip_active":
        sd = opt.state_dict()["state"]
        assert [int(sd[i]["step"]) for i in range(len(tensors))] == [2 if t.name == "skip" else 3 for t in tensors]
        assert torch.equal(shots[1]["skip"]["exp_avg"], shots[0]["skip"]["exp_avg"])


def _same_bits(a, b, keys):
    (pa, oa, _), (pb, ob, _) = a, b
    for name in pa:
        assert torch.equal(pa[name], pb[name]) and torch.equal(pa[name].grad, pb[name].grad), name
        for k in keys:
            sa, sb = oa.state.get(pa[name], {}).get(k), ob.state.get(pb[name], {}).get(k)
            assert (sa is None and sb is None) or torch.equal(sa, sb), (name, k)
    assert torch.equal(oa.last_grad_norm, ob.last_grad_norm) and torch.equal(oa.last_clip_coef, ob.last_clip_coef)


def test_three_steps_are_bit_identical_from_run_to_run():
    _same_bits(_first_sgd("sgd_clip", "nesterov"), _run_sgd("sgd_clip", "nesterov"), RC.SGD_KEYS)
    _same_bits(_first_sgd("sgd_clip", "dampened"), _run_sgd("sgd_clip", "dampened"), RC.SGD_KEYS)
    _same_bits(_first_adam("clip_active"), _run_adam("clip_active"), RC.ADAM_KEYS)


def test_sgd_state_dict_goes_to_torch_sgd_and_back():
    case_name, variant = "sgd_clip", "dampened"
    case, tensors = RC.SGD_CASES[case_name], OC.edge_tensors(_chunk())
    groups = RC.sgd_groups(case_name, variant)
    ref = RC.sgd_reference64(case_name, variant, _chunk())
    # two steps here ("skip" takes one of them), the third in torch.optim.SGD on the loaded state
    params, opt, _ = _run_sgd(case_name, variant, grad_steps=(1, 2))
    params_t = {name: torch.nn.Parameter(p.detach().clone()) for name, p in params.items()}
    opt_t = RC.torch_sgd(case.max_norm)(groups(tensors, params_t))
    opt_t.opt.load_state_dict(opt.state_dict())
    _, _, shots = RC.run(tensors, case, None, None, RC.SGD_KEYS, params=params_t, opt=opt_t, grad_steps=(3,), **KW)
    OC.compare(shots[0], ref[2], "ours -> torch.optim.SGD, step 3", quantities=SGD_Q)
    # and the reverse
    params_t, opt_t, _ = RC.run(tensors, case, RC.torch_sgd(case.max_norm), groups, RC.SGD_KEYS, grad_steps=(1, 2), **KW)
    params_o = {name: torch.nn.Parameter(p.detach().clone()) for name, p in params_t.items()}
    opt_o = _sgd(case.max_norm)(groups(tensors, params_o))
    opt_o.load_state_dict(opt_t.opt.state_dict())
    _, _, shots = RC.run(tensors, case, None, None, RC.SGD_KEYS, params=params_o, opt=opt_o, grad_steps=(3,), **KW)
    torch.cuda.synchronize()
    OC.compare(shots[0], ref[2], "torch.optim.SGD -> ours, step 3", quantities=SGD_Q)
    sd, sd_t = opt_o.state_dict(), opt_t.opt.state_dict()
    assert set(sd["param_groups"][0]) == set(sd_t["param_groups"][0])
    assert all(set(sd["state"][i]) == {"momentum_buffer"} for i in range(len(tensors)))                 # no step key, as in torch


def test_a_tensor_that_never_stepped_round_trips_without_state():
    tensors = OC.edge_tensors(_chunk())
    case = OC.Case("skip_first", 0.0, 1, ("randn", 1.0), {1: ("skip",)})
    skip = [t.name for t in tensors].index("skip")
    for make, torch_make, groups, keys in ((_sgd, RC.torch_sgd, RC.sgd_groups("sgd_no_clip", "momentum"), RC.SGD_KEYS),
                                           (_adam, RC.torch_adam, OC.groups_of, RC.ADAM_KEYS)):
        params, opt, _ = RC.run(tensors, case, make(0.0), groups, keys, **KW)
        sd = opt.state_dict()
        assert sorted(sd["state"]) == [i for i in range(len(tensors)) if i != skip]
        params_t = {name: torch.nn.Parameter(p.detach().clone()) for name, p in params.items()}
        opt_t = torch_make(0.0)(groups(tensors, params_t))
        opt_t.opt.load_state_dict(sd)
        assert skip not in opt_t.opt.state_dict()["state"]
        opt_o = make(0.0)(groups(tensors, {name: torch.nn.Parameter(p.detach().clone()) for name, p in params.items()}))
        opt_o.load_state_dict(opt_t.opt.state_dict())
        back = opt_o.state_dict()
        assert sorted(back["state"]) == sorted(sd["state"])
        for i in sd["state"]:
            for k in keys:
                assert torch.equal(back["state"][i][k], sd["state"][i][k]), (i, k)
            if "step" in sd["state"][i]:
                assert float(back["state"][i]["step"]) == float(sd["state"][i]["step"]) == 1.0


def test_adam_state_dict_goes_to_torch_adam_and_back():
    case, tensors = OC.CASES["clip_active"], OC.edge_tensors(_chunk())
    ref = RC.adam_reference64("clip_active", _chunk())
    params, opt, _ = _run_adam("clip_active", grad_steps=(1, 2))
    params_t = {name: torch.nn.Parameter(p.detach().clone()) for name, p in params.items()}
    opt_t = RC.torch_adam(case.max_norm)(OC.groups_of(tensors, params_t))
    opt_t.opt.load_state_dict(opt.state_dict())
    _, _, shots = RC.run(tensors, case, None, None, RC.ADAM_KEYS, params=params_t, opt=opt_t, grad_steps=(3,), **KW)
    OC.compare(shots[0], ref[2], "ours -> torch.optim.Adam, step 3", quantities=ADAM_Q)
    params_t, opt_t, _ = RC.run(tensors, case, RC.torch_adam(case.max_norm), OC.groups_of, RC.ADAM_KEYS, grad_steps=(1, 2), **KW)
    params_o = {name: torch.nn.Parameter(p.detach().clone()) for name, p in params_t.items()}
    opt_o = _adam(case.max_norm)(OC.groups_of(tensors, params_o))
    opt_o.load_state_dict(opt_t.opt.state_dict())
    _, _, shots = RC.run(tensors, case, None, None, RC.ADAM_KEYS, params=params_o, opt=opt_o, grad_steps=(3,), **KW)
    torch.cuda.synchronize()
    OC.compare(shots[0], ref[2], "torch.optim.Adam -> ours, step 3", quantities=ADAM_Q)
    sd = opt_o.state_dict()
    assert [int(sd["state"][i]["step"]) for i in range(len(tensors))] == [2 if t.name == "skip" else 3 for t in tensors]
    assert set(sd["param_groups"][0]) == set(opt_t.opt.state_dict()["param_groups"][0])


def test_ucn_recipe_on_multi_tensor_groups_under_a_scheduler():
    """build_ucn_optimizer over a stand-in of ~20 tensors in the reference's two groups, MultiStepLR with its milestone at step 2,
    against torch.optim.SGD over the same groups in float64.  lr 0.05 and weight decay 0.3 with gradients ~ 1: the update stands
    clear of the fp32 rounding of p (|p| <= 1: 6e-8 against 0.05) and the decay adds up to a third of the gradient."""
    from unseenobjectswithmeanshift_amd.optim import SGD, build_ucn_optimizer, build_ucn_param_groups
    torch.manual_seed(3)
    net = RC.StandIn()
    ref_net = RC.StandIn().double()
    ref_net.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
    net = net.to(DEV)
    opt = build_ucn_optimizer(net, "sgd", lr=0.05, momentum=0.9, weight_decay=0.3)
    ref_opt = torch.optim.SGD(build_ucn_param_groups(ref_net, 0.3), 0.05, momentum=0.9, foreach=False)
    assert isinstance(opt, SGD) and [len(g["params"]) for g in opt.param_groups] == [len(g["params"]) for g in ref_opt.param_groups]
    got_p = [p for g in opt.param_groups for p in g["params"]]
    ref_p = [p for g in ref_opt.param_groups for p in g["params"]]
    assert len(got_p) == len(list(net.parameters())) == 18 and [p.shape for p in got_p] == [p.shape for p in ref_p]
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[2], gamma=0.1)
    ref_sched = torch.optim.lr_scheduler.MultiStepLR(ref_opt, milestones=[2], gamma=0.1)
    gen = torch.Generator().manual_seed(5)
    uploads = []
    for step in (1, 2, 3):
        before = [p.detach().double().clone() for p in got_p]
        ref_before = [p.detach().clone() for p in ref_p]
        for p, r in zip(got_p, ref_p):
            g = torch.randn(r.shape, generator=gen)
            r.grad = g.double()
            if p.grad is None:
                p.grad = g.to(DEV)
            else:
                p.grad.copy_(g)
        opt.step(), ref_opt.step()
        sched.step(), ref_sched.step()
        uploads.append(opt.uploads)
        worst = dict(update=0.0, momentum_buffer=0.0)
        for i, (p, r) in enumerate(zip(got_p, ref_p)):
            pairs = dict(update=(p.detach().double() - before[i], r.detach() - ref_before[i]),
                         momentum_buffer=(opt.state[p]["momentum_buffer"], ref_opt.state[r]["momentum_buffer"]))
            for q, (a, b) in pairs.items():
                b = b.to(DEV)
                err, scale = float((a.double() - b).abs().max()), float(b.abs().max())
                worst[q] = max(worst[q], err / scale)
                assert err <= OC.RTOL * scale, (step, i, q, err, scale)
        print(f"optim ucn recipe step {step}: " + ", ".join(f"{q} {v:.2e}" for q, v in worst.items()))
    assert opt.param_groups[0]["lr"] == pytest.approx(0.005) and uploads == [1, 1, 2]      # the table, then the rows at the milestone


@pytest.mark.parametrize("rule", ["sgd", "adam"])
def test_step_and_zero_grad_do_not_wait_and_allocate_nothing(rule):
    if rule == "sgd":
        params, opt, _ = _run_sgd("sgd_clip", "nesterov", grad_steps=(1,))           # the warm-up step
    else:
        params, opt, _ = _run_adam("clip_active", grad_steps=(1,))
    torch.cuda.synchronize()
    uploads = opt.uploads
    allocations = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step()
        opt.zero_grad(set_to_none=False)
        assert torch.cuda.memory_stats(DEV)["allocation.all.allocated"] == allocations
        opt.param_groups[3]["lr"] *= 0.5                                # a scheduler's write: an upload, still no wait
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert opt.uploads == uploads + 1
    assert all(torch.isfinite(p).all() for p in params.values())
    assert all(float(p.grad.abs().max()) == 0.0 for p in params.values())


def test_refusals_on_the_device():
    from unseenobjectswithmeanshift_amd.optim import SGD, Adam
    for make in (lambda ps, **kw: SGD(ps, 1e-2, **kw), lambda ps, **kw: Adam(ps, **kw)):
        with pytest.raises(NotImplementedError, match=r"torch\.float64"):
            make([torch.nn.Parameter(torch.zeros(3, device=DEV, dtype=torch.float64))])
        p = torch.nn.Parameter(torch.zeros(4, 6, device=DEV))
        opt = make([p])
        p.grad = torch.ones(6, 4, device=DEV).t()
        with pytest.raises(RuntimeError, match="parameter 0.*not contiguous"):
            opt.step()
        p.grad = None
        opt.step()                                                   # nothing has a gradient: nothing to do, as in torch
        assert float(p.detach().abs().max()) == 0.0 and opt.state_dict()["state"] == {}
    with pytest.raises(ValueError, match="Nesterov"):
        SGD([torch.nn.Parameter(torch.zeros(3, device=DEV))], 1e-2, momentum=0.9, dampening=0.1, nesterov=True)
    with pytest.raises(NotImplementedError, match="amsgrad"):
        Adam([torch.nn.Parameter(torch.zeros(3, device=DEV))], amsgrad=True)
    p = torch.nn.Parameter(torch.zeros(3, device=DEV))
    opt = SGD([p], 1e-2, momentum=0.9)
    p.grad = torch.ones(3, device=DEV)
    opt.param_groups[0].update(nesterov=True, dampening=0.5)          # set behind the constructor's back: refused at the step
    with pytest.raises(ValueError, match="Nesterov"):
        opt.step()
    assert float(p.detach().abs().max()) == 0.0


def test_ucn_embedding_losses_with_the_ucn_optimizer(monkeypatch):
    """Recipe (1) as one call and one step.  The losses are EmbeddingLoss(ucn_backbone_forward_train(network, image, depth), label)
    bit for bit: the call reaches ucn_backbone_forward_train once, with exactly these arguments and no keyword, the features it
    returns are that call's result itself (the same object, nothing done to it), and EmbeddingLoss of that tensor gives the three
    losses' bits.  (A second forward is not taken: tests/test_gpu_ucn_training.py::test_forward_train_is_the_composition records
    that two runs of the library convolutions and batch statistics do not repeat their bits on this GPU.)  Every parameter with a
    gradient moves."""
    from test_backbone_cpu import make_backbone
    from unseenobjectswithmeanshift_amd import training as tr
    from unseenobjectswithmeanshift_amd.embedding_loss import EmbeddingLoss
    from unseenobjectswithmeanshift_amd.optim import build_ucn_optimizer
    net = make_backbone(DEV).train()
    net.miopen_find = False
    gen = torch.Generator().manual_seed(11)
    image, depth = torch.randn(2, 3, 32, 32, generator=gen).to(DEV), torch.randn(2, 3, 32, 32, generator=gen).to(DEV)
    label = torch.zeros(2, 1, 32, 32)
    label[:, :, 4:14, 4:14], label[:, :, 18:30, 10:28] = 1.0, 2.0
    label = label.to(DEV)
    emb = EmbeddingLoss(0.02, 0.5, 1.0, 1.0)
    forward, calls, returned = tr.ucn_backbone_forward_train, [], []

    def spy(*args, **kw):
        calls.append((args, kw))
        returned.append(forward(*args, **kw))
        return returned[-1]

    monkeypatch.setattr(tr, "ucn_backbone_forward_train", spy)
    opt = build_ucn_optimizer(net, "sgd", lr=0.05)
    loss, intra, inter, features = tr.ucn_embedding_losses(net, image, label, depth, embedding_loss=emb)
    assert len(calls) == 1 and calls[0][1] == {} and len(calls[0][0]) == 3
    assert calls[0][0][0] is net and calls[0][0][1] is image and calls[0][0][2] is depth
    assert features is returned[0] and features._version == 0          # the call's own result, not touched in place
    assert features.shape == (2, 64, 32, 32) and features.requires_grad
    again = emb(features.detach(), label)
    assert all(torch.equal(a, b.detach()) for a, b in zip(again, (loss, intra, inter)))
    assert float(loss) > 0
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    opt.zero_grad()
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    with_grad = [n for n, p in net.named_parameters() if p.grad is not None and float(p.grad.abs().max()) > 0]
    assert len(with_grad) >= 200                                       # both towers: the gradient reaches the depth tower too
    assert all(not torch.equal(before[n], p.detach()) for n, p in net.named_parameters() if n in with_grad)


def test_a_group_that_starts_to_keep_a_buffer_takes_torchs_first_step():
    """momentum 0 for a step, then 0.9 with dampening 0.5: torch's buffer is None at the second step, so buf = d, undampened, although
    the tensors have stepped before; the third step is dampened.  Against torch.optim.SGD in float64 on the same groups."""
    from unseenobjectswithmeanshift_amd.optim import SGD
    gen = torch.Generator().manual_seed(9)
    shapes = [(5,), (_chunk() + 3,), (7, 3)]
    start = [0.25 * torch.randn(s, generator=gen) for s in shapes]
    got_p = [torch.nn.Parameter(v.to(DEV)) for v in start]
    ref_p = [torch.nn.Parameter(v.double()) for v in start]
    kw = dict(lr=0.05, momentum=0.0, dampening=0.0, weight_decay=0.3)
    opt, ref = SGD(got_p, **kw), torch.optim.SGD(ref_p, foreach=False, **kw)
    for step in (1, 2, 3):
        if step == 2:
            for o in (opt, ref):
                o.param_groups[0].update(momentum=0.9, dampening=0.5)
        before = [p.detach().double().clone() for p in got_p]
        ref_before = [p.detach().clone() for p in ref_p]
        for p, r in zip(got_p, ref_p):
            g = torch.randn(r.shape, generator=gen)
            p.grad, r.grad = g.to(DEV), g.double()
        opt.step(), ref.step()
        for i, (p, r) in enumerate(zip(got_p, ref_p)):
            pairs = [(p.detach().double() - before[i], r.detach() - ref_before[i])]
            if step > 1:
                pairs.append((opt.state[p]["momentum_buffer"].double(), ref.state[r]["momentum_buffer"]))
            for a, b in pairs:
                b = b.to(DEV)
                assert float((a - b).abs().max()) <= OC.RTOL * float(b.abs().max()), (step, i)
    assert opt._steps_dev.tolist() == [2, 2, 2]                      # counted from the step that made the buffer
