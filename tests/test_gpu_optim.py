"""FullModelClipAdamW on the GPU (csrc/optimizer.hip through unseenobjectswithmeanshift_amd.optim) against the float64 reference of
tests/optim_cases.py: clip_grad_norm_ + torch.optim.AdamW(foreach=False) over the same groups on the CPU.

Bound: the project's fp32 contract per tensor, max|got - ref64| <= 1e-4 max|ref64| with no element left out, for
exp_avg, exp_avg_sq, the clipped .grad, the update p_after - p_before, total_norm and coef.  torch's own fp32 CPU run of the same
cases sits at <= 2e-6 (1.3e-5 for the pure weight-decay update; tests/test_optim_cases_cpu.py); the kernels' figures are printed
(pytest -s) and recorded in DESIGN.md section 5u.  Needs a real MI355X (pytest -m gpu)."""
import functools

import pytest
import torch

import optim_cases as OC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _chunk():
    from unseenobjectswithmeanshift_amd import ops
    return ops.optim_chunk()


def _ours(max_norm):
    from unseenobjectswithmeanshift_amd.optim import FullModelClipAdamW
    return lambda groups: FullModelClipAdamW(groups, max_norm=max_norm)


def _run(name, **kw):
    case = OC.CASES[name]
    out = OC.run(OC.edge_tensors(_chunk()), case, _ours(case.max_norm), device=DEV, dtype=torch.float32, **kw)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _first(name):
    return _run(name)


def test_edge_table_layout_reaches_every_path():
    params, opt, _ = _first("clip_active")
    chunk = _chunk()
    assert opt.chunk == chunk
    assert params["view_pg"].data_ptr() % 16 == 4 and params["view_pg"].grad.data_ptr() % 16 == 4        # the scalar path
    assert params["view_p"].data_ptr() % 16 == 4 and params["view_p"].grad.data_ptr() % 16 == 0
    assert params[f"n{chunk}"].data_ptr() % 16 == 0
    assert opt._n_tensors == len(params) and opt._n_chunks == 4 + 1 + 1 + 2 + 3 + 1 + 2 + 1        # ceil(numel / chunk) per tensor


@pytest.mark.parametrize("name", list(OC.CASES))
def test_matches_reference(name):
    case = OC.CASES[name]
    _, opt, shots = _first(name)
    ref = OC.reference64(name, _chunk())
    assert len(shots) == len(ref) == case.steps
    for step, (got, r) in enumerate(zip(shots, ref), 1):
        OC.compare(got, r, f"{name} step {step}")
    tensors = OC.edge_tensors(_chunk())
    if name in ("clip_idle", "no_clip", "zero_grads", "eps_decides"):                  # coef is exactly 1 and .grad keeps its values
        assert float(shots[0]["coef"]) == 1.0
        given = OC.gradients(tensors, case, 1)
        for t in tensors:
            assert torch.equal(shots[0][t.name]["grad"].float().cpu(), given[t.name]), t.name
    if name == "no_clip":
        assert float(shots[0]["total_norm"]) == 0.0                                     # not computed
    if name == "clip_active":
        assert float(shots[0]["coef"]) < 1e-3
        assert float(shots[1]["skip"]["update"].abs().max()) == 0.0                     # left out of step 2 ...
        assert torch.equal(shots[1]["skip"]["exp_avg"], shots[0]["skip"]["exp_avg"])    # ... state untouched ...
        sd = opt.state_dict()["state"]
        steps = [int(sd[i]["step"]) for i in range(len(tensors))]
        assert steps == [2 if t.name == "skip" else 3 for t in tensors]                 # ... and no step counted


def test_three_steps_are_bit_identical_from_run_to_run():
    params_a, _, _ = _first("clip_active")
    params_b, opt_b, _ = _run("clip_active")
    opt_a = _first("clip_active")[1]
    for name in params_a:
        assert torch.equal(params_a[name], params_b[name]) and torch.equal(params_a[name].grad, params_b[name].grad), name
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(opt_a.state[params_a[name]][k], opt_b.state[params_b[name]][k]), (name, k)
    assert torch.equal(opt_a.last_grad_norm, opt_b.last_grad_norm) and torch.equal(opt_a.last_clip_coef, opt_b.last_clip_coef)


def test_zero_grad_in_place_keeps_addresses_and_uploads_nothing():
    case = OC.CASES["clip_active"]
    tensors = OC.edge_tensors(_chunk())
    params, opt, _ = _run("clip_active", steps=1)
    addresses = {name: p.grad.data_ptr() for name, p in params.items()}
    uploads = opt.uploads
    opt.zero_grad(set_to_none=False)
    for name, p in params.items():
        assert p.grad is not None and p.grad.data_ptr() == addresses[name] and float(p.grad.abs().max()) == 0.0, name
    assert opt.uploads == uploads
    # step 2 leaves "skip" out (one upload: the table changes), step 3 brings it back with a new gradient tensor (one more)
    _, _, shots = OC.run(tensors, case, None, device=DEV, dtype=torch.float32, params=params, opt=opt, first_step=2)
    assert opt.uploads == uploads + 2
    # gradients dropped and made again: new addresses, the step still matches
    opt.zero_grad()
    assert all(p.grad is None for p in params.values())
    ref = OC.reference64("clip_active", _chunk(), 4)
    _, _, more = OC.run(tensors, case, None, device=DEV, dtype=torch.float32, params=params, opt=opt, first_step=4, steps=4)
    assert opt.uploads == uploads + 3
    for step, (got, r) in enumerate(zip(shots + more, ref[1:]), 2):
        OC.compare(got, r, f"after zero_grad, step {step}")
    # an lr change alone uploads the rows, once
    opt.zero_grad(set_to_none=False)
    opt.param_groups[0]["lr"] *= 0.5
    opt.step()
    assert opt.uploads == uploads + 4
    opt.step()
    assert opt.uploads == uploads + 4


def test_step_and_zero_grad_do_not_wait_for_the_gpu():
    params, opt, _ = _run("clip_active", steps=1)                    # the warm-up step
    torch.cuda.synchronize()
    uploads = opt.uploads
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step()
        opt.zero_grad(set_to_none=False)
        opt.param_groups[3]["lr"] = 0.07                             # a scheduler's write: an upload, still no wait
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert opt.uploads == uploads + 1
    assert all(torch.isfinite(p).all() for p in params.values())


def _torch_gpu(max_norm):
    return lambda groups: OC.ClippedTorchAdamW(groups, max_norm, foreach=False)


def test_state_dict_goes_to_torch_adamw_and_back():
    case = OC.CASES["clip_active"]
    tensors = OC.edge_tensors(_chunk())
    ref = OC.reference64("clip_active", _chunk())
    kw = dict(device=DEV, dtype=torch.float32)
    # two steps here ("skip" takes one of them), the third in torch.optim.AdamW on the loaded state
    params, opt, _ = _run("clip_active", steps=2)
    params_t = {name: torch.nn.Parameter(p.detach().clone()) for name, p in params.items()}
    opt_t = _torch_gpu(case.max_norm)(OC.groups_of(tensors, params_t))
    opt_t.opt.load_state_dict(opt.state_dict())
    _, _, shots = OC.run(tensors, case, None, params=params_t, opt=opt_t, first_step=3, **kw)
    OC.compare(shots[0], ref[2], "ours -> torch.optim.AdamW, step 3")
    # and the reverse
    params_t, opt_t, _ = OC.run(tensors, case, _torch_gpu(case.max_norm), steps=2, **kw)
    params_o = {name: torch.nn.Parameter(p.detach().clone()) for name, p in params_t.items()}
    opt_o = _ours(case.max_norm)(OC.groups_of(tensors, params_o))
    opt_o.load_state_dict(opt_t.opt.state_dict())
    _, _, shots = OC.run(tensors, case, None, params=params_o, opt=opt_o, first_step=3, **kw)
    torch.cuda.synchronize()
    OC.compare(shots[0], ref[2], "torch.optim.AdamW -> ours, step 3")
    sd = opt_o.state_dict()
    assert [int(sd["state"][i]["step"]) for i in range(len(tensors))] == [2 if t.name == "skip" else 3 for t in tensors]
    assert set(sd["param_groups"][0]) == set(opt_t.opt.state_dict()["param_groups"][0])


def test_realistic_table_of_the_rgbd_head():
    """The 125 tensors / 9.9 M parameters of build_ucn_head() in the reference's groups, max_norm 0.01, two steps; compared on the
    device in float64."""
    from unseenobjectswithmeanshift_amd.meta_arch import build_ucn_head
    from unseenobjectswithmeanshift_amd.optim import build_optimizer, build_param_groups
    torch.manual_seed(0)
    head = build_ucn_head()
    ref_head = build_ucn_head().double()
    ref_head.load_state_dict({k: v.double() for k, v in head.state_dict().items()})
    head = head.to(DEV)
    opt = build_optimizer(head, base_lr=0.05, max_norm=0.01)
    ref_opt = OC.ClippedTorchAdamW(build_param_groups(ref_head, 0.05), 0.01, lr=0.05, foreach=False)
    got_p = [g["params"][0] for g in opt.param_groups]
    ref_p = [g["params"][0] for g in ref_opt.opt.param_groups]
    assert len(got_p) == len(ref_p) == 125 and sum(p.numel() for p in got_p) == 9886979
    assert [(g["lr"], g["weight_decay"]) for g in opt.param_groups] == [(g["lr"], g["weight_decay"]) for g in ref_opt.opt.param_groups]
    gen = torch.Generator().manual_seed(5)
    for step in (1, 2):
        before = [p.detach().double().clone() for p in got_p]
        ref_before = [p.detach().clone() for p in ref_p]
        for p, r in zip(got_p, ref_p):
            g = 1e-3 * torch.randn(r.shape, generator=gen)
            r.grad = g.double()
            if p.grad is None:
                p.grad = g.to(DEV)
            else:
                p.grad.copy_(g)
        opt.step()
        ref_opt.step()
        worst = dict(update=0.0, exp_avg=0.0, exp_avg_sq=0.0, grad=0.0)
        for i, (p, r) in enumerate(zip(got_p, ref_p)):
            pairs = dict(update=(p.detach().double() - before[i], r.detach() - ref_before[i]),
                         exp_avg=(opt.state[p]["exp_avg"], ref_opt.state[r]["exp_avg"]),
                         exp_avg_sq=(opt.state[p]["exp_avg_sq"], ref_opt.state[r]["exp_avg_sq"]), grad=(p.grad, r.grad))
            for q, (a, b) in pairs.items():
                b = b.to(DEV)
                err, scale = float((a.double() - b).abs().max()), float(b.abs().max())
                worst[q] = max(worst[q], err / scale)
                assert err <= OC.RTOL * scale, (step, i, q, err, scale)
        norm, coef = float(opt.last_grad_norm), float(opt.last_clip_coef)
        ref_norm, ref_coef = float(ref_opt.last_grad_norm), float(ref_opt.last_clip_coef)
        print(f"optim ucn head step {step}: " + ", ".join(f"{q} {v:.2e}" for q, v in worst.items())
              + f", total_norm {abs(norm - ref_norm) / ref_norm:.2e}, coef {abs(coef - ref_coef) / ref_coef:.2e}")
        assert abs(norm - ref_norm) <= OC.RTOL * ref_norm and abs(coef - ref_coef) <= OC.RTOL * ref_coef
    assert opt.uploads == 1


def test_refusals_on_the_device():
    from unseenobjectswithmeanshift_amd.optim import FullModelClipAdamW
    p = torch.nn.Parameter(torch.zeros(4, 6, device=DEV))
    opt = FullModelClipAdamW([p], lr=1e-2)
    p.grad = torch.ones(6, 4, device=DEV).t()
    with pytest.raises(RuntimeError, match="parameter 0.*not contiguous"):
        opt.step()
    p.grad = None
    opt.step()                                                       # nothing has a gradient: nothing to do, as in torch
    assert float(p.detach().abs().max()) == 0.0 and opt.state_dict()["state"] == {}
