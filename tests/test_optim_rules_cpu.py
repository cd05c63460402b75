"""What the cases of tests/optim_rule_cases.py must hold before any kernel is involved, and the host side of optim.SGD / optim.Adam:
the float64 restatements are torch's, the cases tell the rules apart, torch's own fp32 run meets the contract the kernels are held
to, the UCN param groups are the reference's, the header declares and _lib binds the rule entries, the refusals are named.
No GPU; the ABI test needs the built library."""
import math

import pytest
import torch
from torch import nn

import optim_cases as OC
import optim_rule_cases as RC
from unseenobjectswithmeanshift_amd import _lib

CHUNK = 8192


def _final_p(shots_params):
    return {name: p.detach() for name, p in shots_params.items()}


@pytest.mark.parametrize("case_name", list(RC.SGD_CASES))
@pytest.mark.parametrize("variant", list(RC.SGD_VARIANTS))
def test_sgd64_is_torch_sgd(variant, case_name):
    tensors, case = OC.edge_tensors(CHUNK), RC.SGD_CASES[case_name]
    params, _, _ = RC.run(tensors, case, RC.torch_sgd(case.max_norm), RC.sgd_groups(case_name, variant), RC.SGD_KEYS)
    mine = RC.formula_run("sgd", tensors, case, RC.sgd_hyper(case_name, variant))
    for name, p in params.items():
        assert float((mine[name] - p.detach()).abs().max()) <= 1e-12 * float(p.detach().abs().max()), (variant, case_name, name)


@pytest.mark.parametrize("case_name", ["clip_active", "no_clip", "eps_decides"])
def test_adam64_is_torch_adam(case_name):
    tensors, case = OC.edge_tensors(CHUNK), OC.CASES[case_name]._replace(steps=3)
    params, _, _ = RC.run(tensors, case, RC.torch_adam(case.max_norm), OC.groups_of, RC.ADAM_KEYS)
    mine = RC.formula_run("adam", tensors, case, RC.adam_hyper)
    for name, p in params.items():
        assert float((mine[name] - p.detach()).abs().max()) <= 1e-12 * float(p.detach().abs().max()), (case_name, name)


def test_weight_decay_rows_tell_adam_from_adamw():
    tensors, case = OC.edge_tensors(CHUNK), OC.CASES["clip_active"]
    start, grads = OC.values(tensors), OC.gradients(tensors, case, 1)
    checked = 0
    for i, t in enumerate(tensors):
        row = OC.ROWS[i % len(OC.ROWS)]
        if row["weight_decay"] == 0:
            continue
        p, g = start[t.name].double(), grads[t.name].double() * 1e-4            # about what clipping leaves
        z = torch.zeros_like(p)
        adam = RC.adam64(p, g, z, z, 1, eps=OC.EPS, **row)[0] - p
        adamw = OC.adamw64(p, g, z, z, 1, eps=OC.EPS, **row)[0] - p
        assert float((adam - adamw).abs().max()) > 100 * OC.RTOL * float(adam.abs().max()), t.name
        checked += 1
    assert checked >= 6


@pytest.mark.parametrize("case_name", list(RC.SGD_CASES))
def test_first_step_tells_the_undampened_buffer_from_the_dampened(case_name):
    tensors, case = OC.edge_tensors(CHUNK), RC.SGD_CASES[case_name]
    start, grads = OC.values(tensors), OC.gradients(tensors, case, 1)
    hyper = RC.sgd_hyper(case_name, "dampened")
    for i, t in enumerate(tensors):
        p, g = start[t.name].double(), grads[t.name].double()
        first = RC.sgd64(p, g, None, True, **hyper(i))[0] - p
        dampened = RC.sgd64(p, g, torch.zeros_like(p), False, **hyper(i))[0] - p           # buf = (1 - dampening) g from a zero buffer
        assert float((first - dampened).abs().max()) > 100 * OC.RTOL * float(first.abs().max()), t.name


def test_weight_decay_is_resolved_in_every_sgd_case():
    """Dropping weight decay moves the first update of every decayed tensor by more than 100 RTOL of it."""
    for case_name, case in RC.SGD_CASES.items():
        tensors = OC.edge_tensors(CHUNK)
        start, grads = OC.values(tensors), OC.gradients(tensors, case, 1)
        total = math.sqrt(sum(float(g.double().pow(2).sum()) for g in grads.values()))
        coef = min(1.0, case.max_norm / (total + 1e-6)) if case.max_norm > 0 else 1.0
        hyper = RC.sgd_hyper(case_name, "plain")
        for i, t in enumerate(tensors):
            h = hyper(i)
            if h["weight_decay"] == 0:
                continue
            p, g = start[t.name].double(), grads[t.name].double() * coef
            with_wd = RC.sgd64(p, g, None, True, **h)[0] - p
            without = RC.sgd64(p, g, None, True, **dict(h, weight_decay=0.0))[0] - p
            assert float((with_wd - without).abs().max()) > 100 * OC.RTOL * float(with_wd.abs().max()), (case_name, t.name)


@pytest.mark.parametrize("case_name", list(RC.SGD_CASES))
@pytest.mark.parametrize("variant", list(RC.SGD_VARIANTS))
def test_torch_fp32_sgd_meets_the_contract(variant, case_name):
    """The bound is one fp32 arithmetic can meet on these cases: torch's own single-tensor fp32 run on the CPU does."""
    case = RC.SGD_CASES[case_name]
    _, _, shots = RC.run(OC.edge_tensors(CHUNK), case, RC.torch_sgd(case.max_norm), RC.sgd_groups(case_name, variant), RC.SGD_KEYS,
                         dtype=torch.float32)
    ref = RC.sgd_reference64(case_name, variant, CHUNK)
    for step, (got, r) in enumerate(zip(shots, ref), 1):
        OC.compare(got, r, f"torch fp32 sgd {case_name} {variant} step {step}", quantities=("update", "grad") + RC.SGD_KEYS)


@pytest.mark.parametrize("case_name", list(OC.CASES))
def test_torch_fp32_adam_meets_the_contract(case_name):
    case = OC.CASES[case_name]
    _, _, shots = RC.run(OC.edge_tensors(CHUNK), case, RC.torch_adam(case.max_norm), OC.groups_of, RC.ADAM_KEYS, dtype=torch.float32)
    ref = RC.adam_reference64(case_name, CHUNK)
    for step, (got, r) in enumerate(zip(shots, ref), 1):
        OC.compare(got, r, f"torch fp32 adam {case_name} step {step}", quantities=("update", "grad") + RC.ADAM_KEYS)


def test_ucn_param_groups_are_the_reference_two():
    from unseenobjectswithmeanshift_amd.optim import SGD, Adam, build_ucn_optimizer, build_ucn_param_groups
    from unseenobjectswithmeanshift_amd.ucn_backbone import UCNBackbone
    net = UCNBackbone()
    named = list(net.named_parameters())
    groups = build_ucn_param_groups(net)
    assert len(groups) == 2 and all(g["weight_decay"] == 1e-4 and set(g) == {"params", "weight_decay"} for g in groups)
    by_id = {id(p): n for n, p in named}
    assert [by_id[id(p)] for p in groups[0]["params"]] == [n for n, _ in named if "bias" in n]
    assert [by_id[id(p)] for p in groups[1]["params"]] == [n for n, _ in named if "weight" in n]
    ids = [id(p) for g in groups for p in g["params"]]
    assert len(ids) == len(set(ids)) == len(named) and set(ids) == set(by_id)
    assert len(named) > 200                                           # two ResNet34-8s towers
    assert build_ucn_param_groups(net, 0.5)[1]["weight_decay"] == 0.5
    sgd = build_ucn_optimizer(net)
    assert isinstance(sgd, SGD) and isinstance(sgd, torch.optim.Optimizer) and sgd.max_norm == 0.0
    assert [(g["lr"], g["momentum"], g["weight_decay"], len(g["params"])) for g in sgd.param_groups] == [
        (1e-4, 0.9, 1e-4, len(groups[0]["params"])), (1e-4, 0.9, 1e-4, len(groups[1]["params"]))]
    adam = build_ucn_optimizer(net, solver="adam", momentum=0.8, beta=0.99)
    assert isinstance(adam, Adam) and adam.param_groups[0]["betas"] == (0.8, 0.99) and adam.param_groups[1]["lr"] == 1e-4
    with pytest.raises(ValueError, match="solver"):
        build_ucn_optimizer(net, solver="x")


def test_group_keys_are_torchs_and_build_optimizer_has_the_sgd_branch():
    from unseenobjectswithmeanshift_amd.optim import SGD, Adam, FullModelClipAdamW, build_optimizer
    p = lambda: [nn.Parameter(torch.zeros(3))]
    assert set(SGD(p(), 0.1).param_groups[0]) == set(torch.optim.SGD(p(), 0.1).param_groups[0])
    assert set(Adam(p()).param_groups[0]) == set(torch.optim.Adam(p()).param_groups[0])
    assert Adam(p()).param_groups[0]["decoupled_weight_decay"] is False and Adam(p()).max_norm == 0.0
    assert all(c._step_supports_amp_scaling for c in (SGD, Adam, FullModelClipAdamW))
    m = nn.Sequential(nn.Linear(3, 4), nn.LayerNorm(4))
    opt = build_optimizer(m, base_lr=2e-3, max_norm=0.5, optimizer="SGD", momentum=0.8)
    assert isinstance(opt, SGD) and opt.max_norm == 0.5 and len(opt.param_groups) == 4
    assert [(g["lr"], g["weight_decay"], g["momentum"]) for g in opt.param_groups] == [(2e-3, 0.05, 0.8)] * 2 + [(2e-3, 0.0, 0.8)] * 2
    assert isinstance(build_optimizer(m), FullModelClipAdamW)
    with pytest.raises(NotImplementedError, match="LION"):
        build_optimizer(m, optimizer="LION")
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[1], gamma=0.1)
    sched.step()
    assert opt.param_groups[0]["lr"] == pytest.approx(2e-4)


def test_header_declares_and_lib_binds_the_rule_entries():
    from ctypes import c_float, c_int, c_void_p
    P, I = c_void_p, c_int
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    sig, params = _lib._SIGNATURES, _lib._HEADER.params
    assert sig["msm_optim_count_norm"] == (I, [P, P, P, P, P, P, I, I, I, P])
    assert sig["msm_optim_update"] == (I, [I, P, P, P, P, P, P, P, P, I, I, I, c_float, P])
    assert params["msm_optim_update"] == ["rule", "tensors", "chunks", "hyper", "partials", "state", "steps", "grad_scale", "found_inf",
                                          "n_tensors", "n_chunks", "n_rows", "max_norm", "stream"]
    assert {"msm_optim_count_norm", "msm_optim_update"} <= set(_lib.declared_symbols())
    L = _lib.lib()
    assert hasattr(L, "msm_optim_count_norm") and hasattr(L, "msm_optim_update")
    assert L.msm_abi_version() == _lib.ABI_VERSION == _lib.parse_header(text).abi_version >= 43
    from unseenobjectswithmeanshift_amd import ops
    assert ops.OPTIM_RULES == {"adamw": _lib._define(text, "MSM_OPTIM_ADAMW"), "adam": _lib._define(text, "MSM_OPTIM_ADAM"),
                               "sgd": _lib._define(text, "MSM_OPTIM_SGD")}
    # refused before any launch
    assert L.msm_optim_update(7, P(8), P(8), P(8), P(8), P(8), P(8), None, None, 1, 1, 1, c_float(0.0), None) != 0
    assert b"rule = 7" in L.msm_last_error_string()
    assert L.msm_optim_update(2, P(8), P(8), P(8), None, P(8), P(8), None, None, 1, 1, 1, c_float(0.01), None) != 0
    assert b"partials" in L.msm_last_error_string()
    assert L.msm_optim_count_norm(P(8), P(8), P(8), P(8), P(6), None, 1, 1, 1, None) != 0
    assert b"4-byte aligned" in L.msm_last_error_string()
    assert L.msm_optim_count_norm(P(8), P(8), P(8), None, None, None, 1, 1, 1, None) != 0
    assert b"null pointer" in L.msm_last_error_string()


def _classes():
    from unseenobjectswithmeanshift_amd.optim import SGD, Adam
    return {"SGD": lambda params, **kw: SGD(params, 1e-2, **kw), "Adam": lambda params, **kw: Adam(params, **kw)}


@pytest.mark.parametrize("cls", ["SGD", "Adam"])
def test_constructor_refusals_are_named(cls):
    make = _classes()[cls]
    p = lambda *a, **kw: [nn.Parameter(torch.zeros(*(a or (3,)), **kw))]
    with pytest.raises(NotImplementedError, match="maximize"):
        make(p(), maximize=True)
    for dtype in (torch.float64, torch.bfloat16, torch.float16):
        with pytest.raises(NotImplementedError, match=f"{cls}.*" + str(dtype).replace(".", r"\.")):
            make(p() + p(2, 2, dtype=dtype))
    with pytest.raises(RuntimeError, match=f"{cls}.*contiguous"):
        make([nn.Parameter(torch.zeros(4, 3).t())])
    with pytest.raises(NotImplementedError, match="closure"):
        make(p()).step(lambda: 0.0)
    with pytest.raises(ValueError, match="weight_decay"):
        make(p(), weight_decay=-1.0)


def test_adam_refuses_amsgrad_and_sgd_torchs_nesterov_rule():
    from unseenobjectswithmeanshift_amd.optim import SGD, Adam
    p = lambda: [nn.Parameter(torch.zeros(3))]
    with pytest.raises(NotImplementedError, match="amsgrad"):
        Adam(p(), amsgrad=True)
    with pytest.raises(ValueError, match="betas"):
        Adam(p(), betas=(1.0, 0.9))
    with pytest.raises(ValueError, match="Nesterov momentum requires a momentum and zero dampening"):
        SGD(p(), 0.1, momentum=0.9, dampening=0.5, nesterov=True)
    with pytest.raises(ValueError, match="Nesterov"):
        SGD(p(), 0.1, nesterov=True)
    with pytest.raises(ValueError, match="momentum"):
        SGD(p(), 0.1, momentum=-0.5)
    with pytest.raises(ValueError, match="learning rate"):
        SGD(p(), -0.1)


@pytest.mark.parametrize("cls", ["SGD", "Adam"])
def test_a_host_tensor_raises_the_gpu_error_at_step(cls):
    p = nn.Parameter(torch.zeros(3))
    opt = _classes()[cls]([p])
    p.grad = torch.ones(3)
    with pytest.raises(RuntimeError, match=f"{cls}.*must be on the GPU"):
        opt.step()
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        opt.zero_grad(set_to_none=False)
    assert torch.equal(p.detach(), torch.zeros(3)) and p not in opt.state
