"""Cases for optim.SGD and optim.Adam (tests/test_gpu_optim_rules.py and tests/test_gpu_optim_scaler.py on the GPU,
tests/test_optim_rules_cpu.py for what the cases themselves must hold), on the tables, gradients and contract of tests/optim_cases.py:
the edge table, ``RTOL = 1e-4`` of max|ref64| per tensor with no element left out, the update held and not p.

The float64 reference is ``torch.nn.utils.clip_grad_norm_`` followed by ``torch.optim.SGD`` / ``torch.optim.Adam`` (foreach=False)
over the same groups on the CPU.  ``sgd64`` / ``adam64`` restate one step of each from the formulas of include/msm_hip.h.

Adam runs ``optim_cases.CASES`` on ``optim_cases.ROWS``: its update is of the size of lr whatever the gradient, as AdamW's.  SGD's
update is lr times the gradient, so its cases carry rows of their own, chosen so that the update again stands clear of the fp32
rounding of p (2^-24 |p|, |p| ~ 0.25): clipped to a whole-model norm of 0.01 an element of the gradient is about 5e-5, and a learning
rate of 60 to 200 makes the update 3e-3 to 1e-2; weight decay of 2e-4 to 1e-3 then adds about as much to the gradient as the gradient
itself (wd |p| ~ 5e-5 to 2.5e-4), so a kernel that drops or misplaces it misses the bound.  Unclipped (elements ~ 1) the learning
rates are those of optim_cases and the weight decay 0.3 to 0.5 (wd |p| ~ 0.1 of the gradient).
tests/test_optim_rules_cpu.py holds torch's own fp32 run of every case to the same contract: what the kernels are asked for, fp32
arithmetic can give."""
import functools
import math

import torch

import optim_cases as OC

SGD_VARIANTS = {
    "plain": dict(momentum=0.0, dampening=0.0, nesterov=False),
    "momentum": dict(momentum=0.9, dampening=0.0, nesterov=False),
    "dampened": dict(momentum=0.9, dampening=0.5, nesterov=False),
    "nesterov": dict(momentum=0.9, dampening=0.0, nesterov=True),
}
# tensor i of a table takes row i % 3; one row of each set has no weight decay
SGD_ROWS_CLIPPED = (dict(lr=100.0, weight_decay=2e-4), dict(lr=60.0, weight_decay=0.0), dict(lr=200.0, weight_decay=1e-3))
SGD_ROWS = (dict(lr=0.05, weight_decay=0.5), dict(lr=0.03, weight_decay=0.0), dict(lr=0.1, weight_decay=0.3))
SGD_CASES = {c.name: c for c in (
    OC.Case("sgd_clip", 0.01, 3, ("randn", 1.0), {2: ("skip",)}),          # norm ~ 2e2 >> max_norm: clipping is active
    OC.Case("sgd_no_clip", 0.0, 3, ("randn", 1.0), {2: ("skip",)}),
)}
SGD_CASE_ROWS = {"sgd_clip": SGD_ROWS_CLIPPED, "sgd_no_clip": SGD_ROWS}
SGD_KEYS = ("momentum_buffer",)
ADAM_KEYS = ("exp_avg", "exp_avg_sq")


def sgd_groups(case_name, variant):
    rows = SGD_CASE_ROWS[case_name]
    return lambda tensors, params: [dict(params=[params[t.name]], **rows[i % len(rows)], **SGD_VARIANTS[variant])
                                    for i, t in enumerate(tensors)]


class ClippedTorch:
    """clip_grad_norm_ over every parameter (max_norm > 0), then the torch optimizer ``cls``."""

    def __init__(self, cls, groups, max_norm, **kw):
        self.opt = cls(groups, **kw)
        self.max_norm = max_norm
        self.last_grad_norm = self.last_clip_coef = None

    def step(self):
        if self.max_norm > 0:
            params = [p for g in self.opt.param_groups for p in g["params"]]
            self.last_grad_norm = torch.nn.utils.clip_grad_norm_(params, self.max_norm).detach().clone()
            self.last_clip_coef = torch.clamp(self.max_norm / (self.last_grad_norm + 1e-6), max=1.0)
        else:
            self.last_grad_norm, self.last_clip_coef = None, torch.ones(())
        self.opt.step()

    @property
    def state(self):
        return self.opt.state


def snapshot(params, opt, before, keys):
    """What the contract holds after a step, as float64 on the parameters' device."""
    out = {}
    for name, p in params.items():
        st = opt.state.get(p, {})
        out[name] = dict(update=p.detach().double() - before[name], grad=None if p.grad is None else p.grad.double().clone())
        for k in keys:
            out[name][k] = st[k].double().clone() if st.get(k) is not None else None
    norm, coef = opt.last_grad_norm, opt.last_clip_coef
    out["total_norm"] = None if norm is None else norm.double().clone()
    out["coef"] = coef.double().clone()
    return out


def run(tensors, case, make_opt, groups, keys, device="cpu", dtype=torch.float64, seed=0, grad_steps=None, params=None, opt=None,
        pre_step=None):
    """Run `case` on `tensors`: make_opt(groups(tensors, params)) -> an object with step(), state, last_grad_norm, last_clip_coef.
    grad_steps: the 1-based gradient sets to step on, in order (default 1 .. case.steps); pre_step(i, params, opt) is called with
    the gradients of iteration i in place.  Returns (params, opt, [snapshot per step])."""
    if params is None:
        params = OC.make_params(tensors, device, dtype, seed)
        opt = make_opt(groups(tensors, params))
    shots = []
    for i, step in enumerate(grad_steps or range(1, case.steps + 1)):
        OC.set_grads(params, OC.gradients(tensors, case, step, seed), device)
        if pre_step is not None:
            pre_step(i, params, opt)
        before = {name: p.detach().double().clone() for name, p in params.items()}
        opt.step()
        shots.append(snapshot(params, opt, before, keys))
    return params, opt, shots


def torch_sgd(max_norm, **kw):
    return lambda groups: ClippedTorch(torch.optim.SGD, groups, max_norm, foreach=False, **kw)


def torch_adam(max_norm, **kw):
    return lambda groups: ClippedTorch(torch.optim.Adam, groups, max_norm, foreach=False, **kw)


@functools.lru_cache(maxsize=None)
def sgd_reference64(case_name, variant, chunk, grad_steps=None):
    """The float64 reference of an SGD case and variant on the edge table: computed once, shared, never modified."""
    case = SGD_CASES[case_name]
    return run(OC.edge_tensors(chunk), case, torch_sgd(case.max_norm), sgd_groups(case_name, variant), SGD_KEYS, grad_steps=grad_steps)[2]


@functools.lru_cache(maxsize=None)
def adam_reference64(case_name, chunk, grad_steps=None):
    case = OC.CASES[case_name]
    return run(OC.edge_tensors(chunk), case, torch_adam(case.max_norm), OC.groups_of, ADAM_KEYS, grad_steps=grad_steps)[2]


def sgd64(p, g, buf, first, lr, weight_decay, momentum, dampening, nesterov):
    """One SGD step in float64 by the formula; `first`: the tensor's first step (buf = g, undampened).  -> (p, buf)"""
    if weight_decay != 0:
        g = g + weight_decay * p
    if momentum != 0:
        buf = g if first else momentum * buf + (1 - dampening) * g
        g = g + momentum * buf if nesterov else buf
    return p - lr * g, buf


def adam64(p, g, m, v, step, lr, weight_decay, betas, eps):
    """One Adam step in float64 by the formula (torch.optim.adam._single_tensor_adam, no amsgrad).  -> (p, m, v)"""
    b1, b2 = betas
    if weight_decay != 0:
        g = g + weight_decay * p
    m = m + (1 - b1) * (g - m)
    v = b2 * v + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    return p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps), m, v


def formula_run(rule, tensors, case, hyper_of, seed=0):
    """`case` on `tensors` by sgd64 / adam64 in float64 with the clipping of clip_grad_norm_ restated: name -> p after case.steps.
    hyper_of(i) -> the keyword arguments of the rule for tensor i."""
    p = {k: v.double() for k, v in OC.values(tensors, seed).items()}
    state = {t.name: dict(step=0, m=None, v=None) for t in tensors}
    for step in range(1, case.steps + 1):
        grads = {k: None if g is None else g.double() for k, g in OC.gradients(tensors, case, step, seed).items()}
        coef = 1.0
        if case.max_norm > 0:
            total = math.sqrt(sum(float(g.pow(2).sum()) for g in grads.values() if g is not None))
            coef = min(1.0, case.max_norm / (total + 1e-6))
        for i, t in enumerate(tensors):
            g = grads[t.name]
            if g is None:
                continue
            g, st = g * coef, state[t.name]
            st["step"] += 1
            if rule == "sgd":
                p[t.name], st["m"] = sgd64(p[t.name], g, st["m"], st["step"] == 1, **hyper_of(i))
            else:
                z = torch.zeros_like(g)
                m, v = (z, z) if st["m"] is None else (st["m"], st["v"])
                p[t.name], st["m"], st["v"] = adam64(p[t.name], g, m, v, st["step"], **hyper_of(i))
    return p


def adam_hyper(i):
    return dict(eps=OC.EPS, **OC.ROWS[i % len(OC.ROWS)])


def sgd_hyper(case_name, variant):
    rows = SGD_CASE_ROWS[case_name]
    return lambda i: dict(**rows[i % len(rows)], **SGD_VARIANTS[variant])


class StandIn(torch.nn.Module):
    """A handful of conv + BN layers named as the UCN towers name theirs (~20 tensors): what build_ucn_param_groups sees."""

    def __init__(self):
        super().__init__()
        nn = torch.nn
        self.conv1 = nn.Conv2d(3, 8, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(8)
        self.layer1 = nn.Sequential(nn.Conv2d(8, 8, 3, bias=False), nn.BatchNorm2d(8), nn.Conv2d(8, 16, 3, bias=True),
                                    nn.BatchNorm2d(16))
        self.layer2 = nn.Sequential(nn.Conv2d(16, 16, 1, bias=False), nn.BatchNorm2d(16), nn.Conv2d(16, 16, 3, bias=False),
                                    nn.BatchNorm2d(16))
        self.fc = nn.Conv2d(16, 4, 1)
