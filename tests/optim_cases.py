"""Cases for the optimizer tests (tests/test_gpu_optim.py on the GPU, tests/test_optim_cases_cpu.py for what the cases themselves
must hold): tables of tensors with seeded values, per-step gradients, and the float64 reference --
``torch.nn.utils.clip_grad_norm_`` followed by ``torch.optim.AdamW(foreach=False)`` over the same groups on the CPU, the same number
of steps (the reference's construction, MSMFormer/tabletop_train_net_pretrained.py:161-186).

Contract (per tensor, no element left out): max|got - ref64| <= RTOL max|ref64| for exp_avg, exp_avg_sq, the clipped
.grad and the update p_after - p_before; |got - ref64| <= RTOL |ref64| for total_norm and coef.  The update is held, not p: at a
small lr the contract on p would pass an update that is wrong by several per cent.  Learning rates are between 1e-2 and 1e-1 and
parameters of magnitude 0.25, so that the update (>= 0.09 lr in every case here) stands well clear of the fp32 rounding of p
(<= 2^-24 |p|, about 7e-8): 7e-8 / (0.09 * 0.03) = 2.6e-5 of the bound's 1e-4 at worst.
"""
import collections
import functools
import math

import torch

RTOL = 1e-4
EPS = 1e-8
# three hyper-parameter rows that differ in lr, weight decay and betas; tensor i of a table takes row i % 3
ROWS = (dict(lr=0.05, weight_decay=0.05, betas=(0.9, 0.999)),
        dict(lr=0.03, weight_decay=0.0, betas=(0.8, 0.99)),
        dict(lr=0.1, weight_decay=0.3, betas=(0.5, 0.9)))

Tensor = collections.namedtuple("Tensor", "name numel offset_p offset_g")          # offsets: elements into a fresh storage
Case = collections.namedtuple("Case", "name max_norm steps grads skip")            # grads: "randn" scale | "unit" norm | "zero" | "tiny"


def edge_tensors(chunk):
    """Every path of the kernels: below / at / above the 4-element vector width and the chunk size, more than two chunks with a
    scalar tail, a parameter and gradient that both start one element into their storage (the scalar path), a parameter alone
    that does (vector norm and zero, scalar update), and one whose gradient is None on step 2 only."""
    sizes = [1, 3, 4, 5, chunk - 1, chunk, chunk + 1, 2 * chunk + 3]
    tensors = [Tensor(f"n{n}", n, 0, 0) for n in sizes]
    tensors += [Tensor("view_pg", 37, 1, 1), Tensor("view_p", chunk + 6, 1, 0), Tensor("skip", 6, 0, 0)]
    return tensors


CASES = {c.name: c for c in (
    Case("clip_active", 0.01, 3, ("randn", 1.0), {2: ("skip",)}),      # norm ~ 2e2 >> max_norm: clipping is active
    Case("clip_idle", 1.0, 1, ("randn", 1e-3), {}),                    # norm ~ 0.2 < max_norm: coef exactly 1, .grad keeps its values
    Case("clip_eps", 1e-5, 1, ("unit", 2e-5), {}),                     # coef = 1e-5 / (2e-5 + 1e-6) = 0.476, 0.5 without the 1e-6: 5 %
    Case("zero_grads", 0.01, 1, ("zero", 0.0), {}),                    # coef 1, pure weight decay
    Case("no_clip", 0.0, 1, ("randn", 1.0), {}),                       # max_norm = 0: no clipping, grads untouched
    Case("eps_decides", 0.0, 1, ("tiny", 0.0), {}),                    # |g| in 1e-9 .. 1e-7: the denominator is mostly eps
)}


def _storage(gen, numel, offset, scale):
    return (scale * torch.randn(numel + offset, generator=gen))[offset:]


def values(tensors, seed=0):
    """float32 start values, name -> tensor (a view `offset_p` elements into its storage)."""
    gen = torch.Generator().manual_seed(seed)
    return {t.name: _storage(gen, t.numel, t.offset_p, 0.25) for t in tensors}


def gradients(tensors, case, step, seed=0):
    """float32 gradients of `step` (1-based), name -> tensor or None (left out this step)."""
    gen = torch.Generator().manual_seed(1000 * (seed + 1) + step)
    kind, scale = case.grads
    out = {}
    for t in tensors:
        g = torch.randn(t.numel, generator=gen)
        if kind == "randn":
            g = g * scale
        elif kind == "zero":
            g = g * 0.0
        elif kind == "tiny":                                  # log-uniform magnitude in [1e-9, 1e-7], random sign
            g = torch.sign(g) * 10.0 ** (-9.0 + 2.0 * torch.rand(g.shape, generator=gen))
        out[t.name] = g
    if kind == "unit":                                        # the whole model's norm is `scale`
        total = math.sqrt(sum(float(g.double().pow(2).sum()) for g in out.values()))
        out = {k: (g.double() * (scale / total)).float() for k, g in out.items()}
    for t in tensors:                                         # a view `offset_g` elements into its storage
        buf = torch.zeros(t.numel + t.offset_g)
        buf[t.offset_g:] = out[t.name]
        out[t.name] = buf[t.offset_g:]
    for name in case.skip.get(step, ()):
        out[name] = None
    return out


def groups_of(tensors, params):
    """One group per tensor, as the reference builds them; row i % 3."""
    return [dict(params=[params[t.name]], eps=EPS, **ROWS[i % len(ROWS)]) for i, t in enumerate(tensors)]


class ClippedTorchAdamW:
    """The reference's construction: clip_grad_norm_ over every parameter, then torch.optim.AdamW."""

    def __init__(self, groups, max_norm, **kw):
        self.opt = torch.optim.AdamW(groups, **kw)
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


def set_grads(params, grads, device):
    """Give every parameter its gradient of this step: in place where a gradient tensor exists (its address stays), a new tensor
    (keeping the view offset of the case) where there is none, None where the step leaves the parameter out."""
    for name, p in params.items():
        g = grads[name]
        if g is None:
            p.grad = None
        elif p.grad is None:
            full = g._base if g._base is not None else g              # keep the storage offset on the device
            moved = full.to(device=device, dtype=p.dtype)
            p.grad = moved[g.storage_offset():] if g._base is not None else moved
        else:
            p.grad.copy_(g)


def make_params(tensors, device, dtype, seed=0):
    params = {}
    for name, v in values(tensors, seed).items():
        full = (v._base if v._base is not None else v).to(device=device, dtype=dtype)
        params[name] = torch.nn.Parameter(full[v.storage_offset():] if v._base is not None else full)
    return params


def snapshot(params, opt, before):
    """What the contract holds after a step, as float64 on the parameters' device."""
    out = {}
    for name, p in params.items():
        st = opt.state.get(p, {})
        out[name] = dict(update=p.detach().double() - before[name],
                         exp_avg=st["exp_avg"].double().clone() if "exp_avg" in st else None,
                         exp_avg_sq=st["exp_avg_sq"].double().clone() if "exp_avg_sq" in st else None,
                         grad=None if p.grad is None else p.grad.double().clone())
    norm, coef = opt.last_grad_norm, opt.last_clip_coef
    out["total_norm"] = None if norm is None else norm.double().clone()
    out["coef"] = coef.double().clone()
    return out


def run(tensors, case, make_opt, device="cpu", dtype=torch.float64, seed=0, steps=None, params=None, opt=None, first_step=1):
    """Run `case` on `tensors`: make_opt(groups) -> an object with step(), state, last_grad_norm, last_clip_coef.  Returns
    (params, opt, [snapshot per step])."""
    if params is None:
        params = make_params(tensors, device, dtype, seed)
        opt = make_opt(groups_of(tensors, params))
    shots = []
    for step in range(first_step, (steps or case.steps) + 1):
        set_grads(params, gradients(tensors, case, step, seed), device)
        before = {name: p.detach().double().clone() for name, p in params.items()}
        opt.step()
        shots.append(snapshot(params, opt, before))
    return params, opt, shots


@functools.lru_cache(maxsize=None)
def reference64(case_name, chunk, steps=None):
    """The float64 reference of a case on the edge table: computed once, shared, never modified."""
    case = CASES[case_name]
    return run(edge_tensors(chunk), case, lambda groups: ClippedTorchAdamW(groups, case.max_norm, foreach=False), steps=steps)[2]


def compare(got, ref, what, quantities=("update", "exp_avg", "exp_avg_sq", "grad"), verbose=True):
    """Hold one step's snapshot `got` to the contract against `ref`; returns the worst ratio error / max|ref| per quantity."""
    worst = {}
    for name, r in ref.items():
        if name in ("total_norm", "coef"):
            continue
        for q in quantities:
            if r[q] is None:
                assert got[name][q] is None, (what, name, q)
                continue
            assert got[name][q] is not None, (what, name, q)
            g, rr = got[name][q].cpu(), r[q].cpu()
            err, scale = float((g - rr).abs().max()), float(rr.abs().max())
            assert math.isfinite(err), (what, name, q)
            ratio = err / scale if scale else (0.0 if err == 0.0 else math.inf)
            worst[q] = max(worst.get(q, 0.0), ratio)
            assert err <= RTOL * scale, (what, name, q, err, scale)
    for q in ("total_norm", "coef"):
        if ref[q] is None:
            continue
        g, rr = float(got[q]), float(ref[q])
        worst[q] = abs(g - rr) / abs(rr) if rr else abs(g - rr)
        assert abs(g - rr) <= RTOL * abs(rr), (what, q, g, rr)
    if verbose:
        print(f"optim {what}: " + ", ".join(f"{q} {v:.2e}" for q, v in worst.items()))
    return worst


def adamw64(p, g, m, v, step, lr, weight_decay, betas, eps, eps_inside=False):
    """One AdamW step in float64 by the formula (torch.optim.adamw._single_tensor_adamw); eps_inside=True is the variant that puts
    eps inside the bias-correction scaling, (sqrt(v) + eps) / sqrt(bc2) -- the one an 'eps decides' case must tell apart."""
    b1, b2 = betas
    p = p * (1 - lr * weight_decay)
    m = m + (1 - b1) * (g - m)
    v = b2 * v + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    denom = (v.sqrt() + eps) / math.sqrt(bc2) if eps_inside else v.sqrt() / math.sqrt(bc2) + eps
    return p - (lr / bc1) * m / denom, m, v


def eps_placement_gap(chunk):
    """For the eps_decides case (one step, no clipping): per tensor, (max|update_inside - update|, max|update - torch's|, max|update|)
    in float64, where `update` is adamw64's and `inside` its eps_inside variant."""
    tensors, case = edge_tensors(chunk), CASES["eps_decides"]
    ref = reference64("eps_decides", chunk)[0]
    start, grads = values(tensors), gradients(tensors, case, 1)
    out = {}
    for i, t in enumerate(tensors):
        p, g = start[t.name].double(), grads[t.name].double()
        z = torch.zeros_like(p)
        row = ROWS[i % len(ROWS)]
        u = adamw64(p, g, z, z, 1, eps=EPS, **row)[0] - p
        ui = adamw64(p, g, z, z, 1, eps=EPS, eps_inside=True, **row)[0] - p
        out[t.name] = (float((ui - u).abs().max()), float((u - ref[t.name]["update"]).abs().max()), float(u.abs().max()))
    return out
