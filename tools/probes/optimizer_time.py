"""Time the optimizer step of optim.FullModelClipAdamW / optim.Adam / optim.SGD (two launches over a device table) against torch's
optimizer of the same rule on the same groups -- torch.nn.utils.clip_grad_norm_ inside step() as the reference wraps it
(tabletop_train_net_pretrained.py:161-186) -- with torch's default (foreach) path and with fused=True, on the same GPU, the same
tensors, in the same run, the variants alternating.

    python tools/probes/optimizer_time.py [--rule adamw|adam|sgd] [--tables resnet50 ucn towers] [--scaler]
                                          [--reps 30] [--warmup 3] [--max-norm 0.01] [--lr 1e-4]

Tables: the parameter lists of build_resnet50_head() (298 tensors, 15.8 M parameters) and build_ucn_head() (125 tensors, 9.9 M) in
the reference's one-group-per-tensor groups (build_param_groups), and "towers": the two ResNet34-8s towers of UCNBackbone in the two
groups of tools/train_net.py:133-134 (build_ucn_param_groups).  Seeded random gradients of norm >> max_norm are restored before
every step outside the timed region (every step clips when max_norm > 0, as a training step does).

--scaler times ``scaler.step(optimizer)`` of a torch.amp.GradScaler instead of ``optimizer.step()`` (the reference's
AMPTrainer.run_step, :209-246): the gradients are restored multiplied by the scale, and ``scaler.update()`` runs outside the timed
region.  It adds the variant ``hip_unfused``: the same optimizer with ``_step_supports_amp_scaling = False``, i.e. what a GradScaler
did with it before it followed the protocol (foreach unscale, ``found_inf.item()``, then the step without a scale).

Per variant and table two clocks, medians over --reps steps:
    gpu_ms   HIP events recorded around the call on an idle stream: from the first launch's start to the last one's end
    host_ms  wall time from the call until it returns to the host (the queue is empty at the call)
Prints one JSON line per table: both clocks of every variant, the stream floor of the rule (the norm pass reads g when max_norm > 0;
AdamW / Adam read p, g, exp_avg, exp_avg_sq and write p, exp_avg, exp_avg_sq; SGD with momentum reads p, g, buf and writes p, buf;
a clipped or unscaled g is written back: 4 bytes per parameter and stream), the bandwidth the step reaches against that floor (over
gpu_ms, which holds the host's enqueue time between the launches, and over the launches timed one by one), the speedups, and how far
the parameters of the variants are apart after the same steps."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from unseenobjectswithmeanshift_amd import _lib  # noqa: E402
from unseenobjectswithmeanshift_amd import optim  # noqa: E402
from unseenobjectswithmeanshift_amd.meta_arch import build_resnet50_head, build_ucn_head  # noqa: E402
from unseenobjectswithmeanshift_amd.ucn_backbone import UCNBackbone  # noqa: E402

TABLES = {"resnet50": build_resnet50_head, "ucn": build_ucn_head, "towers": UCNBackbone}
TORCH = {"adamw": torch.optim.AdamW, "adam": torch.optim.Adam, "sgd": torch.optim.SGD}
OURS = {"adamw": optim.FullModelClipAdamW, "adam": optim.Adam, "sgd": optim.SGD}
SCALE = 65536.0


def clipped(cls, max_norm):
    """The reference's FullModelGradientClippingOptimizer over `cls`."""
    class Clipped(cls):
        def step(self, closure=None):
            if max_norm > 0:
                params = [p for g in self.param_groups for p in g["params"]]
                scale = getattr(self, "grad_scale", None)
                if scale is not None:
                    # fused=True under a GradScaler: the scaler hands the scale over and the gradients arrive scaled.  Clipping
                    # them as they are would be another update, so they are unscaled here (one foreach launch, as unscale_ does
                    # it) and the fused step gets no scale; found_inf still skips it.
                    torch._foreach_mul_([p.grad for p in params], scale.double().reciprocal().float())
                    self.grad_scale = None
                torch.nn.utils.clip_grad_norm_(params, max_norm)
            return super().step(closure)
    return Clipped


def groups_of(module, table, a):
    if table == "towers":
        groups = optim.build_ucn_param_groups(module)
        for g in groups:
            g["lr"] = a.lr
        return groups
    return optim.build_param_groups(module, a.lr)


def variant(module, table, kind, a, saved):
    """A copy of the table's parameters in its groups, gradients attached, and the optimizer `kind` over them."""
    groups = groups_of(module, table, a)
    for g in groups:
        g["params"] = [torch.nn.Parameter(p.detach().clone()) for p in g["params"]]
    params = [p for g in groups for p in g["params"]]
    for p, s in zip(params, saved):
        p.grad = s.clone()
    rule_kw = {"momentum": a.momentum} if a.rule == "sgd" else {}
    if kind in ("hip", "hip_unfused"):
        cls = OURS[a.rule]
        if kind == "hip_unfused":
            cls = type(cls.__name__ + "Unfused", (cls,), {"_step_supports_amp_scaling": False, "_NAME": cls._NAME, "_RULE": cls._RULE})
        opt = cls(groups, lr=a.lr, max_norm=a.max_norm, **rule_kw)
    else:
        opt = clipped(TORCH[a.rule], a.max_norm)(groups, lr=a.lr, **rule_kw, **({"fused": True} if kind == "torch_fused" else {}))
    return params, opt


def floor_streams(a):
    streams = {"adamw": 7, "adam": 7, "sgd": 5 if a.momentum else 3}[a.rule]
    if a.max_norm > 0:
        streams += 2                                       # the norm pass reads g, the update writes the clipped g
    elif a.scaler:
        streams += 1                                       # the unscaled g is written back
    return streams


def measure(table, a):
    torch.manual_seed(0)
    module = TABLES[table]().cuda()
    shapes = [p.shape for g in groups_of(module, table, a) for p in g["params"]]
    gen = torch.Generator(device="cuda").manual_seed(1)
    saved = [1e-3 * torch.randn(s, device="cuda", generator=gen) for s in shapes]
    given = [s * SCALE for s in saved] if a.scaler else saved
    kinds = ("hip",) + (("hip_unfused",) if a.scaler else ()) + ("torch_default", "torch_fused")
    variants = {k: variant(module, table, k, a, saved) for k in kinds}
    scalers = {k: torch.amp.GradScaler("cuda", init_scale=SCALE, growth_interval=10 ** 9) for k in kinds} if a.scaler else {}
    for scaler in scalers.values():                       # the scale tensor is made by the first scale(): no loss is scaled here
        scaler.scale(torch.zeros((), device="cuda"))
    gpu = {k: [] for k in kinds}
    host = {k: [] for k in kinds}

    def call(k):
        if a.scaler:
            scalers[k].step(variants[k][1])
        else:
            variants[k][1].step()

    def after(k):
        if a.scaler:
            scalers[k].update()

    for rep in range(a.warmup + a.reps):
        for k in kinds:                                   # alternating: the variants see the same machine state
            params, _ = variants[k]
            torch._foreach_copy_([p.grad for p in params], given)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            call(k)
            e1.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            after(k)
            if rep >= a.warmup:
                gpu[k].append(e0.elapsed_time(e1))
                host[k].append((t1 - t0) * 1e3)
    numel = sum(s.numel() for s in saved)
    floor = floor_streams(a) * 4 * numel
    out = {"table": table, "rule": a.rule, "scaler": a.scaler, "tensors": len(saved), "groups": len(variants["hip"][1].param_groups),
           "parameters": numel, "max_norm": a.max_norm, "reps": a.reps, "floor_bytes": floor}
    for k in kinds:
        out[f"{k}_gpu_ms"] = round(statistics.median(gpu[k]), 4)
        out[f"{k}_host_ms"] = round(statistics.median(host[k]), 4)
        out[f"{k}_gpu_ms_min_max"] = [round(min(gpu[k]), 4), round(max(gpu[k]), 4)]
    out["hip_GBps_of_floor"] = round(floor / (out["hip_gpu_ms"] * 1e-3) / 1e9, 1)
    for k in kinds[1:]:
        out[f"speedup_gpu_vs_{k}"] = round(out[f"{k}_gpu_ms"] / out["hip_gpu_ms"], 1)
        out[f"speedup_host_vs_{k}"] = round(out[f"{k}_host_ms"] / out["hip_host_ms"], 1)
        diff = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(variants["hip"][0], variants[k][0]))
        out[f"param_max_diff_vs_{k}"] = diff
    hip_params, hip = variants["hip"]
    with _lib.CallTimer() as timer:                       # the launches on their own (events around each entry point)
        for _ in range(a.reps):
            torch._foreach_copy_([p.grad for p in hip_params], given)
            call("hip")
            after("hip")
    torch.cuda.synchronize()
    out["hip_launch_ms"] = {name: round(statistics.median(ms), 4) for name, ms in timer.durations().items()}
    out["hip_launches_GBps_of_floor"] = round(floor / (sum(out["hip_launch_ms"].values()) * 1e-3) / 1e9, 1)
    out["hip_uploads"] = hip.uploads
    out["last_grad_norm"], out["last_clip_coef"] = float(hip.last_grad_norm), float(hip.last_clip_coef)
    out["faster_on_both_clocks"] = all(out["hip_gpu_ms"] < out[f"{k}_gpu_ms"] and out["hip_host_ms"] < out[f"{k}_host_ms"]
                                       for k in kinds[1:])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rule", default="adamw", choices=sorted(OURS))
    ap.add_argument("--tables", "--heads", nargs="+", default=["resnet50", "ucn"], choices=sorted(TABLES))
    ap.add_argument("--scaler", action="store_true", help="time GradScaler.step(optimizer) on gradients scaled by 65536")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-norm", type=float, default=0.01)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--momentum", type=float, default=0.9, help="--rule sgd")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optimizer_time.py needs a GPU: a CPU run says nothing about these times")
    for name in a.tables:
        print(json.dumps(measure(name, a)), flush=True)


if __name__ == "__main__":
    main()
