"""Time the optimizer step: optim.FullModelClipAdamW (two launches over a device table) against the reference's construction on the
same per-tensor groups -- torch.nn.utils.clip_grad_norm_ followed by torch.optim.AdamW (tabletop_train_net_pretrained.py:161-186) --
with torch's default path and with fused=True, on the same GPU, the same tensors, in the same run, the three alternating.

    python tools/probes/optimizer_time.py [--heads resnet50 ucn] [--reps 30] [--warmup 3] [--max-norm 0.01] [--lr 1e-4]

The parameter lists are those of build_resnet50_head() (298 tensors, 15.8 M parameters) and build_ucn_head() (125 tensors, 9.9 M)
with seeded random gradients of norm >> max_norm, restored before every step outside the timed region (every step clips, as a
training step does).  Per variant and head two clocks, medians over --reps steps:
    gpu_ms   HIP events recorded around step() on an idle stream: from the first launch's start to the last one's end
    host_ms  wall time from the call until step() returns to the host (the queue is empty at the call; nothing is waited for inside)
Prints one JSON line per head: both clocks of the three variants, the 9-stream floor (the norm pass reads g; the update reads p, g,
exp_avg, exp_avg_sq and writes p, exp_avg, exp_avg_sq and the clipped g: 9 x 4 bytes per parameter), the bandwidth the new step reaches
against that floor (over gpu_ms, which holds the host's enqueue time between the two launches, and over the two launches timed
one by one), the speedups, and how far the parameters of the three are apart after the same steps."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from unseenobjectswithmeanshift_amd import _lib  # noqa: E402
from unseenobjectswithmeanshift_amd.meta_arch import build_resnet50_head, build_ucn_head  # noqa: E402
from unseenobjectswithmeanshift_amd.optim import FullModelClipAdamW, build_param_groups  # noqa: E402

HEADS = {"resnet50": build_resnet50_head, "ucn": build_ucn_head}


class ClippedTorch:
    def __init__(self, groups, lr, max_norm, **kw):
        self.opt = torch.optim.AdamW(groups, lr, **kw)
        self.params = [p for g in groups for p in g["params"]]
        self.max_norm = max_norm

    def step(self):
        if self.max_norm > 0:
            torch.nn.utils.clip_grad_norm_(self.params, self.max_norm)
        self.opt.step()


def variant(head, kind, lr, max_norm, saved):
    """A copy of the head's parameters in the reference's groups, gradients attached, and the optimizer `kind` over them."""
    groups = build_param_groups(head, lr)
    for g in groups:
        g["params"] = [torch.nn.Parameter(g["params"][0].detach().clone())]
    params = [g["params"][0] for g in groups]
    for p, s in zip(params, saved):
        p.grad = s.clone()
    if kind == "hip":
        opt = FullModelClipAdamW(groups, lr=lr, max_norm=max_norm)
    else:
        opt = ClippedTorch(groups, lr, max_norm, **({"fused": True} if kind == "torch_fused" else {}))
    return params, opt


def measure(head_name, a):
    torch.manual_seed(0)
    head = HEADS[head_name]().cuda()
    shapes = [g["params"][0].shape for g in build_param_groups(head, a.lr)]
    gen = torch.Generator(device="cuda").manual_seed(1)
    saved = [1e-3 * torch.randn(s, device="cuda", generator=gen) for s in shapes]
    kinds = ("hip", "torch_default", "torch_fused")
    variants = {k: variant(head, k, a.lr, a.max_norm, saved) for k in kinds}
    gpu = {k: [] for k in kinds}
    host = {k: [] for k in kinds}
    for rep in range(a.warmup + a.reps):
        for k in kinds:                                   # alternating: the three see the same machine state
            params, opt = variants[k]
            torch._foreach_copy_([p.grad for p in params], saved)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            opt.step()
            e1.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            if rep >= a.warmup:
                gpu[k].append(e0.elapsed_time(e1))
                host[k].append((t1 - t0) * 1e3)
    numel = sum(s.numel() for s in saved)
    floor = 9 * 4 * numel
    out = {"head": head_name, "tensors": len(saved), "parameters": numel, "max_norm": a.max_norm, "reps": a.reps,
           "floor_bytes": floor}
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
    with _lib.CallTimer() as timer:                       # the two launches on their own (events around each entry point)
        for _ in range(a.reps):
            torch._foreach_copy_([p.grad for p in hip_params], saved)
            hip.step()
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
    ap.add_argument("--heads", nargs="+", default=["resnet50", "ucn"], choices=sorted(HEADS))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-norm", type=float, default=0.01)
    ap.add_argument("--lr", type=float, default=1e-4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optimizer_time.py needs a GPU: a CPU run says nothing about these times")
    for name in a.heads:
        print(json.dumps(measure(name, a)), flush=True)


if __name__ == "__main__":
    main()
