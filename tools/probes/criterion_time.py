"""Time the set criterion (criterion.SetCriterion) against a torch restatement of the reference's loop on the same GPU.

B = 8, Q = 100, 10 predictions of 120 x 160 masks, 8 targets of 480 x 640 per image, P = 12544 (oversample 3, importance 0.75).
HIP events, median of --reps runs after --warmup.  --once: one forward + backward and nothing else (for
`rocprofv3 --kernel-trace --stats -- python tools/probes/criterion_time.py --once`, which counts the launches of one call).

--solver host|device|both (default both): the matcher's solver; every solver asked for is timed in the same process, forward
and forward + backward, with the launch entry points' own times (kernel_ms, msm_lsap_match among them for "device").  Next to
each event time stands `host_ms`: the wall time until the call RETURNS, i.e. how long the host is held before it can queue
the next thing (the host solver waits for the GPU inside the call, the device solver does not).
--targets T: targets per image (default 8); --targets 100 is the dense worst case of the assignment (100 x 100 per problem).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from unseenobjectswithmeanshift_amd import criterion as cr  # noqa: E402

DEV = "cuda"
B, Q, C1, NP, HM, WM, T, HG, WG, P = 8, 100, 3, 10, 120, 160, 8, 480, 640, 12544


def inputs():
    g = torch.Generator().manual_seed(0)
    preds = [{"pred_logits": torch.randn(B, Q, C1, generator=g).to(DEV).requires_grad_(True),
              "pred_masks": (torch.randn(B, Q, HM, WM, generator=g) * 3).to(DEV).requires_grad_(True)} for _ in range(NP)]
    out = dict(preds[0])
    out["aux_outputs"] = preds[1:]
    targets = []
    for _ in range(B):
        blocks = torch.rand((T, HG // 32, WG // 32), generator=g) > 0.7
        m = F.interpolate(blocks[:, None].float(), size=(HG, WG), mode="nearest")[:, 0] > 0
        targets.append({"labels": torch.randint(0, C1 - 1, (T,), generator=g).to(DEV), "masks": m.to(DEV)})
    return out, preds, targets


def point_sample(x, c):
    return F.grid_sample(x, 2.0 * c.unsqueeze(2) - 1.0, align_corners=False).squeeze(3)


def torch_reference(outputs, targets, weights=(2.0, 5.0, 5.0), eos=0.1, oversample=3.0, importance=0.75):
    """The reference's per-prediction, per-image loop (matcher.py:98-149, criterion.py:114-190, 200-247) in torch ops."""
    from scipy.optimize import linear_sum_assignment
    wc, wm, wd = weights
    preds = [outputs] + outputs["aux_outputs"]
    ew = torch.ones(C1, device=DEV)
    ew[-1] = eos
    num_masks = max(float(sum(len(t["labels"]) for t in targets)), 1.0)
    losses = {}
    for pi, o in enumerate(preds):
        idx = []
        with torch.no_grad():
            for b in range(B):
                prob = o["pred_logits"][b].softmax(-1)
                cc = -prob[:, targets[b]["labels"]]
                pts = torch.rand(1, P, 2, device=DEV)
                tm = point_sample(targets[b]["masks"].float()[:, None], pts.repeat(T, 1, 1)).squeeze(1)
                om = point_sample(o["pred_masks"][b][:, None], pts.repeat(Q, 1, 1)).squeeze(1)
                pos = F.binary_cross_entropy_with_logits(om, torch.ones_like(om), reduction="none")
                neg = F.binary_cross_entropy_with_logits(om, torch.zeros_like(om), reduction="none")
                cm = (pos @ tm.T + neg @ (1 - tm).T) / P
                s = om.sigmoid()
                cd = 1 - (2 * s @ tm.T + 1) / (s.sum(-1)[:, None] + tm.sum(-1)[None, :] + 1)
                C = (wm * cm + wc * cc + wd * cd).cpu()
                i, j = linear_sum_assignment(C)
                idx.append((torch.as_tensor(i, dtype=torch.int64), torch.as_tensor(j, dtype=torch.int64)))
        bi = torch.cat([torch.full_like(s, b) for b, (s, _) in enumerate(idx)])
        si = torch.cat([s for s, _ in idx])
        tcls = torch.full((B, Q), C1 - 1, dtype=torch.int64, device=DEV)
        tcls[bi, si] = torch.cat([t["labels"][j.to(DEV)] for t, (_, j) in zip(targets, idx)])
        sfx = "" if pi == 0 else f"_{pi - 1}"
        losses["loss_ce" + sfx] = F.cross_entropy(o["pred_logits"].transpose(1, 2), tcls, ew)
        src = o["pred_masks"][bi, si][:, None]
        tj = torch.cat([j for _, j in idx])
        tgt = torch.stack([t["masks"] for t in targets]).float()[bi, tj][:, None]
        with torch.no_grad():
            n = src.shape[0]
            ns, k = int(P * oversample), int(importance * P)
            pc = torch.rand(n, ns, 2, device=DEV)
            u = -point_sample(src, pc).abs()
            top = torch.topk(u[:, 0], k=k, dim=1)[1] + ns * torch.arange(n, device=DEV)[:, None]
            pc = torch.cat([pc.view(-1, 2)[top.view(-1)].view(n, k, 2), torch.rand(n, P - k, 2, device=DEV)], 1)
            lab = point_sample(tgt, pc).squeeze(1)
        x = point_sample(src, pc).squeeze(1)
        losses["loss_mask" + sfx] = F.binary_cross_entropy_with_logits(x, lab, reduction="none").mean(1).sum() / num_masks
        s = x.sigmoid()
        losses["loss_dice" + sfx] = (1 - (2 * (s * lab).sum(-1) + 1) / (s.sum(-1) + lab.sum(-1) + 1)).sum() / num_masks
    return losses


def timed(fn, reps, warmup, host=False):
    """Median HIP-event time of fn(); host=True: (event time, wall time until fn returned)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts, hs = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        fn()
        hs.append((time.perf_counter() - t0) * 1e3)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return (float(np.median(ts)), float(np.median(hs))) if host else float(np.median(ts))


def main():
    global T
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--solver", choices=("host", "device", "both"), default="both")
    ap.add_argument("--targets", type=int, default=T, help="targets per image")
    ap.add_argument("--no-torch-loop", action="store_true", help="skip the torch restatement of the reference's loop")
    a = ap.parse_args()
    T = a.targets
    out, preds, targets = inputs()
    solvers = ("host", "device") if a.solver == "both" else (a.solver,)
    crits = {s: cr.build_criterion(C1 - 1, class_weight=2.0, mask_weight=5.0, dice_weight=5.0, no_object_weight=0.1, dec_layers=NP,
                                   solver=s).to(DEV) for s in solvers}

    def ref_step():
        sum(torch_reference(out, targets).values()).backward()

    if a.once:
        sum(crits[solvers[0]](out, targets).values()).backward()
        torch.cuda.synchronize()
        return
    from unseenobjectswithmeanshift_amd import _lib
    res = {"shape": dict(B=B, Q=Q, n_pred=NP, masks=[HM, WM], targets_per_image=T, target_size=[HG, WG], P=P)}
    for s in solvers:
        crit = crits[s]

        def fwd():
            return crit(out, targets)

        def step():
            sum(fwd().values()).backward()

        r = {}
        with torch.no_grad():
            r["forward_ms"], r["forward_host_ms"] = timed(fwd, a.reps, a.warmup, host=True)
        r["forward_backward_ms"], r["forward_backward_host_ms"] = timed(step, a.reps, a.warmup, host=True)
        with _lib.CallTimer() as ct:
            with torch.no_grad():
                fwd()
        torch.cuda.synchronize()
        r["kernel_ms"] = {k: round(sum(v), 4) for k, v in ct.durations().items()}
        crit.check_matching()
        res[s] = r
    if not a.no_torch_loop:
        with torch.no_grad():
            res["torch_loop_forward_ms"] = timed(lambda: torch_reference(out, targets), a.reps, a.warmup)
        res["torch_loop_forward_backward_ms"] = timed(ref_step, a.reps, a.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
