"""Time the set criterion (criterion.SetCriterion) against a torch restatement of the reference's loop on the same GPU.

B = 8, Q = 100, 10 predictions of 120 x 160 masks, 8 targets of 480 x 640 per image, P = 12544 (oversample 3, importance 0.75).
HIP events, median of --reps runs after --warmup.  --once: one forward + backward and nothing else (for
`rocprofv3 --kernel-trace --stats -- python tools/probes/criterion_time.py --once`, which counts the launches of one call).
"""
import argparse
import json
import os
import sys

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


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    out, preds, targets = inputs()
    crit = cr.build_criterion(C1 - 1, class_weight=2.0, mask_weight=5.0, dice_weight=5.0, no_object_weight=0.1, dec_layers=NP)

    def ours_fwd():
        return crit(out, targets)

    def ours_step():
        sum(ours_fwd().values()).backward()

    def ref_step():
        sum(torch_reference(out, targets).values()).backward()

    if a.once:
        ours_step()
        torch.cuda.synchronize()
        return
    res = {"shape": dict(B=B, Q=Q, n_pred=NP, masks=[HM, WM], targets_per_image=T, target_size=[HG, WG], P=P)}
    with torch.no_grad():
        res["ours_forward_ms"] = timed(ours_fwd, a.reps, a.warmup)
    res["ours_forward_backward_ms"] = timed(ours_step, a.reps, a.warmup)
    with torch.no_grad():
        res["torch_loop_forward_ms"] = timed(lambda: torch_reference(out, targets), a.reps, a.warmup)
    res["torch_loop_forward_backward_ms"] = timed(ref_step, a.reps, a.warmup)
    from unseenobjectswithmeanshift_amd import _lib
    with _lib.CallTimer() as ct:
        with torch.no_grad():
            ours_fwd()
    torch.cuda.synchronize()
    res["kernel_ms"] = {k: round(sum(v), 4) for k, v in ct.durations().items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
