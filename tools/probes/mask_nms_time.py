"""Time mask NMS for a batch of frames: the device route (two_stage.combine_masks_with_NMS_batched -> msm_mask_nms, HIP events)
against the host route it replaces for the same tensors (.cpu() + two_stage.combine_masks_with_NMS per frame, wall clock).

    python tools/probes/mask_nms_time.py [--frames 16] [--size 480 640] [--k 100] [--candidates 12] [--reps 20]

Prints one JSON line: milliseconds per batch for both routes, the bytes the pack pass reads, and whether the results agree."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from unseenobjectswithmeanshift_amd import ops, two_stage as ts  # noqa: E402
from unseenobjectswithmeanshift_amd.meta_arch import Instances  # noqa: E402


def frames(Fr, K, H, W, n_cand, seed=0):
    """K ellipse masks per frame; about n_cand of them are candidates (score > 0.7), a third of those jittered copies of another."""
    g = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    masks = np.zeros((Fr, K, H, W), dtype=np.float32)
    scores = g.uniform(0.05, 0.65, (Fr, K)).astype(np.float32)
    for f in range(Fr):
        picks = g.choice(K, n_cand + g.randint(-2, 3), replace=False)
        scores[f, picks] = g.uniform(0.71, 0.99, len(picks)).astype(np.float32)
        for k in range(K):
            if k % 3 == 2:
                cy, cx = cy + g.uniform(-6, 6), cx + g.uniform(-6, 6)
            else:
                cy, cx, ry, rx = g.uniform(0, H), g.uniform(0, W), g.uniform(20, H / 4), g.uniform(20, W / 4)
            masks[f, k] = (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2) <= 1
    return torch.from_numpy(masks), torch.from_numpy(scores)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, nargs=2, default=(480, 640))
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--candidates", type=int, default=12)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    H, W = a.size
    masks, scores = frames(a.frames, a.k, H, W, a.candidates)
    masks, scores = masks.cuda(), scores.cuda()
    cand = scores > 0.7
    ws = torch.empty(ops.mask_nms_workspace_bytes(a.frames, a.k, H, W), dtype=torch.uint8, device="cuda")
    for _ in range(3):
        out = ts.combine_masks_with_NMS_batched(masks, scores, cand, 0.7, ws)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(a.reps):
        out = ts.combine_masks_with_NMS_batched(masks, scores, cand, 0.7, ws)
    e1.record()
    torch.cuda.synchronize()
    dev_ms = e0.elapsed_time(e1) / a.reps

    def host_route():
        res = []
        for f in range(a.frames):
            keep = cand[f]
            res.append(ts.combine_masks_with_NMS(Instances((H, W), pred_masks=masks[f][keep], scores=scores[f][keep])))
        return res

    host_route()
    host_reps = max(1, a.reps // 10)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(host_reps):
        ref = host_route()
    host_ms = (time.perf_counter() - t0) * 1e3 / host_reps
    same = all(np.array_equal(out[0][f].cpu().numpy().astype(np.float64), ref[f][0]) and
               np.array_equal(out[1][f].cpu().numpy().astype(np.float64), ref[f][1]) and
               np.array_equal(out[2][f, :int(out[3][f])].cpu().numpy(), ref[f][2]) for f in range(a.frames))
    n_cand = int(cand.sum())
    print(json.dumps({"frames": a.frames, "size": [H, W], "K": a.k, "candidates": n_cand, "kept": int(out[3].sum()),
                      "device_ms": round(dev_ms, 4), "host_ms": round(host_ms, 2), "pack_read_bytes": n_cand * H * W * 4,
                      "all_masks_bytes": masks.numel() * 4, "workspace_bytes": ws.numel(), "results_agree": bool(same)}))


if __name__ == "__main__":
    main()
