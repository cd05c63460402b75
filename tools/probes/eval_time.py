"""Timing of the segmentation metrics (evaluation.py) at 16 frames of 480x640 with about ten labels a side:
  device   the count pass (msm_eval_counts: four launches), HIP events, median of 50
  batched  the whole multilabel_metrics_batched call (counts, one device -> host copy, host step), wall clock, median of 20
  host     the CPU restatement (host_counts + the host step) of the same 16 frames on this host, once
Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from unseenobjectswithmeanshift_amd import evaluation as ev  # noqa: E402
from unseenobjectswithmeanshift_amd import ops  # noqa: E402
from unseenobjectswithmeanshift_amd import synthetic as syn  # noqa: E402


def main():
    B, H, W = 16, 480, 640
    pairs = [syn.synth_label_pair(H, W, 100 + f, "blobs", n_gt=10, n_pred=10) for f in range(B)]
    pred = torch.from_numpy(np.stack([p for p, _ in pairs])).cuda()
    gt = torch.from_numpy(np.stack([g for _, g in pairs])).cuda()
    r = ev.bound_radius(H, W)
    for _ in range(5):
        ops.eval_counts(pred, gt, r)
    torch.cuda.synchronize()
    dev = []
    for _ in range(50):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.eval_counts(pred, gt, r)
        e1.record()
        e1.synchronize()
        dev.append(e0.elapsed_time(e1) * 1e3)
    for _ in range(3):
        ev.multilabel_metrics_batched(pred, gt)
    wall = []
    for _ in range(20):
        torch.cuda.synchronize()
        t = time.perf_counter()
        ev.multilabel_metrics_batched(pred, gt)
        wall.append((time.perf_counter() - t) * 1e6)
    t = time.perf_counter()
    host = [ev.metrics_from_counts(ev.host_counts(p, g)) for p, g in pairs]
    host_us = (time.perf_counter() - t) * 1e6
    got = ev.multilabel_metrics_batched(pred, gt)
    same = all(np.array_equal(np.array([float(a[k]) for k in ev.KEYS]), np.array([float(b[k]) for k in ev.KEYS]), equal_nan=True)
               for a, b in zip(got, host))
    labels = [int(c["labels_gt"].size) for c in ev.device_counts(pred, gt)]
    print(json.dumps({"probe": "eval", "frames": B, "size": [H, W], "radius": r, "gt_labels_mean": float(np.mean(labels)),
                      "device_pass_us_median": round(float(np.median(dev)), 1), "device_pass_us_min": round(float(np.min(dev)), 1),
                      "batched_call_us_median": round(float(np.median(wall)), 1), "host_restatement_us": round(host_us, 1),
                      "batched_equals_host": bool(same)}))


if __name__ == "__main__":
    main()
