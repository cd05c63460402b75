"""Timing of msm_prepare_inputs (input normalisation + zero padding of a batch in one launch) at the two shapes a deployment meets:
  normalise   16 x 3 x 480 x 640 -> the same size (no padding)
  pad         16 x 3 x 720 x 1280 -> 736 x 1280 (720 is not a multiple of 32)
each image only and with a three-channel depth batch next to it (copied and padded by the same launch).
  kernel   ops.prepare_inputs into preallocated outputs; HIP events around a window of back-to-back launches, median of N windows after
           a warm-up, per launch.  Every launch goes through the Python wrapper, so a figure can only be too large (host enqueue).
           Bytes moved = 4 read per input element + 4 written per output element (the padding is written, not read).
  torch    the same definition in torch ops on the same GPU -- (x - mean) / std and F.pad, plus F.pad of the depth: up to four launches --
           timed ALTERNATELY with the kernel, window by window; its image must equal the kernel's (device division is compared, not
           assumed: the count of differing elements is printed).
  copy     a float tensor of the kernel's input size copied by torch (copy_), timed in the same loop: what the box's memory system
           gives a read-once, write-once pass right now (tools/bw_probe.py measures the same on 1 GiB).
Prints one JSON line."""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from unseenobjectswithmeanshift_amd import ops  # noqa: E402

N, LAUNCHES = 30, 100
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]


def window(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


def timed_alternately(fns):
    for fn in fns:
        for _ in range(LAUNCHES):
            fn()
    torch.cuda.synchronize()
    us = [[] for _ in fns]
    for _ in range(N):
        for i, fn in enumerate(fns):
            us[i].append(window(fn, LAUNCHES))
    return [(float(np.median(u)), float(np.min(u))) for u in us]


def main():
    dev = "cuda"
    gen = torch.Generator().manual_seed(0)
    mean, std = torch.tensor(MEAN, device=dev), torch.tensor(STD, device=dev)
    out = {"probe": "prepare_inputs", "windows": N, "launches_per_window": LAUNCHES, "cases": []}
    for name, (B, H, W), frame in (("normalise", (16, 480, 640), (480, 640)), ("pad", (16, 720, 1280), (736, 1280))):
        x = (torch.rand((B, 3, H, W), generator=gen) * 255).to(dev)
        d = torch.rand((B, 3, H, W), generator=gen).to(dev)
        o_x, o_d = torch.empty((B, 3) + frame, device=dev), torch.empty((B, 3) + frame, device=dev)
        pad = (0, frame[1] - W, 0, frame[0] - H)
        for with_depth in (False, True):
            dd, od = (d, o_d) if with_depth else (None, None)
            src = torch.cat([x, d]) if with_depth else x
            dst = torch.empty_like(src)

            def kernel():
                ops.prepare_inputs(x, dd, mean=mean, std=std, frame=frame, out_image=o_x, out_depth=od)

            def chain():
                a = F.pad((x - mean[:, None, None]) / std[:, None, None], pad)
                return a, (F.pad(d, pad) if with_depth else None)

            k, t, c = timed_alternately([kernel, chain, lambda: dst.copy_(src)])
            planes = 2 if with_depth else 1
            moved = 4 * planes * B * 3 * (H * W + frame[0] * frame[1])
            kernel()
            ref = chain()[0]
            out["cases"].append({"case": name, "depth": with_depth, "in": [B, 3, H, W], "frame": list(frame), "bytes": moved,
                                 "kernel_us_median": round(k[0], 2), "kernel_us_min": round(k[1], 2), "kernel_TBps": round(moved / k[0] / 1e6, 3),
                                 "torch_ops_us_median": round(t[0], 2), "kernel_over_torch_ops": round(k[0] / t[0], 3),
                                 "copy_us_median": round(c[0], 2), "copy_TBps": round(2 * 4 * src.numel() / c[0] / 1e6, 3),
                                 "image_elements_differing_from_torch_ops": int((ref != o_x).sum())})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
