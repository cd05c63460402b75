"""Timing of the training targets (targets.instance_targets: msm_target_tables / msm_target_write / msm_sample_labels) on one GPU:
B = 8 label images of 480 x 640 with ten instances each, size divisibility 32, num = 1000.

  kernels  each entry point alone into preallocated or fresh outputs, HIP events around windows of back-to-back calls, median of N
           windows after a warm-up, per call (every call goes through the Python wrapper: a figure can only be too large).  The
           writer against its byte floor B H W read + TT Hp Wp + 4 B Hp Wp written, at the 6.3 TB/s a copy achieves;
  api      instance_targets with and without sampling, with and without counts= (wall clock per call including the wait of the
           counts copy where there is one, and the device time between events);
  torch    a torch restatement of the reference's loops on the same device tensors (unique, one comparison per instance,
           nonzero / min / max for the box, a relabelling loop, randperm per label);
  host     the host path (numpy) plus the upload of its float masks and label map, against the upload of the uint8 images.
Without --step every step runs in a child process of its own under its own time limit; the first failure ends the run.
Prints one JSON line per step."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

B, H, W, D, NUM, INSTANCES = 8, 480, 640, 32, 1000, 10
N = 20
STEPS = {"kernels": 120, "api": 120, "torch": 180, "host": 180}        # seconds


def label_images():
    rng = np.random.default_rng(0)
    raw = np.zeros((B, H, W), np.uint8)
    raw[:, 300:, :] = 1                                                  # the table
    for b in range(B):
        for i in range(INSTANCES):
            y, x = int(rng.integers(40, 330)), int(rng.integers(0, 540))
            h, w = int(rng.integers(60, 140)), int(rng.integers(50, 100))
            raw[b, y:y + h, x:x + w] = 2 + i
    return raw


def window(torch, fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


def timed(torch, fn, launches):
    for _ in range(launches):
        fn()
    torch.cuda.synchronize()
    us = [window(torch, fn, launches) for _ in range(N)]
    return round(float(np.median(us)), 2), round(float(np.min(us)), 2)


def step_kernels():
    import torch
    from unseenobjectswithmeanshift_amd import ops, targets as tg
    dev = "cuda"
    raw = torch.from_numpy(label_images()).to(dev)
    bg = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    tables = ops.target_tables(raw, bg)
    counts = tables[:, 1].tolist()
    toff = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int64, device=dev)
    TT = int(sum(counts))
    masks = torch.empty((TT, H, W), dtype=torch.uint8, device=dev)
    keys = tg.draw_keys((B, H, W), dev, torch.Generator(dev).manual_seed(0))
    label = ops.target_write(raw, tables, toff, TT, frame=(H, W), masks=masks)[0]
    out = {"probe": "targets/kernels", "B": B, "size": [H, W], "instances": counts, "windows": N}
    out["target_tables_us"] = timed(torch, lambda: ops.target_tables(raw, bg), 50)
    med, mn = timed(torch, lambda: ops.target_write(raw, tables, toff, TT, frame=(H, W), masks=masks), 50)
    floor = B * H * W + TT * H * W + 4 * B * H * W
    out["target_write_us"] = [med, mn]
    out["target_write_floor"] = {"bytes": floor, "us_at_6.3TBps": round(floor / 6.3e6, 2), "fraction_of_floor": round(floor / 6.3e6 / med, 3),
                                 "TBps": round(floor / med / 1e6, 3)}
    raw4 = raw.repeat(4, 1, 1)                                           # the same writer on a launch four times as long
    tables4 = ops.target_tables(raw4, bg)
    toff4 = torch.tensor(np.concatenate([[0], np.cumsum(counts * 4)]), dtype=torch.int64, device=dev)
    masks4 = torch.empty((4 * TT, H, W), dtype=torch.uint8, device=dev)
    med4, _ = timed(torch, lambda: ops.target_write(raw4, tables4, toff4, 4 * TT, frame=(H, W), masks=masks4), 20)
    out["target_write_B32"] = {"us": med4, "fraction_of_floor": round(4 * floor / 6.3e6 / med4, 3)}
    del masks4
    scratch = label.clone()

    def sample():
        scratch.copy_(label)
        ops.sample_labels_(scratch, keys, NUM)

    both = timed(torch, sample, 20)
    copy = timed(torch, lambda: scratch.copy_(label), 20)
    out["sample_labels_us"] = [round(both[0] - copy[0], 2), round(both[1] - copy[1], 2)]
    out["sample_labels_note"] = "label copy subtracted; clear + count + 7 x (histogram, scan) + apply = 17 launches"
    print(json.dumps(out))


def step_api():
    import torch
    from unseenobjectswithmeanshift_amd import targets as tg
    dev = "cuda"
    raw = torch.from_numpy(label_images()).to(dev)
    keys = tg.draw_keys((B, H, W), dev, torch.Generator(dev).manual_seed(0))
    counts = tg.instance_targets(raw, size_divisibility=D).counts
    out = {"probe": "targets/api", "B": B, "size": [H, W], "windows": N}
    for name, kw in (("plain", {}), ("counts", {"counts": counts}), ("sampled", {"sample_num": NUM, "keys": keys}),
                     ("sampled_counts", {"sample_num": NUM, "keys": keys, "counts": counts})):
        fn = lambda: tg.instance_targets(raw, size_divisibility=D, **kw)    # noqa: E731
        device_us = timed(torch, fn, 20)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(50):
            fn()
        torch.cuda.synchronize()
        out[name] = {"device_us": device_us, "wall_us_per_call": round((time.perf_counter() - t0) * 1e6 / 50, 1)}
    print(json.dumps(out))


def torch_restatement(torch, raw, num):
    """The reference's loops with torch ops on the device, image by image."""
    targets, labels = [], []
    for b in range(raw.shape[0]):
        lab = raw[b].to(torch.int64)
        lab = torch.where(lab == 1, torch.zeros_like(lab), lab)
        ids = torch.unique(lab)
        inst = ids[1:] if int(ids[0]) == 0 else ids
        masks = torch.zeros((inst.shape[0], H, W), dtype=torch.float32, device=raw.device)
        boxes = torch.zeros((inst.shape[0], 4), device=raw.device)
        for i, v in enumerate(inst):
            masks[i] = (lab == v).float()
            nz = torch.nonzero(masks[i])
            boxes[i] = torch.stack([nz[:, 1].min(), nz[:, 0].min(), nz[:, 1].max(), nz[:, 0].max()]).float()
        dense = lab.clone()
        for k, v in enumerate(ids):
            dense[lab == v] = k
        sampled = torch.full_like(dense, -1)
        for k in range(int(dense.max()) + 1):
            idx = torch.nonzero(dense == k)
            if idx.shape[0] > num:
                idx = idx[torch.randperm(idx.shape[0], device=raw.device)[:num]]
            sampled[idx[:, 0], idx[:, 1]] = k
        targets.append({"labels": torch.ones(inst.shape[0], dtype=torch.int64, device=raw.device), "masks": masks.bool()})
        labels.append(sampled.float())
    return targets, torch.stack(labels)[:, None]


def step_torch():
    import torch
    dev = "cuda"
    raw = torch.from_numpy(label_images()).to(dev)
    torch_restatement(torch, raw, NUM)
    torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        t0 = time.perf_counter()
        torch_restatement(torch, raw, NUM)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"probe": "targets/torch", "B": B, "size": [H, W], "wall_ms_median": round(float(np.median(ms)), 2),
                      "wall_ms_min": round(float(np.min(ms)), 2)}))


def step_host():
    import torch
    from unseenobjectswithmeanshift_amd import targets as tg
    dev = "cuda"
    raw = label_images()
    keys = tg.draw_keys((B, H, W), "cpu", torch.Generator().manual_seed(0))
    ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        hb = tg.instance_targets(raw, size_divisibility=D, sample_num=NUM, keys=keys)
        ms.append((time.perf_counter() - t0) * 1e3)
    fmasks = hb.masks.float().pin_memory()                               # what the reference uploads: T float masks per image
    flabel = hb.label.pin_memory()
    raw_pinned = torch.from_numpy(raw).pin_memory()
    d_masks, d_label, d_raw = (torch.empty_like(t, device=dev) for t in (fmasks, flabel, raw_pinned))

    def up_float():
        d_masks.copy_(fmasks, non_blocking=True)
        d_label.copy_(flabel, non_blocking=True)

    out = {"probe": "targets/host", "B": B, "size": [H, W], "host_numpy_ms_median": round(float(np.median(ms)), 1),
           "upload_float_masks_and_label": {"bytes": fmasks.numel() * 4 + flabel.numel() * 4, "us": timed(torch, up_float, 3)},
           "upload_uint8_images": {"bytes": raw_pinned.numel(), "us": timed(torch, lambda: d_raw.copy_(raw_pinned, non_blocking=True), 10)}}
    dev_batch = tg.instance_targets(torch.from_numpy(raw).to(dev), size_divisibility=D, sample_num=NUM, keys=keys.to(dev))
    out["device_equals_host"] = all(bool(torch.equal(getattr(dev_batch, f).cpu(), getattr(hb, f))) for f in ("masks", "boxes", "ids", "areas", "label"))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    args = ap.parse_args()
    if args.step:
        return {"kernels": step_kernels, "api": step_api, "torch": step_torch, "host": step_host}[args.step]()
    for step in ("kernels", "api", "torch", "host"):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step], timeout=STEPS[step]).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({"probe": f"targets/{step}", "error": f"no result within {STEPS[step]} s"}))
            return 1
        if rc != 0:
            print(json.dumps({"probe": f"targets/{step}", "error": f"exit status {rc}"}))
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
