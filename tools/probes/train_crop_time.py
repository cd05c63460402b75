"""Timing of the training crops (crops.crop_boxes / crop_resize: msm_crop_boxes, msm_train_crop) on one GPU: B = 8 frames of
480 x 640 with a table and six objects each, cropped around one object and resized to 224 x 224, uint8 labels, xyz present.

  kernels  each entry point alone into preallocated outputs, HIP events around windows of back-to-back calls, median of N windows
           after a warm-up, per call (every call goes through the Python wrapper: a figure can only be too large), against its
           byte floor at the 6.3 TB/s a copy achieves.  The floor of msm_train_crop counts what it must read inside the boxes --
           per image the DISTINCT source pixels its taps touch (rows x columns of the C4 taps for colour at 3 bytes, of the C3
           indices for the label at 1 byte and xyz at 12) -- plus every byte it writes (colour 3, label 1, xyz 12 per output
           pixel); sectors and cache lines are not rounded up.  msm_crop_boxes moves some 80 bytes per image: its time is a launch.
  batch    targets.training_batch on device frames with and without ``crop=`` (wall clock around a synchronize: the call waits
           for its count copy), and the same with the augmentations on;
  torch    a torch restatement on the same device tensors: boxes fetched to the host, per image a slice, F.interpolate
           (bilinear, half-pixel centres, float) for the colour and index_select for label and xyz;
  host     the numpy host path (crop_boxes, crop_resize, ingest of the crops) plus the upload of its float tensors.
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

B, H, W, S = 8, 480, 640, 224
N = 20
STEPS = {"kernels": 120, "batch": 150, "torch": 120, "host": 240}        # seconds
CAM = {"fx": 570.3, "fy": 570.3, "x_offset": 320.0, "y_offset": 240.0}


def frames():
    rng = np.random.default_rng(0)
    color = rng.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)
    depth = rng.integers(400, 2000, size=(B, H, W)).astype(np.uint16)
    depth[rng.random((B, H, W)) < 0.1] = 0
    raw = np.zeros((B, H, W), np.uint8)
    raw[:, 300:, :] = 1
    for b in range(B):
        for t in range(6):
            h, w = 40 + 25 * ((t + b) % 4), 50 + 30 * ((2 * t + b) % 4)
            y, x = 60 + 55 * (t % 3) + 5 * b, 40 + 190 * (t // 3 * 2 + t % 2) % 480 + 7 * b
            raw[b, y:y + h, x:x + w] = 2 + t
    return color, depth, raw


def crop_params():
    from unseenobjectswithmeanshift_amd import crops as C
    return C.draw_crop_params(B, rng=np.random.default_rng(2))


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


def wall(torch, fn, repeats):
    fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) * 1e6)
    return round(float(np.median(us)), 1), round(float(np.min(us)), 1)


def against_floor(us, nbytes):
    return {"us": list(us), "bytes": int(nbytes), "floor_us_at_6.3TBps": round(nbytes / 6.3e6, 2),
            "fraction_of_floor": round(nbytes / 6.3e6 / us[0], 3), "TBps": round(nbytes / us[0] / 1e6, 3)}


def crop_floor_bytes(boxes):
    """The byte floor of msm_train_crop for these boxes, as the module docstring counts it."""
    from unseenobjectswithmeanshift_amd import crops as C
    total = 0
    for x0, y0, x1, y1 in np.asarray(boxes)[:, :4].tolist():
        nx, ny = x1 - x0 + 1, y1 - y0 + 1
        bil = [len(set(C.bilinear_taps(n, S)[0].tolist()) | set(C.bilinear_taps(n, S)[1].tolist())) for n in (ny, nx)]
        near = [len(set(C.nearest_index(n, S).tolist())) for n in (ny, nx)]
        total += 3 * bil[0] * bil[1] + (1 + 12) * near[0] * near[1] + S * S * (3 + 1 + 12)
    return total


def step_kernels():
    import torch
    from unseenobjectswithmeanshift_amd import crops as C, frames as fr, ops, targets as tg
    dev = torch.device("cuda")
    color, depth, raw = frames()
    dcolor, ddepth, draw = torch.from_numpy(color).to(dev), torch.from_numpy(depth.view(np.int16)).to(dev), torch.from_numpy(raw).to(dev)
    p = crop_params().to(dev)
    _, xyz = fr.ingest(dcolor, ddepth, CAM)
    tables = ops.target_tables(draw, tg._device_background(dev, tg.BACKGROUND_IDS))
    boxes = ops.crop_boxes(tables, p.table, (H, W))
    outs = dict(out_color=torch.empty((B, S, S, 3), dtype=torch.uint8, device=dev), out_raw=torch.empty((B, S, S), dtype=torch.uint8, device=dev),
                out_xyz=torch.empty((B, 3, S, S), device=dev))
    out = {"probe": "train_crop/kernels", "B": B, "size": [H, W], "crop": S, "windows": N, "boxes": boxes[:, :4].cpu().tolist()}
    out["crop_boxes"] = against_floor(timed(torch, lambda: ops.crop_boxes(tables, p.table, (H, W), out=boxes), 50), B * 18 * 4)
    out["train_crop"] = against_floor(timed(torch, lambda: ops.train_crop(dcolor, draw, xyz, boxes, S, **outs), 50), crop_floor_bytes(boxes.cpu().numpy()))
    full = torch.from_numpy(np.tile(np.array([[0, 0, W - 1, H - 1, 0, -1, 0, 0]], np.int32), (B, 1))).to(dev)
    out["train_crop_whole_image"] = against_floor(timed(torch, lambda: ops.train_crop(dcolor, draw, xyz, full, S, **outs), 50),
                                                  crop_floor_bytes(full.cpu().numpy()))
    out["train_crop_no_xyz"] = list(timed(torch, lambda: ops.train_crop(dcolor, draw, None, boxes, S, out_color=outs["out_color"],
                                                                         out_raw=outs["out_raw"]), 50))
    out["target_tables_us"] = list(timed(torch, lambda: ops.target_tables(draw, tg._device_background(dev, tg.BACKGROUND_IDS)), 20))
    out["module_calls_us"] = list(timed(torch, lambda: C.crop_resize(dcolor, draw, xyz, C.crop_boxes(draw, p), S), 20))
    p.check()
    print(json.dumps(out))


def step_batch():
    import torch
    from unseenobjectswithmeanshift_amd import augment as A, targets as tg
    dev = torch.device("cuda")
    color, depth, raw = frames()
    dcolor, ddepth, draw = torch.from_numpy(color).to(dev), torch.from_numpy(depth.view(np.int16)).to(dev), torch.from_numpy(raw).to(dev)
    p = crop_params().to(dev)
    gen = torch.Generator(dev).manual_seed(0)
    full = A.draw_params(B, H, W, rng=np.random.default_rng(3), device=dev, generator=gen, add_noise=True)
    at_crop = A.draw_params(B, S, S, rng=np.random.default_rng(3), device=dev, generator=gen, add_noise=True)
    at_crop = A.AugmentParams(at_crop.table, at_crop.pixel_noise, full.gp_noise, host_table=at_crop.host_table)
    out = {"probe": "train_crop/batch", "B": B, "size": [H, W], "crop": S, "repeats": N}
    out["training_batch_us"] = list(wall(torch, lambda: tg.training_batch(dcolor, ddepth, draw, CAM, size_divisibility=32), N))
    out["training_batch_crop_us"] = list(wall(torch, lambda: tg.training_batch(dcolor, ddepth, draw, CAM, size_divisibility=32, crop=p, crop_size=S), N))
    out["training_batch_augment_us"] = list(wall(torch, lambda: tg.training_batch(dcolor, ddepth, draw, CAM, size_divisibility=32, augment=full), N))
    out["training_batch_augment_crop_us"] = list(wall(torch, lambda: tg.training_batch(dcolor, ddepth, draw, CAM, size_divisibility=32, augment=at_crop,
                                                                                        crop=p, crop_size=S), N))
    p.check()
    print(json.dumps(out))


def step_torch():
    import torch
    import torch.nn.functional as F
    from unseenobjectswithmeanshift_amd import crops as C, frames as fr
    dev = torch.device("cuda")
    color, depth, raw = frames()
    dcolor, ddepth, draw = torch.from_numpy(color).to(dev), torch.from_numpy(depth.view(np.int16)).to(dev), torch.from_numpy(raw).to(dev)
    p = crop_params().to(dev)
    _, xyz = fr.ingest(dcolor, ddepth, CAM)
    d = torch.arange(S, device=dev)

    def restatement():
        boxes = C.crop_boxes(draw, p).cpu().tolist()                     # the host needs the boxes to slice: one wait
        cs, ls, zs = [], [], []
        for b, (x0, y0, x1, y1, *_) in enumerate(boxes):
            iy, ix = y0 + (d * (y1 - y0 + 1)) // S, x0 + (d * (x1 - x0 + 1)) // S
            c = dcolor[b, y0:y1 + 1, x0:x1 + 1].permute(2, 0, 1)[None].float()
            cs.append(F.interpolate(c, size=(S, S), mode="bilinear", align_corners=False).round().to(torch.uint8)[0].permute(1, 2, 0))
            ls.append(draw[b].index_select(0, iy).index_select(1, ix))
            zs.append(xyz[b].index_select(1, iy).index_select(2, ix))
        return torch.stack(cs), torch.stack(ls), torch.stack(zs)

    out = {"probe": "train_crop/torch", "B": B, "size": [H, W], "crop": S, "repeats": N}
    out["torch_us"] = list(wall(torch, restatement, N))
    got = C.crop_resize(dcolor, draw, xyz, C.crop_boxes(draw, p), S)
    ref = restatement()
    out["max_colour_difference_to_kernel"] = int((got[0].int() - ref[0].int()).abs().max())
    out["labels_and_xyz_equal"] = bool(torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2]))
    print(json.dumps(out))


def step_host():
    import torch
    from unseenobjectswithmeanshift_amd import crops as C, frames as fr
    dev = torch.device("cuda")
    color, depth, raw = frames()
    p = crop_params()
    _, xyz = fr.ingest(color, depth, CAM)
    xyz = xyz.numpy()

    def host_path():
        c, r, z = C.crop_resize(color, raw, xyz, C.crop_boxes(raw, p), S)
        image = fr.ingest(c, None, None)[0]
        return image, torch.from_numpy(r), torch.from_numpy(z)

    def timed_host(fn, repeats=5):
        ms = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            res = fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.median(ms)), 2), res

    out = {"probe": "train_crop/host", "B": B, "size": [H, W], "crop": S}
    out["host_path_ms"], res = timed_host(host_path)
    pinned = [t.pin_memory() for t in res]
    out["upload_crops_us"] = list(wall(torch, lambda: [t.to(dev, non_blocking=True) for t in pinned], N))
    raws = [torch.from_numpy(a).pin_memory() for a in (color, depth.view(np.int16), raw)]
    out["upload_raw_frames_us"] = list(wall(torch, lambda: [t.to(dev, non_blocking=True) for t in raws], N))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=sorted(STEPS))
    args = ap.parse_args()
    if args.step:
        globals()["step_" + args.step]()
        return 0
    for step, limit in STEPS.items():
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step]).returncode
        if rc != 0:
            print(json.dumps({"probe": "train_crop/" + step, "failed": rc}))
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
