"""Timing of msm_ingest_frames (raw BGR8 + depth frames -> image and xyz tensors) on a batch of 16 frames of 480x640:
  kernel   ops.ingest_frames into preallocated outputs, uint16 and float32 depth; HIP events around a window of back-to-back launches
           (KERNEL_LAUNCHES of them: several milliseconds of device work per window), median of N windows after a warm-up, per launch.
           Every launch goes through the Python wrapper, so a figure can only be too large (host enqueue), never too small.  Fraction
           of HBM bandwidth = the 29 bytes per pixel the algorithm must move (3 colour + 2 depth read, 24 written; 31 with float32
           depth) over the time, against the 6.3 TB/s a copy achieves and the 8 TB/s of the data sheet;
  torch    the same definition written with torch ops on the same GPU (what a user would write today: a float conversion, the
           mean subtraction, the index grids, the divisions, a stack), windows of TORCH_LAUNCHES calls.  Its depth input is int32,
           4 bytes per pixel where the kernel reads 2 (torch has no uint16 -> float conversion on the device to rely on): 31 bytes
           per pixel of minimum traffic, were the chain one pass.  The kernel (uint16) and the chain are timed ALTERNATELY, window by
           window, in one loop, so that a drift of the machine meets both;
  host     frames.ingest on numpy arrays (the reference's host step, batched), wall clock, median of 3;
  upload   the host -> device copy of one batch out of pinned memory: the raw arrays next to the two float tensors.
Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from unseenobjectswithmeanshift_amd import frames, ops  # noqa: E402

F, H, W = 16, 480, 640
N, KERNEL_LAUNCHES, TORCH_LAUNCHES = 30, 200, 40
CAM = {"fx": 616.3653, "fy": 616.2043, "x_offset": 321.4837, "y_offset": 240.1759}


def window(fn, launches):
    """Microseconds per call of ``launches`` back-to-back calls between two HIP events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


def timed(fn, launches):
    return timed_alternately([(fn, launches)])[0]


def timed_alternately(cases):
    """[(fn, launches), ...] -> [(median, min) us per call, ...]: after a warm-up of every case, N rounds of one window per case."""
    for fn, launches in cases:
        for _ in range(launches):
            fn()
    torch.cuda.synchronize()
    us = [[] for _ in cases]
    for _ in range(N):
        for i, (fn, launches) in enumerate(cases):
            us[i].append(window(fn, launches))
    return [(float(np.median(u)), float(np.min(u))) for u in us]


def torch_restatement(color, depth_u16_as_i32, cam, mean):
    """The definition in torch ops, as a user would write it on the device."""
    image = color.permute(0, 3, 1, 2).float() / 255.0 - mean.view(1, 3, 1, 1)
    z = depth_u16_as_i32.float() / 1000.0
    ys = torch.arange(H, device=z.device, dtype=torch.float32).view(1, H, 1)
    xs = torch.arange(W, device=z.device, dtype=torch.float32).view(1, 1, W)
    fx, fy, px, py = (cam[:, i].view(-1, 1, 1) for i in range(4))
    return image, torch.stack([(xs - px) * z / fx, (ys - py) * z / fy, z], 1)


def main():
    dev = "cuda"
    rng = np.random.default_rng(0)
    color = rng.integers(0, 256, size=(F, H, W, 3), dtype=np.uint8)
    depth = rng.integers(0, 5000, size=(F, H, W)).astype(np.uint16)
    color_d = torch.from_numpy(color).to(dev)
    d16 = torch.from_numpy(depth).view(torch.int16).to(dev)
    d32 = (torch.from_numpy(depth.astype(np.float32)) / 1000).to(dev)
    di32 = torch.from_numpy(depth.astype(np.int32)).to(dev)              # the torch chain's input (torch has few uint16 kernels)
    cam = frames.camera_table(CAM, F).to(dev)
    lut = torch.from_numpy(frames.image_lut()).to(dev)
    mean = torch.tensor(np.array(frames.PIXEL_MEANS) / 255.0).float().to(dev)
    image = torch.empty((F, 3, H, W), device=dev)
    xyz = torch.empty((F, 3, H, W), device=dev)
    pixels = F * H * W
    out = {"probe": "ingest", "frames": F, "size": [H, W], "windows": N, "launches_per_window": {"kernel": KERNEL_LAUNCHES, "torch_ops": TORCH_LAUNCHES}}

    def kernel(d):
        return lambda: ops.ingest_frames(color_d, d, cam, lut, out_image=image, out_depth=xyz)

    (k16, t_chain), k32 = timed_alternately([(kernel(d16), KERNEL_LAUNCHES), (lambda: torch_restatement(color_d, di32, cam, mean), TORCH_LAUNCHES)]), \
        timed(kernel(d32), KERNEL_LAUNCHES)
    for name, (med, mn), bytes_px in (("u16", k16, 29), ("f32", k32, 31)):
        moved = pixels * bytes_px
        out[f"kernel_{name}"] = {"us_median": round(med, 2), "us_min": round(mn, 2), "bytes": moved, "TBps": round(moved / med / 1e6, 3),
                                 "of_6.3TBps_copy": round(moved / med / 1e6 / 6.3, 3), "of_8TBps_peak": round(moved / med / 1e6 / 8.0, 3)}
    ops.ingest_frames(color_d, d16, cam, lut, out_image=image, out_depth=xyz)
    t_image, t_xyz = torch_restatement(color_d, di32, cam, mean)
    med, mn = t_chain
    out["torch_ops"] = {"us_median": round(med, 1), "us_min": round(mn, 1), "depth_input": "int32 (4 bytes per pixel)",
                        "kernel_u16_over_torch_ops": round(k16[0] / med, 3),
                        "image_elements_differing_from_kernel": int((t_image != image).sum()), "xyz_elements_differing_from_kernel": int((t_xyz != xyz).sum())}
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        h_image, h_xyz = frames.ingest(color, depth, CAM)
        host.append((time.perf_counter() - t0) * 1e3)
    out["host_numpy_ms_median"] = round(float(np.median(host)), 1)
    out["kernel_equals_host_bitwise"] = bool(torch.equal(image.cpu().view(torch.int32), h_image.view(torch.int32)) and
                                             torch.equal(xyz.cpu().view(torch.int32), h_xyz.view(torch.int32)))
    raw_host = [torch.from_numpy(color).pin_memory(), torch.from_numpy(depth).view(torch.int16).pin_memory()]
    raw_dev = [torch.empty_like(t, device=dev) for t in raw_host]
    flt_host = [h_image.pin_memory(), h_xyz.pin_memory()]
    flt_dev = [image, xyz]

    def upload(src, dst):
        for s, d in zip(src, dst):
            d.copy_(s, non_blocking=True)

    up_raw, up_float = timed_alternately([(lambda: upload(raw_host, raw_dev), 8), (lambda: upload(flt_host, flt_dev), 2)])
    out["upload_raw_us_median"], out["upload_float_us_median"] = round(up_raw[0], 1), round(up_float[0], 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
