"""Timing of the training augmentations (augment.augment_color / augment_depth / add_xyz_noise_: msm_augment_color, msm_augment_depth,
msm_xyz_noise) on one GPU: B = 8 frames of 480 x 640, every image taking D1 + D2 (HLS shift and Gaussian pixel noise), ten ellipses
each, uint16 depth, the point-cloud noise from a 120 x 160 field.

  kernels  each entry point alone into preallocated outputs, HIP events around windows of back-to-back calls, median of N windows
           after a warm-up, per call (every call goes through the Python wrapper: a figure can only be too large), against its
           byte floor at the 6.3 TB/s a copy achieves: colour 3 + 3 + 4 bytes per pixel, depth (2 + 4) read twice, xyz 12 + 12;
           the colour kernel also with D1 alone, D2 alone, a 15-tap blur along x and along y, and a plain copy row;
  torch    a torch restatement of the same definitions on the same device tensors;
  host     the numpy host path plus the upload of its float tensors (image, xyz), against the upload of the raw frames.
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

B, H, W, ELLIPSES = 8, 480, 640, 10
N = 20
STEPS = {"kernels": 150, "torch": 180, "host": 240}        # seconds
CAM = {"fx": 570.3, "fy": 570.3, "x_offset": 320.0, "y_offset": 240.0}


def frames():
    rng = np.random.default_rng(0)
    color = rng.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)
    depth = rng.integers(400, 2000, size=(B, H, W)).astype(np.uint16)
    depth[rng.random((B, H, W)) < 0.1] = 0
    return color, depth


def table(**kw):
    from unseenobjectswithmeanshift_amd import augment as A
    rng = np.random.default_rng(1)
    es = [[(np.round(rng.gamma(5.0, 1.0)), np.round(rng.gamma(5.0, 1.0)), int(rng.integers(0, 360)), int(rng.integers(0, 2 ** 32)))
           for _ in range(ELLIPSES)] for _ in range(B)]
    args = dict(chromatic=True, d_h=7.25, d_l=-20.5, d_s=13.75, gaussian=True, sigma=11.37, depth=True,
                multiplier=rng.gamma(1000.0, 0.001, size=B), ellipses=es)
    args.update(kw)
    return A.pack_table(B, **args)


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


def against_floor(us, nbytes):
    return {"us": list(us), "bytes": nbytes, "floor_us_at_6.3TBps": round(nbytes / 6.3e6, 2), "fraction_of_floor": round(nbytes / 6.3e6 / us[0], 3),
            "TBps": round(nbytes / us[0] / 1e6, 3)}


def step_kernels():
    import torch
    from unseenobjectswithmeanshift_amd import augment as A, frames as fr, ops
    dev = torch.device("cuda")
    color, depth = frames()
    dcolor, ddepth = torch.from_numpy(color).to(dev), torch.from_numpy(depth.view(np.int16)).to(dev)
    gen = torch.Generator(dev).manual_seed(0)
    noise = torch.randn((B, H, W), device=dev, generator=gen)
    gp = torch.randn((B, 3, H // 4, W // 4), device=dev, generator=gen)
    p = A.AugmentParams(table(), noise.cpu().numpy(), gp.cpu().numpy()).to(dev)
    status = p._status(dev)
    out_c = torch.empty_like(dcolor)
    out_z = torch.empty((B, H, W), device=dev)
    records = torch.empty((ops.lib().msm_augment_depth_workspace(B, H, W) // 4,), dtype=torch.int32, device=dev)
    _, xyz = fr.ingest(dcolor, ddepth, CAM)
    taps = A._device_taps(dev, H // 4, W // 4, H, W)
    px = B * H * W
    out = {"probe": "augment/kernels", "B": B, "size": [H, W], "ellipses": ELLIPSES, "windows": N}
    out["color_d1_d2"] = against_floor(timed(torch, lambda: ops.augment_color(dcolor, p.table, p.pixel_noise, status, out=out_c), 50), 10 * px)
    for name, kw, nbytes in (("color_d1", dict(gaussian=False), 6), ("color_d2", dict(chromatic=False), 10),
                             ("color_copy", dict(chromatic=False, gaussian=False), 6),
                             ("color_blur15_x", dict(chromatic=False, gaussian=False, blur_size=15, blur_horizontal=True), 6),
                             ("color_blur15_y", dict(chromatic=False, gaussian=False, blur_size=15, blur_horizontal=False), 6),
                             ("color_d1_blur15_x", dict(gaussian=False, blur_size=15, blur_horizontal=True), 6)):
        q = A.AugmentParams(table(**kw)).to(dev)
        out[name] = against_floor(timed(torch, lambda: ops.augment_color(dcolor, q.table, p.pixel_noise, status, out=out_c), 50), nbytes * px)
    run = lambda stages: ops.augment_depth(ddepth, p.table, status, records=records, stages=stages, out=out_z)       # noqa: E731
    out["depth"] = against_floor(timed(torch, lambda: run(3), 50), 2 * (2 + 4) * px)
    out["depth_rows_and_centres_us"] = list(timed(torch, lambda: run(1), 50))
    out["depth_apply_us"] = list(timed(torch, lambda: run(2), 50))
    out["xyz_noise"] = against_floor(timed(torch, lambda: ops.xyz_noise_(xyz, p.gp_noise, taps, 0.005, (H, W)), 50), 24 * px)
    stages = [out["color_d1_d2"]["us"][0], out["depth"]["us"][0], out["xyz_noise"]["us"][0]]
    out["three_stages_us"] = round(sum(stages), 2)
    pipeline = lambda: (A.augment_color(dcolor, p), A.augment_depth(ddepth, p), A.add_xyz_noise_(xyz, p))                # noqa: E731
    out["module_calls_us"] = list(timed(torch, pipeline, 20))
    copy = torch.empty_like(xyz)
    out["copy_xyz_TBps"] = round(2 * xyz.numel() * 4 / timed(torch, lambda: copy.copy_(xyz), 50)[0] / 1e6, 3)
    p.check()
    print(json.dumps(out))


def torch_restatement(torch, F, color, depth, noise, gp, f):
    """D1 + D2, D4 and D5 with torch ops on the device, batch-wide where torch allows."""
    x = color.float() / 255
    b, g, r = x[..., 0], x[..., 1], x[..., 2]
    vmax, vmin = x.amax(-1), x.amin(-1)
    sm, diff = vmax + vmin, vmax - vmin
    lum = sm * 0.5
    s = torch.where(lum < 0.5, diff / sm, diff / ((2 - vmax) - vmin))
    k = 60 / diff
    h = torch.where(vmax == r, (g - b) * k, torch.where(vmax == g, (b - r) * k + 120, (r - g) * k + 240))
    h = torch.where(h < 0, h + 360, h) * 0.5
    flat = diff <= 1.1920929e-07
    h, s = torch.where(flat, 0.0, h), torch.where(flat, 0.0, s)
    dh, dl, ds, sigma = (torch.as_tensor(f[n], device=color.device)[:, None, None] for n in ("d_h", "d_l", "d_s", "sigma"))
    hn = torch.trunc(torch.remainder(torch.round(h) + dh, 180.0))
    ln = torch.trunc(torch.clamp(torch.round(lum * 255) + dl, 0, 255)) / 255
    sn = torch.trunc(torch.clamp(torch.round(s * 255) + ds, 0, 255)) / 255
    p2 = torch.where(ln <= 0.5, ln * (1 + sn), (ln + sn) - ln * sn)
    p1 = 2 * ln - p2
    hh = (hn * 6) / 180
    hh = torch.where(hh >= 6, hh - 6, hh)
    sec = torch.clamp(torch.floor(hh), 0, 5)
    fr = hh - sec
    tab = torch.stack([p2, p1, p1 + (p2 - p1) * (1 - fr), p1 + (p2 - p1) * fr], -1)
    pick = torch.tensor([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]], device=color.device)[sec.long()]
    val = torch.where((sn == 0)[..., None], ln[..., None], torch.gather(tab, -1, pick))
    out = torch.clamp(torch.round(val * 255), 0, 255)
    out = torch.trunc(torch.clamp(out + (sigma * noise)[..., None], 0, 255)).to(torch.uint8)
    # D4
    z = depth.view(torch.int16).to(torch.int32).bitwise_and(0xffff).float() / 1000.0
    z = z * torch.as_tensor(f["multiplier"], device=z.device)[:, None, None]
    ys, xs = torch.meshgrid(torch.arange(H, device=z.device), torch.arange(W, device=z.device), indexing="ij")
    for i in range(z.shape[0]):
        valid = torch.nonzero(z[i].reshape(-1) > 0)[:, 0]
        n = valid.shape[0]
        drop = torch.zeros((H, W), dtype=torch.bool, device=z.device)
        for e in range(int(f["count"][i])):
            idx = valid[(int(f["key"][i, e]) * n) >> 32]
            cy, cx = idx // W, idx % W
            dx, dy = (xs - cx).float(), (ys - cy).float()
            c, s_ = float(f["cos"][i, e]), float(f["sin"][i, e])
            u, v = dx * c + dy * s_, dy * c - dx * s_
            a, bb = max(float(f["rx"][i, e]), 0.5), max(float(f["ry"][i, e]), 0.5)
            drop |= (u * u) / (a * a) + (v * v) / (bb * bb) <= 1
        z[i][drop] = 0
    # D5 on the point cloud of z
    xyz = torch.stack([(xs - CAM["x_offset"]) * z / CAM["fx"], (ys - CAM["y_offset"]) * z / CAM["fy"], z], 1)
    up = F.interpolate(gp, size=(H, W), mode="bicubic", align_corners=False)
    return out, z, torch.where(z[:, None] > 0, xyz + 0.005 * up, xyz)


def step_torch():
    import torch
    import torch.nn.functional as F
    from unseenobjectswithmeanshift_amd import augment as A
    dev = torch.device("cuda")
    color, depth = frames()
    dcolor, ddepth = torch.from_numpy(color).to(dev), torch.from_numpy(depth.view(np.int16)).to(dev)
    gen = torch.Generator(dev).manual_seed(0)
    noise = torch.randn((B, H, W), device=dev, generator=gen)
    gp = torch.randn((B, 3, H // 4, W // 4), device=dev, generator=gen)
    t = table()
    f = A.unpack_table(t)
    c, z, xyz = torch_restatement(torch, F, dcolor, ddepth, noise, gp, f)
    torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        t0 = time.perf_counter()
        torch_restatement(torch, F, dcolor, ddepth, noise, gp, f)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    p = A.AugmentParams(t, noise.cpu().numpy(), gp.cpu().numpy()).to(dev)
    kc, kz = A.augment_color(dcolor, p), A.augment_depth(ddepth, p)
    print(json.dumps({"probe": "augment/torch", "B": B, "size": [H, W], "wall_ms_median": round(float(np.median(ms)), 2),
                      "wall_ms_min": round(float(np.min(ms)), 2),
                      "colour_bytes_differing_from_the_kernel": int((c != kc).sum()), "depth_pixels_differing_from_the_kernel": int((z != kz).sum())}))


def step_host():
    import torch
    from unseenobjectswithmeanshift_amd import augment as A, targets as tg
    dev = torch.device("cuda")
    color, depth = frames()
    rng = np.random.default_rng(0)
    noise = rng.normal(size=(B, H, W)).astype(np.float32)
    gp = rng.normal(size=(B, 3, H // 4, W // 4)).astype(np.float32)
    host = A.AugmentParams(table(), noise, gp)
    raw = np.zeros((B, H, W), np.uint8)
    ms, parts = [], {}
    for _ in range(3):
        t0 = time.perf_counter()
        c = A.augment_color(color, host)
        t1 = time.perf_counter()
        z = A.augment_depth(depth, host)
        t2 = time.perf_counter()
        image, xyz, _ = tg.training_batch(c, z, raw, CAM)
        A.add_xyz_noise_(xyz, host)
        t3 = time.perf_counter()
        ms.append((t3 - t0) * 1e3)
        parts = {"color_ms": round((t1 - t0) * 1e3, 1), "depth_ms": round((t2 - t1) * 1e3, 1), "ingest_targets_xyz_ms": round((t3 - t2) * 1e3, 1)}
    fimage, fxyz = image.pin_memory(), xyz.pin_memory()
    pc, pd = torch.from_numpy(color).pin_memory(), torch.from_numpy(depth.view(np.int16)).pin_memory()
    d_image, d_xyz, d_c, d_d = (torch.empty_like(t, device=dev) for t in (fimage, fxyz, pc, pd))

    def up_float():
        d_image.copy_(fimage, non_blocking=True)
        d_xyz.copy_(fxyz, non_blocking=True)

    def up_raw():
        d_c.copy_(pc, non_blocking=True)
        d_d.copy_(pd, non_blocking=True)

    out = {"probe": "augment/host", "B": B, "size": [H, W], "host_numpy_ms_median": round(float(np.median(ms)), 1), "last_run": parts,
           "upload_float_image_and_xyz": {"bytes": fimage.numel() * 4 + fxyz.numel() * 4, "us": timed(torch, up_float, 3)},
           "upload_raw_frames": {"bytes": pc.numel() + 2 * pd.numel(), "us": timed(torch, up_raw, 10)}}
    p = host.to(dev)
    dimage, dxyz, _ = tg.training_batch(torch.from_numpy(color).to(dev), torch.from_numpy(depth.view(np.int16)).to(dev),
                                        torch.from_numpy(raw).to(dev), CAM, augment=p)
    himage, hxyz, _ = tg.training_batch(color, depth, raw, CAM, augment=host)
    out["device_equals_host"] = bool(torch.equal(dimage.cpu(), himage)) and bool(torch.equal(dxyz.cpu(), hxyz))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    args = ap.parse_args()
    if args.step:
        return {"kernels": step_kernels, "torch": step_torch, "host": step_host}[args.step]()
    for step in ("kernels", "torch", "host"):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step], timeout=STEPS[step]).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({"probe": f"augment/{step}", "error": f"no result within {STEPS[step]} s"}))
            return 1
        if rc != 0:
            print(json.dumps({"probe": f"augment/{step}", "error": f"exit status {rc}"}))
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
