"""Time the deterministic MSDeformAttn backward (msm_msdeform_attn_bwd_det) against the atomic one (msm_msdeform_attn_bwd) in the
same run, on the pixel decoder's encoder shapes, and one pixel-decoder training step with torch's deterministic flag on and off.

    python tools/probes/msda_backward_time.py [--batches 2 8] [--size 480 640] [--windows 7] [--calls 20]

Encoder shapes of tools/probes/pixel_decoder_backward_time.py: the res5 / res4 / res3 maps of an H x W frame (15x20, 30x40, 60x80 at
480 x 640: S = Lq = 6300), M = 8 heads of D = 8 channels, L = 3 levels x P = 4 points; sampling locations = pixel centre + N(0, 2)
pixels, softmax weights, N(0, 1) values and gradients, seeded.  A window is ``calls`` back-to-back calls between two HIP events; the
two forms alternate window by window after a warm-up of both; the figure is the median over the windows, per call, with the
smallest and largest window beside it.  Per batch size one JSON line: the two times, their ratio, the bytes the deterministic
form's accumulate pass adds with 64-bit integer atomics and the rate that time implies IF the whole deterministic call were that
pass (a lower bound of the pass's rate), the same for the atomic form's fp32 adds, the workspace bytes, and whether two
deterministic calls gave equal bits.  Then the training step (training.pixel_decoder_forward_train + backward of a random linear
functional) under torch.use_deterministic_algorithms(True) and (False), alternating.  Records, not gates."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from unseenobjectswithmeanshift_amd import ops, training  # noqa: E402
from unseenobjectswithmeanshift_amd import synthetic as syn  # noqa: E402
from unseenobjectswithmeanshift_amd.meta_arch import build_resnet50_head  # noqa: E402

M, D, P = 8, 8, 4


def window_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def alternate(fns, windows, calls):
    """{name: (median, min, max) ms per call}: every fn warmed up, then ``windows`` rounds of one window each, in turn"""
    for fn in fns.values():
        fn()
        fn()
    times = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            times[k].append(window_ms(fn, calls))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def encoder_inputs(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    levels = [(H // 32, W // 32), (H // 16, W // 16), (H // 8, W // 8)]
    S = sum(h * w for h, w in levels)
    shapes = torch.tensor(levels, dtype=torch.int64)
    start = torch.cat((shapes.new_zeros(1), shapes.prod(1).cumsum(0)[:-1]))
    ref = torch.cat([torch.stack(torch.meshgrid((torch.arange(h) + 0.5) / h, (torch.arange(w) + 0.5) / w, indexing="ij")[::-1], -1).reshape(h * w, 2)
                     for h, w in levels])
    wh = torch.tensor([[w, h] for h, w in levels], dtype=torch.float32)
    off = torch.randn(B, S, M, len(levels), P, 2, generator=g) * 2.0
    loc = ref[None, :, None, None, None, :] + off / wh[None, None, None, :, None, :]
    aw = torch.softmax(torch.randn(B, S, M, len(levels) * P, generator=g), -1).view(B, S, M, len(levels), P)
    value = torch.randn(B, S, M, D, generator=g)
    go = torch.randn(B, S, M * D, generator=g)
    return [t.cuda().contiguous() for t in (value, shapes, start, loc, aw, go)], levels, S


def in_range_corners(loc, levels):
    """number of (query, head, point, corner) that land on a pixel: each adds D values to grad_value"""
    n = 0
    for l, (h, w) in enumerate(levels):
        x, y = loc[:, :, :, l, :, 0] * w - 0.5, loc[:, :, :, l, :, 1] * h - 0.5
        inside = (x > -1) & (y > -1) & (x < w) & (y < h)
        x0, y0 = torch.floor(x), torch.floor(y)
        for dy in (0, 1):
            for dx in (0, 1):
                n += int((inside & (y0 + dy >= 0) & (y0 + dy <= h - 1) & (x0 + dx >= 0) & (x0 + dx <= w - 1)).sum())
    return n


def run_kernels(B, H, W, windows, calls):
    args, levels, S = encoder_inputs(B, H, W, 40 + B)
    ws = torch.empty(ops.ms_deform_attn_backward_det_workspace(B, S, M, D), dtype=torch.uint8, device="cuda")
    fns = {"atomic": lambda: ops.ms_deform_attn_backward(*args, deterministic=False),
           "deterministic": lambda: ops.ms_deform_attn_backward(*args, deterministic=True, workspace=ws)}
    t = alternate(fns, windows, calls)
    a, b = fns["deterministic"](), fns["deterministic"]()
    c = fns["atomic"]()
    corners = in_range_corners(args[3].cpu(), levels)
    det_ms, at_ms = t["deterministic"][0], t["atomic"][0]
    out = {"gpu": torch.cuda.get_device_name(0), "B": B, "size": [H, W], "S": S, "M": M, "D": D, "L": len(levels), "P": P,
           "windows": windows, "calls_per_window": calls,
           "atomic_ms": round(at_ms, 4), "atomic_ms_min_max": [round(v, 4) for v in t["atomic"][1:]],
           "deterministic_ms": round(det_ms, 4), "deterministic_ms_min_max": [round(v, 4) for v in t["deterministic"][1:]],
           "deterministic_over_atomic": round(det_ms / at_ms, 3),
           "added_values": corners * D,
           "int64_added_GBps_if_whole_call_were_the_accumulate_pass": round(corners * D * 8 / det_ms / 1e6, 1),
           "f32_added_GBps_of_the_atomic_call": round(corners * D * 4 / at_ms / 1e6, 1),
           "workspace_bytes": ws.numel(),
           "deterministic_calls_equal": all(torch.equal(x, y) for x, y in zip(a, b)),
           "deterministic_vs_atomic_max_abs_grad_value": float((a[0] - c[0]).abs().max())}
    print(json.dumps(out), flush=True)


def run_step(B, H, W, windows, calls):
    head = build_resnet50_head()
    head.pixel_decoder.load_state_dict(syn.synth_state_dict(syn.pixel_decoder_param_shapes()), strict=True)
    pd = head.pixel_decoder.cuda()
    feats = {k: v.cuda().requires_grad_(True) for k, v in syn.synth_backbone_features(B, H, W, seed=B).items()}
    leaves = list(feats.values()) + list(pd.parameters())
    with torch.no_grad():
        mf, _, ms = training.pixel_decoder_forward_train(pd, feats)
    g = torch.Generator().manual_seed(B)
    weights = [(torch.randn(tuple(t.shape), generator=g) / (t.shape[-2] * t.shape[-1]) ** 0.5).cuda() for t in [mf] + list(ms)]
    del mf, ms

    def step(flag):
        was, was_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
        torch.use_deterministic_algorithms(flag)
        try:
            for t in leaves:
                t.grad = None
            mf, _, ms = training.pixel_decoder_forward_train(pd, feats)
            sum((t * w).sum() for t, w in zip([mf] + list(ms), weights)).backward()
        finally:
            torch.use_deterministic_algorithms(was, warn_only=was_warn)

    t = alternate({"flag_off": lambda: step(False), "flag_on": lambda: step(True)}, windows, calls)
    step(True)
    first = [x.grad.clone() for x in leaves]
    step(True)
    out = {"gpu": torch.cuda.get_device_name(0), "B": B, "size": [H, W], "pixel_decoder_step": True, "windows": windows, "calls_per_window": calls,
           "flag_off_ms": round(t["flag_off"][0], 3), "flag_off_ms_min_max": [round(v, 3) for v in t["flag_off"][1:]],
           "flag_on_ms": round(t["flag_on"][0], 3), "flag_on_ms_min_max": [round(v, 3) for v in t["flag_on"][1:]],
           "flag_on_over_off": round(t["flag_on"][0] / t["flag_off"][0], 3),
           "flag_on_steps_equal": all(torch.equal(a, x.grad) for a, x in zip(first, leaves))}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=(2, 8))
    ap.add_argument("--size", type=int, nargs=2, default=(480, 640))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--step-batch", type=int, default=2, help="batch size of the pixel-decoder step (0: skip it)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("msda_backward_time.py needs a GPU")
    for B in a.batches:
        run_kernels(B, a.size[0], a.size[1], a.windows, a.calls)
    if a.step_batch > 0:
        run_step(a.step_batch, a.size[0], a.size[1], a.windows, max(1, a.calls // 4))


if __name__ == "__main__":
    main()
