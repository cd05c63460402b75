"""Time the 3x3 mask_features convolution under training (training.conv3x3: forward on csrc/conv3x3.hip, weight / bias gradient on
csrc/conv3x3_bwd.hip, input gradient on the implicit GEMM) against torch.nn.functional.conv2d and its autograd on the same GPU, same
tensors, same run.

    python tools/probes/conv3x3_backward_time.py [--batches 2 8] [--size 480 640] [--cout 256] [--reps 5] [--splits N]

Prints one JSON line per batch size: milliseconds (HIP events around one call, median of ``reps`` synchronised repeats after a
warm-up) of the weight gradient, the input gradient, the forward and forward + backward of both routes, TFLOP/s of each HIP figure
against the fp32 MFMA peak (157.3 TFLOP/s), and how far the two routes' results are apart.  Records, not gates."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from unseenobjectswithmeanshift_amd import ops, training  # noqa: E402

PEAK_TFLOPS = 157.3          # fp32-input MFMA, MI355X


def median_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def run(B, H, W, Cout, reps, splits):
    g = torch.Generator().manual_seed(B)
    x = F.normalize(torch.randn(B, 64, H, W, generator=g), dim=1).cuda().requires_grad_(True)
    w = (torch.randn(Cout, 64, 3, 3, generator=g) * (2.0 / 576) ** 0.5).cuda().requires_grad_(True)
    bias = (0.1 * torch.randn(Cout, generator=g)).cuda().requires_grad_(True)
    gout = torch.randn(B, Cout, H, W, generator=g).cuda()
    tok = ops.transpose_last2(x.detach().view(B, 64, H * W))
    flop = 2.0 * B * H * W * Cout * 576           # of the forward, and of each of the two gradients

    def clear():
        x.grad = w.grad = bias.grad = None

    def hip_fwd():
        with torch.no_grad():
            return training.conv3x3(x, w, bias)

    def hip_fwd_bwd():
        clear()
        training.conv3x3(x, w, bias).backward(gout)

    def torch_fwd():
        with torch.no_grad():
            return F.conv2d(x, w, bias, padding=1)

    def torch_fwd_bwd():
        clear()
        F.conv2d(x, w, bias, padding=1).backward(gout)

    out = {"gpu": torch.cuda.get_device_name(0), "B": B, "size": [H, W], "Cout": Cout, "splits": splits, "reps": reps,
           "gflop_per_pass": round(flop / 1e9, 1)}
    ms = {}
    ms["hip_wgrad"] = median_ms(lambda: ops.conv3x3_weight_grad(tok, gout, H, W, splits=splits), reps)
    ms["hip_input_grad"] = median_ms(lambda: ops.conv3x3_input_grad(gout, w.detach(), H, W), reps)
    ms["hip_fwd"] = median_ms(hip_fwd, reps)
    ms["hip_fwd_bwd"] = median_ms(hip_fwd_bwd, reps)
    hip = [t.clone() for t in (x.grad, w.grad, bias.grad)]
    ms["torch_fwd"] = median_ms(torch_fwd, reps)
    ms["torch_fwd_bwd"] = median_ms(torch_fwd_bwd, reps)
    out["ms"] = {k: round(v, 3) for k, v in ms.items()}
    out["tflops"] = {"hip_wgrad": round(flop / ms["hip_wgrad"] / 1e9, 1), "hip_input_grad": round(flop / ms["hip_input_grad"] / 1e9, 1),
                     "hip_fwd": round(flop / ms["hip_fwd"] / 1e9, 1), "hip_fwd_bwd": round(3 * flop / ms["hip_fwd_bwd"] / 1e9, 1),
                     "torch_fwd": round(flop / ms["torch_fwd"] / 1e9, 1), "torch_fwd_bwd": round(3 * flop / ms["torch_fwd_bwd"] / 1e9, 1)}
    out["of_fp32_mfma_peak"] = {k: round(v / PEAK_TFLOPS, 3) for k, v in out["tflops"].items()}
    out["hip_vs_torch_rel_of_max"] = {n: float((a - b).abs().max() / b.abs().max())
                                      for n, a, b in zip(("dx", "dw", "db"), hip, (x.grad, w.grad, bias.grad))}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=(2, 8))
    ap.add_argument("--size", type=int, nargs=2, default=(480, 640))
    ap.add_argument("--cout", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--splits", type=int, default=None, help="pixel ranges of the weight gradient (default: chosen by shape)")
    a = ap.parse_args()
    for B in a.batches:
        run(B, a.size[0], a.size[1], a.cout, a.reps, a.splits)


if __name__ == "__main__":
    main()
