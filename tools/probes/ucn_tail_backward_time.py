"""Time the backward of the UCN embedding tail (training.ucn_embedding_tail: csrc/backbone_bwd.hip) against torch's autograd backward
of the literal expression (two F.interpolate, +, F.normalize x norms) on the same GPU, same tensors, same run, and one whole
forward + backward of training.ucn_backbone_forward_train with the fused tail on and off (the tail's share of a tower step).

    python tools/probes/ucn_tail_backward_time.py [--batches 2 8] [--size 480 640] [--norms 1 2] [--reps 5] [--no-towers] [--no-tail]

Prints one JSON line per (batch, norms): milliseconds (HIP events, median of ``reps`` synchronised repeats after a warm-up) of the
backward alone and of the forward on both routes, the bytes of gout, the backward's GB/s of gout, and how far the two routes'
gradients are apart; then one line per batch for the tower step.  Records, not gates."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from unseenobjectswithmeanshift_amd import ops, synthetic, training  # noqa: E402
from unseenobjectswithmeanshift_amd.ucn_backbone import UCNBackbone  # noqa: E402


def median_ms(fn, reps, setup=None):
    """Median of ``reps`` timed calls of fn after one warm-up; ``setup`` runs before each call, outside the timed window."""
    if setup:
        setup()
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        if setup:
            setup()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def run_tail(B, H, W, norms, reps):
    g = torch.Generator().manual_seed(B)
    h, w = H // 8, W // 8
    cl = lambda t: t.cuda().contiguous(memory_format=torch.channels_last)
    a = cl(torch.randn(B, 64, h, w, generator=g)).requires_grad_(True)
    b = cl(0.5 * torch.randn(B, 64, h, w, generator=g)).requires_grad_(True)
    gout = torch.randn(B, 64, H, W, generator=g).cuda()
    state = {}

    def clear():
        a.grad = b.grad = None

    def graph(fused):
        def make():
            clear()
            state["y"] = training.ucn_embedding_tail(a, b, (H, W), norms=norms, fused=fused)
        return make

    def backward():
        state.pop("y").backward(gout)

    ms = {}
    ms["hip_bwd"] = median_ms(backward, reps, setup=graph(True))
    hip = a.grad.clone()
    assert torch.equal(a.grad, b.grad)
    ms["hip_bwd_kernels"] = median_ms(lambda: ops.ucn_embedding_tail_bwd(a.detach(), b.detach(), gout, norms=norms), reps)
    ms["torch_bwd"] = median_ms(backward, reps, setup=graph(False))
    ref = a.grad.clone()
    with torch.no_grad():
        ms["hip_fwd"] = median_ms(lambda: training.ucn_embedding_tail(a, b, (H, W), norms=norms), reps)
        ms["torch_fwd"] = median_ms(lambda: training.ucn_embedding_tail(a, b, (H, W), norms=norms, fused=False), reps)
    nbytes = gout.numel() * 4
    print(json.dumps({"gpu": torch.cuda.get_device_name(0), "what": "tail", "B": B, "size": [H, W], "norms": norms, "reps": reps,
                      "gout_mb": round(nbytes / 1e6, 1), "ms": {k: round(v, 3) for k, v in ms.items()},
                      "gout_gb_per_s": {k: round(nbytes / ms[k] / 1e6, 1) for k in ("hip_bwd_kernels", "torch_bwd")},
                      "torch_over_hip_bwd": round(ms["torch_bwd"] / ms["hip_bwd"], 2),
                      "hip_vs_torch_rel_of_max": float((hip - ref).abs().max() / ref.abs().max())}), flush=True)


def run_towers(B, H, W, reps):
    net = UCNBackbone(num_units=64, in_channels=3)
    net.load_state_dict(synthetic.ucn_backbone_state_dict(synthetic.ucn_backbone_param_shapes(), salt=6), strict=True)
    net = net.cuda().train()
    g = torch.Generator().manual_seed(100 + B)
    img = torch.randn(B, 3, H, W, generator=g).cuda()
    depth = (0.5 * torch.randn(B, 3, H, W, generator=g)).cuda()
    gout = torch.randn(B, 64, H, W, generator=g).cuda()

    def step(fused):
        def fn():
            for p in net.parameters():
                p.grad = None
            training.ucn_backbone_forward_train(net, img, depth, renormalize=True, fused_tail=fused).backward(gout)
        return fn

    step(True)(), step(False)()                   # MIOpen picks its solvers at the first call of every shape
    ms = {"fused_tail": median_ms(step(True), reps), "torch_tail": median_ms(step(False), reps)}
    print(json.dumps({"gpu": torch.cuda.get_device_name(0), "what": "backbone forward + backward, norms 2", "B": B, "size": [H, W],
                      "reps": reps, "ms": {k: round(v, 3) for k, v in ms.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=(2, 8))
    ap.add_argument("--size", type=int, nargs=2, default=(480, 640))
    ap.add_argument("--norms", type=int, nargs="+", default=(1, 2))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-towers", action="store_true", help="skip the whole backbone step")
    ap.add_argument("--no-tail", action="store_true", help="skip the tail alone")
    a = ap.parse_args()
    for B in a.batches:
        for norms in ([] if a.no_tail else a.norms):
            run_tail(B, a.size[0], a.size[1], norms, a.reps)
    if not a.no_towers:
        for B in a.batches:
            run_towers(B, a.size[0], a.size[1], a.reps)


if __name__ == "__main__":
    main()
