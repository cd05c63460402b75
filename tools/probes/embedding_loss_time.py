"""Time EmbeddingLoss: the fused HIP path (embedding_loss.EmbeddingLoss, HIP events) against a plain-torch restatement of the
reference's loop over the clusters (lib/networks/embedding.py:57-133) on the same GPU, same tensors, same run.

    python tools/probes/embedding_loss_time.py [--batch 8] [--channels 64] [--size 480 640] [--clusters 20] [--reps 10]
                                               [--max-clusters N] [--check64]

Prints one JSON line: milliseconds (HIP events, a window of at least 0.3 s per figure) for forward and forward + backward of both routes, the bytes of x, the floor of a forward +
backward (3 reads + 1 write of x, plus the labels) and the bandwidth the fused path reaches against that floor, and how far the
two routes' losses and gradients are apart; with --check64 also how far each is from the restatement run in float64."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from unseenobjectswithmeanshift_amd.embedding_loss import EmbeddingLoss  # noqa: E402


def torch_loss(x, masks, alpha, delta, lambda_intra, lambda_inter):
    """The reference's cosine / normalised forward, loop for loop: K (B,C,H,W) temporaries for the means, K for the tiled
    means, K (B,H,W) for the weights, and one .item() for K."""
    B = x.shape[0]
    K = int(masks.max().item()) + 1
    means = []
    for k in range(K):
        m = (masks == k).float()
        means.append((x * m).sum(dim=(2, 3)) / (m.sum(dim=(2, 3)) + 1e-10))
    means = F.normalize(torch.stack(means, dim=2), p=2, dim=1)                      # (B,C,K)
    tiled = torch.zeros_like(x)
    for k in range(K):
        tiled = tiled + (masks == k).float() * means[:, :, k, None, None]
    labelled = (masks >= 0).squeeze(1).float()
    d = labelled * (0.5 * (1 - (x * tiled).sum(dim=1)))
    if ((d - alpha) > 0).float().sum() > 0:
        weights = torch.zeros_like(d)
        for k in range(K):
            m = (masks == k).float().squeeze(1)
            weights = weights + m * ((d > alpha).float() * m).sum(dim=(1, 2), keepdim=True)
        intra = lambda_intra * (d.pow(2) / (weights.clamp(min=50.0) * K)).sum() / B
    else:
        intra = x.sum() * 0
    if K > 1:
        dist = 0.5 * (1 - (means.unsqueeze(2) * means.unsqueeze(3)).sum(dim=1))
        hinge = (delta - dist).clamp(min=0) * (1 - torch.eye(K, device=x.device))
        inter = lambda_inter * hinge.pow(2).sum() / (K * (K - 1) / 2 * B)
    else:
        inter = x.sum() * 0
    return intra + inter, intra, inter


def planted(B, C, H, W, K, seed=0):
    g = torch.Generator().manual_seed(seed)
    protos = F.normalize(torch.randn(K, C, generator=g), dim=1)
    coarse = torch.randint(0, K, (B, (H + 31) // 32, (W + 31) // 32), generator=g)          # 32 x 32 blocks: object-sized regions
    labels = coarse.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :H, :W].clone()
    x = F.normalize(protos[labels] + 0.3 * torch.randn(B, H, W, C, generator=g) / C ** 0.5, dim=3).permute(0, 3, 1, 2).contiguous()
    labels = labels.float()
    labels[torch.rand(B, H, W, generator=g) < 0.1] = -1
    return x, labels.reshape(B, 1, H, W)


def time_ms(fn, reps, min_window_ms=300.0):
    """Mean milliseconds per call by HIP events, after a warm-up, over at least ``reps`` calls and ``min_window_ms`` of work."""
    def window(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    fn()
    first = window(reps)
    more = int(min_window_ms / max(first, 1e-3)) + 1
    return first if more <= reps else window(more)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--size", type=int, nargs=2, default=(480, 640))
    ap.add_argument("--clusters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--max-clusters", type=int, default=None, help="rows of the cluster table (default min(64, 16384 // C))")
    ap.add_argument("--check64", action="store_true", help="also run the torch restatement in float64 and report both errors")
    a = ap.parse_args()
    H, W = a.size
    x, labels = planted(a.batch, a.channels, H, W, a.clusters)
    x, labels = x.cuda().requires_grad_(True), labels.cuda()
    alpha, delta = 0.02, 0.5
    crit = EmbeddingLoss(alpha, delta, 1.0, 1.0, max_clusters=a.max_clusters)

    def fused_fwd():
        with torch.no_grad():
            return crit(x, labels)

    def fused_fwd_bwd():
        x.grad = None
        crit(x, labels)[0].backward()

    def torch_fwd():
        with torch.no_grad():
            return torch_loss(x, labels, alpha, delta, 1.0, 1.0)

    def torch_fwd_bwd():
        x.grad = None
        torch_loss(x, labels, alpha, delta, 1.0, 1.0)[0].backward()

    out = {"B": a.batch, "C": a.channels, "size": [H, W], "K": a.clusters, "max_clusters": a.max_clusters, "x_bytes": x.numel() * 4}
    out["fused_fwd_ms"] = round(time_ms(fused_fwd, a.reps), 3)
    out["fused_fwd_bwd_ms"] = round(time_ms(fused_fwd_bwd, a.reps), 3)
    fused_losses, fused_grad = [float(v) for v in fused_fwd()], x.grad.clone()
    crit.check()
    out["torch_fwd_ms"] = round(time_ms(torch_fwd, a.torch_reps), 3)
    out["torch_fwd_bwd_ms"] = round(time_ms(torch_fwd_bwd, a.torch_reps), 3)
    torch_losses = [float(v) for v in torch_fwd()]
    floor = 4 * x.numel() * 4 + 3 * labels.numel() * 4                       # 3 reads + 1 write of x, the labels once per pass
    out["floor_bytes"] = floor
    out["fused_fwd_bwd_GBps_of_floor"] = round(floor / (out["fused_fwd_bwd_ms"] * 1e-3) / 1e9, 1)
    out["fused_fwd_GBps_of_2_reads"] = round((2 * x.numel() * 4 + 2 * labels.numel() * 4) / (out["fused_fwd_ms"] * 1e-3) / 1e9, 1)
    out["speedup_fwd"] = round(out["torch_fwd_ms"] / out["fused_fwd_ms"], 2)
    out["speedup_fwd_bwd"] = round(out["torch_fwd_bwd_ms"] / out["fused_fwd_bwd_ms"], 2)
    out["losses_fused"], out["losses_torch"] = fused_losses, torch_losses
    out["grad_max_diff_rel"] = float((fused_grad - x.grad).abs().max() / x.grad.abs().max())
    if a.check64:
        torch_grad = x.grad.clone()
        x64 = x.detach().double().requires_grad_(True)
        l64 = torch_loss(x64, labels, alpha, delta, 1.0, 1.0)
        l64[0].backward()
        l64 = [float(v.detach()) for v in l64]
        gmax = x64.grad.abs().max()
        rel = lambda got: max(abs(g - r) / abs(r) for g, r in zip(got, l64) if r != 0)  # noqa: E731
        out["fused_vs_f64"] = {"loss_rel": rel(fused_losses), "grad_rel_of_max": float((fused_grad.double() - x64.grad).abs().max() / gmax)}
        out["torch_vs_f64"] = {"loss_rel": rel(torch_losses), "grad_rel_of_max": float((torch_grad.double() - x64.grad).abs().max() / gmax)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
