"""Time the pixel decoder under training (training.pixel_decoder_forward_train) against a torch restatement on the same GPU, same
weights, same run, and the two kernels of csrc/norm_bwd.hip alone against their traffic floors.

    python tools/probes/pixel_decoder_backward_time.py [--batches 2 8] [--size 480 640] [--reps 5]

The restatement is the reference's forward_features in torch's own operators (F.conv2d, F.group_norm, F.interpolate, F.linear,
F.layer_norm and their autograd) with the package's MSDeformAttnFunction for the core.  Prints one JSON line per batch size:
milliseconds (HIP events around one call, median of ``reps`` synchronised repeats after a warm-up) of the forward and of forward +
backward of both routes, the HIP route's time by library entry point (HIP events around every call of one more step), how far the
two routes' gradients are apart (on this random-weight model at 480 x 640 that figure varies from run to run, and both fp32 routes
sit percents of the largest entry away from a float64 run: DESIGN 5t), and for msm_groupnorm_bwd_f32 /
msm_upsample_bilinear_bwd_tokens_f32 on the res2-level maps the time, the bytes the algorithm needs (GroupNorm backward: 4 reads + 1 write of the map; upsampling backward: one
read of the fine map + one write of the coarse one), the time of torch's own backward of the same operator, and the share of the
floor bytes / 8.0 TB/s (HBM3E peak; a float4 copy reaches 6.29 TB/s on this part).  Records, not gates."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from unseenobjectswithmeanshift_amd import _lib, ops, training  # noqa: E402
from unseenobjectswithmeanshift_amd import synthetic as syn  # noqa: E402
from unseenobjectswithmeanshift_amd.meta_arch import build_resnet50_head  # noqa: E402

PEAK_TBS = 8.0               # HBM3E, MI355X


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


def torch_forward(pd, features):
    """msdeformattn.py:315-358 in torch's operators; the MSDeformAttn core is the package's (torch has none)."""
    C = pd.conv_dim
    names = pd.transformer_in_features[::-1]
    dev = features[names[0]].device
    srcs, pos, ref, shapes = [], [], [], []
    for idx, f in enumerate(names):
        x = features[f]
        h, w = int(x.shape[2]), int(x.shape[3])
        shapes.append((h, w))
        conv, gn = pd.input_proj[idx][0], pd.input_proj[idx][1]
        y = F.group_norm(F.conv2d(x, conv.weight, conv.bias), gn.num_groups, gn.weight, gn.bias, gn.eps)
        srcs.append(y.flatten(2).transpose(1, 2))
        pos.append(ops.pos_embed_sine(h, w, pd.pe_layer.num_pos_feats, dev, layout="tokens") + pd.transformer.level_embed[idx])
        ys = (torch.arange(h, device=dev, dtype=torch.float32) + 0.5) / h
        xs = (torch.arange(w, device=dev, dtype=torch.float32) + 0.5) / w
        ref.append(torch.stack([xs[None, :].expand(h, w), ys[:, None].expand(h, w)], -1).reshape(h * w, 2))
    src, pos, ref = torch.cat(srcs, 1), torch.cat(pos, 0), torch.cat(ref, 0)
    B, S, _ = src.shape
    sizes = [h * w for h, w in shapes]
    starts_host = [sum(sizes[:i]) for i in range(len(sizes))]
    ss = torch.tensor(shapes, dtype=torch.int64, device=dev)
    starts = torch.tensor(starts_host, dtype=torch.int64, device=dev)
    norm_wh = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float32, device=dev)
    for layer in pd.transformer.encoder.layers:
        a = layer.self_attn
        M, L, P = a.n_heads, a.n_levels, a.n_points
        q = src + pos
        value = F.linear(src, a.value_proj.weight, a.value_proj.bias).view(B, S, M, C // M)
        off = F.linear(q, a.sampling_offsets.weight, a.sampling_offsets.bias).view(B, S, M, L, P, 2)
        aw = F.softmax(F.linear(q, a.attention_weights.weight, a.attention_weights.bias).view(B, S, M, L * P), -1).view(B, S, M, L, P)
        loc = ref[None, :, None, None, None, :] + off / norm_wh[None, None, None, :, None, :]
        o = training.MSDeformAttnFunction.apply(value, ss, starts, loc.contiguous(), aw.contiguous(), a.im2col_step)
        src = F.layer_norm(src + F.linear(o, a.output_proj.weight, a.output_proj.bias), (C,), layer.norm1.weight, layer.norm1.bias, layer.norm1.eps)
        f = F.linear(F.relu(F.linear(src, layer.linear1.weight, layer.linear1.bias)), layer.linear2.weight, layer.linear2.bias)
        src = F.layer_norm(src + f, (C,), layer.norm2.weight, layer.norm2.bias, layer.norm2.eps)
    out = [src[:, o:o + n].transpose(1, 2).reshape(B, C, h, w) for o, n, (h, w) in zip(starts_host, sizes, shapes)]
    x = features[pd.in_features[0]]
    an, ln = pd.adapter_1.norm, pd.layer_1.norm
    lat = F.group_norm(F.conv2d(x, pd.adapter_1.weight), an.num_groups, an.weight, an.bias, an.eps)
    y = lat + F.interpolate(out[-1], size=lat.shape[-2:], mode="bilinear", align_corners=False)
    y = F.relu(F.group_norm(F.conv2d(y, pd.layer_1.weight, padding=1), ln.num_groups, ln.weight, ln.bias, ln.eps))
    out.append(y)
    return F.conv2d(y, pd.mask_features.weight, pd.mask_features.bias), out[0], out[:pd.maskformer_num_feature_levels]


def functional(mf, ms, weights):
    return sum((t * w).sum() for t, w in zip([mf] + list(ms), weights))


def kernels_alone(B, H, W, reps):
    """The two new kernels on the res2-level maps (B, H*W, 64), and torch's backward of the same operator on NCHW planes."""
    g = torch.Generator().manual_seed(100 + B)
    HW, C, h, w = H * W, 64, H // 2, W // 2
    x = (torch.randn(B, HW, C, generator=g) + 0.5).cuda()
    gout = torch.randn(B, HW, C, generator=g).cuda()
    gamma, beta = (1 + 0.1 * torch.randn(C, generator=g)).cuda(), (0.1 * torch.randn(C, generator=g)).cuda()
    stats = ops.groupnorm_stats(x)
    out = {}
    map_bytes = 4.0 * B * HW * C
    ms = median_ms(lambda: ops.groupnorm_backward(x, gout, stats, gamma, beta, 32, relu=True), reps)
    xp = x.transpose(1, 2).reshape(B, C, H, W).contiguous().requires_grad_(True)
    gp = gout.transpose(1, 2).reshape(B, C, H, W).contiguous()
    gt, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    yt = F.relu(F.group_norm(xp, 32, gt, bt, 1e-5))
    ms_t = median_ms(lambda: torch.autograd.grad(yt, [xp, gt, bt], gp, retain_graph=True), reps)
    out["groupnorm_bwd"] = {"ms": round(ms, 4), "floor_bytes": 5 * map_bytes, "achieved_TBps": round(5 * map_bytes / ms / 1e9, 3),
                            "of_hbm_peak": round(5 * map_bytes / ms / 1e9 / PEAK_TBS, 3), "torch_relu_groupnorm_bwd_ms": round(ms_t, 4)}
    ms = median_ms(lambda: ops.upsample_bilinear_backward(gout, (h, w), (H, W)), reps)
    zp = torch.randn(B, C, h, w, generator=g).cuda().requires_grad_(True)
    up = F.interpolate(zp, size=(H, W), mode="bilinear", align_corners=False)
    ms_t = median_ms(lambda: torch.autograd.grad(up, [zp], gp, retain_graph=True), reps)
    nbytes = map_bytes * 1.25
    out["upsample_bwd"] = {"ms": round(ms, 4), "floor_bytes": nbytes, "achieved_TBps": round(nbytes / ms / 1e9, 3),
                           "of_hbm_peak": round(nbytes / ms / 1e9 / PEAK_TBS, 3), "torch_interpolate_bwd_ms": round(ms_t, 4)}
    return out


def run(B, H, W, reps):
    head = build_resnet50_head()
    head.pixel_decoder.load_state_dict(syn.synth_state_dict(syn.pixel_decoder_param_shapes()), strict=True)
    pd = head.pixel_decoder.cuda()
    params = list(pd.parameters())
    feats = {k: v.cuda().requires_grad_(True) for k, v in syn.synth_backbone_features(B, H, W, seed=B).items()}
    leaves = list(feats.values()) + params
    with torch.no_grad():
        mf, _, ms = training.pixel_decoder_forward_train(pd, feats)
    g = torch.Generator().manual_seed(B)
    weights = [(torch.randn(tuple(t.shape), generator=g) / (t.shape[-2] * t.shape[-1]) ** 0.5).cuda() for t in [mf] + list(ms)]
    del mf, ms

    def clear():
        for t in leaves:
            t.grad = None

    def fwd(route):
        with torch.no_grad():
            route(pd, feats)

    def fwd_bwd(route):
        clear()
        mf, _, ms = route(pd, feats)
        functional(mf, ms, weights).backward()

    out = {"gpu": torch.cuda.get_device_name(0), "B": B, "size": [H, W], "reps": reps}
    t = {}
    t["hip_fwd"] = median_ms(lambda: fwd(training.pixel_decoder_forward_train), reps)
    t["hip_fwd_bwd"] = median_ms(lambda: fwd_bwd(training.pixel_decoder_forward_train), reps)
    hip = [x.grad.clone() for x in leaves]
    t["torch_fwd"] = median_ms(lambda: fwd(torch_forward), reps)
    t["torch_fwd_bwd"] = median_ms(lambda: fwd_bwd(torch_forward), reps)
    out["ms"] = {k: round(v, 3) for k, v in t.items()}
    # where the HIP route's forward + backward goes: HIP events around every library call of one more step (the rest is torch glue)
    with _lib.CallTimer() as timer:
        fwd_bwd(training.pixel_decoder_forward_train)
        torch.cuda.synchronize()
    by_entry = {k: sum(v) for k, v in timer.durations().items()}
    out["hip_fwd_bwd_library_ms"] = round(sum(by_entry.values()), 3)
    out["hip_fwd_bwd_by_entry_point_ms"] = {k: round(v, 3) for k, v in sorted(by_entry.items(), key=lambda kv: -kv[1])[:8]}
    rel = [float((a - x.grad).abs().max() / x.grad.abs().max()) for a, x in zip(hip, leaves)]
    out["hip_vs_torch_worst_rel_of_max"] = {"inputs": max(rel[:4]), "parameters": max(rel[4:])}
    clear()
    del hip
    out["kernels_alone_res2"] = kernels_alone(B, H // 4, W // 4, reps)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=(2, 8))
    ap.add_argument("--size", type=int, nargs=2, default=(480, 640))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pixel_decoder_backward_time.py needs a GPU")
    for B in a.batches:
        run(B, a.size[0], a.size[1], a.reps)


if __name__ == "__main__":
    main()
