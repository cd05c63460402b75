"""Timing of msm_instance_postprocess_resized (instance masks at a requested output size) at B = 8, T = 20, HIP events around
each launch (the library entry on preallocated buffers: resize kernel + finishing kernel), median of 30 after a warm-up:
  up    low 120x160 -> frame and image 480x640 -> output 960x1280
  down  low 200x272 -> frame 800x1088, image 800x1067 -> output 480x640
each next to the torch chain on the same selected maps (two F.interpolate calls, the threshold, the sigmoid and the mean ops),
and the identity kernel (msm_instance_postprocess) at 480x640.  GB/s = bytes of masks written / time.  Prints one JSON line."""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from unseenobjectswithmeanshift_amd import _lib  # noqa: E402
from unseenobjectswithmeanshift_amd.ops import _p, _stream  # noqa: E402

B, Q, T, N = 8, 100, 20, 30


def timed(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(N):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(us)), float(np.min(us))


def case(name, low_hw, frame, image, out, direct=False):
    L = _lib.lib()
    g = torch.Generator().manual_seed(3)
    low = (2.0 * torch.randn(B, Q, *low_hw, generator=g)).cuda()
    qidx = torch.stack([torch.randperm(Q, generator=g)[:T] for _ in range(B)]).to(torch.int32).cuda()
    masks = torch.empty(B, T, *out, device="cuda")
    score, boxes = torch.empty(B, T, device="cuda"), torch.empty(B, T, 4, device="cuda")
    ws = torch.empty(int(L.msm_instance_postprocess_workspace(B, T, *out)), device="cuda")
    identity = tuple(out) == tuple(image)

    def kernel():
        if identity:
            rc = L.msm_instance_postprocess(_p(low), _p(qidx), None, _p(masks), _p(score), _p(boxes), B, Q, T, *low_hw, *image, *frame,
                                            _p(ws), _stream())
        else:
            rc = L.msm_instance_postprocess_resized(_p(low), _p(qidx), None, _p(masks), _p(score), _p(boxes), B, Q, T, *low_hw, *image,
                                                    *frame, *out, _p(ws), _stream())
        _lib.check(rc, name)

    sel = torch.gather(low, 1, qidx.long()[:, :, None, None].expand(-1, -1, *low_hw)).contiguous()

    def chain():
        u = F.interpolate(sel, size=frame, mode="bilinear", align_corners=False)[..., :image[0], :image[1]]
        r = u if identity else F.interpolate(u, size=out, mode="bilinear", align_corners=False)
        binm = (r > 0).float()
        return binm, (r.sigmoid() * binm).flatten(2).sum(2) / (binm.flatten(2).sum(2) + 1e-6)

    if direct:
        with _lib.option("POST_RESIZE_DIRECT", 1):
            k_med, k_min = timed(kernel)
    else:
        k_med, k_min = timed(kernel)
    binm, sc = chain()
    res = {"kernel_us_median": round(k_med, 1), "kernel_us_min": round(k_min, 1),
           "mask_bytes": masks.numel() * 4, "kernel_GBps": round(masks.numel() * 4 / k_med / 1e3, 1),
           "ns_per_output_KB": round(k_med * 1e3 / (masks.numel() * 4 / 1024), 3)}
    if not direct:
        t_med, _ = timed(chain)
        res.update({"torch_chain_us_median": round(t_med, 1), "mask_mismatch_vs_torch": float((binm != masks).float().mean()),
                    "score_max_abs_diff_vs_torch": float((sc - score).abs().max())})
    return res


def main():
    out = {"probe": "postprocess_resize", "B": B, "T": T, "launches": N,
           "up_120x160_480x640_960x1280": case("up", (120, 160), (480, 640), (480, 640), (960, 1280)),
           "down_200x272_800x1067_480x640": case("down", (200, 272), (800, 1088), (800, 1067), (480, 640)),
           "up_direct_loads": case("up_direct", (120, 160), (480, 640), (480, 640), (960, 1280), direct=True),
           "identity_120x160_480x640": case("identity", (120, 160), (480, 640), (480, 640), (480, 640))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
