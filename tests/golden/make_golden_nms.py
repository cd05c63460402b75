"""Generate tests/golden/mask_nms.npz by executing the REFERENCE's nms (lib/fcn/nms.py:3-23) and combine_masks_with_NMS
(lib/fcn/test_utils.py:55-91) -- pure numpy, run through _ref_import.ref_functions like the harness cases of make_golden.py --
on small seeded masks.

Run in the build container only:   python tests/golden/make_golden_nms.py

Per case ``n``: the inputs (``n_masks`` (K,H,W) uint8, ``n_scores`` (K,) float32, ``n_cand`` (K,) bool: the reference sees the
candidates compacted, as get_confident_instances hands them over) and the reference's outputs (``n_label`` / ``n_score`` (H,W)
int16, ``n_bbox`` (N,5) float32, ``n_keep`` (N,) the kept instances as indices into the K inputs, in label order).
Scores and kept areas are distinct in every case (numpy's default argsort leaves ties open; asserted below).  Case ``pair``
holds two masks at IoU exactly 7/10, so the reference decides the <= at the threshold."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ref_import as R  # noqa: E402


class _Inst:
    """Just enough of detectron2.structures.Instances for combine_masks_with_NMS."""

    def __init__(self, **f):
        self.f = f

    def get(self, k):
        return self.f[k]


def rect(H, W, y0, y1, x0, x1):
    m = np.zeros((H, W), dtype=np.uint8)
    m[y0:y1, x0:x1] = 1
    return m


def blobs(seed, K, H, W):
    """K seeded ellipses of assorted sizes (several overlap heavily), distinct scores."""
    g = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    masks = np.zeros((K, H, W), dtype=np.uint8)
    for i in range(K):
        if i % 3 == 2:                                   # a jittered copy of the previous blob: IoU on either side of 0.7
            cy, cx, ry, rx = cy + g.uniform(-1, 1), cx + g.uniform(-1, 1), ry * g.uniform(0.85, 1.1), rx * g.uniform(0.85, 1.1)
        else:
            cy, cx, ry, rx = g.uniform(0, H), g.uniform(0, W), g.uniform(1.2, H / 2.5), g.uniform(1.2, W / 2.5)
        masks[i] = (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2) <= 1
        if masks[i].sum() == 0:
            masks[i, min(H - 1, int(abs(cy)) % H), min(W - 1, int(abs(cx)) % W)] = 1
    scores = (g.permutation(K).astype(np.float32) + g.uniform(0.1, 0.9, K).astype(np.float32)) / np.float32(K + 1)
    cand = g.uniform(0, 1, K) < 0.7
    cand[0] = True
    return masks, scores.astype(np.float32), cand


def _kept_areas_distinct(masks, scores, cand):
    """Whether greedy NMS at 0.7 keeps masks of distinct areas (a seed filter only: main() asserts it of the reference's own result)."""
    idx = np.nonzero(cand)[0]
    flat = masks[idx].reshape(len(idx), -1).astype(np.int64)
    inter = flat @ flat.T
    area = np.diag(inter)
    keep = []
    for i in np.argsort(-scores[idx]):
        if all(inter[i, k] / (area[i] + area[k] - inter[i, k]) <= 0.7 for k in keep):
            keep.append(i)
    return len(set(area[keep].tolist())) == len(keep) and len(idx) >= min(4, len(masks))


def distinct_blobs(seed, K, H, W):
    """blobs() at the first seed of seed, seed + 100, ... whose kept areas are distinct."""
    while not _kept_areas_distinct(*blobs(seed, K, H, W)):
        seed += 100
    return blobs(seed, K, H, W)


def cases():
    out = {}
    # 63 pixels: a single partial word
    out["tiny"] = distinct_blobs(3, 5, 7, 9)
    # 65 pixels: one full word plus one bit.  A (8 px) and B (9 px) share 7: IoU = 7 / 10 exactly; C = A again (IoU 1) at a lower
    # score; D is disjoint from all and reaches into the last pixel (bit 0 of the second word)
    H, W = 5, 13
    A, B = rect(H, W, 0, 1, 0, 8), rect(H, W, 0, 1, 1, 10)
    C, D = A.copy(), rect(H, W, 3, 5, 10, 13)
    out["pair"] = (np.stack([A, B, C, D]), np.array([0.93, 0.81, 0.78, 0.55], dtype=np.float32), np.ones(4, dtype=bool))
    # nested (small inside large: both kept, the large one paints over the small one), identical, disjoint, heavy overlap
    H, W = 24, 32
    big, small = rect(H, W, 2, 20, 3, 25), rect(H, W, 6, 10, 8, 14)
    twin = big.copy()
    far = rect(H, W, 21, 24, 27, 32)
    heavy = rect(H, W, 2, 20, 4, 26)                     # IoU with big = 378 / 414 > 0.7
    skip = rect(H, W, 0, 24, 0, 32)                      # not a candidate: would suppress nothing and paint nothing
    out["mix"] = (np.stack([small, big, skip, twin, far, heavy]), np.array([0.95, 0.9, 0.99, 0.85, 0.75, 0.8], dtype=np.float32),
                  np.array([True, True, False, True, True, True]))
    out["rand33"] = distinct_blobs(11, 33, 24, 32)
    out["rand65"] = distinct_blobs(12, 65, 24, 32)
    return out


def main():
    nms_ns = R.ref_functions("lib/fcn/nms.py", ["nms"], {"np": np})
    tu = R.ref_functions("lib/fcn/test_utils.py", ["combine_masks_with_NMS"], {"torch": torch, "np": np, "nms": nms_ns["nms"]})
    arrs = {}
    for name, (masks, scores, cand) in cases().items():
        idx = np.nonzero(cand)[0]
        m, s = masks[idx].astype(np.float32), scores[idx]
        assert len(np.unique(s)) == len(s), name
        keep = nms_ns["nms"](m, s, 0.7).astype(int)
        areas = m.reshape(len(m), -1).sum(1)
        assert len(np.unique(areas[keep])) == len(keep), (name, areas[keep])
        label, score, bbox = tu["combine_masks_with_NMS"](_Inst(pred_masks=torch.from_numpy(m), scores=torch.from_numpy(s)))
        arrs.update({f"{name}_masks": masks, f"{name}_scores": scores, f"{name}_cand": cand, f"{name}_label": label.astype(np.int16),
                     f"{name}_score": score.astype(np.int16), f"{name}_bbox": bbox, f"{name}_keep": idx[keep].astype(np.int32)})
        print(f"{name}: K={len(masks)} candidates={len(idx)} kept={len(keep)}")
    pk = arrs["pair_keep"].tolist()
    print("pair: kept", pk, "-> the reference", "KEEPS" if 1 in pk else "SUPPRESSES", "the mask at IoU 7/10")
    path = os.path.join(HERE, "mask_nms.npz")
    np.savez_compressed(path, **arrs)
    print(f"mask_nms: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
