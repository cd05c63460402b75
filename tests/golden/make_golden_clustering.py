"""Generate tests/golden/clustering_two_stage.npz with the REFERENCE's UCN two-stage functions: clustering_features,
filter_labels_depth, crop_rois and match_label_crop of lib/fcn/test_dataset.py and the mean_shift_smart_init of
lib/utils/mean_shift.py, all executed from the reference sources through _ref_import.ref_functions with a stand-in ``cfg`` namespace.

Run in the build container only:   python tests/golden/make_golden_clustering.py [--seeds 6]

The driver, test_sample (lib/fcn/test_dataset.py:232-267), is RESTATED below line by line with its line numbers, for one reason: it
hard-codes num_seeds=100 (TD:248; TD:260 takes the default, also 100), and with 100 seeds the first margin below cannot hold -- once
every planted region holds a seed, the best and the runner-up of the thousands of points of a few noise blobs are closer than 1e-5
(``--seeds 100`` prints the figures and refuses: on the first-stage map 80 of the 99 steps lead by less).  The restatement passes
``num_seeds`` = 6 to both clustering_features calls, which the reference's function takes as an argument; everything else is the
driver's.

The scene (tests/clustering_scene.py, shared with the harness tests): 96 x 128, a table plane and three planted objects, one of them
with a hole in its depth (the 0.8 filter removes it); per-object colours plus noise of 1e-2; xyz from pinhole intrinsics.  The
stand-in ``network`` / ``network_crop`` are normalize(W . image) with two fixed 64 x 3 matrices stored in the fixture (two different
"checkpoints", no stored features).  np.random.seed(3); the first indices the reference draws (MS:155) are recorded.

Stored: image / depth (3,H,W) float32, w_net / w_crop (64,3), num_seeds, first_indices (1 + crops), selected (1 + crops, S) int32,
label / filtered / refined (H,W) uint8, rois (crops,4) int16, labels_crop (crops,224,224) int8 (as match_label_crop returns them:
rejected segments -1), near_tie_label / near_tie_refined (H,W) and near_tie_crop (crops,224,224) bool.

The fixture is written only if three margins hold, computed in float64 (summation-order differences between torch on the host, the
oracle and the HIP kernels are ~1e-7):
  * at every seeding step of every map the point the reference picked leads the runner-up by > 1e-5;
  * every pair of converged seeds is farther than 1e-4 from the merge threshold 2 * 0.02;
  * the pixels whose two nearest merged clusters are within 1e-5 of each other (the near-tie masks) are < 0.1 % of each map."""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _ref_import as R  # noqa: E402
import clustering_scene as cs  # noqa: E402

KAPPA, ALPHA = 20, 0.02
SEED_MARGIN, MERGE_MARGIN, TIE_MARGIN, TIE_FRACTION = 1e-5, 1e-4, 1e-5, 1e-3


def margins(X, selected):
    """The three margins of one clustered map in float64 -> (seeding lead, steps below the margin, merge distance, near-tie mask (n,))."""
    X = X.double()
    S = len(selected)
    nearest = torch.full((X.shape[0],), float("inf"), dtype=torch.float64)
    leads = []
    for i in range(1, S):
        nearest = torch.minimum(nearest, 0.5 * (1 - X @ X[selected[i - 1]]))
        picked = float(nearest[selected[i]])
        others = nearest.clone()
        others[selected[i]] = -float("inf")
        leads.append(picked - float(others.max()))               # negative: float64 would have picked another point
    Z = X[selected]
    for _ in range(10):
        Z = F.normalize(torch.exp(KAPPA * (Z @ X.t())) @ X, dim=1)
    d = 0.5 * (1 - Z @ Z.t())
    merge = float((d - 2 * ALPHA).abs().min())
    # merged clusters: with the merge margin holding, "within epsilon" is read off d; the sequential merge (MS:41-76) gives the
    # components of that relation when it is transitive, which is asserted
    near = d <= 2 * ALPHA
    assert torch.equal((near.double() @ near.double()) > 0, near), "seeds within epsilon do not form disjoint groups"
    comp = torch.full((S,), -1, dtype=torch.long)
    k = 0
    for i in range(S):
        if comp[i] < 0:
            comp[near[i]] = k
            k += 1
    tie = torch.zeros(X.shape[0], dtype=torch.bool)
    if k > 1:
        dist = 0.5 * (1 - X @ Z.t())
        per = torch.stack([dist[:, comp == c].min(1).values for c in range(k)], 1)
        two = torch.topk(per, 2, dim=1, largest=False).values
        tie = (two[:, 1] - two[:, 0]) <= TIE_MARGIN
    return min(leads), sum(v <= SEED_MARGIN for v in leads), merge, tie


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=6)
    num_seeds = ap.parse_args().seeds
    sample, w_net, w_crop, _ = cs.scene()
    network, network_crop = cs.network_from(w_net), cs.network_from(w_crop)
    ns_mask = R.ref_functions("lib/utils/mask.py", ["mask_to_tight_box_numpy", "mask_to_tight_box_pytorch", "mask_to_tight_box"],
                              {"torch": torch, "np": np})
    util = type("U", (), {"mask_to_tight_box": staticmethod(ns_mask["mask_to_tight_box"])})
    cfg = type("C", (), {"device": "cpu", "TRAIN": type("T", (), {"SYN_CROP_SIZE": 224, "EMBEDDING_METRIC": "cosine", "EMBEDDING_ALPHA": ALPHA})})
    ms = R.ref_functions("lib/utils/mean_shift.py", ["ball_kernel", "get_label_mode", "connected_components", "seed_hill_climbing_ball",
                                                     "mean_shift_with_seeds", "select_smart_seeds", "mean_shift_smart_init"],
                         {"torch": torch, "F": F, "np": np, "cfg": cfg})
    td = R.ref_functions("lib/fcn/test_dataset.py", ["clustering_features", "crop_rois", "match_label_crop", "filter_labels_depth"],
                         {"torch": torch, "F": F, "cfg": cfg, "util_": util, "np": np, "mean_shift_smart_init": ms["mean_shift_smart_init"]})
    first = []
    ref_randint = np.random.randint

    def randint(lo, hi):
        first.append(int(ref_randint(lo, hi)))
        return first[-1]

    np.random.randint = randint
    try:
        np.random.seed(3)
        # ---- test_sample (TD:232-267), restated; cfg.INPUT == 'RGBD', no 'label' in the sample, cfg.TEST.VISUALIZE off ----
        image = sample["image_color"]                                                                     # TD:235
        depth = sample["depth"]                                                                           # TD:237
        label = None                                                                                      # TD:244
        features = network(image, label, depth).detach()                                                  # TD:247
        raw_label, selected_pixels = td["clustering_features"](features, num_seeds=num_seeds)             # TD:248 (100 there)
        out_label = td["filter_labels_depth"](raw_label, depth, 0.8)                                      # TD:252
        rgb_crop, out_label_crop, rois, depth_crop = td["crop_rois"](image, out_label.clone(), depth)     # TD:257
        assert rgb_crop.shape[0] > 0                                                                      # TD:258
        features_crop = network_crop(rgb_crop, out_label_crop, depth_crop)                                # TD:259
        labels_crop, selected_pixels_crop = td["clustering_features"](features_crop, num_seeds=num_seeds)  # TD:260 (default 100 there)
        out_label_refined, labels_crop = td["match_label_crop"](out_label, labels_crop, out_label_crop, rois, depth_crop)   # TD:261
    finally:
        np.random.randint = ref_randint
    crops = rois.shape[0]
    selected = list(selected_pixels) + list(selected_pixels_crop)
    assert crops == 2 and len(first) == 1 + crops and [int(s[0]) for s in selected] == first
    assert set(torch.unique(raw_label).tolist()) - set(torch.unique(out_label).tolist()), "the depth filter removed nothing"
    maps = [features[0]] + [features_crop[i] for i in range(crops)]
    ok, ties = True, []
    for m, feat in enumerate(maps):
        X = feat.reshape(feat.shape[0], -1).t().contiguous()
        lead, below, merge, tie = margins(X, selected[m])
        frac = float(tie.float().mean())
        print(f"map {m}: n={X.shape[0]} seeds={num_seeds} smallest seeding lead {lead:.3e} ({below} of {num_seeds - 1} steps <= {SEED_MARGIN:g}) "
              f"merge margin {merge:.3e} near ties {int(tie.sum())} ({frac:.5f})")
        ok = ok and lead > SEED_MARGIN and merge > MERGE_MARGIN and frac < TIE_FRACTION
        ties.append(tie.view(feat.shape[1:]))
    if not ok:
        raise SystemExit("the margins do not hold: the fixture is NOT written")
    # refined pixels that a flagged crop pixel can reach: the flags pasted back as match_label_crop pastes the labels (TD:165-177)
    tie_refined = torch.zeros((cs.H, cs.W), dtype=torch.bool)
    for i in range(crops):
        x0, y0, x1, y1 = [int(v) for v in rois[i]]
        small = F.interpolate(ties[1 + i][None, None].float(), size=(y1 - y0 + 1, x1 - x0 + 1), mode="nearest")[0, 0] != 0
        tie_refined[y0:y1 + 1, x0:x1 + 1] |= small
    arrs = dict(image=image[0].numpy(), depth=depth[0].numpy(), w_net=w_net.numpy(), w_crop=w_crop.numpy(), num_seeds=np.int32(num_seeds),
                first_indices=np.array(first, dtype=np.int32), selected=torch.stack(selected).numpy().astype(np.int32),
                label=raw_label[0].numpy().astype(np.uint8), filtered=out_label[0].numpy().astype(np.uint8),
                refined=out_label_refined[0].numpy().astype(np.uint8), rois=rois.numpy().astype(np.int16),
                labels_crop=labels_crop.numpy().astype(np.int8), near_tie_label=ties[0].numpy(),
                near_tie_crop=torch.stack(ties[1:]).numpy(), near_tie_refined=tie_refined.numpy())
    path = os.path.join(HERE, "clustering_two_stage.npz")
    np.savez_compressed(path, **arrs)
    print(f"clustering_two_stage: {os.path.getsize(path) / 1024:.1f} KiB, first indices {first}, rois {rois.tolist()}, "
          f"labels {torch.unique(raw_label).tolist()} -> {torch.unique(out_label).tolist()}, refined {torch.unique(out_label_refined).tolist()}")


if __name__ == "__main__":
    main()
