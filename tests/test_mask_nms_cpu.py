"""Mask NMS for a batch of images, host side (two_stage.combine_masks_with_NMS_batched on host tensors = the definition the HIP
kernels are held to in test_gpu_mask_nms.py): against tests/golden/mask_nms.npz -- the reference's own nms / combine_masks_with_NMS
(lib/fcn/nms.py:3-23, lib/fcn/test_utils.py:55-91) executed by tests/golden/make_golden_nms.py --, against today's per-image
combine_masks_with_NMS, and on what the reference leaves open or cannot do (ties, empty candidates, NaN scores, no candidates).
CPU only."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from nms_cases import PlantedModel, PlantedPredictor, planted_case, planted_samples  # noqa: E402
from unseenobjectswithmeanshift_amd import _lib  # noqa: E402
from unseenobjectswithmeanshift_amd import two_stage as ts  # noqa: E402
from unseenobjectswithmeanshift_amd.meta_arch import Instances  # noqa: E402

CASES = ("tiny", "pair", "mix", "rand33", "rand65")


def fixture_case(g, name):
    return (torch.from_numpy(g[f"{name}_masks"].astype(np.float32))[None], torch.from_numpy(g[f"{name}_scores"])[None],
            torch.from_numpy(g[f"{name}_cand"])[None])


def check_against_fixture(g, name, label, score, bbox, count):
    """One image's results (tensors, any device) against the reference's: every value bit for bit."""
    n = len(g[f"{name}_keep"])
    assert int(count) == n
    assert label.dtype == torch.float32 and score.dtype == torch.float32 and bbox.dtype == torch.float32
    assert np.array_equal(label.cpu().numpy(), g[f"{name}_label"].astype(np.float32)), name
    assert np.array_equal(score.cpu().numpy(), g[f"{name}_score"].astype(np.float32)), name
    assert np.array_equal(bbox.cpu().numpy()[:n], g[f"{name}_bbox"]), name
    assert not bbox.cpu().numpy()[n:].any(), name
    # the kept instances in label order: row r of bbox carries the score of instance keep[r] (scores are distinct in the fixture)
    assert np.array_equal(bbox.cpu().numpy()[:n, 4], g[f"{name}_scores"][g[f"{name}_keep"]]), name


@pytest.mark.parametrize("name", CASES)
def test_host_definition_equals_the_reference(golden, name):
    g = golden("mask_nms")
    label, score, bbox, count = ts.combine_masks_with_NMS_batched(*fixture_case(g, name))
    assert count.dtype == torch.int32 and label.shape[0] == 1
    check_against_fixture(g, name, label[0], score[0], bbox[0], count[0])


def test_the_reference_keeps_a_pair_at_iou_seven_tenths(golden):
    """A (8 px) and B (9 px) share 7 pixels: float32(7) / float32(10) <= float32(0.7).  The REFERENCE decided (the fixture); the
    definition's <= on one fp32 division follows it."""
    g = golden("mask_nms")
    assert 1 in g["pair_keep"].tolist() and 0 in g["pair_keep"].tolist() and 2 not in g["pair_keep"].tolist()
    _, _, _, count = ts.combine_masks_with_NMS_batched(*fixture_case(g, "pair"))
    assert int(count[0]) == 3
    # just under the threshold the same pair is suppressed
    _, _, _, count = ts.combine_masks_with_NMS_batched(*fixture_case(g, "pair"), thresh=float(np.nextafter(np.float32(0.7), np.float32(0))))
    assert int(count[0]) == 2


@pytest.mark.parametrize("name", CASES)
def test_batched_equals_todays_per_image_function(golden, name):
    g = golden("mask_nms")
    masks, scores, cand = fixture_case(g, name)
    inst = Instances(tuple(masks.shape[-2:]), pred_masks=masks[0][cand[0]], scores=scores[0][cand[0]])
    bin_mask, score_mask, bbox = ts.combine_masks_with_NMS(inst)
    label, score, box, count = ts.combine_masks_with_NMS_batched(masks, scores, cand)
    assert np.array_equal(label[0].numpy().astype(np.float64), bin_mask)
    assert np.array_equal(score[0].numpy().astype(np.float64), score_mask)
    assert np.array_equal(box[0, :int(count[0])].numpy(), bbox)


def test_a_batch_is_its_images_one_by_one(golden):
    g = golden("mask_nms")
    names = ("mix", "rand33")                       # 24 x 32 both; pad K to 33 with non-candidates
    K = 33
    masks, scores, cand = torch.zeros(2, K, 24, 32), torch.zeros(2, K), torch.zeros(2, K, dtype=torch.bool)
    for b, name in enumerate(names):
        m, s, c = fixture_case(g, name)
        masks[b, :m.shape[1]], scores[b, :m.shape[1]], cand[b, :m.shape[1]] = m[0], s[0], c[0]
    label, score, bbox, count = ts.combine_masks_with_NMS_batched(masks, scores, cand)
    for b, name in enumerate(names):
        check_against_fixture(g, name, label[b], score[b], bbox[b], count[b])


def test_tie_rules():
    H, W = 6, 10
    masks = torch.zeros(1, 4, H, W)
    masks[0, 0, 0:3, 0:5] = 1                        # 0 and 1 overlap at IoU 12/15 > 0.7 with EQUAL scores: the higher index is
    masks[0, 1, 0:3, 1:5] = 1                        # visited first, so 1 is kept and suppresses 0
    masks[0, 2, 4:6, 0:3] = 1                        # 2 and 3: disjoint, EQUAL areas (6): numbered in the order they were kept,
    masks[0, 3, 4:6, 5:8] = 1                        # i.e. by score -- 3 (0.8) before 2 (0.6)
    scores = torch.tensor([[0.9, 0.9, 0.6, 0.8]])
    label, score, bbox, count = ts.combine_masks_with_NMS_batched(masks, scores, torch.ones(1, 4, dtype=torch.bool))
    assert int(count[0]) == 3
    assert bbox[0, :3].tolist() == [[5, 4, 7, 5, pytest.approx(0.8)], [0, 4, 2, 5, pytest.approx(0.6)], [1, 0, 4, 2, pytest.approx(0.9)]]
    assert label[0, 0, 0] == 0 and label[0, 0, 1] == 4 and label[0, 4, 5] == 2 and label[0, 4, 0] == 3
    assert score[0, 0, 1] == 90 and score[0, 4, 5] == 80 and score[0, 4, 0] == 60 and score[0, 0, 0] == 0
    # equal scores AND equal areas on disjoint masks: the higher index is kept first, so it takes the smaller label
    scores = torch.tensor([[0.1, 0.9, 0.7, 0.7]])
    label, _, bbox, count = ts.combine_masks_with_NMS_batched(masks, scores, torch.tensor([[False, False, True, True]]))
    assert int(count[0]) == 2 and label[0, 4, 5] == 2 and label[0, 4, 0] == 3 and label[0, 0, 1] == 0


def test_empty_and_nan_candidates_are_dropped_and_none_gives_zeros():
    H, W = 5, 13
    masks = torch.zeros(2, 3, H, W)
    masks[:, 0, 1:3, 2:6] = 1
    masks[:, 2] = 1                                  # the whole frame, NaN score
    scores = torch.tensor([[0.5, 0.99, float("nan")]] * 2)
    cand = torch.tensor([[True, True, True], [False, False, False]])
    label, score, bbox, count = ts.combine_masks_with_NMS_batched(masks, scores, cand)
    assert count.tolist() == [1, 0]
    assert bbox[0, 0].tolist() == [2, 1, 5, 2, 0.5] and not bbox[0, 1:].any() and not bbox[1].any()
    assert int((label[0] == 2).sum()) == 8 and int((label[0] != 0).sum()) == 8 and int((score[0] == 50).sum()) == 8
    assert not label[1].any() and not score[1].any()
    # no instance at all
    label, score, bbox, count = ts.combine_masks_with_NMS_batched(torch.zeros(2, 0, H, W), torch.zeros(2, 0), torch.zeros(2, 0, dtype=torch.bool))
    assert label.shape == (2, H, W) and score.shape == (2, H, W) and bbox.shape == (2, 0, 5) and count.tolist() == [0, 0]
    assert not label.any() and not score.any()


def test_planted_case_holds_what_it_says():
    """The generator of the GPU cases (checked here, where no GPU is needed): image 0 keeps one of the identical pair, both of the
    7/10 pair, neither the empty candidate nor the NaN one, and a NaN plane that is no candidate changes nothing."""
    masks, scores, cand = planted_case(5, 3, 33, 24, 32)
    label, score, bbox, count = ts.combine_masks_with_NMS_batched(masks, scores, cand)
    kept = set(bbox[0, :int(count[0]), 4].tolist())
    f32 = lambda v: float(np.float32(v))            # noqa: E731
    assert f32(0.91) in kept and f32(0.9) not in kept and f32(0.99) not in kept
    assert f32(0.95) in kept and f32(0.94) in kept and not any(np.isnan(v) for v in kept)
    assert torch.isnan(masks[0, 8]).all() and not torch.isnan(label).any()
    clean = masks.clone()
    clean[0, 8] = 0
    again = ts.combine_masks_with_NMS_batched(clean, scores, cand)
    assert all(torch.equal(a, b) for a, b in zip(again, (label, score, bbox, count)))
    assert len(set(count.tolist())) > 1 and cand[0].sum() != cand[1].sum()


def test_candidate_flags_are_the_instance_labels_selection():
    g = torch.Generator().manual_seed(3)
    scores, classes = torch.rand(4, 20, generator=g), (torch.rand(4, 20, generator=g) < 0.7).long()
    for kw in (dict(topk=False, confident_score=0.6, low_threshold=0.4, num_class=2), dict(topk=True, confident_score=0.6, low_threshold=0.4, num_class=2),
               dict(topk=True, confident_score=0.6, low_threshold=0.4, num_class=1)):
        flag = ts.candidate_flags(scores, classes, **kw)
        assert flag.dtype == torch.bool and torch.equal(flag, ts.instance_labels(scores, classes, **kw) > 0)


def test_batched_pipeline_with_nms_equals_the_frame_by_frame_pipeline():
    """test_batch_crop_nolabel(use_nms=True) on host tensors against test_sample_crop_nolabel(use_nms=True) per frame -- the
    reference's loop (lib/fcn/test_utils.py:375-406) with its NMS in both stages -- with planted overlapping masks: label images,
    refined label images, score maps and boxes."""
    H, W, Fr = 64, 96, 2
    pred = PlantedPredictor(PlantedModel())
    samples = planted_samples(Fr, H, W, "cpu")
    kw = dict(use_depth=True, topk=False, confident_score=0.6, use_nms=True)
    extras = {}
    labels, refined, rows = ts.test_batch_crop_nolabel(samples, pred, pred, extras=extras, **kw)
    assert len(rows) > Fr and set(extras) == {"out_score", "bbox", "count"}
    assert extras["out_score"].shape == (Fr, H, W) and extras["bbox"].shape == (Fr, 8, 5) and extras["count"].shape == (Fr,)
    plain = ts.test_batch_crop_nolabel(samples, pred, pred, **dict(kw, use_nms=False))
    assert not torch.equal(plain[0], labels)                     # the planted overlaps make NMS matter
    for f, smp in enumerate(samples):
        o_label, o_refined, o_score, o_bbox = ts.test_sample_crop_nolabel(smp, pred, pred, **kw)
        n = int(extras["count"][f])
        assert 0 < n < 8
        assert torch.equal(labels[f].double(), o_label[0].double()), f
        assert torch.equal(refined[f].double(), o_refined[0].double()), f
        assert torch.equal(extras["out_score"][f].double(), o_score[0].double()), f
        assert np.array_equal(extras["bbox"][f, :n].numpy(), o_bbox) and not extras["bbox"][f, n:].any()


def test_abi_symbols_are_declared_and_exported():
    assert {"msm_mask_nms", "msm_mask_nms_workspace"} <= set(_lib.declared_symbols()) and _lib.ABI_VERSION >= 27
    L = _lib.lib()
    assert hasattr(L, "msm_mask_nms") and hasattr(L, "msm_mask_nms_workspace")
    nw = (480 * 640 + 63) // 64
    assert L.msm_mask_nms_workspace(16, 100, 480, 640) >= 16 * 100 * (nw * 8 + 100 * 4)
    for bad in ((1, 257, 8, 8), (1, 0, 8, 8), (0, 4, 8, 8), (1, 4, 0, 8), (1, 4, 8, -1)):
        assert L.msm_mask_nms_workspace(*bad) < 0
    assert b"K" in L.msm_last_error_string()
