"""Golden fixture of the set criterion: run the REFERENCE's SetCriterion and HungarianMatcher
(MSMFormer/meanshiftformer/modeling/criterion.py, matcher.py) on the CPU and store what they produce.

Run in the build container only:   python tests/golden/make_golden_criterion.py   ->  tests/golden/set_criterion.npz

The two reference modules are imported through _ref_import with stand-ins for what they import and is absent here:
  detectron2.projects.point_rend.point_features
            point_sample and get_uncertain_point_coords_with_randomness, written from detectron2's documented definitions
            (grid_sample of 2c - 1, bilinear, zeros, align_corners=False; oversampled points, topk of the uncertainty, then
            uniform points).  The stand-in also records the topk selection of every call.
  detectron2.utils.comm.get_world_size -> 1
  <reference>/utils/misc
            nested_tensor_from_tensor_list (zero padding to the largest shape) and is_dist_avail_and_initialized (False);
            the real module needs torchvision.
Inputs are synthetic.synth_criterion_inputs(seed=SEED) (not stored).  Stored: every loss, the assignments, every random draw
(shape, sum, first 16 values), the selection bitmaps (np.packbits, little bit order, per matched mask) of the predictions in
DETAIL_PREDS, the gradients of the weighted total loss w.r.t. every pred_logits, and w.r.t. the matched masks of the final
prediction's pred_masks (all predictions' would not fit the 1 MiB limit of a committed file).
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _ref_import as R  # noqa: E402
from unseenobjectswithmeanshift_amd import synthetic as syn  # noqa: E402

SEED = 7
NUM_POINTS, OVERSAMPLE, IMPORTANCE = 12544, 3.0, 0.75
CLASS_W, MASK_W, DICE_W, NO_OBJECT_W = 2.0, 5.0, 5.0, 0.1
DEC_LAYERS = 10
DETAIL_PREDS = (0, 9)          # criterion order: 0 = final prediction, 1 + i = aux_outputs[i]

SELECTIONS = []                # (N, Pos) bool per get_uncertain_point_coords_with_randomness call
DRAWS = []                     # (shape, sum, first 16) per torch.rand call


def point_sample(input, point_coords, **kwargs):
    add_dim = False
    if point_coords.dim() == 3:
        add_dim = True
        point_coords = point_coords.unsqueeze(2)
    output = F.grid_sample(input, 2.0 * point_coords - 1.0, **kwargs)
    if add_dim:
        output = output.squeeze(3)
    return output


def get_uncertain_point_coords_with_randomness(coarse_logits, uncertainty_func, num_points, oversample_ratio,
                                               importance_sample_ratio):
    assert oversample_ratio >= 1
    assert 0 <= importance_sample_ratio <= 1
    num_boxes = coarse_logits.shape[0]
    num_sampled = int(num_points * oversample_ratio)
    point_coords = torch.rand(num_boxes, num_sampled, 2, device=coarse_logits.device)
    point_logits = point_sample(coarse_logits, point_coords, align_corners=False)
    point_uncertainties = uncertainty_func(point_logits)
    num_uncertain_points = int(importance_sample_ratio * num_points)
    num_random_points = num_points - num_uncertain_points
    idx = torch.topk(point_uncertainties[:, 0, :], k=num_uncertain_points, dim=1)[1]
    sel = torch.zeros(num_boxes, num_sampled, dtype=torch.bool)
    sel.scatter_(1, idx, True)
    SELECTIONS.append(sel.numpy())
    shift = num_sampled * torch.arange(num_boxes, dtype=torch.long, device=coarse_logits.device)
    idx += shift[:, None]
    point_coords = point_coords.view(-1, 2)[idx.view(-1), :].view(num_boxes, num_uncertain_points, 2)
    if num_random_points > 0:
        point_coords = torch.cat([point_coords, torch.rand(num_boxes, num_random_points, 2, device=coarse_logits.device)], dim=1)
    return point_coords


class _NestedTensor:
    def __init__(self, tensors, mask):
        self.tensors, self.mask = tensors, mask

    def decompose(self):
        return self.tensors, self.mask


def nested_tensor_from_tensor_list(tensor_list):
    assert tensor_list[0].ndim == 3
    max_size = [max(s) for s in zip(*[list(t.shape) for t in tensor_list])]
    b, c, h, w = [len(tensor_list)] + max_size
    tensor = torch.zeros((b, c, h, w), dtype=tensor_list[0].dtype)
    mask = torch.ones((b, h, w), dtype=torch.bool)
    for img, pad_img, m in zip(tensor_list, tensor, mask):
        pad_img[: img.shape[0], : img.shape[1], : img.shape[2]].copy_(img)
        m[: img.shape[1], : img.shape[2]] = False
    return _NestedTensor(tensor, mask)


def install():
    R.install_stubs()
    R._mod("detectron2.projects")
    R._mod("detectron2.projects.point_rend")
    R._mod("detectron2.projects.point_rend.point_features", point_sample=point_sample,
           get_uncertain_point_coords_with_randomness=get_uncertain_point_coords_with_randomness)
    R._mod("detectron2.utils.comm", get_world_size=lambda: 1)
    u = R._mod("refmsm.utils")
    u.__path__ = []
    R._mod("refmsm.utils.misc", nested_tensor_from_tensor_list=nested_tensor_from_tensor_list,
           is_dist_avail_and_initialized=lambda: False)


def main():
    install()
    crit_mod = R.ref("modeling.criterion")
    match_mod = R.ref("modeling.matcher")
    outputs, targets = syn.synth_criterion_inputs(seed=SEED)
    preds = [outputs] + outputs["aux_outputs"]               # criterion order
    leaves = []
    for p in preds:
        p["pred_logits"].requires_grad_(True)
        p["pred_masks"].requires_grad_(True)
        leaves.append(p)
    matcher = match_mod.HungarianMatcher(cost_class=CLASS_W, cost_mask=MASK_W, cost_dice=DICE_W, num_points=NUM_POINTS)
    weight_dict = {"loss_ce": CLASS_W, "loss_mask": MASK_W, "loss_dice": DICE_W}
    aux = {}
    for i in range(DEC_LAYERS - 1):
        aux.update({k + f"_{i}": v for k, v in weight_dict.items()})
    weight_dict.update(aux)
    crit = crit_mod.SetCriterion(2, matcher=matcher, weight_dict=weight_dict, eos_coef=NO_OBJECT_W, losses=["labels", "masks"],
                                 num_points=NUM_POINTS, oversample_ratio=OVERSAMPLE, importance_sample_ratio=IMPORTANCE)
    # record the matcher's assignments and every draw
    indices_all = []
    lsa = match_mod.linear_sum_assignment

    def lsa_rec(c):
        r = lsa(c)
        indices_all.append((np.asarray(r[0], np.int64), np.asarray(r[1], np.int64)))
        return r
    match_mod.linear_sum_assignment = lsa_rec
    rand = torch.rand

    def rand_rec(*a, **k):
        x = rand(*a, **k)
        DRAWS.append((list(x.shape), float(x.double().sum()), x.reshape(-1)[:16].numpy().copy()))
        return x
    torch.rand = rand_rec
    torch.manual_seed(SEED)
    try:
        losses = crit(outputs, targets)
    finally:
        torch.rand = rand
        match_mod.linear_sum_assignment = lsa
    total = sum(losses[k] * weight_dict[k] for k in losses if k in weight_dict)
    total.backward()

    n_pred, B = len(preds), len(targets)
    keys = list(losses.keys())
    out = {"seed": np.int64(SEED), "loss_keys": np.array(keys), "loss_values": np.array([float(losses[k]) for k in keys]),
           "total": np.float64(float(total)), "detail_preds": np.array(DETAIL_PREDS, np.int64)}
    # assignments: per prediction the concatenation over images of (b, i, j)
    rows = []
    for p in range(n_pred):
        per = indices_all[p * B:(p + 1) * B]
        rows.append(np.concatenate([np.stack([np.full(len(i), b), i, j], 1) for b, (i, j) in enumerate(per)]).astype(np.int64))
    out["assign"] = np.stack(rows)                                                          # (n_pred, N, 3)
    out["draw_shapes"] = np.array([d[0] for d in DRAWS], np.int64)
    out["draw_sums"] = np.array([d[1] for d in DRAWS])
    out["draw_first16"] = np.stack([np.pad(d[2], (0, 16 - len(d[2]))) for d in DRAWS]).astype(np.float32)
    assert len(SELECTIONS) == n_pred
    out["sel_bits"] = np.stack([np.packbits(SELECTIONS[p], axis=1, bitorder="little") for p in DETAIL_PREDS])
    out["grad_logits"] = np.stack([p["pred_logits"].grad.numpy() for p in preds]).astype(np.float32)
    a = out["assign"][0]
    out["grad_masks_final"] = preds[0]["pred_masks"].grad[a[:, 0], a[:, 1]].numpy().astype(np.float32)
    path = os.path.join(HERE, "set_criterion.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB): total {float(total):.6f}, {len(DRAWS)} draws, "
          f"N = {a.shape[0]}")


if __name__ == "__main__":
    main()
