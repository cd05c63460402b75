"""Golden fixture of the training targets: run the REFERENCE's TableTopDataset.process_label_to_annos / process_label / sample_pixels
(lib/datasets/tabletop_dataset.py:183-232,303-316, with mask_to_tight_box :101-104 and augmentation.array_to_tensor
lib/utils/augmentation.py:19-32) and PretrainedMeanShiftMaskFormer.prepare_targets
(MSMFormer/meanshiftformer/pretrained_meanshiftformer_model.py:380-395) on small hand-built label images and store the inputs
and what they return.

Run in the build container only:   python tests/golden/make_golden_targets.py   ->  tests/golden/instance_targets.npz

The methods are executed from their source (_ref_import.ref_method) on a stand-in ``self``; the steps between them are
__getitem__'s (:335-337,361-362): the table (id 1) becomes background, then the three methods in the reference's order, on int64
label arrays (sample_pixels needs a signed type for its -1).  What the mapper and the model do with the result and that cannot run
here (pycocotools, detectron2) is restated in two lines each, marked below:
  - gt_masks are the instance masks as bool (BitMasks), gt_classes the records' "category_id": 1 (tabletop_dataset.py:383,
    tablet_instance_mapper.py:144-145,174-175) -- NOT the clip(1, 2) labels process_label_to_annos returns, which __getitem__ drops
    (they are stored as ``annos_labels`` all the same);
  - the padded frame is (H, W) rounded up to the size divisibility and the label map is padded with 0 at the right / bottom
    (ImageList.from_tensors(labels, size_divisibility), pretrained_meanshiftformer_model.py:319-321, pad_value 0).
sample_pixels is random where a label has more than ``num`` pixels; it is recorded only with ``num`` at least every label's
count, where it is deterministic (and returns the dense labels unchanged).
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ref_import as R  # noqa: E402


def rect(a, y0, y1, x0, x1, v):
    a[y0:y1, x0:x1] = v


def make_cases():
    """(name, raw uint8 (H,W), size_divisibility)"""
    cases = []
    a = np.zeros((48, 64), np.uint8)                     # an ordinary scene: background, table, ids 2, 7, 200
    rect(a, 20, 48, 0, 64, 1)
    rect(a, 10, 30, 5, 20, 2)
    rect(a, 15, 40, 30, 41, 7)
    rect(a, 25, 33, 35, 60, 200)                         # overlaps 7: later ids overwrite
    cases.append(("scene", a, 32))
    cases.append(("background_only", np.zeros((20, 24), np.uint8), 32))
    cases.append(("table_only", np.ones((20, 24), np.uint8), 32))
    a = np.full((16, 20), 5, np.uint8)                   # no background pixel at all: id 2 gets dense label 0 and a mask
    rect(a, 0, 16, 0, 9, 2)
    rect(a, 4, 8, 12, 17, 9)
    cases.append(("no_background", a, 32))
    a = np.zeros((12, 18), np.uint8)
    a[7, 11] = 4                                         # a one-pixel instance
    rect(a, 1, 5, 2, 9, 3)
    cases.append(("one_pixel", a, 8))
    a = np.zeros((14, 22), np.uint8)                     # a ring along all four borders, another instance inside
    a[0, :] = a[-1, :] = 6
    a[:, 0] = a[:, -1] = 6
    rect(a, 5, 9, 8, 15, 255)
    cases.append(("borders", a, 16))
    rng = np.random.default_rng(5)
    a = np.zeros((37, 53), np.uint8)                     # odd size, padded to 64 x 64; speckled ids
    rect(a, 18, 37, 0, 53, 1)
    rect(a, 3, 21, 4, 19, 12)
    rect(a, 9, 30, 25, 50, 13)
    sp = rng.random((37, 53)) < 0.05
    a[sp] = rng.integers(2, 6, size=int(sp.sum()), dtype=np.uint8)
    cases.append(("odd_37x53", a, 32))
    cases.append(("d1_37x53", a.copy(), 1))
    return cases


def namespace():
    ns = {"np": np, "torch": torch}
    R.ref_functions("lib/datasets/tabletop_dataset.py", ["mask_to_tight_box"], ns)
    aug = R.ref_functions("lib/utils/augmentation.py", ["array_to_tensor"], {"np": np, "torch": torch})
    ns["augmentation"] = types.SimpleNamespace(array_to_tensor=aug["array_to_tensor"])
    R.ref_method("lib/datasets/tabletop_dataset.py", "TableTopDataset", ["process_label_to_annos", "process_label", "sample_pixels"], ns)
    R.ref_method("MSMFormer/meanshiftformer/pretrained_meanshiftformer_model.py", "PretrainedMeanShiftMaskFormer", ["prepare_targets"], ns)
    return ns


def main():
    ns = namespace()
    me = types.SimpleNamespace()
    cases = make_cases()
    out = {"names": np.array([c[0] for c in cases])}
    for name, raw, d in cases:
        H, W = raw.shape
        foreground_labels = raw.astype(np.int64)
        foreground_labels[foreground_labels == 1] = 0                                   # tabletop_dataset.py:335
        boxes, binary_masks, annos_labels = ns["process_label_to_annos"](me, foreground_labels)
        dense = ns["process_label"](me, foreground_labels)
        counts = np.bincount(dense.reshape(-1))
        num = int(counts.max())
        sampled = ns["sample_pixels"](me, dense, num)
        # restated: the mapper's instances (bool masks, "category_id": 1) and the padded frame of ImageList.from_tensors
        T = binary_masks.shape[0]
        Hp, Wp = (-(-H // d) * d, -(-W // d) * d) if d > 1 else (H, W)
        inst = types.SimpleNamespace(gt_masks=binary_masks.bool(), gt_classes=torch.ones(T, dtype=torch.int64))
        images = types.SimpleNamespace(tensor=torch.zeros(1, 3, Hp, Wp))
        target = ns["prepare_targets"](me, [inst], images)[0]
        label_padded = F.pad(torch.from_numpy(sampled), (0, Wp - W, 0, Hp - H), value=0)
        assert target["masks"].dtype == torch.bool and tuple(target["masks"].shape) == (T, Hp, Wp)
        out[f"{name}_raw"] = raw
        out[f"{name}_d"] = np.int64(d)
        out[f"{name}_boxes"] = boxes.numpy()                                            # float32 (array_to_tensor)
        out[f"{name}_masks"] = binary_masks.numpy().astype(np.uint8)                    # (T,H,W) 0 / 1
        out[f"{name}_annos_labels"] = annos_labels.numpy()
        out[f"{name}_dense"] = dense
        out[f"{name}_sample_num"] = np.int64(num)
        out[f"{name}_sampled"] = sampled
        out[f"{name}_target_labels"] = target["labels"].numpy()
        out[f"{name}_target_masks"] = target["masks"].numpy()                           # (T,Hp,Wp) bool
        out[f"{name}_label_padded"] = label_padded.numpy()
        print(name, (H, W), "->", (Hp, Wp), "T =", T, "K =", int(dense.max()) + 1, "boxes", boxes.numpy().tolist(), flush=True)
    path = os.path.join(HERE, "instance_targets.npz")
    np.savez_compressed(path, **out)
    print(f"instance_targets: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
