"""Training targets, host side (no GPU): the numpy definitions of unseenobjectswithmeanshift_amd.targets against what the
reference's process_label_to_annos / process_label / sample_pixels / prepare_targets returned (tests/golden/instance_targets.npz,
written by tests/golden/make_golden_targets.py), sample_pixels against hand-computed selections, the argument checks of the
criterion for a TargetBatch and the header's declarations.  Every comparison is for equality."""
import numpy as np
import pytest
import torch

from unseenobjectswithmeanshift_amd import _lib
from unseenobjectswithmeanshift_amd import criterion as cr
from unseenobjectswithmeanshift_amd import targets as tg

CASES = ["scene", "background_only", "table_only", "no_background", "one_pixel", "borders", "odd_37x53", "d1_37x53"]


def test_fixture_holds_the_cases(golden):
    g = golden("instance_targets")
    assert [str(n) for n in g["names"]] == CASES
    assert sorted(np.unique(g["scene_raw"]).tolist()) == [0, 1, 2, 7, 200]
    assert 0 not in g["no_background_raw"] and 1 not in g["no_background_raw"]
    assert g["odd_37x53_raw"].shape == (37, 53) and int(g["odd_37x53_d"]) == 32 and int(g["d1_37x53_d"]) == 1
    assert int(g["one_pixel_masks"].sum(axis=(1, 2)).min()) == 1
    assert g["borders_boxes"][0].tolist() == [0.0, 0.0, 21.0, 13.0]


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("kind", ["numpy_u8", "tensor_i32", "tensor_i64"])
def test_host_path_equals_the_reference(golden, name, kind):
    g = golden("instance_targets")
    raw, d = g[f"{name}_raw"], int(g[f"{name}_d"])
    given = {"numpy_u8": raw, "tensor_i32": torch.from_numpy(raw.astype(np.int32)), "tensor_i64": torch.from_numpy(raw.astype(np.int64))}[kind]
    tb = tg.instance_targets(given, size_divisibility=d, label_dtype=torch.int32)
    want_masks = g[f"{name}_target_masks"]
    T, Hp, Wp = want_masks.shape
    assert tb.counts == [T] and tb.toff == [0, T] and len(tb) == 1
    assert tb.masks.dtype == torch.uint8 and tuple(tb.masks.shape) == (T, Hp, Wp)
    np.testing.assert_array_equal(tb.masks.numpy(), want_masks.astype(np.uint8))
    assert tb.boxes.dtype == torch.float32 and g[f"{name}_boxes"].dtype == np.float32
    np.testing.assert_array_equal(tb.boxes.numpy(), g[f"{name}_boxes"].reshape(T, 4))
    assert tb.labels.dtype == torch.int64
    np.testing.assert_array_equal(tb.labels.numpy(), g[f"{name}_target_labels"])
    assert tuple(tb.label.shape) == (1, 1, Hp, Wp) and tb.label.dtype == torch.int32
    np.testing.assert_array_equal(tb.label[0, 0].numpy(), g[f"{name}_label_padded"])
    np.testing.assert_array_equal(tb.areas.numpy(), g[f"{name}_masks"].sum(axis=(1, 2)))
    folded = np.where(raw == 1, 0, raw)
    np.testing.assert_array_equal(tb.ids.numpy(), [v for v in np.unique(folded) if v != 0 or 0 not in folded][-T:] if T else [])
    # .targets: the reference's list, bool views of the one buffer
    (t0,) = tb.targets
    assert t0["masks"].dtype == torch.bool and t0["masks"].data_ptr() == tb.masks.data_ptr()
    np.testing.assert_array_equal(t0["masks"].numpy(), want_masks)
    assert tb.check() is tb
    # float32 label map: the same values
    tf = tg.instance_targets(given, size_divisibility=d)
    assert tf.label.dtype == torch.float32
    np.testing.assert_array_equal(tf.label[0, 0].numpy(), g[f"{name}_label_padded"].astype(np.float32))


@pytest.mark.parametrize("name", CASES)
def test_the_three_methods_by_name(golden, name):
    g = golden("instance_targets")
    folded = g[f"{name}_raw"].astype(np.int64)
    folded[folded == 1] = 0
    boxes, masks, classes = tg.process_label_to_annos(folded)
    np.testing.assert_array_equal(boxes.numpy(), g[f"{name}_boxes"].reshape(-1, 4))
    assert masks.dtype == torch.float32
    np.testing.assert_array_equal(masks.numpy(), g[f"{name}_masks"].astype(np.float32))
    np.testing.assert_array_equal(classes.numpy(), g[f"{name}_target_labels"])
    dense = tg.process_label(folded)
    assert isinstance(dense, np.ndarray) and dense.dtype == folded.dtype
    np.testing.assert_array_equal(dense, g[f"{name}_dense"])
    np.testing.assert_array_equal(tg.process_label(torch.from_numpy(folded)[None])[0].numpy(), g[f"{name}_dense"])
    num = int(g[f"{name}_sample_num"])                       # at least every label's count: the reference is deterministic there
    keys = np.random.default_rng(1).integers(0, 2 ** 31 - 1, size=dense.shape).astype(np.int32)
    np.testing.assert_array_equal(tg.sample_pixels(dense, num, keys=keys), g[f"{name}_sampled"])
    np.testing.assert_array_equal(tg.sample_pixels(dense, num + 5, keys=keys), g[f"{name}_sampled"])


def test_no_background_quirk(golden):
    """Without any background pixel the lowest id gets dense label 0 and still has a mask (as in the reference)."""
    g = golden("instance_targets")
    tb = tg.instance_targets(g["no_background_raw"], label_dtype=torch.int32)
    assert tb.ids.tolist() == [2, 5, 9] and tb.counts == [3]
    lab = tb.label[0, 0].numpy()
    np.testing.assert_array_equal(lab == 0, g["no_background_raw"] == 2)
    np.testing.assert_array_equal(tb.masks[0].numpy().astype(bool), g["no_background_raw"] == 2)


def test_batch_counts_and_status():
    raw = np.zeros((3, 6, 8), np.int32)
    raw[0, 1:3, 1:4] = 5
    raw[0, 4, 6] = 9
    raw[2, :, :] = 3
    tb = tg.instance_targets(raw, size_divisibility=4)
    assert tb.counts == [2, 0, 1] and tb.toff == [0, 2, 2, 3] and tuple(tb.masks.shape) == (3, 8, 8)
    assert [tuple(t["masks"].shape) for t in tb.targets] == [(2, 8, 8), (0, 8, 8), (1, 8, 8)]
    assert tb.boxes.tolist() == [[1, 1, 3, 2], [6, 4, 6, 4], [0, 0, 7, 5]] and tb.areas.tolist() == [6, 1, 48]
    # counts= from the loader: right ones change nothing, wrong ones stay inside the buffer and are reported by check()
    same = tg.instance_targets(raw, size_divisibility=4, counts=[2, 0, 1])
    assert torch.equal(same.masks, tb.masks) and torch.equal(same.label, tb.label)
    same.check()
    wrong = tg.instance_targets(raw, size_divisibility=4, counts=[1, 1, 1])
    assert tuple(wrong.masks.shape) == (3, 8, 8) and int(wrong.masks[1].sum()) == 0 and torch.equal(wrong.masks[0], tb.masks[0])
    with pytest.raises(ValueError, match=r"counts\[0\] = 1, but image 0 holds 2"):
        wrong.check()
    with pytest.raises(ValueError, match="counts"):
        tg.instance_targets(raw, counts=[1, 2])
    # ids outside [0, 1024)
    raw[1, 0, 0] = 1023
    assert tg.instance_targets(raw).check().ids.tolist() == [5, 9, 1023, 3]
    raw[1, 0, 1] = 1024
    bad = tg.instance_targets(raw)
    with pytest.raises(ValueError, match=r"image 1 has 1 pixels with ids outside \[0, 1024\)"):
        bad.check()
    with pytest.raises(TypeError, match="integers"):
        tg.instance_targets(raw.astype(np.float32))


# ---- sample_pixels: hand-computed selections --------------------------------------------------------------------------------
def test_sample_pixels_hand_cases():
    dense = np.array([[0, 0, 1, 1, 1],
                      [0, 2, 1, 1, 0]], dtype=np.int64)          # label 0: 4 pixels (flat 0, 1, 5, 9); 1: 5 (2, 3, 4, 7, 8); 2: 1 (6)
    keys = np.array([[50, 10, 7, 7, 9],
                     [10, 99, 3, 8, 60]], dtype=np.int32)
    # n < num and n == num: everything stays
    np.testing.assert_array_equal(tg.sample_pixels(dense, 6, keys=keys), dense)
    np.testing.assert_array_equal(tg.sample_pixels(dense, 5, keys=keys), dense)
    # n == num + 1 for label 1 (num = 4): its largest (key, index) = (9, flat 4) goes
    want = dense.copy()
    want[0, 4] = -1
    np.testing.assert_array_equal(tg.sample_pixels(dense, 4, keys=keys), want)
    # num = 3: label 0 keeps (10, 1), (10, 5), (50, 0) and loses (60, 9); label 1 keeps (3, 7), (7, 2), (7, 3)
    want = np.array([[0, 0, 1, 1, -1],
                     [0, 2, 1, -1, -1]], dtype=np.int64)
    np.testing.assert_array_equal(tg.sample_pixels(dense, 3, keys=keys), want)
    # num = 1: the smallest key per label, the tie (10, 1) / (10, 5) to the lower index
    want = np.array([[-1, 0, -1, -1, -1],
                     [-1, 2, 1, -1, -1]], dtype=np.int64)
    np.testing.assert_array_equal(tg.sample_pixels(dense, 1, keys=keys), want)
    # all keys equal: the lowest indices win
    want = np.array([[0, 0, 1, 1, -1],
                     [-1, 2, -1, -1, -1]], dtype=np.int64)
    np.testing.assert_array_equal(tg.sample_pixels(dense, 2, keys=np.full_like(keys, 77)), want)
    # negative keys order as signed numbers
    k2 = keys.copy()
    k2[1, 4] = -5
    assert tg.sample_pixels(dense, 1, keys=k2)[1, 4] == 0
    # tensors in, tensors out; a batch is sampled per image; -1 stays -1
    out = tg.sample_pixels(torch.from_numpy(np.stack([dense, want])), 1, keys=torch.from_numpy(np.stack([keys, keys])))
    assert isinstance(out, torch.Tensor) and out[1, 0, 0] == -1 and out[1, 0, 1] == 0 and out[1, 0, 2] == 1 and out[1, 0, 3] == -1
    with pytest.raises(ValueError, match="num"):
        tg.sample_pixels(dense, 0, keys=keys)
    with pytest.raises(TypeError, match="signed"):
        tg.sample_pixels(dense.astype(np.uint8), 2, keys=keys)


@pytest.mark.parametrize("num", [1, 7, 40, 2000])
def test_sample_pixels_properties(golden, num):
    """Per label the count kept is min(n, num), kept pixels are unchanged, the rest are -1; a pure function of its inputs."""
    g = golden("instance_targets")
    dense = np.stack([g["odd_37x53_dense"], np.roll(g["odd_37x53_dense"], 11, axis=1)])
    gen = torch.Generator().manual_seed(4)
    keys = tg.draw_keys(dense.shape, "cpu", gen)
    assert keys.dtype == torch.int32 and int(keys.min()) >= 0
    out = tg.sample_pixels(dense, num, keys=keys)
    for b in range(2):
        for i in np.unique(dense[b]):
            n = int((dense[b] == i).sum())
            assert int((out[b] == i).sum()) == min(n, num)
        kept = out[b] >= 0
        np.testing.assert_array_equal(out[b][kept], dense[b][kept])
        assert set(np.unique(out[b][~kept]).tolist()) <= {-1}
    np.testing.assert_array_equal(out, tg.sample_pixels(dense, num, keys=keys))
    # the same generator state draws the same keys
    again = tg.sample_pixels(dense, num, generator=torch.Generator().manual_seed(4))
    np.testing.assert_array_equal(out, again)


def test_instance_targets_sampling_pads_with_zero(golden):
    g = golden("instance_targets")
    raw = g["odd_37x53_raw"]
    keys = tg.draw_keys((1, 37, 53), "cpu", torch.Generator().manual_seed(2))
    tb = tg.instance_targets(raw, size_divisibility=32, sample_num=20, keys=keys, label_dtype=torch.int32)
    lab = tb.label[0, 0].numpy()
    assert lab.shape == (64, 64) and not lab[37:].any() and not lab[:, 53:].any()           # the padding is 0, not -1
    np.testing.assert_array_equal(lab[:37, :53], tg.sample_pixels(g["odd_37x53_dense"], 20, keys=keys[0].numpy()))
    assert (lab[:37, :53] == -1).any()
    tb.check()


# ---- the criterion's argument checks --------------------------------------------------------------------------------------
def test_criterion_checks_a_target_batch():
    raw = np.zeros((2, 8, 8), np.uint8)
    raw[0, 2:5, 2:5] = 3
    tb = tg.instance_targets(raw)
    out = {"pred_logits": torch.zeros(2, 4, 3), "pred_masks": torch.zeros(2, 4, 4, 4)}
    assert cr._as_batch(tb, torch.device("cpu"), 2) is tb                                   # used as it is: no cat, no conversion
    assert tb.labels32.dtype == torch.int32 and tb.T == [1, 0] and tb.toff == [0, 1, 1]
    listed = cr._as_batch(tb.targets, torch.device("cpu"), 2)
    assert isinstance(listed, cr._Batch) and torch.equal(listed.masks, tb.masks) and listed.toff == tb.toff
    crit = cr.build_criterion(2, class_weight=2.0, mask_weight=5.0, dice_weight=5.0, no_object_weight=0.1, dec_layers=1,
                              train_num_points=16)
    three = {"pred_logits": torch.zeros(3, 4, 3), "pred_masks": torch.zeros(3, 4, 4, 4)}
    with pytest.raises(RuntimeError, match="TargetBatch of 2 images for predictions of 3"):
        crit(three, tb)
    with pytest.raises(RuntimeError, match="TargetBatch of 2 images for predictions of 3"):
        crit.matcher(three, tb)
    with pytest.raises(RuntimeError, match="lives on cpu"):
        cr._as_batch(tb, torch.device("cuda:0"), 2)
    broken = tg.instance_targets(raw)
    broken.masks = broken.masks.to(torch.float32)
    with pytest.raises(RuntimeError, match="uint8"):
        crit(out, broken)
    with pytest.raises(RuntimeError, match="GPU"):                                          # a host batch reaches the kernels' own check
        crit(out, tb)


# ---- header ---------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points():
    assert _lib.ABI_VERSION >= 39
    for name in ("msm_target_tables", "msm_target_write", "msm_sample_labels", "msm_sample_labels_workspace", "msm_target_table_row"):
        assert name in _lib._SIGNATURES and name in _lib.declared_symbols()
    assert _lib._HEADER.params["msm_target_write"][-1] == "stream" and _lib._HEADER.params["msm_sample_labels"][-1] == "stream"
