"""The definitions C1-C4 of unseenobjectswithmeanshift_amd/crops.py on the host path (no GPU): the crop box against an exact
restatement, the choice of the object against instance_targets' own tables, the fixed-point bilinear resize against float64 and
its algebraic properties, the nearest resize, the composition inside targets.training_batch against the reference's literal
per-image order, the reference's method by name, and the C ABI the kernels are declared with."""
import numpy as np
import pytest
import torch

import crop_cases as cc
from unseenobjectswithmeanshift_amd import _lib
from unseenobjectswithmeanshift_amd import augment as A
from unseenobjectswithmeanshift_amd import crops as C
from unseenobjectswithmeanshift_amd import targets as tg

FRACTIONS = (0.05, 0.1, 0.25, 0.5, 0.0)


def _one_object(H, W, box, ident=5):
    raw = np.zeros((1, H, W), np.uint8)
    x_min, y_min, x_max, y_max = box
    raw[0, y_min:y_max + 1, x_min:x_max + 1] = ident
    return raw


def _boxes(raw, keys, fractions, **kw):
    params = C.CropParams(C.pack_crop_table(keys, fractions))
    out = C.crop_boxes(raw, params, **kw)
    params.check()
    return out


# ------------------------------------------------------------------------------------------------------------------------ C2
def test_c2_every_box_of_a_7x9_image_equals_the_exact_restatement():
    H, W = 7, 9
    n = 0
    for x_min in range(W):
        for x_max in range(x_min, W):
            for y_min in range(H):
                for y_max in range(y_min, H):
                    for p in FRACTIONS:
                        got = C.square_pad_clamp_host((x_min, y_min, x_max, y_max), np.float32(p), H, W)
                        assert got == cc.c2_oracle((x_min, y_min, x_max, y_max), p, H, W), (x_min, y_min, x_max, y_max, p)
                        assert 0 <= got[0] < got[2] <= W - 1 and 0 <= got[1] < got[3] <= H - 1      # the redraw never runs
                        n += 1
    assert n == 45 * 28 * 5


@pytest.mark.parametrize("box", [(0, 0, 0, 0), (8, 6, 8, 6), (0, 2, 3, 2), (5, 0, 8, 1), (0, 5, 1, 6), (7, 3, 8, 6), (0, 0, 8, 6)])
def test_c2_through_crop_boxes_at_every_edge(box):
    """Boxes touching each image edge (and the corners, and the whole image) through the batch function: the row carries the box,
    the dense index 1, the raw id and the padding."""
    H, W = 7, 9
    raw = _one_object(H, W, box)
    for p in FRACTIONS:
        row = _boxes(raw, [123456789], [p])[0].tolist()
        if box == (0, 0, 8, 6):                                 # one value everywhere: K == 0, no object is chosen
            assert row == [*cc.c2_oracle(box, p, H, W)[:4], 0, -1, cc.c2_oracle(box, p, H, W)[4], 0]
        else:
            assert row == [*cc.c2_oracle(box, p, H, W)[:4], 1, 5, cc.c2_oracle(box, p, H, W)[4], 0]


def test_c2_ties_round_to_even_and_zero_padding_becomes_25():
    H, W = 60, 60
    # side 10, p 0.25: 2.5 -> 2;  side 14, p 0.25: 3.5 -> 4;  side 2, p 0.25: 0.5 -> 0 -> 25;  one pixel: side 0 -> 25
    for box, padding in (((20, 20, 30, 25), 2), ((20, 20, 34, 25), 4), ((20, 20, 22, 21), 25), ((31, 17, 31, 17), 25)):
        row = _boxes(_one_object(H, W, box), [0], [0.25])[0].tolist()
        assert row[C.COL_PADDING] == padding and row[:4] == list(cc.c2_oracle(box, 0.25, H, W)[:4])
    assert _boxes(_one_object(H, W, (31, 17, 31, 17)), [0], [0.25])[0].tolist()[:4] == [6, 0, 56, 42]
    assert _boxes(_one_object(H, W, (20, 20, 30, 25)), [0], [0.25])[0].tolist()[:4] == [18, 15, 32, 29]    # cy 22.5 -+ 5 -+ 2, truncated


def test_c2_the_smallest_image():
    for box in ((0, 0, 0, 0), (1, 1, 1, 1), (0, 1, 1, 1), (0, 0, 1, 1)):
        for p in FRACTIONS:
            got = C.square_pad_clamp_host(box, np.float32(p), 2, 2)
            assert got == cc.c2_oracle(box, p, 2, 2) and got[:4] == (0, 0, 1, 1)
    raw = np.array([[[0, 4], [0, 0]]], np.uint8)
    assert _boxes(raw, [7], [0.3])[0].tolist() == [0, 0, 1, 1, 1, 4, 25, 0]
    with pytest.raises(ValueError, match="at least 2 x 2"):
        C.crop_boxes(np.zeros((1, 1, 5), np.uint8), C.CropParams(C.pack_crop_table([0], [0.1])))


def test_a_padding_fraction_out_of_range_is_reported_not_carried_out():
    raw = _one_object(12, 20, (3, 3, 6, 8))
    for p in (np.nan, -0.5, 17.0, np.inf):
        params = C.CropParams(C.pack_crop_table([0], [p]))
        assert C.crop_boxes(raw, params)[0].tolist() == [0, 0, 19, 11, 0, -1, 0, C.CROP_BAD_ROW]
        with pytest.raises(ValueError, match="image 0.*padding fraction"):
            params.check()


# ------------------------------------------------------------------------------------------------------------------------ C1
def test_c1_keys_reach_the_first_and_the_last_object():
    raw = cc.label_images()["three"][None]
    first, last = _boxes(np.repeat(raw, 2, 0), [0, 2 ** 32 - 1], [0.1, 0.1]).tolist()
    assert first[C.COL_INDEX:C.COL_ID + 1] == [1, 4] and last[C.COL_INDEX:C.COL_ID + 1] == [3, 9]
    assert C.choose_object_host(4, 3, 0) == (1, 0) and C.choose_object_host(4, 3, 2 ** 32 - 1) == (3, 2)
    assert C.choose_object_host(4, 3, 2 ** 32 // 3 + 1) == (2, 1)
    # every object is reached, and about equally often
    seen = [C.choose_object_host(4, 3, k)[0] for k in np.linspace(0, 2 ** 32 - 1, 3001).astype(np.uint64)]
    assert sorted(set(seen)) == [1, 2, 3] and min(seen.count(i) for i in (1, 2, 3)) >= 1000


def test_c1_without_a_background_pixel_the_instance_row_is_the_dense_index():
    """No background pixel: K_b = T_b, the lowest id holds dense index 0 and, as in the reference (label == idx with idx >= 1), is
    never chosen; instance row t = idx."""
    raw = cc.label_images()["no_background"][None]
    tb = tg.instance_targets(raw)
    assert tb.counts == [4] and tb.ids.tolist() == [4, 7, 9, 12]
    rows = _boxes(np.repeat(raw, 2, 0), [0, 2 ** 32 - 1], [0.1, 0.1]).tolist()
    assert [r[C.COL_INDEX:C.COL_ID + 1] for r in rows] == [[1, 7], [3, 12]]
    assert C.choose_object_host(4, 4, 0) == (1, 1) and C.choose_object_host(4, 4, 2 ** 32 - 1) == (3, 3)
    two = cc.label_images()["two_no_background"][None]
    assert [_boxes(two, [k], [0.1])[0].tolist()[C.COL_INDEX:C.COL_ID + 1] for k in (0, 2 ** 32 - 1)] == [[1, 8], [1, 8]]


@pytest.mark.parametrize("name", ["background_only", "table_only", "one_value"])
def test_c1_nothing_to_choose_gives_the_whole_image(name):
    raw = cc.label_images()[name][None]
    H, W = raw.shape[1:]
    for p in FRACTIONS:
        row = _boxes(raw, [2 ** 31], [p])[0].tolist()
        assert row[:4] == list(cc.c2_oracle((0, 0, W - 1, H - 1), p, H, W)[:4]) and row[C.COL_INDEX:C.COL_ID + 1] == [0, -1]
    assert _boxes(raw, [2 ** 31], [0.5])[0].tolist()[:4] == [0, 0, 19, 11]      # a square around (9.5, 5.5) of side 19, clamped


def test_c1_agrees_with_the_tables_of_instance_targets():
    names, raw = cc.label_batch()
    keys = cc.crop_keys(len(names))
    p = np.linspace(0.05, 0.5, len(names))
    for bg in (tg.BACKGROUND_IDS, (), (0, 1, 4)):
        rows = _boxes(raw, keys, p, background_ids=bg)
        tb = tg.instance_targets(raw, background_ids=bg)
        H, W = raw.shape[1:]
        for b in range(len(names)):
            Kb, Tb = int(tb._status[b][2]), tb.counts[b]
            idx, t = C.choose_object_host(Kb, Tb, keys[b])
            assert rows[b, C.COL_INDEX] == idx
            if t is None:
                box = (0, 0, W - 1, H - 1)
                assert rows[b, C.COL_ID] == -1
            else:
                box = tuple(int(v) for v in tb.boxes[tb.toff[b] + t].tolist())
                assert rows[b, C.COL_ID] == int(tb.ids[tb.toff[b] + t])
                assert tb.label[b, 0][tb.masks[tb.toff[b] + t].bool()].unique().tolist() == [float(idx)]     # dense index of that instance
            assert rows[b, :4].tolist() == list(cc.c2_oracle(box, np.float32(p[b]), H, W)[:4])


# ------------------------------------------------------------------------------------------------------------------------ C4
def test_c4_same_size_reproduces_the_source():
    img = np.random.default_rng(0).integers(0, 256, size=(13, 13, 3), dtype=np.uint8)
    np.testing.assert_array_equal(C.resize_bilinear_host(img, 13), img)


def test_c4_half_size_is_the_rounded_mean_of_four():
    img = np.random.default_rng(1).integers(0, 256, size=(14, 14, 3), dtype=np.uint8).astype(np.int64)
    want = (img[0::2, 0::2] + img[0::2, 1::2] + img[1::2, 0::2] + img[1::2, 1::2] + 2) >> 2
    np.testing.assert_array_equal(C.resize_bilinear_host(img.astype(np.uint8), 7), want)


@pytest.mark.parametrize("value", [0, 1, 127, 254, 255])
def test_c4_a_constant_image_stays_constant(value):
    for ny, nx, S in ((5, 9, 7), (9, 5, 3), (2, 2, 16), (31, 17, 8)):
        assert (C.resize_bilinear_host(np.full((ny, nx, 3), value, np.uint8), S) == value).all()


def test_c4_weights_and_taps():
    for n, S in ((2, 16), (7, 7), (5, 9), (9, 5), (131, 16), (640, 224), (3, 1024)):
        s, s2, w0, w1 = C.bilinear_taps(n, S)
        assert (w0 + w1 == 2048).all() and (w1 >= 0).all() and (w1 < 2048).all()
        assert (0 <= s).all() and (s <= s2).all() and (s2 <= n - 1).all() and (s2 - s <= 1).all()
        src = np.clip((np.arange(S) + 0.5) * n / S - 0.5, 0, n - 1)
        assert np.abs((s + w1 / 2048) - src).max() <= 2.0 ** -12 + 1e-12      # a weight is off by at most half a step


def test_c4_stays_within_0625_of_float64_bilinear():
    """|out - float64 bilinear| <= 0.5 (the final rounding) + 255 * 2 * 2^-12 (the weight quantisation in x and in y) < 0.625, on
    random and on binary images, up- and downscaling, sizes that skip source pixels included."""
    rng = np.random.default_rng(2)
    worst = 0.0
    for i in range(120):
        ny, nx, S = (int(v) for v in rng.integers(2, 40, size=3))
        img = rng.integers(0, 256, size=(ny, nx, 3), dtype=np.uint8)
        if i % 3 == 0:
            img = np.where(img < 128, 0, 255).astype(np.uint8)
        worst = max(worst, np.abs(C.resize_bilinear_host(img, S) - cc.bilinear_f64(img, S)).max())
    for ny, nx, S in ((35, 131, 16), (9, 8, 24), (480, 640, 224)):
        img = rng.integers(0, 2, size=(ny, nx, 3), dtype=np.uint8) * 255
        worst = max(worst, np.abs(C.resize_bilinear_host(img, S) - cc.bilinear_f64(img, S)).max())
    print(f"worst |fixed point - float64| = {worst:.4f}")
    assert worst <= 0.5 + 255 * 2 * 2.0 ** -12 < 0.625


# ------------------------------------------------------------------------------------------------------------------------ C3
def test_c3_nearest():
    a = np.random.default_rng(3).integers(0, 1000, size=(2, 11, 6)).astype(np.int32)
    np.testing.assert_array_equal(C.resize_nearest_host(a[:, :6, :], 6), a[:, :6, :])          # n == S: the identity
    assert C.nearest_index(3, 7).tolist() == [0, 0, 0, 1, 1, 2, 2] and C.nearest_index(7, 3).tolist() == [0, 2, 4]
    for S in (4, 17):                                                                        # n > S and n < S, both axes
        got = C.resize_nearest_host(a, S)
        for dy in range(S):
            for dx in range(S):
                assert (got[:, dy, dx] == a[:, (dy * 11) // S, (dx * 6) // S]).all()
    f = np.random.default_rng(4).normal(size=(3, 5, 9)).astype(np.float32)
    f[0, 2, 3] = 0.0
    assert C.resize_nearest_host(f, 12).dtype == np.float32 and set(np.unique(C.resize_nearest_host(f, 12).view(np.int32))) <= set(np.unique(f.view(np.int32)))


def test_crop_resize_validates_caller_supplied_boxes():
    color, raw, xyz = cc.frame_case(4, 9, 8, 5, Hp=10, Wp=12)
    boxes = cc.box_rows([(0, 0, 7, 8), (5, 2, 3, 6), (0, 0, 8, 8), (1, -1, 4, 4)])      # good; x1 < x0; x1 >= W; negative y0
    c, r, z = C.crop_resize(color, raw, xyz, boxes, 6, size_divisibility=4)
    assert c.shape == (4, 6, 6, 3) and r.shape == (4, 6, 6) and r.dtype == raw.dtype and z.shape == (4, 3, 8, 8)
    assert boxes[:, C.COL_STATUS].tolist() == [0, C.CROP_BAD_BOX, C.CROP_BAD_BOX, C.CROP_BAD_BOX]
    assert not c[1:].any() and not r[1:].any() and not z[1:].any() and not z[:, :, 6:].any() and not z[:, :, :, 6:].any()
    np.testing.assert_array_equal(c[0], C.resize_bilinear_host(color[0], 6))
    np.testing.assert_array_equal(z[0, :, :6, :6].view(np.int32), C.resize_nearest_host(xyz[0, :, :9, :8], 6).view(np.int32))
    assert (z != 777.0).all()


# ------------------------------------------------------------------------------------------------------------------------ composition
def _literal_sample(color, raw, xyz, key, p, S, background_ids=(0, 1)):
    """One sample in the reference's literal order (tabletop_dataset.py:335-358) with this module's C1-C4 in place of the random
    draws and of cv2: fold, process_label, pick, tight box, square / pad / clamp, slice, resize, process_label again, annotations."""
    H, W = raw.shape
    lab = raw.astype(np.int64)
    lab[np.isin(lab, background_ids)] = 0
    values = np.unique(lab)
    dense = np.searchsorted(values, lab)                        # process_label
    K = int(dense.max())
    idx = 1 + ((int(key) * K) >> 32) if K > 0 else 0
    ys, xs = np.nonzero(dense == idx)                           # mask_to_tight_box
    x0, y0, x1, y1, _ = cc.c2_oracle((xs.min(), ys.min(), xs.max(), ys.max()), p, H, W)
    iy = (np.arange(S) * (y1 - y0 + 1)) // S
    ix = (np.arange(S) * (x1 - x0 + 1)) // S
    label_crop = dense[y0:y1 + 1, x0:x1 + 1][iy][:, ix]
    xyz_crop = xyz[:, y0:y1 + 1, x0:x1 + 1][:, iy][:, :, ix]
    img_crop = C.resize_bilinear_host(color[y0:y1 + 1, x0:x1 + 1], S)
    values2 = np.unique(label_crop)
    label2 = np.searchsorted(values2, label_crop)               # the second process_label
    masks, boxes = [], []
    for k, v in enumerate(values2):                             # process_label_to_annos: every value above 0 (all, when 0 is absent)
        if v == 0:
            continue
        m = label2 == k
        yy, xx = np.nonzero(m)
        masks.append(m), boxes.append((xx.min(), yy.min(), xx.max(), yy.max()))
    return img_crop, label2, xyz_crop, np.array(masks).reshape(-1, S, S), np.array(boxes, np.float32).reshape(-1, 4), (x0, y0, x1, y1)


def test_training_batch_with_crop_equals_the_literal_order():
    B, H, W, S = 3, 48, 64, 20
    color, depth, raw = cc.scene(B, H, W, seed=1)
    keys, p = np.array([0, 2 ** 31, 2 ** 32 - 1], np.uint64), np.array([0.05, 0.2, 0.5], np.float32)
    params = C.CropParams(C.pack_crop_table(keys, p))
    image, xyz, batch = tg.training_batch(color, depth, raw, cc.CAM, size_divisibility=32, crop=params, crop_size=S)
    params.check(), batch.check()
    assert tuple(image.shape) == tuple(xyz.shape) == (B, 3, 32, 32) and batch.image_size == (S, S) and tuple(batch.label.shape) == (B, 1, 32, 32)
    full_image, full_xyz, full = tg.training_batch(color, depth, raw, cc.CAM)
    assert full.counts == [3, 3, 3]
    from unseenobjectswithmeanshift_amd import frames
    row = 0
    for b in range(B):
        img_crop, label2, xyz_crop, masks, boxes, roi = _literal_sample(color[b], raw[b], full_xyz[b].numpy(), keys[b], p[b], S)
        assert batch.crop_boxes[b, :4].tolist() == list(roi)
        T = len(masks)
        assert batch.counts[b] == T
        np.testing.assert_array_equal(batch.masks[row:row + T, :S, :S].numpy(), masks)
        np.testing.assert_array_equal(batch.boxes[row:row + T].numpy(), boxes)
        np.testing.assert_array_equal(batch.label[b, 0, :S, :S].numpy(), label2.astype(np.float32))
        np.testing.assert_array_equal(xyz[b, :, :S, :S].numpy().view(np.int32), xyz_crop.view(np.int32))
        np.testing.assert_array_equal(image[b, :, :S, :S].numpy(), frames.ingest(img_crop, None, None)[0].numpy())
        assert not batch.masks[row:row + T, S:].any() and not batch.masks[row:row + T, :, S:].any() and not xyz[b, :, S:].any()
        row += T
    # image 0 is cropped tightly around object 3 (p = 0.05): the other objects leave the crop, and what was dense label 1 of three
    # still is label 1 -- of one; image 2 is cropped around the small object 7 in the corner with half its side as padding
    assert batch.crop_boxes[:, C.COL_ID].tolist() == [3, 5, 7] and batch.counts[0] == 1 and batch.ids[0] == 3
    assert batch.counts[2] < 3 and int(batch.ids[batch.toff[2]:batch.toff[3]][-1]) == 7
    assert sorted(batch.label[2, 0, :S, :S].unique().tolist()) == [float(i) for i in range(batch.counts[2] + 1)]     # renumbered 0 .. T


def test_training_batch_without_crop_is_what_it_was_and_sampling_runs_at_the_crop_size():
    B, H, W, S = 2, 48, 64, 24
    color, depth, raw = cc.scene(B, H, W, seed=2)
    a = tg.training_batch(color, depth, raw, cc.CAM, size_divisibility=32)
    b = tg.training_batch(color, depth, raw, cc.CAM, size_divisibility=32, crop=None)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2].masks, b[2].masks) and a[2].crop_boxes is None
    params = C.CropParams(C.pack_crop_table([5, 2 ** 31], [0.5, 0.5]))
    keys = tg.draw_keys((B, S, S), generator=torch.Generator().manual_seed(3))
    _, _, sampled = tg.training_batch(color, depth, raw, cc.CAM, crop=params, crop_size=S, sample_num=15, keys=keys)
    _, _, plain = tg.training_batch(color, depth, raw, cc.CAM, crop=params, crop_size=S)
    want = tg.sample_pixels(plain.label[:, 0].to(torch.int64), 15, keys=keys)
    assert torch.equal(sampled.label[:, 0].to(torch.int64), want) and (want == -1).any()
    with pytest.raises(ValueError, match="keys"):
        tg.training_batch(color, depth, raw, cc.CAM, crop=params, crop_size=S, sample_num=15, keys=tg.draw_keys((B, H, W)))
    image, xyz, batch = tg.training_batch(color, None, raw, cc.CAM, crop=params, crop_size=S)      # colour only
    assert xyz is None and tuple(image.shape) == (B, 3, S, S)


def test_augmentation_inside_a_cropped_batch_follows_the_reference_order():
    """Depth scaling, ellipses and point-cloud noise before the crop at the frame size, the colour augmentation after it at the
    crop size: each half equals the module's own function applied at that place."""
    B, H, W, S = 2, 48, 64, 24
    color, depth, raw = cc.scene(B, H, W, seed=4)
    rng = np.random.default_rng(5)
    aug = A.draw_params(B, S, S, rng=rng, generator=torch.Generator().manual_seed(1), add_noise=True)
    table = aug.table.copy()
    table[:, A.COL_FLAGS] = (table[:, A.COL_FLAGS] & ~A.FLAG_BLUR) | A.FLAG_GAUSSIAN | A.FLAG_CHROMATIC
    table.view(np.float32)[:, A.COL_SIGMA] = 9.5
    noise = torch.randn((B, S, S), generator=torch.Generator().manual_seed(2)).numpy()
    gp = torch.randn((B, 3, H // 4, W // 4), generator=torch.Generator().manual_seed(3)).numpy()
    aug = A.AugmentParams(table, noise, gp)
    params = C.CropParams(C.pack_crop_table([9, 2 ** 30], [0.3, 0.1]))
    image, xyz, batch = tg.training_batch(color, depth, raw, cc.CAM, augment=aug, crop=params, crop_size=S)
    aug.check(), params.check()
    _, full_xyz, _ = tg.training_batch(color, depth, raw, cc.CAM, augment=A.AugmentParams(table, None, gp))
    c, r, z = C.crop_resize(color, raw, full_xyz.numpy(), batch.crop_boxes, S)
    np.testing.assert_array_equal(xyz.numpy().view(np.int32), z.view(np.int32))
    from unseenobjectswithmeanshift_amd import frames
    np.testing.assert_array_equal(image.numpy(), frames.ingest(A.augment_color(c, A.AugmentParams(table, noise)), None, None)[0].numpy())
    plain = tg.training_batch(color, depth, raw, cc.CAM, crop=params, crop_size=S)
    assert not torch.equal(plain[0], image) and not torch.equal(plain[1], xyz) and torch.equal(plain[2].masks, batch.masks)


def test_a_pixel_noise_field_of_the_frame_size_raises():
    B, H, W, S = 2, 48, 64, 24
    color, depth, raw = cc.scene(B, H, W, seed=4)
    aug = A.AugmentParams(A.pack_table(B, gaussian=True, sigma=3.0), np.zeros((B, H, W), np.float32))
    with pytest.raises(ValueError, match=r"pixel_noise \(2, 48, 64\) must be \(2, 24, 24\)"):
        tg.training_batch(color, depth, raw, cc.CAM, augment=aug, crop=C.CropParams(C.pack_crop_table([0, 0], [0.1, 0.1])), crop_size=S)
    with pytest.raises(ValueError, match="3 crop parameter rows for 2 frames"):
        tg.training_batch(color, depth, raw, cc.CAM, crop=C.CropParams(C.pack_crop_table([0, 0, 0], [0.1] * 3)), crop_size=S)


# ------------------------------------------------------------------------------------------------------------------------ by name
def test_pad_crop_resize_by_name():
    color, depth, raw = cc.scene(1, 48, 64, seed=6)
    dense = tg.process_label(np.where(raw[0] == 1, 0, raw[0]))                     # what __getitem__ hands in: 0 .. 3
    xyz_img = np.random.default_rng(7).normal(size=(48, 64, 3)).astype(np.float32)
    params = C.CropParams(C.pack_crop_table([2 ** 31], [0.2]))
    img_crop, label_crop, depth_crop = C.pad_crop_resize(color[0], dense, xyz_img, size=20, params=params)
    assert img_crop.shape == (20, 20, 3) and label_crop.shape == (20, 20) and depth_crop.shape == (20, 20, 3)
    assert label_crop.dtype == dense.dtype and depth_crop.dtype == np.float32
    ys, xs = np.nonzero(dense == 2)                                                  # key 2^31 of K = 3: idx 2
    x0, y0, x1, y1, _ = cc.c2_oracle((xs.min(), ys.min(), xs.max(), ys.max()), 0.2, 48, 64)
    np.testing.assert_array_equal(img_crop, C.resize_bilinear_host(color[0, y0:y1 + 1, x0:x1 + 1], 20))
    np.testing.assert_array_equal(label_crop, C.resize_nearest_host(dense[y0:y1 + 1, x0:x1 + 1], 20))
    np.testing.assert_array_equal(depth_crop, np.transpose(C.resize_nearest_host(np.transpose(xyz_img, (2, 0, 1))[:, y0:y1 + 1, x0:x1 + 1], 20), (1, 2, 0)))
    # tensors in, tensors out; no depth, no depth; the default draws come from rng and repeat with it
    t = C.pad_crop_resize(torch.from_numpy(color[0]), torch.from_numpy(dense), None, size=20, params=C.CropParams(C.pack_crop_table([2 ** 31], [0.2])))
    assert isinstance(t[0], torch.Tensor) and t[2] is None and np.array_equal(t[0].numpy(), img_crop) and np.array_equal(t[1].numpy(), label_crop)
    a = C.pad_crop_resize(color[0], dense, None, rng=np.random.default_rng(8))
    b = C.pad_crop_resize(color[0], dense, None, rng=np.random.default_rng(8))
    assert a[0].shape == (224, 224, 3) and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_draw_crop_params():
    p = C.draw_crop_params(500, rng=np.random.default_rng(0))
    assert p.table.shape == (500, 2) and p.table.dtype == np.int32 and not p.is_device and len(p) == 500
    assert p.fractions.dtype == np.float32 and 0.05 <= p.fractions.min() < 0.1 and 0.45 < p.fractions.max() < 0.5
    assert p.keys.dtype == np.uint32 and p.keys.min() < 2 ** 27 and p.keys.max() > 2 ** 32 - 2 ** 27
    q = C.draw_crop_params(500, rng=np.random.default_rng(0))
    assert np.array_equal(p.table, q.table)
    g = C.draw_crop_params(64, generator=torch.Generator().manual_seed(1), min_padding=0.2, max_padding=0.2)
    assert (g.fractions == np.float32(0.2)).all() and len(set(g.keys.tolist())) == 64
    with pytest.raises(ValueError, match="min_padding"):
        C.draw_crop_params(1, rng=np.random.default_rng(0), min_padding=0.6, max_padding=0.5)
    assert p.check() is p and p.to("cpu") is p


# ------------------------------------------------------------------------------------------------------------------------ ABI
def test_the_header_declares_the_crop_entry_points():
    assert _lib.ABI_VERSION >= 42
    params = _lib._HEADER.params
    assert {"msm_crop_boxes", "msm_train_crop"} <= set(_lib.declared_symbols())
    assert params["msm_crop_boxes"] == ["tables", "params", "boxes", "B", "H", "W", "stream"]
    assert params["msm_train_crop"] == ["color", "raw", "raw_is_i32", "xyz", "boxes", "color_out", "raw_out", "xyz_out", "B", "H", "W", "Hp",
                                        "Wp", "S", "Sp", "stream"]
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    for name, value in (("MSM_CROP_BOX_ROW", C.CROP_BOX_ROW), ("MSM_CROP_MAX_SIZE", C.MAX_SIZE), ("MSM_CROP_DEGENERATE", C.CROP_DEGENERATE),
                        ("MSM_CROP_BAD_BOX", C.CROP_BAD_BOX), ("MSM_CROP_BAD_ROW", C.CROP_BAD_ROW)):
        assert _lib._define(text, name) == value
