"""The training-crop kernels (pytest -m gpu): msm_crop_boxes / msm_train_crop through unseenobjectswithmeanshift_amd.crops against
the host path of the same module -- EQUAL BITS, every comparison -- with guard bands around every output, boxes that must be
refused without a wild access, the ``crop=`` seam of targets.training_batch and its way into training.ucn_model_losses."""
import numpy as np
import pytest
import torch

import crop_cases as cc
from unseenobjectswithmeanshift_amd import augment as A
from unseenobjectswithmeanshift_amd import crops as C
from unseenobjectswithmeanshift_amd import ops
from unseenobjectswithmeanshift_amd import targets as tg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256                      # elements on either side of an output
FILL = {torch.uint8: 0xA5, torch.int32: -7, torch.float32: -7.0}


def _guarded(shape, dtype, shift=0):
    """(buffer, view): a contiguous tensor of ``shape`` inside a buffer filled with FILL, ``shift`` elements off the guard."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD + shift,), FILL[dtype], dtype=dtype, device=DEV)
    return buf, buf[GUARD + shift:GUARD + shift + n].view(shape)


def _guards_intact(buf, view):
    n, start, fill = view.numel(), view.storage_offset(), FILL[view.dtype]
    return bool((buf[:start] == fill).all()) and bool((buf[start + n:] == fill).all())


def _shifted(a, shift):
    """The array on the device, ``shift`` elements into its storage."""
    t = torch.from_numpy(a)
    buf = torch.zeros((t.numel() + shift + 16,), dtype=t.dtype, device=DEV)
    view = buf[shift:shift + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def _crop(color, raw, xyz, rows, S, Sp, shift=0):
    """ops.train_crop into guarded outputs against the host path on the same box rows; returns the host results."""
    host_boxes = rows.copy()
    want = C._crop_resize_host(color, raw, xyz, host_boxes, S, Sp)
    B = raw.shape[0]
    boxes = torch.from_numpy(rows.copy()).to(DEV)
    ldt = torch.uint8 if raw.dtype == np.uint8 else torch.int32
    outs = [_guarded((B, S, S, 3), torch.uint8, shift), _guarded((B, S, S), ldt, shift)]
    if xyz is not None:
        outs.append(_guarded((B, 3, Sp, Sp), torch.float32, shift))
    got = ops.train_crop(_shifted(color, shift), _shifted(raw, shift), None if xyz is None else _shifted(xyz, shift), boxes, S, frame=Sp,
                         out_color=outs[0][1], out_raw=outs[1][1], out_xyz=outs[2][1] if xyz is not None else None)
    assert all(_guards_intact(buf, view) for buf, view in outs)
    np.testing.assert_array_equal(got[0].cpu().numpy(), want[0])
    np.testing.assert_array_equal(got[1].cpu().numpy(), want[1])
    if xyz is not None:
        np.testing.assert_array_equal(got[2].cpu().numpy().view(np.int32), want[2].view(np.int32))
    else:
        assert got[2] is None
    assert boxes.cpu().numpy().tolist() == host_boxes.tolist()
    return want, host_boxes


def _box_set(H, W):
    """Each corner of the image, the whole image, the smallest legal box, a strip of two rows, a tall box that clamping at the
    right edge made non-square."""
    return cc.box_rows([(0, 0, W // 2, H // 2), (W // 2, 0, W - 1, H // 2), (0, H // 2, W // 2, H - 1), (W // 2, H // 2, W - 1, H - 1),
                        (0, 0, W - 1, H - 1), (3, 4, 4, 5), (0, H - 3, W - 1, H - 2), (W - 4, 1, W - 1, H - 2)])


SHAPES = [(21, 38, 17, 20), (16, 64, 32, 64), (9, 8, 24, 32), (35, 131, 16, 18)]


@pytest.mark.parametrize("mode", ["colour_and_labels", "xyz", "xyz_padded"])
@pytest.mark.parametrize("label", [np.uint8, np.int32], ids=["u8", "i32"])
@pytest.mark.parametrize("H,W,S,Sp", SHAPES, ids=lambda v: str(v))
def test_crop_equals_the_host_path(H, W, S, Sp, label, mode):
    """21 x 38 -> 17: nothing a multiple of 4 (element-wise stores); 16 x 64 -> 32: the vector stores; 9 x 8 -> 24: upscaling in both
    directions; 35 x 131 -> 16: downscaling by more than 2, the taps skip source pixels.  ``xyz_padded``: Hp > H, Wp > W on the
    input and Sp > S on the output, whose padding must be zero."""
    padded = mode == "xyz_padded"
    color, raw, xyz = cc.frame_case(8, H, W, H * W + S, label_dtype=label, with_xyz=mode != "colour_and_labels",
                                    Hp=H + 3 if padded else H, Wp=W + 5 if padded else W)
    want, boxes = _crop(color, raw, xyz, _box_set(H, W), S, Sp if padded else S)
    assert not boxes[:, C.COL_STATUS].any()
    if padded:
        assert not want[2][:, :, S:].any() and not want[2][:, :, :, S:].any() and (want[2] != 777.0).all()
    assert all(want[0][b].std() > 0 for b in range(8))


@pytest.mark.parametrize("label", [np.uint8, np.int32], ids=["u8", "i32"])
def test_crop_with_outputs_off_their_16_byte_alignment(label):
    """S = 32, Sp = 64 would take the vector stores; every tensor one element into its storage takes the element-wise ones."""
    color, raw, xyz = cc.frame_case(8, 16, 64, 11, label_dtype=label, Hp=16, Wp=64)
    a, _ = _crop(color, raw, xyz, _box_set(16, 64), 32, 64, shift=1)
    b, _ = _crop(color, raw, xyz, _box_set(16, 64), 32, 64, shift=0)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_invalid_boxes_give_zeros_and_a_status_bit():
    """x1 < x0, x1 >= W, a negative y0, x0 == x1, values far outside: zeros and MSM_CROP_BAD_BOX for those rows, the good rows
    between them as without them, intact guard bands.  Handled by a bounds check by construction: nothing here can fault."""
    H, W, S = 21, 38, 17
    color, raw, xyz = cc.frame_case(8, H, W, 12, Hp=H + 3, Wp=W + 5)
    rows = cc.box_rows([(0, 0, W - 1, H - 1), (20, 2, 10, 9), (5, 5, W, 9), (2, -1, 9, 9), (3, 4, 4, 5), (7, 3, 7, 9),
                        (-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1), (2 ** 30, 2 ** 30, 2 ** 30 + 5, 2 ** 30 + 5)])
    want, boxes = _crop(color, raw, xyz, rows, S, 20)
    bad = [1, 2, 3, 5, 6, 7]
    assert boxes[:, C.COL_STATUS].tolist() == [C.CROP_BAD_BOX if b in bad else 0 for b in range(8)]
    assert not want[0][bad].any() and not want[1][bad].any() and not want[2][bad].any()
    good, _ = _crop(color[[0, 4]], raw[[0, 4]], xyz[[0, 4]], rows[[0, 4]], S, 20)
    assert all(np.array_equal(w[[0, 4]], g) for w, g in zip(want, good))
    params = C.CropParams(C.pack_crop_table([0] * 8, [0.1] * 8)).to(DEV)
    dboxes = torch.from_numpy(rows).to(DEV)
    C.crop_resize(torch.from_numpy(color).to(DEV), torch.from_numpy(raw).to(DEV), torch.from_numpy(xyz).to(DEV), dboxes, S)
    params.status = dboxes[:, C.COL_STATUS]
    with pytest.raises(ValueError, match="image 1.*does not lie inside"):
        params.check()


@pytest.mark.parametrize("label", [torch.uint8, torch.int32], ids=["u8", "i32"])
@pytest.mark.parametrize("background_ids", [tg.BACKGROUND_IDS, (), (0, 1, 4)], ids=["table", "none", "more"])
def test_crop_boxes_equal_the_host_path(label, background_ids):
    """The CPU cases' label images -- K == 0 in three forms, no background pixel in two -- under keys that reach the first and
    the last object, padding fractions that include 0, ties and one that is refused."""
    names, raw = cc.label_batch()
    raw = np.concatenate([raw, raw])
    B = len(raw)
    keys = cc.crop_keys(B)
    p = np.resize(np.array([0.05, 0.0, 0.25, 0.5, 0.1, 16.0, 17.0, 0.3], np.float32), B)
    host = C.CropParams(C.pack_crop_table(keys, p))
    want = C.crop_boxes(raw, host, background_ids=background_ids)
    dev = host.to(DEV)
    got = C.crop_boxes(torch.from_numpy(raw).to(DEV).to(label), dev, background_ids=background_ids)
    assert got.dtype == torch.int32 and got.cpu().numpy().tolist() == want.tolist()
    assert dev.status.cpu().tolist() == host.status.tolist() and C.CROP_BAD_ROW in host.status.tolist()
    with pytest.raises(ValueError, match="padding fraction"):
        dev.check()
    buf, out = _guarded((B, C.CROP_BOX_ROW), torch.int32)
    rawd = torch.from_numpy(raw).to(DEV)
    tables = ops.target_tables(rawd, tg._device_background(rawd.device, background_ids))
    ops.crop_boxes(tables, dev.table, raw.shape[1:], out=out)
    assert _guards_intact(buf, out) and out.cpu().numpy().tolist() == want.tolist()


def test_crop_boxes_bound_what_they_read_from_a_table():
    """Hand-made table rows that contradict themselves -- counts far too large, an instance box outside the image: the whole
    image and MSM_CROP_BAD_ROW, never an index outside the row.  Bounds checks by construction: nothing here can fault."""
    raw = torch.from_numpy(np.stack([cc.label_images()["three"]] * 4)).to(DEV)
    tables = ops.target_tables(raw, tg._device_background(raw.device, tg.BACKGROUND_IDS))
    inst = 4 + 2 * ops.TARGET_BINS
    tables[0, 2] = 2 ** 31 - 1                                  # K_b: the instance row becomes negative
    tables[1, 1] = 2 ** 31 - 1                                  # T_b and K_b: an instance row beyond the 1023 records
    tables[1, 2] = 2 ** 31 - 1
    tables[2, inst + 4] = 20                                    # x_max of instance 0 == W
    params = C.CropParams(C.pack_crop_table([0, 2 ** 32 - 1, 0, 0], [0.1] * 4)).to(DEV)
    got = ops.crop_boxes(tables, params.table, (12, 20)).cpu().numpy()
    whole = [0, 0, 19, 11, 0, -1, 0, C.CROP_BAD_ROW]
    assert got[:3].tolist() == [whole] * 3
    assert got[3].tolist() == C.crop_boxes(cc.label_images()["three"][None], C.CropParams(C.pack_crop_table([0], [0.1])))[0].tolist()


def test_library_abi_and_refused_shapes():
    from unseenobjectswithmeanshift_amd import _lib
    L = _lib.lib()
    assert L.msm_abi_version() == _lib.ABI_VERSION >= 42 and hasattr(L, "msm_crop_boxes") and hasattr(L, "msm_train_crop")
    color = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=DEV)
    raw = torch.zeros((1, 8, 8), dtype=torch.uint8, device=DEV)
    boxes = torch.from_numpy(cc.box_rows([(0, 0, 7, 7)])).to(DEV)
    with pytest.raises(RuntimeError, match="bad size"):
        ops.train_crop(color, raw, None, boxes, 1025)
    with pytest.raises(RuntimeError, match=r"must lie in \[1, frame"):
        ops.train_crop(color, raw, None, boxes, 8, frame=4)
    with pytest.raises(RuntimeError, match="bad shape"):
        ops.train_crop(color[:, :1].contiguous(), raw[:, :1].contiguous(), None, boxes, 4)
    with pytest.raises(RuntimeError, match="must hold the image"):
        ops.train_crop(color, raw, torch.zeros((1, 3, 7, 8), device=DEV), boxes, 4)
    with pytest.raises(RuntimeError, match="bad shape"):
        ops.crop_boxes(ops.target_tables(raw), torch.zeros((1, 2), dtype=torch.int32, device=DEV), (1, 8))


# ------------------------------------------------------------------------------------------------------------------------ the whole
def _device_scene(B, H, W, seed):
    color, depth, raw = cc.scene(B, H, W, seed)
    return (color, depth, raw), (torch.from_numpy(color).to(DEV), torch.from_numpy(depth.view(np.int16)).to(DEV), torch.from_numpy(raw).to(DEV))


def _augment_pair(B, H, W, S, seed):
    table = A.draw_params(B, S, S, rng=np.random.default_rng(seed), generator=torch.Generator().manual_seed(seed), add_noise=True).table.copy()
    table[0, A.COL_FLAGS] = (table[0, A.COL_FLAGS] & ~A.FLAG_BLUR) | A.FLAG_GAUSSIAN | A.FLAG_CHROMATIC
    table.view(np.float32)[0, A.COL_SIGMA] = 9.5
    noise = torch.randn((B, S, S), generator=torch.Generator().manual_seed(seed + 1)).numpy()
    gp = torch.randn((B, 3, H // 4, W // 4), generator=torch.Generator().manual_seed(seed + 2)).numpy()
    host = A.AugmentParams(table, noise, gp)
    return host, host.to(DEV)


@pytest.mark.parametrize("augment", [False, True], ids=["plain", "augmented"])
@pytest.mark.parametrize("sample_num", [None, 40], ids=["all_pixels", "sampled"])
def test_training_batch_with_crop_equals_the_host_path(augment, sample_num):
    B, H, W, S = 2, 64, 96, 32
    host_frames, dev_frames = _device_scene(B, H, W, seed=3)
    crop = C.CropParams(C.pack_crop_table([2 ** 31, 2 ** 32 - 1], [0.4, 0.15]))
    ha, da = _augment_pair(B, H, W, S, 5) if augment else (None, None)
    kw = {}
    if sample_num:
        keys = tg.draw_keys((B, S, S), generator=torch.Generator().manual_seed(7))
        kw = {"sample_num": sample_num, "keys": keys}
    himage, hxyz, hbatch = tg.training_batch(*host_frames, cc.CAM, size_divisibility=32, augment=ha, crop=crop, crop_size=S, **kw)
    if sample_num:
        kw["keys"] = keys.to(DEV)
    dcrop = crop.to(DEV)
    image, xyz, batch = tg.training_batch(*dev_frames, cc.CAM, size_divisibility=32, augment=da, crop=dcrop, crop_size=S, **kw)
    dcrop.check(), batch.check()
    if augment:
        da.check()
    assert image.is_cuda and tuple(image.shape) == tuple(xyz.shape) == (B, 3, S, S) and batch.image_size == (S, S)
    assert torch.equal(image.cpu(), himage) and torch.equal(xyz.cpu().view(torch.int32), hxyz.view(torch.int32))
    assert batch.counts == hbatch.counts and torch.equal(batch.masks.cpu(), hbatch.masks) and torch.equal(batch.label.cpu(), hbatch.label)
    assert torch.equal(batch.boxes.cpu(), hbatch.boxes) and torch.equal(batch.ids.cpu(), hbatch.ids) and torch.equal(batch.areas.cpu(), hbatch.areas)
    assert batch.crop_boxes.cpu().numpy().tolist() == np.asarray(hbatch.crop_boxes).tolist()
    assert batch.crop_boxes[:, C.COL_ID].tolist() == [5, 7] and (not sample_num or bool((batch.label == -1).any()))


def test_training_batch_without_crop_issues_what_it_issued():
    B, H, W = 2, 64, 96
    _, dev_frames = _device_scene(B, H, W, seed=4)
    a = tg.training_batch(*dev_frames, cc.CAM, size_divisibility=32)
    launches = []
    from unseenobjectswithmeanshift_amd import _lib
    L = _lib.lib()
    saved = {}
    for name in _lib.CallTimer.timed_entry_points():             # every launch entry point, by name, in call order
        saved[name] = getattr(L, name)
        setattr(L, name, lambda *args, _fn=saved[name], _name=name: (launches.append(_name), _fn(*args))[1])
    try:
        b = tg.training_batch(*dev_frames, cc.CAM, size_divisibility=32, crop=None)
    finally:
        for name, fn in saved.items():
            setattr(L, name, fn)
    assert launches == ["msm_ingest_frames", "msm_target_tables", "msm_target_write"]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2].masks, b[2].masks) and torch.equal(a[2].label, b[2].label)
    assert a[2].crop_boxes is None and b[2].crop_boxes is None


def test_cropped_training_batch_feeds_ucn_model_losses():
    from unseenobjectswithmeanshift_amd import criterion as cr
    from unseenobjectswithmeanshift_amd import synthetic as syn
    from unseenobjectswithmeanshift_amd import training as tr
    from unseenobjectswithmeanshift_amd.embedding_loss import EmbeddingLoss
    from unseenobjectswithmeanshift_amd.meta_arch import build_ucn_model
    torch.manual_seed(3)
    model = build_ucn_model(num_queries=8, dec_layers=2)
    with torch.no_grad():
        for name, p in model.sem_seg_head.named_parameters():
            p.copy_(syn.synth_param(name, p.shape, salt=3))
    model.backbone.load_state_dict(syn.ucn_backbone_state_dict(syn.ucn_backbone_param_shapes(), salt=6), strict=True)
    model = model.to(DEV).train()
    model.backbone.miopen_find = False
    B, H, W, S = 2, 64, 96, 32
    _, dev_frames = _device_scene(B, H, W, seed=3)
    _, da = _augment_pair(B, H, W, S, 5)
    crop = C.draw_crop_params(B, rng=np.random.default_rng(1), device=DEV)
    image, xyz, batch = tg.training_batch(*dev_frames, cc.CAM, size_divisibility=32, sample_num=200, generator=torch.Generator(DEV).manual_seed(2),
                                          augment=da, crop=crop, crop_size=S)
    crop.check(), da.check()
    assert tuple(image.shape) == tuple(xyz.shape) == (B, 3, S, S) and all(c >= 1 for c in batch.counts)
    crit = cr.build_criterion(2, class_weight=2.0, mask_weight=5.0, dice_weight=5.0, no_object_weight=0.1, dec_layers=3,
                              train_num_points=112, generator=torch.Generator().manual_seed(9), solver="device")
    losses = tr.ucn_model_losses(model, image, xyz, batch, crit, labels=batch.label, embedding_loss=EmbeddingLoss(0.02, 0.5, 1.0, 1.0),
                                 embedding_weight=0.5)
    assert len(losses) == 3 * 3 + 1 and all(bool(torch.isfinite(v)) for v in losses.values())
    sum(losses.values()).backward()
    batch.check()
    grads = [p.grad for p in model.backbone.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads) and any(float(g.abs().sum()) > 0 for g in grads)


def test_pad_crop_resize_on_a_device_frame():
    color, depth, raw = cc.scene(1, 48, 64, seed=6)
    dense = tg.process_label(np.where(raw[0] == 1, 0, raw[0]))
    xyz_img = np.random.default_rng(7).normal(size=(48, 64, 3)).astype(np.float32)
    table = C.pack_crop_table([2 ** 31], [0.2])
    want = C.pad_crop_resize(color[0], dense, xyz_img, size=20, params=C.CropParams(table))
    got = C.pad_crop_resize(torch.from_numpy(color[0]).to(DEV), torch.from_numpy(dense).to(DEV), torch.from_numpy(xyz_img).to(DEV), size=20,
                            params=C.CropParams(table).to(DEV))
    assert got[1].dtype == torch.uint8
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g.cpu().numpy(), w)
