"""Training targets on the HIP kernels (pytest -m gpu): msm_target_tables / msm_target_write / msm_sample_labels through
unseenobjectswithmeanshift_amd.targets against the reference's results (tests/golden/instance_targets.npz) and against the host
path of the same module, bit for bit; the criterion on a TargetBatch against the criterion on the reference's list; the seam into
training.ucn_model_losses.  Every comparison is for equality."""
import numpy as np
import pytest
import torch

from unseenobjectswithmeanshift_amd import criterion as cr
from unseenobjectswithmeanshift_amd import ops
from unseenobjectswithmeanshift_amd import synthetic as syn
from unseenobjectswithmeanshift_amd import targets as tg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ["scene", "background_only", "table_only", "no_background", "one_pixel", "borders", "odd_37x53", "d1_37x53"]
FIELDS = ("masks", "labels", "boxes", "ids", "areas", "label")


def _same(dev_batch, host_batch):
    assert dev_batch.counts == host_batch.counts and dev_batch.toff == host_batch.toff
    for f in FIELDS:
        a, b = getattr(dev_batch, f), getattr(host_batch, f)
        assert a.is_cuda and a.dtype == b.dtype and a.shape == b.shape, f
        assert torch.equal(a.cpu(), b), f


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("raw_dtype", [torch.uint8, torch.int32])
@pytest.mark.parametrize("label_dtype", [torch.float32, torch.int32])
def test_device_equals_fixture_and_host(golden, name, raw_dtype, label_dtype):
    g = golden("instance_targets")
    raw, d = g[f"{name}_raw"], int(g[f"{name}_d"])
    dev = tg.instance_targets(torch.from_numpy(raw).to(DEV, raw_dtype), size_divisibility=d, label_dtype=label_dtype)
    _same(dev, tg.instance_targets(raw, size_divisibility=d, label_dtype=label_dtype))
    dev.check()
    np.testing.assert_array_equal(dev.masks.cpu().numpy(), g[f"{name}_target_masks"].astype(np.uint8))
    np.testing.assert_array_equal(dev.boxes.cpu().numpy(), g[f"{name}_boxes"].reshape(-1, 4))
    np.testing.assert_array_equal(dev.labels.cpu().numpy(), g[f"{name}_target_labels"])
    np.testing.assert_array_equal(dev.label[0, 0].cpu().numpy(), g[f"{name}_label_padded"].astype(dev.label.cpu().numpy().dtype))
    (t0,) = dev.targets
    assert t0["masks"].dtype == torch.bool and t0["masks"].data_ptr() == dev.masks.data_ptr() and t0["labels"].dtype == torch.int64


@pytest.mark.parametrize("name", ["scene", "no_background", "d1_37x53"])
def test_the_three_methods_on_device_tensors(golden, name):
    g = golden("instance_targets")
    folded = g[f"{name}_raw"].astype(np.int32)
    folded[folded == 1] = 0
    x = torch.from_numpy(folded).to(DEV)
    boxes, masks, classes = tg.process_label_to_annos(x)
    np.testing.assert_array_equal(boxes.cpu().numpy(), g[f"{name}_boxes"])
    np.testing.assert_array_equal(masks.cpu().numpy(), g[f"{name}_masks"].astype(np.float32))
    np.testing.assert_array_equal(classes.cpu().numpy(), g[f"{name}_target_labels"])
    dense = tg.process_label(x)
    np.testing.assert_array_equal(dense.cpu().numpy(), g[f"{name}_dense"])
    num = int(g[f"{name}_sample_num"])
    np.testing.assert_array_equal(tg.sample_pixels(dense, num, generator=torch.Generator(DEV).manual_seed(1)).cpu().numpy(),
                                  g[f"{name}_sampled"])


def _mixed_batch(golden):
    """The edge cases in one 48 x 64 batch: scene, background only, no background, table only, one pixel, borders, speckle."""
    g = golden("instance_targets")
    raw = np.zeros((7, 48, 64), np.uint8)
    raw[0] = g["scene_raw"]
    raw[2] = np.kron(g["no_background_raw"], np.ones((3, 4), np.uint8))[:48, :64]        # 48 x 80 cut to 48 x 64: still no background
    raw[3] = 1
    raw[4, :12, :18] = g["one_pixel_raw"]
    raw[5, 0, :] = raw[5, -1, :] = raw[5, :, 0] = raw[5, :, -1] = 6
    raw[6, :37, :53] = g["odd_37x53_raw"]
    return raw


@pytest.mark.parametrize("shape,d", [((48, 64), 32), ((47, 61), 32), ((47, 61), 1)])
def test_mixed_batch(golden, shape, d):
    """toff and the per-image tables across images with T_b = 0 in the middle; vector and element-wise loads and stores."""
    raw = np.ascontiguousarray(_mixed_batch(golden)[:, :shape[0], :shape[1]])
    host = tg.instance_targets(raw, size_divisibility=d)
    assert host.counts[1] == 0 and host.counts[3] == 0 and host.counts[2] == 3 and min(host.counts[4:]) >= 1
    for dt in (torch.uint8, torch.int32):
        dev = tg.instance_targets(torch.from_numpy(raw).to(DEV, dt), size_divisibility=d)
        _same(dev, host)
        dev.check()


def test_ids_1023_and_1024():
    raw = torch.zeros((2, 20, 32), dtype=torch.int32)
    raw[0, 3:9, 4:30] = 1023
    raw[1, 5, 5] = 7
    ok = tg.instance_targets(raw.to(DEV))
    assert ok.check().ids.tolist() == [1023, 7] and ok.boxes.tolist() == [[4, 3, 29, 8], [5, 5, 5, 5]]
    raw[1, 0, 31] = 1024
    raw[1, 19, 0] = -1
    bad = tg.instance_targets(raw.to(DEV))
    assert bad.counts == [1, 1] and torch.equal(bad.masks.cpu(), ok.masks.cpu())          # they belong to no instance
    with pytest.raises(ValueError, match=r"image 1 has 2 pixels with ids outside \[0, 1024\)"):
        bad.check()
    _same(bad, tg.instance_targets(raw))


def test_counts_from_the_loader(golden, monkeypatch):
    raw = torch.from_numpy(_mixed_batch(golden)).to(DEV)
    ref = tg.instance_targets(raw, size_divisibility=32)
    monkeypatch.setattr(tg, "_fetch_counts", lambda tables: pytest.fail("counts= must not copy the counts back"))
    given = tg.instance_targets(raw, size_divisibility=32, counts=ref.counts)
    _same(given, tg.instance_targets(raw.cpu(), size_divisibility=32))
    given.check()
    # wrong in both directions: rows beyond T_b are zero, instances beyond the count are dropped, check() raises
    for wrong in ([c + 1 for c in ref.counts], [max(c - 1, 0) for c in ref.counts], [0] * 7, [5, 0, 0, 9, 0, 2, 1]):
        got = tg.instance_targets(raw, size_divisibility=32, counts=wrong)
        _same(got, tg.instance_targets(raw.cpu(), size_divisibility=32, counts=wrong))
        with pytest.raises(ValueError, match="counts"):
            got.check()


def test_wrong_counts_never_leave_the_buffer(golden):
    """The mask buffer sits between two guard bands; whatever toff says, the bands keep their bytes."""
    raw = torch.from_numpy(_mixed_batch(golden)).to(DEV)
    tables = ops.target_tables(raw, torch.tensor([0, 1], dtype=torch.int32, device=DEV))
    true = tables[:, 1].tolist()
    G, Hp, Wp = 3, 64, 64
    tables_before = tables.clone()
    for counts in (true, [c + 2 for c in true], [0] * 7, [40, 0, 0, 0, 0, 0, 0], None):
        TT = sum(true) if counts is None else sum(counts)
        # None: offsets that point far outside the buffer, backwards and negative
        toff = [0, 1000, -5, 3, 2 ** 40, 1, 2, TT] if counts is None else np.concatenate([[0], np.cumsum(counts)]).tolist()
        big = torch.full((TT + 2 * G, Hp, Wp), 0xAB, dtype=torch.uint8, device=DEV)
        t = tables_before.clone()
        label, masks, boxes, ids, areas = ops.target_write(raw, t, torch.tensor(toff, dtype=torch.int64, device=DEV), TT,
                                                           frame=(Hp, Wp), masks=big[G:G + TT])
        torch.cuda.synchronize()
        assert bool((big[:G] == 0xAB).all()) and bool((big[G + TT:] == 0xAB).all()), counts
        assert int(masks.max()) <= 1 if TT else True
        mismatch = (t[:, 3] & ops.TARGET_COUNT_MISMATCH).bool().tolist()
        want = [True] * 7 if counts is None else [a != b for a, b in zip(counts, true)]
        if counts is None:                                   # image 5's range [1, 2) happens to hold its one instance
            want[5] = true[5] != 1
        assert mismatch == want, counts
        if counts is not None:                               # a partition of the buffer: every byte is written
            assert int((masks == 0xAB).sum()) == 0


# ---- msm_sample_labels ----------------------------------------------------------------------------------------------------
def _sample_both(dense_np, keys_np, num, label_dtype, image_size=None):
    lab = torch.from_numpy(dense_np).to(DEV, label_dtype).contiguous()
    H, W = image_size or dense_np.shape[1:]
    status = ops.sample_labels_(lab, torch.from_numpy(keys_np).to(DEV), num, image_size)
    want = dense_np.copy()
    want[:, :H, :W] = tg._sample_host(dense_np[:, :H, :W], keys_np, num)
    assert status.tolist() == [0] * dense_np.shape[0]
    np.testing.assert_array_equal(lab.cpu().numpy().astype(np.int64), want)


@pytest.mark.parametrize("label_dtype", [torch.float32, torch.int32])
@pytest.mark.parametrize("keys_kind", ["equal", "few", "signed", "full"])
def test_sample_labels_ties_and_thresholds(golden, label_dtype, keys_kind):
    g = golden("instance_targets")
    base = g["odd_37x53_dense"].astype(np.int64)
    dense = np.stack([base, np.roll(base, 9, axis=1), np.zeros_like(base)])
    dense[2, ::3] = 255                                      # the highest label the sampler takes; labels past the LDS histogram
    dense[2, 1::3, ::2] = 40
    dense[1, 0, :7] = -1                                     # already ignored pixels stay
    rng = np.random.default_rng(3)
    keys = {"equal": np.full(dense.shape, 12345, np.int64), "few": rng.integers(0, 4, size=dense.shape),
            "signed": rng.integers(-2 ** 31, 2 ** 31, size=dense.shape),
            "full": rng.integers(0, 2 ** 31 - 1, size=dense.shape)}[keys_kind].astype(np.int32)
    n = int((base == 5).sum())                               # one label's count: num on the threshold, below and above it
    assert n > 3
    for num in (1, 2, n - 1, n, n + 1, 100, 5000):
        _sample_both(dense, keys, num, label_dtype)


def test_sample_labels_padded_corner(golden):
    g = golden("instance_targets")
    dense = np.zeros((2, 64, 64), np.int64)
    dense[:, :37, :53] = g["odd_37x53_dense"]
    keys = np.random.default_rng(8).integers(0, 2 ** 31 - 1, size=(2, 37, 53)).astype(np.int32)
    keys[1] = 7
    _sample_both(dense, keys, 25, torch.float32, (37, 53))    # the padding (label 0 there) is neither counted nor touched
    lab = torch.full((1, 8, 8), 256.0, device=DEV)
    lab[0, 0, 0] = 1.5
    status = ops.sample_labels_(lab, torch.zeros((1, 8, 8), dtype=torch.int32, device=DEV), 3)
    assert status.tolist() == [64] and bool((lab.flatten()[1:] == 256.0).all())


def test_sampled_targets_at_480x640():
    """One frame of 470 x 630 padded to 480 x 640, 20 labels, num = 1000, keys from a seeded generator."""
    H, W = 470, 630
    raw = np.zeros((1, H, W), np.uint8)
    for i in range(19):
        raw[0, 20 + 10 * (i % 5):300 + 9 * i, 8 + 32 * i:8 + 32 * i + 28] = 2 + 3 * i
    keys = tg.draw_keys((1, H, W), DEV, torch.Generator(DEV).manual_seed(5))
    dev = tg.instance_targets(torch.from_numpy(raw).to(DEV), size_divisibility=32, sample_num=1000, keys=keys)
    host = tg.instance_targets(raw, size_divisibility=32, sample_num=1000, keys=keys.cpu())
    assert host.counts == [19] and tuple(dev.label.shape) == (1, 1, 480, 640)
    _same(dev, host)
    dev.check()
    lab = dev.label[0, 0].cpu()
    assert not lab[H:].any() and not lab[:, W:].any()        # the padding stays 0
    assert [int((lab[:H, :W] == i).sum()) for i in range(20)] == [1000] * 20
    # drawn from the generator inside the call: the same keys
    again = tg.instance_targets(torch.from_numpy(raw).to(DEV), size_divisibility=32, sample_num=1000,
                                generator=torch.Generator(DEV).manual_seed(5))
    assert torch.equal(again.label, dev.label)


# ---- the criterion on a TargetBatch ---------------------------------------------------------------------------------------
def _criterion_runs(golden, solver):
    """One criterion call with backward on the TargetBatch and one on its ``.targets`` list: same predictions, same seed."""
    raw = torch.from_numpy(np.ascontiguousarray(_mixed_batch(golden)[[0, 1, 2]])).to(DEV)
    batch = tg.instance_targets(raw, size_divisibility=32)                # 48 x 64 -> 64 x 64, T = (3, 0, 3)
    assert batch.counts == [3, 0, 3]
    outputs, _ = syn.synth_criterion_inputs(n_pred=3, B=3, T=(3, 0, 3), Q=20, hm=12, wm=16, hg=64, wg=64, seed=2)
    runs = []
    for targets in (batch, batch.targets):
        preds = [{k: v.to(DEV).requires_grad_(True) for k, v in p.items() if k != "aux_outputs"}
                 for p in [outputs] + outputs["aux_outputs"]]
        out = dict(preds[0])
        out["aux_outputs"] = preds[1:]
        crit = cr.build_criterion(2, class_weight=2.0, mask_weight=5.0, dice_weight=5.0, no_object_weight=0.1, dec_layers=3,
                                  train_num_points=500, generator=torch.Generator().manual_seed(7), solver=solver)
        losses = crit(out, targets)
        crit.check_matching()
        sum(losses[k] * crit.weight_dict[k] for k in losses).backward()
        runs.append({"losses": {k: v.detach().cpu() for k, v in losses.items()},
                     "grad_logits": [p["pred_logits"].grad.cpu() for p in preds], "grad_masks": [p["pred_masks"].grad.cpu() for p in preds],
                     "indices": crit.last_indices, "selection": crit.last_selection.cpu(), "points": [t.cpu() for t in crit.last_points]})
    return batch, preds, runs


@pytest.mark.parametrize("solver", ["host", "device"])
def test_criterion_on_a_target_batch_equals_the_list(golden, solver):
    """Losses, assignments, drawn points, importance-sampling selections and the gradients of the class logits: bit for bit."""
    batch, preds, (a, b) = _criterion_runs(golden, solver)
    assert list(a["losses"]) == list(b["losses"]) and len(a["losses"]) == 9
    for k in a["losses"]:
        assert torch.equal(a["losses"][k], b["losses"][k]) and bool(torch.isfinite(a["losses"][k])), k
    for ga, gb in zip(a["grad_logits"], b["grad_logits"]):
        assert torch.equal(ga, gb) and float(ga.abs().sum()) > 0
    assert torch.equal(a["selection"], b["selection"]) and all(torch.equal(x, y) for x, y in zip(a["points"], b["points"]))
    for pa, pb in zip(a["indices"], b["indices"]):
        assert all(torch.equal(i0, i1) and torch.equal(j0, j1) for (i0, j0), (i1, j1) in zip(pa, pb))
    listed = cr._Batch(batch.targets, DEV)                              # what the list path concatenates: the buffer itself
    assert torch.equal(listed.masks, batch.masks) and torch.equal(listed.labels32, batch.labels32) and listed.toff == batch.toff
    m = cr.HungarianMatcher(cost_class=2.0, cost_mask=5.0, cost_dice=5.0, num_points=200, generator=torch.Generator().manual_seed(1))
    ia = m({k: v.detach() for k, v in preds[0].items()}, batch)
    m.generator.manual_seed(1)
    ib = m({k: v.detach() for k, v in preds[0].items()}, batch.targets)
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(ia, ib)) and [len(i) for i, _ in ia] == [3, 0, 3]


@pytest.mark.parametrize("solver", ["host", "device"])
def test_criterion_mask_gradients_bit_identical(golden, solver):
    """The gradients of the mask logits, bit for bit between the TargetBatch and the list.  They can only agree because
    msm_point_loss_bwd itself repeats bit for bit: one workgroup sums a matched mask's gradient in 64-bit fixed point with integer
    atomics (masks up to 20 479 pixels).  With float atomics two identical calls on the LIST differed in about 700 of 34 560
    elements by up to 3.7e-9 at a maximum of 3.2e-2."""
    _, _, (a, b) = _criterion_runs(golden, solver)
    for p, (ga, gb) in enumerate(zip(a["grad_masks"], b["grad_masks"])):
        diff = (ga - gb).abs()
        print(f"grad pred_masks[{p}] ({solver}): {int((ga != gb).sum())} of {ga.numel()} elements differ, max |diff| = "
              f"{float(diff.max()):.3e}, max |grad| = {float(ga.abs().max()):.3e}")
    for ga, gb in zip(a["grad_masks"], b["grad_masks"]):
        assert float(ga.abs().sum()) > 0 and torch.equal(ga, gb)


def test_point_loss_backward_repeats_bit_for_bit():
    """msm_point_loss_bwd at the training size (120 x 160 masks, the fixed-point LDS form) and at a small one: two calls give the
    same bits, and the same values as the float form (global atomics) up to its rounding; a nan gradient poisons whole masks."""
    from test_gpu_criterion import _point_case
    for hm, wm, T in ((120, 160, (3, 0, 5)), (12, 16, (2, 4))):
        masks, tgt, rows, pairs, os_pts, rnd, k, N = _point_case(hm, wm, 480, 640, T, Q=20)
        losses, bits, ws = ops.point_loss_fwd(masks, tgt, pairs, os_pts, rnd, k, 7.0)
        g = torch.tensor([[5.0, 3.0], [5.0, 2.0]], device=DEV)
        runs = [ops.point_loss_bwd(masks, tgt, pairs, os_pts, rnd, ws, g, k, 7.0) for _ in range(3)]
        flt = ops.point_loss_bwd(masks, tgt, pairs, os_pts, rnd, ws, g, k, 7.0, global_atomics=True)
        for p in range(len(masks)):
            assert torch.equal(runs[0][p], runs[1][p]) and torch.equal(runs[0][p], runs[2][p]) and float(runs[0][p].abs().sum()) > 0
            # both are sums of the same fp32 terms, at most 4 P = 4000 per pixel: they differ by the float form's roundings
            err = float((runs[0][p].double() - flt[p].double()).norm() / flt[p].double().norm())
            print(f"fixed point vs float atomics, {hm}x{wm}, prediction {p}: relative L2 {err:.2e}")
            assert err <= 4000 * 2.0 ** -24
        bad = ops.point_loss_bwd(masks, tgt, pairs, os_pts, rnd, ws, torch.tensor([[float("nan"), 3.0], [5.0, 2.0]], device=DEV), k, 7.0)
        matched = [r[2] for r in rows if r[0] == 0]
        flat = bad[0].flatten(0, 1)
        assert bool(torch.isnan(flat[matched]).all()) and not bool(torch.isnan(bad[1]).any())


# ---- the seam: raw frames in, a loss dict out ----------------------------------------------------------------------------------
def test_training_batch_feeds_ucn_model_losses():
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
    rng = np.random.default_rng(0)
    H, W = 60, 90                                            # padded to 64 x 96
    color = torch.from_numpy(rng.integers(0, 256, size=(2, H, W, 3), dtype=np.uint8)).to(DEV)
    depth = torch.from_numpy(rng.integers(400, 2000, size=(2, H, W)).astype(np.int16)).to(DEV)
    raw = np.zeros((2, H, W), np.uint8)
    raw[:, 40:, :] = 1
    for b in range(2):
        for t in range(3):
            raw[b, 4 + 16 * t:18 + 16 * t, 8 + 4 * b:70 + 4 * b] = 3 + 2 * t
    cam = {"fx": 570.3, "fy": 570.3, "x_offset": 45.0, "y_offset": 30.0}
    image, xyz, batch = tg.training_batch(color, depth, torch.from_numpy(raw).to(DEV), cam, size_divisibility=32, sample_num=200,
                                          generator=torch.Generator(DEV).manual_seed(2))
    assert tuple(image.shape) == tuple(xyz.shape) == (2, 3, 64, 96) and tuple(batch.label.shape) == (2, 1, 64, 96)
    assert batch.counts == [3, 3] and tuple(batch.masks.shape) == (6, 64, 96)
    crit = cr.build_criterion(2, class_weight=2.0, mask_weight=5.0, dice_weight=5.0, no_object_weight=0.1, dec_layers=3,
                              train_num_points=112, generator=torch.Generator().manual_seed(9), solver="device")
    losses = tr.ucn_model_losses(model, image, xyz, batch, crit, labels=batch.label, embedding_loss=EmbeddingLoss(0.02, 0.5, 1.0, 1.0),
                                 embedding_weight=0.5)
    assert len(losses) == 3 * 3 + 1 and all(bool(torch.isfinite(v)) for v in losses.values())
    sum(losses.values()).backward()
    batch.check()
    crit.check_matching()
    grads = [p.grad for p in model.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads) and any(float(g.abs().sum()) > 0 for g in grads)
