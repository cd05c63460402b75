"""msm_ingest_frames on the GPU against the host path of frames.py (itself pinned to the definition and to the reference's values in
tests/test_frames_cpu.py): bit for bit, border included, at the smallest shapes that take each of the kernel's paths -- element-wise
and four-pixel loads, element-wise and 16-byte stores, a last workgroup that is not full --, once at the real frame size and once at the
smallest batch of such frames that sends the workgroups round their grid-stride loop a second time; then raw frames through the
two-stage harness and BatchedTwoStage."""
import ctypes

import numpy as np
import pytest
import torch

from unseenobjectswithmeanshift_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -77.25


def raw_frames(F, H, W, kind, seed):
    rng = np.random.default_rng(seed)
    color = rng.integers(0, 256, size=(F, H, W, 3), dtype=np.uint8)
    if kind == "u16":
        depth = rng.integers(0, 5000, size=(F, H, W)).astype(np.uint16)
        depth[:, 0, :3] = [0, 65535, 1]
    else:
        depth = rng.uniform(-1.0, 4.0, size=(F, H, W)).astype(np.float32)
        depth[:, 0, :2] = [0.0, -0.0]
    return color, depth


def cams_for(F, H, W):
    return [{"fx": 616.3653 + 3.1 * f, "fy": 616.2043 - 1.7 * f, "x_offset": W / 2 + 0.4837 + f, "y_offset": H / 2 + 0.1759 - f} for f in range(F)]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def dev_depth(depth):
    t = torch.from_numpy(depth)
    return (t.view(torch.int16) if t.dtype == torch.uint16 else t).to(DEV)


def run_kernel(color, depth, cams, frame, **kw):
    """ops.ingest_frames into sentinel-filled outputs -> (image, xyz or None) on the device."""
    from unseenobjectswithmeanshift_amd import frames, ops
    F, H, W, _ = color.shape
    Hp, Wp = frame
    out_image = torch.full((F, 3, Hp, Wp), SENTINEL, device=DEV)
    out_depth = torch.full((F, 3, Hp, Wp), SENTINEL, device=DEV) if depth is not None else None
    lut = torch.from_numpy(frames.image_lut()).to(DEV)
    cam = frames.camera_table(cams, F).to(DEV) if depth is not None else None
    image, xyz = ops.ingest_frames(torch.from_numpy(color).to(DEV), None if depth is None else dev_depth(depth), cam, lut, frame=frame,
                                   out_image=out_image, out_depth=out_depth, **kw)
    assert image is out_image and xyz is out_depth
    return image, xyz


def host_padded(color, depth, cams, frame, **kw):
    """The host path's tensors placed in a zero frame of the requested size."""
    from unseenobjectswithmeanshift_amd import frames
    F, H, W, _ = color.shape
    image, xyz = frames.ingest(color, depth, cams if depth is not None else None, **kw)
    out = []
    for t in (image, xyz):
        if t is None:
            out.append(None)
            continue
        p = torch.zeros((F, 3) + tuple(frame))
        p[:, :, :H, :W] = t
        out.append(p)
    return out


# F, H, W, frame -> quads = F * Hp * ceil(Wp / 4), workgroups of 256 quads:
#   1x5x7                element-wise everywhere (Wp % 4 != 0); 10 quads: one partial workgroup
#   3x5x7 into 32x32     unaligned rows in, 16-byte stores out, border, per-frame intrinsics; 768 quads = 3 full workgroups
#   2x33x70 into 64x96   row tail after full vectors; 3072 quads = 12 full workgroups
#   2x33x70 into 64x100  the same with a last workgroup that is not full: 3200 quads = 12.5 workgroups
#   2x8x36               the aligned four-pixel path alone; 144 quads: one partial workgroup
#   1x480x640            the real frame size; 76 800 quads = 300 workgroups, one loop iteration each
SHAPES = [(1, 5, 7, (5, 7)), (3, 5, 7, (32, 32)), (2, 33, 70, (64, 96)), (2, 33, 70, (64, 100)), (2, 8, 36, (8, 36)),
          (1, 480, 640, (480, 640))]


@pytest.mark.parametrize("kind", ["u16", "f32"])
@pytest.mark.parametrize("F,H,W,frame", SHAPES)
def test_kernel_equals_host_path_bitwise(F, H, W, frame, kind):
    color, depth = raw_frames(F, H, W, kind, seed=H + W)
    cams = cams_for(F, H, W)
    image, xyz = run_kernel(color, depth, cams, frame)
    ref_image, ref_xyz = host_padded(color, depth, cams, frame)
    assert not (image == SENTINEL).any() and not (xyz == SENTINEL).any()              # every element written, border included
    assert torch.equal(bits(image), bits(ref_image))
    assert torch.equal(bits(xyz), bits(ref_xyz))
    if frame != (H, W):
        assert not bits(image[:, :, H:]).any() and not bits(image[:, :, :, W:]).any() and not bits(xyz[:, :, H:]).any() and not bits(xyz[:, :, :, W:]).any()


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_grid_stride_second_iteration_bitwise(kind):
    """The grid is capped at 2048 workgroups of 256 lanes: beyond 524 288 quads a workgroup takes further quads at a stride of the
    whole grid (the 16 x 480 x 640 batch of the two-stage pipeline: 1 228 800 quads, two to three iterations).  Seven frames of
    480 x 640 are the smallest batch of real frames past the cap: 537 600 quads, the first 13 312 lanes go round a second time, and
    their quads lie in the last frame -- row, frame and column are recomputed there with that frame's own intrinsics."""
    F, H, W = 7, 480, 640
    assert F * H * (W // 4) > 2048 * 256 >= (F - 1) * H * (W // 4)
    color, depth = raw_frames(F, H, W, kind, seed=77)
    cams = cams_for(F, H, W)
    image, xyz = run_kernel(color, depth, cams, (H, W))
    ref_image, ref_xyz = host_padded(color, depth, cams, (H, W))
    assert not (image == SENTINEL).any() and not (xyz == SENTINEL).any()
    assert torch.equal(bits(image), bits(ref_image)) and torch.equal(bits(xyz), bits(ref_xyz))
    tail = 2048 * 256 - (F - 1) * H * (W // 4)                   # quads of the last frame before the second iteration begins
    y0 = tail // (W // 4)
    assert 0 < y0 < H - 1 and torch.equal(bits(xyz[-1, :, y0:]), bits(ref_xyz[-1, :, y0:]))


@pytest.mark.parametrize("F,H,W,frame", [(2, 33, 70, (64, 96)), (2, 8, 36, (8, 36)), (1, 5, 7, (5, 7))])
def test_image_only_and_swapped_channels(F, H, W, frame):
    color, depth = raw_frames(F, H, W, "u16", seed=11)
    cams = cams_for(F, H, W)
    image, none = run_kernel(color, None, None, frame)
    assert none is None and not (image == SENTINEL).any()
    assert torch.equal(bits(image), bits(host_padded(color, None, None, frame)[0]))
    image, xyz = run_kernel(color, depth, cams, frame, swap_rb=True)
    ref_image, ref_xyz = host_padded(color, depth, cams, frame, order="rgb")
    assert torch.equal(bits(image), bits(ref_image)) and torch.equal(bits(xyz), bits(ref_xyz))
    assert torch.equal(bits(image), bits(host_padded(np.ascontiguousarray(color[..., ::-1]), None, None, frame)[0]))


@pytest.mark.parametrize("H,W,frame", [(5, 7, (5, 7)), (8, 36, (32, 64))])
def test_float_depth_nan_becomes_zero_and_inf_propagates(H, W, frame):
    color, depth = raw_frames(2, H, W, "f32", seed=12)
    depth[:, 1, :5] = [np.nan, np.inf, -np.inf, np.nan, 1.5]
    depth[1, :, W // 2] = np.inf                                                     # a column where (x - px) can be small, never 0
    cams = cams_for(2, H, W)
    cams[0]["x_offset"] = 1.0                                                        # x == px at x = 1: 0 * inf = NaN in xyz[0]
    image, xyz = run_kernel(color, depth, cams, frame)
    _, ref = host_padded(color, depth, cams, frame)
    got = xyz.cpu()
    assert torch.isnan(ref).any() and torch.isinf(ref).any()
    assert torch.equal(torch.isnan(got), torch.isnan(ref))                          # NaNs compared as NaN (payloads may differ)
    ok = ~torch.isnan(ref)
    assert torch.equal(bits(got)[ok], bits(ref)[ok])
    assert float(got[0, 2, 1, 0]) == 0.0 and float(got[0, 2, 1, 3]) == 0.0           # NaN depth -> z = 0


def test_frames_module_runs_the_kernel_on_device_tensors():
    from unseenobjectswithmeanshift_amd import frames
    color, depth = raw_frames(2, 33, 70, "u16", seed=13)
    cams = cams_for(2, 33, 70)
    image, xyz = frames.ingest(torch.from_numpy(color).to(DEV), dev_depth(depth), cams, size_divisibility=32)
    ref_image, ref_xyz = frames.ingest(color, depth, cams, size_divisibility=32)
    assert image.is_cuda and tuple(image.shape) == (2, 3, 64, 96)
    assert torch.equal(bits(image), bits(ref_image)) and torch.equal(bits(xyz), bits(ref_xyz))
    s = frames.make_sample(torch.from_numpy(color[0]).to(DEV), dev_depth(depth[0]), cams[0])
    assert s["image_color"].is_cuda and torch.equal(bits(s["depth"]), bits(ref_xyz[0, :, :33, :70]))
    zf = (depth[0].astype(np.float32) / np.float32(1000))
    pts = frames.compute_xyz(torch.from_numpy(zf).to(DEV), cams[0]["fx"], cams[0]["fy"], cams[0]["x_offset"], cams[0]["y_offset"])
    assert tuple(pts.shape) == (33, 70, 3) and torch.equal(bits(pts.permute(2, 0, 1)), bits(ref_xyz[0, :, :33, :70]))
    with pytest.raises(ValueError):
        frames.ingest(torch.from_numpy(color).to(DEV), torch.from_numpy(depth.astype(np.float32)), cams)      # colour on the device, depth on the host


def test_bad_arguments_raise_and_launch_nothing():
    from unseenobjectswithmeanshift_amd import _lib, frames, ops
    L = _lib.lib()
    color = torch.zeros((1, 5, 7, 3), dtype=torch.uint8, device=DEV)
    depth = torch.zeros((1, 5, 7), dtype=torch.float32, device=DEV)
    lut = torch.from_numpy(frames.image_lut()).to(DEV)
    cam = torch.ones((1, 4), device=DEV)
    image = torch.full((1, 3, 5, 7), SENTINEL, device=DEV)
    xyz = torch.full((1, 3, 5, 7), SENTINEL, device=DEV)
    p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())      # noqa: E731
    s = ops._stream()

    def call(color_, depth_, xyz_, H, W, Hp, Wp, div=1000.0):
        return L.msm_ingest_frames(p(color_), p(depth_), 0, div, p(lut), p(cam), p(image), p(xyz_), 1, H, W, Hp, Wp, 0, s)

    for args, what in (((None, depth, xyz, 5, 7, 5, 7), "null"), ((color, depth, xyz, 5, 7, 4, 7), "smaller"),
                       ((color, depth, xyz, 5, 7, 5, 6), "smaller"), ((color, depth, None, 5, 7, 5, 7), "go together"),
                       ((color, None, xyz, 5, 7, 5, 7), "go together"), ((color, depth, xyz, 5, 7, 5, 7, 0.0), "depth_div")):
        rc = call(*args)
        assert rc == -1 and what in L.msm_last_error_string().decode()
        with pytest.raises(RuntimeError, match="msm_ingest_frames"):
            _lib.check(rc, "msm_ingest_frames")
    with pytest.raises(RuntimeError, match="smaller"):
        ops.ingest_frames(color, depth, cam, lut, frame=(4, 7))
    torch.cuda.synchronize()
    assert bool((image == SENTINEL).all()) and bool((xyz == SENTINEL).all())           # nothing was launched
    assert call(color, depth, xyz, 5, 7, 5, 7) == 0
    torch.cuda.synchronize()
    assert not (image == SENTINEL).any()


def _small_model():
    from unseenobjectswithmeanshift_amd.meta_arch import MeanShiftMaskFormer, build_resnet50_head
    head = build_resnet50_head(num_queries=100, dec_layers=3)
    head.pixel_decoder.load_state_dict(syn.synth_state_dict(syn.pixel_decoder_param_shapes()), strict=True)
    head.predictor.load_state_dict(syn.synth_state_dict(syn.decoder_param_shapes(dec_layers=3)), strict=True)
    return MeanShiftMaskFormer(backbone=syn.StandInBackbone().to(DEV).eval(), sem_seg_head=head.to(DEV).eval(), num_queries=100)


def _differing(a, b):
    return int((a != b).sum())


def test_raw_frames_through_the_two_stage_pipeline():
    """BatchedTwoStage and test_batch_crop_nolabel on raw samples: the slot's input buffers hold exactly frames.make_sample's tensors,
    and the results are those of the float samples -- bitwise where two float runs agree bitwise, else within their own difference."""
    from unseenobjectswithmeanshift_amd import frames
    from unseenobjectswithmeanshift_amd import two_stage as ts
    model = _small_model()

    class Pred:
        def batch_tensors(self, samples):
            imgs = torch.stack([x["image"] for x in samples])
            with torch.no_grad():
                return model.inference_images({"image": imgs, "depth": torch.stack([x["depth"] for x in samples])},
                                              tuple(int(v) for v in imgs.shape[-2:]))[:3]

    H, W = 192, 256
    rng = np.random.default_rng(21)
    color = rng.integers(0, 256, size=(2, H, W, 3), dtype=np.uint8)
    depth = rng.integers(300, 3000, size=(2, H, W)).astype(np.uint16)
    depth[rng.random((2, H, W)) < 0.3] = 0                                          # missing depth
    cams = cams_for(2, H, W)
    raw = [{"color": color[f], "depth_raw": depth[f], "camera_params": cams[f]} for f in range(2)]             # host frames (pinned staging)
    raw_dev = [{"color": torch.from_numpy(color[f]).to(DEV), "depth_raw": dev_depth(depth[f]), "camera_params": cams[f]} for f in range(2)]
    flt = [{k: v.to(DEV) for k, v in frames.make_sample(color[f], depth[f], cams[f]).items()} for f in range(2)]
    kw = dict(topk=False, confident_score=0.0)

    def check(run_float, run_raw):
        a, b = run_float(), run_float()
        r = run_raw()
        assert a[2] and len(a[2]) > 0                                                  # there are crops: the second stage ran
        for i in (0, 1):
            d_float, d_raw = _differing(a[i], b[i]), _differing(r[i], a[i])
            print(f"output {i}: float runs differ on {d_float} pixels, raw vs float on {d_raw}")
            assert d_raw <= d_float
        if _differing(a[0], b[0]) == 0 and _differing(a[1], b[1]) == 0:
            assert torch.equal(r[0], a[0]) and torch.equal(r[1], a[1]) and r[2] == a[2]

    pipe = ts.BatchedTwoStage(model, 2, (H, W), use_depth=True, **kw)
    clone = lambda o: (o[0].clone(), o[1].clone(), o[2])      # noqa: E731  (the slot owns the tensors until its next batch)
    check(lambda: clone(pipe(flt)), lambda: clone(pipe(raw)))
    st = pipe._slots[0]
    want_image, want_depth = torch.stack([s["image_color"] for s in flt]), torch.stack([s["depth"] for s in flt])
    assert torch.equal(bits(st["images"]), bits(want_image)) and torch.equal(bits(st["depths"]), bits(want_depth))
    pipe(flt)
    pipe(raw_dev)                                                                    # frames already on the device: no staging
    assert torch.equal(bits(st["images"]), bits(want_image)) and torch.equal(bits(st["depths"]), bits(want_depth))
    res = pipe.run([raw, flt, raw])                                                  # two slots, raw and float batches alternating
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[2][0], res[0][0]) and res[0][2] == res[1][2]
    with pytest.raises(ValueError, match="mixed"):
        pipe([raw[0], flt[1]])
    with pytest.raises(ValueError, match=r"\(192, 256, 3\) expected"):
        pipe([dict(raw[0], color=color[0][:100]), raw[1]])
    with pytest.raises(ValueError, match="one dtype and one place"):                 # host and device frames in one batch
        pipe([raw[0], raw_dev[1]])
    with pytest.raises(ValueError, match="one dtype and one place"):                 # uint16 and float32 depth in one batch
        pipe([raw[0], dict(raw[1], depth_raw=depth[1].astype(np.float32))])
    with pytest.raises(ValueError, match="depth_raw"):
        pipe([dict(r, depth_raw=depth[0].astype(np.float64)) for r in raw])
    # channel order and depth unit are the pipeline's: rgb8 frames with depth in 1/4 mm give the same input tensors
    pipe_rgb = ts.BatchedTwoStage(model, 2, (H, W), use_depth=True, graphs=False, order="rgb", depth_scale=4000.0, **kw)
    frames4 = [{"color": np.ascontiguousarray(color[f][..., ::-1]), "depth_raw": depth[f], "camera_params": cams[f]} for f in range(2)]
    pipe_rgb(frames4)
    torch.cuda.synchronize()
    want4 = frames.ingest(color, depth, cams, depth_scale=4000.0)
    assert torch.equal(bits(pipe_rgb._slots[0]["images"]), bits(want4[0])) and torch.equal(bits(pipe_rgb._slots[0]["depths"]), bits(want4[1]))
    # the eager batch
    check(lambda: ts.test_batch_crop_nolabel(flt, Pred(), Pred(), use_depth=True, **kw),
          lambda: ts.test_batch_crop_nolabel(raw_dev, Pred(), Pred(), use_depth=True, **kw))
    with pytest.raises(ValueError, match="mixed"):
        ts.test_batch_crop_nolabel([raw_dev[0], flt[1]], Pred(), Pred(), **kw)
    with pytest.raises(ValueError, match="one dtype and one place"):
        ts.test_batch_crop_nolabel([raw[0], raw_dev[1]], Pred(), Pred(), **kw)
