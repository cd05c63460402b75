"""frames.py on the host (no GPU): the numpy path of ingest / make_sample / compute_xyz against a literal float32 restatement of the
definition and against values captured from the reference's own read_sample / compute_xyz (tests/golden/frame_ingest.npz, made by
tests/golden/make_golden_frames.py) -- bit for bit, the sign of zero included.  tests/test_gpu_frames.py holds the kernel to this path."""
import re

import numpy as np
import pytest
import torch

from unseenobjectswithmeanshift_amd import _lib, frames

CAM = {"fx": 616.3653, "fy": 616.2043, "x_offset": 321.4837, "y_offset": 240.1759}


def bits(a):
    a = a.numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    assert a.dtype == np.float32
    return np.ascontiguousarray(a).view(np.int32)


def raw_frames(F, H, W, kind, seed):
    """Seeded raw frames with the edge values of the depth formats in the first pixels of every frame."""
    rng = np.random.default_rng(seed)
    color = rng.integers(0, 256, size=(F, H, W, 3), dtype=np.uint8)
    if kind == "u16":
        depth = rng.integers(0, 5000, size=(F, H, W)).astype(np.uint16)
        depth[:, 0, :3] = [0, 65535, 1]
    else:
        depth = rng.uniform(-1.0, 4.0, size=(F, H, W)).astype(np.float32)
        depth[:, 0, :4] = [np.nan, 0.0, -2.5, -0.0]
    return color, depth


def cams_for(F, H, W):
    return [{"fx": 616.3653 + 3.1 * f, "fy": 616.2043 - 1.7 * f, "x_offset": W / 2 + 0.4837 + f, "y_offset": H / 2 + 0.1759 - f} for f in range(F)]


def definition(color, depth, cams, *, depth_scale=1000.0, frame=None, means=frames.PIXEL_MEANS):
    """The issue's definition, pixel by pixel in scalar float32 operations (no broadcasting, no table)."""
    f32 = np.float32
    F, H, W, _ = color.shape
    Hp, Wp = frame or (H, W)
    image = np.zeros((F, 3, Hp, Wp), f32)
    xyz = np.zeros((F, 3, Hp, Wp), f32)
    mean = [f32(m / 255.0) for m in means]
    with np.errstate(all="ignore"):
        for f in range(F):
            fx, fy, px, py = (f32(cams[f][k]) for k in ("fx", "fy", "x_offset", "y_offset"))
            for y in range(H):
                for x in range(W):
                    for c in range(3):
                        image[f, c, y, x] = f32(color[f, y, x, c]) / f32(255) - mean[c]
                    d = depth[f, y, x]
                    if depth.dtype == np.uint16:
                        z = f32(d) / f32(depth_scale)
                    else:
                        z = f32(0) if np.isnan(d) else f32(d)
                    xyz[f, 0, y, x] = ((f32(x) - px) * z) / fx
                    xyz[f, 1, y, x] = ((f32(y) - py) * z) / fy
                    xyz[f, 2, y, x] = z
    return image, xyz


@pytest.mark.parametrize("kind", ["u16", "f32"])
@pytest.mark.parametrize("shape", [(2, 5, 7), (1, 33, 70)])
def test_host_ingest_is_the_definition_bitwise(shape, kind):
    F, H, W = shape
    color, depth = raw_frames(F, H, W, kind, seed=H)
    cams = cams_for(F, H, W)
    ref_image, ref_xyz = definition(color, depth, cams)
    assert np.signbit(ref_xyz).any() and (ref_xyz == 0).any()
    for wrap in (lambda a: a, torch.from_numpy):                  # numpy arrays and host tensors
        image, xyz = frames.ingest(wrap(color), wrap(depth), cams)
        assert image.dtype == xyz.dtype == torch.float32 and tuple(image.shape) == tuple(xyz.shape) == (F, 3, H, W)
        assert np.array_equal(bits(image), bits(ref_image)) and np.array_equal(bits(xyz), bits(ref_xyz))
    # one frame, one dict of intrinsics; image only
    image1, xyz1 = frames.ingest(color[0], depth[0], cams[0])
    assert np.array_equal(bits(image1), bits(ref_image[0])) and np.array_equal(bits(xyz1), bits(ref_xyz[0]))
    image0, none = frames.ingest(color, None, None)
    assert none is None and np.array_equal(bits(image0), bits(ref_image))
    # compute_xyz: the reference's (..., H, W, 3) layout, numpy in -> numpy out
    if kind == "f32":
        c = cams[0]
        pts = frames.compute_xyz(depth[0], c["fx"], c["fy"], c["x_offset"], c["y_offset"], H, W)
        assert isinstance(pts, np.ndarray) and pts.shape == (H, W, 3)
        assert np.array_equal(bits(pts.transpose(2, 0, 1)), bits(ref_xyz[0]))
        assert tuple(frames.compute_xyz(torch.from_numpy(depth), c["fx"], c["fy"], c["x_offset"], c["y_offset"]).shape) == (F, H, W, 3)


def test_uint16_bits_in_int16_are_the_same_depth():
    color, depth = raw_frames(2, 5, 7, "u16", seed=4)
    a = frames.ingest(color, depth, CAM)
    b = frames.ingest(torch.from_numpy(color), torch.from_numpy(depth).view(torch.int16), CAM)
    assert np.array_equal(bits(a[1]), bits(b[1])) and float(a[1][:, 2].max()) == np.float32(65535) / np.float32(1000)
    c = frames.ingest(color, depth, CAM, depth_scale=4000.0)
    assert np.array_equal(bits(c[1][:, 2]), bits(depth.astype(np.float32) / np.float32(4000)))


def test_make_sample_has_read_samples_keys_and_shapes():
    color, depth = raw_frames(1, 33, 70, "u16", seed=5)
    s = frames.make_sample(color[0], depth[0], CAM)
    assert set(s) == {"image_color", "depth"}
    for k in s:
        assert isinstance(s[k], torch.Tensor) and s[k].dtype == torch.float32 and tuple(s[k].shape) == (3, 33, 70)
    assert set(frames.make_sample(color[0], None, None)) == {"image_color"}
    with pytest.raises(ValueError):
        frames.make_sample(color, depth, CAM)


def test_rgb_order_is_bgr_of_the_flipped_input():
    color, depth = raw_frames(2, 5, 7, "f32", seed=6)
    a = frames.ingest(color, depth, CAM, order="bgr")
    b = frames.ingest(np.ascontiguousarray(color[..., ::-1]), depth, CAM, order="rgb")
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
    assert not np.array_equal(bits(a[0]), bits(frames.ingest(color, depth, CAM, order="rgb")[0]))
    with pytest.raises(ValueError):
        frames.ingest(color, depth, CAM, order="gbr")


def test_size_divisibility_pads_right_and_bottom_with_exact_zeros():
    color, depth = raw_frames(2, 33, 70, "u16", seed=7)
    image, xyz = frames.ingest(color, depth, CAM)
    pimage, pxyz = frames.ingest(color, depth, CAM, size_divisibility=32)
    assert tuple(pimage.shape) == tuple(pxyz.shape) == (2, 3, 64, 96)
    for p, t in ((pimage, image), (pxyz, xyz)):
        assert np.array_equal(bits(p[:, :, :33, :70]), bits(t))
        assert not bits(p[:, :, 33:, :]).any() and not bits(p[:, :, :, 70:]).any()          # +0.0 bit patterns
    assert tuple(frames.ingest(color[:, :32, :64], depth[:, :32, :64], CAM, size_divisibility=32)[0].shape) == (2, 3, 32, 64)


def test_image_lut_and_camera_table():
    lut = frames.image_lut()
    assert lut.shape == (3, 256) and lut.dtype == np.float32 and np.unique(lut).size == 768
    assert (np.diff(lut, axis=1) > 0).all()                                             # byte values in order
    assert lut[0, 0] > lut[1, 0] > lut[2, 0]                                            # B, G, R means ascending
    for c, m in enumerate(frames.PIXEL_MEANS):
        assert lut[c, 0] == -np.float32(m / 255.0) and lut[c, 255] == np.float32(1) - np.float32(m / 255.0)
    assert frames.PIXEL_MEANS == (102.9801, 115.9465, 122.7717)
    t = frames.camera_table(CAM, 3)
    assert t.dtype == torch.float32 and tuple(t.shape) == (3, 4)
    assert t[1].tolist() == [float(np.float32(CAM[k])) for k in ("fx", "fy", "x_offset", "y_offset")]
    many = cams_for(3, 5, 7)
    assert frames.camera_table(many, 3)[2, 0].item() == float(np.float32(many[2]["fx"]))
    with pytest.raises(ValueError):
        frames.camera_table(many, 2)


def test_host_path_reproduces_the_reference_fixture(golden):
    g = golden("frame_ingest")
    assert len(g["names"]) == 3
    for name in g["names"]:
        fx, fy, px, py = (float(v) for v in g[f"{name}_cam"])
        s = frames.make_sample(g[f"{name}_color"], g[f"{name}_depth"], {"fx": fx, "fy": fy, "x_offset": px, "y_offset": py})
        assert np.array_equal(bits(s["image_color"]), bits(g[f"{name}_image"])), name
        assert np.array_equal(bits(s["depth"]), bits(g[f"{name}_xyz"])), name
    assert np.isnan(g["f32_9x13_depth"]).any() and np.signbit(g["f32_9x13_xyz"]).any()


def test_raw_samples_through_the_batched_harness_on_the_host():
    """two_stage.test_batch_crop_nolabel takes raw samples: the predictor sees the tensors frames.make_sample builds; a mixed batch
    is refused."""
    from unseenobjectswithmeanshift_amd import two_stage as ts
    color, depth = raw_frames(2, 12, 16, "u16", seed=8)
    cams = cams_for(2, 12, 16)
    raw = [{"color": color[f], "depth_raw": torch.from_numpy(depth[f]), "camera_params": cams[f]} for f in range(2)]
    flt = [frames.make_sample(color[f], depth[f], cams[f]) for f in range(2)]
    seen = []

    class Pred:
        def batch_tensors(self, samples):
            seen.append((torch.stack([s["image"] for s in samples]), torch.stack([s["depth"] for s in samples])))
            n = len(samples)
            masks = torch.zeros((n, 1, 12, 16))
            masks[:, 0, 2:9, 3:11] = 1
            return torch.ones((n, 1)), torch.ones((n, 1), dtype=torch.int64), masks

    a = ts.test_batch_crop_nolabel(raw, Pred(), None, confident_score=0.5)
    b = ts.test_batch_crop_nolabel(flt, Pred(), None, confident_score=0.5)
    assert torch.equal(a[0], b[0]) and a[0].shape == (2, 12, 16)
    for k in range(2):
        assert np.array_equal(bits(seen[0][k]), bits(seen[1][k]))
    with pytest.raises(ValueError, match="mixed"):
        ts.test_batch_crop_nolabel([raw[0], flt[1]], Pred(), None)
    with pytest.raises(ValueError, match="one dtype and one place"):                  # uint16 and float32 depth in one batch
        ts.test_batch_crop_nolabel([raw[0], dict(raw[1], depth_raw=depth[1].astype(np.float32))], Pred(), None)
    with pytest.raises(ValueError, match="expected"):
        ts.test_batch_crop_nolabel([raw[0], dict(raw[1], depth_raw=depth[1][:5])], Pred(), None)
    # channel order and depth unit are passed through to frames.ingest
    rgb4 = [{"color": np.ascontiguousarray(color[f][..., ::-1]), "depth_raw": depth[f], "camera_params": cams[f]} for f in range(2)]
    ts.test_batch_crop_nolabel(rgb4, Pred(), None, confident_score=0.5, order="rgb", depth_scale=4000.0)
    want = frames.ingest(color, depth, cams, depth_scale=4000.0)
    assert np.array_equal(bits(seen[-1][0]), bits(want[0])) and np.array_equal(bits(seen[-1][1]), bits(want[1]))


def test_abi_version_and_symbol():
    with open(_lib.HEADER_PATH) as f:
        header_abi = int(re.search(r"#define\s+MSM_ABI_VERSION\s+(\d+)", f.read()).group(1))
    assert _lib.ABI_VERSION == header_abi >= 26
    assert "msm_ingest_frames" in _lib.declared_symbols() and "msm_ingest_frames" in _lib._SIGNATURES
