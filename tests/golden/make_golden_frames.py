"""Golden fixture of the frame ingest: run the REFERENCE's read_sample / compute_xyz (tools/test_image_with_ms_transformer.py:106-147,
build_matrix_of_indices lib/utils/mask.py:41-46) on small seeded frames and store the inputs and what they return.

Run in the build container only:   python tests/golden/make_golden_frames.py   ->  tests/golden/frame_ingest.npz

The reference functions are executed from their source (_ref_import.ref_functions) in a namespace that binds
  cv2     a stand-in whose imread hands back the seeded arrays of this file by name (read_sample reads its two images with
          cv2.imread; decoding image files is not what the fixture is about),
  util_   build_matrix_of_indices of the reference's lib/utils/mask.py,
  np / torch.
Cases with uint16 depth go through read_sample whole (image and xyz).  The float32-depth case is the ROS listener's path
(ros/test_images_segmentation_transformer.py:159-173): the same image arithmetic (taken from read_sample), NaN depth set to 0
as in run_network:170, then the reference's compute_xyz.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ref_import as R  # noqa: E402

# (name, H, W, seed, depth kind, camera_params) -- intrinsics of a 640x480 RGB-D camera, not representable in float32
CASES = [
    ("u16_5x7", 5, 7, 1, "u16", {"fx": 616.3653, "fy": 616.2043, "x_offset": 3.4837, "y_offset": 2.1759}),
    ("u16_12x20", 12, 20, 2, "u16", {"fx": 570.3422, "fy": 570.3422, "x_offset": 9.5, "y_offset": 5.7301}),
    ("f32_9x13", 9, 13, 3, "f32", {"fx": 1066.778, "fy": 1067.487, "x_offset": 6.2049, "y_offset": 4.0717}),
]


def make_inputs(H, W, seed, kind):
    rng = np.random.default_rng(seed)
    color = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    color.reshape(-1)[:4] = [0, 255, 1, 254]
    if kind == "u16":
        depth = rng.integers(200, 4000, size=(H, W)).astype(np.uint16)
        depth.reshape(-1)[:3] = [0, 65535, 1]
    else:
        depth = rng.uniform(0.2, 4.0, size=(H, W)).astype(np.float32)
        depth.reshape(-1)[:5] = [np.nan, 0.0, -1.25, np.nan, -0.0]
    return color, depth


def namespace(files):
    cv2 = types.ModuleType("cv2")
    cv2.IMREAD_ANYDEPTH = 2
    cv2.imread = lambda name, flags=None: files[name].copy()
    mask_ns = R.ref_functions("lib/utils/mask.py", ["build_matrix_of_indices"], {"np": np})
    util_ = types.SimpleNamespace(build_matrix_of_indices=mask_ns["build_matrix_of_indices"])
    ns = {"np": np, "torch": torch, "cv2": cv2, "util_": util_}
    return R.ref_functions("tools/test_image_with_ms_transformer.py", ["compute_xyz", "read_sample"], ns)


def main():
    files = {}
    ns = namespace(files)
    out = {"names": np.array([c[0] for c in CASES])}
    for name, H, W, seed, kind, cam in CASES:
        color, depth = make_inputs(H, W, seed, kind)
        files["color"] = color
        files["depth"] = depth if kind == "u16" else np.zeros((H, W), np.uint16)
        sample = ns["read_sample"]("color", "depth", cam)
        image = sample["image_color"].numpy()
        if kind == "u16":
            xyz = sample["depth"].numpy()
        else:
            d = depth.copy()
            d[np.isnan(d)] = 0
            xyz = ns["compute_xyz"](d, cam["fx"], cam["fy"], cam["x_offset"], cam["y_offset"], H, W).transpose(2, 0, 1)
        assert image.dtype == np.float32 and xyz.dtype == np.float32 and image.shape == xyz.shape == (3, H, W)
        out[f"{name}_color"] = color
        out[f"{name}_depth"] = depth
        out[f"{name}_cam"] = np.array([cam["fx"], cam["fy"], cam["x_offset"], cam["y_offset"]], np.float64)
        out[f"{name}_image"] = np.ascontiguousarray(image)
        out[f"{name}_xyz"] = np.ascontiguousarray(xyz)
        print(name, image.shape, float(np.abs(image).max()), float(np.nanmax(np.abs(xyz))), flush=True)
    path = os.path.join(HERE, "frame_ingest.npz")
    np.savez_compressed(path, **out)
    print(f"frame_ingest: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
