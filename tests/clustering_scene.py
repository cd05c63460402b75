"""A planted scene for the clustering two-stage harness tests (test_clustering_two_stage_cpu.py, test_gpu_clustering_two_stage.py):
96 x 128, a tilted table plane and three objects, one of them with a hole in its depth so that the 0.8 depth filter removes it;
per-object colours plus noise of 1e-2; xyz from pinhole intrinsics.  The stand-in ``network`` / ``network_crop`` are
normalize(W . image) with two fixed 64 x 3 matrices: two different "checkpoints", and per pixel, so that a frame's embeddings do
not depend on the batch it is in."""
import numpy as np
import torch
import torch.nn.functional as F

H, W = 96, 128


def planted_ids():
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    ids = np.zeros((H, W), dtype=np.int64)                                  # 0 = table
    ids[((yy - 30) / 14) ** 2 + ((xx - 30) / 18) ** 2 <= 1] = 1
    ids[(yy >= 50) & (yy < 82) & (xx >= 60) & (xx < 86)] = 2
    ids[((yy - 28) / 12) ** 2 + ((xx - 98) / 14) ** 2 <= 1] = 3           # the object with the hole in its depth
    return ids


def scene(seed=7):
    """-> (sample {"image_color" (1,3,H,W), "depth" (1,3,H,W)}, w_net (64,3), w_crop (64,3), ids (H,W))."""
    g = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    ids = planted_ids()
    # mean-subtracted colours: four directions far apart, so that two objects' embeddings are farther apart than the vMF kernel
    # at kappa = 20 reaches
    colours = np.array([[0.4, 0.4, 0.4], [0.4, -0.4, -0.4], [-0.4, 0.4, -0.4], [-0.4, -0.4, 0.4]], dtype=np.float32)
    image = colours[ids].transpose(2, 0, 1) + g.normal(0, 1e-2, (3, H, W)).astype(np.float32)
    z = (0.9 + 0.002 * yy - 0.04 * (ids > 0)).astype(np.float32)            # objects stand on the table
    z[(ids == 3) & (xx > 94)] = 0                                           # > 20 % of object 3 without depth
    fx = fy = 120.0
    xyz = np.stack([(xx - W / 2.0) * z / fx, (yy - H / 2.0) * z / fy, z]).astype(np.float32)
    w = g.normal(0, 1, (2, 64, 3)).astype(np.float32)
    sample = {"image_color": torch.from_numpy(image.astype(np.float32))[None], "depth": torch.from_numpy(xyz)[None]}
    return sample, torch.from_numpy(w[0]), torch.from_numpy(w[1]), torch.from_numpy(ids)


def network_from(w):
    """normalize(W . image) as three broadcast multiply-adds per pixel."""
    def net(image, label, depth):
        wd = w.to(image.device)
        f = wd[None, :, 0, None, None] * image[:, 0:1] + wd[None, :, 1, None, None] * image[:, 1:2] + wd[None, :, 2, None, None] * image[:, 2:3]
        return F.normalize(f, p=2, dim=1)
    return net


def flipped(sample):
    """The frame mirrored left-right (the x coordinate of xyz keeps its values: only z > 0 matters to the harness)."""
    return {k: torch.flip(v, dims=[-1]).contiguous() for k, v in sample.items()}


def mirror_index(i, width):
    """Flat pixel index of the mirrored position in a map ``width`` wide."""
    return (i // width) * width + (width - 1 - i % width)


def iou(a, b):
    a, b = a.bool(), b.bool()
    return float((a & b).sum()) / max(1.0, float((a | b).sum()))
