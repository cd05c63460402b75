"""Shared cases and float64 oracles of the training-crop tests (test_train_crop_cpu.py, test_gpu_train_crop.py).

The oracles restate the definitions C2 and C4 of unseenobjectswithmeanshift_amd/crops.py independently of that module: C2 with
fractions.Fraction for everything but the one rounded product, C4's reference as the float64 half-pixel-centre bilinear
interpolation with clamped source coordinates.  Nothing here imports crops.py except to name the columns of a box row."""
import functools
import math
from fractions import Fraction

import numpy as np


# ------------------------------------------------------------------------------------------------------------------------ C2
def c2_oracle(box, p, H, W):
    """The tight box (x_min, y_min, x_max, y_max) of integers and the fraction p (any float; it is rounded to float32 first) ->
    (x0, y0, x1, y1, padding).  Exact rationals, except side * p: ONE float64 product, rounded half to even."""
    x_min, y_min, x_max, y_max = (Fraction(int(v)) for v in box)
    cx, cy = (x_min + x_max) / 2, (y_min + y_max) / 2
    xd, yd = x_max - x_min, y_max - y_min
    if xd > yd:
        y_min, y_max = cy - xd / 2, cy + xd / 2
    else:
        x_min, x_max = cx - yd / 2, cx + yd / 2
    side = x_max - x_min
    prod = float(side) * float(np.float32(p))                   # the float64 product (side is a small integer: exact)
    lo = math.floor(prod)
    rest = Fraction(prod) - lo                                  # exact: a float is a rational
    padding = lo + (1 if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and lo % 2 == 1) else 0)
    if padding == 0:
        padding = 25

    def trunc(q):
        return math.floor(q) if q >= 0 else -math.floor(-q)

    return (max(trunc(x_min - padding), 0), max(trunc(y_min - padding), 0), min(trunc(x_max + padding), W - 1),
            min(trunc(y_max + padding), H - 1), padding)


# ------------------------------------------------------------------------------------------------------------------------ C4
def bilinear_f64(img, S):
    """(ny, nx, C) uint8 -> (S, S, C) float64: bilinear interpolation at half-pixel centres, src = (d + 0.5) n / S - 0.5 clamped
    to [0, n - 1], BEFORE rounding."""
    ny, nx = img.shape[:2]

    def axis(n):
        src = np.clip((np.arange(S, dtype=np.float64) + 0.5) * n / S - 0.5, 0.0, n - 1.0)
        i0 = np.minimum(np.floor(src).astype(np.int64), n - 1)
        return i0, np.minimum(i0 + 1, n - 1), src - i0

    ya, yb, fy = axis(ny)
    xa, xb, fx = axis(nx)
    v = img.astype(np.float64)
    fx, fy = fx[None, :, None], fy[:, None, None]
    top = v[ya][:, xa] * (1 - fx) + v[ya][:, xb] * fx
    bot = v[yb][:, xa] * (1 - fx) + v[yb][:, xb] * fx
    return top * (1 - fy) + bot * fy


# ------------------------------------------------------------------------------------------------------------------------ labels
@functools.lru_cache(maxsize=None)
def label_images():
    """{name: (H, W) uint8 label image}, all 12 x 20, ids as the tabletop data has them (0 background, 1 table, objects above):
    three objects on a table; the same without any background pixel (every pixel an object); background only; table only (folds
    to background); one object id everywhere; two objects and no background."""
    H, W = 12, 20
    out = {}
    a = np.zeros((H, W), np.uint8)
    a[7:, :] = 1
    a[1:4, 2:9] = 4          # wide
    a[2:11, 12:14] = 7       # tall
    a[9, 5] = 9              # a single pixel
    out["three"] = a
    b = a.copy()
    b[b <= 1] = 12           # what was background becomes one more object: no background pixel is left
    out["no_background"] = b
    out["background_only"] = np.zeros((H, W), np.uint8)
    out["table_only"] = np.ones((H, W), np.uint8)
    out["one_value"] = np.full((H, W), 5, np.uint8)
    c = np.full((H, W), 3, np.uint8)
    c[:, 11:] = 8
    out["two_no_background"] = c
    for v in out.values():
        v.setflags(write=False)
    return out


def label_batch():
    """(names, (B,12,20) uint8): label_images() as one batch, in a fixed order."""
    imgs = label_images()
    names = sorted(imgs)
    return names, np.stack([imgs[n] for n in names])


def crop_keys(B):
    """B uint32 keys that reach the first, the last and some middle object: 0, 2^32 - 1, then a fixed scramble."""
    return np.array(([0, 2 ** 32 - 1] + [(i * 2654435761 + 12345) % 2 ** 32 for i in range(B)])[:B], dtype=np.uint64)


# ------------------------------------------------------------------------------------------------------------------------ frames
def frame_case(B, H, W, seed, *, label_dtype=np.uint8, Hp=None, Wp=None, with_xyz=True):
    """Random frames for the crop kernel: colour (B,H,W,3) uint8 (random, with a binary image 0 / 255 as image 0), raw (B,H,W)
    of ``label_dtype`` with ids in [0, 40), xyz (B,3,Hp,Wp) float32 with a tenth of the points zero and a non-zero margin beyond
    (H, W) that a correct crop never reads."""
    rng = np.random.default_rng(seed)
    color = rng.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)
    color[0] = np.where(rng.random((H, W, 3)) < 0.5, 0, 255)
    raw = rng.integers(0, 40, size=(B, H, W)).astype(label_dtype)
    xyz = None
    if with_xyz:
        Hp, Wp = Hp or H, Wp or W
        xyz = rng.normal(size=(B, 3, Hp, Wp)).astype(np.float32)
        xyz[:, :, :H, :W][np.broadcast_to(rng.random((B, 1, H, W)) < 0.1, (B, 3, H, W))] = 0
        xyz[:, :, H:, :] = 777.0
        xyz[:, :, :, W:] = 777.0
    return color, raw, xyz


def box_rows(rows):
    """(B,8) int32 box table from (x0, y0, x1, y1) tuples: what a loader that chooses its own boxes hands to crop_resize."""
    t = np.zeros((len(rows), 8), dtype=np.int32)
    t[:, :4] = np.asarray(rows, dtype=np.int64).reshape(len(rows), 4)
    t[:, 5] = -1
    return t


def scene(B, H, W, seed=0):
    """A synthetic table scene: colour (B,H,W,3) uint8, depth (B,H,W) uint16 millimetres with holes, raw (B,H,W) uint8 with a
    table (1) and three boxes (ids 3, 5, 7) whose position depends on the image; the third is small and sits in a corner, so a
    crop around another object drops it."""
    rng = np.random.default_rng(seed)
    color = rng.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)
    depth = rng.integers(400, 2000, size=(B, H, W)).astype(np.uint16)
    depth[rng.random((B, H, W)) < 0.1] = 0
    raw = np.zeros((B, H, W), np.uint8)
    raw[:, 2 * H // 3:, :] = 1
    for b in range(B):
        raw[b, 6 + 2 * b:6 + 2 * b + H // 4, W // 8 + 3 * b:W // 8 + 3 * b + W // 4] = 3
        raw[b, H // 3:H // 3 + H // 3, W // 2 + 2 * b:W // 2 + 2 * b + W // 6] = 5
        raw[b, H - 4:H - 1, W - 5:W - 1] = 7
    return color, depth, raw


CAM = {"fx": 570.3, "fy": 570.3, "x_offset": 45.0, "y_offset": 30.0}
