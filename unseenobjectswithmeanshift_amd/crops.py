"""Training crops for the second-stage model (TRAIN.SYN_CROP), for a batch, on the side the frames live on.

Own counterpart of the crop path of the reference's training loader, same names where it has them:

  pad_crop_resize   <- TableTopDataset.pad_crop_resize, lib/datasets/tabletop_dataset.py:234-300 (the identical methods of
                       tabletop_object.py:175 and pushing_dataset.py:215), called from __getitem__ :354-358
  draw_crop_params  <- its two random draws per frame (np.random.randint(1, K + 1), np.random.uniform(min, max padding)), made
                       on the host, outside the kernels
  crop_boxes / crop_resize   the batch forms; targets.training_batch(..., crop=params) composes them

The reference resizes with cv2, and cv2 is absent where this project is built, so nothing here is defined as "what cv2 returns".
The numpy host path of this module is the definition, and the HIP kernels (csrc/train_crop.hip) equal it bit for bit.  Every
step is integer arithmetic or float64 arithmetic on small half-integers (exact); the one exception is the product marked (*),
one IEEE double multiplication followed by a round-half-to-even.

C1 the object.  Per image, from the tables of targets.instance_targets for the call's ``background_ids`` (K_b distinct folded
   values, T_b instances) and the caller-drawn ``key`` (uint32): K = K_b - 1 -- the reference's np.max(label) of the dense map.
   K > 0: dense index idx = 1 + ((uint64(key) K) >> 32), instance row t = idx - (K_b - T_b); the region's tight box is that
   instance's.  K == 0 (background only, or one value everywhere): the region is the whole image, box (0, 0, W - 1, H - 1) --
   the reference's idx = 0 branch.  No pixel is reduced again: the boxes are in the table.
C2 the crop box (float64, the reference's arithmetic in its order).  cx = (x_min + x_max) / 2, cy likewise; x_delta = x_max -
   x_min, y_delta likewise; x_delta > y_delta: y_min, y_max = cy -+ x_delta / 2, otherwise (equality included) x_min, x_max =
   cx -+ y_delta / 2; side = x_max - x_min; padding = int(rint(side float64(p))) (*), ties to even as Python's round, 0 -> 25;
   x0 = max(trunc(x_min - padding), 0), x1 = min(trunc(x_max + padding), W - 1), y0 and y1 likewise with H; trunc rounds toward
   zero, as int() does.  H, W >= 2 is required.  Then x0 < x1 and y0 < y1 ALWAYS: the centre of the box lies inside the image
   (cx in [0, W - 1]) and padding >= 1, so x_min - padding <= cx - 1 and x_max + padding >= cx + 1; truncation and clamping keep
   x0 <= max(ceil(cx) - 1, 0) and x1 >= min(floor(cx) + 1, W - 1), which differ whenever W >= 2; y likewise.  The reference's
   redraw loop (`continue` at :281) therefore never runs and is not reproduced.  The status bit CROP_DEGENERATE exists for it
   anyway and is set together with the whole-image box.
C3 nearest (label ids, xyz).  With a source extent n and the output size S, s(d) = (d n) // S; output pixel (dy, dx) reads
   source (y0 + s_y(dy), x0 + s_x(dx)).  Labels keep their dtype and their RAW ids: the reference's second process_label /
   process_label_to_annos pass (:357-358) is invariant under the monotone raw -> dense relabelling, so
   instance_targets(raw_crop, background_ids=<the same>) yields what the reference builds.  xyz is float32, copied bit for bit;
   zeros (invalid depth) stay zeros.
C4 bilinear (uint8 colour), half-pixel centres, integers only.  num = (2 d + 1) n - S, s = num // (2 S) (floor), frac = num -
   2 S s, w1 = (frac 2048 + S) // (2 S), w0 = 2048 - w1; s < 0: s = 0, w1 = 0; s >= n - 1: s = n - 1, w1 = 0; the second tap is
   min(s + 1, n - 1).  Per channel out = ((a wx0 + b wx1) wy0 + (c wx0 + d wx1) wy1 + 2^21) >> 22; the sum stays below 2^31.
   It follows that n == S reproduces the source, n == 2 S is (a + b + c + d + 2) >> 2, a constant image stays constant, and
   |out - float64 bilinear| <= 0.5 + 255 2 2^-12 < 0.625 (the final rounding plus the weight quantisation in x and in y).
   Modelled on OpenCV's 8-bit fixed-point scheme; equality with cv2 is neither claimed nor tested.

A box row (CROP_BOX_ROW int32 words): x0, y0, x1, y1 inclusive, the chosen dense index, the chosen raw id (-1: none), the
padding, status bits.  CROP_BAD_ROW: the padding fraction is not in [0, 16] -- the row then is the whole image with padding 0.
CROP_BAD_BOX: crop_resize found a (caller-supplied) box that does not satisfy 0 <= x0 < x1 <= W - 1, 0 <= y0 < y1 <= H - 1; that
image's three outputs are zeros.  CropParams.check() raises them.  A wrong box or table never makes a kernel read or write
outside its buffers.

Like frames, targets and augment, the functions follow their data: device tensors go through the HIP kernels (ops.crop_boxes,
ops.train_crop: two launches for a whole batch), host tensors and numpy arrays through the definitions in numpy.  There is no
fallback on a device tensor.  Not included: equality with cv2, random numbers inside kernels, RandomFlip / ResizeShortestEdge of
the detectron2 mapper (every shipped yaml has RANDOM_FLIP "none", and 480 is the frames' own short edge).
"""
import numpy as np
import torch

from . import targets as _tg

CROP_BOX_ROW = 8                     # MSM_CROP_BOX_ROW
COL_X0, COL_Y0, COL_X1, COL_Y1, COL_INDEX, COL_ID, COL_PADDING, COL_STATUS = range(CROP_BOX_ROW)
CROP_DEGENERATE, CROP_BAD_BOX, CROP_BAD_ROW = 1, 2, 4      # MSM_CROP_* status bits
MAX_SIZE = 1024                      # MSM_CROP_MAX_SIZE
MAX_PADDING = 16.0                   # the largest padding fraction a row may carry
ZERO_PADDING = 25                    # tabletop_dataset.py:271-272
WEIGHT_ONE = 2048                    # C4: weights in 1 / 2048
_STATUS_TEXT = {CROP_DEGENERATE: "its crop box was degenerate (the whole image was used)",
                CROP_BAD_BOX: "its box does not lie inside the image (the crop is zeros)",
                CROP_BAD_ROW: f"its padding fraction is not in [0, {MAX_PADDING:g}] or its table row contradicts itself"}


def _is_device(x):
    return isinstance(x, torch.Tensor) and x.is_cuda


def _host(x):
    return x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


class CropParams:
    """The random parameters of one batch of crops, a plain container:

      table    (B,2) int32 words: the uint32 key that picks the object and the bits of the float32 padding fraction -- a device
               tensor, a host tensor or a numpy array; where it lives decides which path crop_boxes takes
      keys / fractions   the two columns of a host table as uint32 / float32 (host_table: the numpy table a device table was
               uploaded from, when known)
      status   the status column of the boxes the last crop_boxes / crop_resize call wrote; check() reads it.

    ``to(device)`` uploads (one pinned non-blocking copy)."""

    def __init__(self, table, host_table=None):
        if table.ndim != 2 or table.shape[1] != 2 or table.dtype not in (np.int32, torch.int32):
            raise ValueError(f"table must be (B, 2) int32, got {tuple(table.shape)} {table.dtype}")
        self.table = table
        self.host_table = _host(table) if host_table is None and not _is_device(table) else host_table
        self.status = None

    def __len__(self):
        return self.table.shape[0]

    @property
    def is_device(self):
        return _is_device(self.table)

    @property
    def keys(self):
        return None if self.host_table is None else np.ascontiguousarray(self.host_table[:, 0]).view(np.uint32)

    @property
    def fractions(self):
        return None if self.host_table is None else np.ascontiguousarray(self.host_table[:, 1]).view(np.float32)

    def to(self, device):
        dev = torch.device(device)
        if dev.type == "cpu":
            if self.is_device:
                raise ValueError("CropParams.to: device parameters stay on the device")
            return self
        host = torch.from_numpy(np.ascontiguousarray(_host(self.table))).pin_memory()
        return CropParams(host.to(dev, non_blocking=True), host_table=self.host_table)

    def check(self):
        """Raise ValueError for the rows the last calls could not carry out (see the module).  Waits for the GPU."""
        if self.status is None:
            return self
        st = self.status.cpu().numpy() if isinstance(self.status, torch.Tensor) else np.asarray(self.status)
        for b, bits in enumerate(st.tolist()):
            for bit, text in _STATUS_TEXT.items():
                if bits & bit:
                    raise ValueError(f"crop: image {b}: {text}")
        return self


def pack_crop_table(keys, fractions):
    """(B,2) int32 table from explicit numbers: keys (uint32 values) and padding fractions (stored as float32)."""
    k = np.asarray(keys, dtype=np.uint64).reshape(-1)
    p = np.asarray(fractions, dtype=np.float32).reshape(-1)
    if k.shape != p.shape or (k >= 2 ** 32).any():
        raise ValueError("pack_crop_table: one uint32 key and one padding fraction per image")
    t = np.empty((k.size, 2), dtype=np.int32)
    t[:, 0] = k.astype(np.uint32).view(np.int32)
    t[:, 1] = p.view(np.int32)
    return t


def draw_crop_params(B, *, rng=None, generator=None, min_padding=0.05, max_padding=0.5, device="cpu"):
    """The random parameters of B crops, drawn as the reference draws them per sample: a uniform uint32 key (the object: C1) and
    a padding fraction uniform in [min_padding, max_padding) (cfg.TRAIN.min / max_padding_percentage).  ``rng`` (a
    numpy.random.Generator) draws them on the host; without it a host torch ``generator`` does (default: torch's global one).
    They go to ``device`` in one non-blocking copy from pinned memory; the call never waits for the GPU."""
    if not 0 <= float(min_padding) <= float(max_padding) <= MAX_PADDING:
        raise ValueError(f"draw_crop_params: 0 <= min_padding <= max_padding <= {MAX_PADDING:g} expected")
    if rng is not None:
        keys = rng.integers(0, 2 ** 32, size=B, dtype=np.uint64)
        frac = rng.uniform(min_padding, max_padding, size=B)
    else:
        keys = torch.randint(0, 2 ** 32, (B,), dtype=torch.int64, generator=generator).numpy().astype(np.uint64)
        frac = min_padding + (max_padding - min_padding) * torch.rand((B,), dtype=torch.float64, generator=generator).numpy()
    table = pack_crop_table(keys, frac)
    dev = torch.device(device)
    if dev.type == "cpu":
        return CropParams(table)
    pinned = torch.empty((B, 2), dtype=torch.int32, pin_memory=True)
    pinned.numpy()[:] = table
    dtab = torch.empty((B, 2), dtype=torch.int32, device=dev)
    dtab.copy_(pinned, non_blocking=True)
    return CropParams(dtab, host_table=table)


# ----------------------------------------------------------------------------------------------------------------------------
# the definitions in numpy (host tensors / arrays)
def choose_object_host(Kb, Tb, key):
    """C1: (dense index, instance row) for an image with Kb distinct folded values and Tb instances; (0, None): the whole image."""
    K = int(Kb) - 1
    if K <= 0:
        return 0, None
    idx = 1 + ((int(key) * K) >> 32)
    return idx, idx - (int(Kb) - int(Tb))


def square_pad_clamp_host(box, p, H, W):
    """C2: the tight box (x_min, y_min, x_max, y_max) and the float32 fraction p -> (x0, y0, x1, y1, padding); Python floats are
    float64, round() is round-half-to-even, int() truncates toward zero."""
    x_min, y_min, x_max, y_max = (float(v) for v in box)
    cx, cy = (x_min + x_max) / 2, (y_min + y_max) / 2
    x_delta, y_delta = x_max - x_min, y_max - y_min
    if x_delta > y_delta:
        y_min, y_max = cy - x_delta / 2, cy + x_delta / 2
    else:
        x_min, x_max = cx - y_delta / 2, cx + y_delta / 2
    side = x_max - x_min
    padding = int(round(side * float(np.float32(p))))
    if padding == 0:
        padding = ZERO_PADDING
    return (max(int(x_min - padding), 0), max(int(y_min - padding), 0), min(int(x_max + padding), W - 1),
            min(int(y_max + padding), H - 1), padding)


def _crop_boxes_host(raw, table, background_ids):
    B, H, W = raw.shape
    lab, _ = _tg._fold_host(raw, background_ids)
    keys, frac = table[:, 0].copy().view(np.uint32), table[:, 1].copy().view(np.float32)
    out = np.zeros((B, CROP_BOX_ROW), dtype=np.int32)
    for b in range(B):
        p = frac[b]
        if not (p >= 0 and p <= MAX_PADDING):
            out[b] = (0, 0, W - 1, H - 1, 0, -1, 0, CROP_BAD_ROW)
            continue
        present, ids, _ = _tg._image_tables_host(lab[b])
        idx, t = choose_object_host(len(present), len(ids), keys[b])
        box, chosen = (0, 0, W - 1, H - 1), -1
        if t is not None:
            chosen = int(ids[t])
            box = _tg._box_host(lab[b] == chosen)
        x0, y0, x1, y1, padding = square_pad_clamp_host(box, p, H, W)
        status = 0
        if not (x0 < x1 and y0 < y1):
            x0, y0, x1, y1, status = 0, 0, W - 1, H - 1, CROP_DEGENERATE
        out[b] = (x0, y0, x1, y1, idx, chosen, padding, status)
    return out


def nearest_index(n, S):
    """C3: the source index of every output index along an axis, (S,) int64."""
    return (np.arange(S, dtype=np.int64) * int(n)) // int(S)


def bilinear_taps(n, S):
    """C4 along one axis: (first tap, second tap, w0, w1), four (S,) int64 arrays."""
    n, S = int(n), int(S)
    d = np.arange(S, dtype=np.int64)
    num = (2 * d + 1) * n - S
    s = num // (2 * S)
    frac = num - 2 * S * s
    w1 = (frac * WEIGHT_ONE + S) // (2 * S)
    edge = (s < 0) | (s >= n - 1)
    s = np.clip(s, 0, n - 1)
    w1 = np.where(edge, 0, w1)
    return s, np.minimum(s + 1, n - 1), WEIGHT_ONE - w1, w1


def resize_bilinear_host(img, S):
    """C4 on one (ny, nx, C) uint8 image -> (S, S, C) uint8."""
    ny, nx = img.shape[:2]
    ya, yb, wy0, wy1 = bilinear_taps(ny, S)
    xa, xb, wx0, wx1 = bilinear_taps(nx, S)
    v = img.astype(np.int64)
    top = v[ya][:, xa] * wx0[None, :, None] + v[ya][:, xb] * wx1[None, :, None]
    bot = v[yb][:, xa] * wx0[None, :, None] + v[yb][:, xb] * wx1[None, :, None]
    return ((top * wy0[:, None, None] + bot * wy1[:, None, None] + (1 << 21)) >> 22).astype(np.uint8)


def resize_nearest_host(a, S):
    """C3 on one (..., ny, nx) array -> (..., S, S), values untouched."""
    return a[..., nearest_index(a.shape[-2], S), :][..., nearest_index(a.shape[-1], S)]


def _box_ok(row, H, W):
    x0, y0, x1, y1 = (int(v) for v in row[:4])
    return 0 <= x0 < x1 <= W - 1 and 0 <= y0 < y1 <= H - 1


def _crop_resize_host(color, raw, xyz, boxes, S, Sp):
    B, H, W = raw.shape
    color_out = np.zeros((B, S, S, 3), dtype=np.uint8)
    raw_out = np.zeros((B, S, S), dtype=raw.dtype)
    xyz_out = None if xyz is None else np.zeros((B, 3, Sp, Sp), dtype=np.float32)
    for b in range(B):
        if not _box_ok(boxes[b], H, W):
            boxes[b, COL_STATUS] |= CROP_BAD_BOX
            continue
        x0, y0, x1, y1 = (int(v) for v in boxes[b, :4])
        color_out[b] = resize_bilinear_host(color[b, y0:y1 + 1, x0:x1 + 1], S)
        raw_out[b] = resize_nearest_host(raw[b, y0:y1 + 1, x0:x1 + 1], S)
        if xyz is not None:
            xyz_out[b, :, :S, :S] = resize_nearest_host(xyz[b, :, y0:y1 + 1, x0:x1 + 1], S)
    return color_out, raw_out, xyz_out


# ----------------------------------------------------------------------------------------------------------------------------
def _check_frames(color, raw, who):
    if raw.ndim != 3 or color.ndim != 4 or color.shape[-1] != 3 or tuple(color.shape[:3]) != tuple(raw.shape):
        raise ValueError(f"{who}: colour {tuple(color.shape)} must be (B, H, W, 3) and raw {tuple(raw.shape)} (B, H, W)")
    if color.dtype not in (torch.uint8, np.uint8):
        raise ValueError(f"{who}: colour frames are uint8, got {color.dtype}")


def _check_size(H, W, who):
    if H < 2 or W < 2:
        raise ValueError(f"{who}: frames of at least 2 x 2 pixels are needed, got {H} x {W}")


def crop_boxes(raw, params, background_ids=_tg.BACKGROUND_IDS):
    """C1 + C2 for a batch (B,H,W) of instance label images (uint8 or an integer type) under ``params`` (CropParams) -> boxes
    (B, CROP_BOX_ROW) int32 where the images live (a tensor for a tensor, an array for an array).  ``background_ids``: the ids
    folded to 0, as instance_targets takes them.  On the device: the tables of ops.target_tables and one launch; no wait.
    ``params.status`` becomes the status column of the result."""
    if raw.ndim != 3 or raw.shape[0] != len(params):
        raise ValueError(f"crop_boxes: raw {tuple(raw.shape)} must be (B, H, W) with B = {len(params)}")
    B, H, W = raw.shape
    _check_size(H, W, "crop_boxes")
    if _is_device(raw) != params.is_device:
        raise ValueError("crop_boxes: label images and parameters must live on the same side")
    if _is_device(raw):
        from . import ops
        rawd = _tg._raw_device(raw)
        tables = ops.target_tables(rawd, _tg._device_background(raw.device, background_ids))
        boxes = ops.crop_boxes(tables, params.table, (H, W))
    else:
        r = _host(raw)
        _tg._check_host_ints(r, "crop_boxes")
        res = _crop_boxes_host(r, np.ascontiguousarray(_host(params.table)), background_ids)
        boxes = torch.from_numpy(res) if isinstance(raw, torch.Tensor) else res
    params.status = boxes[:, COL_STATUS]
    return boxes


def crop_resize(color, raw, xyz, boxes, size, size_divisibility=1):
    """C3 + C4 for a batch: colour (B,H,W,3) uint8, raw (B,H,W) integer label images, xyz (B,3,Hp,Wp) float32 (the output of
    frames.ingest; None: none) cropped to each image's row of ``boxes`` (B, CROP_BOX_ROW) int32 -- crop_boxes', or a loader's
    own: only x0, y0, x1, y1 are read -- and resized to ``size`` = S -> (colour (B,S,S,3) uint8, raw (B,S,S) in raw's type (int32
    on the device unless uint8), xyz (B,3,Sp,Sp) or None) with Sp = S rounded up to ``size_divisibility``, zeros beyond S.  A box
    outside the image gives zeros and the CROP_BAD_BOX bit in its status word; the boxes are updated in place."""
    _check_frames(color, raw, "crop_resize")
    B, H, W = raw.shape
    _check_size(H, W, "crop_resize")
    S = int(size)
    Sp = _tg._round_up(S, int(size_divisibility))
    if not 1 <= S <= MAX_SIZE:
        raise ValueError(f"crop_resize: size must lie in [1, {MAX_SIZE}], got {S}")
    where = {_is_device(t) for t in (color, raw, xyz, boxes) if t is not None}
    if len(where) != 1:
        raise ValueError("crop_resize: frames, label images, xyz and boxes must live on the same side")
    if tuple(boxes.shape) != (B, CROP_BOX_ROW) or boxes.dtype not in (np.int32, torch.int32):
        raise ValueError(f"crop_resize: boxes {tuple(boxes.shape)} {boxes.dtype} must be ({B}, {CROP_BOX_ROW}) int32")
    if xyz is not None and (xyz.ndim != 4 or tuple(xyz.shape[:2]) != (B, 3) or xyz.shape[2] < H or xyz.shape[3] < W
                            or xyz.dtype not in (torch.float32, np.float32)):
        raise ValueError(f"crop_resize: xyz {tuple(xyz.shape)} {xyz.dtype} must be float32 ({B}, 3, Hp >= {H}, Wp >= {W})")
    if where.pop():
        from . import ops
        if not boxes.is_contiguous():
            raise ValueError("crop_resize: a contiguous box table (its status words are updated in place)")
        return ops.train_crop(color.contiguous(), _tg._raw_device(raw), None if xyz is None else xyz.contiguous(), boxes, S, frame=Sp)
    r = _host(raw)
    _tg._check_host_ints(r, "crop_resize")
    res = _crop_resize_host(_host(color), r, None if xyz is None else _host(xyz), _host(boxes), S, Sp)
    if isinstance(color, torch.Tensor):
        return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)) for a in res)
    return res


# ----------------------------------------------------------------------------------------------------------------------------
# the reference's method by name: one frame
def pad_crop_resize(img, label, depth, *, size=224, params=None, rng=None, background_ids=()):
    """pad_crop_resize: one (H,W,3) uint8 image, its (H,W) label image and its ordered point cloud (H,W,3) float32 (or None)
    cropped around one randomly chosen object and resized to ``size`` -> (img_crop (S,S,3), label_crop (S,S), depth_crop (S,S,3)
    or None).  The reference hands in the label map process_label made dense, in which every value above 0 is an object
    (``background_ids=()``); a raw label image works the same way with the ids to fold.  ``params``: a CropParams of one row;
    default drawn from ``rng`` with the reference's padding range."""
    if img.ndim != 3 or label.ndim != 2:
        raise ValueError("pad_crop_resize takes one frame (H, W, 3) and its label image (H, W); batches go through crop_boxes / crop_resize")
    device = _is_device(img)
    if params is None:
        params = draw_crop_params(1, rng=np.random.default_rng() if rng is None else rng, device=img.device if device else "cpu")
    xyz = None
    if depth is not None:
        xyz = depth.permute(2, 0, 1)[None].contiguous() if isinstance(depth, torch.Tensor) else np.ascontiguousarray(np.transpose(depth, (2, 0, 1))[None])
    boxes = crop_boxes(label[None], params, background_ids=background_ids)
    c, r, z = crop_resize(img[None], label[None], xyz, boxes, size)
    params.check()
    if isinstance(r, torch.Tensor) and isinstance(label, torch.Tensor) and r.dtype != label.dtype:
        r = r.to(label.dtype)
    if z is not None:
        z = z[0].permute(1, 2, 0).contiguous() if isinstance(z, torch.Tensor) else np.ascontiguousarray(np.transpose(z[0], (1, 2, 0)))
    return c[0], r[0], z
