"""The random augmentations of the reference's training loader, for a batch, on the side the frames live on.

Own counterpart of what TableTopDataset.__getitem__ does to every training sample, same names where it has them:

  chromatic_transform      <- lib/utils/blob.py:74-99 (TRAIN.CHROMATIC, tabletop_dataset.py:364-365)
  add_noise                <- lib/utils/blob.py:102-129 (TRAIN.ADD_NOISE, tabletop_dataset.py:366-367)
  add_noise_to_depth       <- lib/utils/augmentation.py:58-71
  dropout_random_ellipses  <- lib/utils/augmentation.py:92-126
  add_noise_to_xyz         <- lib/utils/augmentation.py:73-90         (the three of process_depth, tabletop_dataset.py:161-181)
  TABLETOP_NOISE_PARAMS    <- data_loading_params, tabletop_dataset.py:37-47
  draw_params              <- every random draw of the above, made on the host, outside the kernels
  augment_color / augment_depth / add_xyz_noise_   the batch forms; targets.training_batch(..., augment=params) composes them

The reference's functions are cv2's (cvtColor, filter2D, ellipse, resize), and cv2 is absent where this project is built, so
nothing here is defined as "what cv2 returns".  Every value is a pure function of the inputs and of the random parameters the
caller hands in (AugmentParams); the definitions below are float32 / integer steps in a fixed order -- one rounding per written
operation, no multiply-add, no reciprocal, round to nearest -- the numpy host path of this module is the definition, and the
HIP kernels (csrc/augment.hip) equal it bit for bit.

D1 chromatic (uint8 BGR -> uint8 BGR, per pixel), OpenCV's documented 8-bit BGR <-> HLS conversion:
  forward   b, g, r = float32(v) / 255;  vmax, vmin = max, min;  sum = vmax + vmin;  diff = vmax - vmin;  l = sum * 0.5
            diff <= FLT_EPSILON: h = s = 0, else
              s = diff / sum  if l < 0.5  else  diff / ((2 - vmax) - vmin)
              k = 60 / diff;  h = (g - b) k  if vmax == r,  else (b - r) k + 120  if vmax == g,  else (r - g) k + 240
              h < 0: h += 360;  h = h * 0.5
            H = rint(h), L = rint(l * 255), S = rint(s * 255) (ties to even); H = 180 can occur and is kept
  shift     H' = trunc(mod(float32(H) + d_h, 180)) with numpy's float32 mod (the sign of the divisor; a tiny negative sum gives
            exactly 180); L' = trunc(clip(float32(L) + d_l, 0, 255)), S' the same with d_s: the reference's .astype('uint8')
  back      l = float32(L') / 255, s = float32(S') / 255;  s == 0: b = g = r = l, else
              p2 = l (1 + s)  if l <= 0.5  else  (l + s) - l s;   p1 = 2 l - p2;   d = p2 - p1
              h = (float32(H') 6) / 180, h >= 6: h -= 6;  sector = floor(h), f = h - sector
              tab = [p2, p1, p1 + d (1 - f), p1 + d f];  (b, g, r) = tab[[1,3,0], [1,0,2], [3,0,1], [0,2,1], [0,1,3], [2,1,0]][sector]
            out = clip(rint(x 255), 0, 255)
D2 Gaussian pixel noise (after D1): out_c = trunc(clip(float32(v_c) + sigma n[y][x], 0, 255)), the same n for the three channels.
D3 motion blur (after D1, instead of D2): a box of ``size`` taps along x or along y, borders reflect-101, exact integers:
  out = (2 sum + size) // (2 size) (size is odd: no tie).  The blurred extent must exceed size // 2.
D4 depth (uint16 or float32 -> float32 metres): z = float32(d) / depth_scale (float32: z = d, NaN -> 0, as frames.ingest), then
  z = z m.  The valid pixels are z > 0 in row-major order, n of them; ellipse i has its centre (cx, cy) at valid pixel number
  (uint64(key_i) n) >> 32 -- all centres from the valid set before any ellipse is applied, n = 0: no dropout.  A pixel becomes 0
  if for any ellipse, in float32:  dx = x - cx, dy = y - cy, u = dx cos + dy sin, v = dy cos - dx sin, a = max(rx, 0.5),
  b = max(ry, 0.5), (u u) / (a a) + (v v) / (b b) <= 1.  This is the analytic ellipse; cv2 fills a polygon approximation that
  differs from it in boundary pixels, and neither is tested against the other.
D5 point-cloud noise, in place on (B,3,Hp,Wp): where xyz[2] > 0 inside the H x W corner, xyz[c] = xyz[c] + scale up(gp[c]);
  up is the separable bicubic (a = -0.75, half-pixel centres src = (dst + 0.5) (h / H) - 0.5, indices clamped to the border,
  the weights float32 from bicubic_taps): r_j = ((w0 v0 + w1 v1) + w2 v2) + w3 v3 along x for the four rows, then the same along
  y.  In float64 this is F.interpolate(mode="bicubic", align_corners=False).

A row of the table that asks for none of D1-D3 copies its image bit for bit.  A row that cannot be carried out -- a blur size
outside BLUR_SIZES, more than ELLIPSE_MAX ellipses, a value that is not finite -- is SKIPPED (the image or depth map is only
converted) and recorded as a status bit, on both paths; AugmentParams.check() raises it.  A wrong table never makes a kernel
read or write outside its buffers.

Like frames and targets, the functions follow their data: device tensors go through the HIP kernels (ops.augment_color,
ops.augment_depth, ops.xyz_noise_), host tensors and numpy arrays through the definitions in numpy.  There is no fallback on a
device tensor.  pad_crop_resize / TRAIN.SYN_CROP lives in crops.py; with targets.training_batch(..., crop=) the colour half
of an AugmentParams applies to the S x S crops and is drawn at that size.  Not included: the label augmentations of
augmentation.py:195-509 (no MSMFormer config uses them), random numbers inside kernels, equality with cv2.
"""
import numpy as np
import torch

from . import frames

TABLETOP_NOISE_PARAMS = {          # tabletop_dataset.py:37-47
    "gamma_shape": 1000.0, "gamma_scale": 0.001,
    "gaussian_scale": 0.005, "gp_rescale_factor": 4,
    "ellipse_dropout_mean": 10, "ellipse_gamma_shape": 5.0, "ellipse_gamma_scale": 1.0,
}
ELLIPSE_MAX = 32                   # ellipses per image; MSM_AUGMENT_ELLIPSE_MAX
BLUR_SIZES = (3, 5, 7, 9, 11, 15)  # blob.py:119
NOISE_LEVEL = 0.1                  # add_noise's ``level``

# the per-image table, int32 words (floats by their bits); MSM_AUGMENT_TABLE_ROW and the MSM_AUGMENT_* columns of msm_hip.h
TABLE_ROW = 176
COL_FLAGS, COL_BLUR_SIZE, COL_BLUR_HORIZONTAL, COL_D_H, COL_D_L, COL_D_S, COL_SIGMA, COL_MULTIPLIER, COL_COUNT = range(9)
COL_ELLIPSES = 16                  # then ELLIPSE_MAX x (rx, ry, cos, sin float32, key uint32)
ELLIPSE_WORDS = 5
FLAG_CHROMATIC, FLAG_GAUSSIAN, FLAG_BLUR, FLAG_DEPTH = 1, 2, 4, 8
# status bits, columns (colour, depth) of the (B,4) status
BAD_ROW, BAD_COUNT, BAD_ELLIPSE, BAD_CENTRE = 1, 2, 4, 8
STATUS_COLOR, STATUS_DEPTH = 0, 1
_STATUS_TEXT = {BAD_ROW: "a value of its row is not finite, out of range or not a known mode (blur size, flags)",
                BAD_COUNT: f"its ellipse count is outside [0, {ELLIPSE_MAX}]",
                BAD_ELLIPSE: "an ellipse has a radius outside [0, 65536] or a (cos, sin) that is not a unit vector",
                BAD_CENTRE: "an ellipse record has its centre outside the image"}

_F = np.float32
_EPS = np.finfo(np.float32).eps
_SECTOR = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])


# ----------------------------------------------------------------------------------------------------------------------------
# the table
def pack_table(B, *, chromatic=False, d_h=0.0, d_l=0.0, d_s=0.0, gaussian=False, sigma=0.0, blur_size=0, blur_horizontal=True,
               depth=False, multiplier=1.0, ellipses=None):
    """(B, TABLE_ROW) int32 table from explicit numbers: every keyword a scalar (for all images) or B values.  ``blur_size`` 0:
    no blur.  ``ellipses``: per image a list of (rx, ry, angle in degrees, key) -- cos and sin are rounded from float64 here.
    Every scalar is stored as float32 or int32, and the stored value is the parameter."""
    t = np.zeros((B, TABLE_ROW), dtype=np.int32)
    tf = t.view(np.float32)

    def per(v, dtype):
        return np.broadcast_to(np.asarray(v, dtype=dtype), (B,))

    blur = per(blur_size, np.int64)
    t[:, COL_FLAGS] = (per(chromatic, bool) * FLAG_CHROMATIC + per(gaussian, bool) * FLAG_GAUSSIAN + (blur != 0) * FLAG_BLUR
                       + per(depth, bool) * FLAG_DEPTH)
    t[:, COL_BLUR_SIZE] = blur
    t[:, COL_BLUR_HORIZONTAL] = per(blur_horizontal, bool)
    for col, v in ((COL_D_H, d_h), (COL_D_L, d_l), (COL_D_S, d_s), (COL_SIGMA, sigma), (COL_MULTIPLIER, multiplier)):
        tf[:, col] = per(v, np.float32)
    if ellipses is not None:
        if len(ellipses) != B:
            raise ValueError(f"ellipses: {len(ellipses)} lists for {B} images")
        for b, es in enumerate(ellipses):
            t[b, COL_COUNT] = len(es)
            for i, (rx, ry, angle, key) in enumerate(es[:ELLIPSE_MAX]):
                o = COL_ELLIPSES + ELLIPSE_WORDS * i
                rad = np.deg2rad(np.float64(angle))
                tf[b, o:o + 4] = (rx, ry, np.cos(rad), np.sin(rad))
                t[b, o + 4] = np.uint32(key).view(np.int32)
    return t


def unpack_table(table):
    """The fields of a host table by name (views where possible): flags, blur_size, blur_horizontal, d_h, d_l, d_s, sigma,
    multiplier, count, and rx, ry, cos, sin (B,ELLIPSE_MAX) float32, key (B,ELLIPSE_MAX) uint32."""
    t = np.ascontiguousarray(table, dtype=np.int32)
    tf = t.view(np.float32)
    e = t[:, COL_ELLIPSES:COL_ELLIPSES + ELLIPSE_WORDS * ELLIPSE_MAX].reshape(-1, ELLIPSE_MAX, ELLIPSE_WORDS)
    ef = e.view(np.float32)
    return {"flags": t[:, COL_FLAGS], "blur_size": t[:, COL_BLUR_SIZE], "blur_horizontal": t[:, COL_BLUR_HORIZONTAL],
            "d_h": tf[:, COL_D_H], "d_l": tf[:, COL_D_L], "d_s": tf[:, COL_D_S], "sigma": tf[:, COL_SIGMA],
            "multiplier": tf[:, COL_MULTIPLIER], "count": t[:, COL_COUNT],
            "rx": ef[..., 0], "ry": ef[..., 1], "cos": ef[..., 2], "sin": ef[..., 3], "key": e[..., 4].view(np.uint32)}


def _is_device(x):
    return isinstance(x, torch.Tensor) and x.is_cuda


def _host(x):
    return x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


class AugmentParams:
    """The random parameters of one batch, a plain container:

      table        (B, TABLE_ROW) int32: the per-image scalars (pack_table / unpack_table) -- a device tensor, a host tensor or
                   a numpy array; where it lives decides which path augment_color / augment_depth take
      pixel_noise  (B,H,W) float32 standard normal or None (D2);   gp_noise (B,3,h,w) float32 standard normal or None (D5)
      gaussian_scale  what D5 multiplies the upsampled field by (the reference's 0.005; NOT multiplied into gp_noise)
      host_table   the numpy table a device table was uploaded from, when known: lets the device path raise for a blur that
                   does not fit the image instead of recording it
      status       (B,4) int32 written by the last augment_color (column 0) / augment_depth (column 1) call; check() reads it.

    ``to(device)`` uploads (one pinned non-blocking copy for the table)."""

    def __init__(self, table, pixel_noise=None, gp_noise=None, gaussian_scale=TABLETOP_NOISE_PARAMS["gaussian_scale"],
                 host_table=None):
        if table.ndim != 2 or table.shape[1] != TABLE_ROW or table.dtype not in (np.int32, torch.int32):
            raise ValueError(f"table must be (B, {TABLE_ROW}) int32, got {tuple(table.shape)} {table.dtype}")
        self.table, self.pixel_noise, self.gp_noise = table, pixel_noise, gp_noise
        self.gaussian_scale = float(gaussian_scale)
        self.host_table = _host(table) if host_table is None and not _is_device(table) else host_table
        self.status = None

    def __len__(self):
        return self.table.shape[0]

    @property
    def is_device(self):
        return _is_device(self.table)

    def to(self, device):
        dev = torch.device(device)
        if dev.type == "cpu":
            if self.is_device:
                raise ValueError("AugmentParams.to: device parameters stay on the device")
            return self
        host = torch.from_numpy(np.ascontiguousarray(_host(self.table))).pin_memory()
        up = [None if t is None else torch.as_tensor(t).to(dev) for t in (self.pixel_noise, self.gp_noise)]
        return AugmentParams(host.to(dev, non_blocking=True), up[0], up[1], self.gaussian_scale, host_table=self.host_table)

    def _status(self, dev=None):
        if self.status is None:
            B = len(self)
            self.status = np.zeros((B, 4), np.int32) if dev is None else torch.zeros((B, 4), dtype=torch.int32, device=dev)
        return self.status

    def check(self):
        """Raise ValueError for the rows the last calls skipped (see the module).  Waits for the GPU."""
        if self.status is None:
            return self
        st = self.status.cpu().numpy() if isinstance(self.status, torch.Tensor) else self.status
        for b in range(st.shape[0]):
            for col, who in ((STATUS_COLOR, "augment_color"), (STATUS_DEPTH, "augment_depth")):
                for bit, text in _STATUS_TEXT.items():
                    if st[b, col] & bit:
                        raise ValueError(f"{who}: image {b} was skipped: {text}")
        return self


def draw_params(B, H, W, *, rng, device="cpu", generator=None, chromatic=True, add_noise=False, depth=True,
                noise_params=TABLETOP_NOISE_PARAMS):
    """The random parameters of B frames of H x W, drawn as the reference draws them per sample (the table in DESIGN 5y):
    ``rng`` (a numpy.random.Generator) draws the per-image scalars on the host, ``generator`` (a torch generator on ``device``,
    default the device's own) the two noise fields with torch.randn where they live.  ``pixel_noise`` is drawn only if some image
    took the Gaussian branch, ``gp_noise`` (B,3,int(H/4),int(W/4)) only with ``depth``.  The ellipse count is poisson(10) clamped
    to ELLIPSE_MAX = 32: at mean 10 a larger draw has a probability below 1e-7.  Everything per-image goes to the device in one
    non-blocking copy from pinned memory; the call never waits for the GPU."""
    p = noise_params
    rows = []
    for _ in range(B):
        f = {}
        if chromatic and rng.random() > 0.1:                            # tabletop_dataset.py:364, blob.py:80-84
            f.update(chromatic=True, d_h=(rng.random() - 0.5) * 0.1 * 180, d_l=(rng.random() - 0.5) * 0.2 * 256,
                     d_s=(rng.random() - 0.5) * 0.2 * 256)
        if add_noise and rng.random() > 0.1:                            # :366, blob.py:105-126
            if rng.random() < 0.9:
                level = rng.uniform(0, NOISE_LEVEL)
                f.update(gaussian=True, sigma=rng.random() * level * 256)
            else:
                size = BLUR_SIZES[int(rng.integers(len(BLUR_SIZES)))]
                f.update(blur_size=size, blur_horizontal=bool(rng.random() < 0.5))
        es = []
        if depth:                                                       # augmentation.py:68, 102-112
            f.update(depth=True, multiplier=rng.gamma(p["gamma_shape"], p["gamma_scale"]))
            n = min(int(rng.poisson(p["ellipse_dropout_mean"])), ELLIPSE_MAX)
            keys = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64)
            rx = np.round(rng.gamma(p["ellipse_gamma_shape"], p["ellipse_gamma_scale"], size=n))
            ry = np.round(rng.gamma(p["ellipse_gamma_shape"], p["ellipse_gamma_scale"], size=n))
            ang = rng.integers(0, 360, size=n)
            es = [(rx[i], ry[i], ang[i], keys[i]) for i in range(n)]
        rows.append(pack_table(1, ellipses=[es], **f))
    table = np.concatenate(rows) if rows else np.zeros((0, TABLE_ROW), np.int32)
    dev = torch.device(device)
    need_pixel = bool((table[:, COL_FLAGS] & FLAG_GAUSSIAN).any())
    h, w = int(H / p["gp_rescale_factor"]), int(W / p["gp_rescale_factor"])
    gdev = dev if generator is None else generator.device

    def randn(shape):
        return torch.randn(shape, dtype=torch.float32, generator=generator, device=gdev).to(dev)

    pixel = randn((B, H, W)) if need_pixel else None
    gp = randn((B, 3, h, w)) if depth else None
    if dev.type == "cpu":
        return AugmentParams(table, None if pixel is None else pixel.numpy(), None if gp is None else gp.numpy(), p["gaussian_scale"])
    pinned = torch.empty((B, TABLE_ROW), dtype=torch.int32, pin_memory=True)
    pinned.numpy()[:] = table
    dtab = torch.empty((B, TABLE_ROW), dtype=torch.int32, device=dev)
    dtab.copy_(pinned, non_blocking=True)
    return AugmentParams(dtab, pixel, gp, p["gaussian_scale"], host_table=table)


# ----------------------------------------------------------------------------------------------------------------------------
# the definitions in numpy (host tensors / arrays)
def bgr_to_hls_host(bgr):
    """D1 forward: uint8 (...,3) BGR -> float32 (...,3) holding the integers H, L, S."""
    f255 = _F(255)
    bf, gf, rf = (bgr[..., c].astype(np.float32) / f255 for c in range(3))
    vmax, vmin = np.maximum(np.maximum(bf, gf), rf), np.minimum(np.minimum(bf, gf), rf)
    sm, diff = vmax + vmin, vmax - vmin
    lum = sm * _F(0.5)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(lum < _F(0.5), diff / sm, diff / ((_F(2) - vmax) - vmin))
        k = _F(60) / diff
        h = np.where(vmax == rf, (gf - bf) * k, np.where(vmax == gf, (bf - rf) * k + _F(120), (rf - gf) * k + _F(240)))
        h = np.where(h < 0, h + _F(360), h) * _F(0.5)
    flat = diff <= _EPS
    h, s = np.where(flat, _F(0), h), np.where(flat, _F(0), s)
    return np.stack([np.rint(h), np.rint(lum * f255), np.rint(s * f255)], axis=-1).astype(np.float32)


def shift_hls_host(hls, d_h, d_l, d_s):
    """D1 shift: float32 integers H, L, S -> H', L', S' (float32 integers) under the float32 parameters."""
    hn = np.trunc(np.mod(hls[..., 0] + _F(d_h), _F(180)))
    ln = np.trunc(np.clip(hls[..., 1] + _F(d_l), _F(0), _F(255)))
    sn = np.trunc(np.clip(hls[..., 2] + _F(d_s), _F(0), _F(255)))
    return np.stack([hn, ln, sn], axis=-1).astype(np.float32)


def hls_to_bgr_host(hls):
    """D1 back: float32 integers H', L', S' (...,3) -> uint8 BGR."""
    hh, lum, s = hls[..., 0], hls[..., 1] / _F(255), hls[..., 2] / _F(255)
    p2 = np.where(lum <= _F(0.5), lum * (_F(1) + s), (lum + s) - lum * s)
    p1 = _F(2) * lum - p2
    d = p2 - p1
    h = (hh * _F(6)) / _F(180)
    h = np.where(h >= _F(6), h - _F(6), h)
    sector = np.clip(np.floor(h), 0, 5)
    f = h - sector
    tab = np.stack([p2, p1, p1 + d * (_F(1) - f), p1 + d * f], axis=-1)
    pick = _SECTOR[sector.astype(np.int64)]                              # (...,3) table positions for b, g, r
    val = np.take_along_axis(tab, pick, axis=-1)
    val = np.where((s == 0)[..., None], lum[..., None], val)
    return np.clip(np.rint(val * _F(255)), 0, 255).astype(np.uint8)


def _reflect101(idx, n):
    idx = np.where(idx < 0, -idx, idx)
    return np.where(idx >= n, 2 * n - 2 - idx, idx)


def _blur_host(img, size, horizontal):
    """D3 on one (H,W,3) uint8 image."""
    axis = 1 if horizontal else 0
    n, half = img.shape[axis], size // 2
    acc = np.zeros(img.shape, dtype=np.int64)
    for k in range(-half, half + 1):
        acc += np.take(img, _reflect101(np.arange(n) + k, n), axis=axis)
    return ((2 * acc + size) // (2 * size)).astype(np.uint8)


def _color_row_ok(f, b, H, W, have_noise):
    """The validity rule of a colour row, as the kernel applies it."""
    flags = int(f["flags"][b])
    if flags & ~15 or (flags & FLAG_GAUSSIAN and flags & FLAG_BLUR):
        return False
    if flags & FLAG_CHROMATIC and not (abs(f["d_h"][b]) <= 180 and abs(f["d_l"][b]) <= 512 and abs(f["d_s"][b]) <= 512):
        return False
    if flags & FLAG_GAUSSIAN and not (abs(f["sigma"][b]) <= 65536 and have_noise):
        return False
    if flags & FLAG_BLUR:
        size, hz = int(f["blur_size"][b]), int(f["blur_horizontal"][b])
        if size not in BLUR_SIZES or hz not in (0, 1) or (W if hz else H) <= size // 2:
            return False
    return True


def _augment_color_host(color, f, noise):
    B, H, W, _ = color.shape
    out = color.copy()
    status = np.zeros((B,), np.int32)
    for b in range(B):
        if not _color_row_ok(f, b, H, W, noise is not None):
            status[b] = BAD_ROW
            continue
        flags = int(f["flags"][b])
        img = out[b]
        if flags & FLAG_CHROMATIC:
            img = hls_to_bgr_host(shift_hls_host(bgr_to_hls_host(img), f["d_h"][b], f["d_l"][b], f["d_s"][b]))
        if flags & FLAG_GAUSSIAN:
            t = f["sigma"][b] * noise[b].astype(np.float32, copy=False)
            img = np.trunc(np.clip(img.astype(np.float32) + t[..., None], _F(0), _F(255))).astype(np.uint8)
        elif flags & FLAG_BLUR:
            img = _blur_host(img, int(f["blur_size"][b]), bool(f["blur_horizontal"][b]))
        out[b] = img
    return out, status


def ellipse_centres_host(z, keys):
    """Definition D4.2: z (H,W), keys uint32 -> (cx, cy) int64 arrays; no valid pixel: empty arrays."""
    valid = np.flatnonzero(z.reshape(-1) > 0)
    if valid.size == 0:
        return np.zeros((0,), np.int64), np.zeros((0,), np.int64)
    idx = valid[(keys.astype(np.uint64) * np.uint64(valid.size)) >> np.uint64(32)]
    return idx % z.shape[1], idx // z.shape[1]


def _ellipse_ok(rx, ry, c, s):
    with np.errstate(invalid="ignore", over="ignore"):
        return bool(rx >= 0 and rx <= 65536 and ry >= 0 and ry <= 65536 and abs((c * c + s * s) - _F(1)) <= _F(1e-3))


def _dropout_host(z, cx, cy, rx, ry, c, s):
    """Definition D4.3 for one ellipse, in place."""
    H, W = z.shape
    dx = (np.arange(W, dtype=np.int64) - cx).astype(np.float32)[None, :]
    dy = (np.arange(H, dtype=np.int64) - cy).astype(np.float32)[:, None]
    u, v = dx * c + dy * s, dy * c - dx * s
    a, b = max(rx, _F(0.5)), max(ry, _F(0.5))
    z[(u * u) / (a * a) + (v * v) / (b * b) <= _F(1)] = 0


def _augment_depth_host(depth, f, depth_scale):
    z = np.array(frames._depth_metres_host(depth, depth_scale), dtype=np.float32)
    B = z.shape[0]
    status = np.zeros((B,), np.int32)
    for b in range(B):
        if not int(f["flags"][b]) & FLAG_DEPTH:
            continue
        m, count = f["multiplier"][b], int(f["count"][b])
        if not np.isfinite(m):
            status[b] |= BAD_ROW
        if count < 0 or count > ELLIPSE_MAX:
            status[b] |= BAD_COUNT
        if status[b]:
            continue
        z[b] = z[b] * m
        cx, cy = ellipse_centres_host(z[b], f["key"][b, :count])
        for i in range(len(cx)):
            e = [f[k][b, i] for k in ("rx", "ry", "cos", "sin")]
            if not _ellipse_ok(*e):
                status[b] |= BAD_ELLIPSE
                continue
            _dropout_host(z[b], int(cx[i]), int(cy[i]), *e)
        if len(cx) == 0:                                                 # no valid pixel: the ellipses are still judged
            for i in range(count):
                if not _ellipse_ok(*[f[k][b, i] for k in ("rx", "ry", "cos", "sin")]):
                    status[b] |= BAD_ELLIPSE
    return z, status


def bicubic_taps(n_in, n_out):
    """The four clamped source indices (n_out,4) int32 and float32 weights (n_out,4) of D5's upsampling along one axis: half-pixel
    centres, a = -0.75, every step float32.  For n_out = 4 n_in the weights are four constants per phase."""
    a = _F(-0.75)
    src = (np.arange(n_out, dtype=np.float32) + _F(0.5)) * (_F(n_in) / _F(n_out)) - _F(0.5)
    i0 = np.floor(src)
    t = src - i0

    def near(x):        # |x| <= 1
        return ((a + _F(2)) * x - (a + _F(3))) * x * x + _F(1)

    def far(x):         # 1 < |x| < 2
        return ((a * x - _F(5) * a) * x + _F(8) * a) * x - _F(4) * a

    w = np.stack([far(t + _F(1)), near(t), near(_F(1) - t), far(_F(2) - t)], axis=-1).astype(np.float32)
    idx = np.clip(i0.astype(np.int64)[:, None] + np.arange(-1, 3), 0, n_in - 1).astype(np.int32)
    return idx, w


def _sum4(w, v):
    """((w0 v0 + w1 v1) + w2 v2) + w3 v3 over the last axis, float32, left to right."""
    return ((w[..., 0] * v[..., 0] + w[..., 1] * v[..., 1]) + w[..., 2] * v[..., 2]) + w[..., 3] * v[..., 3]


def upsample_bicubic_host(gp, H, W):
    """(...,h,w) float32 -> (...,H,W): D5's ``up``."""
    iy, wy = bicubic_taps(gp.shape[-2], H)
    ix, wx = bicubic_taps(gp.shape[-1], W)
    rows = _sum4(wx, gp[..., :, ix])                                     # (...,h,W)
    return _sum4(wy[:, None, :], np.moveaxis(rows[..., iy, :], -2, -1))  # (...,H,W)


def _xyz_noise_host(xyz, gp, scale, H, W):
    up = upsample_bicubic_host(gp.astype(np.float32, copy=False), H, W)
    corner = xyz[:, :, :H, :W]
    where = corner[:, 2:3] > 0
    corner[...] = np.where(where, corner + _F(scale) * up, corner)
    return xyz


# ----------------------------------------------------------------------------------------------------------------------------
_TAPS_DEVICE = {}


def _device_taps(dev, h, w, H, W):
    """D5's tap table on the device: (H + W, 8) int32, rows of four indices and four weight bit patterns, y rows first."""
    key = (str(dev), h, w, H, W)
    if key not in _TAPS_DEVICE:
        rows = []
        for n_in, n_out in ((h, H), (w, W)):
            idx, wts = bicubic_taps(n_in, n_out)
            rows.append(np.concatenate([idx, wts.view(np.int32)], axis=1))
        host = torch.from_numpy(np.concatenate(rows)).pin_memory()
        _TAPS_DEVICE[key] = host.to(dev, non_blocking=True)
    return _TAPS_DEVICE[key]


def _batch(x, ndim, who):
    single = x.ndim == ndim - 1
    x = x[None] if single else x
    if x.ndim != ndim:
        raise ValueError(f"{who}: {tuple(x.shape)} is neither one frame nor a batch")
    return x, single


def _check_blur_fits(params, H, W):
    if params.host_table is None:
        return
    f = unpack_table(params.host_table)
    for b in range(len(params)):
        if int(f["flags"][b]) & FLAG_BLUR and int(f["blur_size"][b]) in BLUR_SIZES:
            size, hz = int(f["blur_size"][b]), int(f["blur_horizontal"][b])
            if (W if hz else H) <= size // 2:
                raise ValueError(f"augment_color: a blur of {size} taps along {'x' if hz else 'y'} needs more than {size // 2} "
                                 f"pixels there, image {b} is {H} x {W}")


def augment_color(color, params):
    """D1-D3 on a batch (B,H,W,3) (or one frame (H,W,3)) of uint8 BGR frames under ``params`` -> a new array of the same kind."""
    x, single = _batch(color, 4, "augment_color")
    if x.shape[-1] != 3 or x.dtype not in (torch.uint8, np.uint8) or x.shape[0] != len(params):
        raise ValueError(f"augment_color: {tuple(x.shape)} {x.dtype} must be uint8 (B, H, W, 3) with B = {len(params)}")
    B, H, W, _ = x.shape
    if params.pixel_noise is not None and tuple(params.pixel_noise.shape) != (B, H, W):
        raise ValueError(f"augment_color: pixel_noise {tuple(params.pixel_noise.shape)} must be {(B, H, W)}")
    _check_blur_fits(params, H, W)
    if _is_device(x) != params.is_device:
        raise ValueError("augment_color: frames and parameters must live on the same side")
    if _is_device(x):
        from . import ops
        out = ops.augment_color(x.contiguous(), params.table, params.pixel_noise, params._status(x.device))
    else:
        res, st = _augment_color_host(np.ascontiguousarray(_host(x)), unpack_table(_host(params.table)),
                                      None if params.pixel_noise is None else _host(params.pixel_noise))
        params._status()[:, STATUS_COLOR] = st
        out = torch.from_numpy(res) if isinstance(color, torch.Tensor) else res
    return out[0] if single else out


def augment_depth(depth, params, depth_scale=1000.0):
    """D4 on a batch (B,H,W) (or one map (H,W)) of uint16 millimetres / ``depth_scale`` or float32 metres -> float32 metres."""
    x, single = _batch(depth, 3, "augment_depth")
    if x.shape[0] != len(params):
        raise ValueError(f"augment_depth: {x.shape[0]} maps for {len(params)} parameter rows")
    if _is_device(x) != params.is_device:
        raise ValueError("augment_depth: depth and parameters must live on the same side")
    if _is_device(x):
        from . import ops
        out = ops.augment_depth(x.contiguous(), params.table, params._status(x.device), depth_div=float(depth_scale))[0]
    else:
        res, st = _augment_depth_host(_host(x), unpack_table(_host(params.table)), depth_scale)
        params._status()[:, STATUS_DEPTH] = st
        out = torch.from_numpy(res) if isinstance(depth, torch.Tensor) else res
    return out[0] if single else out


def add_xyz_noise_(xyz, params, size=None):
    """D5 in place on the (B,3,Hp,Wp) float32 output of frames.ingest; ``size`` = (H, W), the valid corner (default the whole
    map).  Returns xyz."""
    if xyz.ndim != 4 or xyz.shape[1] != 3 or xyz.shape[0] != len(params) or xyz.dtype not in (torch.float32, np.float32):
        raise ValueError(f"add_xyz_noise_: xyz {tuple(xyz.shape)} {xyz.dtype} must be float32 (B, 3, Hp, Wp) with B = {len(params)}")
    gp = params.gp_noise
    if gp is None:
        raise ValueError("add_xyz_noise_: the parameters hold no gp_noise field")
    H, W = tuple(xyz.shape[2:]) if size is None else (int(size[0]), int(size[1]))
    if not (0 < H <= xyz.shape[2] and 0 < W <= xyz.shape[3]):
        raise ValueError(f"add_xyz_noise_: size {(H, W)} does not lie inside {tuple(xyz.shape[2:])}")
    if gp.ndim != 4 or tuple(gp.shape[:2]) != (xyz.shape[0], 3) or gp.shape[2] < 1 or gp.shape[3] < 1:
        raise ValueError(f"add_xyz_noise_: gp_noise {tuple(gp.shape)} must be (B, 3, h, w)")
    if _is_device(xyz) != _is_device(gp):
        raise ValueError("add_xyz_noise_: xyz and gp_noise must live on the same side")
    if _is_device(xyz):
        from . import ops
        if not xyz.is_contiguous():
            raise ValueError("add_xyz_noise_: a contiguous xyz tensor is updated in place")
        ops.xyz_noise_(xyz, gp.contiguous(), _device_taps(xyz.device, gp.shape[2], gp.shape[3], H, W), params.gaussian_scale, (H, W))
    else:
        _xyz_noise_host(_host(xyz), _host(gp), params.gaussian_scale, H, W)
    return xyz


# ----------------------------------------------------------------------------------------------------------------------------
# the reference's functions by name: one frame, thin forms over the batch functions
def _frame_params(x, table, **kw):
    p = AugmentParams(table, **kw)
    return p.to(x.device) if _is_device(x) else p


def _rng(rng):
    return np.random.default_rng() if rng is None else rng


def chromatic_transform(im, label=None, d_h=None, d_s=None, d_l=None, *, rng=None):
    """chromatic_transform: one (H,W,3) uint8 BGR image shifted in HLS space (D1); shifts not given are drawn from ``rng`` as the
    reference draws them.  With ``label`` the pixels where label > 0 keep their input value."""
    rng = _rng(rng)
    d_h = (rng.random() - 0.5) * 0.1 * 180 if d_h is None else d_h
    d_l = (rng.random() - 0.5) * 0.2 * 256 if d_l is None else d_l
    d_s = (rng.random() - 0.5) * 0.2 * 256 if d_s is None else d_s
    p = _frame_params(im, pack_table(1, chromatic=True, d_h=float(d_h), d_l=float(d_l), d_s=float(d_s)))
    out = augment_color(im, p)
    p.check()
    if label is not None:
        keep = (label > 0)[..., None]
        out = torch.where(keep, im, out) if isinstance(im, torch.Tensor) else np.where(keep, im, out)
    return out


def add_noise(image, level=NOISE_LEVEL, *, rng=None, generator=None):
    """add_noise: Gaussian pixel noise (D2, probability 0.9) or a motion blur (D3) on one (H,W,3) uint8 image."""
    rng = _rng(rng)
    H, W = image.shape[:2]
    if rng.random() < 0.9:
        sigma = rng.random() * rng.uniform(0, level) * 256
        dev = image.device if _is_device(image) else torch.device("cpu")
        gdev = dev if generator is None else generator.device
        noise = torch.randn((1, H, W), dtype=torch.float32, generator=generator, device=gdev).to(dev)
        p = _frame_params(image, pack_table(1, gaussian=True, sigma=sigma), pixel_noise=noise if _is_device(image) else noise.numpy())
    else:
        size = BLUR_SIZES[int(rng.integers(len(BLUR_SIZES)))]
        p = _frame_params(image, pack_table(1, blur_size=size, blur_horizontal=bool(rng.random() < 0.5)))
    out = augment_color(image, p)
    p.check()
    return out


def add_noise_to_depth(depth_img, noise_params=TABLETOP_NOISE_PARAMS, *, rng=None):
    """add_noise_to_depth: one (H,W) float32 depth map in metres times a gamma variate (D4.1)."""
    m = _rng(rng).gamma(noise_params["gamma_shape"], noise_params["gamma_scale"])
    p = _frame_params(depth_img, pack_table(1, depth=True, multiplier=m))
    return augment_depth(depth_img, p, depth_scale=1.0)


def dropout_random_ellipses(depth_img, noise_params=TABLETOP_NOISE_PARAMS, *, rng=None):
    """dropout_random_ellipses: about ten random ellipses punched out of one (H,W) float32 depth map (D4.2-3)."""
    rng = _rng(rng)
    n = min(int(rng.poisson(noise_params["ellipse_dropout_mean"])), ELLIPSE_MAX)
    keys = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64)
    rx = np.round(rng.gamma(noise_params["ellipse_gamma_shape"], noise_params["ellipse_gamma_scale"], size=n))
    ry = np.round(rng.gamma(noise_params["ellipse_gamma_shape"], noise_params["ellipse_gamma_scale"], size=n))
    ang = rng.integers(0, 360, size=n)
    p = _frame_params(depth_img, pack_table(1, depth=True, ellipses=[[(rx[i], ry[i], ang[i], keys[i]) for i in range(n)]]))
    return augment_depth(depth_img, p, depth_scale=1.0)


def add_noise_to_xyz(xyz_img, depth_img=None, noise_params=TABLETOP_NOISE_PARAMS, *, generator=None):
    """add_noise_to_xyz: one ordered point cloud (H,W,3) float32 plus upsampled Gaussian noise where its z is positive (D5; the
    reference masks with depth_img > 0, which is the cloud's own z).  Returns a new array of the same kind."""
    H, W = xyz_img.shape[:2]
    h, w = int(H / noise_params["gp_rescale_factor"]), int(W / noise_params["gp_rescale_factor"])
    dev = xyz_img.device if _is_device(xyz_img) else torch.device("cpu")
    gdev = dev if generator is None else generator.device
    gp = torch.randn((1, 3, h, w), dtype=torch.float32, generator=generator, device=gdev).to(dev)
    p = AugmentParams(pack_table(1), gp_noise=gp if _is_device(xyz_img) else gp.numpy(), gaussian_scale=noise_params["gaussian_scale"])
    if isinstance(xyz_img, torch.Tensor):
        x = xyz_img.permute(2, 0, 1)[None].contiguous().clone()
        return add_xyz_noise_(x, p)[0].permute(1, 2, 0).contiguous()
    x = np.ascontiguousarray(np.transpose(xyz_img, (2, 0, 1))[None]).copy()
    return np.ascontiguousarray(np.transpose(add_xyz_noise_(x, p)[0], (1, 2, 0)))
