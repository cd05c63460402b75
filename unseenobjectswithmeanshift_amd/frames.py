"""From a raw camera frame to the network's input tensors.

Own counterpart of the head of every entry point of the reference, same names where it has them:

  PIXEL_MEANS     <- lib/fcn/config.py:377 (BGR)
  compute_xyz     <- lib/fcn/get_backbone.py:96-102 (tools/get_network.py:115-121, ...)
  make_sample     <- read_sample, tools/test_image_with_ms_transformer.py:115-147
                     (the ROS listener's run_network, ros/test_images_segmentation_transformer.py:159-173, with float depth)

A frame is a uint8 (H,W,3) BGR image, a depth image (uint16 millimetres or float32 metres) and four intrinsics.  The definition
(every step fp32, round to nearest -- the reference's arithmetic with the intrinsics rounded to fp32 first):

  image[c][y][x] = lut[c][color[y][x][c']]       lut[c][v] = float32(v) / float32(255) - float32(mean[c] / 255.0)
  z              = float32(d) / depth_scale      uint16 depth;  float32 depth: z = d, NaN -> 0 (run_network:170)
  xyz[0]         = ((float32(x) - px) * z) / fx
  xyz[1]         = ((float32(y) - py) * z) / fy
  xyz[2]         = z
  zeros at the right / bottom up to the next multiple of ``size_divisibility``

Like two_stage, the functions follow their data: device tensors go through the HIP kernel (ops.ingest_frames, one launch for a whole
batch, 5 bytes per pixel uploaded instead of 24); host tensors and numpy arrays -- the unit tests of the logic without a GPU -- through
the same definition in numpy float32 operations.  There is no fallback on a device tensor.
"""
import numpy as np
import torch

PIXEL_MEANS = (102.9801, 115.9465, 122.7717)      # BGR, lib/fcn/config.py:377

_CAM_KEYS = ("fx", "fy", "x_offset", "y_offset")


def image_lut(pixel_means=PIXEL_MEANS):
    """(3,256) float32: lut[c][v] = float32(v) / float32(255) - float32(mean[c] / 255.0) -- read_sample's `im / 255.0 - mean / 255.0`
    (the mean divided in float64 and rounded once, the image in float32) for every byte value."""
    v = np.arange(256, dtype=np.float32) / np.float32(255)
    m = (np.asarray(pixel_means, dtype=np.float64) / 255.0).astype(np.float32)
    if m.shape != (3,):
        raise ValueError("pixel_means: three values, in the channel order of the output")
    return v[None, :] - m[:, None]


def camera_table(camera_params, F):
    """(F,4) float32 tensor of fx, fy, px, py, one row per frame, from the reference's camera_params.json dict (fx, fy, x_offset,
    y_offset) -- for every frame -- or a list of F of them.  An (F,4) or (4,) array / tensor of those values passes through (a
    device tensor stays where it is)."""
    if isinstance(camera_params, dict):
        camera_params = [camera_params] * F
    if isinstance(camera_params, torch.Tensor):
        t = camera_params.to(torch.float32)
    elif isinstance(camera_params, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(camera_params, dtype=np.float32))
    else:
        if len(camera_params) != F:
            raise ValueError(f"camera_params: {len(camera_params)} entries for {F} frames")
        t = torch.from_numpy(np.array([[p[k] for k in _CAM_KEYS] for p in camera_params], dtype=np.float32).reshape(F, 4))
    if t.dim() == 1:
        t = t[None].expand(F, 4)
    if tuple(t.shape) != (F, 4):
        raise ValueError(f"camera_params: {tuple(t.shape)} values for {F} frames, (F, 4) fx, fy, px, py expected")
    return t.contiguous()


def _is_device(*xs):
    """True when the arrays live on the GPU; host tensors / numpy arrays -> False; a mixture is an error."""
    where = {bool(isinstance(x, torch.Tensor) and x.is_cuda) for x in xs if x is not None}
    if len(where) > 1:
        raise ValueError("frames: colour and depth must live on the same side (both on the device or both on the host)")
    return where.pop() if where else False


def _host(x):
    return x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _depth_metres_host(depth, depth_scale):
    """z of the definition for a host depth array: uint16 (or int16 holding the same bits) / depth_scale, float32 with NaN -> 0."""
    if depth.dtype == np.int16:
        depth = depth.view(np.uint16)
    if depth.dtype == np.uint16:
        return depth.astype(np.float32) / np.float32(depth_scale)
    if depth.dtype != np.float32:
        raise TypeError(f"depth must be uint16 (millimetres) or float32 (metres), got {depth.dtype}")
    return np.where(np.isnan(depth), np.float32(0), depth)


def _xyz_host(z, cam):
    """z (F,H,W) float32, cam (F,4) float32 -> (F,3,H,W) float32: the xyz rows of the definition, every step a float32 operation."""
    F_, H, W = z.shape
    col = np.arange(W, dtype=np.float32).reshape(1, 1, W)
    row = np.arange(H, dtype=np.float32).reshape(1, H, 1)
    fx, fy, px, py = (cam[:, i].reshape(F_, 1, 1) for i in range(4))
    out = np.empty((F_, 3, H, W), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        np.divide(np.multiply(col - px, z), fx, out=out[:, 0])
        np.divide(np.multiply(row - py, z), fy, out=out[:, 1])
    out[:, 2] = z
    return out


_LUT_DEVICE = {}


def _device_lut(dev, pixel_means):
    key = (str(dev), tuple(float(m) for m in pixel_means))
    if key not in _LUT_DEVICE:
        _LUT_DEVICE[key] = torch.from_numpy(image_lut(pixel_means)).to(dev)
    return _LUT_DEVICE[key]


def _round_up(v, d):
    return -(-v // d) * d


def ingest(color, depth, camera_params, *, order="bgr", depth_scale=1000.0, size_divisibility=1, out_image=None, out_depth=None,
           pixel_means=PIXEL_MEANS):
    """One frame (H,W,3) or a batch (F,H,W,3) of uint8 colour with its depth ((F,)H,W uint16 millimetres / ``depth_scale``, or float32
    metres; None: image only) -> (image ((F,)3,Hp,Wp), xyz ((F,)3,Hp,Wp) or None) float32 tensors: what read_sample builds, padded
    with zeros at the right / bottom to multiples of ``size_divisibility``.  ``order="rgb"`` is for cameras that deliver rgb8: the
    output is in BGR order either way (the order the means and the checkpoints assume).  ``camera_params``: see camera_table.
    ``out_image`` / ``out_depth`` (batch shaped, device path only) are written in place."""
    if order not in ("bgr", "rgb"):
        raise ValueError(f"order must be 'bgr' or 'rgb', got {order!r}")
    device = _is_device(color, depth)
    single = color.ndim == 3
    if single:
        color = color[None]
        depth = None if depth is None else depth[None]
    if color.ndim != 4 or color.shape[-1] != 3 or color.dtype not in (torch.uint8, np.uint8):
        raise ValueError("color must be uint8 of shape (H, W, 3) or (F, H, W, 3)")
    F_, H, W, _ = color.shape
    if depth is not None and tuple(depth.shape) != (F_, H, W):
        raise ValueError(f"depth {tuple(depth.shape)} does not match the colour frames {(F_, H, W)}")
    d = int(size_divisibility)
    Hp, Wp = (_round_up(H, d), _round_up(W, d)) if d > 1 else (H, W)
    cam = camera_table(camera_params, F_) if depth is not None else None
    if device:
        from . import ops
        dev = color.device
        image, xyz = ops.ingest_frames(color.contiguous(), None if depth is None else depth.contiguous(),
                                       None if cam is None else cam.to(dev), _device_lut(dev, pixel_means),
                                       depth_div=float(depth_scale), swap_rb=order == "rgb", frame=(Hp, Wp), out_image=out_image,
                                       out_depth=out_depth)
    else:
        if out_image is not None or out_depth is not None:
            raise ValueError("out_image / out_depth are for device frames")
        col = _host(color)
        if order == "rgb":
            col = col[..., ::-1]
        lut = image_lut(pixel_means)
        img = np.zeros((F_, 3, Hp, Wp), dtype=np.float32)
        for c in range(3):
            img[:, c, :H, :W] = lut[c][col[..., c]]
        image, xyz = torch.from_numpy(img), None
        if depth is not None:
            out = np.zeros((F_, 3, Hp, Wp), dtype=np.float32)
            out[:, :, :H, :W] = _xyz_host(_depth_metres_host(_host(depth), depth_scale), cam.numpy())
            xyz = torch.from_numpy(out)
    if single:
        return image[0], None if xyz is None else xyz[0]
    return image, xyz


def compute_xyz(depth_img, fx, fy, px, py, height=None, width=None):
    """Depth in metres (H,W) or (F,H,W) -> the ordered point cloud (...,H,W,3), as the reference's compute_xyz returns it (numpy in,
    numpy out; a tensor gives a tensor).  float32 arithmetic with the intrinsics rounded to float32 (NaN depth -> 0); ``height`` /
    ``width`` are the reference's redundant arguments and must match the depth image when given.
    On a device tensor this is the ingest kernel run on a zero colour batch: the kernel has no image-less form, so the call also writes
    (and drops) a 12 bytes-per-pixel image and transposes the result -- about twice the traffic the points alone need.  A per-frame
    loop should call ingest / make_sample, which give the image and the (3,H,W) points the network takes in the same launch."""
    shape = tuple(depth_img.shape)
    if len(shape) not in (2, 3) or (height is not None and height != shape[-2]) or (width is not None and width != shape[-1]):
        raise ValueError(f"compute_xyz: depth {shape} must be (H, W) or (F, H, W) matching height / width")
    single = len(shape) == 2
    d3 = depth_img[None] if single else depth_img
    cam = {"fx": fx, "fy": fy, "x_offset": px, "y_offset": py}
    if _is_device(depth_img):
        # the kernel's xyz path (float32 depth); it needs a colour frame, whose image is dropped
        if d3.dtype != torch.float32:
            raise TypeError("compute_xyz: depth in metres, float32")
        color = torch.zeros(d3.shape + (3,), dtype=torch.uint8, device=d3.device)
        xyz = ingest(color, d3, cam)[1].permute(0, 2, 3, 1).contiguous()
    else:
        z = _depth_metres_host(_host(d3).astype(np.float32, copy=False), 1.0)
        xyz = np.ascontiguousarray(_xyz_host(z, camera_table(cam, z.shape[0]).numpy()).transpose(0, 2, 3, 1))
        if isinstance(depth_img, torch.Tensor):
            xyz = torch.from_numpy(xyz)
    return xyz[0] if single else xyz


def make_sample(color, depth, camera_params, **kw):
    """read_sample for one frame already in memory: {"image_color": (3,H,W), "depth": (3,H,W)} float32 tensors (no "depth" key without
    a depth image) -- what two_stage.test_sample_crop_nolabel takes.  Keyword arguments as ingest."""
    if color.ndim != 3:
        raise ValueError("make_sample takes one frame (H, W, 3); batches go through ingest")
    image, xyz = ingest(color, depth, camera_params, **kw)
    sample = {"image_color": image}
    if xyz is not None:
        sample["depth"] = xyz
    return sample
