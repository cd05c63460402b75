"""msm_prepare_inputs (ops.prepare_inputs) on the GPU against its definition computed on the host in IEEE float32: (x - mean) / std,
zero padding at the right / bottom, depth copied bit for bit.  Every comparison is bitwise; nothing is compared with device torch
arithmetic."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]


def ops():
    from unseenobjectswithmeanshift_amd import ops as o
    return o


def bits(t):
    return t.contiguous().view(torch.int32)


def make_image(shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=g) * 255.0
    flat = x.view(-1)
    if flat.numel() >= 8:
        special = torch.tensor([float("inf"), float("-inf"), 1e-40, -1e-40, 1.401298464324817e-45, 0.0, -0.0, 255.0])
        flat[torch.randperm(flat.numel(), generator=g)[:8]] = special          # +-inf, denormals, signed zeros
    return x


def make_depth(shape, seed):
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(shape, generator=g)                                          # negatives included
    flat = d.view(-1)
    if flat.numel() >= 12:
        idx = torch.randperm(flat.numel(), generator=g)[:12]
        flat[idx[:4]] = 0.0
        b = flat.view(torch.int32)
        b[idx[4:8]] = 0x7FC00001                                                 # NaNs of two different payloads (one of them negative)
        b[idx[8:12]] = -0x3EDCBB                                                 # 0xFFC12345
    return d


def expected(x, d, mean, std, frame):
    """The definition on the host: float32 subtraction and division are IEEE there."""
    H, W = x.shape[-2:]
    pad = (0, frame[1] - W, 0, frame[0] - H)
    y = x if mean is None else (x - torch.tensor(mean)[:, None, None]) / torch.tensor(std)[:, None, None]
    want_d = None
    if d is not None:
        want_d = torch.zeros(d.shape[:2] + tuple(frame), dtype=torch.int32)      # integer copy: F.pad of NaNs is not promised to keep payloads
        want_d[:, :, :H, :W] = bits(d)
    return F.pad(y, pad), want_d


def offset_view(t, off):
    """``t``'s values as a contiguous view ``off`` floats into a larger allocation (the base is 4-byte but not 16-byte aligned for off = 1)."""
    big = torch.empty(t.numel() + 8, device=DEV)
    v = big[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def run(x, d, mean, std, frame, in_off=0, out_off=0):
    o = ops()
    dx = offset_view(x.to(DEV), in_off) if in_off else x.to(DEV)
    dd = None if d is None else (offset_view(d.to(DEV), in_off) if in_off else d.to(DEV))
    nan = lambda t: None if t is None else offset_view(torch.full(tuple(t.shape[:2]) + tuple(frame), float("nan"), device=DEV), out_off)  # noqa: E731
    out_x, out_d = nan(dx), nan(dd)
    assert dx.data_ptr() % 16 == (4 * in_off) % 16 and out_x.data_ptr() % 16 == (4 * out_off) % 16
    kw = {} if mean is None else dict(mean=torch.tensor(mean, device=DEV), std=torch.tensor(std, device=DEV))
    got_x, got_d = o.prepare_inputs(dx, dd, frame=frame, out_image=out_x, out_depth=out_d, **kw)
    assert got_x is out_x and got_d is out_d
    return got_x.cpu(), None if got_d is None else got_d.cpu()


def check(x, d, mean, std, frame, **kw):
    want_x, want_d = expected(x, d, mean, std, frame)
    got_x, got_d = run(x, d, mean, std, frame, **kw)
    assert not torch.isnan(got_x).any()                                          # every element of the NaN-filled output was written
    assert torch.equal(got_x, want_x) and torch.equal(bits(got_x), bits(want_x))
    if d is not None:
        assert torch.equal(bits(got_d), want_d)
    else:
        assert got_d is None


CASES = [  # image shape, frame, input offset, output offset (floats)
    pytest.param((2, 3, 5, 7), (8, 8), 0, 0, id="elementwise-loads-vector-stores"),
    pytest.param((3, 3, 32, 64), (32, 64), 0, 0, id="vector-both-ways-no-padding"),
    pytest.param((1, 3, 30, 44), (32, 64), 0, 0, id="vector-loads-padding-both-ways"),
    pytest.param((2, 3, 6, 8), (7, 10), 0, 0, id="frame-width-not-a-multiple-of-4"),
    pytest.param((3, 3, 32, 64), (32, 64), 1, 0, id="unaligned-input-base"),
    pytest.param((3, 3, 32, 64), (32, 64), 0, 1, id="unaligned-output-base"),
    pytest.param((4, 3, 264, 352), (288, 352), 0, 0, id="more-quads-than-the-capped-grid"),
]


@pytest.mark.parametrize("shape,frame,in_off,out_off", CASES)
def test_prepare_inputs_equals_the_definition(shape, frame, in_off, out_off):
    x, d = make_image(shape, 1), make_depth(shape, 2)
    check(x, d, MEAN, STD, frame, in_off=in_off, out_off=out_off)
    check(x, None, MEAN, STD, frame, in_off=in_off, out_off=out_off)            # without depth
    check(x, d, None, None, frame, in_off=in_off, out_off=out_off)              # without mean / std: pure padding, bitwise
    check(x, d[:, :1].contiguous(), MEAN, STD, frame, in_off=in_off, out_off=out_off)       # Cd = 1


def test_pure_copy_keeps_every_bit():
    """Without mean / std the image goes through as 32-bit words too: NaN payloads survive."""
    d = make_depth((2, 3, 9, 12), 3)
    got, _ = run(d, None, None, None, (12, 16))
    want = torch.zeros((2, 3, 12, 16), dtype=torch.int32)
    want[:, :, :9, :12] = bits(d)
    assert torch.equal(bits(got), want)


def test_defaults_and_empty_batch():
    o = ops()
    x = make_image((2, 3, 6, 8), 4)
    img, dep = o.prepare_inputs(x.to(DEV))                                       # frame defaults to (H, W); fresh outputs
    assert dep is None and torch.equal(bits(img.cpu()), bits(x))
    img, dep = o.prepare_inputs(torch.empty((0, 3, 6, 8), device=DEV), torch.empty((0, 1, 6, 8), device=DEV), frame=(8, 8))
    assert tuple(img.shape) == (0, 3, 8, 8) and tuple(dep.shape) == (0, 1, 8, 8)
    # the entry point itself: N = 0 is MSM_OK and launches nothing (the output keeps what it held)
    from unseenobjectswithmeanshift_amd import _lib
    src, dst = x.to(DEV), torch.full((2, 3, 6, 8), 7.0, device=DEV)
    p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())             # noqa: E731
    rc = _lib.lib().msm_prepare_inputs(p(src), p(None), p(None), p(None), p(dst), p(None), 0, 3, 0, 6, 8, 6, 8,
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0 and bool((dst == 7.0).all())


def test_errors():
    from unseenobjectswithmeanshift_amd import _lib
    o = ops()
    x = torch.rand(1, 3, 8, 8, device=DEV)
    mean, std = torch.tensor(MEAN, device=DEV), torch.tensor(STD, device=DEV)
    out = torch.empty_like(x)
    with pytest.raises(RuntimeError, match=r"msm_prepare_inputs: the frame 7x8 is smaller than the image 8x8"):
        o.prepare_inputs(x, frame=(7, 8))
    with pytest.raises(RuntimeError, match="mean and std go together"):
        o.prepare_inputs(x, mean=mean)
    with pytest.raises(RuntimeError, match="its own input"):
        o.prepare_inputs(x, out_image=x)
    with pytest.raises(RuntimeError, match="its own input"):
        o.prepare_inputs(x, out, out_depth=out)
    with pytest.raises(RuntimeError, match="out_depth without depth"):
        o.prepare_inputs(x, out_depth=torch.empty_like(x))
    with pytest.raises(RuntimeError, match="must be"):
        o.prepare_inputs(x, frame=(8, 8), out_image=torch.empty(1, 3, 8, 12, device=DEV))
    with pytest.raises(RuntimeError, match="contiguous"):
        o.prepare_inputs(x.transpose(2, 3))
    # the library's own checks of the optional pointers' pairing
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())             # noqa: E731
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for args, msg in (((p(x), p(None), p(mean), p(None), p(out), p(None), 1, 3, 0, 8, 8, 8, 8, s), "mean and std go together"),
                      ((p(x), p(x), p(None), p(None), p(out), p(None), 1, 3, 3, 8, 8, 8, 8, s), "depth and depth_out go together"),
                      ((p(x), p(None), p(None), p(None), p(out), p(None), 1, 3, 3, 8, 8, 8, 8, s), "Cd = 3 without depth"),
                      ((p(None), p(None), p(None), p(None), p(out), p(None), 1, 3, 0, 8, 8, 8, 8, s), "null pointer"),
                      ((p(x), p(None), p(None), p(None), p(out), p(None), 1 << 20, 3, 0, 8, 8, 8, 1 << 12, s), "too many for one launch")):
        rc = L.msm_prepare_inputs(*args)
        assert rc != 0
        with pytest.raises(RuntimeError, match=msg):
            _lib.check(rc, "msm_prepare_inputs")
    torch.cuda.synchronize()
