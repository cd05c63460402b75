"""The augmentation kernels (pytest -m gpu): msm_augment_color / msm_augment_depth / msm_xyz_noise through
unseenobjectswithmeanshift_amd.augment against the host path of the same module -- EQUAL BITS, every comparison -- with guard
bands around every output, tables that must be refused without a wild access, and the seam into training.ucn_model_losses."""
import numpy as np
import pytest
import torch

import augment_cases as ac
from unseenobjectswithmeanshift_amd import augment as A
from unseenobjectswithmeanshift_amd import ops
from unseenobjectswithmeanshift_amd import targets as tg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256                      # elements on either side of an output


def _guarded(shape, dtype, fill, shift=0):
    """(buffer, view): a contiguous tensor of ``shape`` inside a buffer filled with ``fill``, ``shift`` elements off the guard."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD + shift,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD + shift:GUARD + shift + n].view(shape)


def _guards_intact(buf, view, fill):
    n, start = view.numel(), view.storage_offset()
    return bool((buf[:start] == fill).all()) and bool((buf[start + n:] == fill).all())


def _color(color, table, noise=None, shift=0, check_fit=True):
    """augment_color on the device into a guarded output, and the host result of the same parameters (``check_fit=False``: a blur
    that does not fit the image is left to the status word on both sides)."""
    host = A.AugmentParams(table.copy(), pixel_noise=noise)
    if not check_fit:
        host.host_table = None
    want = A.augment_color(color, host)
    dev = host.to(DEV)
    dev.host_table = None                                     # the device decides alone
    src_buf = torch.zeros((color.size + 16 + shift,), dtype=torch.uint8, device=DEV)
    src = src_buf[shift:shift + color.size].view(color.shape)
    src.copy_(torch.from_numpy(color))
    buf, out = _guarded(color.shape, torch.uint8, 0xA5, shift)
    got = ops.augment_color(src, dev.table, dev.pixel_noise, dev._status(torch.device(DEV)), out=out)
    assert got.data_ptr() == out.data_ptr() and _guards_intact(buf, out, 0xA5)
    assert dev.status[:, A.STATUS_COLOR].cpu().tolist() == host.status[:, A.STATUS_COLOR].tolist()
    return got.cpu().numpy(), want, host


def _four_modes(B=4):
    return A.pack_table(B, chromatic=[True, False, True, False], d_h=[7.25, 0, -9, 0], d_l=[-20.5, 0, 25.5, 0], d_s=[13.75, 0, -25.5, 0],
                        gaussian=[True, False, False, False], sigma=[11.37, 0, 0, 0], blur_size=[0, 15, 3, 0],
                        blur_horizontal=[True, True, False, True])


@pytest.mark.parametrize("H,W", [(21, 38), (9, 8), (16, 64), (8, 9)])
def test_color_modes_equal_the_host_path(H, W):
    """One row per image: D1 + D2, D3 horizontal 15 alone, D1 + D3 vertical 3, nothing.  21 x 38: 3 W is no multiple of 16;
    9 x 8 / 8 x 9: the smallest legal blur along x (along y: the vertical row gets size 15 there); 16 x 64: one full tile."""
    rng = np.random.default_rng(H * W)
    color = rng.integers(0, 256, size=(4, H, W, 3), dtype=np.uint8)
    noise = rng.normal(size=(4, H, W)).astype(np.float32)
    table = _four_modes()
    if (H, W) == (8, 9):
        table[1, A.COL_BLUR_HORIZONTAL] = 0                    # H = 8: size 15 along y
    got, want, host = _color(color, table, noise)
    host.check()
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got[3], color[3])
    assert all((got[b] != color[b]).mean() > 0.5 for b in range(3))


def test_color_halo_across_tile_and_image_edges():
    """Two tiles plus three pixels in each direction: a halo crosses a tile edge and an image edge at once, every size."""
    H, W = 2 * 16 + 3, 2 * 64 + 3
    rng = np.random.default_rng(1)
    B = 2 * len(A.BLUR_SIZES)
    color = rng.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)
    table = A.pack_table(B, chromatic=[i % 4 == 0 for i in range(B)], d_h=3.5, d_l=4.25, d_s=-6.5,
                         blur_size=[s for s in A.BLUR_SIZES for _ in range(2)], blur_horizontal=[True, False] * len(A.BLUR_SIZES))
    got, want, host = _color(color, table)
    host.check()
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(want[1], ac.blur_oracle(color[1], 3, False))


def test_color_sample_as_one_image():
    """The 2^21-colour sample as a 1 x 2048 x 1024 image under D1 (the vector path): every colour the CPU tests hold to float64."""
    color = ac.color_sample()[:2 ** 21].reshape(1, 2048, 1024, 3).copy()
    got, want, host = _color(color, A.pack_table(1, chromatic=True, d_h=7.25, d_l=-20.5, d_s=13.75))
    host.check()
    np.testing.assert_array_equal(got, want)


def test_color_base_pointer_one_byte_into_its_storage():
    rng = np.random.default_rng(2)
    color = rng.integers(0, 256, size=(4, 16, 64, 3), dtype=np.uint8)       # W % 4 == 0: only the pointers say "bytes"
    noise = rng.normal(size=(4, 16, 64)).astype(np.float32)
    got, want, _ = _color(color, _four_modes(), noise, shift=1)
    np.testing.assert_array_equal(got, want)


def test_color_bad_tables_are_skipped_and_reported():
    """Blur size 4, a blur wider than the image, flags that exclude each other, a shift that is not finite, noise asked for but
    absent: status bits, copied rows, intact guard bands.  Handled by bounds checks by construction: nothing here can fault."""
    rng = np.random.default_rng(3)
    color = rng.integers(0, 256, size=(6, 9, 7, 3), dtype=np.uint8)
    table = A.pack_table(6, blur_size=[4, 15, 0, 0, 0, 3], blur_horizontal=[True, True, True, True, True, False],
                         chromatic=[False, False, False, True, False, False], d_h=[0, 0, 0, np.inf, 0, 0],
                         gaussian=[False, False, False, False, True, False], sigma=1.0)
    table[2, A.COL_FLAGS] = A.FLAG_GAUSSIAN | A.FLAG_BLUR
    table[2, A.COL_BLUR_SIZE] = 2 ** 31 - 1
    got, want, host = _color(color, table, check_fit=False)
    assert host.status[:, A.STATUS_COLOR].tolist() == [A.BAD_ROW] * 5 + [0]
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got[:5], color[:5])
    dev = A.AugmentParams(table).to(DEV)
    with pytest.raises(ValueError, match="needs more than 7 pixels"):        # the host copy of the table lets the call itself raise
        A.augment_color(torch.from_numpy(color).to(DEV), dev)
    dev.host_table = None
    A.augment_color(torch.from_numpy(color).to(DEV), dev)
    with pytest.raises(ValueError, match="image 0 was skipped"):
        dev.check()


def test_library_abi_and_refused_shapes():
    """The loaded library carries the header's version and the new symbols; shapes the kernels do not take are MSM_E_INVALID from the
    entry point and from the workspace query, before any launch."""
    from unseenobjectswithmeanshift_amd import _lib
    L = _lib.lib()
    assert L.msm_abi_version() == _lib.ABI_VERSION >= 41 and L.msm_augment_table_row() == A.TABLE_ROW
    for name in ("msm_augment_color", "msm_augment_depth", "msm_augment_depth_workspace", "msm_xyz_noise"):
        assert hasattr(L, name) and name in _lib.declared_symbols()
    assert _lib._HEADER.params["msm_augment_color"][-1] == _lib._HEADER.params["msm_augment_depth"][-1] == _lib._HEADER.params["msm_xyz_noise"][-1] == "stream"
    assert L.msm_augment_depth_workspace(2, 8193, 16) == -1 and L.msm_augment_depth_workspace(0, 8, 8) == -1
    assert L.msm_augment_depth_workspace(2, 24, 40) == 2 * (ops.AUGMENT_RECORD_ROW + 24) * 4
    tall = torch.zeros((1, 8193, 8), dtype=torch.float32, device=DEV)
    p = A.AugmentParams(A.pack_table(1)).to(DEV)
    with pytest.raises(RuntimeError, match="bad shape"):
        A.augment_depth(tall, p)
    color = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="another"):
        ops.augment_color(color, p.table, None, p._status(torch.device(DEV)), out=color)
    small = torch.zeros((1, ops.AUGMENT_RECORD_ROW), dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="needed"):
        ops.augment_depth(torch.zeros((1, 8, 8), device=DEV), p.table, p._status(torch.device(DEV)), records=small.reshape(-1))


# ------------------------------------------------------------------------------------------------------------------------ depth
def _depth_cases(kind):
    """B = 5 maps of 24 x 40 and their table: all zeros; one valid pixel; an ordinary map with 32 ellipses; the same with none;
    valid pixels only in the last row."""
    H, W = 24, 40
    d = np.stack([ac.depth_map(H, W, 10 + b, kind) for b in range(5)])
    d[0] = 0
    d[1] = 0
    d[1, 17, 23] = 1234 if kind == "u16" else 1.234
    d[4, :H - 1] = 0 if kind == "u16" else np.nan
    corners = [(0, 0, 0, 0), (60, 60, 0, 2 ** 32 - 1)]         # keys 0 and 2^32 - 1: the first and the last valid pixel, radius 0 and 60
    many = [(float(i % 7), float((3 * i) % 5), 11 * i, (i * 2654435761) % 2 ** 32) for i in range(32)]
    last = [(2, 9, 30, 0), (3, 1, 100, 2 ** 32 - 1), (1, 1, 0, 2 ** 31)]
    table = A.pack_table(5, depth=True, multiplier=[1.0173, 0.98, 1.0173, 1.04, 0.97],
                         ellipses=[[(3, 3, 0, 7)], corners[:1], many, [], last])
    return d, table


def _device_depth(depth):
    t = torch.from_numpy(depth.view(np.int16) if depth.dtype == np.uint16 else depth)
    return t.to(DEV)


@pytest.mark.parametrize("kind", ["u16", "f32"])
@pytest.mark.parametrize("W", [40, 38])
def test_depth_equals_the_host_path(kind, W):
    """W = 40 takes the 16-byte loads, W = 38 the element-wise ones."""
    depth, table = _depth_cases(kind)
    depth = np.ascontiguousarray(depth[:, :, :W])
    host = A.AugmentParams(table.copy())
    want = A.augment_depth(depth, host)
    host.check()
    dev = host.to(DEV)
    buf, out = _guarded(depth.shape, torch.float32, -7.0)
    got, records = ops.augment_depth(_device_depth(depth), dev.table, dev._status(torch.device(DEV)), out=out)
    assert _guards_intact(buf, out, -7.0)
    np.testing.assert_array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
    dev.check()
    assert (want[0] == 0).all() and (want[1] == 0).all()       # n = 0; one valid pixel under a radius-0 ellipse at key 0
    assert 0.2 < (want[2] == 0).mean() < 1 and (want[3] == 0).mean() < 0.3 and (want[4, :-1] == 0).all()
    rec = records.cpu().numpy()[:5 * ops.AUGMENT_RECORD_ROW].reshape(5, -1)
    assert rec[:, 0].tolist() == [1, 1, 32, 0, 3] and rec[0, 1] == 0 and rec[1, 1] == 1
    assert rec[1, 8:10].tolist() == [23, 17] and (rec[4, 8 + 1:8 + 36:12] == 23).all()          # centres: the one pixel; the last row
    # through the module, and with no DEPTH flag the map is only converted
    again = A.augment_depth(_device_depth(depth), dev)
    assert torch.equal(again, got)
    plain = A.augment_depth(_device_depth(depth), A.AugmentParams(A.pack_table(5)).to(DEV))
    np.testing.assert_array_equal(plain.cpu().numpy(), A.augment_depth(depth, A.AugmentParams(A.pack_table(5))))


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_depth_corners_and_large_radii(kind):
    """Centres in all four corners, keys 0 and 2^32 - 1, radius 0 and radius 60 (larger than the map)."""
    H, W = 24, 40
    depth = np.stack([ac.depth_map(H, W, 30 + b, kind) for b in range(4)])
    fill = 900 if kind == "u16" else 0.9
    depth[:, 0, 0] = depth[:, H - 1, W - 1] = fill             # the first and the last pixel are valid
    depth[2] = 0
    depth[2, 0, W - 1] = depth[2, H - 1, 0] = fill             # the other two corners, alone
    es = [[(0, 0, 0, 0), (0, 0, 45, 2 ** 32 - 1)], [(60, 1, 20, 0), (1, 60, 20, 2 ** 32 - 1)], [(5, 2, 45, 0), (2, 5, 45, 2 ** 32 - 1)],
          [(60, 60, 0, 2 ** 31)]]
    host = A.AugmentParams(A.pack_table(4, depth=True, multiplier=1.01, ellipses=es))
    want = A.augment_depth(depth, host)
    dev = host.to(DEV)
    got = A.augment_depth(_device_depth(depth), dev)
    np.testing.assert_array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
    dev.check()
    assert want[0, 0, 0] == 0 and want[0, -1, -1] == 0 and (want[0] == 0).sum() == (np.nan_to_num(depth[0]) == 0).sum() + 2
    assert (want[2] == 0).all() and (want[3] == 0).all()


@pytest.mark.parametrize("W", [40, 38])
def test_depth_multipliers_that_underflow_or_are_not_positive(W):
    """Launch (a) tests "z > 0" as d >= a threshold bisected per image: a multiplier that makes small depths underflow to zero (or
    to a subnormal), a negative one (nothing is valid) and a depth scale of 1 with raw values up to 65535."""
    rng = np.random.default_rng(6)
    depth = rng.integers(0, 400, size=(4, 24, W)).astype(np.uint16)
    depth[3] = rng.integers(0, 65536, size=(24, W))
    depth[3, 0, :2] = (65535, 0)
    es = [[(2, 3, 10 * i, (i * 2654435761) % 2 ** 32) for i in range(6)]] * 4
    for scale in (1.0, 1000.0):
        host = A.AugmentParams(A.pack_table(4, depth=True, multiplier=[1e-44, 3e-43, -1.0, 1.0], ellipses=es))
        want = A.augment_depth(depth, host, depth_scale=scale)
        dev = host.to(DEV)
        got = A.augment_depth(_device_depth(depth), dev, depth_scale=scale)
        np.testing.assert_array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
        dev.check()
    assert 0 < (want[0] > 0).sum() < (depth[0] > 0).sum() and not (want[2] > 0).any()


def test_depth_bad_tables_are_skipped_and_reported():
    """Count 33, a multiplier that is not finite, a radius that is not finite, a (cos, sin) of length 0 -- and hand-made records whose
    centre lies outside the image or whose count exceeds 32, given to the second launch alone.  Handled by bounds checks by
    construction: nothing here can fault."""
    H, W = 24, 40
    depth = np.stack([ac.depth_map(H, W, 50, "u16")] * 4)
    table = A.pack_table(4, depth=True, multiplier=[1.0, np.nan, 1.0, 1.0], ellipses=[[(3, 3, 0, 5)]] * 4)
    table[0, A.COL_COUNT] = 33
    tf = table.view(np.float32)
    tf[2, A.COL_ELLIPSES] = np.nan
    tf[3, A.COL_ELLIPSES + 2:A.COL_ELLIPSES + 4] = 0
    host = A.AugmentParams(table.copy())
    want = A.augment_depth(depth, host)
    assert host.status[:, A.STATUS_DEPTH].tolist() == [A.BAD_COUNT, A.BAD_ROW, A.BAD_ELLIPSE, A.BAD_ELLIPSE]
    np.testing.assert_array_equal(want, depth.astype(np.float32) / np.float32(1000))
    dev = host.to(DEV)
    buf, out = _guarded(depth.shape, torch.float32, -7.0)
    got, records = ops.augment_depth(_device_depth(depth), dev.table, dev._status(torch.device(DEV)), out=out)
    assert _guards_intact(buf, out, -7.0)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert dev.status[:, A.STATUS_DEPTH].cpu().tolist() == host.status[:, A.STATUS_DEPTH].tolist()
    with pytest.raises(ValueError, match="ellipse count"):
        dev.check()
    # the second launch alone on hand-made records
    good = A.AugmentParams(A.pack_table(4, depth=True, ellipses=[[(3, 3, 0, 5), (4, 2, 30, 2 ** 31)]] * 4)).to(DEV)
    zeroed = torch.zeros((ops.lib().msm_augment_depth_workspace(4, H, W) // 4,), dtype=torch.int32, device=DEV)
    ref, records = ops.augment_depth(_device_depth(depth), good.table, good._status(torch.device(DEV)), records=zeroed)
    rec = records.cpu().numpy()[:4 * ops.AUGMENT_RECORD_ROW].reshape(4, -1).copy()
    rec[0, 8:10] = (W, 3)                                      # a centre outside the image (its box follows it there)
    rec[0, 10:14] = (W - 4, W + 4, 0, 6)
    rec[1, 8 + 12:8 + 14] = (5, -1)
    rec[1, 8 + 14:8 + 18] = (0, 9, -5, 3)
    rec[2, 0] = 2 ** 31 - 1                                    # a count the launch must bound
    status = torch.zeros((4, 4), dtype=torch.int32, device=DEV)
    handmade = records.clone()
    handmade[:rec.size] = torch.from_numpy(rec.reshape(-1)).to(DEV)
    buf, out = _guarded(depth.shape, torch.float32, -7.0)
    got, _ = ops.augment_depth(_device_depth(depth), good.table, status, records=handmade, stages=2, out=out)
    assert _guards_intact(buf, out, -7.0)
    assert status[:, A.STATUS_DEPTH].cpu().tolist() == [A.BAD_CENTRE, A.BAD_CENTRE, 0, 0]
    got = got.cpu().numpy()
    np.testing.assert_array_equal(got[3], ref[3].cpu().numpy())
    # image 0 lost its first ellipse, image 1 its second; image 2 reads its two entries and then thirty zeroed ones (radius 0 around
    # pixel (0, 0), where 0 / 0 <= 1 is false): nothing more is dropped
    skipped = A.augment_depth(depth[:1], A.AugmentParams(A.pack_table(1, depth=True, ellipses=[[(4, 2, 30, 2 ** 31)]])))
    np.testing.assert_array_equal(got[0], skipped[0])
    np.testing.assert_array_equal(got[1], A.augment_depth(depth[1:2], A.AugmentParams(A.pack_table(1, depth=True, ellipses=[[(3, 3, 0, 5)]])))[0])
    np.testing.assert_array_equal(got[2], ref[2].cpu().numpy())


# ------------------------------------------------------------------------------------------------------------------------ xyz
@pytest.mark.parametrize("H,W,Hp,Wp,h,w", [(24, 40, 24, 40, 6, 10), (22, 38, 22, 38, 5, 9), (24, 40, 32, 64, 6, 10), (24, 40, 24, 40, 40, 50),
                                           (37, 150, 40, 152, 9, 37)])
def test_xyz_noise_equals_the_host_path(H, W, Hp, Wp, h, w):
    """4x and a non-integer scale (the source rows of a tile staged in LDS), a padded frame, a field finer than the image (more
    source rows than the tile stages: the direct form), three tiles in each direction with odd edges."""
    xyz, gp = ac.xyz_case(2, H, W, Hp, Wp, h, w, seed=H + w)
    before = xyz.copy()
    A.add_xyz_noise_(xyz, A.AugmentParams(A.pack_table(2), gp_noise=gp), size=(H, W))
    buf, dx = _guarded(before.shape, torch.float32, -7.0)
    dx.copy_(torch.from_numpy(before))
    dev = A.AugmentParams(A.pack_table(2), gp_noise=gp).to(DEV)
    assert A.add_xyz_noise_(dx, dev, size=(H, W)) is dx and _guards_intact(buf, dx, -7.0)
    got = dx.cpu().numpy()
    np.testing.assert_array_equal(got.view(np.int32), xyz.view(np.int32))
    keep = np.ones(before.shape, bool)
    keep[:, :, :H, :W] = ~np.broadcast_to(before[:, 2:3, :H, :W] > 0, (2, 3, H, W))
    assert (got.view(np.int32)[keep] == before.view(np.int32)[keep]).all() and (got != before).mean() > 0.2


# ------------------------------------------------------------------------------------------------------------------------ the whole
def _frames(B, H, W, seed=0):
    rng = np.random.default_rng(seed)
    color = torch.from_numpy(rng.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)).to(DEV)
    depth = rng.integers(400, 2000, size=(B, H, W)).astype(np.int16)
    depth[rng.random((B, H, W)) < 0.1] = 0
    raw = np.zeros((B, H, W), np.uint8)
    raw[:, 2 * H // 3:, :] = 1
    for b in range(B):
        for t in range(3):
            raw[b, 4 + 16 * t:18 + 16 * t, 8 + 4 * b:70 + 4 * b] = 3 + 2 * t
    return color, torch.from_numpy(depth).to(DEV), torch.from_numpy(raw).to(DEV)


CAM = {"fx": 570.3, "fy": 570.3, "x_offset": 45.0, "y_offset": 30.0}


def test_same_parameters_same_bits_and_no_synchronisation():
    B, H, W = 3, 60, 90
    color, depth, raw = _frames(B, H, W)
    gen = torch.Generator(DEV).manual_seed(4)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        p = A.draw_params(B, H, W, rng=np.random.default_rng(2), device=DEV, generator=gen, add_noise=True)
        runs = []
        for _ in range(2):
            c = A.augment_color(color, p)
            z = A.augment_depth(depth, p)
            xyz = torch.zeros((B, 3, 64, 96), device=DEV)
            xyz[:, :, :H, :W] = 1.0
            A.add_xyz_noise_(xyz, p, size=(H, W))
            runs.append((c, z, xyz))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert p.table.is_cuda and p.gp_noise.is_cuda and tuple(p.gp_noise.shape) == (B, 3, 15, 22)
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    p.check()
    # and they are the host path's bits under the same parameters
    host = A.AugmentParams(p.host_table, None if p.pixel_noise is None else p.pixel_noise.cpu().numpy(), p.gp_noise.cpu().numpy())
    c, z, xyz = runs[0]
    np.testing.assert_array_equal(c.cpu().numpy(), A.augment_color(color.cpu().numpy(), host))
    np.testing.assert_array_equal(z.cpu().numpy(), A.augment_depth(depth.cpu().numpy().view(np.uint16), host))
    hx = np.zeros((B, 3, 64, 96), np.float32)
    hx[:, :, :H, :W] = 1.0
    np.testing.assert_array_equal(xyz.cpu().numpy(), A.add_xyz_noise_(hx, host, size=(H, W)))
    assert (c != color).float().mean() > 0.3 and (z == 0).float().mean() > 0.1 and (xyz[:, :, :H, :W] != 1).float().mean() > 0.9


def test_training_batch_without_augment_is_unchanged_and_with_it_equals_the_host():
    B, H, W = 2, 60, 90
    color, depth, raw = _frames(B, H, W, seed=1)
    a = tg.training_batch(color, depth, raw, CAM, size_divisibility=32)
    b = tg.training_batch(color, depth, raw, CAM, size_divisibility=32, augment=None)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2].masks, b[2].masks) and torch.equal(a[2].label, b[2].label)
    p = A.draw_params(B, H, W, rng=np.random.default_rng(8), device=DEV, generator=torch.Generator(DEV).manual_seed(1), add_noise=True)
    image, xyz, batch = tg.training_batch(color, depth, raw, CAM, size_divisibility=32, augment=p)
    p.check()
    host = A.AugmentParams(p.host_table, None if p.pixel_noise is None else p.pixel_noise.cpu().numpy(), p.gp_noise.cpu().numpy())
    himage, hxyz, hbatch = tg.training_batch(color.cpu().numpy(), depth.cpu().numpy().view(np.uint16), raw.cpu().numpy(), CAM,
                                             size_divisibility=32, augment=host)
    assert torch.equal(image.cpu(), himage) and torch.equal(xyz.cpu(), hxyz) and torch.equal(batch.masks.cpu(), hbatch.masks)
    assert torch.equal(batch.masks, a[2].masks) and not torch.equal(image, a[0]) and not torch.equal(xyz, a[1])   # labels untouched


def test_augmented_training_batch_feeds_ucn_model_losses():
    from unseenobjectswithmeanshift_amd import criterion as cr
    from unseenobjectswithmeanshift_amd import synthetic as syn
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
    B, H, W = 2, 64, 96
    color, depth, raw = _frames(B, H, W, seed=2)
    params = A.draw_params(B, H, W, rng=np.random.default_rng(5), device=DEV, generator=torch.Generator(DEV).manual_seed(6), add_noise=True)
    image, xyz, batch = tg.training_batch(color, depth, raw, CAM, size_divisibility=32, sample_num=200,
                                          generator=torch.Generator(DEV).manual_seed(2), augment=params)
    params.check()
    assert tuple(image.shape) == tuple(xyz.shape) == (B, 3, 64, 96) and batch.counts == [3, 3]
    crit = cr.build_criterion(2, class_weight=2.0, mask_weight=5.0, dice_weight=5.0, no_object_weight=0.1, dec_layers=3,
                              train_num_points=112, generator=torch.Generator().manual_seed(9), solver="device")
    losses = tr.ucn_model_losses(model, image, xyz, batch, crit, labels=batch.label, embedding_loss=EmbeddingLoss(0.02, 0.5, 1.0, 1.0),
                                 embedding_weight=0.5)
    assert len(losses) == 3 * 3 + 1 and all(bool(torch.isfinite(v)) for v in losses.values())
    sum(losses.values()).backward()
    batch.check()
    grads = [p.grad for p in model.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads) and any(float(g.abs().sum()) > 0 for g in grads)


def test_per_frame_forms_on_device_tensors():
    """The reference's names on one device frame: the same bits as on the host under the same draws."""
    rng = np.random.default_rng(0)
    im = rng.integers(0, 256, size=(21, 38, 3), dtype=np.uint8)
    np.testing.assert_array_equal(A.chromatic_transform(torch.from_numpy(im).to(DEV), d_h=7.25, d_s=13.75, d_l=-20.5).cpu().numpy(),
                                  A.chromatic_transform(im, d_h=7.25, d_s=13.75, d_l=-20.5))
    d = (ac.depth_map(24, 40, 3, "u16") / 1000.0).astype(np.float32)
    for fn in (A.add_noise_to_depth, A.dropout_random_ellipses):
        np.testing.assert_array_equal(fn(torch.from_numpy(d).to(DEV), rng=np.random.default_rng(1)).cpu().numpy(), fn(d, rng=np.random.default_rng(1)))
    for seed in (0, 1, 2, 3):                                  # both branches of add_noise occur among these seeds or not: equality holds for blur
        got = A.add_noise(torch.from_numpy(im).to(DEV), rng=np.random.default_rng(seed), generator=torch.Generator().manual_seed(seed))
        np.testing.assert_array_equal(got.cpu().numpy(), A.add_noise(im, rng=np.random.default_rng(seed), generator=torch.Generator().manual_seed(seed)))
    xyz = rng.normal(size=(24, 40, 3)).astype(np.float32)
    got = A.add_noise_to_xyz(torch.from_numpy(xyz).to(DEV), generator=torch.Generator().manual_seed(7))
    np.testing.assert_array_equal(got.cpu().numpy(), A.add_noise_to_xyz(xyz, generator=torch.Generator().manual_seed(7)))
