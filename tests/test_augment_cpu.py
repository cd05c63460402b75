"""The host path of unseenobjectswithmeanshift_amd.augment -- the definitions D1-D5 in numpy float32 and integers -- against the
float64 oracles of augment_cases.py, against what the reference's cv2-free functions return (tests/golden/augment_reference.npz)
and draw_params against its stated ranges.  No GPU.

Figures these tests print (python -m pytest -s), as DESIGN 5y records them: the share of the 2^21 + 264 sample colours whose
float32 H / L / S differs from the rounded float64 value (never by more than one count), the same for the shifted
back-conversion and for D2, and D5's largest error against torch's float64 bicubic."""
import numpy as np
import pytest
import torch

import augment_cases as ac
from unseenobjectswithmeanshift_amd import _lib
from unseenobjectswithmeanshift_amd import augment as A


# ------------------------------------------------------------------------------------------------------------------------ oracles
def test_the_float64_oracle_is_colorsys():
    """The vectorised float64 restatement used below equals the standard library's conversion on a sub-sample."""
    cols = ac.color_sample()
    sub = np.concatenate([cols[:4096], cols[2 ** 21:]])
    np.testing.assert_allclose(ac.hls_forward_f64(sub), ac.colorsys_forward(sub), rtol=0, atol=1e-9)
    hls = np.rint(ac.hls_forward_f64(sub))
    np.testing.assert_allclose(ac.hls_back_f64(hls), ac.colorsys_back(hls), rtol=0, atol=1e-9)


# ------------------------------------------------------------------------------------------------------------------------ D1
@pytest.fixture(scope="module")
def sample_hls():
    cols = ac.color_sample()
    return cols, A.bgr_to_hls_host(cols)


def test_d1_forward_within_one_count(sample_hls):
    cols, got = sample_hls
    want = np.rint(ac.hls_forward_f64(cols))
    diff = np.abs(got.astype(np.float64) - want)
    share = (diff > 0).mean(axis=0) * 100
    print(f"\nD1 forward, {len(cols)} colours: H / L / S differ from float64 at {share[0]:.3f} % / {share[1]:.3f} % / {share[2]:.3f} %, "
          f"largest {diff.max(axis=0).tolist()} counts")
    assert diff.max() <= 1
    assert got.dtype == np.float32 and (got == np.rint(got)).all() and got[:, 0].max() <= 180 and got.min() >= 0


@pytest.mark.parametrize("d_h,d_l,d_s", ac.SHIFTS)
def test_d1_shift_and_back_within_one_count(sample_hls, d_h, d_l, d_s):
    _, hls = sample_hls
    shifted = A.shift_hls_host(hls, np.float32(d_h), np.float32(d_l), np.float32(d_s))
    want_shift = ac.shift_f64(hls, d_h, d_l, d_s)
    np.testing.assert_array_equal(shifted, want_shift)                   # multiples of 1/64: the shift is exact in both
    got = A.hls_to_bgr_host(shifted).astype(np.float64)
    want = np.clip(np.rint(ac.hls_back_f64(want_shift)), 0, 255)
    diff = np.abs(got - want)
    print(f"\nD1 shift ({d_h}, {d_l}, {d_s}) and back: {(diff > 0).any(axis=1).mean() * 100:.4f} % of {len(hls)} colours differ, largest {diff.max()}")
    assert diff.max() <= 1


def test_d1_mod_gives_180_for_a_tiny_negative_sum():
    hls = np.array([[0, 100, 100], [180, 100, 100], [5, 100, 100]], np.float32)
    out = A.shift_hls_host(hls, np.float32(-1e-6), np.float32(0), np.float32(0))
    assert out[:, 0].tolist() == [180.0, 0.0, 4.0]                      # float32(180 - 1e-6) is 180, whose remainder is 0
    assert A.shift_hls_host(hls, np.float32(-180), np.float32(0), np.float32(0))[:, 0].tolist() == [0.0, 0.0, 5.0]
    assert (A.hls_to_bgr_host(np.array([[180, 100, 100]], np.float32)) == A.hls_to_bgr_host(np.array([[0, 100, 100]], np.float32))).all()


def test_d1_structural_identities():
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1).reshape(1, 16, 16, 3)
    p = A.AugmentParams(A.pack_table(1, chromatic=True))
    np.testing.assert_array_equal(A.augment_color(grey, p), grey)         # d = 0 on a grey image: the identity
    for v in (0, 255):
        flat = np.full((1, 8, 8, 3), v, np.uint8)
        q = A.AugmentParams(A.pack_table(1, chromatic=True, d_h=7.25, d_s=13.75, d_l=0.0))
        np.testing.assert_array_equal(A.augment_color(flat, q), flat)
    q.check()
    # the per-frame form by the reference's name
    im = np.ascontiguousarray(ac.color_sample()[:64 * 48].reshape(48, 64, 3))
    a = A.chromatic_transform(im, d_h=7.25, d_s=13.75, d_l=-20.5)
    b = A.augment_color(im[None], A.AugmentParams(A.pack_table(1, chromatic=True, d_h=7.25, d_s=13.75, d_l=-20.5)))[0]
    np.testing.assert_array_equal(a, b)
    label = np.zeros((48, 64), np.int64)
    label[10:20] = 3
    kept = A.chromatic_transform(im, label, d_h=7.25, d_s=13.75, d_l=-20.5)
    np.testing.assert_array_equal(kept[10:20], im[10:20])
    np.testing.assert_array_equal(kept[20:], a[20:])


# ------------------------------------------------------------------------------------------------------------------------ D2
def test_d2_within_one_count_and_exact_without_noise():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, size=(2, 37, 53, 3), dtype=np.uint8)
    noise = rng.normal(size=(2, 37, 53)).astype(np.float32)
    sigma = np.array([11.37, 0.0], np.float32)
    p = A.AugmentParams(A.pack_table(2, gaussian=True, sigma=sigma), pixel_noise=noise)
    got = A.augment_color(img, p).astype(np.float64)
    p.check()
    want = np.trunc(np.clip(img.astype(np.float64) + (sigma.astype(np.float64)[:, None, None] * noise.astype(np.float64))[..., None], 0, 255))
    diff = np.abs(got - want)
    print(f"\nD2: {(diff > 0).mean() * 100:.4f} % of the bytes differ from float64, largest {diff.max()}")
    assert diff.max() <= 1
    np.testing.assert_array_equal(got[1], img[1])
    assert (got[0] != img[0]).mean() > 0.5                               # the noise did something, the same to every channel
    d = got[0] - img[0]
    inner = (img[0].min(axis=-1) > 60) & (img[0].max(axis=-1) < 195)
    assert (np.abs(d[inner] - d[inner][:, :1]) <= 1).all()


# ------------------------------------------------------------------------------------------------------------------------ D3
@pytest.mark.parametrize("shape,size,horizontal", [((9, 8), 15, True), ((8, 9), 15, False), ((21, 38), 3, True), ((21, 38), 3, False),
                                                   ((21, 38), 15, True), ((21, 38), 15, False)])
def test_d3_equals_the_tap_loop(shape, size, horizontal):
    rng = np.random.default_rng(size + shape[0])
    img = rng.integers(0, 256, size=(1,) + shape + (3,), dtype=np.uint8)
    p = A.AugmentParams(A.pack_table(1, blur_size=size, blur_horizontal=horizontal))
    np.testing.assert_array_equal(A.augment_color(img, p)[0], ac.blur_oracle(img[0], size, horizontal))
    p.check()


def test_d3_raises_on_maps_smaller_than_the_halo():
    img = np.zeros((1, 9, 7, 3), np.uint8)
    with pytest.raises(ValueError, match="needs more than 7 pixels"):
        A.augment_color(img, A.AugmentParams(A.pack_table(1, blur_size=15, blur_horizontal=True)))
    with pytest.raises(ValueError, match="needs more than 7 pixels"):
        A.augment_color(img.transpose(0, 2, 1, 3).copy(), A.AugmentParams(A.pack_table(1, blur_size=15, blur_horizontal=False)))


def test_rows_that_ask_for_nothing_or_for_nonsense():
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, size=(4, 12, 16, 3), dtype=np.uint8)
    t = A.pack_table(4, blur_size=[0, 4, 0, 0], chromatic=[False, False, True, False], d_h=[0, 0, np.nan, 0])
    t[3, A.COL_FLAGS] = A.FLAG_GAUSSIAN | A.FLAG_BLUR
    p = A.AugmentParams(t)
    np.testing.assert_array_equal(A.augment_color(img, p), img)
    assert p.status[:, A.STATUS_COLOR].tolist() == [0, A.BAD_ROW, A.BAD_ROW, A.BAD_ROW]
    with pytest.raises(ValueError, match="image 1 was skipped"):
        p.check()


# ------------------------------------------------------------------------------------------------------------------------ D4
@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_d4_equals_the_brute_force_oracle(kind):
    depth = ac.depth_map(24, 40, 5, kind)
    m = np.float32(1.0173)
    p = A.AugmentParams(A.pack_table(1, depth=True, multiplier=m, ellipses=[ac.ORACLE_ELLIPSES]))
    got = A.augment_depth(depth[None], p)[0]
    p.check()
    f = A.unpack_table(p.table)
    es = [(f["rx"][0, i], f["ry"][0, i], f["cos"][0, i], f["sin"][0, i], f["key"][0, i]) for i in range(len(ac.ORACLE_ELLIPSES))]
    want, near, centres, boxes = ac.depth_oracle(depth, 1000.0, m, es)
    assert near.sum() <= 0.01 * min(boxes), (int(near.sum()), boxes)     # the oracle itself stays under the cap
    ok = ~near
    np.testing.assert_array_equal(got[ok] == 0, want[ok] == 0)
    np.testing.assert_allclose(got[ok], want[ok], rtol=1e-6, atol=0)
    assert got.dtype == np.float32 and 0.2 < (got == 0).mean() < 0.95
    # the centres, exactly -- keys 0 and 2^32 - 1 are the first and the last valid pixel
    z = A.augment_depth(depth[None], A.AugmentParams(A.pack_table(1, depth=True, multiplier=m)))[0]
    cx, cy = A.ellipse_centres_host(z, np.array([e[4] for e in es], np.uint32))
    assert list(zip(cx.tolist(), cy.tolist())) == centres
    valid = np.flatnonzero(z.reshape(-1) > 0)
    assert cy[0] * 40 + cx[0] == valid[0] and cy[1] * 40 + cx[1] == valid[-1]


def test_d4_edges():
    zeros = np.zeros((1, 6, 8), np.uint16)
    p = A.AugmentParams(A.pack_table(1, depth=True, multiplier=1.5, ellipses=[[(3, 3, 0, 7)]]))
    assert (A.augment_depth(zeros, p) == 0).all()                        # n = 0: no dropout, nothing to index
    one = zeros.copy()
    one[0, 4, 5] = 1000
    out = A.augment_depth(one, A.AugmentParams(A.pack_table(1, depth=True, multiplier=1.5)))
    assert out[0, 4, 5] == np.float32(1.5) and (out != 0).sum() == 1
    out = A.augment_depth(one, A.AugmentParams(A.pack_table(1, depth=True, ellipses=[[(0, 0, 0, 2 ** 32 - 1)]])))
    assert (out == 0).all()                                              # radius 0 still covers its own centre
    full = np.full((1, 6, 8), 1000, np.uint16)
    out = A.augment_depth(full, A.AugmentParams(A.pack_table(1, depth=True, ellipses=[[(0, 0, 90, 0)]])))
    assert (out == 0).sum() == 1 and out[0, 0, 0] == 0
    t = A.pack_table(2, depth=True, ellipses=[[(2, 2, 0, 0)], [(2, 2, 0, 0)]])
    t[0, A.COL_COUNT] = 33
    t.view(np.float32)[1, A.COL_ELLIPSES] = np.inf
    p = A.AugmentParams(t)
    np.testing.assert_array_equal(A.augment_depth(np.concatenate([full, full]), p), np.ones((2, 6, 8), np.float32))
    assert p.status[:, A.STATUS_DEPTH].tolist() == [A.BAD_COUNT, A.BAD_ELLIPSE]
    with pytest.raises(ValueError, match="ellipse count"):
        p.check()


# ------------------------------------------------------------------------------------------------------------------------ D5
@pytest.mark.parametrize("H,W,Hp,Wp,h,w", [(24, 40, 24, 40, 6, 10), (22, 38, 22, 38, 5, 9), (24, 40, 32, 64, 6, 10), (24, 40, 24, 40, 40, 50),
                                           (37, 150, 40, 152, 9, 37)])
def test_d5_against_torch_float64(H, W, Hp, Wp, h, w):
    xyz, gp = ac.xyz_case(2, H, W, Hp, Wp, h, w, seed=H + w)
    before = xyz.copy()
    p = A.AugmentParams(A.pack_table(2), gp_noise=gp)
    assert A.add_xyz_noise_(xyz, p, size=(H, W)) is xyz
    up = ac.bicubic_f64(gp, H, W)
    where = before[:, 2:3, :H, :W] > 0
    want = before.astype(np.float64)
    want[:, :, :H, :W] += np.where(where, p.gaussian_scale * up, 0)
    err = np.abs(xyz - want).max()
    up32 = torch.nn.functional.interpolate(torch.from_numpy(gp), size=(H, W), mode="bicubic", align_corners=False).numpy()
    up_err = np.abs(A.upsample_bicubic_host(gp, H, W) - up).max() / np.abs(up).max()
    print(f"\nD5 {h}x{w} -> {H}x{W}: upsampled field off float64 by {up_err:.2e} of its maximum (torch's fp32 CPU run: "
          f"{np.abs(up32 - up).max() / np.abs(up).max():.2e}); xyz by {err / np.abs(want).max():.2e}")
    assert up_err <= 1e-4 and err <= 1e-4 * np.abs(want).max()
    keep = np.ones(xyz.shape, bool)
    keep[:, :, :H, :W] = ~np.broadcast_to(where, (2, 3, H, W))
    assert (xyz.view(np.int32)[keep] == before.view(np.int32)[keep]).all()    # z <= 0 and the padding keep their bits
    assert (xyz[:, :, :H, :W][np.broadcast_to(where, (2, 3, H, W))] != before[:, :, :H, :W][np.broadcast_to(where, (2, 3, H, W))]).mean() > 0.99


def test_d5_weights_of_the_4x_case_are_four_constants():
    idx, w = A.bicubic_taps(6, 24)
    assert np.unique(w, axis=0).shape[0] == 4 and w.dtype == np.float32 and idx.min() == 0 and idx.max() == 5
    np.testing.assert_allclose(w.sum(axis=1), 1, atol=1e-6)


# ------------------------------------------------------------------------------------------------------------------------ draw_params
def test_draw_params_ranges_and_reproducibility():
    a = A.draw_params(64, 24, 40, rng=np.random.default_rng(7), generator=torch.Generator().manual_seed(1), add_noise=True)
    b = A.draw_params(64, 24, 40, rng=np.random.default_rng(7), generator=torch.Generator().manual_seed(1), add_noise=True)
    np.testing.assert_array_equal(a.table, b.table)
    np.testing.assert_array_equal(a.pixel_noise, b.pixel_noise)
    np.testing.assert_array_equal(a.gp_noise, b.gp_noise)
    assert a.table.dtype == np.int32 and a.table.shape == (64, A.TABLE_ROW)
    assert a.pixel_noise.shape == (64, 24, 40) and a.gp_noise.shape == (64, 3, 6, 10) and a.gp_noise.dtype == np.float32
    assert a.gaussian_scale == 0.005 and abs(float(a.gp_noise.std()) - 1) < 0.05
    f = A.unpack_table(a.table)
    chroma, gauss, blur = (f["flags"] & A.FLAG_CHROMATIC) != 0, (f["flags"] & A.FLAG_GAUSSIAN) != 0, (f["flags"] & A.FLAG_BLUR) != 0
    assert 40 < chroma.sum() <= 64 and gauss.sum() > 30 and not (gauss & blur).any() and (f["flags"] & A.FLAG_DEPTH).all()
    assert (np.abs(f["d_h"]) <= 9).all() and (np.abs(f["d_l"]) <= 25.6).all() and (np.abs(f["d_s"]) <= 25.6).all()
    assert (f["d_h"][~chroma] == 0).all() and (f["sigma"] >= 0).all() and (f["sigma"] <= 25.6).all() and (f["sigma"][~gauss] == 0).all()
    assert set(f["blur_size"][blur].tolist()) <= set(A.BLUR_SIZES) and (f["blur_size"][~blur] == 0).all()
    assert set(f["blur_horizontal"].tolist()) <= {0, 1}
    assert (np.abs(f["multiplier"] - 1) < 0.2).all() and f["multiplier"].std() > 0.01
    assert (f["count"] >= 0).all() and (f["count"] <= A.ELLIPSE_MAX).all() and 7 < f["count"].mean() < 13
    for b_ in range(64):
        n = f["count"][b_]
        assert (f["rx"][b_, :n] == np.rint(f["rx"][b_, :n])).all() and (f["rx"][b_, :n] >= 0).all() and (f["ry"][b_, :n] <= 40).all()
        np.testing.assert_allclose(f["cos"][b_, :n].astype(np.float64) ** 2 + f["sin"][b_, :n].astype(np.float64) ** 2, 1, atol=1e-6)
        assert (a.table[b_, A.COL_ELLIPSES + A.ELLIPSE_WORDS * n:] == 0).all()
    assert len(np.unique(f["key"][f["count"] > 0, 0])) > 40               # the keys use their 32 bits
    assert f["key"].max() > 2 ** 31


def test_draw_params_clamps_the_poisson_draw_and_skips_unused_fields():
    many = dict(A.TABLETOP_NOISE_PARAMS, ellipse_dropout_mean=60)
    p = A.draw_params(8, 16, 16, rng=np.random.default_rng(0), noise_params=many)
    assert (A.unpack_table(p.table)["count"] == A.ELLIPSE_MAX).all()
    p.check()
    q = A.draw_params(8, 16, 16, rng=np.random.default_rng(0), chromatic=True, add_noise=False, depth=False)
    assert q.pixel_noise is None and q.gp_noise is None and not (A.unpack_table(q.table)["flags"] & ~A.FLAG_CHROMATIC).any()
    rng = np.random.default_rng(0)
    r = A.draw_params(3, 8, 8, rng=rng, chromatic=False, depth=False)
    assert not r.table[:, A.COL_FLAGS].any() and not r.table[:, A.COL_COUNT].any() and rng.random() == np.random.default_rng(0).random()     # nothing was drawn


def test_draw_params_feeds_the_host_pipeline():
    rng = np.random.default_rng(11)
    B, H, W = 3, 24, 40
    p = A.draw_params(B, H, W, rng=rng, add_noise=True, generator=torch.Generator().manual_seed(5))
    color = rng.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)
    depth = ac.depth_map(H, W, 1, "u16")[None].repeat(B, 0)
    from unseenobjectswithmeanshift_amd import targets as tg
    raw = np.zeros((B, H, W), np.uint8)
    raw[:, 5:15, 5:20] = 2
    cam = {"fx": 500.0, "fy": 500.0, "x_offset": 20.0, "y_offset": 12.0}
    image, xyz, batch = tg.training_batch(color, depth, raw, cam, size_divisibility=32, augment=p)
    p.check()
    image0, xyz0, batch0 = tg.training_batch(color, depth, raw, cam, size_divisibility=32)
    assert image.shape == image0.shape == (B, 3, 32, 64) and torch.equal(batch.masks, batch0.masks)
    assert not torch.equal(xyz, xyz0) and torch.isfinite(xyz).all() and (xyz[:, :, H:] == 0).all() and (xyz[:, :, :, W:] == 0).all()
    z = A.augment_depth(depth, p)
    assert torch.equal(xyz[:, 2, :H, :W] == 0, torch.from_numpy(z == 0))
    same = tg.training_batch(color, depth, raw, cam, size_divisibility=32, augment=None)
    assert torch.equal(same[0], image0) and torch.equal(same[1], xyz0)


# ------------------------------------------------------------------------------------------------------------------------ fixture
def test_host_path_matches_the_reference_functions(golden):
    g = golden("augment_reference")
    p = A.AugmentParams(A.pack_table(1, depth=True, multiplier=g["depth_multiplier"]))
    got = A.augment_depth(g["depth_in"][None], p, depth_scale=1.0)[0]
    np.testing.assert_allclose(got, g["depth_out"], rtol=1e-6, atol=0)
    q = A.AugmentParams(A.pack_table(1, gaussian=True, sigma=g["noise_sigma"]), pixel_noise=g["noise_field"][None].astype(np.float32))
    got = A.augment_color(g["noise_in"][None], q)[0]
    assert np.abs(got.astype(np.int64) - g["noise_out"].astype(np.int64)).max() <= 1
    assert (got != g["noise_in"]).mean() > 0.5


# ------------------------------------------------------------------------------------------------------------------------ ABI
def test_abi_declares_the_entry_points():
    syms = _lib.declared_symbols()
    for name in ("msm_augment_color", "msm_augment_depth", "msm_augment_depth_workspace", "msm_augment_table_row", "msm_xyz_noise"):
        assert name in syms and name in _lib._SIGNATURES
    assert _lib.ABI_VERSION >= 41
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    for name, value in (("TABLE_ROW", A.TABLE_ROW), ("ELLIPSE_MAX", A.ELLIPSE_MAX), ("ELLIPSE_WORDS", A.ELLIPSE_WORDS),
                        ("CHROMATIC", A.FLAG_CHROMATIC), ("GAUSSIAN", A.FLAG_GAUSSIAN), ("BLUR", A.FLAG_BLUR), ("DEPTH", A.FLAG_DEPTH),
                        ("BAD_ROW", A.BAD_ROW), ("BAD_COUNT", A.BAD_COUNT), ("BAD_ELLIPSE", A.BAD_ELLIPSE), ("BAD_CENTRE", A.BAD_CENTRE)):
        assert f"#define MSM_AUGMENT_{name} {value}\n" in text, name
    assert A.TABLE_ROW == A.COL_ELLIPSES + A.ELLIPSE_WORDS * A.ELLIPSE_MAX
