"""The fp32 K/V projection after its stores were put under the next unit's MFMAs (csrc/kv_proj.hip: constants requested one pair of
feature blocks ahead, across the unit boundary; the unit loop compiled once per input layout): the raw-key entry points keep their
results bit for bit.  (Unit-norm keys from the projection's epilogue, the other half of that work, were measured and not kept --
profiles/cross_attn_unit_keys.md -- so there is no unit-key entry point to test.)  pytest -m gpu."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 512


def ops():
    from unseenobjectswithmeanshift_amd import ops as _ops
    return _ops


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def closed(got, ref, rtol, atol):
    torch.testing.assert_close(got.double().cpu(), ref, rtol=rtol, atol=atol)


def token_major_view(x):
    """x (B, 64, H, W) as a channels-last view inside a wider token buffer, the way the pixel decoder hands a level over."""
    B, C, H, W = x.shape
    buf = torch.zeros(B, H * W + 7, C, device=x.device)
    buf[:, 3:3 + H * W] = x.flatten(2).transpose(1, 2)
    view = buf[:, 3:3 + H * W].view(B, H, W, C).permute(0, 3, 1, 2)
    assert ops().is_token_major(view) and not view.is_contiguous()
    return view


def case(H, W, sep, seed):
    """x (2, 64, H, W), w (512, 64), the constant -- dense (HW, 512) or separable (H + W, 512) -- and [K | V] in float64."""
    x, w = rnd(2, 64, H, W, seed=seed + 1), rnd(N, 64, seed=seed + 2, scale=0.125)
    c = rnd(H + W if sep else H * W, N, seed=seed + 3)
    dense = (c[:H, None].double() + c[None, H:].double()).reshape(H * W, N) if sep else c.double()
    ref = torch.einsum("bkp,nk->bpn", x.double().flatten(2), w.double()) + dense
    return x.to(DEV), w.to(DEV), c.to(DEV), ref


@pytest.mark.parametrize("sep", [False, True])
def test_kv_project_raw_multi_equals_checked_single(sep):
    """msm_kv_project_multi_f32 is bit-identical to a float64-checked output of the single-job entry point on the same inputs: a
    ragged last 16-token tile (37 = 1 x 37) and an exact one (48 = 6 x 8), dense and separable constants, token-major input (both
    entry points take the weight-stationary kernel there at any size)."""
    xs, ws, cs, cws, singles = [], [], [], [], []
    for (H, W), seed in (((1, 37), 40), ((6, 8), 50)):
        x, w, c, ref = case(H, W, sep, seed)
        view = token_major_view(x)
        cw = W if sep else 0
        single = ops().kv_project(view, w, c, cw)
        closed(single, ref, rtol=1e-5, atol=2e-5)                          # test_kv_project's bound
        xs.append(view), ws.append(w), cs.append(c), cws.append(cw), singles.append(single.clone())
    for got, want in zip(ops().kv_project_multi(xs, ws, cs, cmat_widths=cws), singles):
        assert torch.equal(got, want)


@pytest.mark.parametrize("sep", [False, True])
def test_kv_project_raw_several_units_per_wave(sep):
    """Waves that walk MORE than one unit, in both input layouts: sixteen jobs of 19 x 55 = 1045 tokens (65 tiles + 5 tokens) at B = 2
    get 16 workgroups = 256 waves each for 264 units, so eight waves of every job take two units -- the second unit's x and its
    first pair's constants are requested while the first is computed -- and the others one (the last unit of a wave requests
    itself again).  Jobs alternate NCHW / token-major.  Against float64 and, bit for bit, the single-job entry point (one unit per
    wave at this size)."""
    H, W = 19, 55
    x, w, c, ref = case(H, W, sep, 60)
    cw = W if sep else 0
    view = token_major_view(x)
    single = ops().kv_project(view, w, c, cw)
    closed(single, ref, rtol=1e-5, atol=2e-5)
    xs = [view if j % 2 else x for j in range(16)]
    outs = ops().kv_project_multi(xs, [w] * 16, [c] * 16, cmat_widths=[cw] * 16)
    for got in outs:
        assert torch.equal(got, single)
