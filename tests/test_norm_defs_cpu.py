"""The float64 normalisation definitions of oracle/msm_oracle.py (the yardsticks of tests/test_gpu_norm.py) against torch's
own kernels run in double.  CPU only: keeps the definitions honest without a GPU."""
import pytest
import torch
import torch.nn.functional as F

from oracle import msm_oracle as O


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def close64(a, b, tol=1e-12):
    assert a.dtype == torch.float64 and a.shape == b.shape
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("E,rows", [(64, 1), (128, 37), (512, 5)])
@pytest.mark.parametrize("eps", [1e-5, 1e-3])
def test_layernorm_chain(E, rows, eps):
    x, parts, bias = rnd(rows, E, seed=1), rnd(3, rows, E, seed=2), rnd(E, seed=3)
    g1, b1, g2, b2 = 1 + 0.1 * rnd(E, seed=4), rnd(E, seed=5), 1 + 0.1 * rnd(E, seed=6), rnd(E, seed=7)
    y, y2 = O.layernorm_chain(x, None, None, g1, b1, eps=eps)
    close64(y, F.layer_norm(x, (E,), g1, b1, eps))
    assert y2 is None
    v = x + parts[0] + parts[1] + parts[2] + bias
    y, y2 = O.layernorm_chain(x, parts, bias, g1, b1, True, g2, b2, eps)
    r = F.normalize(F.layer_norm(v, (E,), g1, b1, eps), p=2, dim=-1, eps=1e-12)
    close64(y, r)
    close64(y2, F.layer_norm(r, (E,), g2, b2, eps))
    close64(y.norm(dim=-1), torch.ones(rows, dtype=torch.float64))
    y, _ = O.layernorm_chain(None, parts, None, g1, b1, eps=eps)
    close64(y, F.layer_norm(parts.sum(0), (E,), g1, b1, eps))
    # float32 arguments are widened, not computed in single
    y32, _ = O.layernorm_chain(x.float(), None, None, g1.float(), b1.float(), eps=eps)
    close64(y32, F.layer_norm(x.float().double(), (E,), g1.float().double(), b1.float().double(), eps))


def test_layernorm_chain_zero_rows_stay_finite():
    E = 64
    y, y2 = O.layernorm_chain(rnd(4, E, seed=1), None, None, torch.zeros(E), torch.zeros(E), True, torch.ones(E), torch.zeros(E))
    assert torch.equal(y, torch.zeros(4, E, dtype=torch.float64)) and torch.isfinite(y2).all()


@pytest.mark.parametrize("B,C,H,W,groups", [(2, 64, 16, 24, 32), (1, 4, 3, 5, 1), (3, 32, 1, 1, 32), (1, 256, 15, 20, 256), (2, 128, 7, 9, 32)])
@pytest.mark.parametrize("off", [0.0, 100.0])
def test_groupnorm_tokens(B, C, H, W, groups, off):
    x = rnd(B, C, H, W, seed=1) + off
    g, b = 1 + 0.1 * rnd(C, seed=2), rnd(C, seed=3)
    tok = x.flatten(2).transpose(1, 2).contiguous()
    ref = F.group_norm(x, groups, g, b, 1e-5).flatten(2).transpose(1, 2)
    # off = 100: F.group_norm in double is itself only ~1e-10 accurate there (one-pass moments); the two-pass definition is the exact one
    tol = 1e-12 if off == 0.0 else 1e-9
    close64(O.groupnorm_tokens(tok, g, b, H, W, groups), ref, tol)
    close64(O.groupnorm_tokens(tok, g, b, H, W, groups, relu=True), F.relu(ref), tol)
    close64(O.groupnorm_tokens(tok.float(), g, b, H, W, groups, eps=1e-3),
            F.group_norm(x.float().double(), groups, g, b, 1e-3).flatten(2).transpose(1, 2), tol)


@pytest.mark.parametrize("H,W,uh,uw", [(15, 20, 8, 10), (15, 20, 1, 1), (15, 20, 15, 20), (15, 20, 5, 6), (61, 67, 31, 34), (61, 67, 20, 22),
                                       (16, 24, 8, 12), (16, 24, 5, 8), (3, 5, 7, 11), (1, 1, 4, 4)])
def test_bilinear_upsample_tokens(H, W, uh, uw):
    B, C = 2, 8
    up = rnd(B, C, uh, uw, seed=4)
    ref = F.interpolate(up, size=(H, W), mode="bilinear", align_corners=False).flatten(2).transpose(1, 2)
    tok = up.flatten(2).transpose(1, 2).contiguous()
    close64(O.bilinear_upsample_tokens(tok, (uh, uw), H, W), ref)
    x, g, b = rnd(B, H * W, C, seed=5), 1 + 0.1 * rnd(C, seed=6), rnd(C, seed=7)
    full = O.groupnorm_tokens(x, g, b, H, W, 2, up=tok, up_hw=(uh, uw), relu=True)
    gn = F.group_norm(x.transpose(1, 2).reshape(B, C, H, W), 2, g, b).flatten(2).transpose(1, 2)
    close64(full, F.relu(gn + ref))


@pytest.mark.parametrize("H,W,npf,temperature,scale", [(7, 33, 32, 10000.0, 6.283185307179586), (1, 1, 128, 20.0, 1.0)])
def test_position_embedding_sine_in_double(H, W, npf, temperature, scale):
    p64 = O.position_embedding_sine(1, H, W, npf, temperature, scale, dtype=torch.float64)
    p32 = O.position_embedding_sine(1, H, W, npf, temperature, scale)
    assert p64.dtype == torch.float64 and p32.dtype == torch.float32
    assert float((p64 - p32.double()).abs().max()) < 5e-6
    # against the definition written out element by element
    for (c, y, x) in [(0, 0, 0), (1, H - 1, W - 1), (npf + 2, H // 2, W // 3), (2 * npf - 1, 0, W - 1)]:
        i = c % npf
        e = ((y + 1) / (H + 1e-6) if c < npf else (x + 1) / (W + 1e-6)) * scale
        a = torch.tensor(e / temperature ** (2 * (i // 2) / npf), dtype=torch.float64)
        assert abs(float(p64[0, c, y, x]) - float(a.cos() if i % 2 else a.sin())) < 1e-14
