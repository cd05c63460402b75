"""csrc/gemm.hip (msm_gemm_f32) on every workgroup tile, A layout, epilogue and edge, against the float64 definitions and the derived
bound of tests/gemm_cases.py: every element of every result obeys ``|got - ref| <= tol`` (no rtol / atol, nothing left out; the bound
is proved neither too tight nor toothless on the CPU by tests/test_gemm_cases_cpu.py).  GEMM_TILE forces each of the five tiles onto
shapes with ragged edges, GEMM_SHALLOW the shallow LDS tile onto shapes that default to the deep one.  On top of the bound: all
tiles, deep or shallow, aligned or misaligned pointers give the same bits (each output element is the same chain of
v_mfma_f32_16x16x4_f32 over ascending k on every path, zero-filled tails add exact zeros); NaN / inf in the last row of an operand
stay in their row / column (padded lanes are selected to zero, not multiplied by it); nothing is written outside ``out``; the
argument checks reject what the kernel would silently misread.  Every comparison prints ``RATIO <family> <max error / tol>``
(pytest -s): reported, never asserted.  Needs a real MI355X (pytest -m gpu)."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_cases as G  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -12345.5
TILE_IDS = {G.AUTO: "auto"}
tiles = pytest.mark.parametrize("tile", G.TILES, ids=lambda t: f"tile_{TILE_IDS.get(t, t)}")
shallows = pytest.mark.parametrize("shallow", G.SHALLOWS, ids=lambda s: "deep_auto" if s == G.AUTO else "shallow")


def ops():
    from unseenobjectswithmeanshift_amd import ops as _ops
    return _ops


def dev(t):
    return None if t is None else t.to(DEV)


def misaligned(t):
    """The same data as a contiguous view one float into a larger buffer: 4 bytes off every 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device=DEV, dtype=torch.float32)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def force(lib_option, tile, shallow=G.AUTO):
    lib_option("GEMM_TILE", tile)
    lib_option("GEMM_SHALLOW", shallow)


def inside(family, case, got, ref, tol):
    n = G.outside(got, ref, tol)
    print(f"RATIO {family} {G.ratio(got, ref, tol):.4f}   [{case}]")
    assert n == 0, f"{family} {case}: {n} of {ref.numel()} elements outside the bound, max error / tol = {G.ratio(got, ref, tol):.3f}"


@functools.lru_cache(maxsize=None)
def linear_ref(M, N, K, bias, act):
    a, w, b = G.linear_inputs(M, N, K)
    b = b if bias else None
    return G.linear64(a, None, w, b, act), G.linear_tol(a, None, w, b)


EPILOGUES = ((True, None), (True, "relu"), (False, None), (False, "relu"))


# =============================================================================================
# ops.gemm: K-contiguous A, row-major output
# =============================================================================================
@tiles
@shallows
@pytest.mark.parametrize("M,N,K", G.LINEAR_SHAPES)
def test_gemm_every_tile(lib_option, tile, shallow, M, N, K):
    a, w, b = (dev(t) for t in G.linear_inputs(M, N, K))
    force(lib_option, tile, shallow)
    for bias, act in EPILOGUES:
        got = ops().gemm(a, w, b if bias else None, act=act)
        assert got.shape == (M, N) and got.dtype == torch.float32
        inside("linear", f"{M}x{N}x{K} tile {tile} shallow {shallow} bias {bias} act {act}", got, *linear_ref(M, N, K, bias, act))


@pytest.mark.parametrize("M,N,K", G.LINEAR_SHAPES)
def test_gemm_tile_neutrality(lib_option, M, N, K):
    """The automatic tile's bits from every tile, deep or shallow, and from misaligned operands."""
    a, w, b = (dev(t) for t in G.linear_inputs(M, N, K))
    base = {e: ops().gemm(a, w, b if e[0] else None, act=e[1]) for e in EPILOGUES}
    for tile in G.TILES[1:]:
        for shallow in G.SHALLOWS:
            force(lib_option, tile, shallow)
            for e in EPILOGUES:
                assert torch.equal(ops().gemm(a, w, b if e[0] else None, act=e[1]), base[e]), (tile, shallow, e)
    force(lib_option, G.AUTO, G.AUTO)
    assert torch.equal(ops().gemm(misaligned(a), misaligned(w), b), base[(True, None)])


@pytest.mark.parametrize("which", G.MISALIGN_WHICH)
@pytest.mark.parametrize("M,N,K", G.MISALIGN_SHAPES)
def test_gemm_misaligned_pointers(M, N, K, which):
    """a, w, then both one float off alignment: the guarded element-wise loads, inside the bound and equal to the aligned run."""
    a, w, b = (dev(t) for t in G.linear_inputs(M, N, K))
    aligned = ops().gemm(a, w, b)
    got = ops().gemm(misaligned(a) if which in ("a", "both") else a, misaligned(w) if which in ("w", "both") else w, b)
    inside("linear", f"{M}x{N}x{K} misaligned {which}", got, *linear_ref(M, N, K, True, None))
    assert torch.equal(got, aligned)


@tiles
@shallows
@pytest.mark.parametrize("B,L,K,N", G.A2_SHAPES)
def test_gemm_a2(lib_option, tile, shallow, B, L, K, N):
    """a2 of a's shape (one batch) and a2 (L, K) broadcast over the leading dimension (batch B, stride 0)."""
    a, a2, a2b, w, b = G.a2_inputs(B, L, K, N)
    force(lib_option, tile, shallow)
    for name, second in (("equal", a2), ("broadcast", a2b)):
        got = ops().gemm(dev(a), dev(w), dev(b), a2=dev(second), act="relu")
        assert got.shape == (B, L, N)
        inside("a2", f"{name} {(B, L, K, N)} tile {tile} shallow {shallow}", got, G.linear64(a, second, w, b, "relu"), G.linear_tol(a, second, w, b))
    got = ops().gemm(dev(a), dev(w), a2=dev(a2b))
    inside("a2", f"broadcast, no bias {(B, L, K, N)} tile {tile} shallow {shallow}", got, G.linear64(a, a2b, w, None, None), G.linear_tol(a, a2b, w, None))


@pytest.mark.parametrize("B,L,K,N", G.A2_SHAPES)
def test_gemm_a2_tile_neutrality_and_misaligned(lib_option, B, L, K, N):
    a, a2, a2b, w, b = (dev(t) for t in G.a2_inputs(B, L, K, N))
    base = ops().gemm(a, w, b, a2=a2), ops().gemm(a, w, b, a2=a2b)
    for tile in G.TILES[1:]:
        for shallow in G.SHALLOWS:
            force(lib_option, tile, shallow)
            assert torch.equal(ops().gemm(a, w, b, a2=a2), base[0]) and torch.equal(ops().gemm(a, w, b, a2=a2b), base[1]), (tile, shallow)
    force(lib_option, G.AUTO, G.AUTO)
    cpu = G.a2_inputs(B, L, K, N)
    for k, second in enumerate((a2, a2b)):
        got = ops().gemm(a, w, b, a2=misaligned(second))
        inside("a2", f"misaligned a2 {(B, L, K, N)}", got, G.linear64(cpu[0], cpu[1 + k], cpu[3], cpu[4], None), G.linear_tol(cpu[0], cpu[1 + k], cpu[3], cpu[4]))
        assert torch.equal(got, base[k])


@tiles
@shallows
@pytest.mark.parametrize("K,split_k", G.SPLITK_CASES)
def test_gemm_split_k(lib_option, tile, shallow, K, split_k):
    """Raw parts (split_k, M, N): each part is the product over ITS k range (no part's range is empty), the float64 sum of the
    parts obeys the bound of the whole K."""
    M, N = G.SPLITK_MN
    a, w, _ = G.linear_inputs(M, N, K)
    ranges = G.split_ranges(K, split_k)
    assert ranges is not None and all(k0 < k1 for k0, k1 in ranges)
    force(lib_option, tile, shallow)
    parts = ops().gemm(dev(a), dev(w), split_k=split_k)
    assert parts.shape == (split_k, M, N)
    for s, (k0, k1) in enumerate(ranges):
        ak, wk = a[:, k0:k1], w[:, k0:k1]
        inside("split-K", f"K {K} part {s} of {split_k}: k {k0}..{k1} tile {tile} shallow {shallow}", parts[s],
               G.linear64(ak, None, wk, None, None), G.linear_tol(ak, None, wk, None))
    inside("split-K", f"K {K} / {split_k} summed tile {tile} shallow {shallow}", parts.double().sum(0), *linear_ref(M, N, K, False, None))


@pytest.mark.parametrize("K,split_k", G.SPLITK_CASES)
def test_gemm_split_k_tile_neutrality(lib_option, K, split_k):
    a, w, _ = (dev(t) for t in G.linear_inputs(*G.SPLITK_MN, K))
    base = ops().gemm(a, w, split_k=split_k)
    for tile in G.TILES[1:]:
        for shallow in G.SHALLOWS:
            force(lib_option, tile, shallow)
            assert torch.equal(ops().gemm(a, w, split_k=split_k), base), (tile, shallow)
    force(lib_option, G.AUTO, G.AUTO)
    assert torch.equal(ops().gemm(misaligned(a), misaligned(w), split_k=split_k), base)


def test_gemm_split_k_rejections():
    M, N = G.SPLITK_MN
    a, w, b = (dev(t) for t in G.linear_inputs(M, N, 96))
    with pytest.raises(RuntimeError, match="bias/act"):
        ops().gemm(a, w, b, split_k=3)
    with pytest.raises(RuntimeError, match="bias/act"):
        ops().gemm(a, w, act="relu", split_k=3)
    assert G.split_ranges(64, 8) is None
    a, w = a[:, :64].contiguous(), w[:, :64].contiguous()
    with pytest.raises(RuntimeError, match=r"split_k=8 too large for K=64"):
        ops().gemm(a, w, split_k=8)
    # the same call on the C ABI with an output of our own: an error code, and nothing was launched into it
    from unseenobjectswithmeanshift_amd._lib import lib
    out = torch.full((8, M, N), SENTINEL, device=DEV)
    rc = lib().msm_gemm_f32(ops()._p(a), None, ops()._p(w), None, ops()._p(out), M, N, 64, 1, 64, 1, M * 64, 0, 0, N, 1, M * N, M * N,
                            0, 0, 0, 0, 0, 0, 8, ops()._stream())
    torch.cuda.synchronize()
    assert rc != 0 and b"too large" in lib().msm_last_error_string()
    assert bool((out == SENTINEL).all())


@tiles
@pytest.mark.parametrize("M,N,K", G.POISON_SHAPES)
def test_gemm_poisoned_edges(lib_option, tile, M, N, K):
    """NaN in the last row of a: NaN in the last output row only.  inf in the last row of w: non-finite values in the last output
    column only.  Tiles read past M and N from clamped addresses (that very row) and must SELECT zero there."""
    a, w, b = G.linear_inputs(M, N, K)
    ref, tol = linear_ref(M, N, K, True, None)
    force(lib_option, tile)
    an = a.clone()
    an[M - 1] = float("nan")
    got = ops().gemm(dev(an), dev(w), dev(b))
    assert bool(torch.isnan(got[M - 1]).all())
    inside("linear", f"{M}x{N}x{K} tile {tile} NaN row", got[:M - 1], ref[:M - 1], tol[:M - 1])
    wi = w.clone()
    wi[N - 1] = float("inf")
    got = ops().gemm(dev(a), dev(wi), dev(b))
    assert not bool(torch.isfinite(got[:, N - 1]).any())
    inside("linear", f"{M}x{N}x{K} tile {tile} inf column", got[:, :N - 1], ref[:, :N - 1], tol[:, :N - 1])


@tiles
@pytest.mark.parametrize("offset", G.SENTINEL_OFFSETS)
@pytest.mark.parametrize("N", G.SENTINEL_N)
def test_gemm_writes_stay_inside_out(lib_option, tile, N, offset):
    """out= a contiguous view ``offset`` floats into a sentinel-filled buffer (4: 16-byte stores where N % 4 == 0, 5: scalar stores):
    the result lands in the view, the sentinels before and after it survive."""
    M, K = G.SENTINEL_MK
    for k in (K, K + 1):                                    # vector loads, guarded loads
        a, w, b = (dev(t) for t in G.linear_inputs(M, N, k))
        plain = ops().gemm(a, w, b)
        force(lib_option, tile)
        buf = torch.full((offset + M * N + 67,), SENTINEL, device=DEV)
        out = buf[offset:offset + M * N].view(M, N)
        assert out.data_ptr() % 16 == (offset * 4) % 16
        got = ops().gemm(a, w, b, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert bool((buf[:offset] == SENTINEL).all()) and bool((buf[offset + M * N:] == SENTINEL).all())
        inside("linear", f"{M}x{N}x{k} tile {tile} out at +{offset}", out, *linear_ref(M, N, k, True, None))
        assert torch.equal(out, plain)
        force(lib_option, G.AUTO)


def test_gemm_out_rejections():
    """out must be fp32, contiguous, on a's device and of shape lead + (N,); split_k allocates its own parts."""
    M, N, K = 33, 65, 36
    a, w, b = (dev(t) for t in G.linear_inputs(M, N, K))
    a3 = a[:32].view(2, 16, K)
    for bad in (torch.empty(N, M, device=DEV).t(),                       # right shape, wrong strides
                torch.empty(M, 2 * N, device=DEV)[:, :N],                # a row stride the kernel is not told of
                torch.empty(M, N + 1, device=DEV), torch.empty(M * N, device=DEV), torch.empty(N, M, device=DEV),
                torch.empty(M, N, device=DEV, dtype=torch.float64), torch.empty(M, N, device=DEV, dtype=torch.float16),
                torch.empty(M, N)):
        with pytest.raises(RuntimeError, match="out|GPU"):
            ops().gemm(a, w, b, out=bad)
    with pytest.raises(RuntimeError, match="out"):
        ops().gemm(a3, w, b, out=torch.empty(32, N, device=DEV))         # lead is (2, 16)
    with pytest.raises(RuntimeError, match="out"):
        ops().gemm(a, w, split_k=2, out=torch.empty(2, M, N, device=DEV))
    out = torch.empty(2, 16, N, device=DEV)
    assert ops().gemm(a3, w, b, out=out) is out
    assert torch.equal(out.view(32, N), ops().gemm(a, w, b)[:32])


# =============================================================================================
# conv1x1_nchw_to_tokens: M-contiguous A, vector and matrix bias
# =============================================================================================
@tiles
@pytest.mark.parametrize("kind", G.MCONTIG_BIAS)
@pytest.mark.parametrize("B,Cin,H,W,Cout", G.MCONTIG_SHAPES)
def test_conv1x1_nchw_to_tokens(lib_option, tile, B, Cin, H, W, Cout, kind):
    inp = G.conv1x1_inputs(B, Cin, H, W, Cout)
    x, w, bias = inp[0], inp[1], G.mcontig_bias(inp, kind)
    force(lib_option, tile)
    got = ops().conv1x1_nchw_to_tokens(dev(x), dev(w), dev(bias))
    assert got.shape == (B, H * W, Cout)
    inside("m-contiguous", f"{(B, Cin, H, W, Cout)} tile {tile} bias {kind}", got, G.conv1x1_64(x, w, bias), G.conv1x1_tol(x, w, bias))
    if kind == "matrix":                                    # every image gets the same matrix: on a zero map, exactly it
        got = ops().conv1x1_nchw_to_tokens(torch.zeros_like(x, device=DEV), dev(w), dev(bias))
        for i in range(B):
            assert torch.equal(got[i].cpu(), bias)


def test_conv1x1_nchw_to_tokens_rejects_a_wrong_matrix_bias():
    x, w, _, m = (dev(t) for t in G.conv1x1_inputs(2, 36, 3, 4, 64))
    for bad in (m[:11].contiguous(), m[:, :63].contiguous(), m.t().contiguous(), torch.cat([m, m])):
        with pytest.raises(RuntimeError, match="matrix bias"):
            ops().conv1x1_nchw_to_tokens(x, w, bad)


# =============================================================================================
# conv1x1_tokens_to_nchw: the weight as the A operand, NCHW output, per-row bias, tokens of image b as the per-batch "weight"
# =============================================================================================
@tiles
@shallows
@pytest.mark.parametrize("B,HW,Cin,Cout", G.NCHW_SHAPES)
def test_conv1x1_tokens_to_nchw(lib_option, tile, shallow, B, HW, Cin, Cout):
    x, w, bias, _ = G.conv1x1_inputs(B, Cin, HW, 1, Cout)
    t = dev(G.tokens(x))
    force(lib_option, tile, shallow)
    for b_ in (bias, None):
        got = ops().conv1x1_tokens_to_nchw(t, dev(w), dev(b_))
        assert got.shape == (B, Cout, HW)
        for i in range(B):                                  # image i against image i's tokens
            inside("nchw-out", f"{(B, HW, Cin, Cout)} image {i} tile {tile} shallow {shallow} bias {b_ is not None}", got[i:i + 1],
                   G.conv1x1_64(x[i:i + 1], w, b_, "nchw"), G.conv1x1_tol(x[i:i + 1], w, b_, "nchw"))


# =============================================================================================
# implicit 3x3 convolution over NHWC tokens
# =============================================================================================
@tiles
@pytest.mark.parametrize("B,Cin,H,W,Cout", G.CONV3_TOKEN_SHAPES)
def test_conv3x3_tokens(lib_option, tile, B, Cin, H, W, Cout):
    x, w, _ = G.conv3x3_inputs(B, Cin, H, W, Cout)
    force(lib_option, tile)
    got = ops().conv3x3_tokens(dev(G.tokens(x)), dev(G.tap_major(w)), H, W)
    assert got.shape == (B, H * W, Cout)
    inside("implicit conv", f"tokens {(B, Cin, H, W, Cout)} tile {tile}", got, G.conv3x3_64(x, w), G.conv3x3_tol(x, w))


@tiles
@pytest.mark.parametrize("with_bias", (True, False), ids=("bias", "no_bias"))
@pytest.mark.parametrize("B,Cin,H,W,Cout", G.CONV3_NCHW_SHAPES)
def test_conv3x3_tokens_to_nchw_general_path(lib_option, tile, B, Cin, H, W, Cout, with_bias):
    """Shapes the weight-stationary kernel does not take (Cin != 64, W % 4 != 0, Cout % 64 != 0): the GEMM with NCHW output."""
    assert not (Cin == 64 and Cout % 64 == 0 and W % 4 == 0)
    x, w, bias = G.conv3x3_inputs(B, Cin, H, W, Cout)
    bias = bias if with_bias else None
    force(lib_option, tile)
    got = ops().conv3x3_tokens_to_nchw(dev(G.tokens(x)), dev(G.tap_major(w)), dev(bias), H, W)
    assert got.shape == (B, Cout, H * W)
    inside("implicit conv", f"nchw {(B, Cin, H, W, Cout)} tile {tile} bias {with_bias}", got, G.conv3x3_64(x, w, bias, "nchw"), G.conv3x3_tol(x, w, bias, "nchw"))


def test_conv3x3_rejects_channels_not_a_multiple_of_four():
    x, w, _ = G.conv3x3_inputs(1, 6, 3, 4, 8)
    with pytest.raises(RuntimeError, match="bad implicit-conv arguments"):
        ops().conv3x3_tokens(dev(G.tokens(x)), dev(G.tap_major(w)), 3, 4)
    with pytest.raises(RuntimeError, match="bad implicit-conv arguments"):
        ops().conv3x3_tokens_to_nchw(dev(G.tokens(x)), dev(G.tap_major(w)), None, 3, 4)


# =============================================================================================
# training: the three GEMMs of a linear backward
# =============================================================================================
def test_training_linear_forward_backward():
    """_Linear on x (35, 20), w (7, 20): y and grad_in = g w (K = 7), grad_W = g^T x and grad_b = 1^T g (K = 35, the token count:
    odd, so the guarded loads) against float64 autograd, each within the bound of the GEMM that produces it."""
    from unseenobjectswithmeanshift_amd import training
    x, w, b, g = G.train_inputs()
    xd, wd, bd = (t.double().requires_grad_() for t in (x, w, b))
    yd = torch.nn.functional.linear(xd, wd, bd)
    yd.backward(g.double())
    xg, wg, bg = (dev(t).requires_grad_() for t in (x, w, b))
    y = training.linear(xg, wg, bg)
    y.backward(dev(g))
    ones = torch.ones(1, x.shape[0])
    inside("training", "forward", y, yd.detach(), G.linear_tol(x, None, w, b))
    inside("training", "grad_in", xg.grad, xd.grad, G.linear_tol(g, None, w.t(), None))
    inside("training", "grad_W", wg.grad, wd.grad, G.linear_tol(g.t(), None, x.t(), None))
    inside("training", "grad_b", bg.grad, bd.grad, G.linear_tol(ones, None, g.t(), None)[0])
