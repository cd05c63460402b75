"""Cases shared by tests/test_gemm_cases_cpu.py and tests/test_gpu_gemm.py (not a test module): the shape tables of the fp32 GEMM
(csrc/gemm.hip, msm_gemm_f32), seeded inputs, the float64 definitions and the error bound.  Needs no GPU.

THE BOUND is derived, never measured.  Inputs are fp32 and convert exactly to float64.  Per output element

    tol = 2 * (K + 4) * 2^-24 * (|a + a2| . |w|^T + |bias|)            evaluated in float64

the running-error bound of a length-K fp32 dot product in ANY summation order (K * u * sum|a_k w_k| to first order, u = 2^-24),
one more rounding for a + a2, one for the bias add, and a factor two of margin.  For the implicit 3x3 convolution K = 9 * Cin and the
absolute-value product is the convolution of |x| with |w|.  ReLU is 1-Lipschitz and does not change it; split-K parts are summed in
float64 by the test, so the sum obeys the bound of the whole K.  A comparison is ``(got.double() - ref).abs() <= tol`` on EVERY
element (``outside`` counts the elements that miss); there is no rtol / atol pair and no share of elements is left out."""
import functools

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
AUTO = -1

TILES = (AUTO, 0, 1, 2, 3, 4)                   # MSM_OPT_GEMM_TILE: 128x128, 64x128, 64x64, 32x64, 32x32 workgroup tiles
SHALLOWS = (AUTO, 1)                            # MSM_OPT_GEMM_SHALLOW: 1 keeps the two small tiles off the 128-deep LDS tile
TILE_MN = ((4, 4), (2, 4), (2, 2), (1, 2), (1, 1))

# ops.gemm, K-contiguous A: (M, N, K).  The first seven have K % 4 == 0 (vector loads, every tile), the last three do not (guarded loads)
LINEAR_SHAPES = ((1, 1, 4), (37, 3, 256), (33, 65, 36), (129, 130, 132), (64, 64, 128), (65, 127, 160), (200, 288, 64),
                 (31, 33, 37), (5, 2, 130), (70, 36, 1))
A2_SHAPES = tuple((3, L, K, 40) for L in (50, 33) for K in (64, 256))           # (B, L, K, N)
A2_TILES = TILES
MISALIGN_SHAPES = LINEAR_SHAPES[:7]             # K % 4 == 0: only the pointer keeps them off the vector loads
MISALIGN_WHICH = ("a", "w", "both")
SPLITK_MN = (33, 70)
SPLITK_CASES = ((2048, 8), (1000, 4), (96, 3), (100, 2))                        # (K, split_k)
POISON_SHAPES = ((33, 65, 36), (31, 33, 37))
SENTINEL_N = (3, 34, 36, 130)
SENTINEL_MK = (33, 36)
SENTINEL_OFFSETS = (4, 5)                       # floats: 16-byte aligned (vector stores when N % 4 == 0) and not (scalar stores)

# conv1x1_nchw_to_tokens, M-contiguous A: (B, Cin, H, W, Cout)
MCONTIG_SHAPES = ((2, 36, 3, 4, 64), (2, 20, 1, 3, 5), (1, 64, 5, 7, 33), (3, 256, 6, 6, 130), (1, 2048, 2, 2, 64))
MCONTIG_BIAS = ("none", "vector", "matrix")
# conv1x1_tokens_to_nchw, NCHW output and per-row bias: (B, HW, Cin, Cout)
NCHW_SHAPES = ((2, 12, 36, 64), (1, 35, 64, 33), (3, 1, 20, 5), (2, 130, 256, 130), (2, 7, 18, 9))     # the last: Cin % 4 != 0, guarded loads
# implicit 3x3 convolution: (B, Cin, H, W, Cout)
CONV3_TOKEN_SHAPES = ((2, 4, 1, 1, 8), (1, 4, 1, 5, 3), (1, 12, 5, 1, 33), (2, 64, 7, 9, 64), (1, 8, 3, 33, 130))
CONV3_NCHW_SHAPES = ((2, 12, 5, 6, 64), (1, 64, 7, 9, 64), (1, 8, 4, 4, 33))
TRAIN_SHAPE = (35, 20, 7)                       # x (35, 20), w (7, 20)


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


# ---------------------------------------------------------------------------------------------------------------------------
# float64 definitions and bounds
# ---------------------------------------------------------------------------------------------------------------------------
def _sum64(a, a2):
    return a.double() if a2 is None else a.double() + a2.double()


def linear64(a, a2, w, bias, act):
    """act((a + a2) w^T + bias) in float64; bias is anything that broadcasts against (..., N)."""
    y = _sum64(a, a2) @ w.double().T
    if bias is not None:
        y = y + bias.double()
    return F.relu(y) if act == "relu" else y


def linear_tol(a, a2, w, bias):
    K = a.shape[-1]
    mag = _sum64(a, a2).abs() @ w.double().abs().T
    if bias is not None:
        mag = mag + bias.double().abs()
    return 2.0 * (K + 4) * U32 * mag


def _conv1x1_bias(y, bias, out):
    """y (B, HW, Cout); bias (Cout,) per channel or (HW, Cout) per position, the same matrix for every image."""
    if bias is not None:
        y = y + bias.double()
    return y if out == "tokens" else y.transpose(1, 2)


def conv1x1_64(x, w, bias=None, out="tokens"):
    """1x1 convolution of x (B, Cin, H, W) with w (Cout, Cin) in float64: (B, HW, Cout) tokens or (B, Cout, HW)."""
    y = F.conv2d(x.double(), w.double()[:, :, None, None]).flatten(2).transpose(1, 2)
    return _conv1x1_bias(y, bias, out)


def conv1x1_tol(x, w, bias=None, out="tokens"):
    mag = F.conv2d(x.double().abs(), w.double().abs()[:, :, None, None]).flatten(2).transpose(1, 2)
    return 2.0 * (x.shape[1] + 4) * U32 * _conv1x1_bias(mag, None if bias is None else bias.abs(), out)


def conv3x3_64(x, w, bias=None, out="tokens"):
    """3x3 / pad 1 convolution of x (B, Cin, H, W) with w (Cout, Cin, 3, 3) and a per-channel bias, F.conv2d in float64."""
    y = F.conv2d(x.double(), w.double(), None if bias is None else bias.double(), padding=1).flatten(2)
    return y.transpose(1, 2) if out == "tokens" else y


def conv3x3_tol(x, w, bias=None, out="tokens"):
    mag = F.conv2d(x.double().abs(), w.double().abs(), None if bias is None else bias.double().abs(), padding=1).flatten(2)
    return 2.0 * (9 * x.shape[1] + 4) * U32 * (mag.transpose(1, 2) if out == "tokens" else mag)


def outside(got, ref, tol):
    """Number of elements of ``got`` outside the bound (a NaN or inf in ``got`` is outside)."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape == tol.shape, (got.shape, ref.shape, tol.shape)
    return int((~((got - ref).abs() <= tol)).sum())


def ratio(got, ref, tol):
    """max error / tol over the elements with tol > 0: how much of the derived bound a result uses (reported, never asserted)."""
    err = (got.detach().cpu().double() - ref).abs()
    ok = tol > 0
    return float((err[ok] / tol[ok]).max()) if bool(ok.any()) else 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# seeded inputs (fp32, on the CPU); unit activations, weights scaled K^-0.5, unit biases
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def linear_inputs(M, N, K):
    return rnd(M, K, seed=101), rnd(N, K, seed=102, scale=K ** -0.5), rnd(N, seed=103)


@functools.lru_cache(maxsize=None)
def a2_inputs(B, L, K, N):
    """a (B, L, K), a2 of a's shape, a2 (L, K) broadcast over B, w, bias"""
    return (rnd(B, L, K, seed=111), rnd(B, L, K, seed=112), rnd(L, K, seed=113), rnd(N, K, seed=114, scale=K ** -0.5),
            rnd(N, seed=115))


@functools.lru_cache(maxsize=None)
def conv1x1_inputs(B, Cin, H, W, Cout):
    """x (B, Cin, H, W), w (Cout, Cin), vector bias (Cout,), matrix bias (HW, Cout)"""
    return (rnd(B, Cin, H, W, seed=121), rnd(Cout, Cin, seed=122, scale=Cin ** -0.5), rnd(Cout, seed=123),
            rnd(H * W, Cout, seed=124))


def mcontig_bias(inputs, kind):
    return {"none": None, "vector": inputs[2], "matrix": inputs[3]}[kind]


@functools.lru_cache(maxsize=None)
def conv3x3_inputs(B, Cin, H, W, Cout):
    """x (B, Cin, H, W), w (Cout, Cin, 3, 3), bias (Cout,)"""
    return rnd(B, Cin, H, W, seed=131), rnd(Cout, Cin, 3, 3, seed=132, scale=(9 * Cin) ** -0.5), rnd(Cout, seed=133)


def tokens(x):
    """(B, C, H, W) -> NHWC tokens (B, HW, C), contiguous"""
    return x.flatten(2).transpose(1, 2).contiguous()


def tap_major(w):
    """(Cout, Cin, 3, 3) -> (Cout, 9 * Cin) with k = (ky * 3 + kx) * Cin + c, the implicit GEMM's K order"""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


@functools.lru_cache(maxsize=None)
def train_inputs():
    M, K, N = TRAIN_SHAPE
    return rnd(M, K, seed=141), rnd(N, K, seed=142, scale=K ** -0.5), rnd(N, seed=143), rnd(M, N, seed=144)


# ---------------------------------------------------------------------------------------------------------------------------
# the host's dispatch, restated: which K range a split owns and which kernel instantiation a call takes
# ---------------------------------------------------------------------------------------------------------------------------
def split_ranges(K, split_k):
    """[k0, k1) per split as msm_gemm_f32 cuts K: whole 32-deep sub-tiles per split, the last one takes what is left.  None when
    the library rejects the split (its last part would be empty)."""
    kps = -(-(-(-K // split_k)) // 32) * 32
    if kps * (split_k - 1) >= K:
        return None
    return [(s * kps, min(K, (s + 1) * kps)) for s in range(split_k)]


def instantiation(amode, swap, M, N, K, batch=1, split_k=1, *, vec=True, a2=False, tile=AUTO, shallow=AUTO):
    """(MI, NI, AMODE, SWAP, VEC, HAS_A2, KT) of gemm_kernel for a call, following launch_gemm_o: M, N, K, batch are the library
    call's (for conv1x1_tokens_to_nchw M = Cout, N = HW), ``vec`` whether both operands qualify for 16-byte loads."""
    if not vec:
        return (1, 1, amode, swap, False, a2, 1)
    pick, best, fallback = -1, -1, 4
    for c in range(2, 5):
        bm, bn = 32 * TILE_MN[c][0], 32 * TILE_MN[c][1]
        gm, gn = -(-M // bm), -(-N // bn)
        waste = 1.0 - M * N / (gm * bm * gn * bn)
        blocks = gm * gn * batch * split_k
        if waste > 0.2 and c < 4:
            continue
        if blocks >= 512:
            pick = c
            break
        if blocks > best:
            best, fallback = blocks, c
    if pick < 0:
        pick = fallback
    if 0 <= tile <= 4:
        pick = tile
    kps = split_ranges(K, split_k)[0][1] if split_k > 1 else -(-K // 32) * 32
    deep = amode == 0 and pick >= 3 and kps >= 128 and shallow != 1
    return TILE_MN[pick] + (amode, swap, True, a2, 4 if deep else 1)


def all_instantiations():
    """Every instantiation the library's entry points can launch (ops.py's wrappers fix SWAP per A mode, except that a one-pixel
    map makes conv1x1_tokens_to_nchw's output row-major)."""
    out = set()
    for amode, swap, a2 in ((0, True, False), (0, True, True), (0, False, False), (1, True, False), (2, True, False), (2, False, False)):
        for mi, ni in TILE_MN:
            out.add((mi, ni, amode, swap, True, a2, 1))
        if amode == 0:
            out.add((1, 2, 0, swap, True, a2, 4))
            out.add((1, 1, 0, swap, True, a2, 4))
    for amode, swap, a2 in ((0, True, False), (0, True, True), (0, False, False), (1, True, False)):
        out.add((1, 1, amode, swap, False, a2, 1))
    return out


def table_instantiations():
    """instantiation -> number of (case, option) combinations of the tables above that launch it (epilogue variants and repeated
    launches of one combination count once)."""
    count = {}

    def add(key):
        count[key] = count.get(key, 0) + 1

    for tile in TILES:
        for shallow in SHALLOWS:
            opt = dict(tile=tile, shallow=shallow)
            for M, N, K in LINEAR_SHAPES:
                add(instantiation(0, True, M, N, K, vec=K % 4 == 0, **opt))
            for K, s in SPLITK_CASES:
                add(instantiation(0, True, *SPLITK_MN, K, split_k=s, vec=K % 4 == 0, **opt))
            for B, Cin, H, W, Cout in MCONTIG_SHAPES:
                add(instantiation(1, True, H * W, Cout, Cin, B, vec=(H * W) % 4 == 0 and Cin % 4 == 0, **opt))
            for B, HW, Cin, Cout in NCHW_SHAPES:
                add(instantiation(0, HW == 1, Cout, HW, Cin, B, vec=Cin % 4 == 0, **opt))
            for B, Cin, H, W, Cout in CONV3_TOKEN_SHAPES:
                add(instantiation(2, True, H * W, Cout, 9 * Cin, B, **opt))
            for B, Cin, H, W, Cout in CONV3_NCHW_SHAPES:
                add(instantiation(2, False, H * W, Cout, 9 * Cin, B, **opt))
    for tile in A2_TILES:
        for shallow in SHALLOWS:
            for B, L, K, N in A2_SHAPES:
                add(instantiation(0, True, B * L, N, K, 1, a2=True, tile=tile, shallow=shallow))      # a2 of a's shape: one batch
                add(instantiation(0, True, L, N, K, B, a2=True, tile=tile, shallow=shallow))          # a2 broadcast: batch B
    for M, N, K in MISALIGN_SHAPES:
        for _ in MISALIGN_WHICH:
            add(instantiation(0, True, M, N, K, vec=False))                                           # misaligned pointers
    for B, L, K, N in A2_SHAPES:
        add(instantiation(0, True, B * L, N, K, vec=False, a2=True))                                  # misaligned a2
    return count
