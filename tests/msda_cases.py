"""Cases shared by tests/test_msda_cases_cpu.py and tests/test_gpu_msda.py (not a test module): the geometries that reach every
multi-scale deformable attention kernel (csrc/msda.hip, csrc/msda_generic.hip, the fp16 gathers of csrc/enc_lp.hip), seeded
inputs that sit ON the map borders, the float64 definition, the error bound and the host dispatch restated.  Needs no GPU.

THE DEFINITION is ``oracle.msm_oracle.ms_deform_attn_core`` evaluated in float64 on the fp32 inputs.  For the encoder forms the
sampling locations ``ref + off / (W, H)`` (the module's order, ref = pixel centre / size) and the softmax over the L*P logits are
computed in float64 as well; for the decoder form ``loc`` and ``aw`` are themselves the fp32 inputs.

THE BOUND is derived, never measured, per output element, in float64 (u = 2^-24; ``bound`` takes u so that the float64 kernels get
the same expression with u = 2^-53).  out[b,q,m,d] = sum_i a_i s_i with s_i the zero-padded bilinear sample of point i.

  location   The kernels form x = (ref + off * (1/W)) * W - 0.5 per axis: ref = (r + 0.5) / W (one rounding, <= u (|x| + |off| + 1)
             pixels once multiplied by W), off / W through a reciprocal within 1 ulp and a Newton step (2 u |off|), the sum
             (u (|x| + 0.5)), the product (u (|x| + 0.5)) and the subtraction (u |x|): five roundings,
                 delta = 5 u (|x| + |off| + 1)     pixels, per axis.
             The decoder form rounds only the product and the subtraction (off = 0 in the same expression).
  Lipschitz  The zero-padded bilinear sample is continuous and piecewise linear; its slope along an axis is a blend of differences
             of neighbouring pixels (the zero padding included), <= lip = 2 max|v| over the level for this (image, head, channel).
             A point further than ONE pixel outside the support (-1, size) on either axis samples nothing, exactly and with any
             delta < 1: it contributes nothing.  Otherwise the sample moves by <= lip (delta_x + delta_y).
  softmax    a_i = e_i / sum_j e_j, e_i = exp(l_i - max): the argument's rounding and the scaling by log2 e change e_i by
             2 (max - l_i) u relative, the exponential itself by <= 2 ulp; the denominator's L*P additions give L*P u and its terms'
             errors sum_j a_j 2 (max - l_j) u <= 2 L*P / e u; the reciprocal and the product 4 u:
                 rel_i = (2 (max - l_i) + L*P + c) u,   c = L*P + 8.
  dot        bilinear weights (1 - lh, the two products, times a_i: <= 6 roundings relative to w_k |v_k|; the absolute rounding of
             1 - lh, <= u |v|, is inside the Lipschitz term, whose delta >= 5 u) and L*P accumulations in any order:
             (L*P + 8) u sum_i a_i sum_k w_k |v_k|.

      tol = 2 * ( sum_i a_i near_i lip (delta_x + delta_y)  +  sum_i a_i (rel_i + (L*P + 8) u) sum_k w_k |v_k| )

with a factor two of margin, ``sum_k w_k |v_k|`` from the oracle applied to |value|, plus an underflow floor: a softmax weight of
a row whose logits spread over +-60 is below the smallest normal number, where an operation no longer rounds relatively but by up
to 2^-126 (denormal results flushed; 2^-1022 in float64) -- 8 L*P operations per element, scaled by max(1, max|v|).  A comparison is
``(got.double() - ref).abs() <= tol`` on EVERY element; there is no rtol / atol pair and no share of elements is left out.

fp16 gathers: the definition is the same on the fp16-rounded value and the offsets / fp16-rounded logits the kernel reads; the kernel
accumulates fp32 products of fp32 weights, so the bound gains only the result's rounding, 2^-11 (|ref| + tol) + 2^-24 (the
smallest subnormal).  With the projection computed in the kernel from bf16 hi + lo pairs of src + pos, every projected value carries
2^-17 relative: delta gains 2^-17 |off| and rel_i gains 2^-17 * 2 (|l_i| + |max|).

Backward (kink-free inputs: every coordinate >= 2^-6 from an integer, so no tap changes cell under a perturbation delta << 2^-6;
the definition is float64 autograd through the oracle; T = D + 8 roundings per channel sum):
  grad_value[s]       sum over the taps that hit s of go a w_k: each term (8 + n_s) u relative (n_s atomics in any order) plus
                      |go| a (delta_x + delta_y) since |dw_k / dx| <= 1;
  grad_attn_weight    sum_d go_d s_d: T u sum_d |go_d| sum_k w_k |v_k| + sum_d |go_d| lip_d (delta_x + delta_y);
  grad_sampling_loc   x: W a sum_d go_d ds_d/dx with ds/dx = (1 - lh)(v2 - v1) + lh (v4 - v3), constant in x inside a cell and
                      |d2 s / dx dy| <= 2 lip: W a sum_d |go_d| (T u sum_k |c_k| |v_k| + 2 lip_d delta_y); y alike,
each with the factor two of margin and the underflow floor of its operation count, scaled by max(1, max|go|) max(1, max|v|) and
(W, H)."""
import collections
import functools
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import msm_oracle as O  # noqa: E402

U32, U64 = 2.0 ** -24, 2.0 ** -53
TINY = {U32: 2.0 ** -126, U64: 2.0 ** -1022}       # smallest normal number per unit roundoff
AUTO = -1
MAXL = 8
KINK = 2.0 ** -6

LEVELS_A = ((5, 7), (3, 4), (1, 2))             # S = 49: less than one workgroup of 64 queries, not a multiple of 16, a one-row level
LEVELS_B = ((9, 1), (1, 1), (2, 3))             # S = 16: a one-column level and a one-pixel level
LEVELS_C = ((8, 12), (4, 6), (2, 3))            # S = 126: two workgroups, the second one partial
LEVELS_WIDE = ((15, 20), (8, 10), (4, 5))       # CPU only: the geometry of the bound's scratch run


def levels_of(base, L):
    """``base`` cut or extended (cyclically) to L levels"""
    return tuple(base[i % len(base)] for i in range(L))


# form "enc": the encoder self-attention (queries = the S pixels), run token-major and head-major; "dec": ops.ms_deform_attn
Case = collections.namedtuple("Case", "name form levels B M D P Lq seed")


def _enc(name, levels, B, M, D, P, seed):
    return Case(name, "enc", tuple(levels), B, M, D, P, sum(h * w for h, w in levels), seed)


PIXDEC_CASES = tuple(_enc(f"pd_{n}_B{B}", lv, B, 8, 8, 4, 10 + 2 * i + (B == 3))
                     for i, (n, lv) in enumerate((("A", LEVELS_A), ("B", LEVELS_B), ("C", LEVELS_C))) for B in (1, 3))
HM8_CASES = tuple(_enc(f"hm8_L{L}P{P}_M{M}", levels_of(LEVELS_A if M == 1 else LEVELS_B, L), 2, M, 8, P, 130 + 4 * i + M)
                  for i, (L, P) in enumerate(((1, 1), (2, 2), (4, 4), (8, 2))) for M in (1, 3))
HM4_CASES = (_enc("hm_D16", LEVELS_A, 2, 2, 16, 4, 50), _enc("hm_D32", LEVELS_B, 2, 2, 32, 4, 51),
             _enc("hm_D8_L5P4", levels_of(LEVELS_A, 5), 2, 3, 8, 4, 52))
HM1_CASES = (_enc("hm_D1", LEVELS_A, 2, 3, 1, 4, 53), _enc("hm_D2", LEVELS_B, 2, 3, 2, 4, 54))
TM_CASES = (_enc("tm_D6", LEVELS_A, 2, 3, 6, 4, 55),)         # D = 6: token-major only; head-major must reject it (256 % 12 != 0)
ENC_CASES = PIXDEC_CASES + HM8_CASES + HM4_CASES + HM1_CASES + TM_CASES
HM_REJECT = TM_CASES[0]

DEC_CASES = (Case("dec_D8_Lq7", "dec", LEVELS_A, 2, 2, 8, 4, 7, 60), Case("dec_D8_Lq1", "dec", LEVELS_B, 2, 2, 8, 4, 1, 61),
             Case("dec_D6_Lq7", "dec", LEVELS_B, 2, 2, 6, 4, 7, 62), Case("dec_D71_Lq7", "dec", LEVELS_A, 2, 2, 71, 4, 7, 63),
             Case("dec_L9_Lq7", "dec", levels_of(LEVELS_A, 9), 2, 2, 8, 2, 7, 64), Case("dec_L9_Lq1", "dec", levels_of(LEVELS_B, 9), 1, 2, 8, 2, 1, 65))
FWD_CASES = ENC_CASES + DEC_CASES

BWD_LEVELS = (((5, 7), (1, 2)), LEVELS_B)
BWD_CASES = tuple(Case(f"bwd_D{D}_L{len(lv)}", "bwd", tuple(lv), 2, 2, D, 2, 7, 70 + i)
                  for i, (D, lv) in enumerate(((8, BWD_LEVELS[0]), (64, BWD_LEVELS[1]), (24, BWD_LEVELS[0]), (2, BWD_LEVELS[1]),
                                               (6, BWD_LEVELS[0]), (71, BWD_LEVELS[1]), (8, levels_of(BWD_LEVELS[0], 9)))))
CPU_ONLY_CASES = (_enc("pd_wide_B1", LEVELS_WIDE, 1, 8, 8, 4, 90),)

OPTIONS = (AUTO, 1, 2, 3)                       # MSM_OPT_MSDA_GENERIC


def by_name(name):
    return next(c for c in FWD_CASES + BWD_CASES + CPU_ONLY_CASES if c.name == name)


def shapes_start(levels):
    shapes = torch.tensor(levels, dtype=torch.int64)
    start = torch.cat((shapes.new_zeros(1), shapes.prod(1).cumsum(0)[:-1]))
    return shapes, start


def sizes(levels):
    """(L, 2) float32: (W, H) per level, the divisor of an (x, y) offset"""
    return torch.tensor([[w, h] for h, w in levels], dtype=torch.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# seeded inputs
# ---------------------------------------------------------------------------------------------------------------------------
def encoder_ref(levels):
    """(S, 2) fp32 reference points of the encoder's queries (pixel centres / size, as O.encoder_reference_points) and their
    float64 twin"""
    r32 = O.encoder_reference_points(levels, 1)[0, :, 0]
    r64 = []
    for H, W in levels:
        gy, gx = torch.meshgrid((torch.arange(H, dtype=torch.float64) + 0.5) / H, (torch.arange(W, dtype=torch.float64) + 0.5) / W, indexing="ij")
        r64.append(torch.stack((gx.reshape(-1), gy.reshape(-1)), -1))
    return r32, torch.cat(r64, 0)


def structured_offsets(ref, levels, M, P, g, kink_free=False):
    """ref (B, Q, 2) fp32 -> offsets (B, Q, M, L, P, 2) fp32, per coordinate from a target pixel coordinate on the sampled level,
    off = target - (ref * size - 0.5) in fp32: 40 % target uniform in [-1.5, size + 0.5); 20 % target one of -1, -0.5, 0, size - 1,
    size - 0.5, size; 20 % the offset itself one of -2, -1.5 .. 2 (exact integer / half-integer coordinates on the query's own level);
    10 % far outside, +-(size + 2 + U * 1e4); 10 % Gaussian offsets, sigma 3.  kink_free: every target is moved to at least
    1.5 * 2^-6 from an integer (the backward's variant; -1 and size are integers)."""
    B, Q, _ = ref.shape
    L = len(levels)
    shape = (B, Q, M, L, P, 2)
    size = sizes(levels)[None, None, None, :, None, :].expand(shape)
    base = ref[:, :, None, None, None, :] * size - 0.5                                     # fp32: the query's pixel coordinate on the level
    cls = torch.rand(shape, generator=g)
    u1, u2 = torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    pick6 = torch.randint(0, 6, shape, generator=g)
    pick9 = torch.randint(0, 9, shape, generator=g)
    gauss = torch.randn(shape, generator=g) * 3.0
    t_uniform = -1.5 + u1 * (size + 2.0)
    t_edge = torch.stack((torch.full(shape, -1.0), torch.full(shape, -0.5), torch.zeros(shape), size - 1.0, size - 0.5, size), -1)
    t_edge = t_edge.gather(-1, pick6[..., None])[..., 0]
    far = torch.where(u2 < 0.5, -1.0, 1.0) * (size + 2.0 + u1 * 1e4)
    target = torch.where(cls < 0.4, t_uniform, torch.where(cls < 0.6, t_edge, torch.where(cls < 0.8, base + (pick9.float() * 0.5 - 2.0),
                         torch.where(cls < 0.9, base + far, base + gauss))))
    if kink_free:
        nearest = torch.round(target)
        d = target - nearest
        push = 1.5 * KINK
        target = torch.where(d.abs() < push, nearest + torch.where(d < 0, -push, push), target)
    return (target - base).contiguous()


def structured_logits(B, Q, M, LP, g):
    """(B, Q, M, LP) fp32, a class per (query, head), a quarter each: all equal, randn * 20 (spread over +-60), randn + 60 (all
    shifted by a large constant), plain randn"""
    cls = torch.randint(0, 4, (B, Q, M, 1), generator=g)
    r = torch.randn(B, Q, M, LP, generator=g)
    return torch.where(cls == 0, r[..., :1].expand_as(r), torch.where(cls == 1, r * 20.0, torch.where(cls == 2, r + 60.0, r))).contiguous()


Inputs = collections.namedtuple("Inputs", "value off logits ref32 ref64 proj loc aw")


@functools.lru_cache(maxsize=None)
def inputs(case, kink_free=False):
    """value (B, S, M, D) token-major fp32 randn (every pixel distinct); off (B, Q, M, L, P, 2); logits (B, Q, M, L*P); the fp32 and
    float64 reference points (B or 1, Q, 2); proj (B, S, M*L*P*3) = [offsets | logits], the encoder entry points' input; loc
    (B, Q, M, L, P, 2) = ref + off / (W, H) and aw = softmax(logits) in fp32, the decoder entry point's inputs, from the same draws"""
    g = torch.Generator().manual_seed(case.seed)
    L, LP = len(case.levels), len(case.levels) * case.P
    S = sum(h * w for h, w in case.levels)
    value = torch.randn(case.B, S, case.M, case.D, generator=g)
    if case.form == "enc":
        r32, r64 = encoder_ref(case.levels)
        r32, r64 = r32[None], r64[None]
    else:
        r32 = torch.rand(case.B, case.Lq, 2, generator=g)
        r64 = r32.double()
    off = structured_offsets(r32.expand(case.B, -1, -1), case.levels, case.M, case.P, g, kink_free)
    logits = structured_logits(case.B, case.Lq, case.M, LP, g)
    proj = torch.cat((off.reshape(case.B, case.Lq, -1), logits.reshape(case.B, case.Lq, -1)), -1).contiguous()
    loc = (r32[:, :, None, None, None, :] + off / sizes(case.levels)[None, None, None, :, None, :]).contiguous()
    aw = torch.softmax(logits, -1).view(case.B, case.Lq, case.M, L, case.P).contiguous()
    return Inputs(value, off, logits, r32, r64, proj, loc, aw)


def split_proj(proj, M, L, P):
    """[offsets | logits] columns -> off (B, S, M, L, P, 2), logits (B, S, M, L*P)"""
    B, S, _ = proj.shape
    n = M * L * P
    return proj[..., :2 * n].reshape(B, S, M, L, P, 2), proj[..., 2 * n:].reshape(B, S, M, L * P)


def head_major(value):
    """(B, S, M, D) -> (B, M, S, D) contiguous"""
    return value.permute(0, 2, 1, 3).contiguous()


# ---------------------------------------------------------------------------------------------------------------------------
# the float64 definition and the bound
# ---------------------------------------------------------------------------------------------------------------------------
def loc64(ref64, off, levels):
    """the module's ``ref + off / (W, H)`` in float64 on the fp32 offsets"""
    return ref64[:, :, None, None, None, :] + off.double() / sizes(levels).double()[None, None, None, :, None, :]


def softmax64(logits, L, P):
    return torch.softmax(logits.double(), -1).view(*logits.shape[:-1], L, P)


def pixel_coords(loc, levels):
    """loc (..., L, P, 2) float64 -> pixel coordinates (w_im, h_im) = loc * (W, H) - 0.5"""
    return loc * sizes(levels).double()[:, None, :] - 0.5


def bound(value, levels, loc, aw, off=None, logits=None, u=U32, off_rel=0.0, logit_rel=0.0):
    """tol (B, Q, M*D) float64 for the forward, see the module docstring.  loc, aw float64; off None: the decoder form; logits None:
    the attention weights are inputs.  off_rel / logit_rel: relative error the projected offsets / logits already carry."""
    B, S, M, D = value.shape
    _, Q, _, L, P, _ = loc.shape
    LP = L * P
    xy = pixel_coords(loc, levels)
    size = sizes(levels).double()[:, None, :]
    aoff = torch.zeros_like(xy) if off is None else off.double().abs()
    delta = 5.0 * u * (xy.abs() + aoff + 1.0) + off_rel * aoff
    near = ((xy >= -2.0) & (xy <= size + 1.0)).all(-1)                                      # not further than one pixel outside (-1, size)
    dsum = delta.sum(-1) * near                                                             # (B, Q, M, L, P)
    lip = torch.stack([2.0 * value[:, s0:s0 + h * w].double().abs().amax(1) for (h, w), s0 in zip(levels, shapes_start(levels)[1].tolist())], 1)   # (B, L, M, D)
    move = torch.einsum("bqmlp,blmd->bqmd", aw * dsum, lip)
    rel = torch.full_like(aw, (LP + 8) * u)
    if logits is not None:
        lg = logits.double()
        mx = lg.amax(-1, keepdim=True)
        rs = (2.0 * (mx - lg) + LP + (LP + 8)) * u + logit_rel * 2.0 * (lg.abs() + mx.abs())
        rel = rel + rs.view(B, Q, M, L, P)
    mag = O.ms_deform_attn_core(value.double().abs(), levels, loc, aw * rel)
    return 2.0 * (move.reshape(B, Q, M * D) + mag) + 8 * LP * TINY[u] * max(1.0, float(value.abs().max()))


def definition(case, inp=None):
    """(ref, tol) of a forward case, float64 (B, Q, M*D)"""
    inp = inp or inputs(case)
    L = len(case.levels)
    if case.form == "enc":
        loc, aw = loc64(inp.ref64, inp.off, case.levels), softmax64(inp.logits, L, case.P)
        return O.ms_deform_attn_core(inp.value.double(), case.levels, loc, aw), bound(inp.value, case.levels, loc, aw, inp.off, inp.logits)
    loc, aw = inp.loc.double(), inp.aw.double()
    return O.ms_deform_attn_core(inp.value.double(), case.levels, loc, aw), bound(inp.value, case.levels, loc, aw)


@functools.lru_cache(maxsize=None)
def forward_ref(case):
    return definition(case)


def encoder_ref_from_proj(value, levels, proj, M, P, off_rel=0.0, logit_rel=0.0):
    """(ref, tol) of an encoder form whose offsets / logits are the columns ``proj`` (B, S, M*L*P*3), fp32 or float64"""
    L = len(levels)
    off, logits = split_proj(proj, M, L, P)
    _, r64 = encoder_ref(levels)
    loc, aw = loc64(r64[None], off, levels), softmax64(logits, L, P)
    return (O.ms_deform_attn_core(value.double(), levels, loc, aw),
            bound(value, levels, loc, aw, off, logits, off_rel=off_rel, logit_rel=logit_rel))


def fp16_result_tol(ref, tol):
    """the bound of a result rounded to fp16: one rounding of the result plus the smallest subnormal"""
    return tol + 2.0 ** -11 * (ref.abs() + tol) + 2.0 ** -24


def outside(got, ref, tol):
    """Number of elements of ``got`` outside the bound (a NaN or inf in ``got`` is outside)."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape == tol.shape, (got.shape, ref.shape, tol.shape)
    return int((~((got - ref).abs() <= tol)).sum())


def ratio(got, ref, tol):
    """max error / tol over the elements with tol > 0: the share of the derived bound a result uses (reported, never asserted)."""
    err = (got.detach().cpu().double() - ref).abs()
    ok = tol > 0
    return float((err[ok] / tol[ok]).max()) if bool(ok.any()) else 0.0


def worst(got, ref, tol):
    """(flat index, error, tol) of the element that uses most of its bound"""
    err = (got.detach().cpu().double() - ref).abs()
    r = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    i = int(r.argmax())
    return i, float(err.reshape(-1)[i]), float(tol.reshape(-1)[i])


def coverage(loc, levels):
    """shares of the sampling points of loc (float64): inside the support (-1, size) on both axes; of all points, those in the border
    band (inside the support with a coordinate below 0 or above size - 1); clearly outside (further than one pixel from the support
    on either axis)"""
    xy = pixel_coords(loc, levels)
    size = sizes(levels).double()[:, None, :]
    inside = ((xy > -1.0) & (xy < size)).all(-1)
    band = inside & ((xy < 0.0) | (xy > size - 1.0)).any(-1)
    out = ((xy < -2.0) | (xy > size + 1.0)).any(-1)
    n = inside.numel()
    return dict(inside=float(inside.sum()) / n, band=float(band.sum()) / n, outside=float(out.sum()) / n)


def kink_distance(loc, levels):
    """smallest distance of a pixel coordinate of loc (float64) from an integer"""
    xy = pixel_coords(loc, levels)
    return float((xy - torch.round(xy)).abs().min())


# ---------------------------------------------------------------------------------------------------------------------------
# a restatement of the op with the mistakes a kernel could make (the wrong references of the CPU test); plain = the oracle
# ---------------------------------------------------------------------------------------------------------------------------
def core_variant(value, levels, loc, aw, right_column=False, half_pixel=True):
    """ms_deform_attn_core in the dtype of its inputs.  right_column: the tap column index W is accepted and reads the clamped pixel
    W - 1; half_pixel False: the -0.5 shift is dropped."""
    N, S, M, D = value.shape
    _, Lq, _, L, P, _ = loc.shape
    out = torch.zeros(N, Lq, M, D, dtype=value.dtype)
    n_idx = torch.arange(N)[:, None, None, None]
    m_idx = torch.arange(M)[None, None, :, None]
    start = 0
    for lid, (H, W) in enumerate(levels):
        v = value[:, start:start + H * W]
        start += H * W
        shift = 0.5 if half_pixel else 0.0
        wim, him = loc[:, :, :, lid, :, 0] * W - shift, loc[:, :, :, lid, :, 1] * H - shift
        inside = (him > -1) & (wim > -1) & (him < H) & (wim < W)
        h0, w0 = torch.floor(him), torch.floor(wim)
        lh, lw = him - h0, wim - w0
        h0, w0 = h0.long(), w0.long()
        acc = torch.zeros(N, Lq, M, P, D, dtype=value.dtype)
        for dh, dw, wt in ((0, 0, (1 - lh) * (1 - lw)), (0, 1, (1 - lh) * lw), (1, 0, lh * (1 - lw)), (1, 1, lh * lw)):
            hh, ww = h0 + dh, w0 + dw
            ok = inside & (hh >= 0) & (hh <= H - 1) & (ww >= 0) & (ww <= (W if right_column else W - 1))
            g = v[n_idx, hh.clamp(0, H - 1) * W + ww.clamp(0, W - 1), m_idx]
            acc = acc + g * (wt * ok)[..., None]
        out = out + (acc * aw[:, :, :, lid][..., None]).sum(3)
    return out.reshape(N, Lq, M * D)


WRONG = ("right_column", "no_half_pixel", "swapped_sizes", "softmax_per_level")


def wrong_forward(case, which, inp=None):
    """float64 result of a wrong reference on a forward case, or None where the mistake is not expressible"""
    inp = inp or inputs(case)
    L = len(case.levels)
    v = inp.value.double()
    enc = case.form == "enc"
    loc = loc64(inp.ref64, inp.off, case.levels) if enc else inp.loc.double()
    aw = softmax64(inp.logits, L, case.P) if enc else inp.aw.double()
    if which == "right_column":
        return core_variant(v, case.levels, loc, aw, right_column=True)
    if which == "no_half_pixel":
        return core_variant(v, case.levels, loc, aw, half_pixel=False)
    if which == "swapped_sizes":                # offsets divided by (H, W): the glue of the encoder forms
        if not enc or all(h == w for h, w in case.levels):
            return None
        hw = torch.tensor([[h, w] for h, w in case.levels], dtype=torch.float64)
        return O.ms_deform_attn_core(v, case.levels, inp.ref64[:, :, None, None, None, :] + inp.off.double() / hw[None, None, None, :, None, :], aw)
    if which == "softmax_per_level":
        if not enc or L == 1:
            return None
        lg = inp.logits.double().view(case.B, case.Lq, case.M, L, case.P)
        return O.ms_deform_attn_core(v, case.levels, loc, torch.softmax(lg, -1) / L)
    raise KeyError(which)


# ---------------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------------
BwdInputs = collections.namedtuple("BwdInputs", "value loc aw go")


@functools.lru_cache(maxsize=None)
def bwd_inputs(case):
    """the kink-free draws of a backward case as the decoder form's fp32 inputs, and grad_output (B, Lq, M*D) randn"""
    inp = inputs(case, kink_free=True)
    go = torch.randn(case.B, case.Lq, case.M * case.D, generator=torch.Generator().manual_seed(case.seed + 1000))
    return BwdInputs(inp.value, inp.loc, inp.aw, go)


def autograd64(case, b=None):
    """(grad_value, grad_sampling_loc, grad_attn_weight): float64 autograd through the oracle"""
    b = b or bwd_inputs(case)
    v, loc, aw = (t.double().requires_grad_(True) for t in (b.value, b.loc, b.aw))
    O.ms_deform_attn_core(v, case.levels, loc, aw).backward(b.go.double())
    return v.grad, loc.grad, aw.grad


def bwd_bound(case, b=None, u=U32):
    """(tol_value, tol_loc, tol_weight) float64, see the module docstring"""
    b = b or bwd_inputs(case)
    B, S, M, D = b.value.shape
    _, Lq, _, L, P, _ = b.loc.shape
    v, loc, aw = b.value.double(), b.loc.double(), b.aw.double()
    ago = b.go.double().abs().view(B, Lq, M, 1, D)
    T = (D + 8) * u
    tv, tl, tw = torch.zeros_like(v), torch.zeros_like(loc), torch.zeros_like(aw)
    cnt = torch.zeros(B, S, M, 1, dtype=torch.float64)
    term = torch.zeros_like(v)                                                             # sum |go| a w_k per element
    slide = torch.zeros_like(v)                                                            # sum |go| a (delta_x + delta_y) per element
    n_idx = torch.arange(B)[:, None, None, None].expand(B, Lq, M, P)
    m_idx = torch.arange(M)[None, None, :, None].expand(B, Lq, M, P)
    xy = pixel_coords(loc, case.levels)
    delta = 5.0 * u * (xy.abs() + 1.0)
    start = 0
    for lid, (H, W) in enumerate(case.levels):
        va = v[:, start:start + H * W].abs()
        lip = 2.0 * va.amax(1)[:, None, :, None, :]                                        # (B, 1, M, 1, D)
        wim, him = xy[:, :, :, lid, :, 0], xy[:, :, :, lid, :, 1]
        dx, dy = delta[:, :, :, lid, :, 0], delta[:, :, :, lid, :, 1]
        inside = (him > -1) & (wim > -1) & (him < H) & (wim < W)
        h0, w0 = torch.floor(him), torch.floor(wim)
        lh, lw = him - h0, wim - w0
        h0, w0 = h0.long(), w0.long()
        a = aw[:, :, :, lid]
        sabs = torch.zeros(B, Lq, M, P, D, dtype=torch.float64)
        cxabs, cyabs = torch.zeros_like(sabs), torch.zeros_like(sabs)
        for dh, dw, wt, cx, cy in ((0, 0, (1 - lh) * (1 - lw), 1 - lh, 1 - lw), (0, 1, (1 - lh) * lw, 1 - lh, lw),
                                   (1, 0, lh * (1 - lw), lh, 1 - lw), (1, 1, lh * lw, lh, lw)):
            hh, ww = h0 + dh, w0 + dw
            ok = (inside & (hh >= 0) & (hh <= H - 1) & (ww >= 0) & (ww <= W - 1)).double()
            idx = hh.clamp(0, H - 1) * W + ww.clamp(0, W - 1)
            g = va[n_idx, idx, m_idx] * ok[..., None]
            sabs, cxabs, cyabs = sabs + g * wt[..., None], cxabs + g * cx[..., None], cyabs + g * cy[..., None]
            term[:, start:start + H * W].index_put_((n_idx, idx, m_idx), ago * (a * wt * ok)[..., None], accumulate=True)
            slide[:, start:start + H * W].index_put_((n_idx, idx, m_idx), ago * (a * (dx + dy) * ok)[..., None], accumulate=True)
            cnt[:, start:start + H * W].index_put_((n_idx, idx, m_idx), ok[..., None], accumulate=True)
        ins = inside.double()
        tw[:, :, :, lid] = (ago * (T * sabs + lip * (dx + dy)[..., None])).sum(-1) * ins
        tl[:, :, :, lid, :, 0] = W * a * (ago * (T * cxabs + 2.0 * lip * dy[..., None])).sum(-1) * ins
        tl[:, :, :, lid, :, 1] = H * a * (ago * (T * cyabs + 2.0 * lip * dx[..., None])).sum(-1) * ins
        start += H * W
    tv = (8.0 + cnt) * u * term + slide
    floor = TINY[u] * max(1.0, float(ago.max())) * max(1.0, float(v.abs().max()))
    return (2.0 * tv + (8.0 + cnt) * floor, 2.0 * tl + 8 * D * floor * sizes(case.levels).double()[:, None, :], 2.0 * tw + 8 * D * floor)


@functools.lru_cache(maxsize=None)
def backward_ref(case):
    return autograd64(case), bwd_bound(case)


# ---------------------------------------------------------------------------------------------------------------------------
# the host's dispatch, restated (msm_msdeform_attn_fwd / _enc_fwd / _bwd / _enc_hm_fwd / _enc_fused_fwd of csrc/msda.hip, the
# float64 entry points of csrc/msda_generic.hip, msm_msdeform_attn_enc_lp_fwd / _lp_fused_fwd of csrc/enc_lp.hip)
# ---------------------------------------------------------------------------------------------------------------------------
LAYOUTS = ("dec", "dec64", "tm", "hm", "fused", "lp", "lp_fused", "bwd", "bwd64")


def instantiation(layout, D, L, P, option=AUTO, M=8):
    """The kernel instantiation an entry point launches, or None where it rejects the call.  ``option`` is MSM_OPT_MSDA_GENERIC
    (read by the head-major encoder entry point only); M matters only to the fixed-geometry entry points (M * D = 64)."""
    V = 4 if D % 4 == 0 else 1
    generic = D > 64 or L > MAXL
    if layout == "dec64":
        return "msda_any_fwd_kernel<double>"
    if layout == "bwd64":
        return "msda_any_bwd_kernel<double>"
    if layout == "dec":
        return "msda_any_fwd_kernel<float>" if generic else f"msda_kernel<false,{V}>"
    if layout == "bwd":
        if generic:
            return "msda_any_bwd_kernel<float>"
        d4 = D // V
        return f"msda_bwd_kernel<{V},{'true' if d4 & (d4 - 1) == 0 else 'false'}>"
    if layout == "tm":
        return None if generic else f"msda_kernel<true,{V}>"
    if layout == "hm":
        if generic or 256 % (2 * (D // V)) != 0:
            return None
        if D == 8 and L * P <= 16 and option == 3:
            return "msda_enc_hm8_kernel<false,0,0>"
        if D == 8 and L == 3 and P == 4 and option == AUTO:
            return "msda_enc_hm8_rec_kernel<3,4>"
        if D == 8 and L == 3 and P == 4 and option != 1:
            return "msda_enc_hm8_kernel<true,3,4>"
        if D == 8 and L * P <= 16 and option != 1:
            return "msda_enc_hm8_kernel<true,0,0>"
        return f"msda_enc_hm_kernel<{V}>"
    fixed = D == 8 and M * D == 64 and L == 3 and P == 4
    if layout == "fused":
        return "msda_enc_hm8_fused_kernel<3,4>" if fixed else None
    if layout == "lp":
        return "msda_enc_lp_kernel<3,false>" if fixed else None
    if layout == "lp_fused":
        return "msda_enc_lp_kernel<3,true>" if fixed else None
    raise KeyError(layout)


ALL_INSTANTIATIONS = (
    "msda_kernel<false,4>", "msda_kernel<false,1>", "msda_kernel<true,4>", "msda_kernel<true,1>",
    "msda_enc_hm_kernel<4>", "msda_enc_hm_kernel<1>",
    "msda_enc_hm8_kernel<false,0,0>", "msda_enc_hm8_kernel<true,0,0>", "msda_enc_hm8_kernel<true,3,4>",
    "msda_enc_hm8_rec_kernel<3,4>", "msda_enc_hm8_fused_kernel<3,4>",
    "msda_bwd_kernel<4,true>", "msda_bwd_kernel<4,false>", "msda_bwd_kernel<1,true>", "msda_bwd_kernel<1,false>",
    "msda_any_fwd_kernel<float>", "msda_any_fwd_kernel<double>", "msda_any_bwd_kernel<float>", "msda_any_bwd_kernel<double>",
    "msda_enc_lp_kernel<3,false>", "msda_enc_lp_kernel<3,true>")


def runs(case):
    """[(layout, option)] a case goes through in tests/test_gpu_msda.py: every entry point and option that can take it"""
    L = len(case.levels)
    if case.form == "dec":
        return [("dec", AUTO), ("dec64", AUTO)]
    if case.form == "bwd":
        return [("bwd", AUTO), ("bwd64", AUTO)]
    out = [("tm", AUTO)] + [("hm", o) for o in OPTIONS]
    if case.M == 8 and case.D == 8 and L == 3 and case.P == 4:
        out += [("fused", AUTO), ("lp", AUTO), ("lp_fused", AUTO)]
    return out


def table_instantiations():
    """instantiation -> number of (case, entry point, option) combinations of the tables above that launch it"""
    count = {}
    for case in FWD_CASES + BWD_CASES:
        for layout, option in runs(case):
            k = instantiation(layout, case.D, len(case.levels), case.P, option, case.M)
            if k is not None:
                count[k] = count.get(k, 0) + 1
    return count


# ---------------------------------------------------------------------------------------------------------------------------
# the fused entry points: src, pos and a projection that reproduces structured offsets EXACTLY
# ---------------------------------------------------------------------------------------------------------------------------
Fused = collections.namedtuple("Fused", "src pos wp bp proj")


@functools.lru_cache(maxsize=None)
def fused_inputs(case):
    """The fused gathers compute proj = [sampling_offsets | attention_weights](src + pos) themselves, 288 values per token from 64
    features.  wp is a SELECTION matrix (one 1.0 per row, bias 0), so every projected value is one feature of src + pos, exactly,
    on any matrix pipe and in any k order (0 * x adds exact zeros).  The 64 features of a token are a pool of structured draws:
    feature l*16 + a*8 + k, k < 8, is a structured offset for level l, axis a (structured_offsets with one head and 8 points, so
    each keeps the class mix on ITS level); features 48..63 are 16 structured logits.  Head m, level l, point p reads x from
    k = (p + m) % 8, y from k = (p + 3 m + l) % 8, its logit i from 48 + (i + 5 m) % 16: every head gets its own combination.
    pos (S, 64) holds multiples of 0.25, src = pool - pos; the offsets the kernels see are fp32(src + pos), and ``proj`` is that
    selection (B, S, 288) in the unfused column order, for the definition and for the unfused kernels."""
    assert case.M == 8 and case.D == 8 and len(case.levels) == 3 and case.P == 4
    g = torch.Generator().manual_seed(case.seed + 500)
    S = case.Lq
    r32, _ = encoder_ref(case.levels)
    off = structured_offsets(r32[None].expand(case.B, -1, -1), case.levels, 1, 8, g)       # (B, S, 1, 3, 8, 2)
    pool = torch.cat((off[:, :, 0].permute(0, 1, 2, 4, 3).reshape(case.B, S, 48), structured_logits(case.B, S, 1, 16, g)[:, :, 0]), -1)
    pos = torch.randint(-8, 9, (S, 64), generator=g).float() * 0.25
    src = (pool - pos).contiguous()
    x = src + pos                                                                          # fp32: what the kernels compute
    sel = torch.zeros(288, dtype=torch.int64)
    for m in range(8):
        for l in range(3):
            for p in range(4):
                i = l * 4 + p
                sel[(m * 12 + i) * 2 + 0] = l * 16 + (p + m) % 8
                sel[(m * 12 + i) * 2 + 1] = l * 16 + 8 + (p + 3 * m + l) % 8
                sel[192 + m * 12 + i] = 48 + (i + 5 * m) % 16
    wp = torch.zeros(288, 64)
    wp[torch.arange(288), sel] = 1.0
    return Fused(src, pos, wp, torch.zeros(288), x[..., sel].contiguous())
