"""Cases shared by tests/test_msda_det_cases_cpu.py and tests/test_gpu_msda_deterministic.py (not a test module) for the
deterministic MSDeformAttn backward (csrc/msda_det.hip).  Imports tests/msda_cases.py as is: the float64 definition
(``autograd64``) and the derived per-element bound (``bwd_bound``) are that module's, unchanged.  Needs no GPU.

New backward cases (all ``Case(..., "bwd", ...)``, decoder-form inputs, M = 8, P = 4, B = 2):
  encoder form   Lq = S on LEVELS_C (S = 126: two workgroups, the second partial) and LEVELS_B (a one-column and a one-pixel level)
                 with D in {8, 32} (a power-of-two number of lanes per head), {24, 6} (D/V = 6 lanes, V = 4 and 1) and 64;
  pile-up        every sampling point of the first level of every query lies in ONE cell of that level, the other levels sample
                 nothing: 4 pixels x 8 heads receive 126 x 4 = 504 contributions each, every other destination none; grad_output is
                 positive, so the contributions of a channel do not cancel;
  spread         the channels of grad_output scaled cyclically by 2^-8, 1, 2^8 and EVERY row of logits spread over +-60.

THE MODEL (``model``) restates the definition of the deterministic grad_value in exact integer arithmetic on the CPU:
a contribution is x = w_k * (go_c * a) in fp32; per destination mx = max of w_k * (max_c |go_c| * |a|), cnt = number of
(query, point, corner); k1 = max(exponent field of mx, 1) - 126, c = bit_length(cnt), e = 61 - k1 - c; the result is
float(double(sum of rne(x * 2^e)) * 2^-e) with the sum in int64 (wrapping like the hardware if it overflowed).  ``scale="tensor"``
(one (mx, cnt) for the whole tensor) and ``headroom=False`` (e = 61 - k1) are the two wrong models of the CPU test."""
import collections
import functools
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import msda_cases as C  # noqa: E402

M, P, B = 8, 4, 2


def _case(name, levels, D, seed):
    return C.Case(name, "bwd", tuple(levels), B, M, D, P, sum(h * w for h, w in levels), seed)


ENC_FORM_CASES = tuple(_case(f"det_{n}_D{D}", lv, D, 300 + 10 * i + j)
                       for i, (n, lv) in enumerate((("C", C.LEVELS_C), ("B", C.LEVELS_B))) for j, D in enumerate((8, 32, 24, 6, 64)))
PILE_CASE = _case("det_pile", C.LEVELS_C, 8, 340)
SPREAD_CASE = _case("det_spread", C.LEVELS_C, 8, 341)
NEW_CASES = ENC_FORM_CASES + (PILE_CASE, SPREAD_CASE)
SIX_LANE_CASES = tuple(c for c in ENC_FORM_CASES if c.D in (24, 6))
SUPPORTED_OLD_CASES = tuple(c for c in C.BWD_CASES if c.D <= 64 and len(c.levels) <= C.MAXL)
PILE_CELL = (3, 5)                                  # (row, column) of the cell on level 0 of LEVELS_C (8 x 12)
PILE_ADDERS = 126 * P
ids = lambda cases: [c.name for c in cases]


def by_name(name):
    return next(c for c in NEW_CASES + C.BWD_CASES if c.name == name)


@functools.lru_cache(maxsize=None)
def bwd_inputs(case):
    """BwdInputs(value, loc, aw, go) of a case of this module or of msda_cases.BWD_CASES"""
    if case == PILE_CASE:
        g = torch.Generator().manual_seed(case.seed)
        S, L = case.Lq, len(case.levels)
        value = torch.randn(B, S, M, case.D, generator=g)
        H0, W0 = case.levels[0]
        frac = 2.0 ** -5 + torch.rand(B, S, M, P, 2, generator=g) * (1.0 - 2.0 ** -4)      # >= 2^-5 from the cell's borders: kink-free
        loc = torch.full((B, S, M, L, P, 2), 50.0)                                          # levels 1..: far outside, sample nothing
        loc[:, :, :, 0, :, 0] = (PILE_CELL[1] + frac[..., 0] + 0.5) / W0
        loc[:, :, :, 0, :, 1] = (PILE_CELL[0] + frac[..., 1] + 0.5) / H0
        aw = torch.softmax(torch.randn(B, S, M, L * P, generator=g), -1).view(B, S, M, L, P).contiguous()
        go = torch.randn(B, S, M * case.D, generator=g).abs() + 0.5
        return C.BwdInputs(value, loc.contiguous(), aw, go)
    if case == SPREAD_CASE:
        base = C.bwd_inputs(case)
        g = torch.Generator().manual_seed(case.seed + 2000)
        L = len(case.levels)
        aw = torch.softmax(torch.randn(B, case.Lq, M, L * P, generator=g) * 20.0, -1).view(B, case.Lq, M, L, P).contiguous()
        scale = torch.tensor([2.0 ** -8, 1.0, 2.0 ** 8])[torch.arange(case.D) % 3]
        go = (base.go.view(B, case.Lq, M, case.D) * scale).reshape(B, case.Lq, M * case.D).contiguous()
        return C.BwdInputs(base.value, base.loc, aw, go)
    return C.bwd_inputs(case)


@functools.lru_cache(maxsize=None)
def backward_ref(case):
    """((grad_value, grad_sampling_loc, grad_attn_weight), (tol_value, tol_loc, tol_weight)) float64: msda_cases' definition and bound"""
    b = bwd_inputs(case)
    return C.autograd64(case, b), C.bwd_bound(case, b)


# ---------------------------------------------------------------------------------------------------------------------------
# permutations
# ---------------------------------------------------------------------------------------------------------------------------
Permuted = collections.namedtuple("Permuted", "inputs qperm qinv pperm pinv")


@functools.lru_cache(maxsize=None)
def permuted(case, queries=True, points=True):
    """The case's inputs with the queries permuted (one permutation of Lq) and / or the points permuted within each level (one
    permutation of P per level), and the maps back: for a result r of the permuted call, ``unpermute(r, perm)`` is in the order
    of the original call."""
    b = bwd_inputs(case)
    g = torch.Generator().manual_seed(case.seed + 3000)
    L = len(case.levels)
    qperm = torch.randperm(case.Lq, generator=g) if queries else torch.arange(case.Lq)
    pperm = torch.stack([torch.randperm(case.P, generator=g) if points else torch.arange(case.P) for _ in range(L)])
    if queries and case.Lq > 1:
        assert not torch.equal(qperm, torch.arange(case.Lq))
    lidx = torch.arange(L)[:, None]
    loc = b.loc[:, qperm][:, :, :, lidx, pperm].contiguous()
    aw = b.aw[:, qperm][:, :, :, lidx, pperm].contiguous()
    go = b.go[:, qperm].contiguous()
    return Permuted(C.BwdInputs(b.value, loc, aw, go), qperm, torch.argsort(qperm), pperm, torch.argsort(pperm, 1))


def unpermute(grad, perm):
    """grad_sampling_loc (B, Lq, M, L, P, 2) or grad_attn_weight (B, Lq, M, L, P) of a permuted call -> the original order"""
    L = perm.pinv.shape[0]
    lidx = torch.arange(L, device=grad.device)[:, None]
    return grad[:, :, :, lidx, perm.pinv.to(grad.device)][:, perm.qinv.to(grad.device)]


# ---------------------------------------------------------------------------------------------------------------------------
# the integer model of grad_value
# ---------------------------------------------------------------------------------------------------------------------------
def contributions(case, b):
    """(dest (n,) int64 = (image * S + pixel) * M + head, x (n, D) fp32, bound (n,) fp32) of every in-range corner of every point,
    in fp32 with the kernel's products: w_k * (go_c * a) and w_k * (max_c |go_c| * |a|)"""
    Bn, S, Mh, D = b.value.shape
    _, Lq, _, L, Pn, _ = b.loc.shape
    go = b.go.view(Bn, Lq, Mh, 1, D)
    gmax = go.abs().amax(-1)                                                              # (B, Lq, M, 1)
    n_idx = torch.arange(Bn)[:, None, None, None].expand(Bn, Lq, Mh, Pn)
    m_idx = torch.arange(Mh)[None, None, :, None].expand(Bn, Lq, Mh, Pn)
    dest, xs, bounds = [], [], []
    start = 0
    for lid, (H, W) in enumerate(case.levels):
        him = b.loc[:, :, :, lid, :, 1] * float(H) - 0.5
        wim = b.loc[:, :, :, lid, :, 0] * float(W) - 0.5
        inside = (him > -1) & (wim > -1) & (him < H) & (wim < W)
        h0, w0 = torch.floor(him), torch.floor(wim)
        lh, lw = him - h0, wim - w0
        hh, hw = 1.0 - lh, 1.0 - lw
        h0, w0 = h0.long(), w0.long()
        a = b.aw[:, :, :, lid]
        tg = go * a[..., None]                                                             # (B, Lq, M, P, D) fp32
        tb = gmax * a.abs()
        for dh, dw, wt in ((0, 0, hh * hw), (0, 1, hh * lw), (1, 0, lh * hw), (1, 1, lh * lw)):
            y, x = h0 + dh, w0 + dw
            ok = inside & (y >= 0) & (y <= H - 1) & (x >= 0) & (x <= W - 1)
            d = (n_idx * S + start + y * W + x) * Mh + m_idx
            dest.append(d[ok])
            xs.append((wt[..., None] * tg)[ok])
            bounds.append((wt * tb)[ok])
        start += H * W
    x = torch.cat(xs)
    assert x.dtype == torch.float32
    return torch.cat(dest), x, torch.cat(bounds)


def exponent(mx, cnt, headroom=True):
    """e of a destination from its (mx fp32 >= 0, cnt int64 >= 1)"""
    E = mx.contiguous().view(torch.int32).long() >> 23
    k1 = E.clamp_min(1) - 126
    c = torch.zeros_like(cnt)
    for bit in range(32):
        c = c + (cnt >= (1 << bit)).long()                                                 # bit_length
    return 61 - k1 - (c if headroom else 0)


def pow2(e):
    """2^e in float64 for int64 e in [-1022, 1023], built from the bits (exact)"""
    return ((e + 1023) << 52).contiguous().view(torch.float64)


Model = collections.namedtuple("Model", "grad_value mx cnt e sums abs_sums dest q")


def model(case, b=None, scale="dest", headroom=True):
    """The deterministic grad_value of a case with FINITE inputs, in exact integer arithmetic (module docstring)."""
    b = b or bwd_inputs(case)
    Bn, S, Mh, D = b.value.shape
    n_dest = Bn * S * Mh
    dest, x, bound = contributions(case, b)
    assert bool(torch.isfinite(x).all()) and bool((x.abs() <= bound[:, None]).all())       # fp32 products are monotone
    mx = torch.zeros(n_dest).scatter_reduce(0, dest, bound, "amax")
    cnt = torch.bincount(dest, minlength=n_dest)
    if scale == "tensor":
        mx, cnt_e = mx.max().expand(n_dest), cnt.max().expand(n_dest)
    else:
        assert scale == "dest"
        cnt_e = cnt
    e = exponent(mx, cnt_e.clamp_min(1), headroom)
    xe = x.double() * pow2(e[dest])[:, None]                                                 # exact: a power-of-two scaling, no under/overflow
    q = torch.round(xe)                                                                    # round half to even; integers up to 2^62
    assert bool((q.abs() < 2.0 ** 63).all())
    qi = q.to(torch.int64)
    assert bool((qi.double() == q).all())
    sums = torch.zeros(n_dest, D, dtype=torch.int64).index_add_(0, dest, qi)              # exact, or wrapping modulo 2^64
    abs_sums = torch.zeros(n_dest, D, dtype=torch.float64).index_add_(0, dest, q.abs())
    gv = (sums.double() * pow2(-e)[:, None]).float()
    gv = torch.where((cnt > 0)[:, None], gv, torch.zeros_like(gv))
    return Model(gv.view(Bn, S, Mh, D), mx, cnt, e, sums, abs_sums, dest, qi)
