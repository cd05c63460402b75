"""Hypersphere attention (csrc/attention.hip, csrc/attention_bwd.hip) where single keys and single mask bits decide.

Not a test module and needs no GPU.  It holds
  * the host dispatch restated (``route``: attn_launch, msm_hypersphere_attn_lp_fwd, attn_nsplit and the fused launcher) and, from it,
    which key blocks every (split, wave) takes (``shares``) and the keys at whose edges an index can go wrong (``edge_keys``);
  * the case tables (the smallest shapes that reach every kernel path, mask mode and split / wave edge);
  * seeded input families in which ONE key or ONE mask bit moves the answer by O(0.1 - 1) at every precision:
      U  uniform scores: every key of a head is a positive multiple of one vector, so every unmasked key has weight exactly 1 / n
         and out = normalize(mean of the unmasked V rows) whatever q and kappa are -- a closed form, and the 16-bit rounding of the
         (equal) probabilities cancels between numerator and denominator: every form must meet it to fp32 accuracy;
      D  dominant key masked: q_i = c k_j(i) with only key j(i) masked: a missed bit turns the row into normalize(v_j);
      C  coherent masks: whole key blocks, a wave's whole share, a whole split range, rectangles, fully masked rows (row_any = 0
         attends everywhere), a fully unmasked row;
      Z  degenerate vectors: zero q / k / v rows (the 1e-12 clamp) and rows scaled by 1e-3 / 1e3, on random keys (Zr, unmasked: Z0)
         and on the uniform-score family (Zu);
  * the float64 definition (the chain of oracle.msm_oracle.hypersphere_attention) and the CPU yardsticks of the 16-bit forms.

Forms: f32; lp0 (fp32 K/V, bf16 operands), lp1 (bf16 K/V), lp2 (fp16 K, bf16 V), lp3 (fp32 K/V, fp16 scores) of
msm_hypersphere_attn_lp_fwd; fkv1 / fkv2 (msm_hypersphere_attn_fused_kv_fwd with bf16 / fp16 score operands); bwd.
"""
import functools
import zlib
from collections import namedtuple

import torch
import torch.nn.functional as F

HD = 32
AQCH = 112                      # queries per chunk (AQB * 16)
PSTRIDE = HD + 1
BWD_REC = 2 + 2 * HD
KAPPA = 30.0
MASK_BYTES = (1, 2, 128, 255)   # "nonzero = masked"
FWD_FORMS = ("f32", "lp0", "lp1", "lp2", "lp3")
FKV_FORMS = ("fkv1", "fkv2")
QKCFG = {0: (2, 8), 1: (1, 8), 2: (4, 4)}      # ATTN_QKCFG -> (MQ query blocks per workgroup, NW waves)

# the project's own bounds (tests/test_gpu_ops.py: test_hypersphere_attention, .._low_precision; tests/test_gpu_training.py)
F32_RTOL, F32_ATOL = 1e-4, 2e-5
LP_BOUND = {"bf16": (3e-2, 2e-3), "f16": (1.5e-2, 8e-4)}           # (max, mean) of |got - float64|


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the dispatch, restated
# ---------------------------------------------------------------------------------------------------------------------------
Route = namedtuple("Route", "kernel cfg mq nw mm ns kb_per nkb qchunks operand fallback empty")


def nsplit(B, qchunks, heads, S, target=0):
    """attn_nsplit: min(cdiv(target, B * qchunks * heads), max(1, S // 128)), target 512 unless ATTN_TARGET > 0."""
    ns = cdiv(target if target > 0 else 512, B * qchunks * heads)
    return max(1, min(ns, max(1, S // 128)))


def route(form, B, Lq, S, heads, masked, opts=None):
    """Which kernel a call runs and with what parameters.  opts: {"ATTN_KERNEL": 3, "ATTN_QKCFG": c, "ATTN_TARGET": t, "ATTN_QK_MAX": n}.
    kernel: "qk" (with cfg and its (mq, nw)), "big" (split-K; + combine when ns > 1), "fkv", "bwd".  mm: the mask access mode (0 none;
    1 one word per (query, 4 keys), S % 4 == 0; 2 bytewise; the fused form reads bits: 1).  operand: the type that really multiplies
    ("f32", "bf16", "f16"); fallback: lp0 / lp3 at S <= 128 run the fp32 kernel.  empty: the splits that get no key block."""
    opts = dict(opts or {})
    qchunks = cdiv(Lq, AQCH)
    nkb = cdiv(S, 16)
    if form == "bwd":
        return Route("bwd", None, None, None, 0 if not masked else 1, 1, nkb, nkb, qchunks, "f32", False, ())
    ns = nsplit(B, qchunks, heads, S, opts.get("ATTN_TARGET", 0))
    kb_per = cdiv(nkb, ns)
    empty = tuple(s for s in range(ns) if s * kb_per >= nkb)
    if form in FKV_FORMS:
        assert S % 16 == 0
        return Route("fkv", None, None, 4, 1 if masked else 0, ns, kb_per, nkb, qchunks, "bf16" if form == "fkv1" else "f16", False, empty)
    mm = 0 if not masked else (1 if S % 4 == 0 else 2)
    fallback = form in ("lp0", "lp3") and S <= 128
    operand = "f32" if form == "f32" or fallback else ("f16" if form in ("lp2", "lp3") else "bf16")
    qk_max = opts.get("ATTN_QK_MAX", 0) if opts.get("ATTN_QK_MAX", 0) > 0 else 2048
    if S <= qk_max and opts.get("ATTN_KERNEL", -1) != 3:
        cfg = opts.get("ATTN_QKCFG", -1)
        if cfg < 0:
            cfg = 2 if (B >= 48 and S <= 1024) else (1 if S <= 128 else 0)
        mq, nw = QKCFG.get(cfg, QKCFG[0])
        return Route("qk", cfg if cfg in QKCFG else 0, mq, nw, mm, 1, nkb, nkb, qchunks, operand, fallback, ())
    return Route("big", None, AQCH // 16, 4, mm, ns, kb_per, nkb, qchunks, operand, fallback, empty)


def workspace_floats(B, Lq, S, heads, opts=None):
    """msm_hypersphere_attn_workspace."""
    return B * cdiv(Lq, AQCH) * heads * nsplit(B, cdiv(Lq, AQCH), heads, S, (opts or {}).get("ATTN_TARGET", 0)) * AQCH * PSTRIDE


def path(r):
    """The kernel path of a route as the coverage tables name it."""
    if r.kernel == "qk":
        return f"qk{r.cfg}"
    if r.kernel == "bwd":
        return "bwd"
    return r.kernel + ("E" if r.empty else ("1" if r.ns == 1 else "N"))


def shares(r, S, hw=None):
    """[split][wave] -> the 16-key blocks (index in key order) that wave streams, in its order."""
    if r.kernel == "qk":
        return [[list(range(w, r.nkb, r.nw)) for w in range(r.nw)]]
    if r.kernel == "bwd":
        return [[list(range(r.nkb))]]
    out = []
    for s in range(r.ns):
        beg, end = s * r.kb_per, min(r.nkb, (s + 1) * r.kb_per)
        if r.kernel == "big":
            out.append([list(range(beg + w, end, 4)) for w in range(4)])
            continue
        H, W = hw                                        # fused: units in column-major order u = strip * H + y, a contiguous quarter per wave
        strips = W // 16
        w_per = cdiv(max(end - beg, 0), 4)
        waves = []
        for w in range(4):
            u0 = beg + w * w_per
            waves.append([(u % H) * strips + u // H for u in range(u0, max(u0, min(end, u0 + w_per)))])
        out.append(waves)
    return out


def fkv_features(r, S, hw):
    """What the fused kernel's unit walk does at this shape: idle waves, a wave whose units cross a column strip."""
    H, W = hw
    strips = W // 16
    feats = set()
    for split in shares(r, S, hw):
        if not any(split):
            continue
        for blocks in split:
            if not blocks:
                feats.add("idle")
            elif len({kb % strips for kb in blocks}) > 1:
                feats.add("cross")
    return feats


def edge_keys(r, S, hw=None):
    """Keys at which an index, a clamp or a range bound can go wrong: keys 0, 15, 16, 17, S - 1; every slot 4 lq + r of the first, a middle
    and the last 16-key block; the first and last key of every split range and of every wave's share; 255 .. 257 (the backward's stride)."""
    ks = {0, 15, 16, 17, S - 1, S - 2, 255, 256, 257}
    for kb in (0, r.nkb // 2, r.nkb - 1):
        ks.update(range(16 * kb, 16 * kb + 16))
    for split in shares(r, S, hw):
        seq = [kb for blocks in split for kb in blocks]
        if seq:
            ks.update((16 * min(seq), 16 * max(seq) + 15, 16 * max(seq)))
        for blocks in split:
            if blocks:
                ks.update((16 * blocks[0], 16 * blocks[0] + 15, 16 * blocks[-1], 16 * blocks[-1] + 15))
    return sorted(k for k in ks if 0 <= k < S)


def edge_queries(Lq):
    """Rows at the 16 * MQ group edges (MQ = 1, 2, 4), the chunk edge and the end."""
    return sorted(i for i in {0, 15, 16, 17, 31, 32, 33, 63, 64, 65, 111, 112, Lq - 1} if 0 <= i < Lq)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the case tables
# ---------------------------------------------------------------------------------------------------------------------------
# fam: U, D, C, Zr, Z0 (Zr without a mask), Zu.  ra: how row_any is passed ("given", "none"; "-" without a mask).  hw: (H, W) of the fused form.
Case = namedtuple("Case", "id form fam B Lq S heads opts kappa hw ra")


def _opts_id(opts):
    return "".join(f"-{k[5:].lower()}{v}" for k, v in opts)


def _case(form, fam, B, Lq, S, heads=8, opts=(), kappa=KAPPA, hw=None, ra=None):
    masked = fam != "Z0"
    if ra is None:
        ra = "-" if not masked else ("none" if fam in ("U", "Zu") else "given")
    shape = f"B{B}-Lq{Lq}-S{S}" + (f"-{hw[0]}x{hw[1]}" if hw else "") + (f"-h{heads}" if heads != 8 else "")
    cid = f"{form}-{fam}-{shape}{_opts_id(opts)}" + (f"-k{kappa:g}" if kappa != KAPPA else "") + ("-noany" if fam == "C" and ra == "none" else "")
    return Case(cid, form, fam, B, Lq, S, heads, tuple(opts), kappa, hw, ra)


# the query-split kernel: S gives mask mode 2 at 1/3/15/17/127/129/301, a tail-only block in mode 1 at 4/20/300 and fewer key blocks than
# waves; Lq crosses the 16 * MQ group edges.  Every S meets every configuration; Lq is cycled over the S (the kernel's query and key
# indexing are independent of each other).
QK_S = (1, 3, 4, 15, 16, 17, 20, 127, 128, 129, 300, 301)
QK_LQ = (1, 15, 16, 17, 33, 65, 100)
QK_SHAPES = [(1 + (i % 2), QK_LQ[i % len(QK_LQ)], S) for i, S in enumerate(QK_S)]
QK_RICH = (17, 20, 129, 300, 301)                 # the S at which the families beyond U run (both mask modes, one and many key blocks)
K3 = (("ATTN_KERNEL", 3),)
# the split-K kernel: (B, Lq, S, opts).  S = 16 / 48: ns = 1 with idle waves; 272 / 300 / 301: ns = 2 with splits of 9 / 8 and 10 / 9 blocks and
# a tail in word and byte mask mode; ATTN_TARGET = 1: ns = 1 at the same S; 1296 (1295: the byte mode), B = 1: split 9 of 10 is empty;
# 2064: the length at which the default path takes this kernel (16 splits, the last one empty).
BIG_SHAPES = [(1, 37, 16, K3), (1, 111, 48, K3), (1, 112, 272, K3), (2, 113, 300, K3), (1, 37, 301, K3),
              (2, 113, 300, K3 + (("ATTN_TARGET", 1),)), (1, 37, 301, K3 + (("ATTN_TARGET", 1),)),
              (1, 113, 1296, K3), (1, 111, 1295, K3), (1, 37, 2064, ())]
# the fused K/V form: (B, Lq, H, W).  (1,16) one unit; (3,16) wave 3 idle; (5,32) ten units, wave 1 crosses the strip; (17,16) ns = 2;
# (27,48) S = 1296: the empty split
FKV_SHAPES = [(1, 37, 1, 16), (2, 112, 3, 16), (1, 113, 5, 32), (2, 37, 17, 16), (1, 113, 27, 48)]
BWD_SHAPES = [(1, 1, 1), (2, 5, 7), (1, 4, 255), (1, 8, 256), (2, 9, 257), (1, 100, 300)]
RICH_FAMS = (("D", None), ("C", "given"), ("C", "none"), ("Zr", None), ("Z0", None), ("Zu", None))


def _forward_cases():
    cases = []
    for form in FWD_FORMS:
        for cfg in (0, 1, 2):
            o = (("ATTN_QKCFG", cfg),)
            for B, Lq, S in QK_SHAPES:
                cases.append(_case(form, "U", B, Lq, S, opts=o))
                if S in QK_RICH:
                    cases += [_case(form, fam, B, Lq, S, opts=o, ra=ra) for fam, ra in RICH_FAMS]
        cases.append(_case(form, "U", 48, 17, 20))                            # configuration 2 by default (B >= 48, S <= 1024)
        cases.append(_case(form, "D", 48, 17, 20))
        cases.append(_case(form, "U", 1, 33, 301, heads=3))
        cases.append(_case(form, "D", 1, 33, 301, heads=3))
        for B, Lq, S, o in BIG_SHAPES:
            cases.append(_case(form, "U", B, Lq, S, opts=o))
            cases += [_case(form, fam, B, Lq, S, opts=o, ra=ra) for fam, ra in RICH_FAMS]
        cases.append(_case(form, "U", 1, 111, 301, heads=3, opts=K3))
        cases.append(_case(form, "D", 1, 111, 301, heads=3, opts=K3))
    for fam in ("U", "C", "Zr", "Z0"):                                        # kappa = 1 (D needs a dominant key: kappa = 30 only)
        cases.append(_case("f32", fam, 2, 33, 129, opts=(("ATTN_QKCFG", 0),), kappa=1.0))
        cases.append(_case("f32", fam, 2, 113, 300, opts=K3, kappa=1.0))
    return cases


def _fkv_cases():
    # no zero k / v rows here: K and V are affine images of x inside the kernel, a key with K = 0 or V = 0 is not an input one can state
    cases = []
    for form in FKV_FORMS:
        for B, Lq, H, W in FKV_SHAPES:
            for fam, ra in (("U", None), ("D", None), ("C", "given"), ("C", "none"), ("Zr", None), ("Z0", None), ("Zu", None)):
                cases.append(_case(form, fam, B, Lq, H * W, hw=(H, W), ra=ra))
        cases.append(_case(form, "U", 1, 37, 160, heads=3, hw=(5, 32)))
        cases.append(_case(form, "D", 1, 37, 160, heads=3, hw=(5, 32)))
    return cases


def _bwd_cases():
    # no zero q / k rows here: their gradient is the 1 / 1e-12 of the clamp, which would be the scale of the project's rule for every other row
    cases = []
    for B, Lq, S in BWD_SHAPES:
        for fam in ("U", "D", "C", "Zr", "Z0"):
            if fam == "D" and S < 2:
                continue
            cases.append(_case("bwd", fam, B, Lq, S, ra="-" if fam == "Z0" else "given"))
    cases.append(_case("bwd", "C", 2, 9, 257, kappa=1.0, ra="given"))
    cases.append(_case("bwd", "Z0", 2, 9, 257, kappa=1.0, ra="-"))
    cases.append(_case("bwd", "U", 1, 9, 257, heads=3, ra="given"))
    return cases


FORWARD_CASES = _forward_cases()
FKV_CASES = _fkv_cases()
BWD_CASES = _bwd_cases()
ALL_CASES = FORWARD_CASES + FKV_CASES + BWD_CASES
# strided views (q, k, v as column slices of a (B, ., 3E) buffer) and sentinel runs: one per kernel
STRIDED_CASES = [_case(form, "C", B, Lq, S, opts=o, ra="given") for form in ("f32", "lp1")
                 for B, Lq, S, o in ((2, 33, 129, ()), (1, 37, 301, K3 + (("ATTN_TARGET", 1),)), (2, 113, 300, K3))] + \
                [_case("fkv1", "C", 2, 37, 272, hw=(17, 16), ra="given"), _case("bwd", "C", 2, 9, 257, ra="given")]
SENTINEL_CASES = [_case("f32", "C", 2, 33, 129, ra="given"), _case("lp1", "C", 1, 37, 301, opts=K3 + (("ATTN_TARGET", 1),), ra="given"),
                  _case("f32", "C", 2, 113, 300, opts=K3, ra="given"), _case("lp2", "C", 1, 113, 1296, opts=K3, ra="given"),
                  _case("fkv2", "C", 2, 37, 272, hw=(17, 16), ra="given"), _case("fkv1", "C", 1, 113, 1296, hw=(27, 48), ra="given"),
                  _case("bwd", "C", 2, 9, 257, ra="given")]


def case_route(c):
    return route(c.form, c.B, c.Lq, c.S, c.heads, c.fam != "Z0", dict(c.opts))


def cover_key(c):
    """The combination a case reaches, or None for a row that runs another kernel than its form names (lp0 / lp3 at S <= 128)."""
    r = case_route(c)
    if r.fallback:
        return None
    if c.form == "bwd":
        return None
    if c.form in FKV_FORMS:
        return None
    return (c.form, path(r), r.mm, c.ra)


def required_cover():
    keys = set()
    for form in FWD_FORMS:
        for p in ("qk0", "qk1", "qk2", "big1", "bigN", "bigE"):
            keys.add((form, p, 0, "-"))
            for mm in (1, 2):
                keys.update({(form, p, mm, "given"), (form, p, mm, "none")})
    return keys


def fkv_cover(c):
    r = case_route(c)
    feats = fkv_features(r, c.S, c.hw) | {"ns1" if r.ns == 1 else "nsN"} | ({"empty"} if r.empty else set())
    return {(c.form, c.fam != "Z0", f) for f in feats}


def required_fkv_cover():
    return {(form, m, f) for form in FKV_FORMS for m in (False, True) for f in ("ns1", "nsN", "empty", "idle", "cross")}


def bwd_cover(c):
    return {("masked", c.fam != "Z0"), ("Lq%4", c.Lq % 4), ("S", c.S)}


def required_bwd_cover():
    return {("masked", False), ("masked", True), ("Lq%4", 0), ("Lq%4", 1), ("S", 1), ("S", 255), ("S", 256), ("S", 257)}


# ---------------------------------------------------------------------------------------------------------------------------
# 3. roundings, the float64 definition, the yardsticks
# ---------------------------------------------------------------------------------------------------------------------------
def bf16(t):
    """Round to nearest even to bf16 (pack4 in csrc/bf16.h), value kept in the input's dtype."""
    return t.float().to(torch.bfloat16).to(t.dtype)


def f16(t):
    return t.float().to(torch.float16).to(t.dtype)


def bf16_rne_bits(t):
    """bf16 by integer arithmetic, round to nearest even on the fp32 bits -- what test_attn_cases_cpu pins ``bf16`` to."""
    u = t.float().contiguous().view(torch.int32).to(torch.int64) & 0xffffffff
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return (u - ((u >> 31) << 32)).to(torch.int32).view(torch.float32)


def unit(t):
    return F.normalize(t, p=2, dim=-1, eps=1e-12)


def split_heads(t, heads):
    B, L, _ = t.shape
    return t.view(B, L, heads, HD).permute(0, 2, 1, 3)


def merge_heads(t):
    B, H, L, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, L, H * HD)


def effective_mask(mask, row_any):
    """bool (B, Lq, S): nonzero bytes, switched off in the rows whose row_any is 0 (they attend everywhere)."""
    if mask is None:
        return None
    eff = mask != 0
    if row_any is not None:
        eff = eff & (row_any[..., None] != 0)
    return eff


def definition(q, k, v, heads, mask=None, row_any=None, kappa=KAPPA):
    """The chain of oracle.msm_oracle.hypersphere_attention in float64 with the head split / merge: (B, Lq, E) float64 (differentiable)."""
    qh, kh, vh = (split_heads(t.double(), heads) for t in (q, k, v))
    logits = kappa * torch.matmul(unit(qh), unit(kh).transpose(-2, -1))
    eff = effective_mask(mask, row_any)
    if eff is not None:
        logits = logits.masked_fill(eff[:, None], float("-inf"))
    return merge_heads(unit(torch.matmul(torch.softmax(logits, dim=-1), vh)))


def uniform_closed_form(v, heads, mask, row_any=None):
    """Family U (and any zero q row): out = normalize(mean of the unmasked V rows)."""
    keep = (~effective_mask(mask, row_any)).double()                             # (B, Lq, S)
    vh = split_heads(v.double(), heads)                                          # (B, H, S, 32)
    o = torch.matmul(keep[:, None], vh) / keep.sum(-1)[:, None, :, None]
    return merge_heads(unit(o))


def yardstick(q, k, v, heads, mask, row_any, kappa, operand, way):
    """A 16-bit form on the CPU: q^ and k^ rounded to ``operand`` (bf16 / f16), the probabilities and V to bf16, sums in fp32.
    way 0: every step in fp32 (torch's matmul order); way 1: the same roundings, decided on fp32 values, with float64 arithmetic between
    them (an accumulation order that loses nothing).  Returns (B, Lq, E) float64."""
    r = bf16 if operand == "bf16" else f16
    dt = torch.float32 if way == 0 else torch.float64
    k2 = kappa * 1.4426950408889634
    qh, kh, vh = (split_heads(t.float(), heads) for t in (q, k, v))
    qn, kn = r(unit(qh.to(dt)).float()).to(dt), r(unit(kh.to(dt)).float()).to(dt)
    s = torch.matmul(qn, kn.transpose(-2, -1)).float()
    p = torch.exp2(s.to(dt) * k2 - k2).float()
    eff = effective_mask(mask, row_any)
    if eff is not None:
        p = p.masked_fill(eff[:, None], 0.0)
    l = p.to(dt).sum(-1, keepdim=True)
    o = torch.matmul(bf16(p).to(dt), bf16(vh).to(dt)) / l
    return merge_heads(unit(o.float().to(dt))).double()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the input families
# ---------------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def _mask_bytes(g, *shape):
    return torch.tensor(MASK_BYTES, dtype=torch.uint8)[torch.randint(0, len(MASK_BYTES), shape, generator=g)]


def head_directions(g, heads):
    """One vector per head whose unit vector is exact in fp32, bf16 and fp16: 28 entries +-1 and 4 entries +-3 (norm 8)."""
    d = torch.ones(heads, HD)
    for h in range(heads):
        d[h, torch.randperm(HD, generator=g)[:4]] = 3.0
    return d * (torch.randint(0, 2, (heads, HD), generator=g) * 2 - 1).float()


def _distinct(first, n, S):
    """n distinct keys: ``first`` in order (duplicates dropped), then their right neighbours."""
    out = []
    for kk in first:
        if kk not in out:
            out.append(kk)
    j = 0
    while len(out) < n:
        cand = (out[j % len(out)] + 1 + j // len(out)) % S
        if cand not in out:
            out.append(cand)
        j += 1
    return out[:n]


U_COUNTS = (1, 2, 3, 17)


def uniform_keep(B, Lq, S, edges, counts=U_COUNTS):
    """Family U's unmasked keys per row: n cycles over ``counts`` (17 at the edge queries), the keys cycle over the edge list."""
    eq = edge_queries(Lq)
    keep = []
    for b in range(B):
        for i in range(Lq):
            r = b * Lq + i
            n = min(S, 17 if (i in eq and len(counts) > 1) else counts[r % len(counts)])
            start = (eq.index(i) * 17 + b * 5) if (i in eq and len(counts) > 1) else r
            keep.append(_distinct([edges[(start + t) % len(edges)] for t in range(n)], n, S))
    return keep


def _keep_to_mask(g, B, Lq, S, keep):
    mask = _mask_bytes(g, B, Lq, S)
    for r, ks in enumerate(keep):
        mask[r // Lq, r % Lq, ks] = 0
    return mask


def _coherent_mask(g, c, r, ra):
    """Family C: per row, cycling: a whole 16-key block; every block of one wave's share; a whole split range (half the blocks when there is one
    split); nothing; for the fused form a rectangle in (y, x).  ra "given": rows 1 and Lq - 1 fully masked with row_any = 0."""
    B, Lq, S = c.B, c.Lq, c.S
    sh = shares(r, S, c.hw)
    waves = [blocks for split in sh for blocks in split if blocks]
    splits = [[kb for blocks in split for kb in blocks] for split in sh]
    splits = [s for s in splits if s]
    if len(splits) == 1:
        allb = sorted(splits[0])
        splits = [allb[:max(1, len(allb) // 2)], allb[len(allb) // 2:]]
    mask = torch.zeros(B, Lq, S, dtype=torch.uint8)
    fill = _mask_bytes(g, B, Lq, S)
    npat = 5 if c.hw else 4
    for b in range(B):
        for i in range(Lq):
            row = b * Lq + i
            pat, turn = row % npat, row // npat
            m = torch.zeros(S, dtype=torch.bool)
            blocks = []
            if pat == 0:
                blocks = [turn % r.nkb]
            elif pat == 1:
                blocks = waves[turn % len(waves)]
            elif pat == 2:
                blocks = splits[turn % len(splits)]
            elif pat == 4:
                H, W = c.hw
                y0, x0 = turn % H, (3 * turn) % W
                m.view(H, W)[y0:y0 + 1 + H // 2, x0:x0 + 1 + W // 3] = True
            for kb in blocks:
                m[16 * kb:16 * kb + 16] = True
            if bool(m.all()):
                m[row % S] = False
            mask[b, i][m] = fill[b, i][m]
    row_any = None
    if ra == "given":
        row_any = torch.ones(B, Lq, dtype=torch.int32)
        if Lq >= 3:
            for i in (1, Lq - 1):
                mask[:, i] = fill[:, i]
                row_any[:, i] = 0
    return mask, row_any


def _degenerate(c, q, k, v, edges, bwd):
    """Family Z's rows: q rows 0 / 1 / 2 (and the last) zero / x 1e-3 / x 1e3; the same for three edge keys of k; a zero and a x 1e3 row of v."""
    Lq, S = c.Lq, c.S
    if not bwd:
        q[:, 0] = 0.0
    if Lq > 1:
        q[:, 1] *= 1e-3
    if Lq > 2:
        q[:, 2] *= 1e3
    if Lq > 3:
        q[:, Lq - 1] *= 1e-3
    if k is not None:
        ks = _distinct([edges[0], edges[-1], edges[len(edges) // 2], edges[len(edges) // 3]], min(S, 4), S)
        if not bwd:
            k[:, ks[0]] = 0.0
        if S > 1:
            k[:, ks[1]] *= 1e-3
        if S > 2:
            k[:, ks[2]] *= 1e3
        if S > 3:
            v[:, ks[3]] = 0.0
            v[:, ks[0]] *= 1e3 if not bwd else 1.0
        return ks
    return []


Inputs = namedtuple("Inputs", "q k v mask row_any keep fkv")        # fp32 tensors as the caller holds them; keep: family U's unmasked keys
Fkv = namedtuple("Fkv", "x w rowcol")                                 # x (B, S, 64) fp16-exact, w (2E, 64), rowcol (H + W, 2E)


def fkv_kv(f, hw):
    """K, V of the fused form in float64 from the operands as the kernel rounds them (x and W to fp16): (B, S, E) each."""
    H, W = hw
    const = (f.rowcol[:H, None] + f.rowcol[None, H:]).reshape(H * W, -1).double()
    kv = torch.matmul(f16(f.x).double(), f16(f.w).double().t()) + const
    E = kv.shape[-1] // 2
    return kv[..., :E], kv[..., E:]


def fkv_v_yardstick(f, hw):
    """V as an fp32 F.linear of the fp16 operands plus the constants (the CPU yardstick of the kernel's fp32 MFMA sum)."""
    H, W = hw
    E = f.w.shape[0] // 2
    const = (f.rowcol[:H, None] + f.rowcol[None, H:]).reshape(H * W, -1)
    return F.linear(f16(f.x), f16(f.w[E:])) + const[:, E:]


@functools.lru_cache(maxsize=None)
def _inputs(fam, B, Lq, S, heads, hw, ra, geom, bwd):
    c = Case("", "fkv1" if hw else ("bwd" if bwd else "f32"), fam, B, Lq, S, heads, (), KAPPA, hw, ra)
    r = Route(*geom)
    g = _gen(fam, B, Lq, S, heads, hw, ra, geom, bwd)
    E = heads * HD
    edges = edge_keys(r, S, hw)
    q = _randn(g, B, Lq, E)
    keep, fkv, mask, row_any = None, None, None, None
    uniform = fam in ("U", "Zu")
    if hw:
        H, W = hw
        if uniform:
            # K columns of W zero, the K constants a power-of-two multiple (2^-10 .. 2^10, rows + columns) of one vector per head; V varies
            # through x and the constants on dyadic grids on which every fp32 sum is exact (so V rounds to bf16 one way only)
            d = head_directions(g, heads).reshape(E)
            x = torch.randint(-16, 17, (B, S, 64), generator=g).float() / 16
            w = torch.cat([torch.zeros(E, 64), torch.randint(-16, 17, (E, 64), generator=g).float() / 32])
            rowcol = torch.empty(H + W, 2 * E)
            rowcol[:H, :E] = (2.0 ** torch.randint(-10, 1, (H, 1), generator=g)) * d
            rowcol[H:, :E] = (2.0 ** torch.randint(0, 11, (W, 1), generator=g)) * d
            rowcol[:, E:] = torch.randint(-512, 513, (H + W, E), generator=g).float() / 512
        else:
            x = f16(F.normalize(_randn(g, B, S, 64), dim=-1))
            w = _randn(g, 2 * E, 64) * 0.35
            rowcol = _randn(g, H + W, 2 * E) * 0.3
            rowcol[H:, E:] *= 0.5
        fkv = Fkv(x, w, rowcol)
        k64, v64 = fkv_kv(fkv, hw)
        k, v = k64.float(), v64.float()
    elif uniform:
        d = head_directions(g, heads)
        e = torch.randint(-10, 11, (B, S, heads, 1), generator=g)
        k = ((2.0 ** e) * d).reshape(B, S, E)
        v = _randn(g, B, S, E)
    else:
        k, v = _randn(g, B, S, E), _randn(g, B, S, E)
    if uniform:
        keep = uniform_keep(B, Lq, S, edges, (1,) if bwd else U_COUNTS)
        mask = _keep_to_mask(g, B, Lq, S, keep)
        if fam == "Zu":                                              # (no zero k row here: its cosine 0 would end the uniform scores)
            _degenerate(c, q, None, None, edges, bwd)
            if not hw and S > 1:
                v[:, keep[0][0]] = 0.0                                  # a zero v row among the unmasked keys of row 0
    elif fam == "D":
        j = [edges[(b * Lq + i) % len(edges)] for b in range(B) for i in range(Lq)]
        jt = torch.tensor(j).view(B, Lq)
        q = 1.7 * torch.gather(k, 1, jt[..., None].expand(B, Lq, E))
        mask = torch.zeros(B, Lq, S, dtype=torch.uint8)
        mask.scatter_(2, jt[..., None], _mask_bytes(g, B, Lq, 1))
        keep = j
    elif fam == "C":
        mask, row_any = _coherent_mask(g, c, r, ra)
    elif fam in ("Zr", "Z0"):
        ks = _degenerate(c, q, None if hw else k, v, edges, bwd)
        if fam == "Zr":
            # six random keys per row; the odd rows keep the degenerate keys as well
            keep = [_distinct((ks if r_ % 2 else []) + [int(t) for t in torch.randint(0, S, (6,), generator=g)], min(S, 6), S) for r_ in range(B * Lq)]
            mask = _keep_to_mask(g, B, Lq, S, keep)
    if mask is not None and row_any is None and ra == "given":
        row_any = torch.ones(B, Lq, dtype=torch.int32)
    return Inputs(q, k, v, mask, row_any, keep, fkv)


def inputs(c):
    """The seeded inputs of a case.  They depend on the route only through the splits and the waves' shares (edge keys, coherent masks)."""
    r = case_route(c)
    geom = tuple(r._replace(cfg=None, mq=None, mm=None, qchunks=None, operand=None, fallback=None))
    return _inputs(c.fam, c.B, c.Lq, c.S, c.heads, c.hw, c.ra, geom, c.form == "bwd")


def stored(form, k, v):
    """K and V as the form stores them (the values the float64 reference is fed): lp1 bf16 / bf16, lp2 fp16 / bf16, the fused form K in fp32 and V
    rounded to bf16 once (never stored: that rounding IS the operand), fp32 otherwise."""
    if form == "lp1":
        return bf16(k), bf16(v)
    if form == "lp2":
        return f16(k), bf16(v)
    if form in FKV_FORMS:
        return k, bf16(v)
    return k, v


def operand_v(form, r, v):
    """V as it enters P V: bf16 in every 16-bit kernel, fp32 in the fp32 kernel (also where lp0 / lp3 fall back to it)."""
    return v if r.operand == "f32" else bf16(v)


@functools.lru_cache(maxsize=None)
def _reference(c):
    x = inputs(c)
    k, v = stored(c.form, x.k, x.v)
    r = case_route(c)
    if c.fam in ("U", "Zu"):
        return uniform_closed_form(operand_v(c.form, r, v), c.heads, x.mask, x.row_any)
    return definition(x.q, k, v, c.heads, x.mask, x.row_any, c.kappa)


def reference(c):
    """float64 reference of a forward case: family U / Zu the closed form on V as the form rounds it, else the definition on the stored K / V."""
    return _reference(c._replace(id=""))


def exact(c):
    """Cases judged to fp32 accuracy: the fp32 kernel (also as the fallback of lp0 / lp3) and every form on the uniform-score family."""
    return case_route(c).operand == "f32" or c.fam in ("U", "Zu")


@functools.lru_cache(maxsize=None)
def _yard(c):
    x = inputs(c)
    k, v = stored(c.form, x.k, x.v)
    ref = reference(c)
    errs = [(yardstick(x.q, k, v, c.heads, x.mask, x.row_any, c.kappa, case_route(c).operand, way) - ref).abs() for way in (0, 1)]
    return max(float(e.max()) for e in errs), max(float(e.mean()) for e in errs)


def yard_error(c):
    """(max, mean) error of the CPU yardstick of a 16-bit case against its float64 reference (the larger of the two evaluations)."""
    return _yard(c._replace(id=""))


def lp_bound(c):
    """What a 16-bit case may show: (max, mean).  max: twice the case's yardstick -- the factor covers the accumulation order and the
    rsq / exp2 approximations --, never below the fp32 tolerance (a kernel is not asked for more than fp32 accuracy) and never above the
    project's bound; mean: the project's bound."""
    pmax, pmean = LP_BOUND[case_route(c).operand]
    return min(max(2.0 * yard_error(c)[0], F32_ATOL + F32_RTOL), pmax), pmean


def bwd_reference(c, gout):
    """float64 autograd of the definition: (out, grad_q, grad_k, grad_v)."""
    x = inputs(c)
    q, k, v = (t.double().requires_grad_(True) for t in (x.q, x.k, x.v))
    out = definition(q, k, v, c.heads, x.mask, x.row_any, c.kappa)
    out.backward(gout.double())
    return out.detach(), q.grad, k.grad, v.grad


def bwd_grad_out(c):
    return _randn(_gen("gout", c.B, c.Lq, c.heads), c.B, c.Lq, c.heads * HD)


def bwd_input_scale(c, gout, out64):
    """The scale of a gradient that is identically zero (grad_q, grad_k of family U with one unmasked key), from the inputs:
    kappa max|dO| max|v| / min(|q|, |k|) over the heads, dO = (g - out (out.g)) / |o| in float64."""
    x = inputs(c)
    keepm = (~effective_mask(x.mask, x.row_any)).double() if x.mask is not None else torch.ones(c.B, c.Lq, c.S, dtype=torch.float64)
    vh = split_heads(x.v.double(), c.heads)
    qh, kh = split_heads(x.q.double(), c.heads), split_heads(x.k.double(), c.heads)
    logits = c.kappa * torch.matmul(unit(qh), unit(kh).transpose(-2, -1)).masked_fill(keepm[:, None] == 0, float("-inf"))
    o = torch.matmul(torch.softmax(logits, -1), vh)
    g, oh = split_heads(gout.double(), c.heads), split_heads(out64, c.heads)
    dO = (g - oh * (oh * g).sum(-1, keepdim=True)) / o.norm(dim=-1, keepdim=True)
    return c.kappa * float(dO.abs().max()) * float(vh.abs().max()) / min(float(qh.norm(dim=-1).min()), float(kh.norm(dim=-1).min()))


def bwd_scale(c, ref, gout, out64):
    """The project's rule takes scale = max|ref|.  A reference that is zero up to float64 rounding (below 1e-9 of the input scale) counts
    as identically zero and takes the scale of the inputs."""
    m, s_in = float(ref.abs().max()), bwd_input_scale(c, gout, out64)
    return m if m > 1e-9 * s_in else s_in


def bwd_uniform_grad_v(c, gout):
    """Family U with one unmasked key per row: grad_v of key j is the sum of dO over the rows that chose j, every other row exactly 0."""
    x = inputs(c)
    vh = split_heads(x.v.double(), c.heads)
    g = split_heads(gout.double(), c.heads)
    gv = torch.zeros_like(vh)
    for r, ks in enumerate(x.keep):
        b, i = divmod(r, c.Lq)
        o = vh[b, :, ks[0]]
        oh = unit(o)
        gv[b, :, ks[0]] += (g[b, :, i] - oh * (oh * g[b, :, i]).sum(-1, keepdim=True)) / o.norm(dim=-1, keepdim=True)
    return merge_heads(gv)
