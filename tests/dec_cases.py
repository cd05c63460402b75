"""Cases shared by tests/test_dec_cases_cpu.py and tests/test_gpu_dec_tails.py (not a test module): the host dispatch of the fused
decoder tails (csrc/dec_chain.hip: msm_dec_post_cross / msm_dec_post_self / msm_dec_heads) restated, the tables of the smallest
shapes that reach every tile kind, seeded inputs, the float64 definitions of the three chains and the CPU yardsticks.  Needs no GPU.

THE YARDSTICK of a precision is the chain evaluated on the CPU with the operands rounded the way that form rounds them -- weights
to bf16 / bf16 hi + lo / fp16, the input of every GEMM as a hi + lo bf16 pair or as one fp16 value clamped to +-65504 -- and fp32
accumulation in two ways: ``F.linear`` and one accumulator per output walked strictly in k order (the kernel's structure: an MFMA
accumulator is one running sum; at K = 2048 that chain has several times F.linear's error); short fp16 comparisons add more orders
(``evaluate_orders``).  The reference of a comparison is the float64 definition on the same rounded operands, so what a comparison measures
is accumulation, the row phases and the roundings that flip when a GEMM input sits next to a rounding boundary -- the yardstick
rounds its own fp32 intermediates and meets such flips too.  The rule itself is in tests/test_gpu_dec_tails.py."""
import collections
import functools
import itertools

import torch
import torch.nn.functional as F

E, FF = 256, 2048
AUTO = -1
U32 = 2.0 ** -24
PRECS = ("f32", "bf16", "bf16x2", "f16")
ENTRIES = ("post_cross", "post_self", "heads")
TILE_ROWS = {"TileF8": 8, "TileF16": 16, "TileH16": 16, "TileH16x2": 16, "TileQ16": 16, "TileQ32": 32}
HEADS_PS = {k: (4 if r // 8 > 2 else 8) for k, r in TILE_ROWS.items()}      # partial sums in flight per row (dec_heads_kernel)


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------------
# the host's dispatch, restated
# ---------------------------------------------------------------------------------------------------------------------------
def use_tile8(rows, parts):
    return cdiv(rows, 8) * parts <= 256


def use_tile32(rows, tile32=AUTO):
    return tile32 == 1 or (tile32 != 0 and rows >= 4096)


def default_n_parts(rows, chunks=FF // E):
    """ops.dec_post_self without n_parts: the largest divisor of F / 256 that keeps 16-row tiles x parts within 256 workgroups."""
    tiles = (rows + 15) // 16
    return max(d for d in range(1, chunks + 1) if chunks % d == 0 and (d == 1 or tiles * d <= 256))


def tile_kind(entry, prec, rows, n_parts=None, wq=False, tile32=AUTO):
    """The tile kind msm_dec_<entry>[_<prec>] launches for ``rows`` rows (DEC_TILE32 = tile32)."""
    if prec == "bf16":
        return "TileH16"
    if prec == "bf16x2":
        return "TileH16x2"
    if prec == "f16":
        if entry == "post_cross":                      # 32-row tiles only on request
            return "TileQ32" if tile32 == 1 else "TileQ16"
        return "TileQ32" if use_tile32(rows, tile32) else "TileQ16"
    assert prec == "f32"
    if entry == "post_cross":
        parts = 2
    elif entry == "post_self":
        parts = default_n_parts(rows) if n_parts is None else n_parts
    else:
        parts = 2 if wq else 1
    return "TileF8" if use_tile8(rows, parts) else "TileF16"


def grid_tiles(kind, rows):
    """(tiles with rows, tiles launched): gridDim.x is padded to a multiple of 8 (tile_grid_x)."""
    t = cdiv(rows, TILE_ROWS[kind])
    return t, (t + 7) & ~7


def all_kinds():
    """Every (entry, tile kind) the host can launch."""
    return {(e, k) for e in ENTRIES for k in TILE_ROWS}


# ---------------------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "entry prec B Q n_parts wq tile32 opts")
Case.rows = property(lambda c: c.B * c.Q)
Case.kind = property(lambda c: tile_kind(c.entry, c.prec, c.rows, c.n_parts, c.wq, c.tile32))
Case.id = property(lambda c: f"{c.entry}-{c.prec}-{c.B}x{c.Q}" + ("" if c.n_parts is None else f"-p{c.n_parts}") + ("-wq" if c.wq else "") +
                   ("" if c.tile32 == AUTO else f"-t32_{c.tile32}") + ("" if not c.opts else "-" + "".join(sorted(c.opts))))


def _case(entry, prec, B, Q, n_parts=None, wq=False, tile32=AUTO, opts=""):
    return Case(entry, prec, B, Q, n_parts, wq, tile32, opts)


LP = ("bf16", "bf16x2", "f16")
LP_BQ = ((1, 1), (1, 15), (1, 16), (1, 17), (3, 11), (2, 100))          # rows 1, 15, 16, 17, 33, 200
Q32_BQ = ((1, 31), (3, 11), (3, 21))                                    # rows 31, 33, 63 with DEC_TILE32 = 1
BIG_BQ = (45, 100)                                                      # 4500 rows: TileQ32 by default

CROSS_CASES = tuple(
    [_case("post_cross", "f32", 1, 7), _case("post_cross", "f32", 4, 256),       # TileF8; 1024 rows: 128 tiles x 2 = 256, the boundary
     _case("post_cross", "f32", 5, 205)] +                                       # 1025 rows: TileF16, one row in the last tile, tiles straddle images
    [_case("post_cross", p, B, Q) for p in LP for B, Q in LP_BQ] +
    [_case("post_cross", "f16", B, Q, tile32=1) for B, Q in Q32_BQ])

SELF_CASES = tuple(
    [_case("post_self", "f32", 5, 51, 8),                                        # 255 rows x 8 parts: 32 x 8 = 256, TileF8 at the boundary
     _case("post_self", "f32", 5, 53, 8)] +                                      # 265 rows x 8 parts: TileF16, 265 % 16 = 9
    [_case("post_self", "f32", 5, 53, n) for n in (1, 2, 4)] +
    [_case("post_self", "f32", 3, 7), _case("post_self", "f32", 5, 53)] +        # the wrapper's own n_parts
    [_case("post_self", p, B, Q) for p in LP for B, Q in LP_BQ] +
    [_case("post_self", "f16", B, Q, tile32=1) for B, Q in Q32_BQ] +
    [_case("post_self", "f16", 3, 11, 8, tile32=1), _case("post_self", "f16", *BIG_BQ)])

# dec_heads: opts is a set of letters -- b: linear2's bias, n: the FFN norm, l: unit length, (wq is its own field), o: no `out`,
# d: want_d, z: zero_row_any; the default of the shape tables is everything on (what a decoder layer runs)
FULL = "bdlnz"
HEADS_SHAPE_CASES = tuple(
    [_case("heads", "f32", 4, 256, 8, True, opts=FULL), _case("heads", "f32", 5, 205, 8, True, opts=FULL),      # 1024 / 1025 rows with wq
     _case("heads", "f32", 8, 256, 8, False, opts=FULL), _case("heads", "f32", 3, 683, 8, False, opts=FULL),    # 2048 / 2049 rows without
     _case("heads", "f32", 3, 7, 8, True, opts=FULL)] +
    [_case("heads", p, B, Q, 8, True, opts=FULL) for p in LP for B, Q in LP_BQ] +
    [_case("heads", "f16", B, Q, 8, True, tile32=1, opts=FULL) for B, Q in Q32_BQ] +
    [_case("heads", "f16", *BIG_BQ, 8, True, opts=FULL)])
# partial sums: 0, 1, 3, 8, 9 and 16 slices on TileF8, TileF16, TileQ16 and TileQ32 (PS = 4)
PARTS_COUNTS = (0, 1, 3, 8, 9, 16)
HEADS_PARTS_CASES = tuple(
    _case("heads", p, B, Q, n, True, t32, opts=FULL)
    for p, B, Q, t32 in (("f32", 3, 11, AUTO), ("f32", 5, 205, AUTO), ("f16", 3, 11, AUTO), ("f16", 3, 11, 1)) for n in PARTS_COUNTS)
# optional pieces: all 16 combinations of (bias, FFN norm, unit length, wq) in fp32; a pairwise-covering five in every 16-bit form
PAIRWISE = ((0, 0, 0, 0), (0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0))


def _optcase(prec, combo, extra="d"):
    b, n, l, w = combo
    return _case("heads", prec, 3, 7, 3, bool(w), opts="".join(sorted(("b" if b else "") + ("n" if n else "") + ("l" if l else "") + extra)))


HEADS_OPTION_CASES = tuple(
    [_optcase("f32", c) for c in itertools.product((0, 1), repeat=4)] + [_optcase(p, c) for p in LP for c in PAIRWISE] +
    [_optcase(p, (1, 1, 1, 1), extra) for p in ("f32", "f16") for extra in ("", "o", "z", "dz", "doz")])
HEADS_CASES = tuple(dict.fromkeys(HEADS_SHAPE_CASES + HEADS_PARTS_CASES + HEADS_OPTION_CASES))       # (three rows sit in two tables each)
ALL_CASES = CROSS_CASES + SELF_CASES + HEADS_CASES

# value cases of the row phases (wo = 0, bo = 0, so t = res exactly): (name, entries)
VALUE_CASES = ("shifted", "constant", "tiny", "huge", "zero_l2", "clamp")
VALUE_HEADS_ONLY = ("zero_l2", "clamp")
VALUE_SHAPES = (("f32", 1, 37, AUTO), ("f32", 5, 206, AUTO), ("bf16", 1, 37, AUTO), ("bf16x2", 1, 37, AUTO), ("f16", 1, 37, AUTO),
                ("f16", 1, 37, 1))
# sentinel runs: (prec, B, Q, n_parts, tile32) -- ragged last tiles and padding tiles (tile count no multiple of 8) on every tile kind
SENTINEL_SHAPES = (("f32", 3, 7, 4, AUTO), ("f32", 5, 205, 8, AUTO), ("bf16", 3, 7, 4, AUTO), ("bf16x2", 1, 17, 2, AUTO),
                   ("f16", 3, 11, 4, AUTO), ("f16", 3, 11, 4, 1), ("f16", 1, 1, 1, 1))


def table_kinds(cases=ALL_CASES):
    """(entry, tile kind) -> ids of the table rows that launch it."""
    out = {}
    for c in cases:
        out.setdefault((c.entry, c.kind), []).append(c.id)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# seeded inputs (fp32, CPU)
# ---------------------------------------------------------------------------------------------------------------------------
def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


WEIGHTS = ("wo", "w_in", "w1", "w2", "m0w", "m1w", "m2w", "wq")


@functools.lru_cache(maxsize=None)
def params():
    """One decoder layer's tail parameters: Linear weights scaled K^-0.5, biases 0.1, LayerNorm gains 1 +- 0.1."""
    P = dict(wo=rnd(E, E, seed=4, scale=E ** -0.5), bo=rnd(E, seed=5, scale=0.1), g=1 + rnd(E, seed=6, scale=0.1), b=rnd(E, seed=7, scale=0.1),
             w_in=rnd(3 * E, E, seed=8, scale=E ** -0.5), b_in=rnd(3 * E, seed=9, scale=0.1),
             w1=rnd(FF, E, seed=10, scale=E ** -0.5), b1=rnd(FF, seed=11, scale=0.1), w2=rnd(E, FF, seed=12, scale=FF ** -0.5),
             b2=rnd(E, seed=13, scale=0.1), g1=1 + rnd(E, seed=14, scale=0.1), be1=rnd(E, seed=15, scale=0.1),
             g2=1 + rnd(E, seed=16, scale=0.1), be2=rnd(E, seed=17, scale=0.1), wq=rnd(E, E, seed=40, scale=E ** -0.5),
             bq=rnd(E, seed=41, scale=0.1))
    for i in range(3):
        P[f"m{i}w"], P[f"m{i}b"] = rnd(E, E, seed=20 + i, scale=E ** -0.5), rnd(E, seed=30 + i, scale=0.1)
    return P


@functools.lru_cache(maxsize=None)
def inputs(B, Q):
    """attn_out o, residual res (B * Q, E) and query_pos (Q, E)."""
    return rnd(B * Q, E, seed=1), rnd(B * Q, E, seed=2), rnd(Q, E, seed=3)


@functools.lru_cache(maxsize=None)
def heads_inputs(B, Q, n_parts):
    """x (B * Q, E), parts (n_parts, B * Q, E) of the size of an FFN's partial sums, query_pos (Q, E)."""
    parts = rnd(n_parts, B * Q, E, seed=52, scale=max(n_parts, 1) ** -0.5) if n_parts else None
    return rnd(B * Q, E, seed=51), parts, rnd(Q, E, seed=3)


def value_case(name, rows, P):
    """(res, P') of a value case: res (rows, E); P' has wo = bo = 0 (t = res exactly) and the LayerNorm parameters of the case."""
    P = dict(P, wo=torch.zeros(E, E), bo=torch.zeros(E))
    x = rnd(rows, E, seed=61)
    if name == "shifted":                       # rows far from zero: mean 1e3, unit spread
        x = x + 1e3
    elif name == "constant":                    # zero variance: y = b
        c = torch.tensor([0.7, -3.25, 1000.0, 1.0 / 3.0, 0.0])
        x = c[torch.arange(rows) % 5][:, None].expand(rows, E).contiguous()
    elif name == "tiny":
        x = x * 1e-4
    elif name == "huge":
        x = x * 1e4
    elif name == "zero_l2":                     # a zero vector into the unit-length step
        P.update(g1=torch.zeros(E), be1=torch.zeros(E))
    elif name == "clamp":                       # |LN| ~ 1e-14: the norm is below the 1e-12 clamp
        P.update(g1=P["g1"] * 1e-14, be1=torch.zeros(E))
    else:
        raise KeyError(name)
    return x, P


# ---------------------------------------------------------------------------------------------------------------------------
# operand forms
# ---------------------------------------------------------------------------------------------------------------------------
def _bf16_pair(t):
    hi = t.to(torch.bfloat16).float()
    return hi, (t - hi).to(torch.bfloat16).float()


class Form:
    """How a precision rounds the two operands of every GEMM.  ``w(W)``: the fp32 matrix the products use (hi + lo is exact in fp32:
    17 significant bits); ``w_seq(W)``: the K-order the kernel walks (bf16x2: all hi chunks, then all lo chunks); ``a(t)``: a GEMM
    input, rounded in fp32 whatever dtype it arrives in (the kernels hold fp32 tiles) and returned in that dtype."""

    def __init__(self, prec):
        assert prec in PRECS
        self.prec = prec

    def w(self, W):
        if self.prec == "bf16":
            return W.to(torch.bfloat16).float()
        if self.prec == "f16":
            return W.to(torch.float16).float()
        if self.prec == "bf16x2":
            hi, lo = _bf16_pair(W)
            return hi + lo
        return W

    def w_seq(self, W):
        if self.prec == "bf16x2":
            return torch.cat(_bf16_pair(W), 1)
        return self.w(W)

    def a(self, t):
        if self.prec == "f32":
            return t
        t32 = t.float()
        if self.prec == "f16":
            r = t32.clamp(-65504.0, 65504.0).to(torch.float16).float()
        else:
            hi, lo = _bf16_pair(t32)
            r = hi + lo
        return r.to(t.dtype)

    # relative size of one operand rounding: what a rounding-boundary flip of a GEMM input costs per product
    @property
    def flip(self):
        return {"f32": 0.0, "bf16": 2.0 ** -16, "bf16x2": 2.0 ** -16, "f16": 2.0 ** -10}[self.prec]


# ---------------------------------------------------------------------------------------------------------------------------
# arithmetic: float64 (the definitions) and the two fp32 yardsticks
# ---------------------------------------------------------------------------------------------------------------------------
def linear_seq(a, w, bias):
    """a w^T + bias in fp32 with ONE accumulator per output walked strictly in k order; the bias is added last (gemm_store)."""
    wt = w.t().contiguous()
    acc = torch.zeros(a.shape[0], w.shape[0])
    a = a.contiguous()
    for k in range(a.shape[1]):
        acc.addcmul_(a[:, k:k + 1], wt[k:k + 1])
    return acc if bias is None else acc + bias


class Arith:
    """mode "f64": the definitions (two-pass biased LayerNorm, x / max(|x|, 1e-12), a w^T + b in float64);
    "linear" / "seq": torch's fp32 row phases (F.layer_norm, F.normalize) around F.linear / linear_seq;
    "order": the "linear" arithmetic in another order of the same fp32 operations -- the k index of every GEMM and the columns of
    every row reduction permuted (seeded by ``order``) -- see evaluate_orders."""

    def __init__(self, mode, form, order=0):
        assert mode in ("f64", "linear", "seq", "order")
        self.mode, self.form, self.order = mode, form, order
        self.dt = torch.float64 if mode == "f64" else torch.float32
        self.k_path, self.mag, self.gain = 0, 1.0, 1.0          # f64 only: what tests/test_dec_cases_cpu.py builds its bound from
        self.inputs, self.weights = [], []                      # the input of every GEMM, in call order, before the form rounds it; its W

    def c(self, t):
        return t.to(self.dt)

    def _perm(self, n):
        return torch.randperm(n, generator=torch.Generator().manual_seed(1000 * self.order + n + len(self.inputs)))

    def lin(self, a, W, bias):
        self.inputs.append(a)
        self.weights.append(W)
        a = self.form.a(a)
        if self.mode == "seq":
            a_ = torch.cat([a, a], 1) if self.form.prec == "bf16x2" else a
            return linear_seq(a_, self.form.w_seq(W), bias)
        w = self.form.w(W)
        if self.mode == "linear":
            return F.linear(a, w, bias)
        if self.mode == "order":
            p = self._perm(W.shape[1])
            return F.linear(a[:, p].contiguous(), w[:, p].contiguous(), bias)
        y = a @ w.double().t()
        m = a.abs() @ w.double().abs().t()
        if bias is not None:
            y, m = y + bias.double(), m + bias.double().abs()
        self.k_path += W.shape[1]
        self.mag = max(self.mag, float(m.max()))
        return y

    def ln(self, v, g, b, eps=1e-5):
        if self.mode == "order":
            p = self._perm(v.shape[-1])
            return F.layer_norm(v[:, p].contiguous(), (v.shape[-1],), g[p], b[p], eps)[:, torch.argsort(p)]
        if self.mode != "f64":
            return F.layer_norm(v, (v.shape[-1],), g, b, eps)
        mean = v.mean(-1, keepdim=True)
        var = ((v - mean) ** 2).mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(var + eps)
        self.k_path += v.shape[-1]
        self.gain *= max(1.0, float((rstd * g.double().abs()).max()))
        self.mag = max(self.mag, float(v.abs().max()))
        return (v - mean) * rstd * g.double() + b.double()

    def l2(self, v):
        if self.mode == "order":
            p = self._perm(v.shape[-1])
            return F.normalize(v[:, p].contiguous(), p=2, dim=-1, eps=1e-12)[:, torch.argsort(p)]
        if self.mode != "f64":
            return F.normalize(v, p=2, dim=-1, eps=1e-12)
        n = torch.sqrt((v * v).sum(-1, keepdim=True)).clamp_min(1e-12)
        self.k_path += v.shape[-1]
        self.gain *= max(1.0, float((1.0 / n).max()))
        return v / n


def post_cross(ar, o, res, qpos, P, x_in=None):
    """x = LN(res + o wo^T + bo); qk = (x + query_pos) w_in[:2E]^T + b_in[:2E]; v = x w_in[2E:]^T + b_in[2E:].  o, res (rows, E);
    x_in: the x the projections read instead of the chain's own (the kernel's output)."""
    x = ar.ln(ar.c(res) + ar.lin(ar.c(o), P["wo"], P["bo"]), P["g"], P["b"])
    xs = x if x_in is None else ar.c(x_in)
    qp = ar.c(qpos).repeat(o.shape[0] // qpos.shape[0], 1)             # (Q, E) over the images, or one row per row already
    qk = ar.lin(xs + qp, P["w_in"][:2 * E], P["b_in"][:2 * E])
    v = ar.lin(xs, P["w_in"][2 * E:], P["b_in"][2 * E:])
    return x, qk, v


def post_self(ar, o, res, P, x_in=None):
    """x as above; ffn = relu(x w1^T + b1) w2^T (the sum of the partial sums; linear2's bias is the heads')."""
    x = ar.ln(ar.c(res) + ar.lin(ar.c(o), P["wo"], P["bo"]), P["g"], P["b"])
    xs = x if x_in is None else ar.c(x_in)
    h = torch.relu(ar.lin(xs, P["w1"], P["b1"]))
    return x, ar.lin(h, P["w2"], None)


def heads(ar, x, parts, qpos, P, *, bias=True, norm=True, l2norm=True, wq=True, out_in=None):
    """t = x + sum(parts) [+ b2] [-> LN] [-> unit length]; d = LN_dec(t); e = MLP3(d); q = (t + query_pos) wq^T + bq.
    out_in: the t the query projection reads instead of the chain's own (the kernel's ``out``).  Returns (t, d, e, q | None)."""
    t = ar.c(x)
    if parts is not None and parts.shape[0]:
        t = t + ar.c(parts).sum(0)
    if bias:
        t = t + ar.c(P["b2"])
    if norm:
        t = ar.ln(t, P["g1"], P["be1"])
    if l2norm:
        t = ar.l2(t)
    d = ar.ln(t, P["g2"], P["be2"])
    e = d
    for i in range(3):
        e = ar.lin(e, P[f"m{i}w"], P[f"m{i}b"])
        if i < 2:
            e = torch.relu(e)
    q = None
    if wq:
        ts = t if out_in is None else ar.c(out_in)
        q = ar.lin(ts + ar.c(qpos).repeat(x.shape[0] // qpos.shape[0], 1), P["wq"], P["bq"])
    return t, d, e, q


def evaluate(chain, prec, *args, **kw):
    """(ref, [yard_linear, yard_seq]): the float64 definition on the form's operands and the two fp32 yardsticks; each a tuple of
    the chain's outputs."""
    form = Form(prec)
    return chain(Arith("f64", form), *args, **kw), [chain(Arith(m, form), *args, **kw) for m in ("linear", "seq")]


# The fp16 form and its hidden intermediates.  One fp16 term per activation makes a rounding boundary expensive: a hidden value (FFN
# hidden, MLP hidden, d) that an fp32 evaluation puts on the other side of a boundary than float64 enters its GEMM 2^-10 of itself
# away, some hundred fp32 roundings of the sum it enters.  Every fp32 evaluation has its own such elements: in the 200-row table
# case 73 % of the rows of one F.linear evaluation hold at least one in the FFN's hidden input and 29 % in the MLP's three inputs
# (``crossings``; tests/test_dec_cases_cpu.py asserts the counts), so two evaluations of one row, or of a five-row last tile, often
# hold none where a third, equally accurate one holds one.  That is a sampling problem of the yardstick and is treated as one: for
# the outputs behind a hidden intermediate (the FFN sum, e), over at most ORDER_ROWS rows, the yardstick is joined by N_ORDERS more
# honest fp32 evaluations -- the F.linear arithmetic with the k index of every GEMM and the columns of every row reduction in
# another (seeded) order.  Nothing is rounded any way an fp32 evaluation would not round it.  Outputs whose GEMM input is an exact
# input or an output of the kernel (x, qk, v, q) and the row phases (out, d) keep the two yardsticks, and so does every other form
# (a bf16 hi + lo pair moves by 2^-17 of the value across a boundary, the size of an fp32 rounding).  N_ORDERS from the counts above:
# a crossing's cost varies with the binade of the value and the weight it meets, so a row should be sampled until it has met
# several; at 0.29 per evaluation, 2 + 30 evaluations of one row of the MLP meet nine on average and none with probability 2e-5.
N_ORDERS = 30
ORDER_ROWS = 64


def evaluate_orders(chain, prec, *args, **kw):
    """N_ORDERS further fp32 evaluations of the chain, each in its own order of the same operations (Arith mode "order")."""
    form = Form(prec)
    return [chain(Arith("order", form, j + 1), *args, **kw) for j in range(N_ORDERS)]


def crossings(form, ar64, ar32):
    """Per GEMM of a chain, a (rows, K) mask of the inputs that the fp32 evaluation ``ar32`` rounds to another operand than the
    float64 evaluation ``ar64`` does (both Arith objects after the chain ran)."""
    return [form.a(a32) != form.a(a64).float() for a64, a32 in zip(ar64.inputs, ar32.inputs)]


def heads_kw(case):
    return dict(bias="b" in case.opts, norm="n" in case.opts, l2norm="l" in case.opts, wq=case.wq)


# ---------------------------------------------------------------------------------------------------------------------------
# the weight-fragment orders of the four pack functions (include/msm_hip.h)
# ---------------------------------------------------------------------------------------------------------------------------
def frag_f32(w):
    """packed[((t*(K/64) + kc)*4 + u)*256 + (lq*16 + lj)*4 + c] = W[t*16 + lj][kc*64 + u*16 + lq*4 + c]"""
    N, K = w.shape
    return w.view(N // 16, 16, K // 64, 4, 4, 4).permute(0, 2, 3, 4, 1, 5).contiguous().view(N, K)


def _frag16(m):
    N, K = m.shape
    return m.view(N // 16, 16, K // 64, 2, 2, 4, 4).permute(0, 2, 3, 5, 1, 4, 6).contiguous().view(N // 16, K // 64, 1024)


def frag_16(w, dtype):
    """packed[(((t*(K/64) + kc)*2 + up)*64 + lq*16 + lj)*8 + h*4 + c] = dtype(W[t*16 + lj][kc*64 + (2*up + h)*16 + lq*4 + c])"""
    return _frag16(w).to(dtype).reshape(w.shape)


def frag_bf16x2(w):
    """per row tile: the K / 64 chunks of bf16(W) in the order of frag_16, then the K / 64 chunks of bf16(W - bf16(W))"""
    hi = w.to(torch.bfloat16)
    return torch.cat([_frag16(hi.float()).to(torch.bfloat16), _frag16(w - hi.float()).to(torch.bfloat16)], 1).reshape(w.shape[0], 2 * w.shape[1])
