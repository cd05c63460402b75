"""csrc/dec_chain.hip (msm_dec_post_cross / msm_dec_post_self / msm_dec_heads in all four operand forms) on every tile kind, row edge
and optional piece, against the float64 definitions of tests/dec_cases.py.

THE RULE of every comparison in this file (``Rule.check`` below), tests/test_gpu_norm.py's: on one input compute the float64
definition ``ref``, the CPU yardsticks and the kernel result ``got``, and assert

    max|got - ref| <= max(4 * e_yard, 4 * eps_fp32 * max|ref|)

over ALL elements, and again over the rows of the last tile alone with the yardstick taken on those same rows.  ``e_yard`` is the
larger error of the two CPU yardsticks of the precision against the same ``ref`` (dec_cases: operands rounded as the form rounds
them, fp32 accumulation by F.linear and by one accumulator per output walked in k order, torch's fp32 row phases).  One exception,
a matter of sampling and not of tolerance: the fp16 form rounds hidden activations to ONE fp16 term, a hidden value that an fp32
evaluation puts across a rounding boundary costs 2^-10 of itself (a hundred fp32 roundings), and over one row or a five-row last
tile two evaluations often meet no such element where the kernel meets one -- measured with two: e of one row 1.2e-4 against
5.4e-7, the FFN sum of a last tile 3.7e-5 against 4.4e-6, d and out of the same calls at 0.9 - 1.2.  For the FFN sum and e of the
fp16 form, over at most dec_cases.ORDER_ROWS rows, e_yard is therefore the largest error of the two yardsticks AND of
dec_cases.N_ORDERS further honest fp32 evaluations in other summation orders (dec_cases.evaluate_orders); every other output, scope
and form has the two.  The yardstick is never the kernel.
Where a stage's input is an output of the kernel (x -> qk, v; x -> the FFN; out -> q) reference and yardstick take the kernel's own
output, so errors do not compound across stages; hidden intermediates (FFN hidden, MLP hidden, the row phases of the heads) the
yardstick computes and rounds itself, which gives it the kernel's kind of rounding-boundary flips -- one factor serves fp32, bf16,
bf16x2 and f16.  No tolerance is chosen per case.  Every comparison prints a RULE line (pytest -s); the worst
ratios per (entry point, tile kind, precision) are printed at the end of the module and recorded in DESIGN.md section 4e.
Needs a real MI355X (pytest -m gpu)."""
import ctypes
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dec_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS32 = float(torch.finfo(torch.float32).eps)
SENTINEL = -12345.5
E = C.E
SUFFIX = {"f32": "", "bf16": "_bf16", "bf16x2": "_bf16x2", "f16": "_f16"}
WORST = {}                                     # (entry, tile kind, precision) -> (ratio, where)


def ops():
    from unseenobjectswithmeanshift_amd import ops as _ops
    return _ops


def dev(t):
    return None if t is None else t.to(DEV)


@pytest.fixture(scope="module", autouse=True)
def worst_ratios():
    yield
    print()
    for (entry, kind, prec), (ratio, where) in sorted(WORST.items()):
        print(f"WORST {entry:10s} {kind:9s} {prec:6s} kernel / yardstick {ratio:5.2f}  {where}")


class Rule:
    """One test's comparisons: every output is checked and printed before the test fails on the first miss."""

    def __init__(self, entry, kind, prec, case, rows):
        self.key, self.case, self.misses = (entry, kind, prec), case, []
        self.last = (C.cdiv(rows, C.TILE_ROWS[kind]) - 1) * C.TILE_ROWS[kind]          # first row of the last tile
        self.first_order = 0 if rows <= C.ORDER_ROWS else self.last                    # the rows dec_cases.evaluate_orders is run on

    def orders(self, chain, *args, **kw):
        """The further evaluation orders of the fp16 form over rows [first_order:] (args already cut to those rows); else None."""
        return C.evaluate_orders(chain, self.key[2], *args, **kw) if self.key[2] == "f16" else None

    def check(self, name, got, ref, yards, orders=None):
        got = got.detach().cpu().double().reshape(ref.shape)
        assert bool(torch.isfinite(got).all()), f"{self.case} {name}: not finite"
        for scope, first in (("all rows", 0), ("last tile", self.last)):
            g, r = got[first:], ref[first:]
            e_k = float((g - r).abs().max())
            ys = [y[first:] for y in yards]
            if orders is not None and first >= self.first_order:
                ys += [y[first - self.first_order:] for y in orders]
            e_y = max(float((y.double() - r).abs().max()) for y in ys)
            floor = EPS32 * float(r.abs().max())
            bound = max(4.0 * e_y, 4.0 * floor)
            ratio = e_k / e_y if e_y > 0 else (0.0 if e_k == 0 else float("inf"))
            print(f"RULE [{self.key[0]} {self.key[1]} {self.key[2]}] {self.case} {name} {scope}: kernel {e_k:.3e} yardstick {e_y:.3e} "
                  f"ratio {ratio:.2f} bound {bound:.3e}")
            used = e_k / max(e_y, floor) if max(e_y, floor) > 0 else 0.0              # of the bound's quarter: passes iff <= 4
            if used > WORST.get(self.key, (-1.0, ""))[0]:
                WORST[self.key] = (used, f"{self.case} {name} {scope}")
            if not e_k <= bound:
                self.misses.append(f"{self.case} {name} {scope}: max|got - ref| = {e_k:.3e} > {bound:.3e} (yardstick {e_y:.3e})")

    def done(self):
        assert not self.misses, "\n".join(self.misses)


# ---------------------------------------------------------------------------------------------------------------------------
# device operands and the three calls
# ---------------------------------------------------------------------------------------------------------------------------
def pack(prec, w):
    return {"f32": ops().dec_pack_weight, "bf16": ops().dec_pack_weight_bf16, "bf16x2": ops().dec_pack_weight_bf16x2,
            "f16": ops().dec_pack_weight_f16}[prec](dev(w))


def device_params(prec, P):
    return {k: (pack(prec, v) if k in C.WEIGHTS else dev(v)) for k, v in P.items()}


@functools.lru_cache(maxsize=None)
def default_device_params(prec):
    return device_params(prec, C.params())


def dparams(prec, P):
    return default_device_params(prec) if P is C.params() else device_params(prec, P)


def bq3(t, B, Q):
    return None if t is None else dev(t).view(*t.shape[:-2], B, Q, t.shape[-1])


def call_cross(D, o, res, qpos, B, Q):
    return ops().dec_post_cross(bq3(o, B, Q), bq3(res, B, Q), dev(qpos), D["wo"], D["bo"], D["g"], D["b"], D["w_in"], D["b_in"])


def call_self(D, o, res, B, Q, n_parts=None):
    return ops().dec_post_self(bq3(o, B, Q), bq3(res, B, Q), D["wo"], D["bo"], D["g"], D["b"], D["w1"], D["b1"], D["w2"], n_parts=n_parts)


def call_heads(D, x, parts, qpos, B, Q, *, bias=True, norm=True, l2norm=True, wq=True, opts=""):
    kw = dict(parts=bq3(parts, B, Q), l2norm=l2norm, want_out="o" not in opts, want_d="d" in opts, zero_row_any="z" in opts)
    if bias:
        kw.update(bias=D["b2"])
    if norm:
        kw.update(ln_g=D["g1"], ln_b=D["be1"])
    if wq:
        kw.update(wq=D["wq"], bq=D["bq"], query_pos=dev(qpos))
    mlp = [(D[f"m{i}w"], D[f"m{i}b"]) for i in range(3)]
    r = ops().dec_heads(bq3(x, B, Q), D["g2"], D["be2"], mlp, **kw)
    return r if "z" in opts else r + (None,)


def rows2(t):
    return None if t is None else t.detach().cpu().reshape(-1, t.shape[-1])


def set_tile32(lib_option, tile32):
    if tile32 != C.AUTO:
        lib_option("DEC_TILE32", tile32)


def check_cross(rule, prec, o, res, qpos, B, Q, P):
    x, qk, v = call_cross(dparams(prec, P), o, res, qpos, B, Q)
    assert x.shape == (B, Q, E) and qk.shape == (B, Q, 2 * E) and v.shape == (B, Q, E)
    ref, yards = C.evaluate(C.post_cross, prec, o, res, qpos, P, x_in=rows2(x))
    for i, (name, got) in enumerate((("x", x), ("qk", qk), ("v", v))):
        rule.check(name, got, ref[i], [y[i] for y in yards])
    return x, qk, v


def check_self(rule, prec, o, res, B, Q, P, n_parts=None):
    x, parts = call_self(dparams(prec, P), o, res, B, Q, n_parts)
    assert x.shape == (B, Q, E) and parts.shape[1:] == (B, Q, E) and (n_parts is None or parts.shape[0] == n_parts)
    ref, yards = C.evaluate(C.post_self, prec, o, res, P, x_in=rows2(x))
    rule.check("x", x, ref[0], [y[0] for y in yards])
    f = rule.first_order
    more = rule.orders(C.post_self, o[f:], res[f:], P, x_in=rows2(x)[f:])
    rule.check("parts.sum(0)", parts.double().sum(0), ref[1], [y[1] for y in yards], None if more is None else [y[1] for y in more])
    return x, parts


def check_heads(rule, prec, x, parts, qpos, B, Q, P, kw, opts):
    out, d, e, q, ra = call_heads(dparams(prec, P), x, parts, qpos, B, Q, opts=opts, **kw)
    assert (out is None) == ("o" in opts) and (d is None) == ("d" not in opts) and (q is None) == (not kw["wq"]) and (ra is None) == ("z" not in opts)
    ref, yards = C.evaluate(C.heads, prec, x, parts, qpos, P, out_in=rows2(out), **kw)
    f = rule.first_order
    more = rule.orders(C.heads, x[f:], None if parts is None else parts[:, f:], qpos.repeat(B, 1)[f:], P,
                       out_in=None if out is None else rows2(out)[f:], **kw)
    for i, (name, got) in enumerate((("out", out), ("d", d), ("e", e), ("q", q))):
        if got is not None:
            rule.check(name, got, ref[i], [y[i] for y in yards], [y[i] for y in more] if more is not None and name == "e" else None)
    if ra is not None:
        assert ra.dtype == torch.int32 and ra.shape == (B, Q) and not bool(ra.any())
    return out, d, e, q


# ---------------------------------------------------------------------------------------------------------------------------
# every table row under the rule
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.CROSS_CASES, ids=lambda c: c.id)
def test_post_cross(case, lib_option):
    set_tile32(lib_option, case.tile32)
    rule = Rule("post_cross", case.kind, case.prec, case.id, case.rows)
    check_cross(rule, case.prec, *C.inputs(case.B, case.Q), case.B, case.Q, C.params())
    rule.done()


@pytest.mark.parametrize("case", C.SELF_CASES, ids=lambda c: c.id)
def test_post_self(case, lib_option):
    set_tile32(lib_option, case.tile32)
    rule = Rule("post_self", case.kind, case.prec, case.id, case.rows)
    o, res, _ = C.inputs(case.B, case.Q)
    check_self(rule, case.prec, o, res, case.B, case.Q, C.params(), case.n_parts)
    rule.done()


@pytest.mark.parametrize("case", C.HEADS_CASES, ids=lambda c: c.id)
def test_heads(case, lib_option):
    set_tile32(lib_option, case.tile32)
    rule = Rule("heads", case.kind, case.prec, case.id, case.rows)
    kw = C.heads_kw(case)
    out, _, _, _ = check_heads(rule, case.prec, *C.heads_inputs(case.B, case.Q, case.n_parts), case.B, case.Q, C.params(), kw, case.opts)
    if kw["l2norm"] and out is not None:                               # the definition: every row is an fp32 unit vector
        assert float((out.double().norm(dim=-1) - 1).abs().max()) <= 1e-6
    rule.done()


# ---------------------------------------------------------------------------------------------------------------------------
# value cases of the row phases: wo = 0, bo = 0, so t = res exactly
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", C.VALUE_SHAPES, ids=lambda s: f"{s[0]}-{s[1]}x{s[2]}" + ("" if s[3] == C.AUTO else f"-t32_{s[3]}"))
@pytest.mark.parametrize("name", C.VALUE_CASES)
def test_row_phase_value_cases(name, shape, lib_option):
    prec, B, Q, tile32 = shape
    rows = B * Q
    set_tile32(lib_option, tile32)
    val, P = C.value_case(name, rows, C.params())
    o, _, qpos = C.inputs(B, Q)
    case = f"{name} {prec} {B}x{Q}"
    if name not in C.VALUE_HEADS_ONLY:
        for entry in ("post_cross", "post_self"):
            rule = Rule(entry, C.tile_kind(entry, prec, rows, tile32=tile32), prec, case, rows)
            x = (check_cross(rule, prec, o, val, qpos, B, Q, P) if entry == "post_cross" else check_self(rule, prec, o, val, B, Q, P))[0]
            if name == "constant":                                      # zero variance: y == b up to the rule
                b = P["b"].double().expand(rows, E)
                rule.check("x against b", x, b, [b])
            rule.done()
    kw = dict(bias=False, norm=True, l2norm=True, wq=True)
    rule = Rule("heads", C.tile_kind("heads", prec, rows, wq=True, tile32=tile32), prec, case, rows)
    out, d, e, q = check_heads(rule, prec, val, None, qpos, B, Q, P, kw, "d")
    if name == "zero_l2":                                               # 0 / max(0, 1e-12): exactly 0, never NaN
        assert torch.equal(out.cpu(), torch.zeros(B, Q, E)) and bool(torch.isfinite(d).all())
    elif name == "clamp":
        # a precondition on the INPUT, not a tolerance (as in test_gpu_norm.py): the norm (~1e-13) is below the clamp, so out = LN / 1e-12
        # is neither a unit vector (max ~0.2) nor zero
        assert 1e-3 < float(out.abs().max()) < 0.2
    else:
        assert float((out.double().norm(dim=-1) - 1).abs().max()) <= 1e-6
    rule.done()


# ---------------------------------------------------------------------------------------------------------------------------
# relations, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,B,Q", [("f32", 5, 53), ("f32", 5, 205), ("bf16", 3, 11), ("bf16x2", 3, 11), ("f16", 3, 11)])
def test_post_self_n_parts_return_the_same_x(prec, B, Q):
    """x does not depend on how the hidden dimension is shared out.  In fp32 the split also picks the tile kind (use_tile8) and the
    8-row and 16-row forms add a row's products in different orders: there the variants of one tile kind return the same bits."""
    o, res, _ = C.inputs(B, Q)
    D = default_device_params(prec)
    got = {}
    for n in (1, 2, 4, 8):
        x, parts = call_self(D, o, res, B, Q, n)
        got.setdefault(C.tile_kind("post_self", prec, B * Q, n), []).append((n, x))
    assert prec != "f32" or len(got) == 2
    for kind, xs in got.items():
        for n, x in xs[1:]:
            assert torch.equal(x, xs[0][1]), f"{kind}: n_parts={n} against n_parts={xs[0][0]}"


def all_outputs(prec, B, Q, n_parts, prefetch=None):
    """Every output of the three calls on the table inputs; ``prefetch`` (a function of the device parameters) is requested in
    front of each of them."""
    D = default_device_params(prec)
    o, res, qpos = C.inputs(B, Q)
    x, parts, _ = C.heads_inputs(B, Q, n_parts)
    outs = []
    for call in (lambda: call_cross(D, o, res, qpos, B, Q), lambda: call_self(D, o, res, B, Q, n_parts),
                 lambda: call_heads(D, x, parts, qpos, B, Q, opts="dz")):
        if prefetch is not None:
            ops().dec_set_prefetch(prefetch(D))
        outs += list(call())
    return outs


@pytest.mark.parametrize("B,Q", [(1, 31), (3, 11), (3, 21), (2, 100)])
def test_32_row_tiles_equal_16_row_tiles(B, Q, lib_option):
    """A row's arithmetic does not depend on the tile it sits in: TileQ32 returns what TileQ16 returns, n_parts = 8 included (two trips
    of the heads' partial-sum loop where the 16-row form takes one)."""
    got = {}
    for tile32 in (0, 1):
        lib_option("DEC_TILE32", tile32)
        got[tile32] = all_outputs("f16", B, Q, 8)
    for a, b in zip(got[0], got[1]):
        assert torch.equal(a, b)


SHAPE_IDS = lambda s: f"{s[0]}-{s[1]}x{s[2]}-p{s[3]}" + ("" if s[4] == C.AUTO else f"-t32_{s[4]}")      # noqa: E731


PREFETCH = {"none": None, "one_prefetch_row": lambda D: [D["bo"]], "two_prefetch_rows": lambda D: [D["w1"], D["w2"], None, D["m0w"]]}


@pytest.mark.parametrize("shape", C.SENTINEL_SHAPES, ids=SHAPE_IDS)
def test_prefetch_request_and_repeat_change_nothing(shape, lib_option):
    """A pending dec_set_prefetch request appends one or two rows of workgroups to the grid (gridDim.y, which the 8-row post_cross
    reads to tell its two-part form) and must not change a bit; neither must calling twice.  Every entry on every tile kind.  The
    outputs of a call are poisoned before they are freed, so that a later call that skips a store does not find the right values in
    recycled memory (test_writes_only_its_rows makes the same comparison inside sentinel-filled buffers)."""
    prec, B, Q, n_parts, tile32 = shape
    set_tile32(lib_option, tile32)

    def poison(outs):
        for t in outs:
            t.fill_(-1 if t.dtype == torch.int32 else float("nan"))

    poison(all_outputs(prec, B, Q, n_parts))
    base = [t.clone() for t in all_outputs(prec, B, Q, n_parts)]
    for what, pf in (("repeat", None),) + tuple(PREFETCH.items())[1:]:
        outs = all_outputs(prec, B, Q, n_parts, pf)
        for i, (a, b) in enumerate(zip(base, outs)):
            assert torch.equal(a, b), f"{what}: output {i}"
        poison(outs)
    ops().dec_set_prefetch([])                                          # (an empty list clears a pending request: none is left)


# ---------------------------------------------------------------------------------------------------------------------------
# writes only its rows
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefetch", PREFETCH)
@pytest.mark.parametrize("shape", C.SENTINEL_SHAPES, ids=SHAPE_IDS)
def test_writes_only_its_rows(shape, prefetch, lib_option):
    """Ragged last tiles clamp their loads and guard their stores with ``row < valid``; the padding tiles of tile_grid_x return at
    once.  Every output of the three C entry points sits inside a sentinel-filled buffer: the rows behind ``rows`` and the words in
    front of the buffer stay untouched, and what is inside equals the wrapper's result -- also with a prefetch request pending in
    front of each call (a row the kernel then skipped would keep its sentinels).  (The slices of ``parts`` are rows * E apart
    by definition: a store behind a slice's rows would land in the next slice and break the equality.)"""
    from unseenobjectswithmeanshift_amd._lib import check, lib
    prec, B, Q, n_parts, tile32 = shape
    set_tile32(lib_option, tile32)
    rows, pad = B * Q, 40 * 2 * E                                        # more than a whole 32-row tile of the widest output
    D = default_device_params(prec)
    o, res, qpos = [dev(t) for t in C.inputs(B, Q)]
    xh, parts_in, _ = [dev(t) for t in C.heads_inputs(B, Q, n_parts)]
    want = all_outputs(prec, B, Q, n_parts)                              # x, qk, v | x, parts | out, d, e, q, row_any
    widths = [E, 2 * E, E, E, n_parts * E, E, E, E, E, 1]                # floats per row (parts: all slices), row_any: one int32
    bufs = [torch.full((2 * pad + rows * w,), SENTINEL, device=DEV) if w != 1 else torch.full((2 * pad + rows,), -7, device=DEV, dtype=torch.int32)
            for w in widths]
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + 4 * off)
    o_ = lambda i: p(bufs[i], pad)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    sfx = SUFFIX[prec]

    def request():
        if PREFETCH[prefetch] is not None:
            ops().dec_set_prefetch(PREFETCH[prefetch](D))

    request()
    rc = getattr(lib(), "msm_dec_post_cross" + sfx)(p(o), p(res), p(qpos), p(D["wo"]), p(D["bo"]), p(D["g"]), p(D["b"]), p(D["w_in"]), p(D["b_in"]),
                                                    o_(0), o_(1), o_(2), rows, Q, E, 1e-5, stream)
    check(rc, "msm_dec_post_cross")
    request()
    rc = getattr(lib(), "msm_dec_post_self" + sfx)(p(o), p(res), p(D["wo"]), p(D["bo"]), p(D["g"]), p(D["b"]), p(D["w1"]), p(D["b1"]), p(D["w2"]), C.FF,
                                                   o_(3), o_(4), n_parts, rows, E, 1e-5, stream)
    check(rc, "msm_dec_post_self")
    request()
    rc = getattr(lib(), "msm_dec_heads" + sfx)(p(xh), p(parts_in), n_parts, p(D["b2"]), p(D["g1"]), p(D["be1"]), 1, p(D["g2"]), p(D["be2"]),
                                               p(D["m0w"]), p(D["m0b"]), p(D["m1w"]), p(D["m1b"]), p(D["m2w"]), p(D["m2b"]), p(D["wq"]), p(D["bq"]), p(qpos),
                                               o_(5), o_(6), o_(7), o_(8), o_(9), rows, Q, E, 1e-5, stream)
    check(rc, "msm_dec_heads")
    for i, (buf, w, ref) in enumerate(zip(bufs, widths, want)):
        fill = -7 if w == 1 else SENTINEL
        assert torch.equal(buf[pad:pad + rows * w], ref.reshape(-1)), f"output {i}"
        assert bool((buf[:pad] == fill).all()), f"output {i}: words in front of the buffer"
        assert bool((buf[pad + rows * w:] == fill).all()), f"output {i}: rows behind `rows`"


# ---------------------------------------------------------------------------------------------------------------------------
# rejections
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", C.PRECS)
def test_rejections(prec):
    B, Q = 1, 7
    D = default_device_params(prec)
    o, res, qpos = C.inputs(B, Q)
    x, parts, _ = C.heads_inputs(B, Q, 3)
    mlp = [(D[f"m{i}w"], D[f"m{i}b"]) for i in range(3)]
    for n in (3, 5, 16):                                                # F / 256 = 8
        with pytest.raises(RuntimeError, match="must divide"):
            call_self(D, o, res, B, Q, n)
    with pytest.raises(RuntimeError, match="both be given or both be null"):
        ops().dec_heads(bq3(x, B, Q), D["g2"], D["be2"], mlp, ln_g=D["g1"])
    with pytest.raises(RuntimeError, match="both be given or both be null"):
        ops().dec_heads(bq3(x, B, Q), D["g2"], D["be2"], mlp, ln_b=D["be1"])
    with pytest.raises(RuntimeError, match="needs bq, query_pos and q_out"):
        ops().dec_heads(bq3(x, B, Q), D["g2"], D["be2"], mlp, wq=D["wq"], query_pos=dev(qpos))
    with pytest.raises(RuntimeError, match="needs bq, query_pos and q_out"):
        ops().dec_heads(bq3(x, B, Q), D["g2"], D["be2"], mlp, wq=D["wq"], bq=D["bq"])
    # nothing was launched by the rejected calls: the next call is the plain result
    out, d, e, q, _ = call_heads(D, x, parts, qpos, B, Q)
    assert bool(torch.isfinite(e).all()) and bool(torch.isfinite(q).all())
