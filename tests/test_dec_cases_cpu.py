"""tests/dec_cases.py checked on the CPU: the tables reach every (entry point, tile kind) the host can launch, the float64
definitions are torch's / the oracle's in float64, the fp32 yardsticks agree with them to fp32 accuracy row by row, and the
weight-fragment orders are the formulas of include/msm_hip.h."""
import itertools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dec_cases as C  # noqa: E402
from oracle import msm_oracle as O  # noqa: E402

E = C.E


def test_dispatch_restated():
    """The boundaries named in csrc/dec_chain.hip (use_tile8, use_tile32, DEC_TILE32) and ops.dec_post_self's default n_parts."""
    tk = C.tile_kind
    assert tk("post_cross", "f32", 1024) == "TileF8" and tk("post_cross", "f32", 1025) == "TileF16"
    assert tk("heads", "f32", 1024, wq=True) == "TileF8" and tk("heads", "f32", 1025, wq=True) == "TileF16"
    assert tk("heads", "f32", 2048) == "TileF8" and tk("heads", "f32", 2049) == "TileF16"
    assert tk("post_self", "f32", 255, 8) == "TileF8" and tk("post_self", "f32", 257, 8) == "TileF16"
    assert tk("post_self", "f32", 800, 8) == "TileF16"                       # the headline batch of 8
    assert C.default_n_parts(200) == 8 and C.default_n_parts(800) == 4 and C.default_n_parts(4500) == 1
    assert tk("post_self", "f32", 200) == "TileF8" and tk("post_self", "f32", 800) == "TileF16"
    for entry in ("post_self", "heads"):
        assert tk(entry, "f16", 4095) == "TileQ16" and tk(entry, "f16", 4096) == "TileQ32"
        assert tk(entry, "f16", 4500, tile32=0) == "TileQ16" and tk(entry, "f16", 1, tile32=1) == "TileQ32"
    assert tk("post_cross", "f16", 17300) == "TileQ16" and tk("post_cross", "f16", 31, tile32=1) == "TileQ32"
    assert tk("heads", "bf16", 5000) == "TileH16" and tk("post_self", "bf16x2", 5000) == "TileH16x2"
    assert C.HEADS_PS == {"TileF8": 8, "TileF16": 8, "TileH16": 8, "TileH16x2": 8, "TileQ16": 8, "TileQ32": 4}


def test_tables_reach_every_entry_and_tile_kind():
    got = C.table_kinds()
    for key in sorted(C.all_kinds()):
        assert key in got, f"no table row launches {key}"
        print(f"COVER {key[0]:10s} {key[1]:9s} {len(got[key]):3d} rows, e.g. {got[key][0]}")
    assert set(got) == C.all_kinds()
    assert len({c.id for c in C.ALL_CASES}) == len(C.ALL_CASES)


def test_tables_hold_the_named_edges():
    rows = lambda cases, prec: {c.rows for c in cases if c.prec == prec}
    assert {7, 1024, 1025} <= rows(C.CROSS_CASES, "f32")
    assert {(255, 8), (265, 8), (265, 1), (265, 2), (265, 4)} <= {(c.rows, c.n_parts) for c in C.SELF_CASES if c.prec == "f32"}
    assert {(1024, True), (1025, True), (2048, False), (2049, False), (21, True)} <= {(c.rows, c.wq) for c in C.HEADS_SHAPE_CASES if c.prec == "f32"}
    for cases in (C.CROSS_CASES, C.SELF_CASES, C.HEADS_SHAPE_CASES):
        for p in C.LP:
            assert {1, 15, 16, 17, 33, 200} <= rows(cases, p)
        assert {31, 33, 63} <= {c.rows for c in cases if c.kind == "TileQ32"}
    for cases in (C.SELF_CASES, C.HEADS_SHAPE_CASES):
        assert any(c.rows >= 4096 and c.tile32 == C.AUTO and c.kind == "TileQ32" for c in cases)
    assert max(c.rows for c in C.ALL_CASES) == 4500
    # ragged last tiles, padding tiles and tiles that straddle images
    c = next(c for c in C.CROSS_CASES if c.rows == 1025)
    assert c.kind == "TileF16" and 1025 % 16 == 1 and c.Q % 16 != 0 and C.grid_tiles(c.kind, c.rows) == (65, 72)
    # partial sums: every count on every PS, more than PS, no multiple of PS, two trips at 8 on TileQ32
    for kind in ("TileF8", "TileF16", "TileQ16", "TileQ32"):
        assert {c.n_parts for c in C.HEADS_PARTS_CASES if c.kind == kind} == set(C.PARTS_COUNTS)
    # optional pieces
    combos = lambda prec: {("b" in c.opts, "n" in c.opts, "l" in c.opts, c.wq) for c in C.HEADS_OPTION_CASES if c.prec == prec}
    assert len(combos("f32")) == 16
    for p in C.LP:
        for i, j in itertools.combinations(range(4), 2):
            assert {(c[i], c[j]) for c in combos(p)} == set(itertools.product((False, True), repeat=2)), (p, i, j)
    for letter in "odz":
        assert {letter in c.opts for c in C.HEADS_OPTION_CASES} == {False, True}
    # sentinel runs: a ragged last tile and padding tiles on every tile kind of every entry
    seen = set()
    for prec, B, Q, n_parts, t32 in C.SENTINEL_SHAPES:
        for entry in C.ENTRIES:
            kind = C.tile_kind(entry, prec, B * Q, n_parts, True, t32)
            tiles, grid = C.grid_tiles(kind, B * Q)
            assert (B * Q) % C.TILE_ROWS[kind] != 0 and grid != tiles
            seen.add((entry, kind))
    assert seen == C.all_kinds()


def test_float64_definitions_are_torchs():
    """post_cross / post_self / heads in float64 against nn.LayerNorm, nn.Linear and F.normalize in float64."""
    P = C.params()
    D = {k: v.double() for k, v in P.items()}
    B, Q = 3, 7
    o, res, qpos = C.inputs(B, Q)
    ar = lambda: C.Arith("f64", C.Form("f32"))

    def lin(w, b):
        m = torch.nn.Linear(w.shape[1], w.shape[0], bias=b is not None).double()
        with torch.no_grad():
            m.weight.copy_(w)
            if b is not None:
                m.bias.copy_(b)
        return m

    def norm(g, b):
        m = torch.nn.LayerNorm(E).double()
        with torch.no_grad():
            m.weight.copy_(g), m.bias.copy_(b)
        return m

    with torch.no_grad():
        xr = norm(D["g"], D["b"])(res.double() + lin(D["wo"], D["bo"])(o.double()))
        x, qk, v = C.post_cross(ar(), o, res, qpos, P)
        qp = qpos.double().repeat(B, 1)
        qkv = lin(D["w_in"], D["b_in"])
        torch.testing.assert_close(x, xr, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(qk, qkv(xr + qp)[:, :2 * E], rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(v, qkv(xr)[:, 2 * E:], rtol=1e-12, atol=1e-12)
        x2, ffn = C.post_self(ar(), o, res, P)
        ffn_r = lin(D["w2"], None)(F.relu(lin(D["w1"], D["b1"])(xr)))
        torch.testing.assert_close(x2, xr, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(ffn, ffn_r, rtol=1e-12, atol=1e-12)
        # heads: row phase against oracle.layernorm_chain, the MLP against oracle.prediction_heads
        xh, parts, _ = C.heads_inputs(B, Q, 3)
        t, d, e, q = C.heads(ar(), xh, parts, qpos, P)
        y, y2 = O.layernorm_chain(xh, parts, P["b2"], P["g1"], P["be1"], True, P["g2"], P["be2"])
        torch.testing.assert_close(t, y, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(d, y2, rtol=1e-12, atol=1e-12)
        tn = F.normalize(norm(D["g1"], D["be1"])(xh.double() + parts.double().sum(0) + D["b2"]), p=2, dim=-1, eps=1e-12)
        torch.testing.assert_close(t, tn, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(q, lin(D["wq"], D["bq"])(tn + qp), rtol=1e-12, atol=1e-12)
        # prediction_heads(sd, output (Q, B, E)): with an identity pixel embedding its mask IS the mask embedding
        sd = {"decoder_norm.weight": D["g2"], "decoder_norm.bias": D["be2"], "class_embed.weight": torch.zeros(2, E, dtype=torch.float64),
              "class_embed.bias": torch.zeros(2, dtype=torch.float64)}
        for j in range(3):
            sd[f"mask_embed.layers.{j}.weight"], sd[f"mask_embed.layers.{j}.bias"] = D[f"m{j}w"], D[f"m{j}b"]
        eye = torch.eye(E, dtype=torch.float64).view(1, E, 16, 16).expand(B, E, 16, 16)
        _, mask, _ = O.prediction_heads(sd, tn.view(B, Q, E).transpose(0, 1), eye, None, 8, want_mask=False)
        torch.testing.assert_close(e, mask.reshape(B * Q, E), rtol=1e-12, atol=1e-12)
        # without the optional pieces
        t0, d0, e0, q0 = C.heads(ar(), xh, None, qpos, P, bias=False, norm=False, l2norm=False, wq=False)
        assert torch.equal(t0, xh.double()) and q0 is None
        torch.testing.assert_close(d0, norm(D["g2"], D["be2"])(xh.double()), rtol=1e-12, atol=1e-12)


def _unique_cpu_cases():
    """One table row per distinct CPU evaluation (tile options and n_parts of post_self do not change the values)."""
    seen = {}
    for c in C.ALL_CASES:
        key = (c.entry, c.prec, c.B, c.Q) + ((c.n_parts, c.wq, "".join(k for k in c.opts if k in "bnl")) if c.entry == "heads" else ())
        seen.setdefault(key, c)
    return list(seen.values())


def _evaluate(c):
    P = C.params()
    if c.entry == "post_cross":
        return C.Arith("f64", C.Form(c.prec)), C.post_cross, (*C.inputs(c.B, c.Q), P), {}
    if c.entry == "post_self":
        o, res, _ = C.inputs(c.B, c.Q)
        return C.Arith("f64", C.Form(c.prec)), C.post_self, (o, res, P), {}
    return C.Arith("f64", C.Form(c.prec)), C.heads, (*C.heads_inputs(c.B, c.Q, c.n_parts), P), C.heads_kw(c)


@pytest.mark.parametrize("case", _unique_cpu_cases(), ids=lambda c: c.id)
def test_yardsticks_agree_with_float64(case):
    """Both fp32 yardsticks (and, for the fp16 form, two of the further evaluation orders) against the float64 definition on the
    same operands, row by row.  A row in which the evaluation rounds every GEMM input to the operand float64 rounds it to must agree
    to fp32 accuracy: ``2 (K + 4) u G M``, a first-order running-error bound of the whole chain, worst case in every factor -- K the
    fp32 operations summed into one output along the chain (the K of every GEMM, E per row reduction), u = 2^-24, G the product of
    the gains of the row phases (max rstd |g|, 1 / min norm), M the largest sum_k |a_k w_k| + |b| of any stage.  A row is allowed
    more only for the inputs it is COUNTED to round the other way (dec_cases.crossings): per such input of GEMM i the form's operand
    rounding f (2^-10 for one fp16 term, 2^-16 for a bf16 pair) of M, carried through the GEMMs behind it at their largest absolute
    row sum.  No row gets a crossing it does not have."""
    a64, chain, args, kw = _evaluate(case)
    ref = chain(a64, *args, **kw)
    form = a64.form
    fp32_tol = 2.0 * (a64.k_path + 4) * C.U32 * a64.gain * a64.mag
    norms = [max(1.0, float(form.w(W).abs().sum(1).max())) for W in a64.weights]
    evals = [C.Arith("linear", form), C.Arith("seq", form)] + ([C.Arith("order", form, j) for j in (1, 2)] if case.prec == "f16" else [])
    for ar in evals:
        got = chain(ar, *args, **kw)
        tol = torch.full((args[0].shape[0],), fp32_tol, dtype=torch.float64)
        for i, cross in enumerate(C.crossings(form, a64, ar)):
            behind = 1.0
            for n in norms[i + 1:]:
                behind *= n
            tol += cross.sum(1).double() * form.flip * a64.gain * a64.mag * behind
        assert case.prec != "f32" or bool((tol == fp32_tol).all())
        for name, g, r in zip("abcd", got, ref):
            if r is None:
                assert g is None
                continue
            assert g.dtype == torch.float32 and r.dtype == torch.float64
            err = (g.double() - r).abs().amax(1)
            worst = int((err / tol).argmax())
            assert bool((err <= tol).all()), f"{case.id} {ar.mode} output {name} row {worst}: {float(err[worst]):.3e} > {float(tol[worst]):.3e}"


def test_crossing_counts_behind_the_further_orders():
    """The counts dec_cases quotes for N_ORDERS, from the yardstick alone: rows of the 200-row fp16 case in which one F.linear
    evaluation rounds a hidden GEMM input to another half than float64 does; and that another order is another sample of them."""
    form, P = C.Form("f16"), C.params()
    o, res, _ = C.inputs(2, 100)
    a64, a32, a33 = C.Arith("f64", form), C.Arith("linear", form), C.Arith("order", form, 1)
    for ar in (a64, a32, a33):
        C.post_self(ar, o, res, P)
    ffn = C.crossings(form, a64, a32)[2].any(1)
    assert not bool(C.crossings(form, a64, a32)[0].any())                 # the exact input o rounds the same way everywhere
    x, parts, qp = C.heads_inputs(2, 100, 8)
    b64, b32 = C.Arith("f64", form), C.Arith("linear", form)
    for ar in (b64, b32):
        C.heads(ar, x, parts, qp, P)
    mlp = torch.stack([c.any(1) for c in C.crossings(form, b64, b32)[:3]]).any(0)
    print(f"rows with a crossing: FFN hidden {float(ffn.float().mean()):.3f}, MLP inputs {float(mlp.float().mean()):.3f}")
    assert round(float(ffn.float().mean()), 2) == 0.73 and round(float(mlp.float().mean()), 2) == 0.29
    other = C.crossings(form, a64, a33)[2]
    assert not torch.equal(other, C.crossings(form, a64, a32)[2]) and 0.4 < float(other.any(1).float().mean()) < 0.95
    # an order is the same function in another order of operations: not F.linear's bits
    y32, y33 = C.post_self(C.Arith("linear", form), o, res, P)[1], C.post_self(C.Arith("order", form, 1), o, res, P)[1]
    assert not torch.equal(y32, y33)
    assert len(C.evaluate_orders(C.post_self, "f16", o[:3], res[:3], P)) == C.N_ORDERS
    assert len(C.evaluate(C.post_self, "f16", o[:3], res[:3], P)[1]) == 2


def test_sequential_chain_is_the_larger_error_at_2048_terms():
    """Why the yardstick includes the strictly sequential chain: over the FFN's 2048-term sums it is several times F.linear."""
    o, res, _ = C.inputs(2, 100)
    P = C.params()
    ref, (lin, seq) = C.evaluate(C.post_self, "f32", o, res, P)
    e_lin, e_seq = (float((y[1].double() - ref[1]).abs().max()) for y in (lin, seq))
    print(f"FFN sum, 200 rows: F.linear {e_lin:.3e}, sequential {e_seq:.3e}, ratio {e_seq / e_lin:.2f}")
    assert e_seq > 1.5 * e_lin


def test_forms_round_as_documented():
    t = C.rnd(64, 256, seed=7) * 3
    t[0, 0], t[0, 1] = 1e6, -1e6
    f16 = C.Form("f16").a(t)
    assert float(f16[0, 0]) == 65504.0 and float(f16[0, 1]) == -65504.0
    assert torch.equal(f16[1:], t[1:].to(torch.float16).float())
    for p in ("bf16", "bf16x2"):
        a = C.Form(p).a(t)
        assert float(((a - t).abs() / t.abs()).max()) <= 2.0 ** -16
        assert torch.equal(C.Form(p).a(t.double()), a.double())
    w = C.params()["w1"]
    assert torch.equal(C.Form("bf16").w(w), w.to(torch.bfloat16).float())
    hi = w.to(torch.bfloat16).float()
    assert torch.equal(C.Form("bf16x2").w(w), hi + (w - hi).to(torch.bfloat16).float())
    assert torch.equal(C.Form("bf16x2").w_seq(w), torch.cat([hi, (w - hi).to(torch.bfloat16).float()], 1))
    assert C.Form("f32").w(w) is w and C.Form("f32").a(t) is t


def test_fragment_orders_are_the_headers_formulas():
    """The index formulas of include/msm_hip.h, element by element, on a (32, 128) matrix."""
    N, K = 32, 128
    w = C.rnd(N, K, seed=9)
    kct = K // 64
    want32 = torch.empty(N * K)
    want16 = torch.empty(N * K)
    for t, kc, lq, lj, c in itertools.product(range(N // 16), range(kct), range(4), range(16), range(4)):
        for u in range(4):
            want32[((t * kct + kc) * 4 + u) * 256 + (lq * 16 + lj) * 4 + c] = w[t * 16 + lj, kc * 64 + u * 16 + lq * 4 + c]
        for up, h in itertools.product(range(2), range(2)):
            want16[(((t * kct + kc) * 2 + up) * 64 + lq * 16 + lj) * 8 + h * 4 + c] = w[t * 16 + lj, kc * 64 + (2 * up + h) * 16 + lq * 4 + c]
    assert torch.equal(C.frag_f32(w).reshape(-1), want32)
    for dt in (torch.bfloat16, torch.float16):
        assert torch.equal(C.frag_16(w, dt).reshape(-1), want16.to(dt))
    hi = w.to(torch.bfloat16)
    lo16 = C.frag_16(w - hi.float(), torch.bfloat16).view(N // 16, kct * 1024)
    hi16 = C.frag_16(hi.float(), torch.bfloat16).view(N // 16, kct * 1024)
    assert torch.equal(C.frag_bf16x2(w), torch.cat([hi16, lo16], 1).reshape(N, 2 * K))
