"""tests/attn_cases.py checked on the CPU: the restated dispatch at the boundaries csrc/attention.hip names, the tables reach every
(form, kernel path, mask mode, row_any) combination, the float64 definition is the oracle's, the input families are decisive (one key or one
mask bit moves the float64 answer by far more than any tolerance), bf16 rounds to nearest even, and every 16-bit yardstick stays inside the
project's bounds."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attn_cases as C  # noqa: E402
from oracle import msm_oracle as O  # noqa: E402


def test_dispatch_restated():
    """The boundaries named in attn_launch, msm_hypersphere_attn_lp_fwd and attn_nsplit."""
    r = lambda S, B=2, Lq=100, form="f32", masked=True, **o: C.route(form, B, Lq, S, 8, masked, o)
    assert r(2048).kernel == "qk" and r(2049).kernel == "big"
    assert (r(128).cfg, r(129).cfg) == (1, 0) and (r(128).mq, r(128).nw) == (1, 8) and (r(129).mq, r(129).nw) == (2, 8)
    assert (r(1024, B=48).cfg, r(1025, B=48).cfg, r(1024, B=47).cfg) == (2, 0, 0) and (r(20, B=48).mq, r(20, B=48).nw) == (4, 4)
    assert r(20, B=48).cfg == 2 and r(20, B=48, ATTN_QKCFG=1).cfg == 1
    assert r(100, ATTN_KERNEL=3).kernel == "big" and r(100, ATTN_KERNEL=3).ns == 1
    assert r(300, ATTN_KERNEL=3).ns == 2 and r(300, ATTN_KERNEL=3, ATTN_TARGET=1).ns == 1
    assert r(4800, B=1).ns == 37 and r(4800, B=8).ns == 8                             # S // 128 and cdiv(512, 64)
    for Lq in (1, 37, 112):
        e = r(1296, B=1, Lq=Lq, ATTN_KERNEL=3)
        assert (e.ns, e.kb_per, e.nkb, e.empty) == (10, 9, 81, (9,))
    assert (r(300, Lq=112).qchunks, r(300, Lq=113).qchunks) == (1, 2) and C.AQCH == 112
    assert (r(300, masked=False).mm, r(300).mm, r(301).mm, r(302).mm, r(303).mm, r(304).mm) == (0, 1, 2, 2, 2, 1)
    # the operand type that really runs: fp32 K/V at S <= 128 stay on the fp32 kernel in the low-precision entry point
    for form, op in (("lp0", "bf16"), ("lp3", "f16")):
        assert (r(128, form=form).operand, r(128, form=form).fallback) == ("f32", True)
        assert (r(129, form=form).operand, r(129, form=form).fallback) == (op, False)
    assert r(100, form="lp1").operand == "bf16" and r(100, form="lp2").operand == "f16" and not r(100, form="lp1").fallback
    assert C.route("lp0", 2, 100, 100, 8, False).fallback and C.route("lp0", 2, 20, 37, 8, True).fallback    # two rows of the older test
    # split ranges of the table's shapes: 9 / 8 and 10 / 9 blocks
    assert [len(sum(s, [])) for s in C.shares(r(272, B=1, ATTN_KERNEL=3), 272)] == [9, 8]
    assert [len(sum(s, [])) for s in C.shares(r(301, B=1, ATTN_KERNEL=3), 301)] == [10, 9]
    d = r(2064, B=1, Lq=37)
    assert (d.kernel, d.ns, d.kb_per, d.empty) == ("big", 16, 9, (15,))
    # the fused form's unit walk
    f = lambda H, W, B=1, Lq=37: (C.route("fkv1", B, Lq, H * W, 8, True), H * W, (H, W))
    assert C.shares(*f(1, 16)) == [[[0], [], [], []]]
    assert C.shares(*f(3, 16)) == [[[0], [1], [2], []]]
    assert C.shares(*f(5, 32))[0][1] == [6, 8, 1] and C.fkv_features(*f(5, 32)) == {"cross"}     # units 3, 4 of strip 0, unit 0 of strip 1
    assert f(17, 16, B=2)[0].ns == 2 and f(27, 48, Lq=113)[0].empty == (9,)
    assert C.workspace_floats(1, 113, 1296, 8) == 2 * 8 * 10 * 112 * 33


def test_tables_reach_every_combination():
    got = {}
    for c in C.FORWARD_CASES:
        key = C.cover_key(c)
        if key is not None:
            got.setdefault(key, []).append(c.id)
    for key in sorted(C.required_cover()):
        assert key in got, f"no table row reaches {key}"
        print(f"COVER {key[0]:4s} {key[1]:5s} mm={key[2]} row_any={key[3]:6s} {len(got[key]):3d} rows, e.g. {got[key][0]}")
    fk = {}
    for c in C.FKV_CASES:
        for key in C.fkv_cover(c):
            fk.setdefault(key, []).append(c.id)
    for key in sorted(C.required_fkv_cover()):
        assert key in fk, f"no table row reaches {key}"
        print(f"COVER {key[0]:4s} masked={key[1]!s:5s} {key[2]:6s} {len(fk[key]):3d} rows, e.g. {fk[key][0]}")
    bw = set().union(*(C.bwd_cover(c) for c in C.BWD_CASES))
    for key in sorted(C.required_bwd_cover(), key=repr):
        assert key in bw, f"no table row reaches {key}"
        print(f"COVER bwd  {key[0]}={key[1]}")
    fall = [c.id for c in C.FORWARD_CASES if C.case_route(c).fallback]
    print(f"lp0 / lp3 rows that run the fp32 kernel (S <= 128, labelled, judged as f32): {len(fall)}, e.g. {fall[0]}")
    assert fall and all(c.form in ("lp0", "lp3") and c.S <= 128 for c in C.FORWARD_CASES if C.case_route(c).fallback)
    assert len({c.id for c in C.ALL_CASES}) == len(C.ALL_CASES)


def test_tables_hold_the_named_edges():
    qk = [c for c in C.FORWARD_CASES if C.case_route(c).kernel == "qk"]
    big = [c for c in C.FORWARD_CASES if C.case_route(c).kernel == "big"]
    for form in C.FWD_FORMS:
        for cfg in (0, 1, 2):
            rows = [c for c in qk if c.form == form and dict(c.opts).get("ATTN_QKCFG") == cfg]
            assert {c.S for c in rows} == set(C.QK_S) and {c.Lq for c in rows} == set(C.QK_LQ)
        assert any(c.form == form and c.B == 48 and not c.opts and C.case_route(c).cfg == 2 for c in qk)
        assert any(c.form == form and c.heads == 3 for c in qk) and any(c.form == form and c.heads == 3 for c in big)
        mine = [c for c in big if c.form == form]
        assert {16, 48, 272, 300, 301, 1296, 2064} <= {c.S for c in mine} and {37, 111, 112, 113} <= {c.Lq for c in mine}
        assert any(c.S == 2064 and not c.opts for c in mine)
        assert {C.case_route(c).ns for c in mine if c.S in (300, 301)} == {1, 2}
    assert {(c.hw, c.Lq) for c in C.FKV_CASES if c.heads == 8} == {((1, 16), 37), ((3, 16), 112), ((5, 32), 113), ((17, 16), 37), ((27, 48), 113)}
    assert sum(c.B == 2 for c in C.FKV_CASES if c.fam == "U" and c.form == "fkv1") == 2
    assert {(c.B, c.Lq, c.S) for c in C.BWD_CASES if c.heads == 8} == set(C.BWD_SHAPES)
    assert {c.kappa for c in C.FORWARD_CASES if c.form == "f32"} == {1.0, 30.0} == {c.kappa for c in C.BWD_CASES}
    assert max(c.S for c in C.ALL_CASES) == 2064 and max(c.Lq for c in C.ALL_CASES) == 113
    kernels = lambda cases: {(C.case_route(c).kernel, C.case_route(c).ns > 1) for c in cases}
    assert kernels(C.SENTINEL_CASES) == {("qk", False), ("big", False), ("big", True), ("fkv", True), ("bwd", False)}
    assert kernels(C.STRIDED_CASES) >= {("qk", False), ("big", False), ("big", True), ("fkv", True), ("bwd", False)}


def test_float64_definition_is_the_oracles():
    for c in (C._case("f32", "C", 2, 33, 129, ra="given"), C._case("f32", "Zr", 1, 17, 37), C._case("f32", "Z0", 2, 5, 7),
              C._case("f32", "U", 1, 33, 301, heads=3), C._case("f32", "C", 2, 9, 20, kappa=1.0, ra="none")):
        x = C.inputs(c)
        B, H = c.B, c.heads
        hd = lambda t: C.split_heads(t.double(), H).reshape(B * H, -1, 32)
        add = None
        if x.mask is not None:
            eff = C.effective_mask(x.mask, x.row_any)
            add = torch.zeros(B, 1, c.Lq, c.S, dtype=torch.float64).masked_fill(eff[:, None], float("-inf")).expand(B, H, c.Lq, c.S).reshape(B * H, c.Lq, c.S)
        o, _ = O.hypersphere_attention(hd(x.q), hd(x.k), hd(x.v), add, kappa=c.kappa)
        ref = C.merge_heads(o.view(B, H, c.Lq, 32))
        torch.testing.assert_close(C.definition(x.q, x.k, x.v, H, x.mask, x.row_any, c.kappa), ref, rtol=1e-12, atol=1e-12)
    # mask bytes other than 0 / 1 are in the tables, and they all mean "masked"
    m = C.inputs(C._case("f32", "U", 2, 33, 129)).mask
    assert set(m.unique().tolist()) == {0, *C.MASK_BYTES}


def test_bf16_rounds_to_nearest_even():
    """pack4 (csrc/bf16.h) states round to nearest even; the references round V with torch's conversion: the same function, ties included."""
    g = torch.Generator().manual_seed(1)
    t = torch.randn(1 << 16, generator=g) * 3
    ties = torch.tensor([1.00390625, 1.01171875, -1.00390625, 3.0078125, 0.0, 2.0 ** -20, 65280.0])      # 1 + 2^-8: tie -> even (1.0); 1 + 3 * 2^-8 -> 1 + 2^-6
    t = torch.cat([t, ties])
    assert torch.equal(C.bf16(t), C.bf16_rne_bits(t))
    assert C.bf16(ties)[:4].tolist() == [1.0, 1.015625, -1.0, 3.0]
    assert torch.equal(C.bf16(t.double()), C.bf16(t).double())


def _unique(cases, fams):
    """One case per distinct input set (attn_cases.inputs is cached: forms and options that share a geometry share the tensors)."""
    seen = {}
    for c in cases:
        if c.fam in fams:
            seen.setdefault(id(C.inputs(c)), c)
    return list(seen.values())


U_UNIQUE = _unique(C.FORWARD_CASES + C.FKV_CASES, ("U", "Zu"))
D_UNIQUE = _unique(C.FORWARD_CASES + C.FKV_CASES, ("D",))
TOL_MAX = C.F32_ATOL + C.F32_RTOL                      # the largest tolerance of an element of a unit vector


def test_uniform_family_is_the_closed_form_and_decisive():
    """Family U: the float64 definition IS normalize(mean of the unmasked V rows), at kappa 30 and 1 and for any q; and in every row unmasking
    one more key next to an unmasked one, or masking one unmasked key (n > 1), moves the float64 output by at least 100 tolerances."""
    worst = float("inf")
    for c in U_UNIQUE:
        x = C.inputs(c)
        k, v = C.stored(c.form, x.k, x.v)
        closed = C.uniform_closed_form(v, c.heads, x.mask, x.row_any)
        for kappa in (30.0, 1.0):
            torch.testing.assert_close(C.definition(x.q, k, v, c.heads, x.mask, x.row_any, kappa), closed, rtol=1e-12, atol=1e-12)
        assert all(len(set(ks)) == len(ks) for ks in x.keep)
        assert (x.mask == 0).sum(-1).flatten().tolist() == [len(ks) for ks in x.keep]
        if c.fam == "U" and c.B * c.Lq >= 33:
            assert {n for ks in x.keep for n in [len(ks)]} >= {min(n, c.S) for n in C.U_COUNTS}
            used = {kk for ks in x.keep for kk in ks}
            edges = C.edge_keys(C.case_route(c), c.S, c.hw)
            missing = [e for e in edges if e not in used]
            assert len(missing) <= len(edges) // 4 or c.B * c.Lq < 100, (c.id, missing)
        if c.fam != "U":
            continue                                                                 # (Zu holds a zero v row: unmasking it moves nothing, by construction)
        vh = C.split_heads(v.double(), c.heads)                                      # (B, H, S, 32)
        oh = C.split_heads(closed, c.heads)                                          # (B, H, Lq, 32)
        for r, ks in enumerate(x.keep):
            b, i = divmod(r, c.Lq)
            tot = vh[b][:, ks].sum(1)
            trials = []
            nb = next((kk + dlt for kk in ks for dlt in (1, -1) if 0 <= kk + dlt < c.S and kk + dlt not in ks), None)
            if nb is not None:
                trials.append((tot + vh[b][:, nb]) / (len(ks) + 1))
            if len(ks) > 1:
                trials.append((tot - vh[b][:, ks[r % len(ks)]]) / (len(ks) - 1))
            for o in trials:
                move = float((C.unit(o) - oh[b][:, i]).abs().amax(-1).min())          # the least moved head
                worst = min(worst, move)
                assert move >= 100 * TOL_MAX, (c.id, r, move)
    print(f"family U: {len(U_UNIQUE)} input sets, least move of a head's output by one key {worst:.3f} (tolerance {TOL_MAX:.1e})")


def test_dominant_family_margin():
    """Family D: with the one masked key unmasked the row is normalize(v_j): ten times the loosest bound away, in every row."""
    worst = float("inf")
    for c in D_UNIQUE:
        x = C.inputs(c)
        k, v = C.stored(c.form, x.k, x.v)
        a = C.definition(x.q, k, v, c.heads, x.mask, x.row_any)
        b = C.definition(x.q, k, v, c.heads, None, None)
        assert int((x.mask != 0).sum()) == c.B * c.Lq and bool(((x.mask != 0).sum(-1) == 1).all())
        margin = float((a - b).abs().amax(-1).min())
        worst = min(worst, margin)
        assert margin >= 10 * C.LP_BOUND["bf16"][0], (c.id, margin)
    print(f"family D: {len(D_UNIQUE)} input sets, least margin of a row {worst:.3f}")


def test_coherent_and_degenerate_families_are_what_they_say():
    c = C._case("f32", "C", 2, 113, 300, opts=C.K3, ra="given")
    x, r = C.inputs(c), C.case_route(c)
    m = x.mask != 0
    assert x.row_any[:, 1].tolist() == [0, 0] and bool(m[:, 1].all()) and bool(m[:, c.Lq - 1].all()) and int((x.row_any == 0).sum()) == 4
    assert bool((~m).all(-1).any())                                                  # a fully unmasked row
    blocks = m.view(c.B, c.Lq, -1)[..., :288].reshape(c.B, c.Lq, 18, 16)
    assert bool((blocks.all(-1) | ~blocks.any(-1)).all())                            # whole 16-key blocks only
    split0 = sorted(kb for w in C.shares(r, c.S)[0] for kb in w)
    assert any(bool(m[0, i, :16 * len(split0)].all()) and not bool(m[0, i, 16 * len(split0):].any()) for i in range(c.Lq))
    n = C.inputs(c._replace(ra="none"))
    assert n.row_any is None and not bool((n.mask != 0).all(-1).any())
    f = C.inputs(C._case("fkv1", "C", 1, 113, 160, hw=(5, 32), ra="given"))
    rect = lambda R: 0 < int(R.sum()) < R.numel() and torch.equal(R, R.any(1)[:, None] & R.any(0)[None]) and int(R.any(1).sum()) > 1
    assert any(rect(row.view(5, 32)) for row in (f.mask[0] != 0))                    # a rectangle in (y, x)
    z = C.inputs(C._case("f32", "Zr", 2, 33, 129))
    assert not z.q[:, 0].any() and bool((z.k.abs().sum(-1) == 0).any()) and bool((z.v.abs().sum(-1) == 0).any())
    ref = C.definition(z.q, z.k, z.v, 8, z.mask, z.row_any)
    torch.testing.assert_close(ref[:, 0], C.uniform_closed_form(z.v, 8, z.mask, z.row_any)[:, 0], rtol=1e-12, atol=1e-12)   # a zero q row: uniform weights
    assert bool(torch.isfinite(ref).all())


def test_fused_uniform_family_rounds_v_one_way():
    """Family U of the fused form: every fp32 sum behind V is exact, so the CPU yardstick (fp32 F.linear) and float64 round V to the same
    bf16 value in every element -- the one-ulp allowance of an element that rounds the other way is used by no element."""
    for c in (c for c in C.FKV_CASES if c.fam in ("U", "Zu") and c.form == "fkv1"):
        x = C.inputs(c)
        k64, v64 = C.fkv_kv(x.fkv, c.hw)
        flips = int((C.bf16(C.fkv_v_yardstick(x.fkv, c.hw)) != C.bf16(v64.float())).sum())
        print(f"{c.id}: V elements the yardstick rounds the other way: {flips} of {v64.numel()}")
        assert flips == 0 and torch.equal(v64.float().double(), v64) and torch.equal(k64.float().double(), k64)
        kh = C.split_heads(k64, c.heads)
        assert float((C.unit(kh) - C.unit(kh)[:, :, :1]).abs().max()) < 1e-15         # one direction per head
        assert float(kh.norm(dim=-1).max() / kh.norm(dim=-1).min()) > 100.0


LP_UNIQUE = {}
for _c in C.FORWARD_CASES + C.FKV_CASES:
    if not C.exact(_c):
        LP_UNIQUE.setdefault((id(C.inputs(_c)), _c.form, _c.kappa), _c)
LP_UNIQUE = list(LP_UNIQUE.values())


def test_yardsticks_stay_inside_the_project_bounds():
    """The CPU yardstick of every 16-bit case on families D, C and Z against float64 on the same stored K / V: inside the project's bounds
    (3e-2 / 2e-3; 1.5e-2 / 8e-4 with fp16 scores).  Twice its maximum is what the GPU may show."""
    worst = {}
    for c in LP_UNIQUE:
        op = C.case_route(c).operand
        emax, emean = C.yard_error(c)
        pmax, pmean = C.LP_BOUND[op]
        print(f"YARD {c.id:48s} {op:4s} max {emax:.2e} mean {emean:.2e}")
        assert emax < pmax and emean < pmean, c.id
        w = worst.setdefault(op, [0.0, 0.0])
        w[0], w[1] = max(w[0], emax), max(w[1], emean)
    print("worst yardstick per operand type:", {k: (f"{v[0]:.2e}", f"{v[1]:.2e}") for k, v in worst.items()})


def test_backward_references():
    """Family U with one unmasked key: grad_q and grad_k vanish and grad_v is the closed form; the input scale is finite and positive."""
    for c in (c for c in C.BWD_CASES if c.fam == "U"):
        gout = C.bwd_grad_out(c)
        out, gq, gk, gv = C.bwd_reference(c, gout)
        s_in = C.bwd_input_scale(c, gout, out)
        assert 0 < s_in < float("inf")
        assert float(gq.abs().max()) <= 1e-9 * s_in and float(gk.abs().max()) <= 1e-9 * s_in
        assert C.bwd_scale(c, gq, gout, out) == s_in and C.bwd_scale(c, gv, gout, out) == float(gv.abs().max())
        closed = C.bwd_uniform_grad_v(c, gout)
        torch.testing.assert_close(gv, closed, rtol=1e-10, atol=1e-12)
        chosen = torch.zeros(c.B, c.S, dtype=torch.bool)
        for r, ks in enumerate(C.inputs(c).keep):
            assert len(ks) == 1
            chosen[r // c.Lq, ks[0]] = True
        assert not closed[~chosen].any()
