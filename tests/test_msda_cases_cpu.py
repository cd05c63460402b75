"""tests/msda_cases.py checked on the CPU: for every case of its tables the derived bound is (a) not too tight -- the oracle
evaluated in float32, in its own operation order (torch's fp32 locations and softmax included), lies inside it in every element,
forward and backward -- and (b) not toothless -- wrong references (the right-column tap index W accepted, the half-pixel shift
dropped, offsets divided by (H, W), a softmax per level; for the backward grad_sampling_loc not scaled by (W, H)) lie outside it in
at least one element of every case where they are expressible and in at least 40 % of elements overall.  Also: the seeded inputs
sit where they are meant to (border band, inside, clearly outside, no all-zero output row, no kink in the backward variant), the
analytic float64 backward agrees with float64 autograd, and the restated host dispatch reaches every MSDA kernel instantiation."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import msda_cases as C  # noqa: E402
from oracle import msm_oracle as O  # noqa: E402

FWD = C.FWD_CASES + C.CPU_ONLY_CASES
ids = lambda cases: [c.name for c in cases]


def _loc64(case):
    inp = C.inputs(case)
    return C.loc64(inp.ref64, inp.off, case.levels) if case.form == "enc" else inp.loc.double()


def _wrong(case):
    out = {}
    for which in C.WRONG:
        bad = C.wrong_forward(case, which)
        if bad is not None:
            out[which] = bad
    return out


@pytest.mark.parametrize("case", FWD, ids=ids(FWD))
def test_forward_fp32_oracle_inside_and_wrong_references_outside(case):
    inp = C.inputs(case)
    ref, tol = C.forward_ref(case)
    assert ref.dtype == tol.dtype == torch.float64 and bool((tol >= 0).all()) and bool(torch.isfinite(tol).all())
    o32 = O.ms_deform_attn_core(inp.value, case.levels, inp.loc, inp.aw)
    assert o32.dtype == torch.float32
    n = C.outside(o32, ref, tol)
    print(f"{case.name}: the fp32 oracle uses {C.ratio(o32, ref, tol):.3f} of the bound, median bound {float(tol.median()):.2e}")
    assert n == 0, f"{case.name}: the fp32 oracle leaves the bound in {n} of {ref.numel()} elements"
    assert float(tol.median()) < 1e-4, "a bound this wide would say little in fp32"
    # the restated op of the wrong references is the oracle when nothing is wrong
    assert torch.equal(C.core_variant(inp.value.double(), case.levels, _loc64(case), inp.aw.double()),
                       O.ms_deform_attn_core(inp.value.double(), case.levels, _loc64(case), inp.aw.double()))
    wrong = _wrong(case)
    assert {"right_column", "no_half_pixel"} <= set(wrong)
    assert ("swapped_sizes" in wrong) == (case.form == "enc" and any(h != w for h, w in case.levels))
    assert ("softmax_per_level" in wrong) == (case.form == "enc" and len(case.levels) > 1)
    for kind, bad in wrong.items():
        assert C.outside(bad, ref, tol) >= 1, f"{case.name}: the reference with {kind} passes the bound"


def test_wrong_references_outside_in_40_percent_overall():
    miss, total = {}, {}
    for case in FWD:
        ref, tol = C.forward_ref(case)
        for kind, bad in _wrong(case).items():
            miss[kind] = miss.get(kind, 0) + C.outside(bad, ref, tol)
            total[kind] = total.get(kind, 0) + ref.numel()
    assert set(miss) == set(C.WRONG)
    for kind in miss:
        print(f"{kind}: outside the bound in {miss[kind]} of {total[kind]} elements")
        assert miss[kind] >= 0.4 * total[kind]


@pytest.mark.parametrize("case", FWD, ids=ids(FWD))
def test_forward_inputs_cover_the_borders(case):
    cov = C.coverage(_loc64(case), case.levels)
    ref, _ = C.forward_ref(case)
    print(f"{case.name}: inside {cov['inside']:.3f}, border band {cov['band']:.3f}, clearly outside {cov['outside']:.3f}")
    assert cov["band"] >= 0.25 and cov["inside"] >= 0.30 and cov["outside"] >= 0.05, cov
    live = float((ref.abs().amax(-1) > 0).double().mean())
    if case.M * len(case.levels) * case.P >= 12:
        assert live == 1.0, "an all-zero output row checks nothing"
    else:       # 1 to 4 sampling points per query, 40 to 60 % of them outside by design: a share of the rows has to be zero
        assert live >= 0.30, live


@pytest.mark.parametrize("case", C.BWD_CASES, ids=ids(C.BWD_CASES))
def test_backward_fp32_oracle_inside_and_unscaled_grad_loc_outside(case):
    b = C.bwd_inputs(case)
    assert C.kink_distance(b.loc.double(), case.levels) >= C.KINK
    cov = C.coverage(b.loc.double(), case.levels)
    assert cov["band"] >= 0.25 and cov["inside"] >= 0.30 and cov["outside"] >= 0.05, cov
    refs, tols = C.backward_ref(case)
    # the analytic backward in float64 IS the autograd of the oracle
    ana = O.ms_deform_attn_core_backward(b.value.double(), case.levels, b.loc.double(), b.aw.double(), b.go.double())
    for name, a, r in zip(("grad_value", "grad_sampling_loc", "grad_attn_weight"), ana, refs):
        assert torch.allclose(a, r, rtol=1e-12, atol=1e-13), (name, float((a - r).abs().max()))
    g32 = O.ms_deform_attn_core_backward(b.value, case.levels, b.loc, b.aw, b.go)
    for name, g, r, t in zip(("grad_value", "grad_sampling_loc", "grad_attn_weight"), g32, refs, tols):
        assert g.dtype == torch.float32 and bool((t >= 0).all()) and bool(torch.isfinite(t).all())
        n = C.outside(g, r, t)
        print(f"{case.name} {name}: the fp32 oracle uses {C.ratio(g, r, t):.3f} of the bound")
        assert n == 0, f"{case.name} {name}: the fp32 oracle leaves the bound in {n} of {r.numel()} elements"
    assert bool((refs[1] != 0).any()) and bool((refs[0] != 0).any())
    unscaled = refs[1] / C.sizes(case.levels).double()[:, None, :]
    n = C.outside(unscaled, refs[1], tols[1])
    assert n >= 1, f"{case.name}: grad_sampling_loc without the (W, H) scale passes the bound"


def test_unscaled_grad_loc_outside_in_40_percent_overall():
    """(of the elements the mistake changes: where both sizes of a level are 1, or the gradient is zero, it changes nothing)"""
    miss = total = 0
    for case in C.BWD_CASES:
        refs, tols = C.backward_ref(case)
        unscaled = refs[1] / C.sizes(case.levels).double()[:, None, :]
        miss += C.outside(unscaled, refs[1], tols[1])
        total += int((unscaled != refs[1]).sum())
    print(f"unscaled grad_sampling_loc: outside the bound in {miss} of the {total} elements it changes")
    assert miss >= 0.4 * total


def test_fused_projection_reproduces_structured_offsets():
    """The selection projection of the fused entry points: exact in fp32, every head its own combination, and the projected
    locations keep the border coverage."""
    for case in C.PIXDEC_CASES:
        f = C.fused_inputs(case)
        x = f.src + f.pos
        assert torch.equal(torch.nn.functional.linear(x, f.wp, f.bp), f.proj)
        assert bool(((f.wp == 1).sum(1) == 1).all()) and int((f.wp != 0).sum()) == 288
        off, logits = C.split_proj(f.proj, 8, 3, 4)
        assert all(not torch.equal(off[:, :, 0], off[:, :, m]) for m in range(1, 8))
        _, r64 = C.encoder_ref(case.levels)
        cov = C.coverage(C.loc64(r64[None], off, case.levels), case.levels)
        assert cov["band"] >= 0.25 and cov["inside"] >= 0.30 and cov["outside"] >= 0.05, (case.name, cov)
        inp = C.inputs(case)
        ref, tol = C.encoder_ref_from_proj(inp.value, case.levels, f.proj, 8, 4)
        assert bool((ref.abs().amax(-1) > 0).all())
        o32 = O.ms_deform_attn_core(inp.value, case.levels, (C.encoder_ref(case.levels)[0][None, :, None, None, None, :]
                                    + off / C.sizes(case.levels)[None, None, None, :, None, :]), torch.softmax(logits, -1).view(case.B, case.Lq, 8, 3, 4))
        assert C.outside(o32, ref, tol) == 0


def test_outside_counts_non_finite_values():
    ref, tol = torch.zeros(3, dtype=torch.float64), torch.ones(3, dtype=torch.float64)
    assert C.outside(torch.tensor([0.5, float("nan"), float("inf")]), ref, tol) == 2
    assert C.outside(torch.tensor([1.0, -1.0, 1.5]), ref, tol) == 1


def test_tables_reach_every_instantiation():
    """Every kernel of csrc/msda.hip, csrc/msda_generic.hip and the gathers of csrc/enc_lp.hip is launched by at least one
    (case, entry point, option) of the tables; the head-major entry point rejects D = 6."""
    count = C.table_instantiations()
    assert set(count) == set(C.ALL_INSTANTIATIONS), sorted(set(C.ALL_INSTANTIATIONS) ^ set(count))
    assert len(count) == 21
    for key in C.ALL_INSTANTIATIONS:
        print(f"{key}: {count[key]} runs")
    r = C.HM_REJECT
    assert C.instantiation("hm", r.D, len(r.levels), r.P, C.AUTO, r.M) is None
    assert C.instantiation("tm", r.D, len(r.levels), r.P, C.AUTO, r.M) == "msda_kernel<true,1>"
    assert C.instantiation("fused", 8, 2, 6, C.AUTO, 8) is None and C.instantiation("lp", 8, 4, 3, C.AUTO, 8) is None
    # the issue's list, by entry point
    assert C.instantiation("hm", 8, 3, 4, 3) == "msda_enc_hm8_kernel<false,0,0>"
    assert C.instantiation("hm", 8, 2, 2, C.AUTO) == C.instantiation("hm", 8, 2, 2, 2) == "msda_enc_hm8_kernel<true,0,0>"
    assert C.instantiation("hm", 8, 3, 4, 1) == C.instantiation("hm", 8, 5, 4, C.AUTO) == C.instantiation("hm", 16, 3, 4, 3) == "msda_enc_hm_kernel<4>"
    assert C.instantiation("hm", 2, 3, 4, 2) == "msda_enc_hm_kernel<1>"
    assert C.instantiation("bwd", 64, 3, 2) == "msda_bwd_kernel<4,true>" and C.instantiation("bwd", 24, 2, 2) == "msda_bwd_kernel<4,false>"
    assert C.instantiation("bwd", 2, 3, 2) == "msda_bwd_kernel<1,true>" and C.instantiation("bwd", 6, 2, 2) == "msda_bwd_kernel<1,false>"
    assert C.instantiation("bwd", 8, 9, 2) == C.instantiation("bwd", 71, 3, 2) == "msda_any_bwd_kernel<float>"
