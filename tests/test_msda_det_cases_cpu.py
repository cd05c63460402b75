"""tests/msda_det_cases.py checked on the CPU, and what of the deterministic MSDeformAttn backward needs no GPU.

The integer model of the definition (per-destination (mx, cnt), e, rne(x * 2^e), exact integer sum, one rounding back) meets
msda_cases.bwd_bound on every element of every case, and is bit-identical under a permutation of the queries and of the points
within each level.  Two wrong models leave the bound: one scale per tensor (elements fed only by tiny softmax weights fall under its
quantum) and e without the headroom for cnt (the 504 adders of the pile-up case overflow int64).  The fp32 oracle stays inside the
bound on the new cases (its share of the bound is printed), so the inputs are meetable by the reference alone.  Also: the two new
symbols and ABI 40, and the flag plumbing of ops.ms_deform_attn_backward up to the point where a GPU is needed."""
import os
import sys
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import msda_cases as C  # noqa: E402
import msda_det_cases as K  # noqa: E402
from oracle import msm_oracle as O  # noqa: E402

ALL = K.SUPPORTED_OLD_CASES + K.NEW_CASES


@pytest.mark.parametrize("case", ALL, ids=K.ids(ALL))
def test_integer_model_meets_the_bound_and_has_no_order(case):
    b = K.bwd_inputs(case)
    (ref, _, _), (tol, _, _) = K.backward_ref(case)
    m = K.model(case, b)
    assert float(m.abs_sums.max()) < 2.0 ** 61, "the headroom rule keeps every sum of magnitudes below 2^61"
    n = C.outside(m.grad_value, ref, tol)
    print(f"{case.name}: the integer model uses {C.ratio(m.grad_value, ref, tol):.4f} of the bound, largest cnt {int(m.cnt.max())}")
    assert n == 0, f"{case.name}: the integer model leaves the bound in {n} of {ref.numel()} elements"
    for queries, points in ((True, False), (False, True), (True, True)):
        pm = K.model(case, K.permuted(case, queries, points).inputs)
        assert torch.equal(pm.grad_value, m.grad_value) and torch.equal(pm.sums, m.sums), (case.name, queries, points)
        assert torch.equal(pm.mx, m.mx) and torch.equal(pm.cnt, m.cnt)


def test_pile_up_case_piles_up():
    case = K.PILE_CASE
    m = K.model(case)
    S = case.Lq
    cnt = m.cnt.view(K.B, S, K.M)
    hit = cnt > 0
    W0 = case.levels[0][1]
    pixels = sorted((K.PILE_CELL[0] + dy) * W0 + K.PILE_CELL[1] + dx for dy in (0, 1) for dx in (0, 1))
    assert sorted(set(hit.nonzero()[:, 1].tolist())) == pixels
    assert bool((cnt[:, pixels] == K.PILE_ADDERS).all()) and K.PILE_ADDERS == 504
    # the int64 sums are the sums of Python integers
    d = int(m.cnt.argmax())
    rows = m.q[m.dest == d]
    assert rows.shape[0] == 504
    for c in range(case.D):
        assert sum(int(v) for v in rows[:, c].tolist()) == int(m.sums[d, c])


def test_permutations_are_inverted_by_unpermute():
    case = K.SPREAD_CASE
    b, perm = K.bwd_inputs(case), K.permuted(case)
    assert not torch.equal(perm.inputs.loc, b.loc)
    assert torch.equal(K.unpermute(perm.inputs.loc, perm), b.loc) and torch.equal(K.unpermute(perm.inputs.aw, perm), b.aw)
    assert torch.equal(perm.inputs.go[:, perm.qinv], b.go)


def test_wrong_models_leave_the_bound():
    spread_like = (K.SPREAD_CASE,) + K.ENC_FORM_CASES          # the spread case and the cases whose logits reach +-60
    missed = {"tensor": 0, "headroom": 0}
    for case in spread_like:
        (ref, _, _), (tol, _, _) = K.backward_ref(case)
        missed["tensor"] += C.outside(K.model(case, scale="tensor").grad_value, ref, tol)
    print(f"one scale per tensor: outside the bound in {missed['tensor']} elements of the spread / +-60 cases")
    assert C.outside(K.model(K.SPREAD_CASE, scale="tensor").grad_value, *[t[0] for t in K.backward_ref(K.SPREAD_CASE)]) >= 1
    # e without the headroom for cnt: the pile-up's 504 same-sign adders of up to 2^61 each overflow int64
    case = K.PILE_CASE
    (ref, _, _), (tol, _, _) = K.backward_ref(case)
    bad = K.model(case, headroom=False)
    missed["headroom"] = C.outside(bad.grad_value, ref, tol)
    print(f"no cnt headroom: largest sum of magnitudes 2^{float(torch.log2(bad.abs_sums.max())):.2f}, outside the bound in "
          f"{missed['headroom']} elements of the pile-up case")
    assert float(bad.abs_sums.max()) >= 2.0 ** 63 and missed["headroom"] >= 1


@pytest.mark.parametrize("case", K.NEW_CASES, ids=K.ids(K.NEW_CASES))
def test_fp32_oracle_inside_the_bound_on_the_new_cases(case):
    b = K.bwd_inputs(case)
    assert C.kink_distance(b.loc.double(), case.levels) >= C.KINK
    refs, tols = K.backward_ref(case)
    g32 = O.ms_deform_attn_core_backward(b.value, case.levels, b.loc, b.aw, b.go)
    for name, g, r, t in zip(("grad_value", "grad_sampling_loc", "grad_attn_weight"), g32, refs, tols):
        assert g.dtype == torch.float32 and bool((t >= 0).all()) and bool(torch.isfinite(t).all())
        n = C.outside(g, r, t)
        print(f"{case.name} {name}: the fp32 oracle uses {C.ratio(g, r, t):.3f} of the bound")
        assert n == 0, f"{case.name} {name}: the fp32 oracle leaves the bound in {n} of {r.numel()} elements"
    assert bool((refs[0] != 0).any()) and bool((refs[1] != 0).any())


def test_case_tables():
    assert [c.D for c in K.ENC_FORM_CASES] == [8, 32, 24, 6, 64] * 2
    assert all(c.Lq == sum(h * w for h, w in c.levels) and c.M == 8 and c.P == 4 and c.B == 2 for c in K.NEW_CASES)
    assert {C.instantiation("bwd", c.D, 3, 4) for c in K.SIX_LANE_CASES} == {"msda_bwd_kernel<4,false>", "msda_bwd_kernel<1,false>"}
    assert [c.D for c in K.SUPPORTED_OLD_CASES] == [8, 64, 24, 2, 6]
    b = K.bwd_inputs(K.SPREAD_CASE)
    ratio = b.go.view(2, 126, 8, 8).abs().amax((0, 1, 2))
    assert float(ratio[2] / ratio[0]) > 2.0 ** 14
    spread = torch.log(b.aw.view(2, 126, 8, 12).clamp_min(1e-45))
    assert float((spread.amax(-1) - spread.amin(-1)).median()) > 40.0


def test_abi_declares_the_deterministic_backward():
    from unseenobjectswithmeanshift_amd import _lib
    assert {"msm_msdeform_attn_bwd_det", "msm_msdeform_attn_bwd_det_workspace"} <= set(_lib.declared_symbols())
    assert _lib.ABI_VERSION >= 40


def test_flag_plumbing_without_a_gpu():
    from unseenobjectswithmeanshift_amd import ops
    was, was_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    shapes, start = C.shapes_start(((2, 2),))
    v64 = torch.zeros(1, 4, 1, 4, dtype=torch.float64)
    loc64, aw64, go64 = torch.zeros(1, 1, 1, 1, 1, 2, dtype=torch.float64), torch.zeros(1, 1, 1, 1, 1, dtype=torch.float64), torch.zeros(1, 1, 4, dtype=torch.float64)
    try:
        torch.use_deterministic_algorithms(False)
        assert ops.msda_backward_deterministic(None) is False and ops.msda_backward_deterministic(True) is True
        with pytest.raises(RuntimeError, match="must be on the GPU"):                      # not the determinism error
            ops.ms_deform_attn_backward(v64, shapes, start, loc64, aw64, go64)
        with pytest.raises(RuntimeError, match="ms_deform_attn_backward does not have a deterministic implementation"):
            ops.ms_deform_attn_backward(v64, shapes, start, loc64, aw64, go64, deterministic=True)
        torch.use_deterministic_algorithms(True)
        assert ops.msda_backward_deterministic(None) is True and ops.msda_backward_deterministic(False) is False
        with pytest.raises(RuntimeError, match="ms_deform_attn_backward does not have a deterministic implementation"):
            ops.ms_deform_attn_backward(v64, shapes, start, loc64, aw64, go64)
        with pytest.raises(RuntimeError, match="must be on the GPU"):                      # deterministic=False overrides the flag
            ops.ms_deform_attn_backward(v64, shapes, start, loc64, aw64, go64, deterministic=False)
        torch.use_deterministic_algorithms(True, warn_only=True)
        assert ops.msda_backward_deterministic(None) is True
        with pytest.warns(UserWarning, match="ms_deform_attn_backward does not have a deterministic implementation"):
            with pytest.raises(RuntimeError, match="must be on the GPU"):                  # warned, then went on to the atomic kernel's checks
                ops.ms_deform_attn_backward(v64, shapes, start, loc64, aw64, go64)
        # float32 inside the range: no warning and no determinism error, with or without the flag
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            with pytest.raises(RuntimeError, match="must be on the GPU"):
                ops.ms_deform_attn_backward(v64.float(), shapes, start, loc64.float(), aw64.float(), go64.float())
    finally:
        torch.use_deterministic_algorithms(was, warn_only=was_warn)
