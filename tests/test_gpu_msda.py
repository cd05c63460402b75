"""Every multi-scale deformable attention kernel (csrc/msda.hip, csrc/msda_generic.hip, the fp16 gathers of csrc/enc_lp.hip) on
the cases of tests/msda_cases.py -- sampling points ON the map borders, one-row / one-column / one-pixel levels, offsets far
outside, equal / widely spread / shifted logits -- against the float64 definition and the derived bound: every element of every
result obeys ``|got - ref| <= tol`` (no rtol / atol, nothing left out; tests/test_msda_cases_cpu.py proves the bound neither too
tight nor toothless).  Every case goes through every entry point and MSDA_GENERIC option that can take it (msda_cases.runs); every
comparison prints ``RATIO <kernel instantiation> <max error / tol>`` (pytest -s): reported, never asserted.

Bitwise identities: the fused gather (sampling projection in the kernel) equals the default owner-record gather on the same projected
values, as DESIGN.md and docs/HISTORY.md claim, and that is asserted with torch.equal.  The ONE exception to "same products, same
order as the owner-record gather" is msda_enc_hm8_kernel<true,3,4>: it is reached only under MSDA_GENERIC = 2, which keeps the IEEE
divisions and expf in its prologue where the default multiplies by reciprocals and uses v_exp_f32, so it (like MSDA_GENERIC = 1 / 3)
only has to meet the bound; whether the bits agree is printed, not asserted.  Also run: msda_pack_proj_kernel (by the fused test) and
value_to_hm_kernel (torch.equal with the permutation, in the head-major test).

The fused entry points get the structured offsets EXACTLY: their projection is a selection matrix (msda_cases.fused_inputs), so
every projected offset / logit is one feature of src + pos whatever the matrix pipe does.  Needs a real MI355X (pytest -m gpu)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import msda_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
HM_CASES = tuple(c for c in C.ENC_CASES if c is not C.HM_REJECT)
ids = lambda cases: [c.name for c in cases]
OPT_IDS = {C.AUTO: "auto"}


def ops():
    from unseenobjectswithmeanshift_amd import ops as _ops
    return _ops


def dev(t):
    return t.to(DEV).contiguous()


def geometry(case):
    shapes, start = C.shapes_start(case.levels)
    return dev(shapes), dev(start)


def inside(kernel, case, got, ref, tol):
    n = C.outside(got, ref, tol)
    print(f"RATIO {kernel} {C.ratio(got, ref, tol):.4f}   [{case.name}]")
    i, err, t = C.worst(got, ref, tol)
    assert n == 0, (f"{kernel} {case.name}: {n} of {ref.numel()} elements outside the bound; worst element {i} "
                    f"(index {tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape))}): error {err:.3e}, bound {t:.3e}")


def rows(out_hm):
    """(B, M, S, D) head-major result -> (B, S, M*D)"""
    B, M, S, D = out_hm.shape
    return out_hm.permute(0, 2, 1, 3).reshape(B, S, M * D)


# =============================================================================================
# decoder form: ops.ms_deform_attn, fp32 and fp64
# =============================================================================================
@pytest.mark.parametrize("case", C.DEC_CASES, ids=ids(C.DEC_CASES))
def test_decoder_form(case):
    inp = C.inputs(case)
    ref, tol = C.forward_ref(case)
    shapes, start = geometry(case)
    L = len(case.levels)
    got = ops().ms_deform_attn(dev(inp.value), shapes, start, dev(inp.loc), dev(inp.aw))
    assert got.shape == (case.B, case.Lq, case.M * case.D) and got.dtype == torch.float32
    inside(C.instantiation("dec", case.D, L, case.P), case, got, ref, tol)
    # float64: the same inputs widened; the same bound with u = 2^-53 on every element, and 1e-12 of the result's scale
    got64 = ops().ms_deform_attn(dev(inp.value.double()), shapes, start, dev(inp.loc.double()), dev(inp.aw.double()))
    assert got64.dtype == torch.float64
    tol64 = C.bound(inp.value, case.levels, inp.loc.double(), inp.aw.double(), u=C.U64)
    inside(C.instantiation("dec64", case.D, L, case.P), case, got64, ref, tol64)
    assert float((got64.cpu() - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


# =============================================================================================
# encoder forms: token-major, head-major under every MSDA_GENERIC
# =============================================================================================
@pytest.mark.parametrize("case", C.ENC_CASES, ids=ids(C.ENC_CASES))
def test_encoder_token_major(case):
    inp = C.inputs(case)
    ref, tol = C.forward_ref(case)
    shapes, start = geometry(case)
    got = ops().ms_deform_attn_encoder(dev(inp.value.view(case.B, case.Lq, case.M * case.D)), shapes, start, dev(inp.proj), case.M, case.P)
    assert got.shape == ref.shape
    inside(C.instantiation("tm", case.D, len(case.levels), case.P), case, got, ref, tol)


@pytest.mark.parametrize("option", C.OPTIONS, ids=lambda o: f"generic_{OPT_IDS.get(o, o)}")
@pytest.mark.parametrize("case", HM_CASES, ids=ids(HM_CASES))
def test_encoder_head_major(case, option, lib_option):
    inp = C.inputs(case)
    ref, tol = C.forward_ref(case)
    shapes, start = geometry(case)
    kernel = C.instantiation("hm", case.D, len(case.levels), case.P, option, case.M)
    assert kernel is not None
    vh = dev(C.head_major(inp.value))
    if case.D % 4 == 0:                         # the library's own layout change (value_to_hm_kernel) moves every pixel where the gather looks
        assert torch.equal(ops().value_to_head_major(dev(inp.value.view(case.B, case.Lq, case.M * case.D)), case.M), vh)
    lib_option("MSDA_GENERIC", option)
    got = ops().ms_deform_attn_encoder(vh, shapes, start, dev(inp.proj), case.M, case.P)
    assert got.shape == ref.shape
    inside(kernel, case, got, ref, tol)


def test_head_major_rejects_six_channels_per_head():
    case = C.HM_REJECT
    inp = C.inputs(case)
    shapes, start = geometry(case)
    assert C.instantiation("hm", case.D, len(case.levels), case.P, C.AUTO, case.M) is None
    with pytest.raises(RuntimeError):
        ops().ms_deform_attn_encoder(dev(C.head_major(inp.value)), shapes, start, dev(inp.proj), case.M, case.P)


# =============================================================================================
# the fused gather: sampling projection in the kernel
# =============================================================================================
@pytest.mark.parametrize("case", C.PIXDEC_CASES, ids=ids(C.PIXDEC_CASES))
def test_encoder_fused(case, lib_option):
    inp, f = C.inputs(case), C.fused_inputs(case)
    ref, tol = C.encoder_ref_from_proj(inp.value, case.levels, f.proj, 8, 4)
    shapes, start = geometry(case)
    vh = dev(C.head_major(inp.value))
    wpack, bpack = ops().pack_msda_proj(dev(f.wp), dev(f.bp), 8, 3, 4)
    got = ops().ms_deform_attn_encoder_fused(vh, shapes, start, dev(f.src), dev(f.pos), wpack, bpack, 4)
    inside(C.instantiation("fused", 8, 3, 4), case, got, ref, tol)
    # the unfused kernels on the same (exactly reproduced) projection
    default = ops().ms_deform_attn_encoder(vh, shapes, start, dev(f.proj), 8, 4)
    inside(C.instantiation("hm", 8, 3, 4), case, default, ref, tol)
    assert torch.equal(got, default), "the fused gather is bitwise the owner-record gather"
    for option in (1, 2, 3):                    # IEEE divisions / expf in the prologue: inside the bound, not bitwise the default
        lib_option("MSDA_GENERIC", option)
        other = ops().ms_deform_attn_encoder(vh, shapes, start, dev(f.proj), 8, 4)
        inside(C.instantiation("hm", 8, 3, 4, option), case, other, ref, tol)
        print(f"MSDA_GENERIC={option} bitwise the default: {torch.equal(other, default)}   [{case.name}]")


# =============================================================================================
# fp16 gathers: stored records and projection in the kernel
# =============================================================================================
@pytest.mark.parametrize("case", C.PIXDEC_CASES, ids=ids(C.PIXDEC_CASES))
def test_encoder_lp(case):
    inp = C.inputs(case)
    shapes, start = geometry(case)
    v16 = C.head_major(inp.value).to(torch.float16)
    value16 = v16.float().permute(0, 2, 1, 3).contiguous()                                 # token-major, fp16-valued
    proj_hm = ops().proj_to_head_major_records(dev(inp.proj))
    proj_r = ops().proj_records_to_columns(proj_hm).cpu()                                  # what the kernel reads: fp32 offsets, fp16-rounded logits
    assert torch.equal(proj_r[..., :192], inp.proj[..., :192])
    assert torch.equal(proj_r[..., 192:], inp.proj[..., 192:].to(torch.float16).float())
    ref, tol = C.encoder_ref_from_proj(value16, case.levels, proj_r, 8, 4)
    got = ops().ms_deform_attn_encoder_lp(dev(v16), shapes, start, proj_hm, 4)
    assert got.shape == (case.B, 8, case.Lq, 8) and got.dtype == torch.float16
    inside(C.instantiation("lp", 8, 3, 4), case, rows(got), ref, C.fp16_result_tol(ref, tol))


@pytest.mark.parametrize("case", C.PIXDEC_CASES, ids=ids(C.PIXDEC_CASES))
def test_encoder_lp_fused(case):
    inp, f = C.inputs(case), C.fused_inputs(case)
    shapes, start = geometry(case)
    v16 = C.head_major(inp.value).to(torch.float16)
    value16 = v16.float().permute(0, 2, 1, 3).contiguous()
    proj64 = torch.nn.functional.linear(f.src.double() + f.pos.double(), f.wp.double(), f.bp.double())
    ref, tol = C.encoder_ref_from_proj(value16, case.levels, proj64, 8, 4, off_rel=2.0 ** -17, logit_rel=2.0 ** -17)
    wpack, bpack = ops().pack_msda_proj_lp(dev(f.wp), dev(f.bp))
    got = ops().ms_deform_attn_encoder_lp_fused(dev(v16), shapes, start, dev(f.src), dev(f.pos), wpack, bpack, 4)
    assert got.shape == (case.B, 8, case.Lq, 8) and got.dtype == torch.float16
    inside(C.instantiation("lp_fused", 8, 3, 4), case, rows(got), ref, C.fp16_result_tol(ref, tol))


# =============================================================================================
# backward
# =============================================================================================
GRADS = ("grad_value", "grad_sampling_loc", "grad_attn_weight")


@pytest.mark.parametrize("case", C.BWD_CASES, ids=ids(C.BWD_CASES))
def test_backward(case):
    b = C.bwd_inputs(case)
    refs, tols = C.backward_ref(case)
    shapes, start = geometry(case)
    L = len(case.levels)
    got = ops().ms_deform_attn_backward(dev(b.value), shapes, start, dev(b.loc), dev(b.aw), dev(b.go))
    for name, g, r, t in zip(GRADS, got, refs, tols):
        assert g.dtype == torch.float32
        inside(f"{C.instantiation('bwd', case.D, L, case.P)} {name}", case, g, r, t)
    got64 = ops().ms_deform_attn_backward(*(dev(t.double()) if t.is_floating_point() else t
                                            for t in (b.value, shapes, start, b.loc, b.aw, b.go)))
    for name, g, r, t in zip(GRADS, got64, refs, C.bwd_bound(case, u=C.U64)):
        assert g.dtype == torch.float64
        inside(f"{C.instantiation('bwd64', case.D, L, case.P)} {name}", case, g, r, t)
        assert float((g.cpu() - r).abs().max()) <= 1e-12 * float(r.abs().max())


def test_backward_through_the_autograd_function():
    from unseenobjectswithmeanshift_amd.training import MSDeformAttnFunction
    case = C.BWD_CASES[0]
    b = C.bwd_inputs(case)
    refs, tols = C.backward_ref(case)
    shapes, start = geometry(case)
    value, loc, aw = (dev(t).requires_grad_(True) for t in (b.value, b.loc, b.aw))
    out = MSDeformAttnFunction.apply(value, shapes, start, loc, aw, 64)
    fref = C.O.ms_deform_attn_core(b.value.double(), case.levels, b.loc.double(), b.aw.double())
    inside("MSDeformAttnFunction forward", case, out, fref, C.bound(b.value, case.levels, b.loc.double(), b.aw.double()))
    out.backward(dev(b.go))
    for name, g, r, t in zip(GRADS, (value.grad, loc.grad, aw.grad), refs, tols):
        inside(f"MSDeformAttnFunction {name}", case, g, r, t)


# =============================================================================================
# the argument checks
# =============================================================================================
def test_rejections():
    case = C.BWD_CASES[0]
    b = C.bwd_inputs(case)
    shapes, start = geometry(case)
    args = (dev(b.value), shapes, start, dev(b.loc), dev(b.aw))
    with pytest.raises(RuntimeError):
        ops().ms_deform_attn_backward(*args, dev(b.go[:, :, :-1]))                        # mismatched grad_output
    with pytest.raises(RuntimeError):
        ops().ms_deform_attn_backward(*args, dev(b.go[:, :-1]))
    with pytest.raises(RuntimeError):
        ops().ms_deform_attn_backward(*args, dev(b.go.double()))
    # the fused entry points take 3 levels x 4 points only
    pd = C.PIXDEC_CASES[0]
    inp, f = C.inputs(pd), C.fused_inputs(pd)
    vh = dev(C.head_major(inp.value))
    wpack, bpack = ops().pack_msda_proj(dev(f.wp), dev(f.bp), 8, 3, 4)
    wpack_lp, bpack_lp = ops().pack_msda_proj_lp(dev(f.wp), dev(f.bp))
    src, pos = dev(f.src), dev(f.pos)
    proj_hm = ops().proj_to_head_major_records(dev(inp.proj))
    two, four = ((5, 7), (7, 2)), ((5, 7), (3, 4), (1, 1), (1, 1))                        # S = 49 each
    for levels, P in ((two, 2), (four, 4), (C.LEVELS_A, 2), (two, 6), (four, 3)):         # L*P = 4, 16, 6; 12 but not 3 x 4
        assert sum(h * w for h, w in levels) == pd.Lq
        sh, st = (dev(t) for t in C.shapes_start(levels))
        L = len(levels)
        assert C.instantiation("fused", 8, L, P) is None and C.instantiation("lp", 8, L, P) is None
        with pytest.raises(RuntimeError):
            ops().ms_deform_attn_encoder_fused(vh, sh, st, src, pos, wpack, bpack, P)
        with pytest.raises(RuntimeError):
            ops().ms_deform_attn_encoder_lp_fused(vh.half(), sh, st, src, pos, wpack_lp, bpack_lp, P)
        with pytest.raises(RuntimeError):
            ops().ms_deform_attn_encoder_lp(vh.half(), sh, st, proj_hm, P)
        if L * P != 12:
            with pytest.raises(RuntimeError):
                ops().pack_msda_proj(dev(torch.zeros(8 * L * P * 3, 64)), dev(torch.zeros(8 * L * P * 3)), 8, L, P)
