"""The deterministic MSDeformAttn backward (csrc/msda_det.hip; ops.ms_deform_attn_backward(..., deterministic=True) and torch's
global flag) on a real MI355X (pytest -m gpu).

Accuracy is msda_cases' float64 definition and derived per-element bound, unchanged, no element left out; every comparison prints
``RATIO <what> <max error / tol>`` (pytest -s): reported, never asserted.  Everything else here is a BIT claim (torch.equal): the
same bits on every call; under a permutation of the queries and of the points within each level; for an image alone and in a
batch; for a workspace of one image and of the whole batch.  No test runs the atomic kernel to look for a difference."""
import functools
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import msda_cases as C  # noqa: E402
import msda_det_cases as K  # noqa: E402
import pd_bwd_cases as PD  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
GRADS = ("grad_value", "grad_sampling_loc", "grad_attn_weight")
ALL = K.SUPPORTED_OLD_CASES + K.NEW_CASES
ORDER_CASES = K.ENC_FORM_CASES[:5] + K.SIX_LANE_CASES[2:] + (K.PILE_CASE, K.SPREAD_CASE)


def ops():
    from unseenobjectswithmeanshift_amd import ops as _ops
    return _ops


def dev(t):
    return t.to(DEV).contiguous()


def geometry(case):
    shapes, start = C.shapes_start(case.levels)
    return dev(shapes), dev(start)


def run(case, b=None, **kw):
    b = b or K.bwd_inputs(case)
    shapes, start = geometry(case)
    kw.setdefault("deterministic", True)
    return ops().ms_deform_attn_backward(dev(b.value), shapes, start, dev(b.loc), dev(b.aw), dev(b.go), **kw)


@functools.lru_cache(maxsize=None)
def result(case):
    """the deterministic backward of a case, computed once and left unchanged"""
    return run(case)


def inside(what, case, got, ref, tol):
    n = C.outside(got, ref, tol)
    print(f"RATIO {what} {C.ratio(got, ref, tol):.4f}   [{case.name}]")
    i, err, t = C.worst(got, ref, tol)
    assert n == 0, (f"{what} {case.name}: {n} of {ref.numel()} elements outside the bound; worst element {i}: error {err:.3e}, bound {t:.3e}")


def accurate(case, got=None):
    refs, tols = K.backward_ref(case)
    for name, g, r, t in zip(GRADS, got or result(case), refs, tols):
        assert g.dtype == torch.float32
        inside(f"msda_det {name}", case, g, r, t)


def equal3(a, b, what):
    for name, x, y in zip(GRADS, a, b):
        assert torch.equal(x, y), f"{what}: {name} differs in {int((x != y).sum())} of {x.numel()} elements"


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL, ids=K.ids(ALL))
def test_accuracy(case):
    accurate(case)


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL, ids=K.ids(ALL))
def test_three_calls_give_the_same_bits(case):
    first = result(case)
    for _ in range(2):
        equal3(run(case), first, f"{case.name}: a repeated call")


# 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ORDER_CASES, ids=K.ids(ORDER_CASES))
def test_order_of_queries_and_points_does_not_matter(case):
    gv, gl, gw = result(case)
    for queries, points in ((True, False), (False, True), (True, True)):
        perm = K.permuted(case, queries, points)
        pv, pl, pw = run(case, perm.inputs)
        what = f"{case.name}: queries permuted {queries}, points permuted {points}"
        assert torch.equal(pv, gv), f"{what}: grad_value differs in {int((pv != gv).sum())} elements"
        equal3((gv, K.unpermute(pl, perm), K.unpermute(pw, perm)), (gv, gl, gw), what)


# 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", (K.ENC_FORM_CASES[0], K.ENC_FORM_CASES[3], K.ENC_FORM_CASES[9], K.SPREAD_CASE),
                         ids=K.ids((K.ENC_FORM_CASES[0], K.ENC_FORM_CASES[3], K.ENC_FORM_CASES[9], K.SPREAD_CASE)))
def test_an_image_alone_equals_its_row_of_the_batch(case):
    b = K.bwd_inputs(case)
    whole = result(case)
    for i in range(case.B):
        alone = run(case, C.BwdInputs(*(t[i:i + 1] for t in b)))
        equal3(alone, tuple(t[i:i + 1] for t in whole), f"{case.name}: image {i} alone")


# 5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", (K.ENC_FORM_CASES[0], K.ENC_FORM_CASES[2]), ids=K.ids((K.ENC_FORM_CASES[0], K.ENC_FORM_CASES[2])))
def test_workspace_size_does_not_matter_and_its_neighbours_stay_untouched(case):
    S = case.Lq
    one = ops().ms_deform_attn_backward_det_workspace(1, S, case.M, case.D)
    assert one == S * case.M * 8 * (case.D + 1) and ops().ms_deform_attn_backward_det_workspace(case.B, S, case.M, case.D) == case.B * one
    whole = result(case)
    equal3(run(case, workspace_images=1), whole, f"{case.name}: a workspace of one image")
    guard = 4096
    for images in (1, case.B):
        buf = torch.full((guard + images * one + guard,), 0xA5, dtype=torch.uint8, device=DEV)
        equal3(run(case, workspace=buf[guard:guard + images * one]), whole, f"{case.name}: the caller's workspace of {images} image(s)")
        assert bool((buf[:guard] == 0xA5).all()) and bool((buf[guard + images * one:] == 0xA5).all()), "a guard band was written"
        assert not bool((buf[guard:guard + images * one] == 0xA5).all())
    # a workspace between one and two images runs image by image and leaves the rest alone
    buf = torch.full((guard + 2 * one - 16 + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    equal3(run(case, workspace=buf[guard:guard + 2 * one - 16]), whole, f"{case.name}: a workspace of one image and a bit")
    assert bool((buf[:guard] == 0xA5).all()) and bool((buf[guard + one:] == 0xA5).all())
    short = torch.empty(one, dtype=torch.uint8, device=DEV)[:one - 1]
    with pytest.raises(RuntimeError, match=r"msm_msdeform_attn_bwd_det: workspace of \d+ bytes is smaller than one image's \d+ bytes"):
        run(case, workspace=short)


@pytest.mark.parametrize("images", (1, 2), ids=("one_image_workspace", "whole_batch_workspace"))
def test_a_captured_graph_replays_the_same_bits(images):
    """nothing in the call allocates or synchronises: it captures into a HIP graph (four kernel nodes per group of images; with a
    one-image workspace the second group re-uses the first one's bytes)"""
    case = K.ENC_FORM_CASES[2]
    b = K.bwd_inputs(case)
    shapes, start = geometry(case)
    args = (dev(b.value), shapes, start, dev(b.loc), dev(b.aw), dev(b.go))
    ws = torch.empty(ops().ms_deform_attn_backward_det_workspace(images, case.Lq, case.M, case.D), dtype=torch.uint8, device=DEV)
    whole = result(case)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        equal3(ops().ms_deform_attn_backward(*args, deterministic=True, workspace=ws), whole, "on a side stream")
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = ops().ms_deform_attn_backward(*args, deterministic=True, workspace=ws)
    for _ in range(2):
        for t in static:
            t.zero_()
        ws.fill_(0xA5)
        graph.replay()
        torch.cuda.synchronize()
        equal3(static, whole, "a replayed graph")


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_spread_and_pile_up_cases_within_the_per_element_bound():
    for case in (K.SPREAD_CASE, K.PILE_CASE):
        accurate(case)
    gv = result(K.PILE_CASE)[0]
    assert int((gv != 0).any(-1).sum()) == 4 * K.M * K.B, "the pile-up case feeds 4 pixels per head and image"


def test_the_kernel_agrees_with_the_integer_model_within_the_bound():
    """(the model and the kernel round the pixel coordinate differently -- a fused multiply-add -- so this is no bit claim; where the
    fp32 contributions agree, the sums do)"""
    for case in (K.PILE_CASE, K.ENC_FORM_CASES[0]):
        m = K.model(case).grad_value
        gv = result(case)[0].cpu()
        (ref, _, _), (tol, _, _) = K.backward_ref(case)
        assert C.outside(gv, m.double(), 2.0 * tol) == 0
        print(f"{case.name}: {float((gv == m).double().mean()):.4f} of the elements equal the integer model's bit for bit")


# 7 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", (float("inf"), float("nan")), ids=("inf", "nan"))
def test_a_non_finite_grad_output_poisons_only_its_own_destinations(bad):
    case = K.ENC_FORM_CASES[0]
    b = K.bwd_inputs(case)
    clean = result(case)[0].cpu()
    img, head = 1, 3

    def touched_by(q):
        """destinations (B, S, M) that receive a contribution of (img, q, head): with unit weights and an indicator grad_output the
        model's bound is a bilinear weight, positive on every in-range corner (the inputs are kink-free)"""
        ind = torch.zeros(case.B, case.Lq, case.M, case.D)
        ind[img, q, head] = 1.0
        return (K.model(case, C.BwdInputs(b.value, b.loc, torch.ones_like(b.aw), ind.reshape(b.go.shape))).mx > 0).view(case.B, case.Lq, case.M)

    q = next(q for q in range(17, case.Lq) if bool(touched_by(q).any()))
    touched = touched_by(q)
    assert 1 <= int(touched.sum()) == int(touched[img, :, head].sum()) < case.Lq
    go = b.go.clone().view(case.B, case.Lq, case.M, case.D)
    go[img, q, head, 5] = bad
    gv = run(case, b._replace(go=go.reshape(b.go.shape)))[0].cpu()
    nonfinite = ~torch.isfinite(gv)
    assert bool(nonfinite.any())
    assert bool((nonfinite.any(-1) <= touched).all()), "a destination the query and head do not touch became non-finite"
    assert torch.equal(nonfinite.all(-1), nonfinite.any(-1)), "a marked destination is NaN in all its D channels"
    assert torch.equal(nonfinite.any(-1), touched), "every destination that received a non-finite contribution is marked"
    assert bool(torch.isnan(gv[nonfinite]).all())
    assert torch.equal(gv[~nonfinite], clean[~nonfinite]), "an unmarked destination changed"


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_torchs_flag_selects_the_deterministic_backward():
    from unseenobjectswithmeanshift_amd import MultiScaleDeformableAttention as MSDA
    from unseenobjectswithmeanshift_amd.training import MSDeformAttnFunction
    case = K.ENC_FORM_CASES[2]                                                              # D/V = 6: the atomic form has three atomic outputs
    b = K.bwd_inputs(case)
    shapes, start = geometry(case)
    want = result(case)
    was, was_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        value, loc, aw = (dev(t).requires_grad_(True) for t in (b.value, b.loc, b.aw))
        MSDeformAttnFunction.apply(value, shapes, start, loc, aw, 64).backward(dev(b.go))
        equal3((value.grad, loc.grad, aw.grad), want, "MSDeformAttnFunction under the flag")
        equal3(tuple(MSDA.ms_deform_attn_backward(dev(b.value), shapes, start, dev(b.loc), dev(b.aw), dev(b.go), 64)), want,
               "the drop-in module under the flag")
        equal3(ops().ms_deform_attn_backward(dev(b.value), shapes, start, dev(b.loc), dev(b.aw), dev(b.go)), want, "ops under the flag")
        unsupported = [c for c in C.BWD_CASES if c.D > 64 or len(c.levels) > C.MAXL]
        assert sorted((c.D, len(c.levels)) for c in unsupported) == [(8, 9), (71, 3)]
        calls = [(c, C.bwd_inputs(c), False) for c in unsupported] + [(C.BWD_CASES[0], C.bwd_inputs(C.BWD_CASES[0]), True)]
        for c, cb, f64 in calls:
            cs, ct = geometry(c)
            args = [dev(t.double() if f64 else t) for t in (cb.value, cb.loc, cb.aw, cb.go)]
            args = (args[0], cs, ct, args[1], args[2], args[3])
            torch.use_deterministic_algorithms(True)
            with pytest.raises(RuntimeError, match="ms_deform_attn_backward does not have a deterministic implementation"):
                ops().ms_deform_attn_backward(*args)
            torch.use_deterministic_algorithms(True, warn_only=True)
            with pytest.warns(UserWarning, match="ms_deform_attn_backward does not have a deterministic implementation"):
                got = ops().ms_deform_attn_backward(*args)
            refs, tols = C.backward_ref(c)
            for name, g, r, t in zip(GRADS, got, refs, C.bwd_bound(c, u=C.U64) if f64 else tols):
                inside(f"atomic kernel under warn_only {name}", c, g, r, t)
        # an explicit request outside the range raises whatever the flag says (no quiet fall-back)
        c = unsupported[0]
        cb = C.bwd_inputs(c)
        cs, ct = geometry(c)
        torch.use_deterministic_algorithms(False)
        with pytest.raises(RuntimeError, match="does not have a deterministic implementation"):
            ops().ms_deform_attn_backward(dev(cb.value), cs, ct, dev(cb.loc), dev(cb.aw), dev(cb.go), deterministic=True)
    finally:
        torch.use_deterministic_algorithms(was, warn_only=was_warn)
    # flag off: today's kernel, within the existing test's tolerance (no bit claim)
    assert not torch.are_deterministic_algorithms_enabled() or was
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = run(case, deterministic=False)
    refs, tols = K.backward_ref(case)
    for name, g, r, t in zip(GRADS, got, refs, tols):
        inside(f"{C.instantiation('bwd', case.D, 3, case.P)} {name}", case, g, r, t)


def test_the_library_itself_refuses_shapes_outside_its_range():
    """(ops raises before it calls the library; the entry point has no fall-back of its own either: checked before any launch)"""
    from unseenobjectswithmeanshift_amd import _lib
    o = ops()
    for c in (x for x in C.BWD_CASES if x.D > 64 or len(x.levels) > C.MAXL):
        b = C.bwd_inputs(c)
        shapes, start = geometry(c)
        t = [dev(x) for x in (b.value, b.loc, b.aw, b.go)]
        outs = [torch.empty_like(t[0]), torch.empty_like(t[1]), torch.empty_like(t[2])]
        S = t[0].shape[1]
        ws = torch.empty(o.ms_deform_attn_backward_det_workspace(c.B, S, c.M, c.D), dtype=torch.uint8, device=DEV)
        rc = _lib.lib().msm_msdeform_attn_bwd_det(o._p(t[0]), o._p(shapes), o._p(start), o._p(t[1]), o._p(t[2]), o._p(t[3]), o._p(outs[0]),
                                                  o._p(outs[1]), o._p(outs[2]), c.B, S, c.M, c.D, len(c.levels), c.Lq, c.P, o._p(ws),
                                                  ws.numel(), o._stream())
        assert rc != 0
        with pytest.raises(RuntimeError, match=r"msm_msdeform_attn_bwd_det: D=\d+, L=\d+: the deterministic backward covers D <= 64 and L <= 8"):
            _lib.check(rc, "msm_msdeform_attn_bwd_det")


# 9 ------------------------------------------------------------------------------------------------------------------------
def _pixel_decoder_step(seed):
    from unseenobjectswithmeanshift_amd import training as tr
    from unseenobjectswithmeanshift_amd.modeling import MSDeformAttnPixelDecoder, ShapeSpec
    shape = {k: ShapeSpec(channels=c, stride=s) for k, c, s in zip(("res2", "res3", "res4", "res5"), PD.PD_IN_CHANNELS, (4, 8, 16, 32))}
    pd = MSDeformAttnPixelDecoder(shape, transformer_dropout=0.0, transformer_nheads=8, transformer_dim_feedforward=PD.PD_FFN,
                                  transformer_enc_layers=PD.PD_ENC_LAYERS, conv_dim=PD.PD_CONV_DIM, mask_dim=PD.PD_MASK_DIM, norm="GN",
                                  transformer_in_features=["res3", "res4", "res5"], common_stride=4)
    pd.load_state_dict(PD.pd_state_dict(seed), strict=True)
    pd = pd.to(DEV)
    feats = {k: v.to(DEV).requires_grad_(True) for k, v in PD.pd_features(seed).items()}
    mf, enc, ms = tr.pixel_decoder_forward_train(pd, feats)
    PD.pd_functional(mf, enc, ms, seed).backward()
    torch.cuda.synchronize()
    grads = {"g_in__" + k: v.grad for k, v in feats.items()}
    grads.update({"g__" + n: p.grad for n, p in pd.named_parameters()})
    return grads


def test_pixel_decoder_gradients_repeat_bit_for_bit_under_the_flag():
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pixel_decoder_backward.npz")
    seed = int(np.load(golden)["seed"])
    was, was_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        first, second = _pixel_decoder_step(seed), _pixel_decoder_step(seed)
    finally:
        torch.use_deterministic_algorithms(was, warn_only=was_warn)
    assert sorted(first) == sorted(second) and len(first) == 4 + len(PD.pd_param_shapes())
    differ = [k for k in first if first[k] is None or not torch.equal(first[k], second[k])]
    print(f"pixel decoder under the flag: {len(first) - len(differ)} of {len(first)} gradient tensors repeat bit for bit")
    assert not differ, f"gradients that differ between two runs under torch.use_deterministic_algorithms(True): {differ}"
