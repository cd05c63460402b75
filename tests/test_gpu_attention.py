"""The hypersphere attention kernels (csrc/attention.hip, csrc/attention_bwd.hip) on the tables of tests/attn_cases.py: inputs in which
a single key or a single mask bit moves the answer by O(0.1 - 1), on every kernel path, mask mode, split and wave edge, against float64.

  * f32, and every form on the uniform-score family (U, Zu): rtol 1e-4 / atol 2e-5 against the float64 closed form / definition on V as
    the form rounds it.  The fused form's family U builds V from sums that are exact in fp32, so no element of V rounds to bf16 another
    way than float64's (the count the CPU yardstick shows is 0, asserted in test_attn_cases_cpu) and no element gets an allowance.
  * the 16-bit forms on families D, C, Z: at most twice the case's CPU yardstick (attn_cases.lp_bound), never above the project's
    3e-2 / 2e-3 (1.5e-2 / 8e-4 with fp16 scores); observed and yardstick are printed per case.
  * bwd: float64 autograd of the definition, err < 2e-4 scale + 1e-7 (tests/test_gpu_training.py); family U's closed-form grad_v.
  * strided views bit-equal to contiguous calls; sentinel runs of the C entry points.

Observed on an MI355X, maximum over all cases of a kind (|got - float64|):
  * f32 (also as the fallback of lp0 / lp3 at S <= 128) on D, C, Z: 2.2e-6; every form on U / Zu, the fused form included: 1.3e-7;
  * bf16 score operands (lp0, lp1) on D, C, Z: max 1.89e-2, mean 1.05e-3 -- the CPU yardstick's own 1.89e-2 / 1.05e-3; fused (fkv1): 1.69e-2 /
    7.8e-4 (yardstick 1.69e-2); the largest observed / bound ratio of a case is 0.63;
  * fp16 score operands (lp2, lp3): max 3.95e-3, mean 2.9e-4 (yardstick 3.95e-3); fused (fkv2): 2.36e-3 / 1.4e-4 (yardstick 2.36e-3);
    observed and yardstick agree to two digits in every case: the kernels round where the yardstick does;
  * bwd: largest err / scale 5.7e-6 (grad_k, 100 x 300 unmasked) against the rule's 2e-4.
"""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attn_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -12345.678


def ops():
    from unseenobjectswithmeanshift_amd import ops as _ops
    return _ops


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def set_options(lib_option, c):
    for name, value in c.opts:
        lib_option(name, value)


def device_kv(form, k, v):
    """K and V as the form's entry point takes them (attn_cases.stored already rounded the values)."""
    if form == "lp1":
        return dev(k).to(torch.bfloat16), dev(v).to(torch.bfloat16)
    if form == "lp2":                  # half bit patterns inside a bfloat16-typed tensor, as kv_project_multi(keys_f16=True) writes them
        return dev(k).to(torch.float16).view(torch.bfloat16), dev(v).to(torch.bfloat16)
    return dev(k), dev(v)


def fkv_operands(c, x):
    H, _ = c.hw
    E = c.heads * C.HD
    rowcol = dev(x.fkv.rowcol)
    return dict(x_f16=dev(x.fkv.x).to(torch.float16), w_packed=ops().attn_pack_kv_weights(dev(x.fkv.w), c.heads), rowcol=rowcol,
                col_v_t=rowcol[H:, E:].t().contiguous())


def forward(c, x, q=None, k=None, v=None):
    """The wrapper call of a forward case; q / k / v: device tensors to use instead (strided views)."""
    kw = dict(masked=dev(x.mask), row_any=dev(x.row_any), kappa=c.kappa)
    q = dev(x.q) if q is None else q
    if c.form in C.FKV_FORMS:
        f = fkv_operands(c, x)
        return ops().hypersphere_attention_fused_kv(q, f["x_f16"], f["w_packed"], f["rowcol"], f["col_v_t"], c.hw, c.heads,
                                                    keys_f16=c.form == "fkv2", **kw)
    if k is None:
        k, v = device_kv(c.form, *C.stored(c.form, x.k, x.v))
    return ops().hypersphere_attention(q, k, v, c.heads, low_precision=c.form != "f32", keys_f16=c.form in ("lp2", "lp3"), **kw)


def assert_unit_rows(got, ref, heads):
    """The output normalisation is fp32 in every form: norm 1 (0 where the float64 row is the zero vector: the mean of a zero v row alone)."""
    nrm = lambda t: t.reshape(t.shape[0], t.shape[1], heads, C.HD).norm(dim=-1)
    torch.testing.assert_close(nrm(got.cpu()), nrm(ref).float().round(), rtol=1e-5, atol=1e-5)


def check_f32(got, ref, what):
    err = (got.double() - ref).abs()
    tol = C.F32_ATOL + C.F32_RTOL * ref.abs()
    over = int((err > tol).sum())
    print(f"F32 {what:52s} max |d| {float(err.max()):.2e}  over tolerance {over}")
    assert bool(torch.isfinite(got).all()), what
    if over:
        b, i, e = (int(t) for t in torch.unravel_index((err - tol).argmax(), err.shape))
        raise AssertionError(f"{what}: {over} elements over rtol 1e-4 / atol 2e-5, worst at image {b} query {i} column {e}: "
                             f"got {float(got[b, i, e]):.6f} want {float(ref[b, i, e]):.6f}")


@pytest.mark.parametrize("case", C.FORWARD_CASES + C.FKV_CASES, ids=lambda c: c.id)
def test_forward(case, lib_option):
    c = case
    set_options(lib_option, c)
    x = C.inputs(c)
    got = forward(c, x)
    assert got.shape == (c.B, c.Lq, c.heads * C.HD) and got.dtype == torch.float32
    ref = C.reference(c)
    r = C.case_route(c)
    label = c.id + (" [runs the fp32 kernel]" if r.fallback else "")
    if C.exact(c):
        if c.form in C.FKV_FORMS:
            # elements of V the CPU yardstick rounds to bf16 another way than float64: none in this family (all sums exact in fp32), so no
            # output element may use the one-ulp allowance: the share allowed is 2 x 0
            _, v64 = C.fkv_kv(x.fkv, c.hw)
            flips = int((C.bf16(C.fkv_v_yardstick(x.fkv, c.hw)) != C.bf16(v64.float())).sum())
            print(f"    {c.id}: V roundings that differ in the yardstick {flips}, allowance used 0")
            assert flips == 0
        check_f32(got.cpu(), ref, label)
    else:
        err = (got.cpu().double() - ref).abs()
        bmax, bmean = C.lp_bound(c)
        ymax, ymean = C.yard_error(c)
        print(f"LP  {label:52s} {r.operand:4s} observed max {float(err.max()):.2e} mean {float(err.mean()):.2e} | yardstick max {ymax:.2e} mean {ymean:.2e}"
              f" | bound {bmax:.2e} / {bmean:.1e}")
        assert bool(torch.isfinite(got).all()), label
        assert float(err.max()) <= bmax and float(err.mean()) <= bmean, label
    assert_unit_rows(got, ref, c.heads)


@pytest.mark.parametrize("case", C.BWD_CASES, ids=lambda c: c.id)
def test_backward(case):
    c = case
    x = C.inputs(c)
    gout = C.bwd_grad_out(c)
    out64, gq, gk, gv = C.bwd_reference(c, gout)
    kw = dict(masked=dev(x.mask), row_any=dev(x.row_any), kappa=c.kappa)
    q, k, v = dev(x.q), dev(x.k), dev(x.v)
    fwd = ops().hypersphere_attention(q, k, v, c.heads, **kw)
    check_f32(fwd.cpu(), out64 if c.fam != "U" else C.reference(c), c.id + " (forward)")
    got = ops().hypersphere_attention_backward(q, k, v, c.heads, dev(gout), **kw)
    for g, ref, name in zip(got, (gq, gk, gv), "qkv"):
        scale = C.bwd_scale(c, ref, gout, out64)
        err = float((g.cpu().double() - ref).abs().max())
        print(f"BWD {c.id:40s} grad_{name} max |d| {err:.2e} scale {scale:.2e} ratio {err / scale:.1e}")
        assert bool(torch.isfinite(g).all()) and err < 2e-4 * scale + 1e-7, (c.id, name, err, scale)
    if c.fam == "U":
        closed = C.bwd_uniform_grad_v(c, gout)
        chosen = torch.zeros(c.B, c.S, dtype=torch.bool)
        for row, ks in enumerate(x.keep):
            chosen[row // c.Lq, ks[0]] = True
        g = got[2].cpu()
        assert float((g.double() - closed).abs().max()) < 2e-4 * float(closed.abs().max()) + 1e-7
        assert int(torch.count_nonzero(g[~chosen])) == 0                         # a key no row may attend to gets exactly no gradient


@pytest.mark.parametrize("case", C.STRIDED_CASES, ids=lambda c: c.id)
def test_strided_views_are_bit_equal(case, lib_option):
    """q, k and v as column slices of (B, ., 3E) buffers: the same bits as the contiguous call."""
    c = case
    set_options(lib_option, c)
    x = C.inputs(c)
    E = c.heads * C.HD
    qbuf = torch.full((c.B, c.Lq, 3 * E), 7.0, device=DEV)
    qbuf[..., E:2 * E] = dev(x.q)
    qv = qbuf[..., E:2 * E]
    assert not qv.is_contiguous()
    if c.form in C.FKV_FORMS:
        assert torch.equal(forward(c, x, q=qv), forward(c, x))
        return
    k, v = device_kv(c.form, *C.stored(c.form, x.k, x.v)) if c.form != "bwd" else (dev(x.k), dev(x.v))
    kvbuf = torch.full((c.B, c.S, 3 * E), 7.0, device=DEV, dtype=k.dtype)
    kvbuf[..., :E], kvbuf[..., 2 * E:] = k, v
    kv_, vv = kvbuf[..., :E], kvbuf[..., 2 * E:]
    if c.form == "bwd":
        kw = dict(masked=dev(x.mask), row_any=dev(x.row_any), kappa=c.kappa)
        gout = dev(C.bwd_grad_out(c))
        a = ops().hypersphere_attention_backward(qv, kv_, vv, c.heads, gout, **kw)
        b = ops().hypersphere_attention_backward(dev(x.q), k, v, c.heads, gout, **kw)
        assert all(torch.equal(s, t) and s.is_contiguous() for s, t in zip(a, b))
        return
    assert torch.equal(forward(c, x, q=qv, k=kv_, v=vv), forward(c, x))


def _sentinel_buffers(sizes, pad):
    return [torch.full((2 * pad + n,), SENTINEL, device=DEV) for n in sizes]


@pytest.mark.parametrize("case", C.SENTINEL_CASES, ids=lambda c: c.id)
def test_writes_only_its_outputs(case, lib_option):
    """The C entry points with the outputs and the workspace inside sentinel-filled buffers: nothing in front of them or behind
    B Lq E outputs (the backward: B S E for grad_k / grad_v) and the stated workspace size changes, every output element is written,
    and what is written is the wrapper's result."""
    from unseenobjectswithmeanshift_amd._lib import check, lib
    c = case
    set_options(lib_option, c)
    x = C.inputs(c)
    B, Lq, S, H, E = c.B, c.Lq, c.S, c.heads, c.heads * C.HD
    pad = 4096
    p = lambda t, off=0: ctypes.c_void_p(0 if t is None else t.data_ptr() + 4 * off)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    q, mask, row_any = dev(x.q), dev(x.mask), dev(x.row_any)
    if c.form == "bwd":
        k, v, gout = dev(x.k), dev(x.v), dev(C.bwd_grad_out(c))
        want = ops().hypersphere_attention_backward(q, k, v, H, gout, masked=mask, row_any=row_any, kappa=c.kappa)
        need = lib().msm_hypersphere_attn_bwd_workspace(B, Lq, H)
        assert need == B * H * Lq * C.BWD_REC
        sizes = [B * Lq * E, B * S * E, B * S * E, need]
        bufs = _sentinel_buffers(sizes, pad)
        rc = lib().msm_hypersphere_attn_bwd(p(q), p(k), p(v), p(mask), p(row_any), p(gout), p(bufs[0], pad), p(bufs[1], pad), p(bufs[2], pad), B, Lq, S, H,
                                            E, Lq * E, E, S * E, E, S * E, c.kappa, p(bufs[3], pad), need, stream)
        check(rc, "msm_hypersphere_attn_bwd")
        outputs = list(zip(bufs[:3], sizes[:3], want))
    else:
        want = forward(c, x)
        need = lib().msm_hypersphere_attn_workspace(B, Lq, S, H)
        assert need == C.workspace_floats(B, Lq, S, H, dict(c.opts))
        sizes = [B * Lq * E, need]
        bufs = _sentinel_buffers(sizes, pad)
        if c.form in C.FKV_FORMS:
            f = fkv_operands(c, x)
            bits = ops().attn_pack_mask_bits(mask)
            assert bits.numel() * 2 == lib().msm_attn_mask_bits_bytes(B, Lq, S)
            rc = lib().msm_hypersphere_attn_fused_kv_fwd(p(q), p(f["x_f16"]), p(f["w_packed"]), p(f["rowcol"]), p(f["col_v_t"]), 2 if c.form == "fkv2" else 1,
                                                         p(bits), p(row_any), p(bufs[0], pad), B, Lq, c.hw[0], c.hw[1], H, E, Lq * E, c.kappa,
                                                         p(bufs[1], pad), need, stream)
            check(rc, "msm_hypersphere_attn_fused_kv_fwd")
        else:
            k, v = device_kv(c.form, *C.stored(c.form, x.k, x.v))
            if c.form == "f32":
                rc = lib().msm_hypersphere_attn_fwd(p(q), p(k), p(v), p(mask), p(row_any), p(bufs[0], pad), B, Lq, S, H, E, Lq * E, E, S * E, E, S * E,
                                                    c.kappa, p(bufs[1], pad), need, stream)
            else:
                fmt = {"lp0": 0, "lp1": 1, "lp2": 2, "lp3": 3}[c.form]
                rc = lib().msm_hypersphere_attn_lp_fwd(p(q), p(k), p(v), fmt, p(mask), p(row_any), p(bufs[0], pad), B, Lq, S, H, E, Lq * E, E, S * E, E, S * E,
                                                       c.kappa, p(bufs[1], pad), need, stream)
            check(rc, "msm_hypersphere_attn_fwd")
        outputs = [(bufs[0], sizes[0], want)]
    for i, (buf, n) in enumerate(zip(bufs, sizes)):
        assert bool((buf[:pad] == SENTINEL).all()), f"buffer {i}: words in front of it"
        assert bool((buf[pad + n:] == SENTINEL).all()), f"buffer {i}: words behind its {n} floats"
    for i, (buf, n, ref) in enumerate(outputs):
        inside = buf[pad:pad + n]
        assert bool((inside != SENTINEL).all()), f"output {i}: elements never written"
        assert torch.equal(inside, ref.reshape(-1)), f"output {i}"
    r = C.case_route(c)
    if r.kernel in ("big", "fkv") and r.ns > 1:
        assert bool((bufs[1][pad:pad + sizes[1]] != SENTINEL).any())             # the partials went through the workspace
