"""tests/gemm_cases.py checked on the CPU: for every case of its tables the derived bound is (a) not too tight -- torch's own fp32
result (F.linear / F.conv2d in float32, a summation order of its own) lies inside it in every element -- and (b) not toothless --
three wrong references (the last k-term dropped, the bias shifted by one column, one tap of the 3x3 weight zeroed) lie outside it
in at least one element of every case where they are expressible, and in the large majority of elements overall.  Also: the restated
host dispatch reaches every kernel instantiation from the tables, and no split of the split-K cases is empty."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_cases as G  # noqa: E402


def _linear_case(name, a, a2, w, bias):
    K = a.shape[-1]
    a32 = a if a2 is None else a + a2
    wrong = {"last k dropped": G.linear64(a[..., :K - 1], None if a2 is None else a2[..., :K - 1], w[:, :K - 1], bias, None)}
    if bias is not None and w.shape[0] > 1:
        wrong["bias shifted"] = G.linear64(a, a2, w, bias.roll(1, -1), None)
    return name, G.linear64(a, a2, w, bias, None), G.linear_tol(a, a2, w, bias), F.linear(a32, w) if bias is None else F.linear(a32, w) + bias, wrong


def _conv1x1_case(name, x, w, bias, out):
    Cin = x.shape[1]
    y32 = F.conv2d(x, w[:, :, None, None]).flatten(2).transpose(1, 2)
    if bias is not None:
        y32 = y32 + bias
    wrong = {"last k dropped": G.conv1x1_64(x[:, :Cin - 1], w[:, :Cin - 1], bias, out)}
    if bias is not None and w.shape[0] > 1:
        wrong["bias shifted"] = G.conv1x1_64(x, w, bias.roll(1, -1), out)
    return name, G.conv1x1_64(x, w, bias, out), G.conv1x1_tol(x, w, bias, out), y32 if out == "tokens" else y32.transpose(1, 2), wrong


def _conv3x3_case(name, x, w, bias, out):
    y32 = F.conv2d(x, w, bias, padding=1).flatten(2)
    wrong = {}
    if x.shape[2] > 1 and x.shape[3] > 1:          # k = 9 * Cin - 1 is tap (2, 2): on a one-pixel-wide or -high map it only ever meets padding
        w_last = w.clone()
        w_last[:, -1, 2, 2] = 0
        wrong["last k dropped"] = G.conv3x3_64(x, w_last, bias, out)
    w_tap = w.clone()
    w_tap[:, :, 1, 1] = 0
    wrong["tap zeroed"] = G.conv3x3_64(x, w_tap, bias, out)
    if bias is not None and w.shape[0] > 1:
        wrong["bias shifted"] = G.conv3x3_64(x, w, bias.roll(1), out)
    return name, G.conv3x3_64(x, w, bias, out), G.conv3x3_tol(x, w, bias, out), y32.transpose(1, 2) if out == "tokens" else y32, wrong


def _cases():
    for M, N, K in G.LINEAR_SHAPES:
        a, w, b = G.linear_inputs(M, N, K)
        yield _linear_case(f"linear {M}x{N}x{K} bias", a, None, w, b)
        yield _linear_case(f"linear {M}x{N}x{K}", a, None, w, None)
    for shape in G.A2_SHAPES:
        a, a2, a2b, w, b = G.a2_inputs(*shape)
        yield _linear_case(f"a2 {shape}", a, a2, w, b)
        yield _linear_case(f"a2 broadcast {shape}", a, a2b.expand_as(a), w, b)
    for K, s in G.SPLITK_CASES:
        a, w, _ = G.linear_inputs(*G.SPLITK_MN, K)
        yield _linear_case(f"split-K {K}/{s}", a, None, w, None)
    for shape in G.MCONTIG_SHAPES:
        inp = G.conv1x1_inputs(*shape)
        for kind in G.MCONTIG_BIAS:
            yield _conv1x1_case(f"m-contiguous {shape} bias {kind}", inp[0], inp[1], G.mcontig_bias(inp, kind), "tokens")
    for B, HW, Cin, Cout in G.NCHW_SHAPES:
        x, w, b, _ = G.conv1x1_inputs(B, Cin, HW, 1, Cout)
        yield _conv1x1_case(f"nchw-out {(B, HW, Cin, Cout)}", x, w, b, "nchw")
    for shape in G.CONV3_TOKEN_SHAPES:
        x, w, _ = G.conv3x3_inputs(*shape)
        yield _conv3x3_case(f"conv3x3 tokens {shape}", x, w, None, "tokens")
    for shape in G.CONV3_NCHW_SHAPES:
        x, w, b = G.conv3x3_inputs(*shape)
        yield _conv3x3_case(f"conv3x3 nchw {shape} bias", x, w, b, "nchw")
        yield _conv3x3_case(f"conv3x3 nchw {shape}", x, w, None, "nchw")
    x, w, b, g = G.train_inputs()
    yield _linear_case("training forward", x, None, w, b)
    yield _linear_case("training grad_in", g, None, w.t().contiguous(), None)
    yield _linear_case("training grad_W", g.t().contiguous(), None, x.t().contiguous(), None)
    yield _linear_case("training grad_b", torch.ones(1, g.shape[0]), None, g.t().contiguous(), None)


CASES = list(_cases())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fp32_inside_and_wrong_references_outside(case):
    name, ref, tol, t32, wrong = case
    assert ref.dtype == tol.dtype == torch.float64 and t32.dtype == torch.float32
    assert bool((tol >= 0).all()) and bool(torch.isfinite(tol).all())
    assert G.outside(t32, ref, tol) == 0, f"{name}: torch's fp32 result leaves the bound in {G.outside(t32, ref, tol)} of {ref.numel()} elements"
    print(f"{name}: torch fp32 uses {G.ratio(t32, ref, tol):.3f} of the bound")
    assert "last k dropped" in wrong or "tap zeroed" in wrong
    for kind, bad in wrong.items():
        assert G.outside(bad, ref, tol) >= 1, f"{name}: the reference with {kind} passes the bound"


def test_wrong_references_outside_in_the_large_majority():
    miss, total = {}, {}
    for name, ref, tol, _, wrong in CASES:
        for kind, bad in wrong.items():
            miss[kind] = miss.get(kind, 0) + G.outside(bad, ref, tol)
            total[kind] = total.get(kind, 0) + ref.numel()
    assert set(miss) == {"last k dropped", "bias shifted", "tap zeroed"}
    for kind in miss:
        print(f"{kind}: outside the bound in {miss[kind]} of {total[kind]} elements")
        assert miss[kind] >= 0.9 * total[kind]


def test_outside_counts_non_finite_values():
    ref, tol = torch.zeros(3, dtype=torch.float64), torch.ones(3, dtype=torch.float64)
    assert G.outside(torch.tensor([0.5, float("nan"), float("inf")]), ref, tol) == 2
    assert G.outside(torch.tensor([1.0, -1.0, 1.5]), ref, tol) == 1


def test_split_ranges():
    for K, s in G.SPLITK_CASES:
        r = G.split_ranges(K, s)
        assert len(r) == s and r[0][0] == 0 and r[-1][1] == K
        assert all(k0 < k1 and k0 % 32 == 0 for k0, k1 in r) and all(r[i][1] == r[i + 1][0] for i in range(s - 1))
    assert G.split_ranges(1000, 4)[-1] == (768, 1000) and G.split_ranges(100, 2)[-1] == (64, 100)
    assert G.split_ranges(64, 8) is None            # kps = 32: splits 2..7 would own nothing, the library rejects the call


def test_tables_reach_every_instantiation():
    """Every gemm_kernel instantiation the entry points can launch is launched by at least one case of the tables, each
    (tile, shallow) pair and each A mode included."""
    count = G.table_instantiations()
    assert set(count) == G.all_instantiations(), sorted(G.all_instantiations() ^ set(count))
    assert len(count) == 40
    for key in sorted(count):
        print("gemm_kernel<MI=%d, NI=%d, AMODE=%d, SWAP=%d, VEC=%d, A2=%d, KT=%d>: %d cases" % (*key, count[key]))
