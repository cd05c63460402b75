"""Host-side weight layouts (unseenobjectswithmeanshift_amd/packing.py) without a GPU: bit pins of every packed stream, the index
formulas the docstrings and include/msm_hip.h give, the record round trip and the bf16 term splitter.  The built library is used
for its stream-size queries only."""
import importlib.util
import json
import os

import pytest
import torch

from unseenobjectswithmeanshift_amd import packing as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_packing_pins", os.path.join(GOLDEN, "make_packing_pins.py"))
pins_gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pins_gen)

CASES = dict(pins_gen.cases())
with open(pins_gen.PINS) as _f:
    PINS = json.load(_f)

PUBLIC = ("pack_conv_in_weight", "pack_conv_in_weight_lp", "dense_kv_constant", "mask_conv_fold_weight", "MASK_CONV_K", "MASK_CONV_LD",
          "pack_encoder_prologue", "pack_encoder_prologue_hm", "pack_encoder_block", "pack_encoder_block_split", "pack_encoder_block_lp",
          "pack_encoder_block_hm", "pack_encoder_block_hm_small", "pack_msda_proj_lp", "proj_to_head_major_records",
          "proj_records_to_columns", "PROJ_REC_FLOATS")


# ---- bit pins -----------------------------------------------------------------------------------------------------------------
def test_pins_cover_every_case():
    """packing_pins.json was recorded by tests/golden/make_packing_pins.py before the packing code moved out of ops.py and is not
    regenerated: it and the generator's cases name the same calls, and every function of the module is among them."""
    assert set(CASES) == set(PINS)
    called = {name.split("[")[0] for name in PINS}
    assert {n for n in PUBLIC if n.startswith(("pack_", "proj_", "dense_", "mask_"))} <= called
    assert {"_korder_L", "_korder_natural", "_frag_blocks", "_value_row_perm", "_proj_row_perm_per_head", "bf16_terms", "constants"} <= called


@pytest.mark.parametrize("name", sorted(PINS))
def test_packed_bytes_match_the_pins(name):
    """dtype, shape and SHA-256 of the bytes of what the call returns, for the seeded CPU inputs of make_packing_pins.cases()."""
    assert pins_gen.digest(CASES[name]()) == PINS[name]


def test_ops_exports_the_packing_functions():
    from unseenobjectswithmeanshift_amd import ops
    for name in PUBLIC:
        assert getattr(ops, name) is getattr(P, name), name


# ---- definitions: brute-force indexing of the documented formulas -----------------------------------------------------------------
def bf16_integers(*shape):
    """A tensor of distinct integers every one of which bf16 holds exactly: +-(m << e), 8-bit m."""
    n = 1
    for s in shape:
        n *= s
    vals = list(range(1, 128)) + [m << e for e in range(65) for m in range(128, 256)]
    vals = [float(v) for v in vals] + [-float(v) for v in vals]
    assert n <= len(vals)
    w = torch.tensor(vals[:n], dtype=torch.float32)[torch.randperm(n, generator=torch.Generator().manual_seed(n))].reshape(shape)
    assert torch.equal(w.to(torch.bfloat16).float(), w) and w.unique().numel() == n
    return w


def test_pack_conv_in_weight_formula():
    Cin = 24
    w = bf16_integers(64, Cin)
    packed, wl = P.pack_conv_in_weight(w).tolist(), w.tolist()
    assert len(packed) == 64 * Cin
    for o in range(64):
        for k in range(Cin):
            assert packed[(((k // 8) * 4 + o // 16) * 64 + ((k % 8) // 2) * 16 + o % 16) * 2 + k % 2] == wl[o][k]
    with pytest.raises(RuntimeError):
        P.pack_conv_in_weight(torch.zeros(64, 12))


def test_pack_conv_in_weight_lp_formula():
    Cin = 256
    w = bf16_integers(64, Cin)
    packed = P.pack_conv_in_weight_lp(w)
    assert packed.dtype == torch.bfloat16 and packed.numel() == 2 * 64 * Cin
    p, wl = packed.float().reshape(Cin // 32, 4, 2, 4, 16, 8).tolist(), w.tolist()
    for o in range(64):
        for k in range(Cin):
            assert p[k // 32][o // 16][0][(k % 32) // 8][o % 16][k % 8] == wl[o][k]            # plane 0 = bf16(w) = w
            assert p[k // 32][o // 16][1][(k % 32) // 8][o % 16][k % 8] == 0.0                 # plane 1 = bf16(w - plane 0)


def test_rowblocks_formula():
    w = bf16_integers(48, 64)
    blocks, wl = P.rowblocks(w), w.tolist()
    assert tuple(blocks.shape) == (3, 1024)
    b = blocks.reshape(3, 2, 4, 16, 2, 4).tolist()                                             # [block][G][lq][lj][hh][c]
    for rb in range(3):
        for G in range(2):
            for lq in range(4):
                for lj in range(16):
                    for hh in range(2):
                        for c in range(4):
                            assert b[rb][G][lq][lj][hh][c] == wl[rb * 16 + lj][(2 * G + hh) * 16 + lq * 4 + c]


def test_w2pairs_formula():
    d_ffn = 96
    w = bf16_integers(64, d_ffn)
    pairs, wl = P.w2pairs(w, d_ffn), w.tolist()
    assert tuple(pairs.shape) == (d_ffn // 32, 2048)
    b = pairs.reshape(d_ffn // 32, 4, 4, 16, 2, 4).tolist()                                    # [P][ob][lq][lj][hh][c]
    for Pp in range(d_ffn // 32):
        for ob in range(4):
            for lq in range(4):
                for lj in range(16):
                    for hh in range(2):
                        for c in range(4):
                            assert b[Pp][ob][lq][lj][hh][c] == wl[ob * 16 + lj][(2 * Pp + hh) * 16 + lq * 4 + c]


@pytest.mark.parametrize("order", ["L", "natural"])
@pytest.mark.parametrize("R,K", [(32, 64), (16, 128)])
def test_frag_blocks_formula(order, R, K):
    cpu = torch.device("cpu")
    korder = (P._korder_L if order == "L" else P._korder_natural)(K, cpu)
    assert tuple(korder.shape) == (K // 32, 4, 8) and sorted(korder.reshape(-1).tolist()) == list(range(K))
    w = bf16_integers(R, K)
    blocks, wl, ko = P._frag_blocks(w, korder), w.tolist(), korder.tolist()
    assert tuple(blocks.shape) == (R // 16, K // 32, 512)
    b = blocks.reshape(R // 16, K // 32, 64, 8).tolist()
    for rb in range(R // 16):
        for G in range(K // 32):
            for kq in range(4):
                for i in range(16):
                    for j in range(8):
                        col = (2 * G + (j >> 2)) * 16 + 4 * kq + (j & 3) if order == "L" else 32 * G + 8 * kq + j
                        assert ko[G][kq][j] == col
                        assert b[rb][G][kq * 16 + i][j] == wl[rb * 16 + i][col]


def test_pair_hl_stacks_the_two_terms():
    w = torch.randn(32, 64, generator=torch.Generator().manual_seed(5))
    kL = P._korder_L(64, torch.device("cpu"))
    h, l = P.bf16_terms(w, 2)
    pair = P.pair_hl(w, kL)
    assert tuple(pair.shape) == (2, 2, 2, 512)
    assert torch.equal(pair[:, :, 0], P._frag_blocks(h, kL)) and torch.equal(pair[:, :, 1], P._frag_blocks(l, kL))


def test_row_permutations():
    cpu = torch.device("cpu")
    perm = P._value_row_perm(cpu).tolist()
    assert sorted(perm) == list(range(64))
    for rb in range(4):
        for lq in range(4):
            for r in range(4):
                assert perm[16 * rb + 4 * lq + r] == (4 * (rb >> 1) + lq) * 8 + 4 * (rb & 1) + r
    heads, LP = 8, 12
    perm = P._proj_row_perm_per_head(heads, LP, cpu).tolist()
    assert sorted(perm) == list(range(heads * 3 * LP))
    for m in range(heads):
        for c in range(3 * LP):
            assert perm[m * 36 + c] == (m * 2 * LP + c if c < 2 * LP else heads * 2 * LP + m * LP + c - 2 * LP)


def test_round4_weight_layouts_match_the_header_formulas():
    """Host-side packing of the round-4 kernels, checked against the index formulas include/msm_hip.h documents (pure tensor code:
    runs without a GPU): the hi + lo fragment order of msm_conv1x1_in_lp, the separable K/V constant, and the sizes the library
    reports for the bf16 plan's prologue blocks."""
    from unseenobjectswithmeanshift_amd import ops
    from unseenobjectswithmeanshift_amd._lib import lib
    g = torch.Generator().manual_seed(3)
    Cin = 512
    w = torch.randn(64, Cin, generator=g) * Cin ** -0.5
    wp = ops.pack_conv_in_weight_lp(w)
    assert wp.dtype == torch.bfloat16 and wp.numel() == 2 * 64 * Cin
    hi = w.to(torch.bfloat16)
    planes = torch.stack([hi, (w - hi.float()).to(torch.bfloat16)])
    k, o = torch.meshgrid(torch.arange(Cin), torch.arange(64), indexing="ij")
    for pl in range(2):
        idx = ((((k // 32) * 4 + o // 16) * 2 + pl) * 64 + ((k % 32) // 8) * 16 + o % 16) * 8 + k % 8
        assert torch.equal(wp[idx], planes[pl].t())
    # hi + lo carries the weight to 2^-16 relative
    assert float(((planes[0].float() + planes[1].float()) - w).abs().max()) <= float(w.abs().max()) * 2.0 ** -15
    with pytest.raises(RuntimeError):
        ops.pack_conv_in_weight_lp(torch.zeros(64, 128))
    # separable K/V constant: H row vectors then W column vectors; token (y, x) gets row[y] + col[x]
    H, W, N = 5, 7, 256
    rc = torch.randn(H + W, N, generator=g)
    dense = ops.dense_kv_constant(rc, W)
    assert tuple(dense.shape) == (H * W, N) and torch.equal(dense.view(H, W, N)[3, 4], rc[3] + rc[H + 4])
    assert ops.dense_kv_constant(dense, 0) is dense
    # the prologue blocks of the bf16 plan: value (16 KiB) + projection (72 KiB) as [row block][k-group][hi, lo] 1-KiB fragments
    assert lib().msm_encoder_prologue_hm_weight_bytes() == 16384 + 18 * 4096
    blocks, small = ops.pack_encoder_prologue_hm(torch.randn(64, 64, generator=g), torch.randn(288, 64, generator=g),
                                                 torch.randn(64, generator=g), torch.randn(288, generator=g))
    assert blocks.dtype == torch.int16 and blocks.numel() * 2 == 16384 + 18 * 4096 and small.numel() == 352


def test_packed_results_do_not_alias_the_parameters():
    """The projection's rows go into the hm streams in the checkpoint's own order (no gather): what the packers return must still
    be storage of its own, since modeling caches it next to the Parameters."""
    m, v = pins_gen.layer(96, 9)
    srcs = list(m.values()) + list(v.values())
    outs = [P.pack_encoder_block_hm(m["wo"], m["w1"], m["w2"], m["wv"], m["wp"]),
            P.pack_encoder_block_hm_small(*[v[k] for k in ("bo", "g1", "be1", "b1", "b2", "g2", "be2", "bv", "bp")]),
            *P.pack_encoder_prologue_hm(m["wv"], m["wp"], v["bv"], v["bp"]), *P.pack_msda_proj_lp(m["wp"], v["bp"])]
    ptrs = {t.untyped_storage().data_ptr() for t in srcs}
    assert all(o.untyped_storage().data_ptr() not in ptrs for o in outs)


def test_size_mismatch_is_a_runtime_error():
    """A stream that disagrees with the library's size is reported by an exception, not an assert (python -O keeps it)."""
    with pytest.raises(RuntimeError, match=r"pack_x: built 10 bytes, the kernel expects 12"):
        P._expect("pack_x", 10, 12)
    P._expect("pack_x", 12, 12)


# ---- round trip of the sampling records -----------------------------------------------------------------------------------------
def test_proj_records_round_trip():
    p = torch.randn(2, 40, 288, generator=torch.Generator().manual_seed(8))
    rec = P.proj_to_head_major_records(p)
    assert tuple(rec.shape) == (2, 8, 40, P.PROJ_REC_FLOATS) and rec.dtype == torch.float32
    want = torch.cat([p[..., :192], p[..., 192:].to(torch.float16).float()], -1)                # the logits travel as fp16
    assert torch.equal(P.proj_records_to_columns(rec), want)


# ---- the term splitter ----------------------------------------------------------------------------------------------------------
def test_bf16_terms():
    """bf16 keeps 8 significant bits, so each term leaves at most 2^-8 of what it rounds: two terms carry w to 2^-16 |w|, and after
    two terms at most 8 of an fp32's 24 bits are left, which the third holds exactly.  Sums in float64 (exact for these)."""
    w = torch.randn(256, 257, generator=torch.Generator().manual_seed(4))
    wd = w.double()
    (h1,) = P.bf16_terms(w, 1)
    assert torch.equal(h1, w.to(torch.bfloat16).float())
    h, m = P.bf16_terms(w, 2)
    assert torch.equal(h, h1) and torch.equal(m, (w - h).to(torch.bfloat16).float())
    assert bool(((h.double() + m.double() - wd).abs() <= 2.0 ** -16 * wd.abs()).all())
    h3, m3, l3 = P.bf16_terms(w, 3)
    assert torch.equal(h3, h) and torch.equal(m3, m) and torch.equal(l3, ((w - h) - m).to(torch.bfloat16).float())
    assert torch.equal(h3.double() + m3.double() + l3.double(), wd)
    for t in (h3, m3, l3):
        assert t.dtype == torch.float32 and torch.equal(t.to(torch.bfloat16).float(), t)
