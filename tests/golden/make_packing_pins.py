"""Bit pins of the host-side weight packing: dtype, shape and SHA-256 of what every layout function returns for seeded CPU inputs.

    python tests/golden/make_packing_pins.py   ->  tests/golden/packing_pins.json

The record is taken ONCE, at the commit a refactor of the packing code starts from, and is not regenerated afterwards:
tests/test_packing_cpu.py recomputes every case with the same cases() below and compares.  The functions are looked up in
unseenobjectswithmeanshift_amd.packing, or in ops at a commit that predates that module, so the script runs on both sides of
the move.  Needs the built library for the stream-size queries only; no GPU.

Not pinned: the identity row gather the bf16 plan once applied to the sampling projection (torch.arange; it is gone), and the
three-term splitter on its own (it had no name before the move; the f32_split streams pin it).
"""
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PINS = os.path.join(HERE, "packing_pins.json")
D, HEADS, LP, PW = 64, 8, 12, 288            # d_model, heads, levels x points, rows of [sampling_offsets | attention_weights]
D_FFN = (1024, 96, 160)                       # shipped; 96 and 160 pad the hm stream to 128, 160 (like 1024) pads the lp stream to 3 pairs


def _module():
    try:
        from unseenobjectswithmeanshift_amd import packing
        return packing
    except ImportError:
        from unseenobjectswithmeanshift_amd import ops
        return ops


def _randn(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def layer(d_ffn, seed):
    """One encoder layer's matrices and vectors at checkpoint-like magnitudes."""
    n = iter(range(seed * 100, seed * 100 + 100))
    mats = dict(wo=_randn(next(n), D, D, scale=D ** -0.5), w1=_randn(next(n), d_ffn, D, scale=D ** -0.5),
                w2=_randn(next(n), D, d_ffn, scale=d_ffn ** -0.5), wv=_randn(next(n), D, D, scale=D ** -0.5),
                wp=_randn(next(n), PW, D, scale=0.05))
    vecs = dict(bo=_randn(next(n), D), g1=_randn(next(n), D), be1=_randn(next(n), D), b1=_randn(next(n), d_ffn), b2=_randn(next(n), D),
                g2=_randn(next(n), D), be2=_randn(next(n), D), bv=_randn(next(n), D), bp=_randn(next(n), PW))
    return mats, vecs


def cases():
    """(name, thunk) for every pinned call; a thunk returns a tensor or a tuple of tensors."""
    P = _module()
    cpu = torch.device("cpu")
    two_terms = (lambda w: P.bf16_terms(w, 2)) if hasattr(P, "bf16_terms") else P._hl
    out = []
    for cin in (256, 2048):
        w = _randn(cin, D, cin, scale=cin ** -0.5)
        out.append((f"pack_conv_in_weight[cin={cin}]", lambda w=w: P.pack_conv_in_weight(w)))
        out.append((f"pack_conv_in_weight_lp[cin={cin}]", lambda w=w: P.pack_conv_in_weight_lp(w)))
    rc = _randn(11, 5 + 7, 256)
    out.append(("dense_kv_constant[width=7]", lambda: P.dense_kv_constant(rc, 7)))
    out.append(("dense_kv_constant[width=0]", lambda: P.dense_kv_constant(rc, 0)))
    cw, cb = _randn(12, 256, D, 3, 3, scale=1 / 24), _randn(13, 256, scale=0.1)
    out.append(("mask_conv_fold_weight[bias]", lambda: P.mask_conv_fold_weight(cw, cb)))
    out.append(("mask_conv_fold_weight[no bias]", lambda: P.mask_conv_fold_weight(cw)))
    out.append(("constants", lambda: torch.tensor([P.MASK_CONV_K, P.MASK_CONV_LD, P.PROJ_REC_FLOATS])))
    for i, d_ffn in enumerate(D_FFN):
        m, v = layer(d_ffn, i + 1)
        for nxt in (False, True):
            a = (m["wo"], m["w1"], m["w2"]) + ((m["wv"], m["wp"]) if nxt else ())
            tag = f"[d_ffn={d_ffn},next={int(nxt)}]"
            out.append(("pack_encoder_block" + tag, lambda a=a: P.pack_encoder_block(*a)))
            out.append(("pack_encoder_block_split" + tag, lambda a=a: P.pack_encoder_block_split(*a)))
            out.append(("pack_encoder_block_lp" + tag, lambda a=a: P.pack_encoder_block_lp(*a)))
            for f16 in (False, True):
                out.append((f"pack_encoder_block_hm[d_ffn={d_ffn},next={int(nxt)},ffn_f16={int(f16)}]",
                            lambda a=a, f16=f16: P.pack_encoder_block_hm(*a, ffn_f16=f16)))
            s = [v[k] for k in ("bo", "g1", "be1", "b1", "b2", "g2", "be2")] + ([v["bv"], v["bp"]] if nxt else [])
            out.append(("pack_encoder_block_hm_small" + tag, lambda s=s: P.pack_encoder_block_hm_small(*s)))
    m, v = layer(1024, 7)
    out.append(("pack_encoder_prologue", lambda: P.pack_encoder_prologue(m["wv"], m["wp"])))
    out.append(("pack_encoder_prologue_hm", lambda: P.pack_encoder_prologue_hm(m["wv"], m["wp"], v["bv"], v["bp"])))
    out.append(("pack_msda_proj_lp", lambda: P.pack_msda_proj_lp(m["wp"], v["bp"], HEADS, 3, 4)))
    proj = _randn(21, 2, 40, PW)
    out.append(("proj_to_head_major_records", lambda: P.proj_to_head_major_records(proj, HEADS, LP)))
    out.append(("proj_records_to_columns", lambda: P.proj_records_to_columns(P.proj_to_head_major_records(proj, HEADS, LP), HEADS, LP)))
    for K in (64, 1024):
        out.append((f"_korder_L[K={K}]", lambda K=K: P._korder_L(K, cpu)))
        out.append((f"_korder_natural[K={K}]", lambda K=K: P._korder_natural(K, cpu)))
    out.append(("_frag_blocks[L]", lambda: P._frag_blocks(m["wp"], P._korder_L(D, cpu))))
    out.append(("_frag_blocks[natural]", lambda: P._frag_blocks(m["w2"], P._korder_natural(1024, cpu))))
    out.append(("bf16_terms[2]", lambda: tuple(two_terms(m["w1"]))))
    out.append(("_value_row_perm", lambda: P._value_row_perm(cpu)))
    out.append(("_proj_row_perm_per_head", lambda: P._proj_row_perm_per_head(HEADS, LP, cpu)))
    return out


def digest(result):
    """[{dtype, shape, sha256}] of a tensor or a tuple of tensors (the bytes of the contiguous tensor)."""
    tensors = result if isinstance(result, (tuple, list)) else (result,)
    return [{"dtype": str(t.dtype), "shape": list(t.shape),
             "sha256": hashlib.sha256(t.detach().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()} for t in tensors]


def main():
    pins = {name: digest(thunk()) for name, thunk in cases()}
    with open(PINS, "w") as f:
        json.dump(pins, f, indent=1)
        f.write("\n")
    print(f"{len(pins)} cases -> {PINS} ({os.path.getsize(PINS) / 1024:.1f} KiB) from {_module().__name__}")


if __name__ == "__main__":
    main()
