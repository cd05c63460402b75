"""Host-side weight layouts: a checkpoint's matrices as the operand streams the kernels read (include/msm_hip.h).

Pure torch reshapes and permutes, on whatever device the weights live on (a CPU will do); the library is asked for a stream's
size only, never to launch.  They run once per parameter version, before capture.  Packers that launch a kernel
(dec_pack_weight*, pack_mask_features_*, attn_pack_*, pack_msda_proj, ms_pack_bf16) are launch wrappers and live in ops.py;
every public name here is importable from ops as well.
"""
import torch

from ._lib import lib


# ---- shared pieces: bf16 terms, row blocks, MFMA fragment blocks -------------------------------------------------------------
def bf16_terms(w, n):
    """w as a sum of n bf16 terms h, m, l, ...: each the bf16 rounding of what the earlier ones leave, the residual formed left to
    right in fp32 ((w - h) - m).  Returns n fp32 tensors holding bf16 values: two carry w to 2^-16 relative, three carry it exactly
    (24 mantissa bits) unless the last term underflows."""
    terms, r = [], w
    for _ in range(n):
        if terms:
            r = r - terms[-1]
        terms.append(r.to(torch.bfloat16).float())
    return terms


def _bits(t, dtype=torch.bfloat16):
    """fp32 -> the int16 bit patterns of its 16-bit roundings (to nearest even)."""
    return t.to(dtype).contiguous().view(torch.int16)


def _expect(who, built, need, unit="bytes"):
    if built != need:
        raise RuntimeError(f"{who}: built {built} {unit}, the kernel expects {int(need)}")


def rowblocks(w):
    """(N, 64) -> (N/16, 1024), the K = 32 kernels' 16-row blocks: block[G][lq][lj][hh][c] = W[r0 + lj][(2G + hh)*16 + lq*4 + c]."""
    return w.reshape(-1, 16, 2, 2, 4, 4).permute(0, 2, 4, 1, 3, 5).reshape(-1, 1024)


def w2pairs(w, d_ffn):
    """linear2 (64, d_ffn) -> (d_ffn/32, 2048), one row per pair P of 16-wide hidden blocks:
    [ob][lq][lj][hh][c] = W[ob*16 + lj][(2P + hh)*16 + lq*4 + c]."""
    return w.reshape(4, 16, d_ffn // 32, 2, 4, 4).permute(2, 0, 4, 1, 3, 5).reshape(-1, 2048)


def _k_grids(K, device):
    """Index grids of a K-wide contraction in v_mfma_f32_16x16x32_bf16 fragments: 32-wide group G, lane quarter kq, element j."""
    return (torch.arange(K // 32, device=device).view(-1, 1, 1), torch.arange(4, device=device).view(1, -1, 1),
            torch.arange(8, device=device).view(1, 1, -1))


def _korder_L(K, device):
    """k order "L" of a K-wide contraction whose B operand comes from layout-L registers (lane (token, lq) holds features
    fb*16 + lq*4 + r): 32-wide group G, lane quarter kq, element j  <->  column (2G + (j >> 2))*16 + 4 kq + (j & 3)."""
    G, kq, j = _k_grids(K, device)
    return (2 * G + (j >> 2)) * 16 + 4 * kq + (j & 3)


def _korder_natural(K, device):
    """The k order of operands read straight from memory: (G, kq, j) <-> column 32 G + 8 kq + j."""
    G, kq, j = _k_grids(K, device)
    return 32 * G + 8 * kq + j


def _frag_blocks(w, korder):
    """w (R, K) -> (R/16, K/32, 512): 1-KiB A-operand blocks of v_mfma_f32_16x16x32_bf16, block[rb][G][kq*16 + i][j] =
    w[rb*16 + i][korder[G][kq][j]]."""
    R, K = w.shape
    t = w.reshape(R // 16, 16, K)[:, :, korder]              # (rb, i, G, kq, j)
    return t.permute(0, 2, 3, 1, 4).reshape(R // 16, K // 32, 512)


def pair_hl(w, korder):
    """(R, K) -> (R/16, K/32, 2, 512): the fragment blocks of w's two bf16 terms side by side, [rb][G][h, l]."""
    h, l = bf16_terms(w, 2)
    return torch.stack([_frag_blocks(h, korder), _frag_blocks(l, korder)], 2)


# ---- input projections (csrc/conv_in.hip) -----------------------------------------------------------------------------------
def pack_conv_in_weight(w):
    """(64, Cin) 1x1-convolution weight -> the fragment order msm_conv1x1_in_f32 reads (include/msm_hip.h):
    packed[(((k//8)*4 + o//16)*64 + ((k%8)//2)*16 + o%16)*2 + k%2] = w[o][k]."""
    O, Cin = w.shape
    if O != 64 or Cin % 8:
        raise RuntimeError("pack_conv_in_weight needs a (64, Cin) weight with Cin a multiple of 8")
    return w.reshape(4, 16, Cin // 8, 4, 2).permute(2, 0, 3, 1, 4).contiguous().reshape(-1)


def pack_conv_in_weight_lp(w):
    """(64, Cin) weight -> the hi + lo bf16 fragment order msm_conv1x1_in_lp reads (include/msm_hip.h):
    packed[g][o//16][plane][(k%32)//8][o%16][k%8] = plane(w)[o][k], g = k//32, plane 0 = bf16(w), plane 1 = bf16(w - plane 0)."""
    O, Cin = w.shape
    if O != 64 or Cin % 256:
        raise RuntimeError("pack_conv_in_weight_lp needs a (64, Cin) weight with Cin a multiple of 256")
    planes = torch.stack(bf16_terms(w, 2)).to(torch.bfloat16)                        # (2, 64, Cin)
    return planes.reshape(2, 4, 16, Cin // 32, 4, 8).permute(3, 1, 0, 4, 2, 5).contiguous().reshape(-1)


# ---- decoder constants -------------------------------------------------------------------------------------------------------
def dense_kv_constant(cmat, cmat_width):
    """The (H*W, N) matrix of a separable constant [(H row vectors | W column vectors), N] (cmat_width = W; 0: cmat itself)."""
    if not cmat_width:
        return cmat
    h = cmat.shape[0] - cmat_width
    return (cmat[:h, None, :] + cmat[None, h:, :]).reshape(h * cmat_width, cmat.shape[1]).contiguous()


MASK_CONV_K = 576            # 9 taps x 64 channels; column 576 of a folded filter row is the per-query constant
MASK_CONV_LD = 580           # row length of mask_conv_fold_weight's GEMM output (16-byte aligned rows)


def mask_conv_fold_weight(weight, bias=None):
    """Conv2d(64, Cm, 3, padding=1) weight (Cm, 64, 3, 3) [+ bias (Cm,)] -> the (580, Cm) matrix Wf with
    gemm(e, Wf)[b, q] = [F[b, q, 64 * (3 ky + kx) + c] = sum_o e[b, q, o] W[o, c, ky, kx] | e[b, q, :] . bias | 0 0 0]:
    the per-query 3x3 filters mask_conv3x3_folded convolves the 64-channel feature with (the convolution folded into the embedding)."""
    Cm, C, kh, kw = weight.shape
    if (C, kh, kw) != (64, 3, 3):
        raise RuntimeError("mask_conv_fold_weight: a (Cm, 64, 3, 3) convolution weight")
    wf = torch.zeros((MASK_CONV_LD, Cm), device=weight.device, dtype=torch.float32)
    wf[:MASK_CONV_K] = weight.detach().float().permute(2, 3, 1, 0).reshape(MASK_CONV_K, Cm)
    if bias is not None:
        wf[MASK_CONV_K] = bias.detach().float()
    return wf


# ---- the fp32 encoder (csrc/enc_block.hip; msdeformattn.py:122-131) ---------------------------------------------------------------
def pack_encoder_prologue(wv, wp):
    """Weight stream of msm_encoder_prologue_fwd: value_proj (64,64) then [sampling_offsets | attention_weights]
    (proj_width,64) as consecutive 16-row blocks, zero-padded to the stream length."""
    pw = wp.shape[0]
    n = int(lib().msm_encoder_prologue_stream_floats(pw))
    out = torch.zeros(n, device=wv.device, dtype=torch.float32)
    out[:64 * 64] = wv.reshape(-1)
    out[64 * 64:64 * 64 + pw * 64] = wp.reshape(-1)
    return out


def pack_encoder_block(wo, w1, w2, wv=None, wp=None):
    """Pack one encoder layer's matrices into the weight stream consumed by msm_encoder_block_fwd.

    Stream = chunks of 8 blocks, one block = 1024 floats (4 KiB):
      chunk 0            : output_proj  -- 4 row blocks [16 out rows][64 k] (+4 zero blocks)
      chunks 1..d_ffn/64 : 4 x ( linear1 row block [16 hidden rows][64 k] , linear2 block [64 out rows][16 hidden] )
      then (only with the next layer's wv/wp): value_proj 4 row blocks, then [offsets|weights] row blocks,
      continuing into further chunks of 8.
    A "row block" is 16 consecutive rows of a (N, 64) weight; the kernel applies the LDS swizzle itself."""
    dev = wo.device
    d_ffn = w1.shape[0]
    blocks = [wo.reshape(4, 1024)] + [torch.zeros(4, 1024, device=dev)]
    w1b = w1.reshape(d_ffn // 16, 1024)                                                # (hb, 16 rows * 64 k)
    w2b = w2.reshape(64, d_ffn // 16, 16).permute(1, 0, 2).reshape(d_ffn // 16, 1024)    # (hb, 64 rows * 16 k)
    blocks.append(torch.stack([w1b, w2b], 1).reshape(-1, 1024))                        # interleaved per hb
    if wv is not None:
        npb = wp.shape[0] // 16
        tail = torch.cat([wv.reshape(4, 1024), wp.reshape(npb, 1024)], 0)
        pad = (-tail.shape[0]) % 8
        blocks += [tail, torch.zeros(pad, 1024, device=dev)]
    return torch.cat(blocks, 0).reshape(-1).contiguous()


# ---- the K = 32 encoder kernels: f32_split and the bf16 plan's fallback (csrc/enc_block_split.hip) --------------------------------
def pack_encoder_block_split(wo, w1, w2, wv=None, wp=None):
    """One encoder layer's matrices as the triple-split weight stream of msm_encoder_block_split_fwd (include/msm_hip.h):
    every fp32 weight as w = h + m + l with h = bf16(w), m = bf16(w - h), l = bf16(w - h - m); 2-KiB blocks in the fragment
    order of v_mfma_f32_16x16x32_bf16, a logical block = its (h, m, l) blocks, 12 blocks per stage.
    Returns an int16 tensor (bf16 bit patterns)."""
    d_ffn = w1.shape[0]

    def triples(w, blocks=rowblocks):                     # (n, 3k): [h | m | l] per logical block
        return torch.cat([blocks(t) for t in bf16_terms(w, 3)], 1)

    w1t = triples(w1).reshape(d_ffn // 32, 2 * 3 * 1024)                                      # per stage: W1(q0) h,m,l | W1(q1) h,m,l
    w2t = triples(w2, lambda t: w2pairs(t, d_ffn))                                            # per stage: W2 h | m | l (4 KiB each)
    blocks = [triples(wo).reshape(-1), torch.cat([w1t, w2t], 1).reshape(-1)]
    if wv is not None:
        pt = triples(wp).reshape(-1)
        blocks += [triples(wv).reshape(-1), pt, torch.zeros((-(pt.numel() // 1024)) % 12 * 1024, device=wo.device)]
    out = _bits(torch.cat(blocks, 0)).reshape(-1)
    _expect("pack_encoder_block_split", out.numel() * 2, lib().msm_encoder_block_split_stream_bytes(d_ffn, 0 if wp is None else wp.shape[0]))
    return out


def pack_encoder_block_lp(wo, w1, w2, wv=None, wp=None):
    """One encoder layer's matrices as the weight stream of msm_encoder_block_lp_fwd (include/msm_hip.h): the low-precision
    mode on the K = 32 kernel -- projections as [h, m] bf16 pairs, linear1 / linear2 as single bf16 copies, three hidden pairs
    per 12-block stage.  Returns an int16 tensor (bf16 bit patterns)."""
    dev = wo.device
    d_ffn = w1.shape[0]

    def proj_stages(w):                                   # [h, m] per row block, zero padded to whole 12-block stages
        t = torch.stack([rowblocks(t) for t in bf16_terms(w, 2)], 1).reshape(-1, 1024)
        return torch.cat([t, torch.zeros((-t.shape[0]) % 12, 1024, device=dev)], 0).reshape(-1)

    npair = d_ffn // 32
    ffn = torch.cat([rowblocks(w1).reshape(npair, 2048), w2pairs(w2, d_ffn)], 1)    # per pair: W1(q0) | W1(q1) | W2: 4 blocks, rounded below
    ffn = torch.cat([ffn, torch.zeros((-npair) % 3, 4096, device=dev)], 0).reshape(-1)
    blocks = [proj_stages(wo), ffn]
    if wv is not None:
        blocks += [proj_stages(wv), proj_stages(wp)]
    out = _bits(torch.cat(blocks, 0)).reshape(-1)
    _expect("pack_encoder_block_lp", out.numel() * 2, lib().msm_encoder_block_lp_stream_bytes(d_ffn, 0 if wp is None else wp.shape[0]))
    return out


# ---- the bf16 plan's encoder with head-major 16-bit activations (csrc/enc_lp.hip) -------------------------------------------------
# The [sampling_offsets | attention_weights] projection keeps the reference's own row order in these streams (offsets of every
# head, then the logits), so a 16-row block of the MFMA output is all offsets or all logits; only value_proj is permuted.
def _value_row_perm(device):
    """Row (16 rb + 4 lq + r) of the packed value_proj = value feature head*8 + dim with head = 4 (rb >> 1) + lq,
    dim = 4 (rb & 1) + r: a lane's row blocks 2j, 2j + 1 are the eight dims of one head (one 16-byte store)."""
    rb = torch.arange(4, device=device).view(-1, 1, 1)
    lq = torch.arange(4, device=device).view(1, -1, 1)
    r = torch.arange(4, device=device).view(1, 1, -1)
    return ((4 * (rb >> 1) + lq) * 8 + 4 * (rb & 1) + r).reshape(-1)


def _proj_row_perm_per_head(heads, LP, device):
    """Row m*36 + c of the per-head projection blocks of msm_msdeform_attn_enc_lp_fused_fwd = reference row m*2LP + c (offsets,
    c < 2LP) or heads*2LP + m*LP + c - 2LP (logits)."""
    m = torch.arange(heads, device=device).view(-1, 1)
    c = torch.arange(3 * LP, device=device).view(1, -1)
    return torch.where(c < 2 * LP, m * 2 * LP + c, heads * 2 * LP + m * LP + c - 2 * LP).reshape(-1)


def pack_encoder_block_hm(wo, w1, w2, wv=None, wp=None, ffn_f16=False):
    """One encoder layer's matrices as the weight stream of msm_encoder_block_hm_fwd (include/msm_hip.h): resident block
    [output_proj | next layer's value_proj] as [h, l] bf16 pairs, linear1 / linear2 as single bf16 copies -- ``ffn_f16``: as IEEE
    halves (precision "f16") --, four pairs of 16-wide hidden blocks per 32-KiB stage, then (wv / wp given) the next layer's
    sampling projection as [h, l] pairs, eight row blocks per stage.  Returns an int16 tensor (bit patterns)."""
    dev = wo.device
    d_ffn = w1.shape[0]
    if wo.shape != (64, 64) or w1.shape[1] != 64 or tuple(w2.shape) != (64, d_ffn) or d_ffn % 32:
        raise RuntimeError("pack_encoder_block_hm: d_model 64, d_ffn a multiple of 32")
    if (wv is None) != (wp is None) or (wp is not None and tuple(wp.shape) != (288, 64)):
        raise RuntimeError("pack_encoder_block_hm: wv and wp (288, 64) go together")
    pad = (-d_ffn) % 128
    kL = _korder_L(64, dev)
    res = [pair_hl(wo, _korder_natural(64, dev)).reshape(-1)]
    res.append(pair_hl(wv[_value_row_perm(dev)], kL).reshape(-1) if wv is not None else torch.zeros(16 * 512, device=dev))
    w1p = torch.cat([w1, torch.zeros(pad, 64, device=dev)], 0)
    w2p = torch.cat([w2, torch.zeros(64, pad, device=dev)], 1)
    npair = (d_ffn + pad) // 32
    b1 = _frag_blocks(w1p, kL).reshape(npair, 4 * 512)                        # [P][q][G][512]
    b2 = _frag_blocks(w2p, _korder_L(d_ffn + pad, dev)).permute(1, 0, 2).reshape(npair, 4 * 512)     # [P][ob][512]
    parts = [_bits(torch.cat(res)), _bits(torch.cat([b1, b2], 1).reshape(-1), torch.float16 if ffn_f16 else torch.bfloat16)]
    if wp is not None:
        pj = pair_hl(wp, kL).reshape(-1)                                      # 18 row blocks x 4 KiB
        parts.append(_bits(torch.cat([pj, torch.zeros(3 * 16384 - pj.numel(), device=dev)])))
    out = torch.cat(parts).contiguous()
    _expect("pack_encoder_block_hm", out.numel() * 2, lib().msm_encoder_block_hm_stream_bytes(d_ffn, int(wp is not None)))
    return out


def pack_encoder_block_hm_small(bo, g1, be1, b1, b2, g2, be2, bv=None, bp=None):
    """The fp32 parameter vector of msm_encoder_block_hm_fwd (value_proj biases in the packed row order, linear1 bias zero
    padded to whole stages)."""
    dev = bo.device
    d_ffn = b1.numel()
    bvp = bv[_value_row_perm(dev)] if bv is not None else torch.zeros(64, device=dev)
    bpp = bp if bp is not None else torch.zeros(288, device=dev)
    out = torch.cat([bo, g1, be1, b2, g2, be2, bvp, bpp, b1, torch.zeros((-d_ffn) % 128, device=dev)]).contiguous()
    _expect("pack_encoder_block_hm_small", out.numel(), lib().msm_encoder_block_hm_small_floats(d_ffn), "floats")
    return out


def pack_encoder_prologue_hm(wv, wp, bv, bp):
    """Layer 0's value_proj (64, 64) and [sampling_offsets | attention_weights] (288, 64) as the weight blocks and bias vector of
    msm_encoder_prologue_hm_fwd: the blocks of pack_encoder_block_hm, value first.  Returns (int16 blocks, float32 small)."""
    dev = wv.device
    if tuple(wv.shape) != (64, 64) or tuple(wp.shape) != (288, 64):
        raise RuntimeError("pack_encoder_prologue_hm: value_proj (64, 64) and a (288, 64) sampling projection")
    kL = _korder_L(64, dev)
    blocks = _bits(torch.cat([pair_hl(wv[_value_row_perm(dev)], kL).reshape(-1), pair_hl(wp, kL).reshape(-1)]))
    _expect("pack_encoder_prologue_hm", blocks.numel() * 2, lib().msm_encoder_prologue_hm_weight_bytes())
    small = torch.cat([bv[_value_row_perm(dev)], bp]).contiguous()
    return blocks, small


def pack_msda_proj_lp(wp, bp, heads=8, n_levels=3, n_points=4):
    """[sampling_offsets ; attention_weights] weight (heads*L*P*3, 64) and bias -> the per-head [h, l] bf16 fragment stream
    (int16, 12 KiB per head) and bias table (heads, 48) of msm_msdeform_attn_enc_lp_fused_fwd."""
    LP = n_levels * n_points
    if tuple(wp.shape) != (heads * LP * 3, 64) or bp.numel() != wp.shape[0] or LP != 12:
        raise RuntimeError("pack_msda_proj_lp: the shipped geometry only (3 levels x 4 points)")
    dev = wp.device
    perm = _proj_row_perm_per_head(heads, LP, dev)
    rows = torch.zeros(heads, 48, 64, device=dev)
    bias = torch.zeros(heads, 48, device=dev)
    rows[:, :3 * LP] = wp[perm].reshape(heads, 3 * LP, 64)
    bias[:, :3 * LP] = bp[perm].reshape(heads, 3 * LP)
    blocks = pair_hl(rows.reshape(heads * 48, 64), _korder_L(64, dev))        # (heads*3, 2, 2, 512)
    return _bits(blocks.reshape(-1)), bias.contiguous()


PROJ_REC_FLOATS = 30     # the bf16 plan's sampling projection: 120 bytes per (image, head, token) = 24 fp32 offsets + 12 fp16 logits, plane-major
                         # per (image, head) (csrc/enc_lp.hip, EH_REC); tensors are typed (B, 8, S, 30) float32 for their size only


def proj_to_head_major_records(proj, heads=8, LP=12):
    """(B, S, heads*LP*3) fp32 in the reference's [offsets | logits] column order -> the bf16 plan's sampling projection
    (B, heads, S, 30) float32-TYPED (120 bytes per token; NOT a (.., S, 30) array): per (image, head) six planes [S][4 floats] of fp32
    offsets then three planes [S][4 halves] of fp16 logits (csrc/enc_lp.hip, EH_REC).  Torch ops: tests and the unfused front end
    only; the fused prologue writes this layout itself."""
    B, S, W = proj.shape
    off = proj[..., :heads * 2 * LP].reshape(B, S, heads, 2 * LP // 4, 4).permute(0, 2, 3, 1, 4).reshape(B, heads, -1)          # (B, heads, 6 S 4)
    lg = proj[..., heads * 2 * LP:].reshape(B, S, heads, LP // 4, 4).permute(0, 2, 3, 1, 4).to(torch.float16).reshape(B, heads, -1)
    return torch.cat([off, lg.contiguous().view(torch.float32)], -1).view(B, heads, S, PROJ_REC_FLOATS).contiguous()


def proj_records_to_columns(rec, heads=8, LP=12):
    """Inverse of proj_to_head_major_records (the logits come back as the fp16 values the planes hold): (B, S, heads*LP*3) fp32."""
    B, M, S, _ = rec.shape
    flat = rec.reshape(B, M, S * PROJ_REC_FLOATS)
    off = flat[..., :S * 2 * LP].reshape(B, M, 2 * LP // 4, S, 4).permute(0, 3, 1, 2, 4).reshape(B, S, M * 2 * LP)
    lg = flat[..., S * 2 * LP:].contiguous().view(torch.float16).reshape(B, M, LP // 4, S, 4).permute(0, 3, 1, 2, 4).reshape(B, S, M * LP).float()
    return torch.cat([off, lg], -1).contiguous()
