"""Thin torch-tensor front end over the C ABI (include/msm_hip.h).

torch is used for device memory and streams only: every function checks its arguments, allocates
the outputs with torch.empty on the inputs' device and launches the HIP kernels of libmsm_hip.so
on torch's current stream.  Tensors must be fp32 and live on a ROCm device; there is no CPU path.
The weight layouts that need no launch (pack_encoder_block*, pack_conv_in_weight*, ...) are packing.py's, re-exported here.
"""
import ctypes
import warnings

import torch

from ._lib import check, lib
from .packing import (MASK_CONV_K, MASK_CONV_LD, PROJ_REC_FLOATS, dense_kv_constant, mask_conv_fold_weight, pack_conv_in_weight,  # noqa: F401
                      pack_conv_in_weight_lp, pack_encoder_block, pack_encoder_block_hm, pack_encoder_block_hm_small,
                      pack_encoder_block_lp, pack_encoder_block_split, pack_encoder_prologue, pack_encoder_prologue_hm,
                      pack_msda_proj_lp, proj_records_to_columns, proj_to_head_major_records)

KAPPA = 30.0  # attention_util.py:26


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """torch's current HIP stream of the current device as a void*.  torch.cuda.current_stream() costs ~8 us of Python
    per call (device-index resolution + a Stream object) -- a tenth of a small-batch forward; the raw accessor the
    public call itself ends in costs ~0.3 us."""
    if _raw_stream is not None and _cur_device is not None:
        return ctypes.c_void_p(_raw_stream(_cur_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _chk(t, name, dtype=torch.float32):
    if t is None:
        return
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be on the GPU (no CPU path in unseenobjectswithmeanshift_amd)")
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must be {dtype}, got {t.dtype}")


def _c(t, name, dtype=torch.float32):
    _chk(t, name, dtype)
    if t is not None and not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")
    return t


# ----------------------------------------------------------------------------------------------
def gemm(a, w, bias=None, *, a2=None, act=None, out=None, split_k=1):
    """out[..., n] = act((a + a2) @ w.T + bias) for row-major a (..., K) and w (N, K).
    split_k > 1 returns raw partial sums of shape (split_k, ..., N) (bias/act must be None, and so must out).
    out: an fp32 contiguous tensor of shape (..., N) on a's device to write into (a contiguous view at a storage offset is fine)."""
    _c(a, "a"), _c(w, "w"), _c(bias, "bias"), _c(a2, "a2")
    K = a.shape[-1]
    N = w.shape[0]
    M = a.numel() // K
    a2_sb = 0
    if a2 is not None:
        if a2.shape == a.shape:
            batch, Mb = 1, M
        else:
            # a2 broadcast over the leading batch dim of a: a (B, L, K), a2 (L, K)
            if a.dim() != 3 or tuple(a2.shape) != tuple(a.shape[1:]):
                raise RuntimeError("a2 must match a or a[0]")
            batch, Mb = a.shape[0], a.shape[1]
    else:
        batch, Mb = 1, M
    lead = a.shape[:-1]
    if split_k > 1:
        if bias is not None or act is not None:
            raise RuntimeError("split_k output is raw: bias/act are applied by the consumer")
        if out is not None:
            raise RuntimeError("split_k allocates its (split_k, ..., N) parts itself: out must be None")
        out = torch.empty((split_k,) + tuple(lead) + (N,), device=a.device, dtype=torch.float32)
    elif out is None:
        out = torch.empty(tuple(lead) + (N,), device=a.device, dtype=torch.float32)
    else:
        _c(out, "out")
        if out.device != a.device or tuple(out.shape) != tuple(lead) + (N,):
            raise RuntimeError(f"out must be {tuple(lead) + (N,)} on {a.device}, got {tuple(out.shape)} on {out.device}")
    rc = lib().msm_gemm_f32(_p(a), _p(a2), _p(w), _p(bias), _p(out), Mb, N, K, batch,
                            K, 1, Mb * K, a2_sb, 0, N, 1, Mb * N, M * N,
                            0, 0, 0, 0, 1 if bias is not None else 0, 1 if act == "relu" else 0,
                            split_k, _stream())
    check(rc, "msm_gemm_f32")
    return out


def conv1x1_nchw_to_tokens(x, w, bias=None):
    """x (B, Cin, H, W) NCHW -> tokens (B, H*W, Cout) = x^T w^T + bias (a 1x1 Conv2d read through
    the GEMM's M-contiguous A path; no transpose pass).  bias: (Cout,) per channel, or (H*W, Cout) a
    per-position matrix shared by the batch."""
    _c(x, "x"), _c(w, "w"), _c(bias, "bias")
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    HW = H * W
    out = torch.empty((B, HW, Cout), device=x.device, dtype=torch.float32)
    mode = 0 if bias is None else (1 if bias.dim() == 1 else 3)
    if mode == 3 and tuple(bias.shape) != (HW, Cout):
        raise RuntimeError("matrix bias must be (H*W, Cout)")
    rc = lib().msm_gemm_f32(_p(x), None, _p(w), _p(bias), _p(out), HW, Cout, Cin, B,
                            1, HW, Cin * HW, 0, 0, Cout, 1, HW * Cout, 0,
                            0, 0, 0, 0, mode, 0, 1, _stream())
    check(rc, "msm_gemm_f32(conv1x1 nchw)")
    return out


def conv1x1_in(x, w_packed, bias=None, *, out=None, stats=None, stats_cleared=False, lp=False):
    """Input projection of the pixel decoder: x (B, Cin, H, W) NCHW, w_packed = pack_conv_in_weight(w (64, Cin)) ->
    tokens (B, H*W, 64) = x^T w^T + bias  (``lp``: w_packed = pack_conv_in_weight_lp(w), hi + lo bf16 operands on the bf16
    matrix pipe, fp32 results; Cin a multiple of 256),
    plus the GroupNorm moments of the result.  ``out``: a (B, H*W, 64) view with unit channel stride, row stride 64 and
    any batch stride (e.g. ``buf[:, s:s + H*W]`` of the concatenated token buffer of the encoder); ``stats``: a
    (B, 64, 2) float64 tensor that receives (sum, sum of squares) per (image, channel) -- accumulated into when
    ``stats_cleared`` (the caller zeroed it), else zeroed first.  Returns (out, stats).  Cin must be a multiple of 128
    (conv1x1_nchw_to_tokens + groupnorm_stats cover other shapes)."""
    _c(x, "x"), _c(w_packed, "w_packed", torch.bfloat16 if lp else torch.float32), _c(bias, "bias"), _c(stats, "stats", torch.float64)
    B, Cin, H, W = x.shape
    HW = H * W
    if w_packed.numel() != (128 if lp else 64) * Cin or Cin % (256 if lp else 128) or HW % 4:
        raise RuntimeError("conv1x1_in needs a packed (64, Cin) weight, Cin a multiple of 128 (lp: 256) and H*W a multiple of 4")
    if out is None:
        out = torch.empty((B, HW, 64), device=x.device, dtype=torch.float32)
    _chk(out, "out")
    if tuple(out.shape) != (B, HW, 64) or out.stride(2) != 1 or out.stride(1) != 64 or (B > 1 and out.stride(0) < HW * 64):
        raise RuntimeError("out must be (B, H*W, 64) with strides (>= H*W*64, 64, 1)")
    if stats is None:
        stats = torch.empty((B, 64, 2), device=x.device, dtype=torch.float64)
        stats_cleared = False
    elif tuple(stats.shape) != (B, 64, 2):
        raise RuntimeError("stats must be (B, 64, 2) float64")
    fn = lib().msm_conv1x1_in_lp if lp else lib().msm_conv1x1_in_f32
    rc = fn(_p(x), _p(w_packed), _p(bias), _p(out), out.stride(0) if B > 1 else HW * 64, _p(stats), 1 if stats_cleared else 0, B, Cin, HW,
            _stream())
    check(rc, "msm_conv1x1_in_lp" if lp else "msm_conv1x1_in_f32")
    return out, stats


def conv1x1_in_multi(xs, ws_packed, biases, out, stats, stats_cleared=False, lp=False):
    """conv1x1_in for up to four levels in one launch (``lp``: ws_packed from pack_conv_in_weight_lp, the bf16 matrix pipe; ``lp="wide"``: the
    same arithmetic with the weight broadcast through LDS -- eight-wave workgroups over adjacent 64-pixel tiles x K slices, for batches that
    fill the chip that way (msm_conv1x1_in_multi_wide)).  xs: list of (B, Cin_l, H_l, W_l) NCHW maps (deepest Cin first),
    ws_packed / biases: per level (a bias may be None), out: (B, sum H_l*W_l, 64) token buffer or a token-range view of a larger
    one (level l fills its token range), stats: (L, B, 64, 2) float64 moments (accumulated into when ``stats_cleared``)."""
    L = len(xs)
    B = xs[0].shape[0]
    S = sum(x.shape[2] * x.shape[3] for x in xs)
    _chk(out, "out"), _c(stats, "stats", torch.float64)
    if tuple(out.shape) != (B, S, 64) or tuple(stats.shape) != (L, B, 64, 2) or out.stride(2) != 1 or out.stride(1) != 64 \
            or (B > 1 and out.stride(0) < S * 64):
        raise RuntimeError("conv1x1_in_multi: out must be (B, sum HW, 64) with strides (>= sum HW * 64, 64, 1) and stats (L, B, 64, 2)")
    for x, w, b in zip(xs, ws_packed, biases):
        _c(x, "x"), _c(w, "w_packed", torch.bfloat16 if lp else torch.float32), _c(b, "bias")
        if x.shape[0] != B or w.numel() != (128 if lp else 64) * x.shape[1]:
            raise RuntimeError("conv1x1_in_multi: inconsistent level shapes")
    vp = ctypes.c_void_p * L
    ia = ctypes.c_int32 * L
    xa, wa = vp(*[x.data_ptr() for x in xs]), vp(*[w.data_ptr() for w in ws_packed])
    ba = vp(*[0 if b is None else b.data_ptr() for b in biases])
    cin, hw = ia(*[x.shape[1] for x in xs]), ia(*[x.shape[2] * x.shape[3] for x in xs])
    name = "msm_conv1x1_in_multi_wide" if lp == "wide" else "msm_conv1x1_in_multi_lp" if lp else "msm_conv1x1_in_multi_f32"
    fn = getattr(lib(), name)
    rc = fn(L, ctypes.cast(xa, ctypes.c_void_p), ctypes.cast(wa, ctypes.c_void_p), ctypes.cast(ba, ctypes.c_void_p),
            ctypes.cast(cin, ctypes.c_void_p), ctypes.cast(hw, ctypes.c_void_p), _p(out), out.stride(0) if B > 1 else S * 64, _p(stats),
            1 if stats_cleared else 0, B, _stream())
    check(rc, name)
    return out, stats


def is_token_major(x):
    """True for a (B, C, H, W) tensor stored [B][H*W][C] (torch channels_last, possibly with a larger batch stride),
    e.g. the NCHW-shaped views the pixel decoder returns over its token buffer."""
    if x.dim() != 4:
        return False
    B, C, H, W = x.shape
    return x.stride(1) == 1 and x.stride(3) == C and x.stride(2) == W * C and x.stride(0) >= H * W * C and C > 1


def kv_project(x, w, cmat, cmat_width=0):
    """Folded K/V projection: x (B, 64, H, W), w (N, 64), cmat (H*W, N) -> (B, H*W, N).
    x is contiguous NCHW or token-major (is_token_major).  Maps with N in {256, 512} take the weight-stationary
    kernel (csrc/kv_proj.hip); small NCHW ones, where copying w into every CU's LDS costs more than it saves, and
    other shapes take the tiled GEMM.  ``cmat_width`` = W: the constant is separable, cmat = (H + W, N) holds H row vectors then
    W column vectors and token (y, x) gets row[y] + col[x] (include/msm_hip.h)."""
    _chk(x, "x"), _c(w, "w"), _c(cmat, "cmat")
    B, C, H, W = x.shape
    N = w.shape[0]
    if cmat_width and (cmat_width != W or tuple(cmat.shape) != (H + W, N)):
        raise RuntimeError(f"kv_project: a separable constant must be ({H + W}, N) with cmat_width = {W}")
    tokens = is_token_major(x) and not x.is_contiguous()
    if not tokens:
        _c(x, "x")
    if C != 64 or N not in (256, 512) or (not tokens and B * H * W < 8192):
        return conv1x1_nchw_to_tokens(x.contiguous(), w, dense_kv_constant(cmat, cmat_width))
    if tuple(w.shape) != (N, C) or (not cmat_width and tuple(cmat.shape) != (H * W, N)):
        raise RuntimeError(f"kv_project: w must be (N, {C}) and cmat ({H * W}, N)")
    out = torch.empty((B, H * W, N), device=x.device, dtype=torch.float32)
    rc = lib().msm_kv_project_f32(_p(x), _p(w), _p(cmat), _p(out), B, C, H * W, N, 1 if tokens else 0, x.stride(0), int(cmat_width), _stream())
    check(rc, "msm_kv_project_f32")
    return out


def conv1x1_tokens_to_nchw(t, w, bias=None):
    """tokens (B, HW, Cin) -> (B, Cout, HW) with the weight as the MFMA A operand so that the
    NCHW output rows are written contiguously (bias is per output row)."""
    _c(t, "t"), _c(w, "w"), _c(bias, "bias")
    B, HW, Cin = t.shape
    Cout = w.shape[0]
    out = torch.empty((B, Cout, HW), device=t.device, dtype=torch.float32)
    # A = w (M=Cout, shared over batch), "W" = tokens of image b ([N=HW][K=Cin])
    rc = lib().msm_gemm_f32(_p(w), None, _p(t), _p(bias), _p(out), Cout, HW, Cin, B,
                            Cin, 1, 0, 0, HW * Cin, HW, 1, Cout * HW, 0,
                            0, 0, 0, 0, 2 if bias is not None else 0, 0, 1, _stream())
    check(rc, "msm_gemm_f32(conv1x1 to nchw)")
    return out


def conv3x3_tokens(t, w_tap_major, H, W):
    """3x3 / pad 1 convolution over an NHWC token map t (B, H*W, Cin) with weights permuted to
    (Cout, 9*Cin) tap-major; returns (B, H*W, Cout).  No bias (the reference layer has a norm)."""
    _c(t, "t"), _c(w_tap_major, "w")
    B, HW, Cin = t.shape
    Cout = w_tap_major.shape[0]
    out = torch.empty((B, HW, Cout), device=t.device, dtype=torch.float32)
    rc = lib().msm_gemm_f32(_p(t), None, _p(w_tap_major), None, _p(out), HW, Cout, 9 * Cin, B,
                            Cin, 1, HW * Cin, 0, 0, Cout, 1, HW * Cout, 0,
                            2, H, W, Cin, 0, 0, 1, _stream())
    check(rc, "msm_gemm_f32(conv3x3)")
    return out


def conv3x3_c64(t, w_tap_major, H, W, *, stats=None, stats_cleared=False, bf16=False, split=False):
    """3x3 / pad 1 convolution of a 64-channel token map t (B, H*W, 64) to 64 channels, weight (64, 9*64) tap-major, with
    the GroupNorm moments of the result as a by-product: returns (out (B, H*W, 64), stats (B, 64, 2) float64).  ``stats``
    given: accumulated into when ``stats_cleared`` (the caller zeroed it), else zeroed first.  ``bf16``: the low-precision
    mode (bf16 MFMA operands -- weight single, activations hi + lo --, fp32 accumulation and output); ``bf16="f16"``: IEEE-half
    operands, one term each (precision "f16").  ``split``: t is the
    (3, B, H*W, 64) bf16 planes of groupnorm_tokens(split_planes=True); fp32-accurate results from six bf16 MFMAs per product.
    A float16 ``t`` (groupnorm_tokens(out_f16=True)) is the "f16" form on operands already rounded: the same output bits, the kernel
    that keeps a unit's loads in flight at once (msm_conv3x3_c64_f16h)."""
    half_in = t.dtype == torch.float16
    if half_in and (split or bf16 != "f16"):
        raise RuntimeError("conv3x3_c64: a float16 map is the input of the bf16=\"f16\" form only")
    if split:
        _c(t, "t", torch.bfloat16)
        if t.dim() != 4 or t.shape[0] != 3:
            raise RuntimeError("conv3x3_c64(split=True) needs the (3, B, H*W, 64) bf16 planes")
        _, B, HW, C = t.shape
    else:
        _c(t, "t", torch.float16 if half_in else torch.float32)
        B, HW, C = t.shape
    _c(w_tap_major, "w"), _c(stats, "stats", torch.float64)
    if C != 64 or tuple(w_tap_major.shape) != (64, 576) or HW != H * W:
        raise RuntimeError("conv3x3_c64 needs a (B, H*W, 64) map and a (64, 576) tap-major weight")
    out = torch.empty((B, HW, C), device=t.device, dtype=torch.float32)
    if stats is None:
        stats = torch.empty((B, 64, 2), device=t.device, dtype=torch.float64)
        stats_cleared = False
    elif tuple(stats.shape) != (B, 64, 2):
        raise RuntimeError("stats must be (B, 64, 2) float64")
    name = "msm_conv3x3_c64_split" if split else "msm_conv3x3_c64_f16h" if half_in else ("msm_conv3x3_c64_f16" if bf16 == "f16" else "msm_conv3x3_c64_bf16" if bf16 else "msm_conv3x3_c64_f32")
    rc = getattr(lib(), name)(_p(t), _p(w_tap_major), _p(out), _p(stats), 1 if stats_cleared else 0, B, H, W, _stream())
    check(rc, name)
    return out, stats


def conv3x3_tokens_to_nchw(t, w_tap_major, bias, H, W, bf16=False):
    """3x3 / pad 1 convolution of an NHWC token map with the output written directly as NCHW (B, Cout, H*W)
    (SimpleBasePixelDecoder.mask_features, fpn.py:237-246: Conv2d 3x3 with bias).  64 input channels, Cout % 64 == 0 and
    W % 4 == 0 take the weight-stationary kernel (csrc/conv3x3.hip), other shapes the implicit GEMM.  ``bf16`` (low-precision
    mode, weight-stationary shapes only): the weight rounded to one bf16, activations as hi + lo operands, fp32 result;
    ``bf16="f16"``: IEEE-half operands, one term each."""
    _c(t, "t"), _c(w_tap_major, "w"), _c(bias, "bias")
    B, HW, Cin = t.shape
    Cout = w_tap_major.shape[0]
    out = torch.empty((B, Cout, HW), device=t.device, dtype=torch.float32)
    if Cin == 64 and Cout % 64 == 0 and Cout <= 1024 and W % 4 == 0 and HW == H * W:
        name = "msm_conv3x3_c64_nchw_f16" if bf16 == "f16" else "msm_conv3x3_c64_nchw_bf16" if bf16 else "msm_conv3x3_c64_nchw_f32"
        rc = getattr(lib(), name)(_p(t), _p(w_tap_major), _p(bias), _p(out), B, H, W, Cout, _stream())
        check(rc, name)
        return out
    rc = lib().msm_gemm_f32(_p(t), None, _p(w_tap_major), _p(bias), _p(out), HW, Cout, 9 * Cin, B,
                            Cin, 1, HW * Cin, 0, 0, 1, HW, Cout * HW, 0,
                            2, H, W, Cin, 1 if bias is not None else 0, 0, 1, _stream())
    check(rc, "msm_gemm_f32(conv3x3 -> nchw)")
    return out


def conv3x3_weight_grad(tok, gout, H, W, *, splits=None, want_bias=True):
    """Weight and bias gradient of the 3x3 / pad 1 convolution of a 64-channel token map (the backward of conv3x3_tokens_to_nchw
    with respect to its weight and bias; csrc/conv3x3_bwd.hip): tok (B, H*W, 64) the forward's input, gout (B, Cout, H, W) or
    (B, Cout, H*W) the gradient of its NCHW output, Cout a multiple of 64 up to 1024, any H, W.  Returns (dw (Cout, 576) tap-major,
    dbias (Cout,) or None when not ``want_bias``).  ``splits``: the number of pixel ranges whose partial sums are added in a
    second launch (None: chosen by shape); the result is bit-identical from call to call for a given (shape, splits)."""
    _c(tok, "tok"), _c(gout, "gout")
    if tok.dim() != 3 or gout.dim() not in (3, 4):
        raise RuntimeError("conv3x3_weight_grad needs tok (B, H*W, 64) and gout (B, Cout, H, W)")
    B, HW, C = tok.shape
    Cout = gout.shape[1]
    if C != 64 or HW != H * W or gout.shape[0] != B or gout.numel() != B * Cout * HW:
        raise RuntimeError("conv3x3_weight_grad needs tok (B, H*W, 64) and gout (B, Cout, H, W)")
    splits = 0 if splits is None else int(splits)
    if splits < 0:
        raise RuntimeError("conv3x3_weight_grad: splits must be None or >= 1")
    n = lib().msm_conv3x3_c64_wgrad_workspace(B, H, W, Cout, splits)
    if n < 0:
        check(int(n), "msm_conv3x3_c64_wgrad_workspace")
    ws = torch.empty((n,), device=tok.device, dtype=torch.float32)
    dw = torch.empty((Cout, 9 * C), device=tok.device, dtype=torch.float32)
    db = torch.empty((Cout,), device=tok.device, dtype=torch.float32) if want_bias else None
    rc = lib().msm_conv3x3_c64_wgrad(_p(tok), _p(gout), _p(dw), _p(db), _p(ws), B, H, W, Cout, splits, _stream())
    check(rc, "msm_conv3x3_c64_wgrad")
    return dw, db


def conv3x3_input_grad(gout, w, H, W):
    """Input gradient of the 3x3 / pad 1 convolution y = conv2d(x, w, padding=1): gout (B, Cout, H, W) the gradient of y, w the
    parameter (Cout, Cin, 3, 3) -> (B, Cin, H, W).  It is the convolution of gout with the mirrored taps,
    w'[c][(dy*3 + dx)*Cout + o] = w[o][c][2 - dy][2 - dx]: gout transposed once to tokens (msm_transpose_f32), the weight rearranged on
    the device, then the implicit-GEMM mode of msm_gemm_f32 writing NCHW planes."""
    _c(gout, "gout"), _chk(w, "w")
    if gout.dim() != 4 or w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or w.shape[0] != gout.shape[1] or tuple(gout.shape[2:]) != (H, W):
        raise RuntimeError("conv3x3_input_grad needs gout (B, Cout, H, W) and w (Cout, Cin, 3, 3)")
    B, Cout = gout.shape[:2]
    Cin = w.shape[1]
    HW = H * W
    if Cout % 4:
        raise RuntimeError("conv3x3_input_grad needs Cout a multiple of 4")
    gtok = transpose_last2(gout.view(B, Cout, HW))                                          # (B, HW, Cout)
    wm = w.flip(2, 3).permute(1, 2, 3, 0).reshape(Cin, 9 * Cout).contiguous()
    out = torch.empty((B, Cin, HW), device=gout.device, dtype=torch.float32)
    rc = lib().msm_gemm_f32(_p(gtok), None, _p(wm), None, _p(out), HW, Cin, 9 * Cout, B,
                            Cout, 1, HW * Cout, 0, 0, 1, HW, Cin * HW, 0,
                            2, H, W, Cout, 0, 0, 1, _stream())
    check(rc, "msm_gemm_f32(conv3x3 input gradient)")
    return out.view(B, Cin, H, W)


def conv3x3_input_grad_tokens(gtok, w, H, W):
    """conv3x3_input_grad on token maps: gtok (B, H*W, Cout) the gradient of the token output of conv3x3_c64 / conv3x3_tokens, w the
    parameter (Cout, Cin, 3, 3) -> (B, H*W, Cin).  The same implicit GEMM on the mirrored taps, reading and writing tokens: no
    transposes."""
    _c(gtok, "gtok"), _chk(w, "w")
    if gtok.dim() != 3 or w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or w.shape[0] != gtok.shape[2] or gtok.shape[1] != H * W:
        raise RuntimeError("conv3x3_input_grad_tokens needs gtok (B, H*W, Cout) and w (Cout, Cin, 3, 3)")
    B, HW, Cout = gtok.shape
    Cin = w.shape[1]
    if Cout % 4:
        raise RuntimeError("conv3x3_input_grad_tokens needs Cout a multiple of 4")
    wm = w.flip(2, 3).permute(1, 2, 3, 0).reshape(Cin, 9 * Cout).contiguous()
    out = torch.empty((B, HW, Cin), device=gtok.device, dtype=torch.float32)
    rc = lib().msm_gemm_f32(_p(gtok), None, _p(wm), None, _p(out), HW, Cin, 9 * Cout, B,
                            Cout, 1, HW * Cout, 0, 0, Cin, 1, HW * Cin, 0,
                            2, H, W, Cout, 0, 0, 1, _stream())
    check(rc, "msm_gemm_f32(conv3x3 input gradient, tokens)")
    return out


def groupnorm_backward(x, gout, stats, gamma, beta, groups=32, *, eps=1e-5, relu=False, splits=None, want_dx=True, want_dgamma=True,
                       want_dbeta=True):
    """Backward of groupnorm_tokens (csrc/norm_bwd.hip): x, gout (B, HW, C), stats (B, C, 2) float64 the forward's moments
    (groupnorm_stats(x)), gamma, beta (C,); ``relu``: the forward applied a ReLU (the mask y > 0 is recomputed, nothing is stored).
    Returns (dx (B, HW, C), dgamma (C,), dbeta (C,)), None for each one not wanted.  C a multiple of 4 and of ``groups``, at most 256.
    ``splits``: the number of pixel ranges per image whose partial sums are added in index order (None: ranges of 256 pixels); the
    result is bit-identical from call to call for a given (shape, splits)."""
    _c(x, "x"), _c(gout, "gout"), _c(stats, "stats", torch.float64), _c(gamma, "gamma"), _c(beta, "beta")
    if x.dim() != 3 or gout.shape != x.shape:
        raise RuntimeError("groupnorm_backward needs x and gout (B, HW, C)")
    B, HW, C = x.shape
    groups = int(groups)
    if tuple(stats.shape) != (B, C, 2) or tuple(gamma.shape) != (C,) or tuple(beta.shape) != (C,):
        raise RuntimeError("groupnorm_backward needs stats (B, C, 2) float64 and gamma, beta (C,)")
    if groups < 1 or C % groups or C % 4 or C > 256:
        raise RuntimeError(f"groupnorm_backward needs C a multiple of 4 and of groups, at most 256 (C={C}, groups={groups})")
    splits = 0 if splits is None else int(splits)
    if splits < 0:
        raise RuntimeError("groupnorm_backward: splits must be None or >= 1")
    n = lib().msm_groupnorm_bwd_workspace(B, HW, C, groups, splits)
    if n < 0:
        check(int(n), "msm_groupnorm_bwd_workspace")
    ws = torch.empty((n,), device=x.device, dtype=torch.float32)
    dx = torch.empty_like(x) if want_dx else None
    dg = torch.empty((C,), device=x.device, dtype=torch.float32) if want_dgamma else None
    db = torch.empty((C,), device=x.device, dtype=torch.float32) if want_dbeta else None
    rc = lib().msm_groupnorm_bwd_f32(_p(x), _p(gout), _p(stats), _p(gamma), _p(beta), _p(dx), _p(dg), _p(db), _p(ws), B, HW, C, groups,
                                     float(eps), 1 if relu else 0, splits, _stream())
    check(rc, "msm_groupnorm_bwd_f32")
    return dx, dg, db


def upsample_bilinear(x, hw, HW):
    """F.interpolate(size=HW, mode="bilinear", align_corners=False) of a token map x (B, h*w, C) -> (B, H*W, C): the fused add of
    groupnorm_tokens(up=...) as an operator of its own, same arithmetic (csrc/norm_bwd.hip).  x dense or a token-range slice of a larger
    buffer (row stride C, any batch stride); C a multiple of 4."""
    _chk(x, "x")
    (h, w), (H, W) = (int(hw[0]), int(hw[1])), (int(HW[0]), int(HW[1]))
    if x.dim() != 3 or x.shape[1] != h * w or min(h, w, H, W) < 1 or x.shape[2] % 4:
        raise RuntimeError("upsample_bilinear needs x (B, h*w, C) with C a multiple of 4 and h, w, H, W >= 1")
    B, _, C = x.shape
    if x.stride(2) != 1 or x.stride(1) != C or (B > 1 and x.stride(0) < h * w * C):
        raise RuntimeError("upsample_bilinear: x must have strides (>= h*w*C, C, 1)")
    out = torch.empty((B, H * W, C), device=x.device, dtype=torch.float32)
    rc = lib().msm_upsample_bilinear_tokens_f32(_p(x), x.stride(0) if B > 1 else 0, _p(out), B, h, w, H, W, C, _stream())
    check(rc, "msm_upsample_bilinear_tokens_f32")
    return out


def upsample_bilinear_backward(gout, hw, HW):
    """Adjoint of the bilinear token-map upsampling (csrc/norm_bwd.hip): gout (B, H*W, C) -> (B, h*w, C), C a multiple of 4.  Gather
    form, no atomics: bit-identical from call to call."""
    _c(gout, "gout")
    (h, w), (H, W) = (int(hw[0]), int(hw[1])), (int(HW[0]), int(HW[1]))
    if gout.dim() != 3 or gout.shape[1] != H * W or min(h, w, H, W) < 1 or gout.shape[2] % 4:
        raise RuntimeError("upsample_bilinear_backward needs gout (B, H*W, C) with C a multiple of 4 and h, w, H, W >= 1")
    B, _, C = gout.shape
    gin = torch.empty((B, h * w, C), device=gout.device, dtype=torch.float32)
    check(lib().msm_upsample_bilinear_bwd_tokens_f32(_p(gout), _p(gin), B, h, w, H, W, C, _stream()), "msm_upsample_bilinear_bwd_tokens_f32")
    return gin


def layernorm(x, g1, b1, *, parts=None, bias=None, l2norm=False, g2=None, b2=None, eps=1e-5):
    """LayerNorm(x + sum(parts) + bias) [-> unit length] [-> second LayerNorm].  Returns y or (y, y2)."""
    _c(x, "x"), _c(parts, "parts"), _c(bias, "bias"), _c(g1, "g1"), _c(b1, "b1"), _c(g2, "g2"), _c(b2, "b2")
    ref = x if x is not None else parts[0]
    E = ref.shape[-1]
    rows = ref.numel() // E
    y = torch.empty_like(ref)
    y2 = torch.empty_like(ref) if g2 is not None else None
    n_parts = 0 if parts is None else parts.shape[0]
    rc = lib().msm_layernorm_f32(_p(x), _p(parts), n_parts, rows * E, _p(bias), _p(g1), _p(b1),
                                 1 if l2norm else 0, _p(g2), _p(b2), _p(y), _p(y2), rows, E, eps, _stream())
    check(rc, "msm_layernorm_f32")
    return (y, y2) if g2 is not None else y


def groupnorm_tokens(x, gamma, beta, H, W, groups=32, *, up=None, up_hw=None, relu=False, eps=1e-5, stats=None, stats_ready=False,
                     split_planes=False, out_f16=False):
    """GroupNorm over an NHWC token map x (B, H*W, C); optionally adds the bilinear upsample of `up` (B, uh*uw, C) -- dense
    or a token-range slice of a larger buffer (row stride C, any batch stride) -- and applies ReLU.  ``stats``: a zeroed
    (B, C, 2) float64 scratch to accumulate the moments in (saves the fill launch) -- or, with ``stats_ready``, the finished
    moments of x (the producer of x accumulated them: no moments pass).  ``split_planes``: the result as three bf16 planes
    (3, B, H*W, C) with y = h + m + l exactly (the activation operand of conv3x3_c64(split=...)) instead of fp32.  ``out_f16``: the
    result as (B, H*W, C) float16, clamped to the half range (the operand conv3x3_c64(bf16="f16") rounds to, written once)."""
    if split_planes and out_f16:
        raise RuntimeError("groupnorm_tokens: split_planes and out_f16 are different output forms")
    _c(x, "x"), _c(gamma, "gamma"), _c(beta, "beta"), _chk(up, "up")
    B, HW, C = x.shape
    if stats_ready:
        _c(stats, "stats", torch.float64)
        if stats is None or tuple(stats.shape) != (B, C, 2):
            raise RuntimeError("stats_ready needs stats (B, C, 2) float64")
    else:
        stats = groupnorm_stats(x, stats)
    y = torch.empty((3,) + tuple(x.shape), device=x.device, dtype=torch.bfloat16) if split_planes else \
        torch.empty(x.shape, device=x.device, dtype=torch.float16) if out_f16 else torch.empty_like(x)
    uh, uw = (0, 0) if up is None else up_hw
    usb = 0
    if up is not None:
        if tuple(up.shape) != (B, uh * uw, C) or up.stride(2) != 1 or up.stride(1) != C or (B > 1 and up.stride(0) < uh * uw * C):
            raise RuntimeError("up must be (B, uh*uw, C) with strides (>= uh*uw*C, C, 1)")
        usb = up.stride(0) if B > 1 else 0
    name = "msm_groupnorm_apply_split" if split_planes else "msm_groupnorm_apply_f16" if out_f16 else "msm_groupnorm_apply_f32"
    rc = getattr(lib(), name)(_p(x), _p(stats), _p(gamma), _p(beta), _p(up), uh, uw, usb, _p(y), B, H, W, C, groups, eps, 1 if relu else 0, _stream())
    check(rc, name)
    return y


def groupnorm_nchw(x, stats, gamma, beta, *, groups=32, eps=1e-5, relu=False):
    """GroupNorm (+ReLU) of a token map x (B, HW, C) from its moments ``stats`` (B, C, 2) float64, written as NCHW planes
    (B, C, HW): the activation the folded mask step contracts with.  C <= 128, HW % 4 == 0."""
    _c(x, "x"), _c(stats, "stats", torch.float64), _c(gamma, "gamma"), _c(beta, "beta")
    B, HW, C = x.shape
    y = torch.empty((B, C, HW), device=x.device, dtype=torch.float32)
    rc = lib().msm_groupnorm_apply_nchw_f32(_p(x), _p(stats), _p(gamma), _p(beta), _p(y), B, HW, C, int(groups), float(eps),
                                            1 if relu else 0, _stream())
    check(rc, "msm_groupnorm_apply_nchw_f32")
    return y


def groupnorm_nchw_pool(x, stats, gamma, beta, H, W, sizes, *, groups=32, eps=1e-5, relu=False, zero_rows=0):
    """groupnorm_nchw of a 64-channel token map x (B, H*W, 64) and pool_mask_taps of the result in one launch
    (msm_groupnorm_nchw_pool_f32; W % 4 == 0): -> (act (B, 64, H, W), [pooled (B, th*tw, 64) per (th, tw) of ``sizes``],
    flags).  ``flags``: a cleared (B, zero_rows) int32 buffer, None when zero_rows == 0.  Bit-equal to the two launches."""
    _c(x, "x"), _c(stats, "stats", torch.float64), _c(gamma, "gamma"), _c(beta, "beta")
    B, HW, C = x.shape
    if C != 64 or HW != H * W or not 1 <= len(sizes) <= 4:
        raise RuntimeError("groupnorm_nchw_pool needs a (B, H*W, 64) token map and 1..4 target sizes")
    y = torch.empty((B, C, H, W), device=x.device, dtype=torch.float32)
    outs = [torch.empty((B, int(th) * int(tw), 64), device=x.device, dtype=torch.float32) for th, tw in sizes]
    n = len(sizes)
    ths = (ctypes.c_int32 * n)(*[int(s[0]) for s in sizes])
    tws = (ctypes.c_int32 * n)(*[int(s[1]) for s in sizes])
    ptrs = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
    flags = torch.empty((B, int(zero_rows)), device=x.device, dtype=torch.int32) if zero_rows else None
    rc = lib().msm_groupnorm_nchw_pool_f32(_p(x), _p(stats), _p(gamma), _p(beta), _p(y), B, int(H), int(W), C, int(groups), float(eps),
                                           1 if relu else 0, n, ctypes.cast(ths, ctypes.c_void_p), ctypes.cast(tws, ctypes.c_void_p),
                                           ctypes.cast(ptrs, ctypes.c_void_p), _p(flags), B * int(zero_rows), _stream())
    check(rc, "msm_groupnorm_nchw_pool_f32")
    return y, outs, flags


def groupnorm_stats(x, stats=None):
    """Per-(image, channel) double (sum, sum of squares) of a token map x (B, HW, C) -> (B, C, 2) float64.  ``stats``: a
    ZEROED (B, C, 2) float64 tensor to accumulate into (then no fill launch is issued)."""
    _c(x, "x"), _c(stats, "stats", torch.float64)
    B, HW, C = x.shape
    cleared = stats is not None
    if stats is None:
        stats = torch.empty((B, C, 2), device=x.device, dtype=torch.float64)
    elif tuple(stats.shape) != (B, C, 2):
        raise RuntimeError("stats must be (B, C, 2) float64")
    check(lib().msm_groupnorm_stats_f32(_p(x), _p(stats), 1 if cleared else 0, B, HW, C, _stream()), "msm_groupnorm_stats_f32")
    return stats


def tokens_proj_nchw(x, w, bias=None, *, gn=None, relu=False):
    """1x1 convolution from tokens x (B, HW, 64) to NCHW (B, N, HW) with an optional GroupNorm (+ReLU) applied to x on
    the fly: gn = (stats from groupnorm_stats(x), gamma, beta, groups, eps).  N in {256, 512}; other shapes use
    conv1x1_tokens_to_nchw on a materialised GroupNorm output."""
    _c(x, "x"), _c(w, "w"), _c(bias, "bias")
    B, HW, C = x.shape
    N = w.shape[0]
    stats = gamma = beta = None
    groups, eps = 1, 0.0
    if gn is not None:
        stats, gamma, beta, groups, eps = gn
        _c(stats, "stats", torch.float64), _c(gamma, "gamma"), _c(beta, "beta")
    out = torch.empty((B, N, HW), device=x.device, dtype=torch.float32)
    rc = lib().msm_tokens_proj_nchw_f32(_p(x), _p(w), _p(bias), _p(stats), _p(gamma), _p(beta), int(groups), float(eps),
                                        1 if relu else 0, _p(out), B, C, HW, N, _stream())
    check(rc, "msm_tokens_proj_nchw_f32")
    return out


def pos_embed_sine(H, W, num_pos_feats, device, *, layout="nchw", add_c=None, temperature=10000.0,
                   scale=6.283185307179586):
    """PositionEmbeddingSine(normalize=True) for one map: (2N, H, W) for layout 'nchw',
    (H*W, 2N) for 'tokens' (optionally with a per-channel vector added)."""
    C = 2 * num_pos_feats
    _c(add_c, "add_c")
    if layout == "nchw":
        out = torch.empty((C, H, W), device=device, dtype=torch.float32)
        s_c, s_p = H * W, 1
    else:
        out = torch.empty((H * W, C), device=device, dtype=torch.float32)
        s_c, s_p = 1, C
    rc = lib().msm_pos_embed_sine(_p(out), H, W, num_pos_feats, s_c, s_p, _p(add_c), temperature, scale, _stream())
    check(rc, "msm_pos_embed_sine")
    return out


def transpose_last2(x):
    """(B, R, C) -> (B, C, R)"""
    _c(x, "x")
    B, R, C = x.shape
    out = torch.empty((B, C, R), device=x.device, dtype=torch.float32)
    check(lib().msm_transpose_f32(_p(x), _p(out), B, R, C, _stream()), "msm_transpose_f32")
    return out


def l2_normalize_nchw(x, eps=1e-12):
    """F.normalize(x, p=2, dim=1) for an NCHW map (B, C, H, W) (msm_l2_normalize_nchw_f32)."""
    _c(x, "x")
    B, C, H, W = x.shape
    y = torch.empty_like(x)
    check(lib().msm_l2_normalize_nchw_f32(_p(x), _p(y), B, C, H * W, float(eps), _stream()), "msm_l2_normalize_nchw_f32")
    return y


def msda_locations(offsets, logits, reference_points, spatial_shapes):
    """The glue of the general MSDeformAttn.forward (ms_deform_attn.py:101-109): offsets (N,Lq,M,L,P,2), logits (N,Lq,M,L*P),
    reference_points (N,Lq,L,2), spatial_shapes (L,2) int64 -> (sampling_locations (N,Lq,M,L,P,2), attention_weights (N,Lq,M,L,P))."""
    _c(offsets, "offsets"), _c(logits, "logits"), _c(reference_points, "reference_points"), _c(spatial_shapes, "spatial_shapes", torch.int64)
    N, Lq, M, L, P, _ = offsets.shape
    if tuple(logits.shape) != (N, Lq, M, L * P) or tuple(reference_points.shape) != (N, Lq, L, 2):
        raise RuntimeError("msda_locations: logits must be (N,Lq,M,L*P) and reference_points (N,Lq,L,2)")
    loc = torch.empty_like(offsets)
    attn = torch.empty((N, Lq, M, L, P), device=offsets.device, dtype=torch.float32)
    check(lib().msm_msda_locations(_p(offsets), _p(logits), _p(reference_points), _p(spatial_shapes), _p(loc), _p(attn), N * Lq, M, L, P,
                                   _stream()), "msm_msda_locations")
    return loc, attn


def pack_mask_features_bf16(mask_features, f16=False):
    """fp32 NCHW (B, C, H, W) -> the channel-quad packed bf16 layout (B, C/4, H*W, 4) (int16 bit patterns) the bf16 mask
    step streams; do it once per forward, the 10 mask steps of a decoder pass reuse it.  ``f16`` (precision "f16"): IEEE-half
    elements, returned as a torch.float16 tensor -- mask_logits(packed_bf16=...) picks the fp16 MFMAs by that dtype."""
    _c(mask_features, "mask_features")
    B, C, H, W = mask_features.shape
    out = torch.empty((B, C // 4, H * W, 4), device=mask_features.device, dtype=torch.float16 if f16 else torch.int16)
    name = "msm_pack_mask_features_f16" if f16 else "msm_pack_mask_features_bf16"
    rc = getattr(lib(), name)(_p(mask_features), _p(out), B, C, H * W, _stream())
    check(rc, name)
    return out


def pack_mask_features_split(mask_features):
    """fp32 NCHW (B, 64, H, W) -> the exact three-term bf16 split (B, 3, 8, H*W, 8) (int16 bit patterns) of the fp32-accurate
    mask step on the bf16 matrix pipe (msm_mask_logits_split_fwd); once per forward."""
    _c(mask_features, "mask_features")
    B, C, H, W = mask_features.shape
    out = torch.empty((B, 3, C // 8, H * W, 8), device=mask_features.device, dtype=torch.int16)
    check(lib().msm_pack_mask_features_split(_p(mask_features), _p(out), B, C, H * W, _stream()), "msm_pack_mask_features_split")
    return out


def pool_mask_taps(act, sizes, zero_rows=0):
    """The 64-channel factored mask features act (B, 64, H, W) reduced bilinearly (align_corners=False) to each (th, tw) of
    ``sizes`` (H / th = W / tw in {2, 4, 8}: the mean of the four centre taps of every cell) -> list of token-major
    (B, th*tw, 64) tensors.  One launch (csrc/attn_mask.hip).  ``zero_rows`` = Q > 0: the same launch also clears a (B, Q) int32
    buffer (the row flags of the first attn_mask_pooled call), returned as a second result."""
    _c(act, "act")
    B, C, H, W = act.shape
    if C != 64 or not 1 <= len(sizes) <= 4:
        raise RuntimeError("pool_mask_taps needs a (B, 64, H, W) activation and 1..4 target sizes")
    outs = [torch.empty((B, int(th) * int(tw), 64), device=act.device, dtype=torch.float32) for th, tw in sizes]
    n = len(sizes)
    ths = (ctypes.c_int32 * n)(*[int(s[0]) for s in sizes])
    tws = (ctypes.c_int32 * n)(*[int(s[1]) for s in sizes])
    ptrs = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
    flags = torch.empty((B, int(zero_rows)), device=act.device, dtype=torch.int32) if zero_rows else None
    rc = lib().msm_pool_mask_taps(_p(act), B, H, W, n, ctypes.cast(ths, ctypes.c_void_p), ctypes.cast(tws, ctypes.c_void_p),
                                  ctypes.cast(ptrs, ctypes.c_void_p), _p(flags), B * int(zero_rows), _stream())
    check(rc, "msm_pool_mask_taps")
    return (outs, flags) if zero_rows else outs


def attn_mask_pooled(mask_embed, pooled, *, qbias=None, row_any=None, bits=False, f16=False):
    # f16: False = the fp32 MFMA chain, True = single IEEE-half operands, "x3" = hi + lo IEEE-half pairs (three terms: fp32-class logits)
    """The next layer's attention mask from the pooled activation (pool_mask_taps): attn (B, Q, T) uint8 =
    (einsum('bqc,btc->bqt', mask_embed, pooled) + qbias[b, q]) < 0 and row_any (B, Q) int32 (1 where a row keeps an unmasked
    key).  mask_embed: (B, Q, 64), contiguous or the leading 64 columns of a wider row-major buffer; qbias (B, Q), any uniform
    element stride; row_any: an already ZEROED buffer (saves the fill launch).  Equal to the attention-mask output of
    mask_logits(..., target_size) on the unpooled activation up to fp32 summation order.
    ``bits`` (T % 16 == 0): attn comes back bit-packed and blocked instead -- int16 (B, ceil(Q / 112), T / 16, 16, 8), the layout of
    attn_pack_mask_bits, what hypersphere_attention_fused_kv reads.  ``f16`` (16-bit plans): IEEE-half operands on the 16-bit matrix
    pipe (fp32 accumulation) instead of the fp32 MFMA chain."""
    _chk(mask_embed, "mask_embed"), _c(pooled, "pooled"), _chk(qbias, "qbias")
    B, Q, C = mask_embed.shape
    T = pooled.shape[1]
    if C != 64 or tuple(pooled.shape) != (B, T, 64):
        raise RuntimeError("attn_mask_pooled needs a (B, Q, 64) embedding and a (B, T, 64) pooled activation")
    if mask_embed.stride(2) != 1 or (B > 1 and mask_embed.stride(0) != Q * mask_embed.stride(1)) or mask_embed.stride(1) < C:
        raise RuntimeError("mask_embed must be (B,Q,C) with unit column stride and uniformly spaced rows")
    qb_ld = 0
    if qbias is not None:
        if tuple(qbias.shape) != (B, Q) or (B > 1 and qbias.stride(0) != Q * qbias.stride(1)):
            raise RuntimeError("qbias must be (B,Q) with uniformly spaced elements")
        qb_ld = qbias.stride(1)
    if bits:
        if T % 16:
            raise RuntimeError("attn_mask_pooled(bits=True) needs T % 16 == 0")
        attn = torch.empty((B, (Q + 111) // 112, T // 16, 16, 8), device=mask_embed.device, dtype=torch.int16)
    else:
        attn = torch.empty((B, Q, T), device=mask_embed.device, dtype=torch.uint8)
    cleared = row_any is not None
    if row_any is None:
        row_any = torch.empty((B, Q), device=mask_embed.device, dtype=torch.int32)
    else:
        _c(row_any, "row_any", torch.int32)
    rc = lib().msm_attn_mask_pooled(_p(mask_embed), mask_embed.stride(1), _p(qbias), qb_ld, _p(pooled), _p(attn), _p(row_any),
                                    1 if cleared else 0, (1 if bits else 0) | (4 if f16 == "x3" else (2 if f16 else 0)), B, Q, T, _stream())
    check(rc, "msm_attn_mask_pooled")
    return attn, row_any


def mask_logits(mask_embed, mask_features, *, want_mask=True, target_size=None, sparse=False, row_any=None, packed_bf16=None,
                qbias=None, packed_split=None):
    """einsum('bqc,bchw->bqhw') (+ qbias[b, q]) with the next layer's attention mask fused.
    Returns (mask (B,Q,H,W) or None, attn (B,Q,th*tw) uint8 or None, row_any (B,Q) int32 or None).
    mask_embed: (B,Q,C), contiguous or the leading C columns of a wider row-major buffer; qbias: (B,Q) per-query constant
    (any uniform element stride) -- together they serve the folded form of the step (modeling.FoldedMaskFeatures).
    row_any: an already ZEROED (B,Q) int32 buffer (dec_heads(zero_row_any=True) provides one) -- saves the fill launch.
    packed_bf16: pack_mask_features_bf16(mask_features) -> the step runs with bf16 operands / fp32 accumulation.
    packed_split: pack_mask_features_split(mask_features) (C = 64) -> fp32-accurate on the bf16 matrix pipe (exact 3-term splits)."""
    _chk(mask_embed, "mask_embed"), _c(mask_features, "mask_features"), _chk(qbias, "qbias")
    B, Q, C = mask_embed.shape
    if mask_embed.stride(2) != 1 or (B > 1 and mask_embed.stride(0) != Q * mask_embed.stride(1)) or mask_embed.stride(1) < C:
        raise RuntimeError("mask_embed must be (B,Q,C) with unit column stride and uniformly spaced rows")
    embed_ld = mask_embed.stride(1)
    qb_ld = 0
    if qbias is not None:
        if tuple(qbias.shape) != (B, Q) or (B > 1 and qbias.stride(0) != Q * qbias.stride(1)):
            raise RuntimeError("qbias must be (B,Q) with uniformly spaced elements")
        qb_ld = qbias.stride(1)
    _, Cf, H, W = mask_features.shape
    if Cf != C:
        raise RuntimeError(f"mask_embed has {C} columns, mask_features {Cf} channels")
    dev = mask_embed.device
    mask = torch.empty((B, Q, H, W), device=dev, dtype=torch.float32) if want_mask else None
    attn = None
    th = tw = 0
    flags = 1 if sparse else 0
    if target_size is not None:
        th, tw = int(target_size[0]), int(target_size[1])
        attn = torch.empty((B, Q, th * tw), device=dev, dtype=torch.uint8)
        if row_any is None:
            row_any = torch.empty((B, Q), device=dev, dtype=torch.int32)
        else:
            _c(row_any, "row_any", torch.int32)
            flags |= 2
    else:
        row_any = None
    if packed_split is not None:
        _c(packed_split, "packed_split", torch.int16)
        rc = lib().msm_mask_logits_split_fwd(_p(mask_embed), _p(packed_split), _p(mask), _p(attn), _p(row_any),
                                             B, Q, C, H, W, th, tw, flags, embed_ld, _p(qbias), qb_ld, _stream())
        check(rc, "msm_mask_logits_split_fwd")
        return mask, attn, row_any
    if packed_bf16 is not None:
        half = packed_bf16.dtype == torch.float16                 # pack_mask_features_bf16(..., f16=True): MSM_MASK_F16
        _c(packed_bf16, "packed_bf16", torch.float16 if half else torch.int16)
        rc = lib().msm_mask_logits_bf16_fwd(_p(mask_embed), _p(packed_bf16), _p(mask), _p(attn), _p(row_any),
                                            B, Q, C, H, W, th, tw, flags | (4 if half else 0), embed_ld, _p(qbias), qb_ld, _stream())
        check(rc, "msm_mask_logits_bf16_fwd")
    else:
        rc = lib().msm_mask_logits_fwd(_p(mask_embed), _p(mask_features), _p(mask), _p(attn), _p(row_any),
                                       B, Q, C, H, W, th, tw, flags, embed_ld, _p(qbias), qb_ld, _stream())
        check(rc, "msm_mask_logits_fwd")
    return mask, attn, row_any


def hypersphere_attention(q, k, v, heads, *, masked=None, row_any=None, kappa=KAPPA, low_precision=False, keys_f16=False):
    """q (B,Lq,E), k/v (B,S,E) already projected (last dim contiguous, may be column slices of a
    wider buffer); masked uint8 (B,Lq,S): ANY nonzero byte means masked (1, 2, 128, 255 alike); row_any int32 (B,Lq): 0 switches a row's
    mask off (a fully masked row attends everywhere).  Returns (B,Lq,E).
    low_precision (or bf16 k / v): bf16 MFMA operands with fp32 accumulation (msm_hypersphere_attn_lp_fwd); k and v may then be
    torch.bfloat16 (as written by kv_project_multi(..., out_dtype=torch.bfloat16)) or float32.
    keys_f16 (precision "f16"): q^ / k^ enter the score MFMAs as IEEE halves; a 16-bit k then holds HALF bit patterns (the K columns
    of kv_project_multi(..., keys_f16=True): a torch.bfloat16-typed view whose bits are fp16), v stays bf16."""
    kv_bf16 = k.dtype == torch.bfloat16
    if kv_bf16 != (v.dtype == torch.bfloat16):
        raise RuntimeError("k and v must have the same dtype")
    _chk(q, "q")
    for t, n in ((k, "k"), (v, "v")):
        _chk(t, n, torch.bfloat16 if kv_bf16 else torch.float32)
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        if t.stride(-1) != 1:
            raise RuntimeError(f"{n}: last dim must be contiguous")
    _c(masked, "masked", torch.uint8), _c(row_any, "row_any", torch.int32)
    B, Lq, E = q.shape
    S = k.shape[1]
    if E != heads * 32:
        raise RuntimeError("head_dim must be 32")
    out = torch.empty((B, Lq, E), device=q.device, dtype=torch.float32)
    need = lib().msm_hypersphere_attn_workspace(B, Lq, S, heads)
    ws = torch.empty((need,), device=q.device, dtype=torch.float32)
    if kv_bf16 or low_precision:
        fmt = (2 if kv_bf16 else 3) if keys_f16 else (1 if kv_bf16 else 0)
        rc = lib().msm_hypersphere_attn_lp_fwd(_p(q), _p(k), _p(v), fmt, _p(masked), _p(row_any), _p(out), B, Lq, S, heads,
                                               q.stride(1), q.stride(0), k.stride(1), k.stride(0), v.stride(1), v.stride(0),
                                               kappa, _p(ws), need, _stream())
        check(rc, "msm_hypersphere_attn_lp_fwd")
        return out
    rc = lib().msm_hypersphere_attn_fwd(_p(q), _p(k), _p(v), _p(masked), _p(row_any), _p(out), B, Lq, S, heads,
                                        q.stride(1), q.stride(0), k.stride(1), k.stride(0), v.stride(1), v.stride(0),
                                        kappa, _p(ws), need, _stream())
    check(rc, "msm_hypersphere_attn_fwd")
    return out


def attn_pack_kv_weights(w, heads):
    """[K rows | V rows] folded projection weight (2 * heads * 32, 64) fp32 -> the fp16 MFMA fragments of hypersphere_attention_fused_kv
    (msm_attn_pack_kv_weights): (heads, 8, 64, 8) float16."""
    _c(w, "w")
    if tuple(w.shape) != (2 * heads * 32, 64):
        raise RuntimeError("attn_pack_kv_weights: w must be (2 * heads * 32, 64)")
    out = torch.empty((heads, 8, 64, 8), device=w.device, dtype=torch.float16)
    check(lib().msm_attn_pack_kv_weights(_p(w), _p(out), int(heads), _stream()), "msm_attn_pack_kv_weights")
    return out


def tokens_f16(x):
    """A level feature (B, 64, H, W) -- NCHW or a token-major (channels_last) view -- as the (B, H*W, 64) float16 token matrix
    hypersphere_attention_fused_kv streams (one pass per forward: every layer of the decoder reads the same feature)."""
    _chk(x, "x")
    B, C, H, W = x.shape
    if is_token_major(x) and not x.is_contiguous():
        t = x.permute(0, 2, 3, 1)                                  # (B, H, W, C) view: rows contiguous inside an image
        n = H * W * C
        if t.stride(3) == 1 and t.stride(2) == C and t.stride(1) == W * C and n % 8 == 0 and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0 and B <= 65535:
            # a level's token range of a wider buffer (the encoder's concatenated levels): converted in place, one launch
            out = torch.empty((B, H * W, C), device=x.device, dtype=torch.float16)
            check(lib().msm_f32_to_f16_rows(_p(t), _p(out), B, n, t.stride(0), _stream()), "msm_f32_to_f16_rows")
            return out
        return to_f16(t.reshape(B, H * W, C).contiguous())
    x = x.contiguous()
    if C != 64:
        return to_f16(transpose_last2(x.view(B, C, H * W)))
    out = torch.empty((B, H * W, C), device=x.device, dtype=torch.float16)
    check(lib().msm_nchw_to_tokens_f16(_p(x), _p(out), B, C, H * W, _stream()), "msm_nchw_to_tokens_f16")
    return out


def mask_conv3x3_folded(x_f16, F, size, *, bits=True, row_any=None):
    """The UCN path's mask step with the mask_features convolution folded into the embedding (msm_mask_conv3x3_folded; 16-bit plans):
    x_f16 = tokens_f16(level feature) (B, H*W, 64) float16; F (B, Q, >= 577) fp32 = gemm(e, mask_conv_fold_weight(w, b)); size = (H, W),
    W % 16 == 0, Q <= 112.  bits=True: returns (mask bits int16 (B, 1, S / 16, 16, 8) as hypersphere_attention_fused_kv reads them
    [bit = logit < 0], row_any int32 (B, Q)); ``row_any`` given: a buffer the caller already cleared (dec_heads zero_row_any).
    bits=False: returns the fp32 logits (B, Q, H, W)."""
    _c(x_f16, "x_f16", torch.float16), _c(F, "F"), _c(row_any, "row_any", torch.int32)
    B, Q, ldf = F.shape
    H, W = int(size[0]), int(size[1])
    S = H * W
    if tuple(x_f16.shape) != (B, S, 64) or F.stride(2) != 1 or F.stride(1) % 4 or F.stride(0) % 4 or ldf < MASK_CONV_K + 1:
        raise RuntimeError("mask_conv3x3_folded: x_f16 (B, H*W, 64) float16 and F (B, Q, >= 577) with 16-byte aligned rows")
    if W % 16 or Q > 112:
        raise RuntimeError("mask_conv3x3_folded: W % 16 == 0 and Q <= 112")
    if bits:
        out = torch.empty((B, 1, S // 16, 16, 8), device=F.device, dtype=torch.int16)
        cleared = row_any is not None
        if row_any is None:
            row_any = torch.empty((B, Q), device=F.device, dtype=torch.int32)
        elif tuple(row_any.shape) != (B, Q):
            raise RuntimeError("mask_conv3x3_folded: row_any must be (B, Q)")
        check(lib().msm_mask_conv3x3_folded(_p(x_f16), _p(F), F.stride(1), F.stride(0), _p(out), _p(row_any), 1 if cleared else 0, None,
                                            B, Q, H, W, _stream()), "msm_mask_conv3x3_folded")
        return out, row_any
    out = torch.empty((B, Q, H, W), device=F.device, dtype=torch.float32)
    check(lib().msm_mask_conv3x3_folded(_p(x_f16), _p(F), F.stride(1), F.stride(0), None, None, 0, _p(out), B, Q, H, W, _stream()),
          "msm_mask_conv3x3_folded")
    return out


def attn_pack_mask_bits(masked):
    """uint8 mask (B, Lq, S) (nonzero = masked), S % 16 == 0 -> the bit-packed, blocked form hypersphere_attention_fused_kv reads
    (msm_attn_pack_mask_bits): int16 (B, ceil(Lq / 112), S / 16, 16, 8), word [b, qc, kb, lj, m] bit k = masked[b, 112 qc + 16 m + lj, 16 kb + k]."""
    _c(masked, "masked", torch.uint8)
    B, Lq, S = masked.shape
    if S % 16:
        raise RuntimeError("attn_pack_mask_bits: S must be a multiple of 16")
    out = torch.empty((B, (Lq + 111) // 112, S // 16, 16, 8), device=masked.device, dtype=torch.int16)
    assert out.numel() * 2 == lib().msm_attn_mask_bits_bytes(B, Lq, S)
    check(lib().msm_attn_pack_mask_bits(_p(masked), _p(out), B, Lq, S, _stream()), "msm_attn_pack_mask_bits")
    return out


def hypersphere_attention_fused_kv(q, x_f16, w_packed, rowcol, col_v_t, size, heads, *, masked=None, row_any=None, kappa=KAPPA, keys_f16=False):
    """Cross attention over a long key sequence with the folded K/V projection inside the kernel (msm_hypersphere_attn_fused_kv_fwd;
    16-bit plans): q (B, Lq, E) projected queries; x_f16 = tokens_f16(level feature) (B, H*W, 64); w_packed = attn_pack_kv_weights(w);
    rowcol (H + W, 2E) the separable constants of kv_project(cmat_width=W); col_v_t (E, W) = rowcol[H:, E:].t(); size = (H, W), W % 16 == 0.
    masked: uint8 (B, Lq, S), any nonzero byte = masked, packed here, or the int16 bit-packed form (attn_pack_mask_bits / attn_mask_pooled(bits=True)).
    keys_f16: q^ / k^ as IEEE halves (precision "f16") instead of bf16.  Returns (B, Lq, E)."""
    _chk(q, "q"), _c(x_f16, "x_f16", torch.float16), _c(w_packed, "w_packed", torch.float16), _c(rowcol, "rowcol"), _c(col_v_t, "col_v_t")
    prepacked = masked is not None and masked.dtype == torch.int16            # attn_mask_pooled(bits=True) / attn_pack_mask_bits output
    _c(masked, "masked", torch.int16 if prepacked else torch.uint8), _c(row_any, "row_any", torch.int32)
    if q.stride(-1) != 1:
        raise RuntimeError("q: last dim must be contiguous")
    B, Lq, E = q.shape
    H, W = int(size[0]), int(size[1])
    S = H * W
    mshape = (B, (Lq + 111) // 112, S // 16, 16, 8) if prepacked else (B, Lq, S)
    if E != heads * 32 or tuple(x_f16.shape) != (B, S, 64) or tuple(rowcol.shape) != (H + W, 2 * E) or tuple(col_v_t.shape) != (E, W) \
            or tuple(w_packed.shape) != (heads, 8, 64, 8) or (masked is not None and tuple(masked.shape) != mshape):
        raise RuntimeError("hypersphere_attention_fused_kv: inconsistent shapes")
    out = torch.empty((B, Lq, E), device=q.device, dtype=torch.float32)
    need = lib().msm_hypersphere_attn_workspace(B, Lq, S, heads)
    ws = torch.empty((need,), device=q.device, dtype=torch.float32)
    bits = None if masked is None else (masked if prepacked else attn_pack_mask_bits(masked))     # one 16-byte load per lane and key block in the kernel
    rc = lib().msm_hypersphere_attn_fused_kv_fwd(_p(q), _p(x_f16), _p(w_packed), _p(rowcol), _p(col_v_t), 2 if keys_f16 else 1, _p(bits), _p(row_any),
                                                 _p(out), B, Lq, H, W, heads, q.stride(1), q.stride(0), kappa, _p(ws), need, _stream())
    check(rc, "msm_hypersphere_attn_fused_kv_fwd")
    return out


def hypersphere_attention_backward(q, k, v, heads, grad_out, *, masked=None, row_any=None, kappa=KAPPA):
    """Gradient of hypersphere_attention: returns (grad_q (B,Lq,E), grad_k (B,S,E), grad_v (B,S,E)), contiguous."""
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        _chk(t, n)
        if t.stride(-1) != 1:
            raise RuntimeError(f"{n}: last dim must be contiguous")
    _c(grad_out, "grad_out"), _c(masked, "masked", torch.uint8), _c(row_any, "row_any", torch.int32)
    if masked is not None and row_any is None:
        # a fully masked row has a zero softmax denominator in the recomputation (NaN gradients); the forward resets such rows
        # through row_any (DEC:618), so the backward needs the same flags
        raise RuntimeError("hypersphere_attention_backward: row_any is required whenever masked is given")
    B, Lq, E = q.shape
    S = k.shape[1]
    if E != heads * 32 or tuple(grad_out.shape) != (B, Lq, E):
        raise RuntimeError("head_dim must be 32 and grad_out (B,Lq,E)")
    gq = torch.empty((B, Lq, E), device=q.device, dtype=torch.float32)
    gk = torch.empty((B, S, E), device=q.device, dtype=torch.float32)
    gv = torch.empty((B, S, E), device=q.device, dtype=torch.float32)
    need = lib().msm_hypersphere_attn_bwd_workspace(B, Lq, heads)
    ws = torch.empty((need,), device=q.device, dtype=torch.float32)
    rc = lib().msm_hypersphere_attn_bwd(_p(q), _p(k), _p(v), _p(masked), _p(row_any), _p(grad_out), _p(gq), _p(gk), _p(gv), B, Lq, S, heads,
                                        q.stride(1), q.stride(0), k.stride(1), k.stride(0), v.stride(1), v.stride(0), kappa, _p(ws), need, _stream())
    check(rc, "msm_hypersphere_attn_bwd")
    return gq, gk, gv


# ----------------------------------------------------------------------------------------------
# fused decoder-layer tails (csrc/dec_chain.hip)
# ----------------------------------------------------------------------------------------------
def dec_pack_weight(w):
    """(N, K) torch Linear weight -> the MFMA-fragment order the dec_* kernels stream (include/msm_hip.h)."""
    _c(w, "w")
    N, K = w.shape
    packed = torch.empty_like(w)
    rc = lib().msm_dec_pack_weight(_p(w), _p(packed), N, K, _stream())
    check(rc, "msm_dec_pack_weight")
    return packed


def dec_pack_weight_bf16(w):
    """(N, K) fp32 Linear weight -> bf16 in the fragment order of the low-precision dec_* kernels (msm_dec_pack_weight_bf16);
    the result (dtype torch.bfloat16, shape (N, K), NOT row-major) is what dec_post_cross / dec_post_self / dec_heads take as
    a weight in that mode: they pick the bf16 entry points by the weights' dtype."""
    _c(w, "w")
    N, K = w.shape
    packed = torch.empty((N, K), device=w.device, dtype=torch.bfloat16)
    rc = lib().msm_dec_pack_weight_bf16(_p(w), _p(packed), N, K, _stream())
    check(rc, "msm_dec_pack_weight_bf16")
    return packed


def dec_pack_weight_bf16x2(w):
    """(N, K) fp32 Linear weight -> hi + lo bf16 fragments [bf16(W) | bf16(W - bf16(W))] (msm_dec_pack_weight_bf16x2; dtype
    torch.bfloat16, shape (N, 2 K), NOT row-major): what the "bf16" plan's tails multiply by since round 6 -- the dec_* wrappers pick the
    _bf16x2 entry points by the mark this function leaves on the tensor."""
    _c(w, "w")
    N, K = w.shape
    packed = torch.empty((N, 2 * K), device=w.device, dtype=torch.bfloat16)
    rc = lib().msm_dec_pack_weight_bf16x2(_p(w), _p(packed), N, K, _stream())
    check(rc, "msm_dec_pack_weight_bf16x2")
    packed._msm_x2 = True
    return packed


def dec_pack_weight_f16(w):
    """(N, K) fp32 Linear weight -> IEEE half in the fragment order of the 16-bit dec_* kernels (msm_dec_pack_weight_f16; dtype
    torch.float16, shape (N, K), NOT row-major): precision "f16" -- the dec_* wrappers pick the _f16 entry points by this dtype."""
    _c(w, "w")
    N, K = w.shape
    packed = torch.empty((N, K), device=w.device, dtype=torch.float16)
    rc = lib().msm_dec_pack_weight_f16(_p(w), _p(packed), N, K, _stream())
    check(rc, "msm_dec_pack_weight_f16")
    return packed


_DEC_SUFFIX = {torch.float32: "", torch.bfloat16: "_bf16", torch.float16: "_f16"}


def _wdtype(*ws):
    """Common dtype of the packed weight matrices of a dec_* call (fp32, bf16 or fp16 fragments, never mixed)."""
    dts = {w.dtype for w in ws if w is not None}
    if len(dts) != 1 or next(iter(dts)) not in _DEC_SUFFIX:
        raise RuntimeError(f"packed weights must be all float32, all bfloat16 or all float16, got {sorted(map(str, dts))}")
    return next(iter(dts))


def _dec_suffix(*ws):
    """Entry-point suffix for the packed weights of a dec_* call: by dtype, and "_bf16x2" for hi + lo bf16 fragments (all or none)."""
    wd = _wdtype(*ws)
    x2 = {bool(getattr(w, "_msm_x2", False)) for w in ws if w is not None}
    if len(x2) != 1:
        raise RuntimeError("packed weights must be all hi + lo bf16 fragments (dec_pack_weight_bf16x2) or none")
    return "_bf16x2" if x2.pop() else _DEC_SUFFIX[wd]


def dec_post_cross(attn_out, res, query_pos, wo, bo, ln_g, ln_b, w_in, b_in, eps=1e-5):
    """Weight matrices of the three dec_* calls are dec_pack_weight() outputs.
    x = LN(res + attn_out wo^T + bo); qk = (x + query_pos) w_in[:2E]^T + b_in[:2E]; v = x w_in[2E:]^T + b_in[2E:].
    attn_out/res (B,Q,E); query_pos (Q,E).  Returns (x (B,Q,E), qk (B,Q,2E), v (B,Q,E))."""
    wd = _wdtype(wo, w_in)
    for t, n in ((attn_out, "attn_out"), (res, "res"), (query_pos, "query_pos"), (bo, "bo"), (ln_g, "ln_g"), (ln_b, "ln_b"), (b_in, "b_in")):
        _c(t, n)
    _c(wo, "wo", wd), _c(w_in, "w_in", wd)
    B, Q, E = attn_out.shape
    x = torch.empty_like(attn_out)
    qk = torch.empty((B, Q, 2 * E), device=attn_out.device, dtype=torch.float32)
    v = torch.empty_like(attn_out)
    fn = getattr(lib(), "msm_dec_post_cross" + _dec_suffix(wo, w_in))
    rc = fn(_p(attn_out), _p(res), _p(query_pos), _p(wo), _p(bo), _p(ln_g), _p(ln_b), _p(w_in), _p(b_in), _p(x), _p(qk), _p(v), B * Q, Q, E,
            eps, _stream())
    check(rc, "msm_dec_post_cross")
    return x, qk, v


def dec_post_self(attn_out, res, wo, bo, ln_g, ln_b, w1, b1, w2, n_parts=None, eps=1e-5):
    """x = LN(res + attn_out wo^T + bo); parts (n_parts, B, Q, E): partial sums over equal slices of the hidden
    dimension of linear2(relu(linear1(x))), without linear2's bias.  Default n_parts: about 200 workgroups."""
    wd = _wdtype(wo, w1, w2)
    for t, n in ((attn_out, "attn_out"), (res, "res"), (bo, "bo"), (ln_g, "ln_g"), (ln_b, "ln_b"), (b1, "b1")):
        _c(t, n)
    _c(wo, "wo", wd), _c(w1, "w1", wd), _c(w2, "w2", wd)
    B, Q, E = attn_out.shape
    F = w1.shape[0]
    x = torch.empty_like(attn_out)
    chunks = F // E
    if n_parts is None:
        tiles = (B * Q + 15) // 16
        n_parts = max(d for d in range(1, chunks + 1) if chunks % d == 0 and (d == 1 or tiles * d <= 256))
    parts = torch.empty((n_parts, B, Q, E), device=attn_out.device, dtype=torch.float32)
    fn = getattr(lib(), "msm_dec_post_self" + _dec_suffix(wo, w1, w2))
    rc = fn(_p(attn_out), _p(res), _p(wo), _p(bo), _p(ln_g), _p(ln_b), _p(w1), _p(b1), _p(w2), F, _p(x), _p(parts), n_parts, B * Q, E, eps,
            _stream())
    check(rc, "msm_dec_post_self")
    return x, parts


def dec_heads(x, dec_g, dec_b, mlp, *, parts=None, bias=None, ln_g=None, ln_b=None, l2norm=False, wq=None, bq=None,
              query_pos=None, want_out=True, want_d=False, zero_row_any=False, eps=1e-5):
    """t = x + sum(parts) + bias [-> LN] [-> unit length]; d = LN_dec(t); e = MLP3(d); q = (t + query_pos) wq^T + bq.
    mlp = [(w0,b0),(w1,b1),(w2,b2)].  Returns (out|None, d|None, e, q|None), plus a zeroed (B,Q) int32 row_any buffer
    for the following mask step when zero_row_any."""
    wd = _wdtype(wq, *[w for w, _ in mlp])
    for i, t in enumerate([x, parts, bias, ln_g, ln_b, dec_g, dec_b, bq, query_pos] + [b for _, b in mlp]):
        _c(t, f"dec_heads arg {i}")
    for i, t in enumerate([wq] + [w for w, _ in mlp]):
        _c(t, f"dec_heads weight {i}", wd)
    B, Q, E = x.shape
    out = torch.empty_like(x) if want_out else None
    d = torch.empty_like(x) if want_d else None
    e = torch.empty_like(x)
    q = torch.empty_like(x) if wq is not None else None
    ra = torch.empty((B, Q), device=x.device, dtype=torch.int32) if zero_row_any else None
    n_parts = 0 if parts is None else parts.shape[0]
    (m0w, m0b), (m1w, m1b), (m2w, m2b) = mlp
    fn = getattr(lib(), "msm_dec_heads" + _dec_suffix(wq, *[w for w, _ in mlp]))
    rc = fn(_p(x), _p(parts), n_parts, _p(bias), _p(ln_g), _p(ln_b), 1 if l2norm else 0, _p(dec_g), _p(dec_b), _p(m0w), _p(m0b), _p(m1w),
            _p(m1b), _p(m2w), _p(m2b), _p(wq), _p(bq), _p(query_pos), _p(out), _p(d), _p(e), _p(q), _p(ra), B * Q, Q, E, eps, _stream())
    check(rc, "msm_dec_heads")
    return (out, d, e, q, ra) if zero_row_any else (out, d, e, q)


def dec_heads_mask(x, dec_g, dec_b, mlp, pooled, row_any, *, qcol=64, bits=False, f16=False, parts=None, bias=None, ln_g=None, ln_b=None, l2norm=False,
                   wq=None, bq=None, query_pos=None, want_out=True, want_d=False, eps=1e-5):
    """dec_heads (16-bit weight fragments) with the next layer's attention mask at key resolution as the kernel's epilogue
    (msm_dec_heads_mask): the values of dec_heads(...) followed by attn_mask_pooled(e[..., :64], pooled, qbias=e[..., qcol],
    row_any=row_any, bits=bits, f16=f16), bit for bit, in one launch.  ``mlp[-1]`` must be the folded final layer ([e Wm | e.bm | ..]);
    ``row_any`` (B, Q) int32 must arrive ZEROED.  Returns (out|None, d|None, e, q|None, attn, row_any)."""
    wd = _wdtype(wq, *[w for w, _ in mlp])
    if wd not in (torch.bfloat16, torch.float16) or _dec_suffix(wq, *[w for w, _ in mlp]) == "_bf16x2":
        raise RuntimeError("dec_heads_mask needs single bf16 or fp16 weight fragments (the fp32 plan and the hi + lo bf16 form keep the two launches)")
    for i, t in enumerate([x, parts, bias, ln_g, ln_b, dec_g, dec_b, bq, query_pos, pooled] + [b for _, b in mlp]):
        _c(t, f"dec_heads_mask arg {i}")
    for i, t in enumerate([wq] + [w for w, _ in mlp]):
        _c(t, f"dec_heads_mask weight {i}", wd)
    _c(row_any, "row_any", torch.int32)
    B, Q, E = x.shape
    T = pooled.shape[1]
    if tuple(pooled.shape) != (B, T, 64) or tuple(row_any.shape) != (B, Q):
        raise RuntimeError("dec_heads_mask needs a (B, T, 64) pooled activation and a (B, Q) row_any buffer")
    out = torch.empty_like(x) if want_out else None
    d = torch.empty_like(x) if want_d else None
    e = torch.empty_like(x)
    q = torch.empty_like(x) if wq is not None else None
    if bits:
        if T % 16:
            raise RuntimeError("dec_heads_mask(bits=True) needs T % 16 == 0")
        attn = torch.empty((B, (Q + 111) // 112, T // 16, 16, 8), device=x.device, dtype=torch.int16)
    else:
        attn = torch.empty((B, Q, T), device=x.device, dtype=torch.uint8)
    n_parts = 0 if parts is None else parts.shape[0]
    (m0w, m0b), (m1w, m1b), (m2w, m2b) = mlp
    rc = lib().msm_dec_heads_mask(_p(x), _p(parts), n_parts, _p(bias), _p(ln_g), _p(ln_b), 1 if l2norm else 0, _p(dec_g), _p(dec_b), _p(m0w), _p(m0b),
                                  _p(m1w), _p(m1b), _p(m2w), _p(m2b), _p(wq), _p(bq), _p(query_pos), _p(out), _p(d), _p(e), _p(q), _p(pooled), T,
                                  int(qcol), _p(attn), _p(row_any), (1 if bits else 0) | (2 if wd == torch.float16 else 0) | (4 if f16 else 0), B * Q, Q, E, eps, _stream())
    check(rc, "msm_dec_heads_mask")
    return out, d, e, q, attn, row_any


def dec_set_prefetch(tensors):
    """The NEXT dec_post_cross / dec_post_self / dec_heads(_mask) call of this thread touches the storage of ``tensors`` (<= 6 contiguous
    device tensors: the packed weights of the launches behind it in the chain) from an extra row of workgroups, so that every XCD's L2
    holds them when those launches start (msm_dec_set_prefetch).  Speed only; an empty list clears a pending request."""
    ts = [t for t in tensors if t is not None and t.numel() > 0][:6]
    for t in ts:
        if not t.is_cuda or not t.is_contiguous():
            raise RuntimeError("dec_set_prefetch needs contiguous device tensors")
    n = len(ts)
    ptrs = (ctypes.c_void_p * max(n, 1))(*[t.data_ptr() for t in ts])
    nbytes = (ctypes.c_int64 * max(n, 1))(*[t.numel() * t.element_size() for t in ts])
    check(lib().msm_dec_set_prefetch(ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(nbytes, ctypes.c_void_p), n), "msm_dec_set_prefetch")


def l2_prefetch(tensors):
    """Touch the storage of up to 8 device tensors per launch so that every XCD's L2 holds it (msm_l2_prefetch): issued on a side stream
    beside a kernel that leaves the fabric idle, ahead of the kernel that streams these bytes.  Speed only."""
    ts = [t for t in tensors if t is not None and t.numel() > 0]
    for t in ts:
        if not t.is_cuda or not t.is_contiguous():
            raise RuntimeError("l2_prefetch needs contiguous device tensors")
    for i in range(0, len(ts), 8):
        grp = ts[i:i + 8]
        ptrs = (ctypes.c_void_p * len(grp))(*[t.data_ptr() for t in grp])
        nbytes = (ctypes.c_int64 * len(grp))(*[t.numel() * t.element_size() for t in grp])
        check(lib().msm_l2_prefetch(ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(nbytes, ctypes.c_void_p), len(grp), _stream()), "msm_l2_prefetch")


def _msda_dtype(value, others):
    """float32 or float64 like the reference's dispatch (ms_deform_attn_cuda.cu:69); every floating tensor the same."""
    dt = value.dtype
    if dt not in (torch.float32, torch.float64):
        raise RuntimeError(f"ms_deform_attn: value must be float32 or float64, got {dt}")
    for t, name in others:
        _c(t, name, dt)
    return dt


def ms_deform_attn(value, spatial_shapes, level_start_index, sampling_locations, attention_weights):
    """Reference-ABI core op: value (N,S,M,D), shapes (L,2) int64, start (L,) int64,
    loc (N,Lq,M,L,P,2), w (N,Lq,M,L,P) -> (N,Lq,M*D).  float32 or float64."""
    dt = _msda_dtype(value, ((value, "value"), (sampling_locations, "sampling_locations"),
                             (attention_weights, "attention_weights")))
    _c(spatial_shapes, "spatial_shapes", torch.int64), _c(level_start_index, "level_start_index", torch.int64)
    N, S, M, D = value.shape
    _, Lq, _, L, P, _ = sampling_locations.shape
    out = torch.empty((N, Lq, M * D), device=value.device, dtype=dt)
    fn, what = ((lib().msm_msdeform_attn_fwd, "msm_msdeform_attn_fwd") if dt == torch.float32 else
                (lib().msm_msdeform_attn_fwd_f64, "msm_msdeform_attn_fwd_f64"))
    rc = fn(_p(value), _p(spatial_shapes), _p(level_start_index), _p(sampling_locations),
            _p(attention_weights), _p(out), N, S, M, D, L, Lq, P, _stream())
    check(rc, what)
    return out


MSDA_DET_MAX_D, MSDA_DET_MAX_L = 64, 8     # the range of msm_msdeform_attn_bwd_det (float32)


def msda_backward_deterministic(deterministic=None):
    """The form ms_deform_attn_backward takes: ``deterministic`` itself, or torch's global flag when it is None."""
    return torch.are_deterministic_algorithms_enabled() if deterministic is None else bool(deterministic)


def ms_deform_attn_backward_det_workspace(N, S, M, D):
    """Bytes of workspace the deterministic backward takes for N images (msm_msdeform_attn_bwd_det_workspace)."""
    return int(lib().msm_msdeform_attn_bwd_det_workspace(int(N), int(S), int(M), int(D)))


def _msda_det_supported(value, sampling_locations):
    """False (after a warning) where the deterministic backward does not exist and torch's warn-only mode is on; raises otherwise."""
    D, L = value.shape[3], sampling_locations.shape[3]
    if value.dtype == torch.float32 and D <= MSDA_DET_MAX_D and L <= MSDA_DET_MAX_L:
        return True
    msg = (f"ms_deform_attn_backward does not have a deterministic implementation for dtype {value.dtype}, D={D}, L={L} "
           f"(float32, D <= {MSDA_DET_MAX_D}, L <= {MSDA_DET_MAX_L} only), but a deterministic result was requested "
           "(deterministic=True or torch.use_deterministic_algorithms(True))")
    if torch.is_deterministic_algorithms_warn_only_enabled():
        warnings.warn(msg + "; running the atomic kernel, whose last bits depend on scheduling", UserWarning, stacklevel=3)
        return False
    raise RuntimeError(msg + ". Pass deterministic=False, or torch.use_deterministic_algorithms(True, warn_only=True), to run the atomic kernel.")


def ms_deform_attn_backward(value, spatial_shapes, level_start_index, sampling_locations, attention_weights, grad_output,
                            deterministic=None, workspace_images=None, workspace=None):
    """Reference-ABI backward: returns (grad_value, grad_sampling_loc, grad_attn_weight).  float32 or float64.
    deterministic: None follows torch.are_deterministic_algorithms_enabled(), True / False force the choice.  The deterministic form
    (msm_msdeform_attn_bwd_det: float32, D <= 64, L <= 8) gives results that are a pure function of the inputs -- the same bits
    on every call, under any order of queries or points and for any batch around an image; outside its range a request raises, or
    warns and runs the atomic kernel under torch's warn_only mode.  Its workspace is allocated here for the whole batch, for
    ``workspace_images`` images (the images then run in groups; same bits), or is the caller's ``workspace`` (a contiguous uint8
    device tensor of at least one image's bytes, see ms_deform_attn_backward_det_workspace)."""
    det = msda_backward_deterministic(deterministic) and _msda_det_supported(value, sampling_locations)
    dt = _msda_dtype(value, ((value, "value"), (sampling_locations, "sampling_locations"),
                             (attention_weights, "attention_weights"), (grad_output, "grad_output")))
    _c(spatial_shapes, "spatial_shapes", torch.int64), _c(level_start_index, "level_start_index", torch.int64)
    N, S, M, D = value.shape
    _, Lq, _, L, P, _ = sampling_locations.shape
    if tuple(grad_output.shape) != (N, Lq, M * D):
        raise RuntimeError(f"grad_output must be {(N, Lq, M * D)}, got {tuple(grad_output.shape)}")
    gv = torch.empty_like(value)
    gl = torch.empty_like(sampling_locations)
    gw = torch.empty_like(attention_weights)
    if det:
        if workspace is None:
            images = N if workspace_images is None else max(1, min(N, int(workspace_images)))
            workspace = torch.empty(ms_deform_attn_backward_det_workspace(images, S, M, D), device=value.device, dtype=torch.uint8)
        else:
            _c(workspace, "workspace", torch.uint8)
        rc = lib().msm_msdeform_attn_bwd_det(_p(value), _p(spatial_shapes), _p(level_start_index), _p(sampling_locations),
                                             _p(attention_weights), _p(grad_output), _p(gv), _p(gl), _p(gw),
                                             N, S, M, D, L, Lq, P, _p(workspace), workspace.numel(), _stream())
        check(rc, "msm_msdeform_attn_bwd_det")
        return gv, gl, gw
    fn, what = ((lib().msm_msdeform_attn_bwd, "msm_msdeform_attn_bwd") if dt == torch.float32 else
                (lib().msm_msdeform_attn_bwd_f64, "msm_msdeform_attn_bwd_f64"))
    rc = fn(_p(value), _p(spatial_shapes), _p(level_start_index), _p(sampling_locations),
            _p(attention_weights), _p(grad_output), _p(gv), _p(gl), _p(gw),
            N, S, M, D, L, Lq, P, _stream())
    check(rc, what)
    return gv, gl, gw


def kv_project_multi(xs, ws, cmats, out_dtype=torch.float32, split=False, cmat_widths=None, keys_f16=False):
    """kv_project for a list of jobs in one launch: xs[j] (B, 64, H_j, W_j) contiguous NCHW or token-major
    (is_token_major), ws[j] (N, 64), cmats[j] (H_j*W_j, N) -> list of (B, H_j*W_j, N).  N in {256, 512}, <= 16 jobs.
    out_dtype torch.bfloat16: low-precision mode (bf16 MFMAs: w rounded to bf16, x as a hi + lo pair; bf16 output).
    split: fp32 results on the bf16 matrix pipe (exact three-term splits, msm_kv_project_multi_split).
    cmat_widths[j] = W_j: separable constants, cmats[j] (H_j + W_j, N) (see kv_project); all jobs or none.
    keys_f16 (out_dtype bfloat16, N = 512; precision "f16"): IEEE-half operands, and the K columns [:, :, :256] of the result hold
    HALF bit patterns (the tensor stays typed bfloat16: only hypersphere_attention(..., keys_f16=True) should read them), V bf16."""
    if keys_f16 and (out_dtype != torch.bfloat16 or ws[0].shape[0] != 512):
        raise RuntimeError("kv_project_multi: keys_f16 goes with out_dtype=torch.bfloat16 and N = 512 ([K | V])")
    if split and out_dtype != torch.float32:
        raise RuntimeError("kv_project_multi: split is the fp32-accurate form (float32 output)")
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError("kv_project_multi: out_dtype must be float32 or bfloat16")
    n = len(xs)
    B, N = xs[0].shape[0], ws[0].shape[0]
    outs, tok, sb, hw = [], [], [], []
    cws = [int(v) for v in cmat_widths] if cmat_widths is not None else [0] * n
    for x, w, c, cw in zip(xs, ws, cmats, cws):
        _chk(x, "x"), _c(w, "w"), _c(c, "cmat")
        Bx, C, H, W = x.shape
        t = is_token_major(x) and not x.is_contiguous()
        if not t:
            _c(x, "x")
        if Bx != B or C != 64 or w.shape[0] != N or tuple(w.shape) != (N, 64) or cw not in (0, W) \
                or tuple(c.shape) != ((H + W, N) if cw else (H * W, N)):
            raise RuntimeError("kv_project_multi: inconsistent job shapes")
        tok.append(1 if t else 0)
        sb.append(x.stride(0) if t else C * H * W)
        hw.append(H * W)
        outs.append(torch.empty((B, H * W, N), device=x.device, dtype=out_dtype))
    vp = ctypes.c_void_p * n
    arr = lambda ts: ctypes.cast(vp(*[t.data_ptr() for t in ts]), ctypes.c_void_p)
    ia, la = (ctypes.c_int32 * n), (ctypes.c_int64 * n)
    fn = (lib().msm_kv_project_multi_split if split else lib().msm_kv_project_multi_f32) if out_dtype == torch.float32 else lib().msm_kv_project_multi_bf16
    extra = (int(bool(keys_f16)),) if out_dtype == torch.bfloat16 else ()
    rc = fn(n, arr(xs), arr(ws), arr(cmats), arr(outs), ctypes.cast(ia(*hw), ctypes.c_void_p), ctypes.cast(ia(*tok), ctypes.c_void_p),
            ctypes.cast(la(*sb), ctypes.c_void_p), ctypes.cast(ia(*cws), ctypes.c_void_p), B, 64, N, *extra, _stream())
    check(rc, "msm_kv_project_multi")
    return outs


def value_to_head_major(value, heads):
    """(N, S, C) token-major value -> (N, heads, S, C/heads), the layout ms_deform_attn_encoder gathers fastest from."""
    _c(value, "value")
    N, S, C = value.shape
    out = torch.empty((N, heads, S, C // heads), device=value.device, dtype=torch.float32)
    rc = lib().msm_value_to_head_major_f32(_p(value), _p(out), N, S, heads, C // heads, _stream())
    check(rc, "msm_value_to_head_major_f32")
    return out


def ms_deform_attn_encoder(value, spatial_shapes, level_start_index, proj, heads, n_points):
    """Encoder self-attention form: proj (N,S,heads*L*P*3) raw offsets+logits; value (N,S,C) token-major, or
    (N,heads,S,C/heads) head-major as written by encoder_block(value_heads=heads).  Returns (N,S,C)."""
    _c(value, "value"), _c(proj, "proj")
    _c(spatial_shapes, "spatial_shapes", torch.int64), _c(level_start_index, "level_start_index", torch.int64)
    L = spatial_shapes.shape[0]
    if value.dim() == 4:
        N, M, S, D = value.shape
        if M != heads:
            raise RuntimeError("head-major value must be (N, heads, S, C/heads)")
        out = torch.empty((N, S, M * D), device=value.device, dtype=torch.float32)
        rc = lib().msm_msdeform_attn_enc_hm_fwd(_p(value), _p(spatial_shapes), _p(level_start_index), _p(proj), _p(out),
                                                N, S, M, D, L, n_points, _stream())
        check(rc, "msm_msdeform_attn_enc_hm_fwd")
        return out
    N, S, C = value.shape
    out = torch.empty((N, S, C), device=value.device, dtype=torch.float32)
    rc = lib().msm_msdeform_attn_enc_fwd(_p(value), _p(spatial_shapes), _p(level_start_index), _p(proj), _p(out),
                                         N, S, heads, C // heads, L, n_points, _stream())
    check(rc, "msm_msdeform_attn_enc_fwd")
    return out


def pack_msda_proj(wp, bp, heads, n_levels, n_points):
    """[sampling_offsets ; attention_weights] weight (heads*L*P*3, 64) and bias -> the per-head fragment-order stream and bias
    table of ms_deform_attn_encoder_fused (msm_msda_pack_proj)."""
    _c(wp, "wp"), _c(bp, "bp")
    if tuple(wp.shape) != (heads * n_levels * n_points * 3, 64) or bp.numel() != wp.shape[0]:
        raise RuntimeError(f"pack_msda_proj: weight must be ({heads * n_levels * n_points * 3}, 64) with a bias per row")
    wpack = torch.empty(heads * 3 * 4 * 64 * 4, device=wp.device, dtype=torch.float32)
    bpack = torch.empty(heads * 48, device=wp.device, dtype=torch.float32)
    check(lib().msm_msda_pack_proj(_p(wp), _p(bp), _p(wpack), _p(bpack), heads, n_levels, n_points, _stream()), "msm_msda_pack_proj")
    return wpack, bpack


def ms_deform_attn_encoder_fused(value_hm, spatial_shapes, level_start_index, src, pos, wpack, bpack, n_points):
    """Encoder self-attention with the sampling projection computed in the kernel: value_hm (N,heads,S,8) head-major,
    src (N,S,64) the layer input, pos (S,64); wpack / bpack from pack_msda_proj.  Returns (N,S,64)."""
    _c(value_hm, "value_hm"), _c(src, "src"), _c(pos, "pos"), _c(wpack, "wpack"), _c(bpack, "bpack")
    _c(spatial_shapes, "spatial_shapes", torch.int64), _c(level_start_index, "level_start_index", torch.int64)
    N, M, S, D = value_hm.shape
    if tuple(src.shape) != (N, S, M * D) or tuple(pos.shape) != (S, M * D):
        raise RuntimeError("ms_deform_attn_encoder_fused: src must be (N,S,C) and pos (S,C) for a (N,heads,S,C/heads) value")
    out = torch.empty((N, S, M * D), device=src.device, dtype=torch.float32)
    rc = lib().msm_msdeform_attn_enc_fused_fwd(_p(value_hm), _p(spatial_shapes), _p(level_start_index), _p(src), _p(pos), _p(wpack),
                                               _p(bpack), _p(out), N, S, M, D, spatial_shapes.shape[0], n_points, _stream())
    check(rc, "msm_msdeform_attn_enc_fused_fwd")
    return out


# ----------------------------------------------------------------------------------------------
# mean shift (lib/utils/mean_shift.py)
# ----------------------------------------------------------------------------------------------
def ms_pack_bf16(X):
    """X (n,64) fp32 -> the bf16 copy (msm_ms_bf16_rows(n), 64) (rows zero-padded to whole 32-point slabs) that the "bf16" precision
    of the clustering streams instead of X (ms_select_seeds / ms_hill_climb with xb=...)."""
    _c(X, "X")
    n, d = X.shape
    xb = torch.empty((lib().msm_ms_bf16_rows(n), d), device=X.device, dtype=torch.bfloat16)
    check(lib().msm_ms_pack_bf16(_p(X), n, d, _p(xb), _stream()), "msm_ms_pack_bf16")
    return xb


def _check_xb(xb, n, d, who):
    """``xb`` must be the whole padded copy ms_pack_bf16 makes: the kernels read entire 32-row slabs, so a shorter buffer (even one
    with n rows) would be read past its end."""
    _c(xb, "xb", torch.bfloat16)
    want = (int(lib().msm_ms_bf16_rows(n)), d)
    if tuple(xb.shape) != want:
        raise RuntimeError(f"{who}: xb has shape {tuple(xb.shape)}, expected ms_pack_bf16(X) of shape {want}")
    return xb


MS_METRICS = ("cosine", "euclidean")


def _ms_l2(metric, who):
    """True for the Euclidean entry points (msm_ms_*_l2), False for the cosine ones; anything else is not a metric."""
    if metric not in MS_METRICS:
        raise ValueError(f"{who}: metric must be 'cosine' or 'euclidean', not {metric!r}")
    return metric == "euclidean"


def _ms_select_seeds(X, num_seeds, first, first_index, stepwise, give_up_mask, metric="cosine"):
    """X (M,n,64); ``first`` int64 (M,) on the device, or None with the host scalar ``first_index`` (one map: nothing is copied)."""
    M, n, d = X.shape
    seeds = torch.empty((M, num_seeds, d), device=X.device, dtype=torch.float32)
    idx = torch.empty((M, num_seeds), device=X.device, dtype=torch.int64)
    need = lib().msm_ms_seed_workspace(M, n)
    ws = torch.empty((need,), device=X.device, dtype=torch.float32)
    if _ms_l2(metric, "ms_select_seeds"):
        # one launch per step whatever ``stepwise`` says: the persistent kernels, and with them the give-up, are cosine-only
        rc = lib().msm_ms_select_seeds_l2(_p(X), M, n, d, num_seeds, _p(first), first_index, _p(seeds), _p(idx), _p(ws), need, _stream())
        check(rc, "msm_ms_select_seeds_l2")
        return seeds, idx
    rc = lib().msm_ms_select_seeds(_p(X), M, n, d, num_seeds, _p(first), first_index, _p(seeds), _p(idx), _p(ws), need,
                                   (1 if stepwise else 0) | (2 if give_up_mask else 0), give_up_mask, _stream())
    check(rc, "msm_ms_select_seeds")
    return seeds, idx


def ms_select_seeds(X, num_seeds, first_index, stepwise=False, _test_give_up=False, xb=None, metric="cosine"):
    """Farthest-point seeding.  X (n,64) unit rows (``metric`` "euclidean": any rows, distance ||x - s||_2, always one launch per
    step and never a give-up; fp32 only, ``xb`` is not used).  Returns (seeds (S,64), indices int64 (S,)).  The single-launch
    persistent kernel (maps up to 393 216 rows) needs its workgroups co-resident; if other work holds the CUs it gives up
    and every index is -1 -- callers re-issue with ``stepwise=True`` (mean_shift.mean_shift_smart_init does).
    ``xb`` (ms_pack_bf16(X); precision "bf16"): maps beyond the fp32 persistent kernel's reach work on the bf16 copy -- one
    persistent launch that keeps 917 504 rows on chip (VGPRs + LDS) and streams the rest per step, or (``stepwise``) one
    launch per step over the copy; distances are those of the rounded points, so the indices may differ from the fp32 path's."""
    _c(X, "X")
    n, d = X.shape
    if _ms_l2(metric, "ms_select_seeds"):
        if xb is not None:
            raise ValueError("ms_select_seeds: the bf16 copy (xb) serves the cosine metric only")
        seeds, idx = _ms_select_seeds(X[None], num_seeds, None, int(first_index), True, 0, metric)
        return seeds[0], idx[0]
    if xb is not None and n > 393216:
        _check_xb(xb, n, d, "ms_select_seeds")
        seeds = torch.empty((num_seeds, d), device=X.device, dtype=torch.float32)
        idx = torch.empty((num_seeds,), device=X.device, dtype=torch.int64)
        need = lib().msm_ms_seed_workspace(1, n)
        ws = torch.empty((need,), device=X.device, dtype=torch.float32)
        rc = lib().msm_ms_select_seeds_bf16(_p(xb), _p(X), n, d, num_seeds, int(first_index), _p(seeds), _p(idx), _p(ws), need,
                                            (1 if stepwise else 0) | (2 if _test_give_up else 0), _stream())
        check(rc, "msm_ms_select_seeds_bf16")
        return seeds, idx
    seeds, idx = _ms_select_seeds(X[None], num_seeds, None, int(first_index), stepwise, 1 if _test_give_up else 0)
    return seeds[0], idx[0]


def ms_hill_climb(X, Z, kappa, iters, precision="f32", xb=None, metric="cosine"):
    """iters x { Z = normalize(exp(kappa Z X^T) X) }; returns the updated copy of Z.  ``metric`` "euclidean": iters x
    { W = exp(-kappa ||z - x||^2), Z = W X / clamp(sum W, min=1) }, precision "f32" only (anything else raises ValueError).  precision "f32": fp32 MFMAs;
    "f32_split": fp32 results from six bf16 MFMAs per product on exact three-term splits (msm_ms_hill_climb_split);
    "bf16": single bf16 products over the bf16 copy ``xb`` = ms_pack_bf16(X) (made here when not given), seeds as h + l terms."""
    if precision not in ("f32", "f32_split", "bf16"):
        raise ValueError(f"ms_hill_climb: precision must be 'f32', 'f32_split' or 'bf16', not {precision!r}")
    if _ms_l2(metric, "ms_hill_climb") and precision != "f32":
        raise ValueError(f"ms_hill_climb: the Euclidean metric has the exact fp32 plan only, not precision={precision!r}")
    _c(X, "X"), _c(Z, "Z")
    if precision == "f32":
        return ms_hill_climb_batched(X[None], Z[None], kappa, iters, metric)[0]
    n, d = X.shape
    S = Z.shape[0]
    Z = Z.clone()
    if precision == "bf16":
        xb = ms_pack_bf16(X) if xb is None else _check_xb(xb, n, d, "ms_hill_climb")
        need = lib().msm_ms_hill_climb_workspace(n, S)
        ws = torch.empty((need,), device=X.device, dtype=torch.float32)
        check(lib().msm_ms_hill_climb_bf16(_p(xb), n, d, _p(Z), S, float(kappa), int(iters), _p(ws), need, _stream()), "msm_ms_hill_climb_bf16")
        return Z
    need = lib().msm_ms_hill_climb_split_workspace(n, S)
    ws = torch.empty((need,), device=X.device, dtype=torch.float32)
    check(lib().msm_ms_hill_climb_split(_p(X), n, d, _p(Z), S, float(kappa), int(iters), _p(ws), need, _stream()), "msm_ms_hill_climb_split")
    return Z


def ms_assign(X, Z, seed_labels, num_labels, metric="cosine"):
    """labels[i] = seed_labels[first argmin_s 0.5(1 - X_i.Z_s)] (``metric`` "euclidean": argmin_s ||X_i - Z_s||), counts = bincount(labels)."""
    labels, counts = ms_assign_batched(X[None], Z[None], seed_labels[None], num_labels, metric)
    return labels[0], counts[0]


def ms_connected_components(Z, epsilon, metric="cosine"):
    """mean_shift.py:41-76 on the device: Z (S,64) -> (seed_labels (S,) int64, num (2,) int32 = [labels that survive =
    len(unique(seed_labels)), labels created]).  ``metric`` "euclidean": membership ||z_j - z_i||_2 <= epsilon."""
    seed_labels, num = ms_connected_components_batched(Z[None], epsilon, metric)
    return seed_labels[0], num[0]


def ms_relabel_largest_zero(labels, counts, num_alive=None):
    """mean_shift.py:211-227 in place: label 0 <-> the first-argmax label of counts[:num], num = len(unique(seed_labels)) read from
    the device tensor ``num_alive`` (ms_connected_components()[1], or its first element alone) when given, else every entry of counts."""
    ms_relabel_largest_zero_batched(labels.view(1, -1), counts.view(1, -1), num_alive)
    return labels


# ---- M maps of one size per call (exact fp32 plan; the single-map ops above are their M = 1 views, "f32_split" / "bf16" are per map) ----
def _first_indices_device(first_indices, M, n, device, who):
    """int64 (M,) device tensor of first seed indices.  A host sequence / array / tensor is range-checked here; a device tensor is
    taken as it is (no host synchronisation; the kernel clamps into the map)."""
    if torch.is_tensor(first_indices) and first_indices.is_cuda:
        _c(first_indices, "first_indices", torch.int64)
        if first_indices.numel() != M:
            raise RuntimeError(f"{who}: {first_indices.numel()} first indices for {M} maps")
        return first_indices.reshape(M)
    host = torch.as_tensor(first_indices, dtype=torch.int64).reshape(-1)
    if host.numel() != M:
        raise RuntimeError(f"{who}: {host.numel()} first indices for {M} maps")
    if int(host.min()) < 0 or int(host.max()) >= n:
        raise RuntimeError(f"{who}: first indices must lie in [0, {n})")
    return host.to(device)


def ms_select_seeds_batched(X, num_seeds, first_indices, stepwise=False, _test_give_up=None, metric="cosine"):
    """ms_select_seeds for M maps of one size: X (M,n,64) unit rows, first_indices (M,) -> (seeds (M,S,64), indices int64 (M,S)),
    each map's bit-identical to ms_select_seeds(X[m], num_seeds, first_indices[m]).  Maps of 4096 .. 393 216 rows share grouped
    persistent launches (a map is held by cdiv(n, 1536) workgroups, as many maps per launch as the CUs hold); a group that loses
    co-residency reports -1 for its own map's indices only -- re-issue those maps with ``stepwise=True`` (one launch per step for
    all maps; mean_shift.mean_shift_smart_init_batched does).  ``_test_give_up``: maps whose give-up flag starts raised (tests).
    ``metric`` "euclidean": rows of any length, distance ||x - s||_2, one launch per step for every n -- no index is ever -1."""
    _c(X, "X")
    M, n, d = X.shape
    first = _first_indices_device(first_indices, M, n, X.device, "ms_select_seeds_batched")
    mask = 0
    for m in (_test_give_up or ()):
        if not 0 <= int(m) < min(M, 64):
            raise RuntimeError("ms_select_seeds_batched: _test_give_up names maps 0 .. min(M, 64) - 1")
        mask |= 1 << int(m)
    return _ms_select_seeds(X, num_seeds, first, 0, stepwise, mask, metric)


def ms_hill_climb_batched(X, Z, kappa, iters, metric="cosine"):
    """ms_hill_climb (precision "f32") for M maps: X (M,n,64), Z (M,S,64) -> the updated copy of Z; a map's result does not depend
    on its neighbours (same per-map grid, slab walk and summation order for every M), with either ``metric``."""
    _c(X, "X"), _c(Z, "Z")
    M, n, d = X.shape
    if Z.dim() != 3 or Z.shape[0] != M or Z.shape[2] != d:
        raise RuntimeError(f"ms_hill_climb_batched: Z has shape {tuple(Z.shape)}, expected ({M}, S, {d})")
    S = Z.shape[1]
    Z = Z.clone()
    if _ms_l2(metric, "ms_hill_climb_batched"):
        need = M * lib().msm_ms_hill_climb_l2_workspace(n, S)
        ws = torch.empty((need,), device=X.device, dtype=torch.float32)
        check(lib().msm_ms_hill_climb_l2(_p(X), M, n, d, _p(Z), S, float(kappa), int(iters), _p(ws), need, _stream()), "msm_ms_hill_climb_l2")
        return Z
    need = M * lib().msm_ms_hill_climb_workspace(n, S)
    ws = torch.empty((need,), device=X.device, dtype=torch.float32)
    check(lib().msm_ms_hill_climb(_p(X), M, n, d, _p(Z), S, float(kappa), int(iters), _p(ws), need, _stream()), "msm_ms_hill_climb")
    return Z


def ms_assign_batched(X, Z, seed_labels, num_labels, metric="cosine"):
    """ms_assign for M maps: X (M,n,64), Z (M,S,64), seed_labels int64 (M,S) -> (labels int64 (M,n), counts int64 (M,num_labels))."""
    _c(X, "X"), _c(Z, "Z"), _c(seed_labels, "seed_labels", torch.int64)
    M, n, d = X.shape
    if Z.dim() != 3 or Z.shape[0] != M or Z.shape[2] != d or tuple(seed_labels.shape) != tuple(Z.shape[:2]):
        raise RuntimeError(f"ms_assign_batched: Z {tuple(Z.shape)} / seed_labels {tuple(seed_labels.shape)} do not match X {tuple(X.shape)}")
    labels = torch.empty((M, n), device=X.device, dtype=torch.int64)
    counts = torch.empty((M, num_labels), device=X.device, dtype=torch.int64)
    name = "msm_ms_assign_l2" if _ms_l2(metric, "ms_assign_batched") else "msm_ms_assign"
    rc = getattr(lib(), name)(_p(X), M, n, d, _p(Z), Z.shape[1], _p(seed_labels), _p(labels), _p(counts), num_labels, _stream())
    check(rc, name)
    return labels, counts


def ms_connected_components_batched(Z, epsilon, metric="cosine"):
    """ms_connected_components for M seed sets, one wave each: Z (M,S,64) -> (seed_labels int64 (M,S), num int32 (M,2))."""
    _c(Z, "Z")
    M, S, d = Z.shape
    seed_labels = torch.empty((M, S), device=Z.device, dtype=torch.int64)
    num = torch.empty((M, 2), device=Z.device, dtype=torch.int32)
    name = "msm_ms_connected_components_l2" if _ms_l2(metric, "ms_connected_components_batched") else "msm_ms_connected_components"
    check(getattr(lib(), name)(_p(Z), M, S, d, float(epsilon), _p(seed_labels), _p(num), _stream()), name)
    return seed_labels, num


def ms_relabel_largest_zero_batched(labels, counts, num_alive=None):
    """ms_relabel_largest_zero per map, in place: labels int64 (M,n), counts int64 (M,num_labels), num_alive int32 (M,2)
    (ms_connected_components_batched()[1]) or None.  Map m reads num_alive[m][0] only, so one map may pass that element alone."""
    _c(labels, "labels", torch.int64), _c(counts, "counts", torch.int64), _c(num_alive, "num_alive", torch.int32)
    M, n = labels.shape
    if counts.dim() != 2 or counts.shape[0] != M:
        raise RuntimeError(f"ms_relabel_largest_zero_batched: counts has shape {tuple(counts.shape)}, expected ({M}, num_labels)")
    if num_alive is not None and tuple(num_alive.shape) != (M, 2) and not (M == 1 and num_alive.numel() >= 1):
        raise RuntimeError(f"ms_relabel_largest_zero_batched: num_alive has shape {tuple(num_alive.shape)}, expected ({M}, 2) "
                           "(one map may pass its count alone: any tensor with at least one element)")
    rc = lib().msm_ms_relabel_largest_zero(_p(labels), M, n, _p(counts), counts.shape[1], _p(num_alive), _stream())
    check(rc, "msm_ms_relabel_largest_zero")
    return labels


# ----------------------------------------------------------------------------------------------
# instance post-processing (pretrained_meanshiftformer_model.py:337-343, 461-497)
# ----------------------------------------------------------------------------------------------
def topk_class_scores(pred_logits, topk, gather=None, gather_cols=None):
    """Top-K (query, class) pairs of softmax(pred_logits)[..., :-1] per image (PM:461-470): (scores (B,T), classes (B,T) int64,
    query index (B,T) int32).  ``gather``: a (B, Q, >= gather_cols) per-query matrix with unit column stride; the selected rows'
    leading ``gather_cols`` columns come back as a fourth result (B, T, gather_cols), copied by the same launch."""
    _c(pred_logits, "pred_logits")
    B, Q, K1 = pred_logits.shape
    dev = pred_logits.device
    scores = torch.empty((B, topk), device=dev, dtype=torch.float32)
    classes = torch.empty((B, topk), device=dev, dtype=torch.int64)
    qidx = torch.empty((B, topk), device=dev, dtype=torch.int32)
    if gather is None:
        rc = lib().msm_topk_class_scores(_p(pred_logits), B, Q, K1, topk, _p(scores), _p(classes), _p(qidx), _stream())
        check(rc, "msm_topk_class_scores")
        return scores, classes, qidx
    _chk(gather, "gather")
    cols = int(gather_cols)
    if gather.dim() != 3 or gather.shape[0] != B or gather.shape[1] != Q or gather.shape[2] < cols or gather.stride(2) != 1 \
            or (B > 1 and gather.stride(0) != Q * gather.stride(1)):
        raise RuntimeError("gather must be (B, Q, >= gather_cols) with unit column stride and uniformly spaced rows")
    sel = torch.empty((B, topk, cols), device=dev, dtype=torch.float32)
    rc = lib().msm_topk_class_scores_gather(_p(pred_logits), B, Q, K1, topk, _p(scores), _p(classes), _p(qidx), _p(gather),
                                            gather.stride(1), cols, _p(sel), _stream())
    check(rc, "msm_topk_class_scores_gather")
    return scores, classes, qidx, sel


def instance_postprocess(mask_logits, query_index, image_size, class_scores=None, padded_size=None, output_size=None):
    """mask_logits (B,Q,h,w), query_index int32 (B,T) -> (pred_masks (B,T,H,W) float 0/1,
    score (B,T) = mean mask probability [* class_scores], boxes (B,T,4)).  The logits are upsampled to ``padded_size``
    (the frame the network saw, default = image_size) and cropped to image_size = (H, W), as the reference does for
    inputs padded to the size divisibility (PM:337-343 + sem_seg_postprocess, PM:354-357).  ``output_size`` (OH, OW) other than
    image_size: the cropped logits are interpolated a second time to that size (sem_seg_postprocess's resize, the "height" /
    "width" of a sample whose image was resized for the network) and masks (B,T,OH,OW), scores and boxes are taken there, in
    one pass (msm_instance_postprocess_resized)."""
    _c(mask_logits, "mask_logits"), _c(query_index, "query_index", torch.int32), _c(class_scores, "class_scores")
    B, Q, h, w = mask_logits.shape
    T = query_index.shape[1]
    H, W = int(image_size[0]), int(image_size[1])
    Hs, Ws = (H, W) if padded_size is None else (int(padded_size[0]), int(padded_size[1]))
    OH, OW = (H, W) if output_size is None else (int(output_size[0]), int(output_size[1]))
    if OH <= 0 or OW <= 0:
        raise RuntimeError(f"instance_postprocess: output_size {OH}x{OW} must be positive")
    dev = mask_logits.device
    masks = torch.empty((B, T, OH, OW), device=dev, dtype=torch.float32)
    score = torch.empty((B, T), device=dev, dtype=torch.float32)
    boxes = torch.empty((B, T, 4), device=dev, dtype=torch.float32)
    ws = torch.empty((int(lib().msm_instance_postprocess_workspace(B, T, OH, OW)),), device=dev, dtype=torch.float32)
    if (OH, OW) == (H, W):
        rc = lib().msm_instance_postprocess(_p(mask_logits), _p(query_index), _p(class_scores), _p(masks), _p(score), _p(boxes),
                                            B, Q, T, h, w, H, W, Hs, Ws, _p(ws), _stream())
        check(rc, "msm_instance_postprocess")
    else:
        rc = lib().msm_instance_postprocess_resized(_p(mask_logits), _p(query_index), _p(class_scores), _p(masks), _p(score),
                                                    _p(boxes), B, Q, T, h, w, H, W, Hs, Ws, OH, OW, _p(ws), _stream())
        check(rc, "msm_instance_postprocess_resized")
    return masks, score, boxes


def label_stats(labels, weight=None, k=1024):
    """labels (B,H,W) float32 with integer values in [0,k), weight (B,H,W) float32 or None ->
    (stats (B,k,5) int32 = area, x_min, y_min, x_max, y_max; wsum (B,k) float32; overflow (B,) int32)."""
    _c(labels, "labels"), _c(weight, "weight")
    B, H, W = labels.shape
    dev = labels.device
    stats = torch.empty((B, k, 5), device=dev, dtype=torch.int32)
    wsum = torch.empty((B, k), device=dev, dtype=torch.float32)
    overflow = torch.empty((B,), device=dev, dtype=torch.int32)
    rc = lib().msm_label_stats(_p(labels), _p(weight), _p(stats), _p(wsum), _p(overflow), B, H, W, int(k), _stream())
    check(rc, "msm_label_stats")
    return stats, wsum, overflow



def eval_counts_row(L):
    """int32 values per image of msm_eval_counts' counts table at label capacity L."""
    return 8 + 6 * int(L) + 3 * int(L) * int(L)


def eval_counts(pred, gt, radius, L=64):
    """Integer counts of multilabel_metrics for B pairs of label images (msm_eval_counts): pred, gt (B,H,W) float32 with
    integer values in [0, 1024), disk radius `radius` -> counts (B, eval_counts_row(L)) int32 laid out as include/msm_hip.h
    documents (header, label tables, tp / fgm / gtm [L][L])."""
    _c(pred, "pred"), _c(gt, "gt")
    if pred.shape != gt.shape or pred.dim() != 3:
        raise RuntimeError(f"eval_counts: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} must be the same (B,H,W)")
    B, H, W = pred.shape
    dev = pred.device
    counts = torch.empty((B, eval_counts_row(L)), device=dev, dtype=torch.int32)
    nbytes = lib().msm_eval_counts_workspace(B)
    ws = torch.empty((max(1, nbytes // 4),), device=dev, dtype=torch.int32)
    check(lib().msm_eval_counts(_p(pred), _p(gt), _p(counts), _p(ws), nbytes, B, H, W, int(radius), int(L), _stream()),
          "msm_eval_counts")
    return counts


# ---- set criterion (criterion.py): matching costs and point-sampled mask losses of every prediction of one call ----
def _device_table(values, dev):
    """int64 table (pointers, offsets) -> device, by a pinned host-to-device copy (no sync)."""
    host = torch.tensor(values, dtype=torch.int64).pin_memory()
    return host.to(dev, non_blocking=True)


def _check_preds(tensors, name, ndim):
    if not tensors:
        raise RuntimeError(f"{name}: at least one prediction is needed")
    for i, t in enumerate(tensors):
        _c(t, f"{name}[{i}]")
        if t.dim() != ndim or t.shape != tensors[0].shape or t.device != tensors[0].device:
            raise RuntimeError(f"{name}[{i}]: shape {tuple(t.shape)} / {t.device} differs from {name}[0] "
                               f"{tuple(tensors[0].shape)} / {tensors[0].device}")


def _check_targets(tgt, dev):
    _c(tgt, "tgt_masks", torch.uint8)
    if tgt.dim() != 3 or tgt.device != dev:
        raise RuntimeError(f"tgt_masks must be (T, Hg, Wg) uint8 on {dev}, got {tuple(tgt.shape)} on {tgt.device}")


def match_cost(logits, masks, tgt_masks, labels, toff, points, w_class=1.0, w_mask=1.0, w_dice=1.0):
    """The matcher's cost matrices of every (prediction, image) in one launch (msm_match_cost).  logits: list of (B,Q,C+1),
    masks: list of (B,Q,Hm,Wm) fp32 (one entry per prediction, not stacked), tgt_masks (T,Hg,Wg) uint8 0/1 targets of the
    whole batch, labels (T,) int32, toff: B + 1 host ints (image b's targets are rows toff[b]..toff[b+1]), points
    (n_pred,B,P,2) -> cost (n_pred,Q,T): image b's matrix is cost[:, :, toff[b]:toff[b+1]]."""
    _check_preds(logits, "logits", 3), _check_preds(masks, "masks", 4)
    dev = masks[0].device
    n_pred = len(masks)
    B, Q, C1 = logits[0].shape
    _, _, Hm, Wm = masks[0].shape
    if len(logits) != n_pred or masks[0].shape[:2] != (B, Q) or logits[0].device != dev:
        raise RuntimeError("match_cost: logits and masks must be per-prediction lists of (B,Q,C+1) / (B,Q,Hm,Wm)")
    _check_targets(tgt_masks, dev)
    _c(labels, "labels", torch.int32), _c(points, "points")
    toff = [int(v) for v in toff]
    TT = tgt_masks.shape[0]
    if len(toff) != B + 1 or toff[0] != 0 or toff[-1] != TT or any(b < a for a, b in zip(toff, toff[1:])):
        raise RuntimeError(f"match_cost: toff {toff} does not partition {TT} targets over {B} images")
    if labels.shape != (TT,) or points.dim() != 4 or points.shape[:2] != (n_pred, B) or points.shape[3] != 2:
        raise RuntimeError(f"match_cost: labels {tuple(labels.shape)} / points {tuple(points.shape)} do not fit")
    P = points.shape[2]
    max_T = max([b - a for a, b in zip(toff, toff[1:])] + [0])
    cost = torch.empty((n_pred, Q, TT), device=dev, dtype=torch.float32)
    table = _device_table([t.data_ptr() for t in logits] + [t.data_ptr() for t in masks] + toff, dev)
    check(lib().msm_match_cost(_p(table), _p(tgt_masks), _p(labels), _p(points), _p(cost), n_pred, B, Q, C1, Hm, Wm,
                               tgt_masks.shape[1], tgt_masks.shape[2], P, TT, max_T, float(w_class), float(w_mask),
                               float(w_dice), _stream()), "msm_match_cost")
    return cost


LSAP_MAX_DIM = 1024     # MSM_LSAP_MAX_DIM: rows / columns of one assignment problem of msm_lsap_match


def lsap_match(cost, toff, labels, no_object, out=None):
    """The assignments of every (prediction, image) cost matrix of match_cost, solved on the device (msm_lsap_match), exactly
    as criterion.lsap_numpy solves them.  cost (n_pred,Q,T) fp32 as match_cost returns it, toff: B + 1 host ints, labels (T,)
    int32, no_object: the class of an unmatched query -> (pairs (n_pred*N,4) int32 rows (prediction, n, b*Q+q, target row) as
    point_loss_fwd reads them, N = sum_b min(Q, T_b), images in order and q ascending; target_classes (n_pred,B,Q) int64;
    status (n_pred,B) int32: 0 solved, 1 nan / -inf in the matrix, 2 infeasible, 3 a loop bound was hit; a problem with a
    non-zero status holds the pairs (q = j, target j)).  out: (pairs, target_classes, status) tensors to write into.
    Nothing here waits for the GPU: the statuses are for the caller to read when it chooses to."""
    if cost.dim() != 3:
        raise RuntimeError(f"lsap_match: cost must be (n_pred, Q, T), got {tuple(cost.shape)}")
    n_pred, Q, TT = cost.shape
    toff = [int(v) for v in toff]
    B = len(toff) - 1
    if B < 0 or toff[0] != 0 or toff[-1] != TT or any(b < a for a, b in zip(toff, toff[1:])):
        raise RuntimeError(f"lsap_match: toff {toff} does not partition {TT} targets")
    counts = [b - a for a, b in zip(toff, toff[1:])]
    max_T = max(counts + [0])
    if max(Q, max_T) > LSAP_MAX_DIM:
        raise ValueError(f"lsap_match: {Q} queries x {max_T} targets: one side exceeds the supported {LSAP_MAX_DIM}")
    if n_pred < 1 or Q < 1:
        raise RuntimeError(f"lsap_match: cost {tuple(cost.shape)} needs at least one prediction and one query")
    _c(cost, "cost"), _c(labels, "labels", torch.int32)
    dev = cost.device
    if labels.shape != (TT,) or labels.device != dev:
        raise RuntimeError(f"lsap_match: labels {tuple(labels.shape)} on {labels.device} must be ({TT},) on {dev}")
    poff = [0]
    for t in counts:
        poff.append(poff[-1] + min(Q, t))
    N = poff[-1]
    if out is None:
        pairs = torch.empty((n_pred * N, 4), device=dev, dtype=torch.int32)
        target_classes = torch.empty((n_pred, B, Q), device=dev, dtype=torch.int64)
        status = torch.empty((n_pred, B), device=dev, dtype=torch.int32)
    else:
        pairs, target_classes, status = out
        _c(pairs, "pairs", torch.int32), _c(target_classes, "target_classes", torch.int64), _c(status, "status", torch.int32)
        if (pairs.shape != (n_pred * N, 4) or target_classes.shape != (n_pred, B, Q) or status.shape != (n_pred, B)
                or {pairs.device, target_classes.device, status.device} != {dev}):
            raise RuntimeError(f"lsap_match: out must be ({n_pred * N}, 4) int32, ({n_pred}, {B}, {Q}) int64 and ({n_pred}, {B}) "
                               f"int32 on {dev}")
    table = _device_table(toff + poff, dev)
    check(lib().msm_lsap_match(_p(cost), _p(table), _p(labels), _p(pairs), _p(target_classes), _p(status), n_pred, B, Q, TT,
                               max_T, N, int(no_object), _stream()), "msm_lsap_match")
    return pairs, target_classes, status


def _point_loss_args(masks, tgt_masks, pairs, os_points, rnd_points, k):
    _check_preds(masks, "masks", 4)
    dev = masks[0].device
    _check_targets(tgt_masks, dev)
    _c(pairs, "pairs", torch.int32), _c(os_points, "os_points"), _c(rnd_points, "rnd_points")
    n_pred = len(masks)
    B, Q, Hm, Wm = masks[0].shape
    N = os_points.shape[1] if os_points.dim() == 4 else -1
    Pos = os_points.shape[2] if os_points.dim() == 4 else -1
    if (os_points.dim() != 4 or os_points.shape[0] != n_pred or os_points.shape[3] != 2 or rnd_points.dim() != 4
            or rnd_points.shape[:2] != (n_pred, N) or rnd_points.shape[3] != 2 or pairs.shape != (n_pred * N, 4)):
        raise RuntimeError(f"point_loss: os_points {tuple(os_points.shape)}, rnd_points {tuple(rnd_points.shape)} and pairs "
                           f"{tuple(pairs.shape)} must be (n_pred,N,Pos,2), (n_pred,N,P-k,2), (n_pred*N,4)")
    P = int(k) + rnd_points.shape[2]
    if not 0 <= int(k) <= Pos:
        raise RuntimeError(f"point_loss: k={k} outside [0, {Pos}]")
    return dev, n_pred, N, B * Q, Hm, Wm, Pos, P


def point_loss_workspace_bytes(n_pairs, k):
    return int(lib().msm_point_loss_workspace(int(n_pairs), int(k)))


def point_loss_fwd(masks, tgt_masks, pairs, os_points, rnd_points, k, num_masks):
    """loss_masks of every prediction in one pass (msm_point_loss_fwd): masks list of (B,Q,Hm,Wm) fp32, tgt_masks (T,Hg,Wg)
    uint8, pairs (n_pred*N,4) int32 rows (prediction, n, b*Q+q, target row), os_points (n_pred,N,Pos,2), rnd_points
    (n_pred,N,P-k,2), k selected points per mask -> (losses (2,n_pred) = loss_mask, loss_dice; sel_bits (n_pred*N,
    ceil(Pos/32)) int32 selection bitmaps; workspace for point_loss_bwd)."""
    dev, n_pred, N, BQ, Hm, Wm, Pos, P = _point_loss_args(masks, tgt_masks, pairs, os_points, rnd_points, k)
    n_pairs = n_pred * N
    losses = torch.empty((2, n_pred), device=dev, dtype=torch.float32)
    bits = torch.empty((n_pairs, (Pos + 31) // 32), device=dev, dtype=torch.int32)
    nbytes = point_loss_workspace_bytes(n_pairs, k)
    ws = torch.empty((max(1, nbytes // 4),), device=dev, dtype=torch.int32)
    table = _device_table([t.data_ptr() for t in masks], dev)
    check(lib().msm_point_loss_fwd(_p(table), _p(tgt_masks), _p(pairs), _p(os_points), _p(rnd_points), _p(losses), _p(bits),
                                   _p(ws), nbytes, n_pred, N, BQ, tgt_masks.shape[0], Hm, Wm, tgt_masks.shape[1],
                                   tgt_masks.shape[2], Pos, int(k), P, float(num_masks), _stream()), "msm_point_loss_fwd")
    return losses, bits, ws


def point_loss_bwd(masks, tgt_masks, pairs, os_points, rnd_points, workspace, grad_losses, k, num_masks, global_atomics=False):
    """Gradient of point_loss_fwd's losses (msm_point_loss_bwd): grad_losses (2,n_pred) -> list of (B,Q,Hm,Wm) gradients, zero
    outside the matched masks.  global_atomics forces the global float-atomic scatter (the path of masks above 128 KiB)."""
    dev, n_pred, N, BQ, Hm, Wm, Pos, P = _point_loss_args(masks, tgt_masks, pairs, os_points, rnd_points, k)
    _c(grad_losses, "grad_losses")
    _c(workspace, "workspace", torch.int32)
    if grad_losses.shape != (2, n_pred):
        raise RuntimeError(f"point_loss_bwd: grad_losses {tuple(grad_losses.shape)} must be (2, {n_pred})")
    grads = [torch.zeros_like(m) for m in masks]
    nbytes = point_loss_workspace_bytes(n_pred * N, k)
    if workspace.numel() * 4 < nbytes:
        raise RuntimeError(f"point_loss_bwd: workspace of {workspace.numel() * 4} bytes, {nbytes} needed")
    table = _device_table([t.data_ptr() for t in masks] + [t.data_ptr() for t in grads], dev)
    check(lib().msm_point_loss_bwd(_p(table), _p(tgt_masks), _p(pairs), _p(os_points), _p(rnd_points), _p(workspace), nbytes,
                                   _p(grad_losses), n_pred, N, BQ, tgt_masks.shape[0], Hm, Wm, tgt_masks.shape[1],
                                   tgt_masks.shape[2], Pos, int(k), P, float(num_masks), 1 if global_atomics else 0,
                                   _stream()), "msm_point_loss_bwd")
    return grads


def label_image(masks, inst_labels):
    """masks (B,K,H,W) float (non-zero = inside), inst_labels (B,K) float -> (B,H,W) float label images (msm_label_image)."""
    _c(masks, "masks"), _c(inst_labels, "inst_labels")
    B, K, H, W = masks.shape
    out = torch.empty((B, H, W), device=masks.device, dtype=torch.float32)
    check(lib().msm_label_image(_p(masks), _p(inst_labels), _p(out), B, K, H, W, _stream()), "msm_label_image")
    return out


def mask_nms_workspace_bytes(B, K, H, W):
    """Bytes of workspace msm_mask_nms needs for masks (B,K,H,W) (bit planes + the intersection matrix)."""
    n = lib().msm_mask_nms_workspace(int(B), int(K), int(H), int(W))
    if n < 0:
        check(int(n), "msm_mask_nms_workspace")
    return int(n)


def mask_nms(masks, scores, candidate, thresh=0.7, workspace=None):
    """Mask NMS of B images in five launches without a host synchronisation (msm_mask_nms; the definition is in
    include/msm_hip.h and two_stage.combine_masks_with_NMS_batched): masks (B,K,H,W) float32 (non-zero = inside), scores (B,K)
    float32, candidate (B,K) bool or uint8 -> (label (B,H,W) float32, score (B,H,W) float32, bbox (B,K,5) float32, count (B,)
    int32, inst_labels (B,K) int32).  ``workspace``: a uint8 tensor of at least mask_nms_workspace_bytes(B,K,H,W) bytes that a
    caller replaying the launches from a HIP graph owns; allocated here when None."""
    _c(masks, "masks"), _c(scores, "scores")
    if candidate is not None and candidate.dtype == torch.bool:
        candidate = candidate.view(torch.uint8)
    _c(candidate, "candidate", torch.uint8)
    if candidate is None:
        raise RuntimeError("candidate must be a (B,K) bool or uint8 tensor on the GPU")
    B, K, H, W = masks.shape
    if tuple(scores.shape) != (B, K) or tuple(candidate.shape) != (B, K):
        raise RuntimeError(f"scores / candidate must be (B,K) = ({B},{K}), got {tuple(scores.shape)} / {tuple(candidate.shape)}")
    dev = masks.device
    need = mask_nms_workspace_bytes(B, K, H, W)
    if workspace is None:
        workspace = torch.empty(need, device=dev, dtype=torch.uint8)
    _c(workspace, "workspace", torch.uint8)
    label = torch.empty((B, H, W), device=dev, dtype=torch.float32)
    score_img = torch.empty((B, H, W), device=dev, dtype=torch.float32)
    bbox = torch.empty((B, K, 5), device=dev, dtype=torch.float32)
    count = torch.empty((B,), device=dev, dtype=torch.int32)
    inst_labels = torch.empty((B, K), device=dev, dtype=torch.int32)
    rc = lib().msm_mask_nms(_p(masks), _p(scores), _p(candidate), float(thresh), _p(label), _p(score_img), _p(bbox), _p(count),
                            _p(inst_labels), _p(workspace), workspace.numel(), B, K, H, W, _stream())
    check(rc, "msm_mask_nms")
    return label, score_img, bbox, count, inst_labels


EMBLOSS_METRICS = {"cosine": 0, "euclidean": 1}
EMBLOSS_TABLE_FLOATS = 16384     # max_clusters * C: the per-wave table of msm_embloss_fwd in LDS (64 KiB)
EMBLOSS_MAX_CLUSTERS = 1024


def embloss_max_clusters(C, max_clusters=None):
    """The cluster-table rows of msm_embloss_fwd for C channels: min(64, 16384 // C) by default; a request the table cannot hold
    raises ValueError (before any launch)."""
    C = int(C)
    if C < 1:
        raise ValueError(f"EmbeddingLoss: C must be at least 1, got {C}")
    if max_clusters is None:
        max_clusters = min(64, EMBLOSS_TABLE_FLOATS // C)
    max_clusters = int(max_clusters)
    if max_clusters < 1 or max_clusters > EMBLOSS_MAX_CLUSTERS or max_clusters * C > EMBLOSS_TABLE_FLOATS:
        raise ValueError(f"EmbeddingLoss: max_clusters = {max_clusters} with C = {C} is outside 1 <= max_clusters <= "
                         f"{EMBLOSS_MAX_CLUSTERS}, max_clusters * C <= {EMBLOSS_TABLE_FLOATS} (the cluster table lives in LDS)")
    return max_clusters


def embloss_workspace_bytes(B, C, HW, max_clusters):
    """Bytes of workspace msm_embloss_fwd / _bwd need (partial tables, centres, centre-path vectors)."""
    n = lib().msm_embloss_workspace(int(B), int(C), int(HW), int(max_clusters))
    if n < 0:
        check(int(n), "msm_embloss_workspace")
    return int(n)


def _embloss_args(x, labels, max_clusters, metric):
    if metric not in EMBLOSS_METRICS:
        raise ValueError(f"EmbeddingLoss: metric must be 'cosine' or 'euclidean', got {metric!r}")
    if x.dim() != 4:
        raise RuntimeError(f"x must be (B,C,H,W), got {tuple(x.shape)}")
    B, C, H, W = x.shape
    Kt = embloss_max_clusters(C, max_clusters)          # the size limits raise first: they need no device
    _chk(x, "x"), _chk(labels, "labels")
    if B < 1 or H * W < 1 or labels.numel() != B * H * W:
        raise RuntimeError(f"x (B,C,H,W) = {tuple(x.shape)} needs B, H W >= 1 and labels (B,1,H,W), got {tuple(labels.shape)}")
    _c(x, "x"), _c(labels, "labels")
    return B, C, H * W, Kt


def embloss_fwd(x, labels, alpha, delta, lambda_intra, lambda_inter, metric="cosine", normalize=True, max_clusters=None,
                workspace=None):
    """msm_embloss_fwd (the definition is in include/msm_hip.h): x (B,C,H,W) float32, labels (B,1,H,W) or (B,H,W) float32, both
    contiguous on the GPU -> (losses (3,) = loss, intra, inter; info int32; workspace), six launches, no host synchronisation.
    ``info`` = [K, status, branch flag, 0, n (B,Kt), N (B,Kt)] (embloss_info splits it); the workspace holds what embloss_bwd
    reads, so a caller that passes its own (a uint8 tensor of embloss_workspace_bytes(...) bytes, for a HIP graph) must run the
    backward before the next forward on it."""
    B, C, HW, Kt = _embloss_args(x, labels, max_clusters, metric)
    need = embloss_workspace_bytes(B, C, HW, Kt)
    if workspace is None:
        workspace = torch.empty(need, device=x.device, dtype=torch.uint8)
    _c(workspace, "workspace", torch.uint8)
    losses = torch.empty(3, device=x.device, dtype=torch.float32)
    info = torch.empty(4 + 2 * B * Kt, device=x.device, dtype=torch.int32)
    rc = lib().msm_embloss_fwd(_p(x), _p(labels), _p(losses), _p(info), _p(workspace), workspace.numel(), B, C, HW, Kt,
                               EMBLOSS_METRICS[metric], int(bool(normalize)), float(alpha), float(delta), float(lambda_intra),
                               float(lambda_inter), _stream())
    check(rc, "msm_embloss_fwd")
    return losses, info, workspace


def embloss_bwd(x, labels, grad_losses, workspace, metric="cosine", max_clusters=None):
    """msm_embloss_bwd: grad_losses (3,) float32 on the GPU (d/d loss, intra, inter) and the workspace of the forward on the
    same x and labels -> grad_x, one launch."""
    B, C, HW, Kt = _embloss_args(x, labels, max_clusters, metric)
    _c(grad_losses, "grad_losses"), _c(workspace, "workspace", torch.uint8)
    if grad_losses.numel() != 3:
        raise RuntimeError(f"grad_losses must hold 3 values, got {tuple(grad_losses.shape)}")
    grad_x = torch.empty_like(x)
    rc = lib().msm_embloss_bwd(_p(x), _p(labels), _p(grad_losses), _p(workspace), workspace.numel(), _p(grad_x), B, C, HW, Kt,
                               EMBLOSS_METRICS[metric], _stream())
    check(rc, "msm_embloss_bwd")
    return grad_x


def embloss_info(info, B):
    """info of embloss_fwd -> dict(K, status, flag: 0-d int32 views; n, N: (B, max_clusters) int32 views).  Device tensors:
    reading them synchronises (tests and EmbeddingLoss.check())."""
    Kt = (info.numel() - 4) // (2 * B)
    return dict(K=info[0], status=info[1], flag=info[2], n=info[4:4 + B * Kt].view(B, Kt), N=info[4 + B * Kt:].view(B, Kt))


# ---- optimizers (optim.py): clip_grad_norm_ + AdamW, Adam or SGD over a device-resident table of tensors, step counts on the device ----
OPTIM_REC = 8           # int64 per tensor record: p, g, exp_avg, exp_avg_sq addresses, numel, row (of hyper and steps), flags, 0
OPTIM_HYP = 8           # doubles per hyper-parameter row: lr, weight_decay, beta1, beta2, eps, momentum, dampening, nesterov
OPTIM_ALIGNED = 1       # MSM_OPTIM_ALIGNED: p, g, exp_avg and exp_avg_sq are all 16-byte aligned
OPTIM_ALIGNED_G = 2     # MSM_OPTIM_ALIGNED_G: g is


def optim_chunk():
    """MSM_OPTIM_CHUNK: the elements of one chunk of the optimizer's chunk list (one workgroup's work)."""
    return int(lib().msm_optim_chunk())


def _optim_tables(tensors, chunks, n_tensors, n_chunks):
    _c(tensors, "tensors", torch.int64), _c(chunks, "chunks", torch.int64)
    if n_tensors < 1 or tensors.numel() < n_tensors * OPTIM_REC or n_chunks < n_tensors or chunks.numel() < 2 * n_chunks:
        raise RuntimeError(f"optimizer tables: {n_tensors} records need {n_tensors * OPTIM_REC} int64 (got {tensors.numel()}), "
                           f"{n_chunks} chunks need {2 * n_chunks} (got {chunks.numel()}), every tensor has a chunk")


OPTIM_RULES = {"adamw": 0, "adam": 1, "sgd": 2}        # MSM_OPTIM_ADAMW, MSM_OPTIM_ADAM, MSM_OPTIM_SGD


def _optim_scalar(t, name, device):
    """grad_scale / found_inf as GradScaler sets them: one float32 on the tables' device, or None.  The value is never read here."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.numel() != 1 or t.device != device:
        raise RuntimeError(f"optimizer: {name} must be one torch.float32 element on {device}, got "
                           f"{tuple(t.shape)} {t.dtype} on {t.device}" if isinstance(t, torch.Tensor) else
                           f"optimizer: {name} must be a tensor, got {type(t).__name__}")
    return t.data_ptr()


def optim_count_norm(tensors, chunks, partials, steps, n_tensors, n_chunks, n_rows, grad_scale=None, found_inf=None):
    """msm_optim_count_norm: partials[c] = sum of (g / grad_scale)^2 over chunk c (double) and steps[row] += 1 for every tensor of
    the table unless found_inf says the step is skipped, one launch.  tensors / chunks: int64 device tables in the layout of
    include/msm_hip.h, partials float64 (n_chunks,), steps int64 (n_rows,)."""
    _optim_tables(tensors, chunks, n_tensors, n_chunks)
    _c(partials, "partials", torch.float64), _c(steps, "steps", torch.int64)
    if partials.numel() < n_chunks or n_rows < 1 or steps.numel() < n_rows:
        raise RuntimeError(f"optim_count_norm: partials needs {n_chunks} doubles (got {partials.numel()}), steps {n_rows} int64 "
                           f"(got {steps.numel()})")
    check(lib().msm_optim_count_norm(_p(tensors), _p(chunks), _p(partials), _p(steps), _optim_scalar(grad_scale, "grad_scale", tensors.device),
                                     _optim_scalar(found_inf, "found_inf", tensors.device), n_tensors, n_chunks, n_rows, _stream()),
          "msm_optim_count_norm")


def optim_update(rule, tensors, chunks, hyper, partials, state, steps, n_tensors, n_chunks, n_rows, max_norm, grad_scale=None,
                 found_inf=None):
    """msm_optim_update: the update of `rule` ("adamw", "adam", "sgd") on every chunk with step = steps[row], the gradient unscaled
    by grad_scale and the whole step skipped on found_inf, one launch (two with max_norm <= 0: the counts move in a launch of their
    own and partials may be None).  hyper float64 (n_rows, 8), state int64 (2,), steps int64 (n_rows,)."""
    _optim_tables(tensors, chunks, n_tensors, n_chunks)
    _c(hyper, "hyper", torch.float64), _c(partials, "partials", torch.float64), _c(state, "state", torch.int64)
    _c(steps, "steps", torch.int64)
    if n_rows < 1 or hyper.numel() < n_rows * OPTIM_HYP or state.numel() < 2 or steps.numel() < n_rows or (
            max_norm > 0 and (partials is None or partials.numel() < n_chunks)):
        raise RuntimeError(f"optim_update: {n_rows} rows need {n_rows * OPTIM_HYP} doubles (got {hyper.numel()}) and {n_rows} step "
                           f"counts (got {steps.numel()}), state 2 int64, max_norm > 0 partials of {n_chunks} doubles")
    check(lib().msm_optim_update(OPTIM_RULES[rule], _p(tensors), _p(chunks), _p(hyper), _p(partials), _p(state), _p(steps),
                                 _optim_scalar(grad_scale, "grad_scale", tensors.device),
                                 _optim_scalar(found_inf, "found_inf", tensors.device), n_tensors, n_chunks, n_rows, float(max_norm),
                                 _stream()), "msm_optim_update")


def optim_zero(tensors, chunks, n_tensors, n_chunks):
    """msm_optim_zero: g = 0 for every chunk of the table, one launch."""
    _optim_tables(tensors, chunks, n_tensors, n_chunks)
    check(lib().msm_optim_zero(_p(tensors), _p(chunks), n_tensors, n_chunks, _stream()), "msm_optim_zero")


def crop_resize(rgb, depth, labels, table, size):
    """ROI crops of a batch of frames in one launch (msm_crop_resize): rgb / depth (F,3,H,W), labels (F,H,W) float, table (N,8)
    int32 rows (frame, label, x0, y0, x1, y1, 0, 0) -> (rgb_crops (N,3,S,S), mask_crops (N,S,S), depth_crops or None)."""
    _c(rgb, "rgb"), _c(depth, "depth"), _c(labels, "labels"), _c(table, "table", torch.int32)
    N = table.shape[0]
    F_, _, H, W = rgb.shape
    dev = rgb.device
    rgb_out = torch.empty((N, 3, size, size), device=dev, dtype=torch.float32)
    mask_out = torch.empty((N, size, size), device=dev, dtype=torch.float32)
    depth_out = torch.empty((N, 3, size, size), device=dev, dtype=torch.float32) if depth is not None else None
    check(lib().msm_crop_resize(_p(rgb), _p(depth), _p(labels), _p(table), _p(rgb_out), _p(depth_out), _p(mask_out), N, H, W, int(size),
                                _stream()), "msm_crop_resize")
    return rgb_out, mask_out, depth_out


def paste_labels(renum, table, order, frame_start, frames, H, W):
    """Paste-back of a batch (msm_paste_labels): renum (N,S,S) float, table (N,8) int32, order (N,) int32, frame_start (F+1,)
    int32 -> refined (F,H,W) float."""
    _c(renum, "renum"), _c(table, "table", torch.int32), _c(order, "order", torch.int32), _c(frame_start, "frame_start", torch.int32)
    refined = torch.empty((frames, H, W), device=renum.device, dtype=torch.float32)
    check(lib().msm_paste_labels(_p(renum), _p(table), _p(order), _p(frame_start), _p(refined), frames, H, W, renum.shape[-1], _stream()),
          "msm_paste_labels")
    return refined


_DEPTH_U16 = (torch.uint16, torch.int16)          # int16 holding the same bits (torch builds without uint16 kernels)


def ingest_frames(color, depth, cam, lut, *, depth_div=1000.0, swap_rb=False, frame=None, out_image=None, out_depth=None):
    """Raw camera frames -> the network's input tensors in one launch (msm_ingest_frames): color (F,H,W,3) uint8, depth (F,H,W)
    uint16 / int16 bits (z = d / depth_div) or float32 (metres, NaN -> 0) or None, cam (F,4) float fx, fy, px, py, lut (3,256)
    float (frames.image_lut) -> (image (F,3,Hp,Wp), xyz (F,3,Hp,Wp) or None), zero outside the H x W image.  ``frame`` = (Hp, Wp)
    (default (H, W)); ``out_image`` / ``out_depth`` are written in place when given (e.g. the static input buffers of a graph slot)."""
    _c(color, "color", torch.uint8), _c(cam, "cam"), _c(lut, "lut")
    if color.dim() != 4 or color.shape[-1] != 3:
        raise RuntimeError(f"ingest_frames: color {tuple(color.shape)} must be (F, H, W, 3)")
    F_, H, W, _ = color.shape
    Hp, Wp = (H, W) if frame is None else (int(frame[0]), int(frame[1]))
    dev = color.device
    if tuple(lut.shape) != (3, 256):
        raise RuntimeError(f"ingest_frames: lut {tuple(lut.shape)} must be (3, 256)")
    is_u16 = 0
    if depth is not None:
        if depth.dtype not in _DEPTH_U16 + (torch.float32,):
            raise RuntimeError(f"ingest_frames: depth must be uint16 (or int16 bits) or float32, got {depth.dtype}")
        _c(depth, "depth", depth.dtype)
        is_u16 = 1 if depth.dtype in _DEPTH_U16 else 0
        if tuple(depth.shape) != (F_, H, W):
            raise RuntimeError(f"ingest_frames: depth {tuple(depth.shape)} must be {(F_, H, W)}")
        if cam is None or tuple(cam.shape) != (F_, 4):
            raise RuntimeError(f"ingest_frames: cam must be ({F_}, 4) fx, fy, px, py")
    elif out_depth is not None:
        raise RuntimeError("ingest_frames: out_depth without depth")
    outs = []
    for t, name, want in ((out_image, "out_image", True), (out_depth, "out_depth", depth is not None)):
        if t is None:
            t = torch.empty((F_, 3, Hp, Wp), device=dev, dtype=torch.float32) if want else None
        else:
            _c(t, name)
            if tuple(t.shape) != (F_, 3, Hp, Wp) or t.device != dev:
                raise RuntimeError(f"ingest_frames: {name} {tuple(t.shape)} on {t.device} must be {(F_, 3, Hp, Wp)} on {dev}")
        outs.append(t)
    image, xyz = outs
    check(lib().msm_ingest_frames(_p(color), _p(depth), is_u16, float(depth_div), _p(lut), _p(cam), _p(image), _p(xyz), F_, H, W, Hp, Wp,
                                  1 if swap_rb else 0, _stream()), "msm_ingest_frames")
    return image, xyz


def prepare_inputs(image, depth=None, *, mean=None, std=None, frame=None, out_image=None, out_depth=None):
    """What a meta-arch applies in front of the network, in one launch (msm_prepare_inputs): image (N,C,H,W) -> ((image - mean[c]) /
    std[c], or the same bits without ``mean`` / ``std`` (C values each, on the device)) padded with zeros at the right / bottom to
    ``frame`` = (Hp, Wp) (default (H, W)); depth (N,Cd,H,W) or None is copied bit for bit into the same frame -> (image_out
    (N,C,Hp,Wp), depth_out (N,Cd,Hp,Wp) or None).  ``out_image`` / ``out_depth`` are written in place when given (e.g. the static
    inputs of a graph slot); an output cannot be its own input."""
    _c(image, "image"), _c(depth, "depth"), _c(mean, "mean"), _c(std, "std")
    if image.dim() != 4:
        raise RuntimeError(f"prepare_inputs: image {tuple(image.shape)} must be (N, C, H, W)")
    N, C, H, W = image.shape
    Hp, Wp = (H, W) if frame is None else (int(frame[0]), int(frame[1]))
    dev = image.device
    if (mean is None) != (std is None):
        raise RuntimeError("prepare_inputs: mean and std go together")
    for t, name in ((mean, "mean"), (std, "std")):
        if t is not None and (t.numel() != C or t.device != dev):
            raise RuntimeError(f"prepare_inputs: {name} {tuple(t.shape)} on {t.device} must hold {C} values on {dev}")
    Cd = 0
    if depth is not None:
        if depth.dim() != 4 or depth.shape[0] != N or tuple(depth.shape[2:]) != (H, W) or depth.device != dev:
            raise RuntimeError(f"prepare_inputs: depth {tuple(depth.shape)} on {depth.device} must be ({N}, Cd, {H}, {W}) on {dev}")
        Cd = depth.shape[1]
    elif out_depth is not None:
        raise RuntimeError("prepare_inputs: out_depth without depth")
    outs = []
    for t, name, ch in ((out_image, "out_image", C), (out_depth, "out_depth", Cd)):
        if t is None:
            t = torch.empty((N, ch, Hp, Wp), device=dev, dtype=torch.float32) if ch else None
        else:
            _c(t, name)
            if tuple(t.shape) != (N, ch, Hp, Wp) or t.device != dev:
                raise RuntimeError(f"prepare_inputs: {name} {tuple(t.shape)} on {t.device} must be {(N, ch, Hp, Wp)} on {dev}")
        outs.append(t)
    image_out, depth_out = outs
    if N == 0:                                    # (an empty tensor has no address to hand over)
        return image_out, depth_out
    check(lib().msm_prepare_inputs(_p(image), _p(depth), _p(mean), _p(std), _p(image_out), _p(depth_out), N, C, Cd, H, W, Hp, Wp,
                                   _stream()), "msm_prepare_inputs")
    return image_out, depth_out


# ---- training targets from instance label images (targets.py; csrc/targets.hip) ----
TARGET_BINS = 1024           # MSM_TARGET_BINS: instance ids lie in [0, 1024)
SAMPLE_MAX_LABELS = 256      # MSM_SAMPLE_MAX_LABELS: dense labels per image msm_sample_labels selects for
TARGET_COUNT_MISMATCH = 1    # MSM_TARGET_COUNT_MISMATCH: bit of tables[b][3]
_RAW_DTYPES = (torch.uint8, torch.int32)
_LABEL_DTYPES = (torch.float32, torch.int32)


def _check_raw(raw, who):
    if raw.dtype not in _RAW_DTYPES:
        raise RuntimeError(f"{who}: raw must be uint8 or int32, got {raw.dtype}")
    _c(raw, "raw", raw.dtype)
    if raw.dim() != 3 or 0 in raw.shape:
        raise RuntimeError(f"{who}: raw {tuple(raw.shape)} must be a non-empty (B, H, W)")


def target_tables(raw, background_ids=None):
    """The per-image tables of a batch of instance label images in one launch (msm_target_tables): raw (B,H,W) uint8 or int32
    with ids in [0, 1024), background_ids: int32 device tensor of the ids folded to 0 (None: none) -> tables (B, row) int32
    laid out as include/msm_hip.h documents: [0] out-of-range pixels, [1] T_b, [2] K_b, [3] status bits of target_write, the
    id -> dense index and id -> mask row tables, the instance records (id, area, x_min, y_min, x_max, y_max)."""
    _check_raw(raw, "target_tables")
    _c(background_ids, "background_ids", torch.int32)
    B, H, W = raw.shape
    tables = torch.empty((B, lib().msm_target_table_row()), device=raw.device, dtype=torch.int32)
    n_bg = 0 if background_ids is None else background_ids.numel()
    check(lib().msm_target_tables(_p(raw), 1 if raw.dtype == torch.int32 else 0, _p(background_ids if n_bg else None), n_bg,
                                  _p(tables), B, H, W, _stream()), "msm_target_tables")
    return tables


def target_write(raw, tables, toff=None, total=0, *, frame=None, label_dtype=torch.float32, masks=None):
    """The padded dense label map and, with ``toff``, the (TT,Hp,Wp) uint8 masks of a batch in one launch (msm_target_write):
    raw and tables as target_tables took / returned them, toff: (B+1,) int64 DEVICE tensor of mask-row offsets and ``total`` =
    TT rows in the buffer (the launch never writes another row: a count that disagrees with the device's sets bit 0 of
    tables[b][3]), frame = (Hp, Wp) (default (H, W)) -> (label (B,Hp,Wp) of ``label_dtype`` float32 / int32, masks or None,
    boxes (TT,4) float32, ids (TT,) int32, areas (TT,) int32).  ``masks``: a (TT,Hp,Wp) uint8 buffer to write into."""
    _check_raw(raw, "target_write")
    _c(tables, "tables", torch.int32), _c(toff, "toff", torch.int64)
    B, H, W = raw.shape
    dev = raw.device
    Hp, Wp = (H, W) if frame is None else (int(frame[0]), int(frame[1]))
    if tuple(tables.shape) != (B, lib().msm_target_table_row()) or tables.device != dev:
        raise RuntimeError(f"target_write: tables {tuple(tables.shape)} on {tables.device} do not belong to {B} images on {dev}")
    if label_dtype not in _LABEL_DTYPES:
        raise RuntimeError(f"target_write: label_dtype must be float32 or int32, got {label_dtype}")
    label = torch.empty((B, Hp, Wp), device=dev, dtype=label_dtype)
    boxes = ids = areas = None
    TT = int(total)
    if toff is None:
        if masks is not None or TT:
            raise RuntimeError("target_write: masks need toff")
    else:
        if tuple(toff.shape) != (B + 1,) or toff.device != dev or TT < 0:
            raise RuntimeError(f"target_write: toff {tuple(toff.shape)} on {toff.device} must be ({B + 1},) on {dev}")
        if masks is None:
            masks = torch.empty((TT, Hp, Wp), device=dev, dtype=torch.uint8)
        _c(masks, "masks", torch.uint8)
        if tuple(masks.shape) != (TT, Hp, Wp) or masks.device != dev:
            raise RuntimeError(f"target_write: masks {tuple(masks.shape)} on {masks.device} must be {(TT, Hp, Wp)} on {dev}")
        boxes = torch.empty((TT, 4), device=dev, dtype=torch.float32)
        ids = torch.empty((TT,), device=dev, dtype=torch.int32)
        areas = torch.empty((TT,), device=dev, dtype=torch.int32)
    # an empty mask buffer has no address: the kernel still takes the toff path (status, nothing to write) through a dummy
    mp = masks if masks is None or TT else torch.empty((1,), device=dev, dtype=torch.uint8)
    check(lib().msm_target_write(_p(raw), 1 if raw.dtype == torch.int32 else 0, _p(tables), _p(toff), _p(label),
                                 1 if label_dtype == torch.float32 else 0, _p(mp), _p(boxes if TT else mp), _p(ids if TT else mp),
                                 _p(areas if TT else mp), B, H, W, Hp, Wp, TT, _stream()), "msm_target_write")
    return label, masks, boxes, ids, areas


def sample_labels_(label, keys, num, image_size=None):
    """sample_pixels in place (msm_sample_labels): label (B,Hp,Wp) float32 or int32 dense labels, keys (B,H,W) int32, (H, W) =
    ``image_size`` (default: the whole map) the corner that is sampled.  Per image and label in [0, 256) with more than
    ``num`` pixels, the ``num`` smallest by (key, flat index) stay and the others become -1.  Returns status (B,) int32: pixels
    whose label is not an integer below 256 (for the caller to read when it chooses to; nothing here waits)."""
    if label.dtype not in _LABEL_DTYPES:
        raise RuntimeError(f"sample_labels_: label must be float32 or int32, got {label.dtype}")
    _c(label, "label", label.dtype), _c(keys, "keys", torch.int32)
    if label.dim() != 3 or 0 in label.shape:
        raise RuntimeError(f"sample_labels_: label {tuple(label.shape)} must be a non-empty (B, Hp, Wp)")
    B, Hp, Wp = label.shape
    H, W = (Hp, Wp) if image_size is None else (int(image_size[0]), int(image_size[1]))
    if tuple(keys.shape) != (B, H, W) or keys.device != label.device or not (0 < H <= Hp and 0 < W <= Wp):
        raise RuntimeError(f"sample_labels_: keys {tuple(keys.shape)} on {keys.device} must be {(B, H, W)} on {label.device}, "
                           f"inside the {Hp}x{Wp} map")
    if int(num) < 1:
        raise ValueError(f"sample_labels_: num must be at least 1, got {num}")
    dev = label.device
    nbytes = lib().msm_sample_labels_workspace(B)
    if nbytes < 0:
        check(int(nbytes), "msm_sample_labels_workspace")
    ws = torch.empty((nbytes // 4,), device=dev, dtype=torch.int32)
    status = torch.empty((B,), device=dev, dtype=torch.int32)
    check(lib().msm_sample_labels(_p(label), 1 if label.dtype == torch.float32 else 0, _p(keys), _p(status), _p(ws), nbytes, B, H, W,
                                  Hp, Wp, int(num), _stream()), "msm_sample_labels")
    return status


# ---- random augmentations of the training loader (augment.py; csrc/augment.hip) ----
AUGMENT_RECORD_ROW = 392     # MSM_AUGMENT_RECORD_ROW: int32 words of one image's ellipse records, B blocks at the head of the workspace


def _check_augment_table(table, status, B, dev, who):
    _c(table, "table", torch.int32), _c(status, "status", torch.int32)
    if tuple(table.shape) != (B, lib().msm_augment_table_row()) or table.device != dev:
        raise RuntimeError(f"{who}: table {tuple(table.shape)} on {table.device} must be ({B}, {lib().msm_augment_table_row()}) on {dev}")
    if tuple(status.shape) != (B, 4) or status.device != dev:
        raise RuntimeError(f"{who}: status {tuple(status.shape)} on {status.device} must be ({B}, 4) on {dev}")


def augment_color(color, table, noise, status, *, out=None):
    """D1-D3 of augment.py on a batch in one launch (msm_augment_color): color (B,H,W,3) uint8 BGR, table (B,176) int32
    (augment.pack_table), noise (B,H,W) float32 or None, status (B,4) int32 whose column 0 the launch writes -> a new (B,H,W,3)
    uint8 tensor (or ``out``, a contiguous tensor of that shape that is not ``color``).  Nothing here waits."""
    _c(color, "color", torch.uint8), _c(noise, "noise")
    if color.dim() != 4 or color.shape[-1] != 3 or 0 in color.shape:
        raise RuntimeError(f"augment_color: color {tuple(color.shape)} must be a non-empty (B, H, W, 3)")
    B, H, W, _ = color.shape
    dev = color.device
    _check_augment_table(table, status, B, dev, "augment_color")
    if noise is not None and (tuple(noise.shape) != (B, H, W) or noise.device != dev):
        raise RuntimeError(f"augment_color: noise {tuple(noise.shape)} on {noise.device} must be {(B, H, W)} on {dev}")
    if out is None:
        out = torch.empty_like(color)
    _c(out, "out", torch.uint8)
    if out.shape != color.shape or out.device != dev or out.data_ptr() == color.data_ptr():
        raise RuntimeError(f"augment_color: out {tuple(out.shape)} on {out.device} must be another {tuple(color.shape)} tensor on {dev}")
    check(lib().msm_augment_color(_p(color), _p(table), _p(noise), _p(out), _p(status), B, H, W, _stream()), "msm_augment_color")
    return out


def augment_depth(depth, table, status, *, depth_div=1000.0, records=None, stages=3, out=None):
    """D4 of augment.py on a batch (msm_augment_depth, three launches): depth (B,H,W) uint16 / int16 bits (z = d / depth_div) or float32
    (metres, NaN -> 0), table and status as augment_color (column 1 is written) -> (out (B,H,W) float32, new or given, records).  ``records``
    (int32, msm_augment_depth_workspace bytes: B blocks of AUGMENT_RECORD_ROW words, then the row counts) and ``stages`` (1: row
    counts and centres, 2: apply, 3: all) are for tests of the last launch on hand-made records."""
    if depth.dtype not in _DEPTH_U16 + (torch.float32,):
        raise RuntimeError(f"augment_depth: depth must be uint16 (or int16 bits) or float32, got {depth.dtype}")
    _c(depth, "depth", depth.dtype)
    if depth.dim() != 3 or 0 in depth.shape:
        raise RuntimeError(f"augment_depth: depth {tuple(depth.shape)} must be a non-empty (B, H, W)")
    B, H, W = depth.shape
    dev = depth.device
    _check_augment_table(table, status, B, dev, "augment_depth")
    nbytes = lib().msm_augment_depth_workspace(B, H, W)
    if nbytes < 0:
        check(int(nbytes), "msm_augment_depth_workspace")
    if records is None:
        records = torch.empty((nbytes // 4,), device=dev, dtype=torch.int32)
    _c(records, "records", torch.int32)
    if records.numel() * 4 < nbytes or records.device != dev:
        raise RuntimeError(f"augment_depth: records of {records.numel() * 4} bytes on {records.device}, {nbytes} needed on {dev}")
    if out is None:
        out = torch.empty((B, H, W), device=dev, dtype=torch.float32)
    _c(out, "out")
    if tuple(out.shape) != (B, H, W) or out.device != dev:
        raise RuntimeError(f"augment_depth: out {tuple(out.shape)} on {out.device} must be {(B, H, W)} on {dev}")
    check(lib().msm_augment_depth(_p(depth), 1 if depth.dtype in _DEPTH_U16 else 0, float(depth_div), _p(table), _p(out), _p(status),
                                  _p(records), records.numel() * 4, int(stages), B, H, W, _stream()), "msm_augment_depth")
    return out, records


def xyz_noise_(xyz, gp, taps, scale, size=None):
    """D5 of augment.py in place in one launch (msm_xyz_noise): xyz (B,3,Hp,Wp) float32, gp (B,3,h,w) float32, taps (H + W, 8)
    int32 (augment._device_taps), ``size`` = (H, W) the valid corner (default the whole map).  Returns xyz."""
    _c(xyz, "xyz"), _c(gp, "gp"), _c(taps, "taps", torch.int32)
    if xyz.dim() != 4 or xyz.shape[1] != 3 or 0 in xyz.shape:
        raise RuntimeError(f"xyz_noise_: xyz {tuple(xyz.shape)} must be a non-empty (B, 3, Hp, Wp)")
    B, _, Hp, Wp = xyz.shape
    H, W = (Hp, Wp) if size is None else (int(size[0]), int(size[1]))
    if gp.dim() != 4 or tuple(gp.shape[:2]) != (B, 3) or 0 in gp.shape or gp.device != xyz.device:
        raise RuntimeError(f"xyz_noise_: gp {tuple(gp.shape)} on {gp.device} must be ({B}, 3, h, w) on {xyz.device}")
    if not (0 < H <= Hp and 0 < W <= Wp) or tuple(taps.shape) != (H + W, 8) or taps.device != xyz.device:
        raise RuntimeError(f"xyz_noise_: size {(H, W)} must lie inside {(Hp, Wp)} and taps {tuple(taps.shape)} be ({H + W}, 8)")
    check(lib().msm_xyz_noise(_p(xyz), _p(gp), _p(taps), float(scale), B, H, W, Hp, Wp, gp.shape[2], gp.shape[3], _stream()),
          "msm_xyz_noise")
    return xyz


# ---- training crops, TRAIN.SYN_CROP (crops.py; csrc/train_crop.hip) ----
CROP_BOX_ROW = 8             # MSM_CROP_BOX_ROW: x0, y0, x1, y1, dense index, raw id, padding, status bits
CROP_MAX_SIZE = 1024         # MSM_CROP_MAX_SIZE
CROP_DEGENERATE, CROP_BAD_BOX, CROP_BAD_ROW = 1, 2, 4      # MSM_CROP_* bits of boxes[b][7]


def crop_boxes(tables, params, image_size, *, out=None):
    """One crop box per image in one launch (msm_crop_boxes): tables (B, row) int32 as target_tables returned them for the FULL
    frames, params (B,2) int32 words -- a uint32 key and the bits of the float32 padding fraction -- ``image_size`` = (H, W) ->
    boxes (B, CROP_BOX_ROW) int32 (new, or ``out``): x0, y0, x1, y1 inclusive, the chosen dense index and raw id, the padding,
    status bits.  Nothing here waits."""
    _c(tables, "tables", torch.int32), _c(params, "params", torch.int32)
    H, W = int(image_size[0]), int(image_size[1])
    if tables.dim() != 2 or tables.shape[0] == 0 or tables.shape[1] != lib().msm_target_table_row():
        raise RuntimeError(f"crop_boxes: tables {tuple(tables.shape)} must be a non-empty (B, {lib().msm_target_table_row()})")
    B, dev = tables.shape[0], tables.device
    if tuple(params.shape) != (B, 2) or params.device != dev:
        raise RuntimeError(f"crop_boxes: params {tuple(params.shape)} on {params.device} must be ({B}, 2) on {dev}")
    if out is None:
        out = torch.empty((B, CROP_BOX_ROW), device=dev, dtype=torch.int32)
    _c(out, "out", torch.int32)
    if tuple(out.shape) != (B, CROP_BOX_ROW) or out.device != dev:
        raise RuntimeError(f"crop_boxes: out {tuple(out.shape)} on {out.device} must be ({B}, {CROP_BOX_ROW}) on {dev}")
    check(lib().msm_crop_boxes(_p(tables), _p(params), _p(out), B, H, W, _stream()), "msm_crop_boxes")
    return out


def train_crop(color, raw, xyz, boxes, size, *, frame=None, out_color=None, out_raw=None, out_xyz=None):
    """Crop and resize a batch in one launch (msm_train_crop): color (B,H,W,3) uint8 (bilinear, C4 of crops.py), raw (B,H,W) uint8
    or int32 (nearest, ids kept) and xyz (B,3,Hp,Wp) float32 or None (nearest, bit for bit), each inside its image's row of
    ``boxes`` (B, CROP_BOX_ROW) int32, resized to ``size`` = S -> (color (B,S,S,3), raw (B,S,S), xyz (B,3,Sp,Sp) or None), Sp =
    ``frame`` (default S), zeros beyond S.  A row whose box does not lie inside the image gives zeros and gets CROP_BAD_BOX ORed
    into boxes[b][7].  ``out_*``: contiguous tensors to write into."""
    _c(color, "color", torch.uint8), _c(xyz, "xyz"), _c(boxes, "boxes", torch.int32)
    _check_raw(raw, "train_crop")
    if color.dim() != 4 or color.shape[-1] != 3 or tuple(color.shape[:3]) != tuple(raw.shape) or raw.device != color.device:
        raise RuntimeError(f"train_crop: color {tuple(color.shape)} must be (B, H, W, 3) and raw {tuple(raw.shape)} (B, H, W) beside it")
    B, H, W = raw.shape
    dev = color.device
    S = int(size)
    Sp = S if frame is None else int(frame)
    if tuple(boxes.shape) != (B, CROP_BOX_ROW) or boxes.device != dev:
        raise RuntimeError(f"train_crop: boxes {tuple(boxes.shape)} on {boxes.device} must be ({B}, {CROP_BOX_ROW}) on {dev}")
    Hp, Wp = H, W
    if xyz is not None:
        if xyz.dim() != 4 or tuple(xyz.shape[:2]) != (B, 3) or xyz.device != dev:
            raise RuntimeError(f"train_crop: xyz {tuple(xyz.shape)} on {xyz.device} must be ({B}, 3, Hp, Wp) on {dev}")
        Hp, Wp = xyz.shape[2:]
    elif out_xyz is not None:
        raise RuntimeError("train_crop: out_xyz without xyz")
    if not 1 <= S <= Sp:
        raise RuntimeError(f"train_crop: size {S} must lie in [1, frame = {Sp}]")
    outs = []
    for t, name, shape, dtype in ((out_color, "out_color", (B, S, S, 3), torch.uint8), (out_raw, "out_raw", (B, S, S), raw.dtype),
                                  (out_xyz, "out_xyz", (B, 3, Sp, Sp), torch.float32)):
        if t is None:
            t = torch.empty(shape, device=dev, dtype=dtype) if (name != "out_xyz" or xyz is not None) else None
        else:
            _c(t, name, dtype)
            if tuple(t.shape) != shape or t.device != dev:
                raise RuntimeError(f"train_crop: {name} {tuple(t.shape)} on {t.device} must be {shape} on {dev}")
        outs.append(t)
    check(lib().msm_train_crop(_p(color), _p(raw), 1 if raw.dtype == torch.int32 else 0, _p(xyz), _p(boxes), _p(outs[0]), _p(outs[1]),
                               _p(outs[2]), B, H, W, Hp, Wp, S, Sp, _stream()), "msm_train_crop")
    return tuple(outs)


# ----------------------------------------------------------------------------------------------
# backbone glue (csrc/backbone_ops.hip)
# ----------------------------------------------------------------------------------------------
_GLUE_DTYPES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


def bias_act_nhwc_(x, bias, residual=None, relu=True):
    """In place on a channels_last (B, C, H, W) map (fp32 or bfloat16): x = act(x + bias[c] (+ residual)) in one pass
    (msm_bias_act_nhwc) -- the bias kernel MIOpen appends to a convolution, F.relu, the residual add and its ReLU of a ResNet block
    as ONE launch.  bias (C,) and residual (same shape and memory format) in x's dtype.  Returns x."""
    if x.dtype not in _GLUE_DTYPES or not x.is_cuda:
        raise RuntimeError("bias_act_nhwc_: a float32, bfloat16 or float16 map on the GPU")
    if x.dim() != 4 or not x.is_contiguous(memory_format=torch.channels_last):
        raise RuntimeError("bias_act_nhwc_: x must be (B, C, H, W) in channels_last memory")
    B, C, H, W = x.shape
    if bias.dtype != x.dtype or tuple(bias.shape) != (C,) or not bias.is_contiguous() or bias.device != x.device:
        raise RuntimeError("bias_act_nhwc_: bias must be (C,) in x's dtype on x's device")
    if residual is not None and (residual.dtype != x.dtype or residual.shape != x.shape or residual.device != x.device
                                 or not residual.is_contiguous(memory_format=torch.channels_last)):
        raise RuntimeError("bias_act_nhwc_: residual must match x (shape, dtype, channels_last)")
    check(lib().msm_bias_act_nhwc(_p(x), _p(bias), _p(residual), 1 if relu else 0, B * H * W, C, _GLUE_DTYPES[x.dtype], _stream()),
          "msm_bias_act_nhwc")
    return x


def nhwc_to_nchw_f32(x):
    """A channels_last (B, C, H, W) map (fp32 or bfloat16) as contiguous NCHW fp32 planes in one pass (msm_nhwc_to_nchw_f32)."""
    if x.dtype not in _GLUE_DTYPES or not x.is_cuda or x.dim() != 4 or not x.is_contiguous(memory_format=torch.channels_last):
        raise RuntimeError("nhwc_to_nchw_f32: a channels_last float32 / bfloat16 / float16 (B, C, H, W) map on the GPU")
    B, C, H, W = x.shape
    out = torch.empty((B, C, H, W), device=x.device, dtype=torch.float32)
    check(lib().msm_nhwc_to_nchw_f32(_p(x), _p(out), B, C, H * W, _GLUE_DTYPES[x.dtype], _stream()), "msm_nhwc_to_nchw_f32")
    return out


def ucn_embedding_tail(a, b=None, size=None, norms=1, eps=1e-12):
    """The tail of the UCN RGB-D backbone in one pass (msm_ucn_embedding_tail): a, b (B, 64, h, w) fp32 channels_last maps of the two towers
    (b None: one tower) -> (B, 64, H, W) contiguous fp32 = N(..N(upsample_bilinear(a) + upsample_bilinear(b))), align_corners=True,
    N = F.normalize over the channels applied ``norms`` (0..2) times."""
    if a.dtype != torch.float32 or not a.is_cuda or a.dim() != 4 or a.shape[1] != 64:
        raise RuntimeError("ucn_embedding_tail: (B, 64, h, w) float32 maps on the GPU")
    a = a if a.is_contiguous(memory_format=torch.channels_last) else a.contiguous(memory_format=torch.channels_last)
    if b is not None:
        if b.shape != a.shape or b.dtype != a.dtype or b.device != a.device:
            raise RuntimeError("ucn_embedding_tail: the two towers' maps must match")
        b = b if b.is_contiguous(memory_format=torch.channels_last) else b.contiguous(memory_format=torch.channels_last)
    B, _, h, w = a.shape
    H, W = int(size[0]), int(size[1])
    out = torch.empty((B, 64, H, W), device=a.device, dtype=torch.float32)
    check(lib().msm_ucn_embedding_tail(_p(a), _p(b), _p(out), B, h, w, H, W, int(norms), float(eps), _stream()), "msm_ucn_embedding_tail")
    return out


def ucn_embedding_tail_bwd(a, b, gout, norms=1, eps=1e-12):
    """Backward of ``ucn_embedding_tail`` (msm_ucn_embedding_tail_bwd): a, b (B, 64, h, w) fp32 maps of the two towers as the forward took
    them (b None: one tower), gout (B, 64, H, W) fp32 contiguous -> gin (B, 64, h, w) fp32 channels_last, the gradient of a and of b alike
    (add fusion).  Deterministic: the same bits at every call."""
    if a.dtype != torch.float32 or not a.is_cuda or a.dim() != 4 or a.shape[1] != 64:
        raise RuntimeError("ucn_embedding_tail_bwd: (B, 64, h, w) float32 maps on the GPU")
    a = a if a.is_contiguous(memory_format=torch.channels_last) else a.contiguous(memory_format=torch.channels_last)
    if b is not None:
        if b.shape != a.shape or b.dtype != a.dtype or b.device != a.device:
            raise RuntimeError("ucn_embedding_tail_bwd: the two towers' maps must match")
        b = b if b.is_contiguous(memory_format=torch.channels_last) else b.contiguous(memory_format=torch.channels_last)
    B, _, h, w = a.shape
    if gout.dim() != 4 or gout.shape[0] != B or gout.shape[1] != 64 or gout.dtype != torch.float32 or gout.device != a.device:
        raise RuntimeError("ucn_embedding_tail_bwd: gout must be a (B, 64, H, W) float32 map on the towers' device")
    _c(gout, "gout")
    H, W = int(gout.shape[2]), int(gout.shape[3])
    n = lib().msm_ucn_embedding_tail_bwd_workspace(B, H, w)
    check(min(n, 0), "msm_ucn_embedding_tail_bwd_workspace")
    ws = torch.empty(n, device=a.device, dtype=torch.float32)
    gin = torch.empty((B, 64, h, w), device=a.device, dtype=torch.float32, memory_format=torch.channels_last)
    check(lib().msm_ucn_embedding_tail_bwd(_p(a), _p(b), _p(gout), _p(gin), _p(ws), n, B, h, w, H, W, int(norms), float(eps), _stream()),
          "msm_ucn_embedding_tail_bwd")
    return gin


def to_f16(t):
    """fp32 -> fp16 (round to nearest even, clamped to the half range) on the HIP path (msm_f32_to_f16)."""
    _c(t, "t")
    out = torch.empty(t.shape, device=t.device, dtype=torch.float16)
    check(lib().msm_f32_to_f16(_p(t), _p(out), t.numel(), _stream()), "msm_f32_to_f16")
    return out


# ----------------------------------------------------------------------------------------------
# fused encoder (msdeformattn.py:122-131); the weight streams come from packing.py
# ----------------------------------------------------------------------------------------------
def encoder_prologue(raw, stats, gn_params, level_starts, stream, small, pos, proj_width, *, groups=32, eps=1e-5, value_heads=0,
                     bf16_hm=False):
    """raw (B,S,64) concatenated input projections (conv1x1_in), stats (L,B,64,2) float64 their GroupNorm moments,
    gn_params (L,2,64) = gamma, beta, level_starts: L+1 token offsets (0..S).  Normalises raw IN PLACE (-> src) and
    returns (src, value, proj) for the first encoder layer: value (B,S,64) or head-major (B,heads,S,64/heads),
    proj (B,S,proj_width) = [sampling_offsets | attention_weights](src + pos).  bf16_hm (8 heads, proj_width 288): value and
    proj are the bf16 plan's head-major fp16 tensors (B,8,S,8) and (B,8,S,36) (encoder_block_hm)."""
    _c(raw, "raw"), _c(stats, "stats", torch.float64), _c(gn_params, "gn_params"), _c(stream, "stream"), _c(small, "small"), _c(pos, "pos")
    B, S, C = raw.shape
    L = len(level_starts) - 1
    if C != 64 or tuple(stats.shape) != (L, B, 64, 2) or tuple(gn_params.shape) != (L, 2, 64) or tuple(pos.shape) != (S, 64):
        raise RuntimeError("encoder_prologue: inconsistent shapes")
    if small.numel() != 64 + proj_width:
        raise RuntimeError("encoder_prologue: small must hold the 64 value_proj biases and the proj_width projection biases")
    dev = raw.device
    if bf16_hm:
        value = torch.empty((B, 8, S, 8), device=dev, dtype=torch.float16)
        proj = torch.empty((B, 8, S, PROJ_REC_FLOATS), device=dev, dtype=torch.float32)
    else:
        value = torch.empty((B, value_heads, S, 64 // value_heads) if value_heads else (B, S, 64), device=dev, dtype=torch.float32)
        proj = torch.empty((B, S, proj_width), device=dev, dtype=torch.float32) if proj_width else None     # 0: value projection only
    ls = (ctypes.c_int32 * (L + 1))(*[int(v) for v in level_starts])
    rc = lib().msm_encoder_prologue_fwd(_p(raw), _p(stats), _p(gn_params), ctypes.cast(ls, ctypes.c_void_p), L, int(groups), float(eps),
                                        _p(stream), _p(small), _p(pos), _p(raw), _p(value), _p(proj), B, S, int(proj_width),
                                        int(value_heads), int(bool(bf16_hm)), _stream())
    check(rc, "msm_encoder_prologue_fwd")
    return raw, value, proj


def _encoder_tail(entry, wdtype, attn, src, wstream, small, d_ffn, proj_width, pos, tokens_per_image, want_next, value_heads, eps,
                  proj_none_if_empty=False):
    """The launch the three encoder-tail wrappers share: ``entry`` is the msm_encoder_block*_fwd to call, ``wdtype`` the dtype its
    wstream has.  proj_none_if_empty: proj_out is None, not a (B, S, 0) tensor, when proj_width == 0."""
    _c(attn, "attn"), _c(src, "src"), _c(wstream, "wstream", wdtype), _c(small, "small"), _c(pos, "pos")
    B, S, C = src.shape
    src_out = torch.empty_like(src)
    value_out = proj_out = None
    if want_next:
        value_out = torch.empty((B, value_heads, S, C // value_heads), device=src.device, dtype=torch.float32) \
            if value_heads else torch.empty_like(src)
        if proj_width or not proj_none_if_empty:
            proj_out = torch.empty((B, S, proj_width), device=src.device, dtype=torch.float32)
    rc = getattr(lib(), entry)(_p(attn), _p(src), _p(wstream), _p(small), _p(pos), _p(src_out), _p(value_out), _p(proj_out),
                               B * S, tokens_per_image or S, d_ffn, proj_width, int(value_heads), eps, _stream())
    check(rc, entry)
    return src_out, value_out, proj_out


def encoder_block(attn, src, wstream, small, d_ffn, proj_width, *, pos=None, tokens_per_image=None, want_next=True,
                  value_heads=0, eps=1e-5):
    """One fused encoder-layer tail.  attn/src (B,S,64).  Returns (src_out, value_out, proj_out) with the
    last two None when want_next is False.  value_heads = h > 0: value_out is head-major (B,h,S,64/h)."""
    # proj_width == 0: the next layer's gather computes its own sampling projection (ms_deform_attn_encoder_fused)
    return _encoder_tail("msm_encoder_block_fwd", torch.float32, attn, src, wstream, small, d_ffn, proj_width, pos, tokens_per_image,
                         want_next, value_heads, eps, proj_none_if_empty=True)


def encoder_block_split(attn, src, wstream, small, d_ffn, proj_width, *, pos=None, tokens_per_image=None, want_next=True,
                        value_heads=0, eps=1e-5):
    """encoder_block in fp32 accuracy on the bf16 matrix pipe (wstream from pack_encoder_block_split): fp32 in, fp32 out."""
    return _encoder_tail("msm_encoder_block_split_fwd", torch.int16, attn, src, wstream, small, d_ffn, proj_width, pos, tokens_per_image,
                         want_next, value_heads, eps)


def encoder_block_lp(attn, src, wstream, small, d_ffn, proj_width, *, pos=None, tokens_per_image=None, want_next=True,
                     value_heads=0, eps=1e-5):
    """encoder_block in the low-precision mode on the K = 32 kernel (wstream from pack_encoder_block_lp); fp32 in, fp32 out."""
    return _encoder_tail("msm_encoder_block_lp_fwd", torch.int16, attn, src, wstream, small, d_ffn, proj_width, pos, tokens_per_image,
                         want_next, value_heads, eps)


# ---- the bf16 plan's encoder layers with head-major bf16 activations (csrc/enc_lp.hip) ------------------------------------
def encoder_prologue_hm(raw, stats, gn_params, level_starts, blocks, small, pos, *, groups=32, eps=1e-5):
    """encoder_prologue for the bf16 plan with its projections on the bf16 matrix pipe (msm_encoder_prologue_hm_fwd): normalises raw
    IN PLACE (-> src), returns (src, value (B,8,S,8) fp16, proj (B,8,S,36) fp16).  blocks / small: pack_encoder_prologue_hm."""
    _c(raw, "raw"), _c(stats, "stats", torch.float64), _c(gn_params, "gn_params"), _c(blocks, "blocks", torch.int16), _c(small, "small"), _c(pos, "pos")
    B, S, C = raw.shape
    L = len(level_starts) - 1
    if C != 64 or tuple(stats.shape) != (L, B, 64, 2) or tuple(gn_params.shape) != (L, 2, 64) or tuple(pos.shape) != (S, 64) or small.numel() != 352:
        raise RuntimeError("encoder_prologue_hm: inconsistent shapes")
    value = torch.empty((B, 8, S, 8), device=raw.device, dtype=torch.float16)
    proj = torch.empty((B, 8, S, PROJ_REC_FLOATS), device=raw.device, dtype=torch.float32)
    ls = (ctypes.c_int32 * (L + 1))(*[int(v) for v in level_starts])
    rc = lib().msm_encoder_prologue_hm_fwd(_p(raw), _p(stats), _p(gn_params), ctypes.cast(ls, ctypes.c_void_p), L, int(groups), float(eps),
                                           _p(blocks), _p(small), _p(pos), _p(raw), _p(value), _p(proj), B, S, _stream())
    check(rc, "msm_encoder_prologue_hm_fwd")
    return raw, value, proj


def encoder_block_hm(attn_hm, src, wstream, small, d_ffn, *, pos=None, want_next=True, eps=1e-5, ffn_f16=False):
    """One encoder-layer tail of the bf16 plan: attn_hm (B, 8, S, 8) fp16, src (B, S, 64) fp32 -> (src_out fp32, and for the
    NEXT layer value_hm (B, 8, S, 8) fp16 and the sampling records proj_hm (B, 8, S, 30) float32-typed (24 fp32 offsets + 12 fp16
    logits), or None, None)."""
    _c(attn_hm, "attn_hm", torch.float16), _c(src, "src"), _c(wstream, "wstream", torch.int16), _c(small, "small"), _c(pos, "pos")
    B, S, C = src.shape
    if C != 64 or tuple(attn_hm.shape) != (B, 8, S, 8):
        raise RuntimeError("encoder_block_hm: src (B, S, 64) and attn_hm (B, 8, S, 8)")
    if want_next and (pos is None or tuple(pos.shape) != (S, 64)):
        raise RuntimeError("encoder_block_hm: the next layer's projection needs pos (S, 64)")
    if wstream.numel() * 2 != lib().msm_encoder_block_hm_stream_bytes(int(d_ffn), int(want_next)):
        raise RuntimeError("encoder_block_hm: wstream does not match d_ffn / want_next (pack_encoder_block_hm)")
    src_out = torch.empty_like(src)
    value_out = torch.empty_like(attn_hm) if want_next else None
    proj_out = torch.empty((B, 8, S, PROJ_REC_FLOATS), device=src.device, dtype=torch.float32) if want_next else None
    rc = lib().msm_encoder_block_hm_fwd(_p(attn_hm), _p(src), _p(wstream), _p(small), _p(pos if want_next else None), _p(src_out), _p(value_out),
                                        _p(proj_out), B * S, S, int(d_ffn), float(eps), int(bool(ffn_f16)), _stream())
    check(rc, "msm_encoder_block_hm_fwd")
    return src_out, value_out, proj_out


def ms_deform_attn_encoder_lp(value_hm, spatial_shapes, level_start_index, proj_hm, n_points=4):
    """Encoder self-attention gather of the bf16 plan: value_hm (B, 8, S, 8) fp16, proj_hm (B, 8, S, 30) 120-byte records (fp32 offsets,
    logits).  Returns attn_hm (B, 8, S, 8) fp16."""
    _c(value_hm, "value_hm", torch.float16), _c(proj_hm, "proj_hm", torch.float32)
    _c(spatial_shapes, "spatial_shapes", torch.int64), _c(level_start_index, "level_start_index", torch.int64)
    B, M, S, D = value_hm.shape
    if tuple(proj_hm.shape) != (B, M, S, PROJ_REC_FLOATS):
        raise RuntimeError("ms_deform_attn_encoder_lp: proj_hm must be (B, heads, S, 30) float32-typed 120-byte records")
    out = torch.empty_like(value_hm)
    rc = lib().msm_msdeform_attn_enc_lp_fwd(_p(value_hm), _p(spatial_shapes), _p(level_start_index), _p(proj_hm), _p(out), B, S, M, D,
                                            spatial_shapes.shape[0], int(n_points), _stream())
    check(rc, "msm_msdeform_attn_enc_lp_fwd")
    return out


def ms_deform_attn_encoder_lp_fused(value_hm, spatial_shapes, level_start_index, src, pos, wpack, bpack, n_points=4):
    """The same gather with the sampling projection of src + pos computed in the kernel (wpack / bpack from pack_msda_proj_lp)."""
    _c(value_hm, "value_hm", torch.float16), _c(src, "src"), _c(pos, "pos"), _c(wpack, "wpack", torch.int16), _c(bpack, "bpack")
    _c(spatial_shapes, "spatial_shapes", torch.int64), _c(level_start_index, "level_start_index", torch.int64)
    B, M, S, D = value_hm.shape
    if tuple(src.shape) != (B, S, M * D) or tuple(pos.shape) != (S, M * D):
        raise RuntimeError("ms_deform_attn_encoder_lp_fused: src (B, S, 64), pos (S, 64)")
    out = torch.empty_like(value_hm)
    rc = lib().msm_msdeform_attn_enc_lp_fused_fwd(_p(value_hm), _p(spatial_shapes), _p(level_start_index), _p(src), _p(pos), _p(wpack),
                                                  _p(bpack), _p(out), B, S, M, D, spatial_shapes.shape[0], int(n_points), _stream())
    check(rc, "msm_msdeform_attn_enc_lp_fused_fwd")
    return out
