"""Differentiable forward of the hypersphere decoder on the HIP kernels (SURVEY.md section 8 f rank 3: decoder backward).

The reference fine-tunes the decoder with torch autograd through its eager modules (MSMFormer/tabletop_train_net_pretrained.py:
209-246; hypersphere attention AU:30-82, decoder layers DEC:206-315, prediction heads DEC:660-682).  Here the heavy operators
are torch.autograd.Function wrappers whose forward AND backward run in libmsm_hip.so:

    linear / 1x1 input projection   forward msm_gemm_f32; backward two msm_gemm_f32 calls (grad_in = g W, grad_W = g^T x)
    hypersphere attention core      forward msm_hypersphere_attn_fwd; backward msm_hypersphere_attn_bwd (probabilities
                                    recomputed blockwise, nothing of size Lq x S stored)
    Q x pixel-embedding mask step   forward msm_mask_logits_fwd (logits + the NON-differentiable attention-mask bits of the
                                    next layer, detached in the reference too, DEC:680); backward two GEMMs per image
    MSDeformAttn core (pixel decoder)  MultiScaleDeformableAttention.ms_deform_attn_forward / _backward (round 1)
    3x3 mask_features convolution   forward msm_conv3x3_c64_nchw_f32 (implicit GEMM when W % 4 != 0); backward
                                    msm_conv3x3_c64_wgrad (weight, bias) and the implicit GEMM on the mirrored taps (input):
                                    ``conv3x3``; with it ``head_forward_train`` / ``head_losses`` train the RGB-D head
                                    (SimpleBasePixelDecoder + the single-level decoder) from the embedding to the loss dict
    GroupNorm (+ ReLU) on token maps forward msm_groupnorm_stats_f32 + msm_groupnorm_apply_f32; backward msm_groupnorm_bwd_f32 (``group_norm_tokens``)
    bilinear FPN upsampling         forward msm_upsample_bilinear_tokens_f32; backward its gather-form adjoint (``upsample_bilinear_tokens``)
    3x3 FPN output convolution      forward msm_conv3x3_c64_f32; backward msm_conv3x3_c64_wgrad with Cout = 64 and the implicit GEMM, on
                                    tokens in and out: with these ``pixel_decoder_forward_train`` / ``segmentation_head_forward_train`` /
                                    ``segmentation_head_losses`` train the ResNet-50 head (MSDeformAttnPixelDecoder + the multi-level
                                    decoder) from the backbone's four feature maps to the loss dict
    UCN embedding tail              forward msm_ucn_embedding_tail (x8 bilinear upsampling of both towers, add fusion, one or two channel
                                    normalisations in one pass); backward msm_ucn_embedding_tail_bwd (two launches, fixed summation
                                    order): ``ucn_embedding_tail``; with it and the towers' own modules under torch autograd (stock
                                    convolutions: MIOpen) ``ucn_towers_forward_train`` / ``ucn_backbone_forward_train`` /
                                    ``ucn_model_losses`` train the RGB-D model from images

and the cheap row-local glue (LayerNorm, ReLU, residual adds, L2 normalisation of 256-wide rows: < 1 % of the FLOPs) is left to
torch's own differentiable elementwise ops on the device tensors.  ``decoder_forward_train`` follows the reference's literal
operation order (no folded K/V constants, no folded mask features: those are inference-time rewrites of frozen weights) and
returns the reference's full output dict including ``aux_outputs`` (deep supervision needs them).  The inference ``forward`` of
the modules is untouched.

Pinned by tests/golden/decoder_backward.npz: gradients of a fixed random functional of all ten predictions with respect to the
inputs and every parameter, from float64 autograd through the imported reference decoder.
"""
import torch
import torch.nn.functional as F

from . import ops

KAPPA = 30.0  # attention_util.py:26


class MSDeformAttnFunction(torch.autograd.Function):
    """The MSDeformAttn core under autograd, both passes in libmsm_hip.so (float and double): the counterpart of the reference's
    ops/functions/ms_deform_attn_func.py:32-49 for code that builds on this package; the reference's own class works unmodified
    on the drop-in module (MultiScaleDeformableAttention.py).  apply(value, spatial_shapes, level_start_index, sampling_locations,
    attention_weights, im2col_step) -> (N, Lq, M * D)."""

    @staticmethod
    def forward(ctx, value, spatial_shapes, level_start_index, sampling_locations, attention_weights, im2col_step=64):
        from . import MultiScaleDeformableAttention as msda
        ctx.step = im2col_step
        ctx.save_for_backward(value, spatial_shapes, level_start_index, sampling_locations, attention_weights)
        return msda.ms_deform_attn_forward(value, spatial_shapes, level_start_index, sampling_locations, attention_weights, im2col_step)

    @staticmethod
    def backward(ctx, grad_output):
        from . import MultiScaleDeformableAttention as msda
        grads = msda.ms_deform_attn_backward(*ctx.saved_tensors, grad_output.contiguous(), ctx.step)
        return grads[0], None, None, grads[1], grads[2], None


def _t2(x):
    """(R, C) -> (C, R) contiguous through the library's transpose kernel."""
    return ops.transpose_last2(x.reshape(1, *x.shape))[0]


def _gemm_over_rows(a, w):
    """a (N, R) @ w (K, R)^T -> (N, K) where the reduction runs over R rows of a token map (a weight or bias gradient).  From 4096
    rows on, the reduction is cut into up to 64 parts of at least 2048 rows (msm_gemm_f32's split_k: the few output tiles of a
    64 ... 1024-wide layer would otherwise leave most of the chip idle for a 150 000-row reduction) and the parts are added in
    index order."""
    parts = min(64, a.shape[-1] // 2048)
    if parts <= 1:
        return ops.gemm(a, w)
    return ops.gemm(a, w, split_k=parts).sum(0)


class _Linear(torch.autograd.Function):
    """y = x W^T + b over the last dimension (F.linear, AU:134-140 / DEC:296-300,329-341)."""

    @staticmethod
    def forward(ctx, x, w, b):
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        wc = w.contiguous()
        ctx.save_for_backward(x2, wc)
        ctx.has_bias = b is not None
        ctx.in_shape = x.shape
        y = ops.gemm(x2, wc, None if b is None else b.contiguous())
        return y.view(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, g):
        x2, w = ctx.saved_tensors
        g2 = g.reshape(-1, g.shape[-1]).contiguous()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = ops.gemm(g2, _t2(w)).view(ctx.in_shape)                      # (M,N) (N,K)
        if ctx.needs_input_grad[1]:
            gw = _gemm_over_rows(_t2(g2), _t2(x2))                             # (N,M) (M,K)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            ones = torch.ones((1, g2.shape[0]), device=g2.device, dtype=torch.float32)
            gb = _gemm_over_rows(ones, _t2(g2))[0]                             # column sums on the MFMA path
        return gx, gw, gb


def linear(x, w, b=None):
    return _Linear.apply(x, w, b)


class _HypersphereAttention(torch.autograd.Function):
    """Attention core on already projected (B, L, E) tensors; ``masked`` uint8 (B, Lq, S), ``row_any`` int32 (B, Lq)."""

    @staticmethod
    def forward(ctx, q, k, v, masked, row_any, heads, kappa):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        ctx.save_for_backward(q, k, v, masked, row_any)
        ctx.heads, ctx.kappa = heads, kappa
        return ops.hypersphere_attention(q, k, v, heads, masked=masked, row_any=row_any, kappa=kappa)

    @staticmethod
    def backward(ctx, g):
        q, k, v, masked, row_any = ctx.saved_tensors
        gq, gk, gv = ops.hypersphere_attention_backward(q, k, v, ctx.heads, g.contiguous(), masked=masked, row_any=row_any, kappa=ctx.kappa)
        return gq, gk, gv, None, None, None, None


class _MaskStep(torch.autograd.Function):
    """mask = einsum("bqc,bchw->bqhw", e, F) (DEC:668) plus the next layer's attention-mask bytes and row flags (DEC:675-680,
    non-differentiable outputs)."""

    @staticmethod
    def forward(ctx, e, feat, target_size):
        e, feat = e.contiguous(), feat.contiguous()
        ctx.save_for_backward(e, feat)
        mask, attn, row_any = ops.mask_logits(e, feat, want_mask=True, target_size=target_size)
        if attn is None:
            attn = torch.empty(0, device=e.device, dtype=torch.uint8)
            row_any = torch.empty(0, device=e.device, dtype=torch.int32)
        ctx.mark_non_differentiable(attn, row_any)
        return mask, attn, row_any

    @staticmethod
    def backward(ctx, g, _ga, _gr):
        e, feat = ctx.saved_tensors
        B, Q, C = e.shape
        HW = feat.shape[2] * feat.shape[3]
        g3 = g.reshape(B, Q, HW).contiguous()
        f3 = feat.view(B, C, HW)
        ge = gf = None
        if ctx.needs_input_grad[0]:
            ge = torch.stack([ops.gemm(g3[b], f3[b]) for b in range(B)])                       # (Q,HW) (HW,C)
        if ctx.needs_input_grad[1]:
            gf = torch.stack([ops.gemm(_t2(e[b]), _t2(g3[b])) for b in range(B)]).view_as(feat)   # (C,Q) (Q,HW)
        return ge, gf, None


def _unit(x, eps=1e-12):
    return x / x.norm(dim=-1, keepdim=True).clamp_min(eps)


def _attention(attn_mod, query, key, value, masked, row_any):
    """MeanShiftAttention.forward (AU:474-540, three-linear branch AU:134-140) on batch-major (B, L, E) tensors."""
    E = attn_mod.embed_dim
    w, b = attn_mod.in_proj_weight, attn_mod.in_proj_bias
    q = linear(query, w[:E], b[:E])
    k = linear(key, w[E:2 * E], b[E:2 * E])
    v = linear(value, w[2 * E:], b[2 * E:])
    o = _HypersphereAttention.apply(q, k, v, masked, row_any, attn_mod.num_heads, KAPPA)
    return linear(o, attn_mod.out_proj.weight, attn_mod.out_proj.bias)


def _heads(dec, out, mask_features, target_size):
    """forward_prediction_heads (DEC:660-682)."""
    d = F.layer_norm(out, (out.shape[-1],), dec.decoder_norm.weight, dec.decoder_norm.bias)
    cls = linear(d, dec.class_embed.weight, dec.class_embed.bias)
    e = d
    n = len(dec.mask_embed.layers)
    for j, layer in enumerate(dec.mask_embed.layers):
        e = linear(e, layer.weight, layer.bias)
        if j < n - 1:
            e = F.relu(e)
    mask, attn, row_any = _MaskStep.apply(e, mask_features, target_size)
    return cls, mask, (attn if target_size is not None else None), (row_any if target_size is not None else None)


def decoder_forward_train(dec, x, mask_features):
    """Differentiable MeanShiftTransformerDecoder.forward (DEC:540-658) for ``dec`` (modeling.MeanShiftTransformerDecoder or the
    single-level PretrainedMeanShiftTransformerDecoder): x list of (B, C, H_l, W_l) level maps, mask_features (B, mask_dim, H, W).
    Returns {"pred_logits", "pred_masks", "aux_outputs"} with autograd history through the HIP kernels."""
    from torch import nn
    L = dec.num_feature_levels
    assert len(x) == L
    B = x[0].shape[0]
    E = dec.query_feat.weight.shape[1]
    src, pos, sizes = [], [], []
    for i in range(L):
        h, w = int(x[i].shape[-2]), int(x[i].shape[-1])
        sizes.append((h, w))
        pos.append(dec._pos_tokens(h, w, x[i].device))                                    # (hw, E), input independent
        tok = x[i].flatten(2).transpose(1, 2)                                             # (B, hw, C)
        if isinstance(dec.input_proj[i], nn.Conv2d):
            tok = linear(tok, dec.input_proj[i].weight.view(E, -1), dec.input_proj[i].bias)
        src.append(tok + dec.level_embed.weight[i])                                       # DEC:575
    qpos = dec.query_embed.weight[None]
    out = dec.query_feat.weight[None].expand(B, -1, -1)
    pred_cls, pred_mask = [], []
    cls, mask, attn, row_any = _heads(dec, out, mask_features, sizes[0])
    pred_cls.append(cls)
    pred_mask.append(mask)
    for i in range(dec.num_layers):
        lvl = i % L                                                                       # DEC:608
        ca = dec.transformer_cross_attention_layers[i]
        t2 = _attention(ca.meanshift_attn, out + qpos, src[lvl] + pos[lvl], src[lvl], attn, row_any)      # DEC:245-253; row_any: DEC:618
        out = F.layer_norm(out + t2, (E,), ca.norm.weight, ca.norm.bias)
        sa = dec.transformer_self_attention_layers[i]
        qk = out + qpos
        t2 = _attention(sa.self_attn, qk, qk, out, None, None)                            # DEC:171-179
        out = F.layer_norm(out + t2, (E,), sa.norm.weight, sa.norm.bias)
        ff = dec.transformer_ffn_layers[i]
        t2 = linear(F.relu(linear(out, ff.linear1.weight, ff.linear1.bias)), ff.linear2.weight, ff.linear2.bias)
        out = F.layer_norm(out + t2, (E,), ff.norm.weight, ff.norm.bias)                  # DEC:296-304
        if dec.decoder_block_norm:
            out = _unit(out)                                                              # DEC:637-638
        last = i == dec.num_layers - 1
        cls, mask, attn, row_any = _heads(dec, out, mask_features, None if last else sizes[(i + 1) % L])
        pred_cls.append(cls)
        pred_mask.append(mask)
    return {"pred_logits": pred_cls[-1], "pred_masks": pred_mask[-1],
            "aux_outputs": [{"pred_logits": a, "pred_masks": b} for a, b in zip(pred_cls[:-1], pred_mask[:-1])]}


class _Conv3x3(torch.autograd.Function):
    """y = conv2d(x, weight, bias, padding=1) for a 64-channel map (SimpleBasePixelDecoder.mask_features, fpn.py:237-246,281-284): the
    forward is the inference path's (transpose to tokens, then the weight-stationary kernel when W % 4 == 0 and the implicit GEMM
    otherwise); backward: msm_conv3x3_c64_wgrad on the saved token map for weight and bias, ops.conv3x3_input_grad (the mirrored
    convolution of the gradient on the implicit GEMM) for the input.  fp32 only."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        B, C, H, W = x.shape
        Cout = weight.shape[0]
        if C != 64 or tuple(weight.shape) != (Cout, 64, 3, 3) or Cout % 64 or Cout > 1024:
            raise RuntimeError("training.conv3x3 needs x (B, 64, H, W) and weight (Cout, 64, 3, 3) with Cout a multiple of 64 up to 1024")
        tok = ops.transpose_last2(x.contiguous().view(B, C, H * W))                       # NHWC tokens
        w = weight.permute(0, 2, 3, 1).reshape(Cout, 9 * C).contiguous()
        y = ops.conv3x3_tokens_to_nchw(tok, w, None if bias is None else bias.contiguous(), int(H), int(W))
        ctx.save_for_backward(tok, weight)
        ctx.has_bias = bias is not None
        ctx.hw = (int(H), int(W))
        return y.view(B, Cout, H, W)

    @staticmethod
    def backward(ctx, g):
        tok, weight = ctx.saved_tensors
        H, W = ctx.hw
        g = g.contiguous()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = ops.conv3x3_input_grad(g, weight, H, W)
        want_bias = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or want_bias:
            dw, gb = ops.conv3x3_weight_grad(tok, g, H, W, want_bias=want_bias)
            if ctx.needs_input_grad[1]:
                Cout = weight.shape[0]
                gw = dw.view(Cout, 3, 3, 64).permute(0, 3, 1, 2).contiguous()              # tap-major -> (Cout, 64, 3, 3)
        return gx, gw, gb


def conv3x3(x, weight, bias=None):
    """Differentiable 3x3 / pad 1 convolution of a (B, 64, H, W) map, both passes in libmsm_hip.so: weight (Cout, 64, 3, 3),
    bias (Cout,) or None -> (B, Cout, H, W)."""
    return _Conv3x3.apply(x, weight, bias)


def head_forward_train(head, features):
    """Differentiable MeanShiftMaskFormerHead.layers for the RGB-D configuration (pixel decoder SimpleBasePixelDecoder + the
    single-level decoder; meanshift_former_head.py:121-126, fpn.py:274-290): ``features`` {"res5": (B, 64, H, W)} the channel-
    normalised embedding; mask_features = conv3x3(embedding) (the embedding itself when mask_dim == 64, fpn.py:281-284), then
    decoder_forward_train.  Returns {"pred_logits", "pred_masks", "aux_outputs"}; gradients reach the embedding, the convolution
    and the decoder.  The head's inference ``forward`` is untouched."""
    from .modeling import SimpleBasePixelDecoder
    pd = head.pixel_decoder
    if not isinstance(pd, SimpleBasePixelDecoder):
        raise NotImplementedError(f"head_forward_train: {type(pd).__name__} (MSDeformAttnPixelDecoder) is not yet differentiable; "
                                  "only SimpleBasePixelDecoder is")
    if len(pd.in_features) != 1:
        raise NotImplementedError("head_forward_train: the RGB-D pixel decoder takes one feature map (the embedding)")
    y = features[pd.in_features[0]]
    if pd.mask_dim == 64:
        mask_features = y
    else:
        mask_features = conv3x3(y, pd.mask_features.weight, pd.mask_features.bias)
    return decoder_forward_train(head.predictor, [y], mask_features)


class _GroupNormTokens(torch.autograd.Function):
    """GroupNorm (+ ReLU) of a token map (B, HW, C): forward ops.groupnorm_stats + ops.groupnorm_tokens, backward
    msm_groupnorm_bwd_f32 on the saved input and its float64 moments (the ReLU mask is recomputed from them)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, groups, eps, relu):
        x, gamma, beta = x.contiguous(), gamma.contiguous(), beta.contiguous()
        stats = ops.groupnorm_stats(x)
        y = ops.groupnorm_tokens(x, gamma, beta, x.shape[1], 1, groups, relu=relu, eps=eps, stats=stats, stats_ready=True)
        ctx.save_for_backward(x, stats, gamma, beta)
        ctx.cfg = (int(groups), float(eps), bool(relu))
        return y

    @staticmethod
    def backward(ctx, g):
        x, stats, gamma, beta = ctx.saved_tensors
        groups, eps, relu = ctx.cfg
        need = ctx.needs_input_grad
        if not any(need[:3]):
            return None, None, None, None, None, None
        dx, dg, db = ops.groupnorm_backward(x, g.contiguous(), stats, gamma, beta, groups, eps=eps, relu=relu, want_dx=need[0],
                                            want_dgamma=need[1], want_dbeta=need[2])
        return dx, dg, db, None, None, None


def group_norm_tokens(x, gamma, beta, groups=32, eps=1e-5, relu=False):
    """Differentiable GroupNorm (then ReLU when ``relu``) of a token map x (B, HW, C), both passes in libmsm_hip.so: C a multiple
    of 4 and of ``groups``, at most 256.  A frozen x, gamma or beta gets no gradient (and costs no work)."""
    return _GroupNormTokens.apply(x, gamma, beta, groups, eps, relu)


class _UpsampleBilinearTokens(torch.autograd.Function):
    """F.interpolate(size=HW, mode="bilinear", align_corners=False) on token maps (msdeformattn.py:349): forward
    msm_upsample_bilinear_tokens_f32, backward its gather-form adjoint."""

    @staticmethod
    def forward(ctx, x, hw, HW):
        C = x.shape[2]
        if x.stride(2) != 1 or x.stride(1) != C or (x.shape[0] > 1 and x.stride(0) < x.shape[1] * C):
            x = x.contiguous()
        ctx.sizes = (tuple(hw), tuple(HW))
        return ops.upsample_bilinear(x, hw, HW)

    @staticmethod
    def backward(ctx, g):
        hw, HW = ctx.sizes
        return ops.upsample_bilinear_backward(g.contiguous(), hw, HW), None, None


def upsample_bilinear_tokens(x, hw, HW):
    """Differentiable bilinear resize of a token map x (B, h*w, C) from ``hw`` = (h, w) to ``HW`` = (H, W) -> (B, H*W, C)."""
    return _UpsampleBilinearTokens.apply(x, hw, HW)


class _TransposeLast2(torch.autograd.Function):
    """(B, R, C) -> (B, C, R) contiguous through the library's transpose kernel, in both directions (NCHW planes <-> tokens)."""

    @staticmethod
    def forward(ctx, x):
        return ops.transpose_last2(x.contiguous())

    @staticmethod
    def backward(ctx, g):
        return ops.transpose_last2(g.contiguous())


class _Conv3x3Tokens(torch.autograd.Function):
    """The FPN output convolution (layer_1: 64 -> 64, 3x3 / pad 1, no bias; msdeformattn.py:272-281) on token maps in and out:
    forward msm_conv3x3_c64_f32, backward msm_conv3x3_c64_wgrad (Cout = 64) and the implicit GEMM on the mirrored taps, both without
    leaving the token layout (``_Conv3x3`` is the planes-out sibling for the mask_features convolution of the RGB-D head)."""

    @staticmethod
    def forward(ctx, tok, weight, H, W):
        if tok.dim() != 3 or tok.shape[2] != 64 or tuple(weight.shape) != (64, 64, 3, 3) or tok.shape[1] != H * W:
            raise RuntimeError("training: the FPN output convolution needs a (B, H*W, 64) token map and a (64, 64, 3, 3) weight")
        tok = tok.contiguous()
        y, _ = ops.conv3x3_c64(tok, weight.permute(0, 2, 3, 1).reshape(64, 576).contiguous(), int(H), int(W))
        ctx.save_for_backward(tok, weight)
        ctx.hw = (int(H), int(W))
        return y

    @staticmethod
    def backward(ctx, g):
        tok, weight = ctx.saved_tensors
        H, W = ctx.hw
        g = g.contiguous()
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = ops.conv3x3_input_grad_tokens(g, weight, H, W)
        if ctx.needs_input_grad[1]:
            dw, _ = ops.conv3x3_weight_grad(tok, ops.transpose_last2(g), H, W, want_bias=False)
            gw = dw.view(64, 3, 3, 64).permute(0, 3, 1, 2).contiguous()                   # tap-major -> (64, 64, 3, 3)
        return gx, gw, None, None


def _encoder_layer(layer, src, pos, ref, norm_wh, ss, starts):
    """MSDeformAttnTransformerEncoderLayer.forward (msdeformattn.py:116-131) with MSDeformAttn.forward (ms_deform_attn.py:95-125)
    written out: the projections are ``linear``, the core MSDeformAttnFunction; the softmax over the L * P logits and the location
    arithmetic (:101-109) are torch's row-local ops."""
    a = layer.self_attn
    B, S, C = src.shape
    M, L, P = a.n_heads, a.n_levels, a.n_points
    q = src + pos
    value = linear(src, a.value_proj.weight, a.value_proj.bias).view(B, S, M, C // M)
    off = linear(q, a.sampling_offsets.weight, a.sampling_offsets.bias).view(B, S, M, L, P, 2)
    aw = F.softmax(linear(q, a.attention_weights.weight, a.attention_weights.bias).view(B, S, M, L * P), -1).view(B, S, M, L, P)
    loc = ref[None, :, None, None, None, :] + off / norm_wh[None, None, None, :, None, :]
    o = MSDeformAttnFunction.apply(value, ss, starts, loc, aw, a.im2col_step)
    src = F.layer_norm(src + linear(o, a.output_proj.weight, a.output_proj.bias), (C,), layer.norm1.weight, layer.norm1.bias, layer.norm1.eps)
    f = linear(F.relu(linear(src, layer.linear1.weight, layer.linear1.bias)), layer.linear2.weight, layer.linear2.bias)
    return F.layer_norm(src + f, (C,), layer.norm2.weight, layer.norm2.bias, layer.norm2.eps)


def pixel_decoder_forward_train(pd, features):
    """Differentiable MSDeformAttnPixelDecoder.forward_features (msdeformattn.py:315-358) in the reference's literal order, for
    ``pd`` = modeling.MSDeformAttnPixelDecoder and ``features`` {"res2".."res5": (B, C_l, H_l, W_l)}: input projections (1x1
    convolution as ``linear`` on tokens, GroupNorm), sine position + level_embed (:61-85), the encoder layers, the per-level split,
    the res2 FPN step (lateral 1x1 + GroupNorm, + bilinear upsample, 3x3 output convolution + GroupNorm + ReLU) and the 1x1
    mask_features convolution.  Returns (mask_features (B, mask_dim, H, W), transformer_encoder_features, multi_scale_features) as
    forward_features does; gradients reach every parameter of ``pd`` and the four feature maps.  Heavy operators run in
    libmsm_hip.so in both directions (GEMMs, MSDeformAttn core, GroupNorm, upsampling, 3x3 convolution, transposes); LayerNorm over
    the conv_dim-wide rows, the softmax over L * P logits, ReLU and the adds are torch's.  Neither the inference ``forward_features`` nor
    any cache of ``pd`` is touched.  fp32; conv_dim 64 (the 3x3 kernels), DROPOUT 0 (every shipped yaml)."""
    if getattr(pd, "transformer_dropout", 0.0) > 0:
        raise NotImplementedError("pixel_decoder_forward_train: transformer dropout > 0 is not implemented (every shipped yaml has DROPOUT: 0.0)")
    C = pd.conv_dim
    if C != 64:
        raise NotImplementedError("pixel_decoder_forward_train: the 3x3 convolution backward needs conv_dim == 64")
    names = pd.transformer_in_features[::-1]                                              # res5, res4, res3
    dev = features[names[0]].device
    B = features[names[0]].shape[0]
    toks, pos, ref, shapes = [], [], [], []
    for idx, f in enumerate(names):
        x = features[f].float()
        h, w = int(x.shape[2]), int(x.shape[3])
        shapes.append((h, w))
        conv, gn = pd.input_proj[idx][0], pd.input_proj[idx][1]
        t = linear(_TransposeLast2.apply(x.reshape(B, x.shape[1], h * w)), conv.weight.view(C, -1), conv.bias)
        toks.append(group_norm_tokens(t, gn.weight, gn.bias, gn.num_groups, gn.eps))
        pos.append(ops.pos_embed_sine(h, w, pd.pe_layer.num_pos_feats, dev, layout="tokens") + pd.transformer.level_embed[idx])   # :75
        ys = (torch.arange(h, device=dev, dtype=torch.float32) + 0.5) / h                  # pixel centres, valid ratio 1 (:141-153)
        xs = (torch.arange(w, device=dev, dtype=torch.float32) + 0.5) / w
        ref.append(torch.stack([xs[None, :].expand(h, w), ys[:, None].expand(h, w)], -1).reshape(h * w, 2))
    src = torch.cat(toks, 1)
    pos, ref = torch.cat(pos, 0), torch.cat(ref, 0)
    sizes = [h * w for h, w in shapes]
    starts_host = [sum(sizes[:i]) for i in range(len(sizes))]
    ss = torch.tensor(shapes, dtype=torch.int64, device=dev)
    starts = torch.tensor(starts_host, dtype=torch.int64, device=dev)
    norm_wh = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float32, device=dev)   # ms_deform_attn.py:104
    for layer in pd.transformer.encoder.layers:
        src = _encoder_layer(layer, src, pos, ref, norm_wh, ss, starts)
    levels = [src[:, o:o + n] for o, n in zip(starts_host, sizes)]                        # (B, h*w, C) token ranges
    out = [z.transpose(1, 2).view(B, C, h, w) for z, (h, w) in zip(levels, shapes)]       # NCHW-shaped views, as forward_features returns
    # the one FPN level on res2 (:343-351)
    x = features[pd.in_features[0]].float()
    H, W = int(x.shape[2]), int(x.shape[3])
    lat = linear(_TransposeLast2.apply(x.reshape(B, x.shape[1], H * W)), pd.adapter_1.weight.view(C, -1), None)
    an, ln = pd.adapter_1.norm, pd.layer_1.norm
    y = group_norm_tokens(lat, an.weight, an.bias, an.num_groups, an.eps) + upsample_bilinear_tokens(levels[-1], shapes[-1], (H, W))
    y = _Conv3x3Tokens.apply(y, pd.layer_1.weight, H, W)
    y = group_norm_tokens(y, ln.weight, ln.bias, ln.num_groups, ln.eps, relu=True)
    out.append(_TransposeLast2.apply(y).view(B, C, H, W))
    mf = linear(y, pd.mask_features.weight.view(pd.mask_dim, C), pd.mask_features.bias)
    mask_features = _TransposeLast2.apply(mf).view(B, pd.mask_dim, H, W)
    return mask_features, out[0], out[:pd.maskformer_num_feature_levels]


def segmentation_head_forward_train(head, features):
    """Differentiable MeanShiftMaskFormerHead.layers for the ResNet-50 configuration (meanshift_former_head.py:121-126):
    pixel_decoder_forward_train, then decoder_forward_train on its multi-scale features and mask features.  Returns
    {"pred_logits", "pred_masks", "aux_outputs"}; gradients reach every parameter of the head and the backbone feature maps.
    (The RGB-D head, whose pixel decoder is SimpleBasePixelDecoder, is ``head_forward_train``'s.)"""
    from .modeling import MSDeformAttnPixelDecoder
    pd = head.pixel_decoder
    if not isinstance(pd, MSDeformAttnPixelDecoder):
        raise NotImplementedError(f"segmentation_head_forward_train: {type(pd).__name__} is not MSDeformAttnPixelDecoder; "
                                  "head_forward_train trains the SimpleBasePixelDecoder head")
    mask_features, _, multi_scale_features = pixel_decoder_forward_train(pd, features)
    return decoder_forward_train(head.predictor, multi_scale_features, mask_features)


def segmentation_head_losses(head, features, targets, criterion):
    """One training step of the ResNet-50 head from the backbone's feature maps to the weighted loss dict
    (tabletop_train_net_pretrained.py:209-246): segmentation_head_forward_train -> ``criterion`` -> weighted_losses."""
    return weighted_losses(criterion(segmentation_head_forward_train(head, features), targets), criterion.weight_dict)


def weighted_losses(losses, weight_dict):
    """meanshiftformer_model.py:279-285: every loss with a weight in ``weight_dict`` times that weight; the others dropped."""
    return {k: v * weight_dict[k] for k, v in losses.items() if k in weight_dict}


def decoder_losses(dec, x, mask_features, targets, criterion):
    """decoder_forward_train -> criterion (criterion.SetCriterion) -> weighted_losses: the weighted loss dict of one training
    step of the decoder; ``sum(decoder_losses(...).values()).backward()`` runs every backward on the HIP kernels."""
    return weighted_losses(criterion(decoder_forward_train(dec, x, mask_features), targets), criterion.weight_dict)


def _head_losses_normalised(head, norm, targets, criterion, labels, embedding_loss, embedding_weight):
    """head_losses after its normalisation: ``norm`` (B, 64, H, W) is the channel-normalised embedding."""
    outputs = head_forward_train(head, {head.pixel_decoder.in_features[0]: norm})
    losses = criterion(outputs, targets)
    weights = dict(criterion.weight_dict)
    if embedding_loss is not None:
        losses["embedding_loss"] = embedding_loss(norm, labels)[0]
        weights["embedding_loss"] = embedding_weight
    return weighted_losses(losses, weights)


def head_losses(head, embedding, targets, criterion, *, labels=None, embedding_loss=None, embedding_weight=None):
    """The training branch of the RGB-D meta-arch (pretrained_meanshiftformer_model.py:298-333) from the backbone's embedding
    (B, 64, H, W) to the weighted loss dict: F.normalize over channels (once), head_forward_train, ``criterion``, and -- with
    ``embedding_loss`` (embedding_loss.EmbeddingLoss; ``labels`` and ``embedding_weight`` are then required) --
    losses["embedding_loss"] = embedding_loss(normalised, labels)[0] times that weight.  ``criterion.weight_dict`` is left as it is
    (the reference writes the embedding weight into it, :323)."""
    if embedding_loss is not None and (labels is None or embedding_weight is None):
        raise ValueError("head_losses: embedding_loss needs labels and embedding_weight")
    norm = F.normalize(embedding, p=2, dim=1)
    return _head_losses_normalised(head, norm, targets, criterion, labels, embedding_loss, embedding_weight)


# ---------------------------------------------------------------------------------------------------------------------------
# the UCN RGB-D backbone under autograd (lib/fcn/train.py:37-76 trains it against EmbeddingLoss; the RGB-D meta-arch leaves it
# unfrozen, pretrained_meanshiftformer_model.py:150-152)
# ---------------------------------------------------------------------------------------------------------------------------
def _tail_torch(a, b, size, norms, eps):
    """The definition of the embedding tail: nn.functional.upsample_bilinear of each tower, add fusion, F.normalize ``norms`` times
    (resnet_dilated.py:325, SEG.py:104-114, pretrained_meanshiftformer_model.py:298)."""
    u = F.interpolate(a, size=size, mode="bilinear", align_corners=True)
    if b is not None:
        u = u + F.interpolate(b, size=size, mode="bilinear", align_corners=True)
    for _ in range(norms):
        u = F.normalize(u, p=2, dim=1, eps=eps)
    return u


class _UCNEmbeddingTail(torch.autograd.Function):
    """ops.ucn_embedding_tail forward, msm_ucn_embedding_tail_bwd backward (u and the normalised vectors are recomputed from the
    saved low-resolution maps; the full-resolution output is not kept for the backward)."""

    @staticmethod
    def forward(ctx, a, b, size, norms, eps):
        cl = lambda t: t if t.is_contiguous(memory_format=torch.channels_last) else t.contiguous(memory_format=torch.channels_last)
        a = cl(a)
        b = None if b is None else cl(b)
        ctx.save_for_backward(a, b)
        ctx.cfg = (int(norms), float(eps))
        return ops.ucn_embedding_tail(a, b, size, norms=norms, eps=eps)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        need_a, need_b = ctx.needs_input_grad[0], b is not None and ctx.needs_input_grad[1]
        if not (need_a or need_b):
            return None, None, None, None, None
        norms, eps = ctx.cfg
        gin = ops.ucn_embedding_tail_bwd(a, b, g.contiguous(), norms=norms, eps=eps)     # y.sum().backward() hands over stride 0
        return (gin if need_a else None), (gin if need_b else None), None, None, None


def ucn_embedding_tail(a, b, size, norms=1, eps=1e-12, fused=True):
    """Differentiable tail of the UCN backbone: a, b (B, 64, h, w) fp32 low-resolution maps of the two towers in any memory format
    (b None: one tower) -> (B, 64, H, W) = N(..N(upsample_bilinear(a) + upsample_bilinear(b))) for size = (H, W), N = F.normalize over
    the channels applied ``norms`` (0..2) times.  fused: ops.ucn_embedding_tail forward and the msm_ucn_embedding_tail_bwd kernels
    backward (one gradient tensor for both towers); ``fused=False`` or host tensors: the literal torch expression, which is the
    definition."""
    norms = int(norms)
    if norms < 0 or norms > 2:
        raise ValueError("ucn_embedding_tail: norms must be 0, 1 or 2")
    size = (int(size[0]), int(size[1]))
    if not fused or not a.is_cuda:
        return _tail_torch(a, b, size, norms, eps)
    return _UCNEmbeddingTail.apply(a, b, size, norms, eps)


def _tower_forward_train(tower, x):
    """Resnet34_8s up to its 1/8-resolution embedding (resnet_dilated.py:287-327 without the upsampling; resnet.py:43-73,248-258)
    through the tower's own modules: nothing folded, every BatchNorm2d follows its own ``training`` flag."""
    net = tower.resnet34_8s
    x = F.max_pool2d(F.relu(net.bn1(net.conv1(x))), 3, stride=2, padding=1)
    for i in range(4):
        for blk in getattr(net, f"layer{i + 1}"):
            y = F.relu(blk.bn1(blk.conv1(x)))
            y = blk.bn2(blk.conv2(y))
            x = F.relu(y + (x if blk.downsample is None else blk.downsample(x)))
    return net.fc(x)


def ucn_towers_forward_train(backbone, img, depth=None):
    """The two towers of ``backbone`` (ucn_backbone.UCNBackbone) under autograd -> (lo_a, lo_b or None), the (B, num_units, h, w)
    1/8-resolution maps the tail upsamples.  conv1 -> bn1 -> ReLU -> max-pool -> BasicBlocks -> fc through the modules themselves
    (MIOpen convolutions and their autograd): a BatchNorm2d in training mode normalises with batch statistics and updates its running
    statistics (the reference's ``network.train()``, lib/fcn/train.py:43), one in eval mode uses its running statistics.  One stream,
    fp32; neither ``backbone.forward`` nor its folded-weight cache is touched."""
    from ._plan import miopen_find
    if backbone.backbone_dtype != "f32":
        raise NotImplementedError("ucn_towers_forward_train: fp32 only (backbone_dtype is %r)" % (backbone.backbone_dtype,))
    if depth is not None and backbone.fcn_depth is None:
        raise RuntimeError("this backbone was built without a depth tower")
    with miopen_find(bool(getattr(backbone, "miopen_find", True)) and img.is_cuda):
        lo_a = _tower_forward_train(backbone.fcn, img.float())
        lo_b = _tower_forward_train(backbone.fcn_depth, depth.float()) if depth is not None else None
    return lo_a, lo_b


def ucn_backbone_forward_train(backbone, img, depth=None, *, renormalize=False, fused_tail=True):
    """``backbone(img, None, depth)`` under autograd -> (B, 64, H, W): ucn_towers_forward_train, then ucn_embedding_tail with
    norms = backbone.normalize + renormalize (``renormalize``: the meta-arch's F.normalize of the backbone's output,
    pretrained_meanshiftformer_model.py:298, inside the tail).  Works whatever ``backbone.training`` is: the BatchNorm modules decide
    for themselves."""
    lo_a, lo_b = ucn_towers_forward_train(backbone, img, depth)
    if fused_tail and lo_a.is_cuda and lo_a.shape[1] != 64:
        raise NotImplementedError("ucn_backbone_forward_train: the fused tail needs num_units == 64 (fused_tail=False runs torch's)")
    norms = (1 if backbone.normalize else 0) + (1 if renormalize else 0)
    return ucn_embedding_tail(lo_a, lo_b, img.shape[2:], norms=norms, fused=fused_tail)


def ucn_model_losses(model, image, depth, targets, criterion, *, labels=None, embedding_loss=None, embedding_weight=None):
    """The training branch of the RGB-D meta-arch from images (pretrained_meanshiftformer_model.py:283-333) for ``model`` =
    meta_arch.PretrainedMeanShiftMaskFormer: image (B, 3, H, W) and depth (B, 3, H, W) xyz (None: colour only), normalised and padded
    as ``model`` takes them -> the weighted loss dict.  The backbone runs under autograd (ucn_backbone_forward_train) with the
    meta-arch's F.normalize (:298) as the tail's second normalisation, the rest is head_losses after its normalisation: the
    embedding loss sees the same normalised tensor (:318 normalises a unit vector again).  Gradients reach every parameter of the
    backbone and of the head."""
    if embedding_loss is not None and (labels is None or embedding_weight is None):
        raise ValueError("ucn_model_losses: embedding_loss needs labels and embedding_weight")
    norm = ucn_backbone_forward_train(model.backbone, image, depth if model.use_depth else None, renormalize=True)
    return _head_losses_normalised(model.sem_seg_head, norm, targets, criterion, labels, embedding_loss, embedding_weight)


def ucn_embedding_losses(network, image, label, depth=None, *, embedding_loss):
    """The training branch of the UCN embedding network (SEGNET.forward lib/networks/SEG.py:88-120 with its embedding loss, as
    train_segnet calls it, lib/fcn/train.py:57) for ``network`` = ucn_backbone.UCNBackbone and ``embedding_loss`` =
    embedding_loss.EmbeddingLoss: image (B, 3, H, W), label (B, 1, H, W) cluster ids, depth (B, 3, H, W) xyz or None ->
    (loss, intra_cluster_loss, inter_cluster_loss, features), features (B, num_units, H, W) under autograd
    (ucn_backbone_forward_train).  ``loss.backward()`` reaches every parameter of the towers that ran."""
    features = ucn_backbone_forward_train(network, image, depth)
    loss, intra, inter = embedding_loss(features, label)
    return loss, intra, inter, features
