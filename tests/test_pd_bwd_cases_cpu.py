"""The pixel-decoder backward's yardsticks and interface, without a GPU: the float64 definitions of tests/pd_bwd_cases.py against
independent restatements (the closed GroupNorm-backward formula written out with sums; the upsampling matrix built entry by entry
and transposed), the header / ABI of the new entry points, their argument checks, and the golden file of the pixel-decoder case."""
import os
import re

import numpy as np
import pytest
import torch

import pd_bwd_cases as K
from unseenobjectswithmeanshift_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pixel_decoder_backward.npz")


@pytest.mark.parametrize("name", list(K.GN_CASES))
def test_groupnorm_definition_matches_restatement(name):
    ref, alt = K.gn_reference64(name), K.gn_restatement64(name)
    for k in ("y", "dx", "dgamma", "dbeta"):
        assert ref[k].dtype == torch.float64 and ref[k].shape == alt[k].shape
        # px1: a group of two values leaves ~eps / var of gamma * g in dx, so float64 itself keeps ~1e-12 of it there
        tol = 1e-10 if name == "px1" else 1e-12
        assert float((ref[k] - alt[k]).abs().max()) <= tol * float(ref[k].abs().max()), (name, k)


@pytest.mark.parametrize("name", list(K.UP_CASES))
def test_upsample_definition_matches_restatement(name):
    ref, alt = K.up_reference64(name), K.up_restatement64(name)
    for k in ("y", "dx"):
        assert ref[k].dtype == torch.float64 and ref[k].shape == alt[k].shape
        assert float((ref[k] - alt[k]).abs().max()) <= 1e-12 * float(ref[k].abs().max()), (name, k)


def test_planted_inputs_and_cases():
    assert {n: tuple(c[:5]) for n, c in K.GN_CASES.items()} == {
        "px1": (1, 1, 64, 32, False), "row": (2, 7, 64, 32, True), "odd": (3, 65, 64, 32, True), "wide4": (2, 36, 128, 32, False),
        "c256": (1, 33, 256, 32, True), "tall": (1, 660, 64, 32, True)}
    assert [tuple(c[:4]) for c in K.UP_CASES.values()] == [(2, 3, 4, 6), (2, 3, 5, 7), (1, 1, 3, 4), (1, 5, 1, 10), (15, 20, 30, 40),
                                                           (3, 4, 3, 4)]
    assert K.GN_SPLIT_CASES == ("odd", "tall") and K.GN_SPLITS == (1, 3, 7) and K.RTOL == 1e-4 and (K.UP_B, K.UP_C) == (2, 64)
    for name, c in K.GN_CASES.items():
        x, gamma, beta, g = K.gn_planted(name)
        assert tuple(x.shape) == tuple(g.shape) == (c.B, c.HW, c.C) and tuple(gamma.shape) == tuple(beta.shape) == (c.C,)
        assert all(t.dtype == torch.float32 for t in (x, gamma, beta, g))
        ref = K.gn_reference64(name)
        if c.relu:
            assert ref["margin"] > K.RELU_MARGIN                                  # no pre-ReLU value near the kink
            assert 0.2 < float((ref["y"] == 0).double().mean()) < 0.8            # the mask is neither empty nor full
    same = K.up_reference64("same")
    assert torch.equal(same["y"], K.up_planted("same")[0].double()) and torch.equal(same["dx"], K.up_planted("same")[1].double())


def test_header_and_abi():
    names = {"msm_groupnorm_bwd_f32", "msm_groupnorm_bwd_workspace", "msm_upsample_bilinear_bwd_tokens_f32",
             "msm_upsample_bilinear_tokens_f32"}
    assert names <= set(_lib.declared_symbols()) and names <= set(_lib._SIGNATURES)
    with open(_lib.HEADER_PATH) as f:
        header_abi = int(re.search(r"#define\s+MSM_ABI_VERSION\s+(\d+)", f.read()).group(1))
    assert _lib.ABI_VERSION == header_abi >= 36                             # 35: the ABI before the pixel-decoder backward
    assert _lib._HEADER.params["msm_groupnorm_bwd_f32"][-4:] == ["eps", "relu", "splits", "stream"]
    assert _lib._HEADER.params["msm_groupnorm_bwd_workspace"] == ["B", "HW", "C", "groups", "splits"]
    assert _lib._HEADER.params["msm_upsample_bilinear_bwd_tokens_f32"] == ["gout", "gin", "B", "h", "w", "H", "W", "C", "stream"]
    L = _lib.lib()
    assert all(hasattr(L, n) for n in names)


def test_workspace_query():
    L = _lib.lib()
    # doubles counted in floats: B * splits * 2 * C range sums + B * 2 * C image sums
    assert L.msm_groupnorm_bwd_workspace(3, 65, 64, 32, 7) == 2 * (3 * 7 * 2 * 64 + 3 * 2 * 64)
    assert L.msm_groupnorm_bwd_workspace(1, 1, 64, 32, 0) == 2 * (2 * 64 + 2 * 64)                # one pixel: one range
    assert L.msm_groupnorm_bwd_workspace(1, 660, 64, 32, 0) == 2 * (3 * 2 * 64 + 2 * 64)          # ranges of 256 pixels
    assert L.msm_groupnorm_bwd_workspace(8, 120 * 160, 64, 32, 0) == 2 * (8 * 75 * 2 * 64 + 8 * 2 * 64)
    for bad in ((0, 4, 64, 32, 0), (1, 0, 64, 32, 0), (1, 4, 66, 33, 0), (1, 4, 64, 48, 0), (1, 4, 320, 32, 0), (1, 4, 64, 0, 0),
                (1, 4, 64, 32, -1), (1, 4, 64, 32, 4097), (65536, 4, 64, 32, 0)):
        assert L.msm_groupnorm_bwd_workspace(*bad) == -1, bad
        assert b"msm_groupnorm_bwd_workspace" in L.msm_last_error_string()


def test_entry_points_exist():
    from unseenobjectswithmeanshift_amd import ops, training
    for fn in (ops.groupnorm_backward, ops.upsample_bilinear_backward, ops.upsample_bilinear, ops.conv3x3_input_grad_tokens,
               training.group_norm_tokens, training.upsample_bilinear_tokens, training.pixel_decoder_forward_train,
               training.segmentation_head_forward_train, training.segmentation_head_losses):
        assert callable(fn)
    for cls in (training._GroupNormTokens, training._UpsampleBilinearTokens, training._Conv3x3Tokens):
        assert issubclass(cls, torch.autograd.Function)


def test_host_tensors_raise():
    from unseenobjectswithmeanshift_amd import ops, training
    x, gamma, beta, g = K.gn_planted("row")
    stats = torch.zeros(2, 64, 2, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.groupnorm_backward(x, g, stats, gamma, beta, 32, relu=True)
    with pytest.raises(RuntimeError, match="GPU"):
        training.group_norm_tokens(x, gamma, beta, relu=True)
    ux, ug = K.up_planted("x2")
    with pytest.raises(RuntimeError, match="GPU"):
        ops.upsample_bilinear_backward(ug, (2, 3), (4, 6))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.upsample_bilinear(ux, (2, 3), (4, 6))
    with pytest.raises(RuntimeError, match="GPU"):
        training.upsample_bilinear_tokens(ux, (2, 3), (4, 6))


def test_pixel_decoder_train_argument_checks():
    from unseenobjectswithmeanshift_amd import training
    from unseenobjectswithmeanshift_amd.meta_arch import build_resnet50_head, build_ucn_head
    head = build_resnet50_head(num_queries=4, dec_layers=1, enc_layers=1)
    head.pixel_decoder.transformer_dropout = 0.1
    with pytest.raises(NotImplementedError, match="dropout"):
        training.pixel_decoder_forward_train(head.pixel_decoder, {})
    with pytest.raises(NotImplementedError, match="head_forward_train"):
        training.segmentation_head_forward_train(build_ucn_head(num_queries=4, dec_layers=1), {})


def test_golden_file():
    assert os.path.getsize(GOLDEN) < 1024 * 1024
    z = np.load(GOLDEN)
    seed = int(z["seed"])
    coord, relu, worst32 = (float(v) for v in z["margins"])
    assert coord > 1e-4 and relu > 1e-5 and worst32 <= 0.25               # the generator's three seed conditions
    sd = K.pd_state_dict(seed)
    feats = K.pd_features(seed)
    keys = ["out__mask_features", "out__ms0", "out__ms1", "out__ms2"] + ["g_in__" + k for k in feats] + ["g__" + k for k in sd]
    assert sorted(k for k in z.files if not k.startswith("err32__") and k not in ("seed", "margins")) == sorted(keys)
    for k in keys:
        ref = z[k]
        assert ref.dtype == np.float32 and np.isfinite(ref).all() and float(np.abs(ref).max()) > 0
        # the reference's own fp32 run stays within a quarter of the contract on every tensor
        assert float(z["err32__" + k]) <= 0.25 * K.RTOL * float(np.abs(ref).max()), k
    assert z["out__mask_features"].shape == (K.PD_BATCH, K.PD_MASK_DIM // K.PD_MF_STRIDE, 12, 20)
    assert z["out__ms0"].shape == (2, 64, 2, 3) and z["out__ms2"].shape == (2, 64, 6, 10)
    for k, v in feats.items():
        assert z["g_in__" + k].shape == tuple(v.shape)
    for k, v in sd.items():
        assert z["g__" + k].shape == tuple(v.shape)
