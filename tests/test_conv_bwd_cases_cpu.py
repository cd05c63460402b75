"""The 3x3 convolution backward's yardstick and interface, without a GPU: the float64 definition of tests/conv_bwd_cases.py against
an independent nine-term restatement, the structural zeros of the cases, the header / ABI of msm_conv3x3_c64_wgrad and the training
entry points' argument checks."""
import re

import pytest
import torch

import conv_bwd_cases as CC
from unseenobjectswithmeanshift_amd import _lib


@pytest.mark.parametrize("name", list(CC.CASES))
def test_definition_matches_restatement(name):
    ref, alt = CC.reference64(name), CC.restatement64(name)
    for k in ("y", "dx", "dw", "db"):
        assert ref[k].dtype == torch.float64 and ref[k].shape == alt[k].shape
        scale = float(ref[k].abs().max())
        assert float((ref[k] - alt[k]).abs().max()) <= 1e-12 * scale, (name, k)


@pytest.mark.parametrize("name", list(CC.CASES))
def test_structural_zeros(name):
    z = CC.structural_zero_taps(name)
    dw = CC.reference64(name)["dw"]
    expect = {"px1": 8, "row": 6, "col": 6, "edges": 6}.get(name, 0)
    assert int(z.sum()) == expect
    if expect:
        assert float(dw[:, :, z].abs().max()) == 0.0                                        # exactly, in the definition itself
    assert float(dw[:, :, ~z].abs().amax(dim=(0, 1)).min()) > 0.0                           # every other tap carries data


def test_planted_inputs():
    for name, c in CC.CASES.items():
        x, w, bias, g = CC.planted(name)
        assert tuple(x.shape) == (c.B, 64, c.H, c.W) and tuple(w.shape) == (c.Cout, 64, 3, 3)
        assert tuple(bias.shape) == (c.Cout,) and tuple(g.shape) == (c.B, c.Cout, c.H, c.W)
        assert c.Cout % 64 == 0 and all(t.dtype == torch.float32 for t in (x, w, bias, g))
        n = x.norm(dim=1)
        if name == "edges":
            assert float(x[..., 1:-1].abs().max()) == 0.0 and float(g[..., 1:-1].abs().max()) == 0.0
            n = n[..., [0, -1]]
        assert float((n - 1).abs().max()) < 1e-6
    assert CC.CASES["wide"].W % 4 == 0 and CC.CASES["odd"].W % 4 and CC.CASES["odd"].H * CC.CASES["odd"].W == 65


def test_tap_major_layout():
    w = torch.arange(64 * 64 * 9, dtype=torch.float64).view(64, 64, 3, 3)
    t = CC.tap_major(w)
    assert float(t[5, (2 * 3 + 1) * 64 + 7]) == float(w[5, 7, 2, 1])


def test_header_and_abi():
    names = {"msm_conv3x3_c64_wgrad", "msm_conv3x3_c64_wgrad_workspace"}
    assert names <= set(_lib.declared_symbols()) and names <= set(_lib._SIGNATURES)
    with open(_lib.HEADER_PATH) as f:
        header_abi = int(re.search(r"#define\s+MSM_ABI_VERSION\s+(\d+)", f.read()).group(1))
    assert _lib.ABI_VERSION == header_abi >= 35                             # 34: the ABI before msm_conv3x3_c64_wgrad
    assert _lib._HEADER.params["msm_conv3x3_c64_wgrad"][-2:] == ["splits", "stream"]
    assert _lib._HEADER.params["msm_conv3x3_c64_wgrad_workspace"] == ["B", "H", "W", "Cout", "splits"]


def test_workspace_query():
    L = _lib.lib()
    assert L.msm_conv3x3_c64_wgrad_workspace(3, 5, 13, 128, 3) == 3 * 128 * 577
    assert L.msm_conv3x3_c64_wgrad_workspace(1, 1, 1, 64, 0) == 64 * 577           # one pixel: one range
    auto = L.msm_conv3x3_c64_wgrad_workspace(8, 480, 640, 256, 0)
    assert auto > 0 and auto % (256 * 577) == 0
    for bad in ((0, 4, 4, 64, 0), (1, 0, 4, 64, 0), (1, 4, 0, 64, 0), (1, 4, 4, 96, 0), (1, 4, 4, 1088, 0), (1, 4, 4, 64, -1),
                (1, 4, 4, 64, 4097)):
        assert L.msm_conv3x3_c64_wgrad_workspace(*bad) == -1


def test_training_entry_points_exist():
    from unseenobjectswithmeanshift_amd import ops, training
    for fn in (training.conv3x3, training.head_forward_train, training.head_losses, ops.conv3x3_weight_grad, ops.conv3x3_input_grad):
        assert callable(fn)
    assert issubclass(training._Conv3x3, torch.autograd.Function)


def test_head_forward_train_rejects_the_resnet50_head():
    from unseenobjectswithmeanshift_amd import training
    from unseenobjectswithmeanshift_amd.meta_arch import build_resnet50_head
    head = build_resnet50_head(num_queries=4, dec_layers=1, enc_layers=1)
    with pytest.raises(NotImplementedError, match="MSDeformAttnPixelDecoder"):
        training.head_forward_train(head, {"res5": torch.zeros(1, 64, 4, 4)})


def test_host_tensors_raise():
    from unseenobjectswithmeanshift_amd import ops, training
    x, w, bias, g = CC.planted("row")
    tok = x.flatten(2).transpose(1, 2).contiguous()
    with pytest.raises(RuntimeError, match="GPU"):
        ops.conv3x3_weight_grad(tok, g, 1, 7)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.conv3x3_input_grad(g, w, 1, 7)
    with pytest.raises(RuntimeError, match="GPU"):
        training.conv3x3(x, w, bias)


def test_head_losses_needs_labels_with_embedding_loss():
    from unseenobjectswithmeanshift_amd import training
    with pytest.raises(ValueError, match="labels"):
        training.head_losses(None, torch.zeros(1, 64, 2, 2), [], None, embedding_loss=object())
