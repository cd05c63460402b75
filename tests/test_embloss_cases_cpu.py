"""EmbeddingLoss without a GPU: the float64 definition of tests/embloss_cases.py against the reference's own results
(tests/golden/embedding_loss.npz), the conditions the cases promise, the C ABI and the module's argument checks."""
import inspect
import re

import pytest
import torch

import embloss_cases as EC
from unseenobjectswithmeanshift_amd import _lib


def _rel(a, b):
    return abs(a - b) / abs(b) if b != 0 else abs(a)


@pytest.mark.parametrize("name", EC.GOLDEN_CASES)
def test_definition_matches_reference(golden, name):
    G = golden("embedding_loss")
    x, _ = EC.planted(name)
    assert abs(EC.checksum(x) - float(G[f"{name}_checksum"])) <= 1e-9 * max(1.0, abs(float(G[f"{name}_checksum"])))
    r = EC.reference64(name)
    for got, want in zip((r["loss"], r["intra"], r["inter"]), G[f"{name}_losses64"]):
        assert _rel(got, float(want)) <= 1e-12
    flat = r["grad"].reshape(-1)
    gmax = float(G[f"{name}_grad_max"])
    sample = flat if name == "0" else flat[EC.grad_sample_index(flat.numel())]
    assert float((sample - torch.from_numpy(G[f"{name}_grad"])).abs().max()) <= 1e-10 * gmax
    assert abs(float(flat.abs().max()) - gmax) <= 1e-10 * gmax
    assert abs(float(flat.sum()) - float(G[f"{name}_grad_sum"])) <= 1e-10 * gmax * flat.numel() ** 0.5
    # the reference's own fp32 run: the yardstick of the GPU test's errors (recorded in DESIGN.md)
    assert float(G[f"{name}_loss32_err"]) <= 1e-5 and float(G[f"{name}_grad32_err"]) <= 1e-5


@pytest.mark.parametrize("name", list(EC.CASES))
def test_case_conditions(name):
    case, r = EC.CASES[name], EC.reference64(name)
    x, labels = EC.planted(name)
    assert x.dtype == torch.float32 and tuple(x.shape) == (case.B, case.C, case.H, case.W) and r["K"] == case.K
    in_cluster = r["labelled"] & ~r["stray"]
    assert float(((r["d"] - EC.ALPHA).abs()[in_cluster]).min()) >= EC.MARGIN
    assert 0.05 < float((~r["labelled"]).double().mean())                   # unlabelled pixels in every case
    if name.startswith("6"):
        assert r["intra"] == 0.0 and int(r["N"].sum()) == 0
    else:
        assert r["intra"] > 0
    if name in ("0", "3", "4", "5"):
        assert r["inter"] > 0
    if name in ("1", "6k1"):
        assert r["K"] == 1 and r["inter"] == 0.0
    if name == "6k1":
        assert r["loss"] == 0.0 and float(r["grad"].abs().max()) == 0.0
    if name == "6":
        assert r["inter"] > 0 and float(r["grad"].abs().max()) > 0
    if name in ("0", "3", "7i", "7s"):
        assert int(r["n"][:, 1].sum()) == 0                                 # cluster 1 is empty in every image
    if name == "0":
        N = r["N"][r["n"] > 0]
        assert int((N > 50).sum()) > 0 and int(((N > 0) & (N < 50)).sum()) > 0 and case.H * case.W % 4 != 0
    if name == "4":
        assert int(r["N"].max()) < 50 and case.K * case.C == 16384 and int(r["n"].min()) > 0
    if name == "5":
        assert not bool(r["labelled"][1].any()) and int(r["n"][2, 1:].sum()) == 0 and int(r["n"][2, 0]) > 0
    if name == "7i":
        assert labels.dtype == torch.int64
    if name == "7s":
        assert int(r["stray"].sum()) == 9 and r["intra"] > EC.reference64("0")["intra"]
    # the gradient is 0 on unlabelled pixels
    assert float(r["grad"].permute(0, 2, 3, 1)[~r["labelled"].reshape(case.B, case.H, case.W)].abs().max()) == 0.0


def test_header_and_abi():
    declared = set(_lib.declared_symbols())
    assert {"msm_embloss_workspace", "msm_embloss_fwd", "msm_embloss_bwd"} <= declared
    assert {"msm_embloss_workspace", "msm_embloss_fwd", "msm_embloss_bwd"} <= set(_lib._SIGNATURES)
    with open(_lib.HEADER_PATH) as f:
        header_abi = int(re.search(r"#define\s+MSM_ABI_VERSION\s+(\d+)", f.read()).group(1))
    assert _lib.ABI_VERSION == header_abi >= 34                             # 33: the ABI before msm_embloss_*
    assert _lib._HEADER.params["msm_embloss_fwd"][-1] == "stream" and _lib._HEADER.params["msm_embloss_bwd"][-1] == "stream"


def test_workspace_query_limits():
    L = _lib.lib()
    assert L.msm_embloss_workspace(2, 64, 943, 64) > 0
    assert L.msm_embloss_workspace(1, 256, 1024, 64) > 0
    for bad in ((1, 256, 1024, 65), (1, 0, 16, 4), (0, 4, 16, 4), (1, 4, 0, 4), (1, 4, 16, 0), (1, 1, 16, 1025)):
        assert L.msm_embloss_workspace(*bad) == -1


def test_module_argument_checks():
    from unseenobjectswithmeanshift_amd import ops
    from unseenobjectswithmeanshift_amd.embedding_loss import EmbeddingLoss
    assert ops.embloss_max_clusters(64) == 64 and ops.embloss_max_clusters(256) == 64 and ops.embloss_max_clusters(1024) == 16
    assert ops.embloss_max_clusters(7) == 64 and ops.embloss_max_clusters(16, 1024) == 1024
    labels = torch.zeros(1, 1, 4, 4)
    with pytest.raises(ValueError, match="max_clusters"):                   # max_clusters * C > 16384
        EmbeddingLoss(0.02, 0.5, 1.0, 1.0, max_clusters=65)(torch.zeros(1, 256, 4, 4), labels)
    with pytest.raises(ValueError, match="max_clusters"):
        EmbeddingLoss(0.02, 0.5, 1.0, 1.0)(torch.zeros(1, 16385, 4, 4), labels)
    with pytest.raises(ValueError, match="C must be at least 1"):            # C < 1
        EmbeddingLoss(0.02, 0.5, 1.0, 1.0)(torch.zeros(1, 0, 4, 4), labels)
    with pytest.raises(RuntimeError, match="GPU"):                          # a host tensor: there is no CPU path
        EmbeddingLoss(0.02, 0.5, 1.0, 1.0)(torch.zeros(1, 8, 4, 4), labels)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.embloss_fwd(torch.zeros(1, 8, 4, 4), labels, 0.02, 0.5, 1.0, 1.0)
    with pytest.raises(RuntimeError, match="float32"):                      # a dtype other than fp32
        EmbeddingLoss(0.02, 0.5, 1.0, 1.0)(torch.zeros(1, 8, 4, 4, dtype=torch.float64), labels)
    with pytest.raises(RuntimeError, match="float32"):
        EmbeddingLoss(0.02, 0.5, 1.0, 1.0)(torch.zeros(1, 8, 4, 4, dtype=torch.float16), labels)
    with pytest.raises(ValueError, match="metric"):
        EmbeddingLoss(0.02, 0.5, 1.0, 1.0, metric="manhattan")


def test_module_shape():
    from unseenobjectswithmeanshift_amd.embedding_loss import EmbeddingLoss
    crit = EmbeddingLoss(0.02, 0.5, 1.0, 1.0)
    assert len(crit.state_dict()) == 0 and list(crit.parameters()) == [] and list(crit.buffers()) == []
    params = list(inspect.signature(EmbeddingLoss.__init__).parameters.values())
    assert [p.name for p in params] == ["self", "alpha", "delta", "lambda_intra", "lambda_inter", "metric", "normalize", "max_clusters"]
    assert params[5].default == "cosine" and params[6].default is True
    assert params[7].kind is inspect.Parameter.KEYWORD_ONLY and params[7].default is None
    crit = EmbeddingLoss(0.02, 0.5, 1.0, 2.0, "euclidean", False)           # the reference's positional order
    assert (crit.alpha, crit.delta, crit.lambda_intra, crit.lambda_inter, crit.metric, crit.normalize) == (0.02, 0.5, 1.0, 2.0, "euclidean", False)
    assert crit.last_status is None
    crit.check()                                                            # nothing to report before a call
