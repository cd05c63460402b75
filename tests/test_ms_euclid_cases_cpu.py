"""The float64 definitions of tests/ms_euclid_cases.py against the reference's recorded results
(tests/golden/mean_shift_euclidean.npz, made by tests/golden/make_golden_ms_euclidean.py), the conditions under which the GPU tests
may compare exactly, and the host-side contract of metric="euclidean".  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import ms_euclid_cases as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", E.GOLDEN_CASES)
def test_definitions_reproduce_the_reference(case, golden):
    g = golden("mean_shift_euclidean")
    X, _ = E.planted(case)
    assert E.checksum(X) == pytest.approx(float(g[f"c{case}_checksum"]), rel=1e-12)
    assert int(g[f"c{case}_first"]) == E.first_index(case)
    h = E.smart_init64(case)
    assert np.array_equal(h["sel"].numpy(), g[f"c{case}_sel"])
    assert np.abs(h["Z"].numpy() - g[f"c{case}_Z64"]).max() <= 1e-12
    assert np.abs(h["Z"].numpy() - g[f"c{case}_Z_ref"].astype(np.float64)).max() <= 1e-6
    assert np.array_equal(h["seed_labels"].numpy(), g[f"c{case}_seed_labels"])
    assert np.array_equal(h["labels"].numpy(), g[f"c{case}_labels"].astype(np.int64))
    # the fp32 direct-difference form of the helper is the reference's arithmetic
    Z32, _ = E.hill32(X, X[h["sel"]], E.KAPPA, E.ITERS)
    assert np.abs(Z32.numpy() - g[f"c{case}_Z_ref"]).max() <= 1e-6


@pytest.mark.parametrize("case", E.GOLDEN_CASES)
def test_exact_comparisons_are_legitimate(case, golden):
    g = golden("mean_shift_euclidean")
    h = E.smart_init64(case)
    margin = float(h["seeding"]["margin"][1:].min())
    print(f"case {case}: smallest relative top-2 margin of a seeding step {margin:.3e}")
    assert margin >= 1e-4
    assert E.eps_margin(h["Z"]) >= 1e-4 and E.eps_margin(torch.from_numpy(g[f"c{case}_Z_ref"])) >= 1e-4
    counts = np.sort(np.bincount(g[f"c{case}_labels"].astype(np.int64)))
    assert counts[-1] > counts[-2]                               # the largest-cluster swap has one answer


@pytest.mark.parametrize("case", range(len(E.CASES)))
def test_far_seed_takes_the_clamp_branch(case):
    X, _ = E.planted(case)
    _, sw = E.hill64(X, E.far_seed(case)[None], E.KAPPA, 1)
    assert 0.0 < float(sw[0]) < 0.5
    assert float(torch.cdist(E.far_seed(case)[None].double(), X.double()).min()) > 0.5 * E.CASES[case][5]


def test_chain_is_order_dependent():
    """The hand-built chain: the float64 restatement gives the labels worked out by hand in ms_euclid_cases (mode branch, tie,
    overwritten neighbour), no pair sits on epsilon, and the same seeds in line order merge into one label per run."""
    Z = E.chain()
    labels, (alive, created) = E.components64(Z, E.EPS)
    assert E.eps_margin(Z) >= 5e-3
    assert labels.tolist() == E.CHAIN_LABELS and (alive, created) == (6, 6)
    plain, num = E.components64(Z[torch.argsort(Z[:, 1])], E.EPS)
    assert plain.tolist() == [0] * 6 + [1] * 12 and num == (2, 2)


def test_header_declares_the_entry_points():
    from unseenobjectswithmeanshift_amd import _lib
    with open(os.path.join(ROOT, "include", "msm_hip.h")) as f:
        src = f.read()
    names = ["msm_ms_select_seeds_l2", "msm_ms_hill_climb_l2", "msm_ms_hill_climb_l2_workspace", "msm_ms_assign_l2",
             "msm_ms_connected_components_l2"]
    declared = set(_lib.declared_symbols())
    for name in names:
        assert re.search(r"\b%s\(" % name, src) and name in declared
    assert int(re.search(r"#define\s+MSM_ABI_VERSION\s+(\d+)", src).group(1)) >= 32
    L = _lib.lib()
    assert all(hasattr(L, name) for name in names)
    # 65 floats per seed row and workgroup: the weights' sum rides with the partial sums
    assert L.msm_ms_hill_climb_l2_workspace(1000, 20) * 64 == L.msm_ms_hill_climb_workspace(1000, 20) * 65


def test_host_tensors_and_bad_arguments_raise():
    from unseenobjectswithmeanshift_amd import mean_shift as ms
    from unseenobjectswithmeanshift_amd import two_stage as ts
    X, _ = E.planted(1)
    Z = X[:5].contiguous()
    calls = [lambda: ms.ball_kernel(Z, X, 20.0, metric="euclidean"),
             lambda: ms.connected_components(Z, E.EPS, metric="euclidean"),
             lambda: ms.seed_hill_climbing_ball(X, Z, 20.0, metric="euclidean"),
             lambda: ms.mean_shift_with_seeds(X, Z, 20.0, metric="euclidean"),
             lambda: ms.select_smart_seeds(X, 5, metric="euclidean", first_index=0),
             lambda: ms.mean_shift_smart_init(X, 20.0, num_seeds=5, metric="euclidean", first_index=0),
             lambda: ms.mean_shift_smart_init_batched(X[None], 20.0, num_seeds=5, first_indices=[0], metric="euclidean"),
             lambda: ms.clustering_features(X[:32].t().reshape(1, 64, 4, 8), num_seeds=5, metric="euclidean")]
    for call in calls:
        with pytest.raises(NotImplementedError):
            call()
    for precision in ("f32_split", "bf16"):
        with pytest.raises(ValueError):
            ms.mean_shift_smart_init(X, 20.0, num_seeds=5, metric="euclidean", first_index=0, precision=precision)
        with pytest.raises(ValueError):
            ms.seed_hill_climbing_ball(X, Z, 20.0, metric="euclidean", precision=precision)
        with pytest.raises(ValueError):
            ms.clustering_features(X[:32].t().reshape(1, 64, 4, 8), num_seeds=5, metric="euclidean", precision=precision)
    for call in (lambda: ms.connected_components(Z, E.EPS, metric="manhattan"),
                 lambda: ms.mean_shift_smart_init(X, 20.0, num_seeds=5, metric="l2", first_index=0),
                 lambda: ms.clustering_features(X[:32].t().reshape(1, 64, 4, 8), metric="")):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(NotImplementedError):                     # init_seeds keeps raising, whatever the metric
        ms.select_smart_seeds(X, 5, init_seeds=Z, num_init_seeds=1)
    # the harness forwards the metric to the default clustering only; host tensors still need a caller's cluster
    import inspect
    for fn in (ts.test_sample_clustering, ts.test_batch_clustering):
        assert inspect.signature(fn).parameters["metric"].default == "cosine"
