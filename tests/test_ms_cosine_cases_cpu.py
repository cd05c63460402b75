"""The float64 definitions of tests/ms_cosine_cases.py against oracle/msm_oracle.py (fp32, the reference's arithmetic) and the
reference's recorded results (tests/golden/mean_shift.npz), and the properties of the inputs without which the GPU tests of
tests/test_gpu_meanshift_cosine.py would pass vacuously.  No GPU."""
import numpy as np
import pytest
import torch

import ms_cosine_cases as C
from oracle import msm_oracle as O
from unseenobjectswithmeanshift_amd import synthetic as syn


def _replay_agrees(X, S, first, picks):
    """Replay ``picks`` in float64: every pick is a maximum to 2 E, and the float64 argmax itself wherever the step's margin exceeds
    2 E.  -> the replay."""
    r = C.seeding64(X, S, first, forced=np.asarray(picks))
    assert (r["pick"][1:] >= r["top"][1:] - 2 * C.E).all()
    clear = r["margin"] > 2 * C.E
    assert (r["idx"][clear] == r["best"][clear]).all()
    return r


# ---- the definitions against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.ALL)
def test_seeding_against_the_oracle(case):
    X, _ = C.planted(case)
    S = C.CASES[case][3]
    seeds, idx = O.select_smart_seeds(X, S, C.first_index(case))
    r = _replay_agrees(X, S, C.first_index(case), idx.numpy())
    assert int(idx[0]) == C.first_index(case) and torch.equal(seeds, X[idx])
    own = C.seeds64(case)
    assert len(set(own["idx"].tolist())) == S and own["idx"][0] == C.first_index(case)
    if float(own["margin"][1:].min(initial=np.inf)) > 2 * C.E:     # no near tie anywhere: the two sequences are the same
        assert np.array_equal(r["idx"], own["idx"])


@pytest.mark.parametrize("iters", [1, C.ITERS])
@pytest.mark.parametrize("case", C.ALL)
def test_hill_climb_against_the_oracle(case, iters):
    """hill32 is the oracle's arithmetic; err32, the yardstick of the GPU test, is a few fp32 roundings of coordinates of magnitude
    0.1 ... 1 (measured 2.4e-8 ... 1.8e-7 over the table; it depends on the host's BLAS and thread count): never 0, which would
    leave the GPU test its floor only, never above 4e-7 = 7 ulps of 1."""
    X, _ = C.planted(case)
    h = C.hill_case(case, iters)
    Zo = O.seed_hill_climbing_ball(X, h["Z0"], C.KAPPA, iters)
    assert float((Zo.double() - h["Z64"]).abs().max()) <= 1e-6 and float((Zo - h["Z32"]).abs().max()) <= 1e-6
    assert float((h["Z64"].norm(dim=1) - 1).abs().max()) <= 1e-12
    print(f"case {case} iters {iters}: err32 {h['err32']:.2e}  far seed {h['err32_far']:.2e}")
    assert 1e-8 <= h["err32"] <= 4e-7
    if C.CASES[case][3] > 1:
        assert 0.0 < h["err32_far"] <= h["err32"]
        dots = X.double() @ h["Z0"][-1].double()
        assert -0.95 <= float(dots.min()) and float(dots.max()) <= 0.1          # behind every point: each weight is tiny


@pytest.mark.parametrize("case", C.MULTI)
def test_smart_init_against_the_oracle(case):
    """The float64 pipeline and the oracle's fp32 one find the same clusters (near ties of the seeding may number them differently),
    the largest as label 0."""
    X, _ = C.planted(case)
    S = C.CASES[case][3]
    labels, sel, Z, seed_labels = O.mean_shift_smart_init(X, C.KAPPA, S, C.ITERS, C.first_index(case), C.EPS)
    own = C.smart_init64(case)
    _replay_agrees(X, S, C.first_index(case), sel.numpy())
    assert C.same_partition(labels, own["labels"])
    assert int(torch.bincount(labels).argmax()) == 0 and int(torch.bincount(own["labels"]).argmax()) == 0
    if np.array_equal(sel.numpy(), own["sel"].numpy()):
        assert float((Z.double() - own["Z"]).abs().max()) <= 1e-6
        assert torch.equal(seed_labels, own["seed_labels"]) and torch.equal(labels, own["labels"])


# ---- the definitions against the reference's recorded results --------------------------------------------------------------------
def test_definitions_reproduce_the_golden_pieces(golden):
    g = golden("mean_shift")
    X, _ = C.planted(0)                                             # the map of the golden's pieces, another first index
    first = int(g["s_first"])
    r = _replay_agrees(X, 20, first, g["s_sel"])
    own = C.seeding64(X, 20, first)
    assert float(own["margin"][1:].min()) > 2 * C.E and np.array_equal(own["idx"], g["s_sel"]) and np.array_equal(r["idx"], own["idx"])
    seeds = torch.from_numpy(g["s_seeds"])
    assert torch.equal(seeds, X[torch.from_numpy(own["idx"])])
    Z = C.hill64(X, seeds, C.KAPPA, C.ITERS)
    assert float((Z - torch.from_numpy(g["s_Z"]).double()).abs().max()) <= 1e-6
    assert C.eps_margin(Z) >= 1e-4
    assert np.array_equal(O.connected_components(Z, C.EPS).numpy(), g["s_cc"])
    W = torch.exp(C.KAPPA * (seeds.double() @ X.double().t()))
    assert np.allclose(W.sum(1).numpy(), g["s_kernel_sum"], rtol=1e-5, atol=0)


def test_definitions_reproduce_the_golden_clustering(golden):
    g = golden("mean_shift")
    X, _ = syn.synth_unit_embeddings(4800, 64, clusters=8, sigma=0.15, seed=18)
    first = int(g["a_first"])
    _replay_agrees(X, 50, first, g["a_sel"])
    Z = C.hill64(X, X[torch.from_numpy(g["a_sel"])], C.KAPPA, C.ITERS)
    seed_labels = O.connected_components(Z, C.EPS)
    labels = seed_labels[torch.argmin(C.dist64(X, Z), dim=1)]
    labels = C.relabel_largest_zero(labels, len(torch.unique(seed_labels)))
    assert torch.equal(labels, torch.from_numpy(g["a_labels"]).long())


# ---- the conditions on the inputs ------------------------------------------------------------------------------------------------
def test_the_bound():
    assert C.E == 64 * 2.0 ** -24 * 0.5 + 2.0 ** -24 and 1.9e-6 < C.E < 2.1e-6
    for case in C.ALL:
        assert float((C.planted(case)[0].double().norm(dim=1) - 1).abs().max()) <= 2e-7      # unit rows: E holds as it stands
    assert C.hill_bound(0.0) == 2.0 ** -22 and C.hill_bound(1e-7) == 4e-7


def test_the_table_reaches_every_path():
    """What the sizes were chosen for (the host's dispatch rules, restated)."""
    n = [c[0] for c in C.CASES]
    S = [c[3] for c in C.CASES]
    assert n[1] < 16 == n[2] and S[2] == 16 and S[3] == 1 and S[4] == 17 and n[4] % 16 == 15 and n[0] % 16 == 0
    assert n[5] >= 4096 and n[5] % 16 and n[6] == 4096 and S[6] == 128
    assert C.launch_widths(S[0]) == [2] and C.launch_widths(S[5]) == [4] and C.launch_widths(S[6]) == [8]
    assert C.launch_widths(S[7]) == [5, 4] and C.launch_widths(S[8]) == [7, 7, 5] and C.launch_widths(S[9]) == [3]
    slabs = -(-n[7] // 16)
    assert (slabs + 3) // 4 > 512 and slabs - 2048 == 2 and n[7] % 16 == 5      # grid capped at 512 x 4 waves: two second slabs
    assert S[7] % 16 == 1 and -(-S[7] // 128) == 2 and -(-S[8] // 128) == 3 and S[8] == 304
    # MS_CHUNK = 1 .. 8 on 19 seed blocks: the widest launch of each walk; 6 and 8 come from 16 k seeds launched on their own
    assert [max(C.launch_widths(304, cap)) for cap in range(1, 9)] == [1, 2, 3, 4, 5, 5, 7, 7]
    assert [C.launch_widths(16 * k) for k in range(1, 9)] == [[k] for k in range(1, 9)]
    for tag, tiles in (("ng2", 2), ("ng3", 3)):
        m = C.SEED_MAPS[tag][0]
        assert -(-m // 131072) == tiles and -(-(m - 16) // 131072) == tiles - 1 and m % 16 == 3
    m = C.SEED_MAPS["bf16"][0]
    assert m > 393216 and m % 32 and m % 16


@pytest.mark.parametrize("case", C.EXACT_SEEDING)
def test_small_maps_have_unique_picks(case):
    assert float(C.seeds64(case)["margin"][1:].min()) >= 1e-5


@pytest.mark.parametrize("case", C.ALL)
def test_raw_seeds_show_the_argmin(case):
    """Assignment (a): on the raw seeds at most 1 % of the points have a runner-up within 2 E; the float64 argmin passes its own
    check, a neighbouring seed does not."""
    X, _ = C.planted(case)
    Z = X[torch.from_numpy(C.seeds64(case)["idx"])]
    am = torch.argmin(C.dist64(X, Z), dim=1)
    chk = C.assign_check(X, Z, am)
    print(f"case {case}: {100 * chk['ambiguous']:.2f} % of the points are ambiguous")
    assert chk["admissible"] and chk["exact"] and chk["ambiguous"] <= 0.01
    assert len(set(am.tolist())) == Z.shape[0]                      # distinct seeds: each one wins at least itself
    if Z.shape[0] > 1:
        wrong = C.assign_check(X, Z, (am + 1) % Z.shape[0])
        assert not wrong["admissible"] and not wrong["exact"]


@pytest.mark.parametrize("case", C.MULTI)
def test_behind_seeds_expose_the_padding(case):
    """For at least half of the points every seed of behind_seeds is farther than 0.5 + 2 E: a zero padding row would win them."""
    X, _ = C.planted(case)
    Z = C.behind_seeds(case)
    d = C.dist64(X, Z)
    assert float((d.min(dim=1).values > 0.5 + 2 * C.E).float().mean()) >= 0.5
    assert float((Z.double().norm(dim=1) - 1).abs().max()) <= 2e-7
    assert C.assign_check(X, Z, torch.argmin(d, dim=1))["ambiguous"] <= 0.02


@pytest.mark.parametrize("case", C.MULTI)
def test_float64_pipeline_recovers_the_planted_partition(case):
    _, ids = C.planted(case)
    own = C.smart_init64(case)
    assert C.same_partition(own["labels"], ids)
    assert C.eps_margin(own["Z"]) >= 1e-4                           # measured 4e-2: seeds either coincide or are far apart
    counts = torch.sort(torch.bincount(own["labels"])).values
    assert counts[-1] > counts[-2] and int(torch.bincount(own["labels"]).argmax()) == 0
    assert not C.same_partition(torch.where(torch.arange(len(ids)) == 0, own["labels"].max() + 1, own["labels"]), ids)


def test_tie_rows():
    X, _ = C.planted(C.LIMIT)
    Z = C.tie_seeds()
    raw = X[torch.from_numpy(C.seeds64(C.LIMIT)["idx"])]
    d = C.dist64(X, Z)
    am = torch.argmin(d, dim=1)                                     # first argmin: never a copy
    for src, dst in C.TIES:
        assert src < dst and torch.equal(Z[dst], Z[src]) and torch.equal(Z[src], raw[src]) and not torch.equal(raw[dst], raw[src])
        won = am == src
        assert int(won.sum()) >= 1 and int((am == dst).sum()) == 0
        others = d[won].clone()
        others[:, [src, dst]] = np.inf
        assert float((others.min(dim=1).values - d[won][:, src]).min()) > 2 * C.E       # only the copy is near
    # same block, another lane | same lane, the next block | same lane and block position, the next chunk of eight blocks
    (a, b), (c, e), (f, h) = C.TIES
    assert a // 16 == b // 16 and a % 16 != b % 16
    assert c % 16 == e % 16 and e // 16 == c // 16 + 1
    assert f % 16 == h % 16 and (h // 16) % 8 == (f // 16) % 8 and h // 128 == f // 128 + 1


def test_euclidean_limit_case():
    import ms_euclid_cases as L2
    h = C.euclid_limit_case()
    assert h["Z0"].shape == (304, 64) and torch.unique(h["Z0"], dim=0).shape[0] == 304
    assert h["err32"] <= 5e-7 and float(L2.hill64(h["X"], h["Z0"][-1:], L2.KAPPA, 1)[1][0]) < 0.5
