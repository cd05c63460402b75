"""The classic clustering for M maps of one size per call (ops.ms_*_batched, mean_shift.mean_shift_smart_init_batched, the
batched route of mean_shift.clustering_features) against the single-map ops called in a loop with the same first indices.
The single-map ops are the M = 1 case of the same kernels and entry points, so what these tests prove is that a map's result
does not depend on M, on its neighbours or on how maps are spread over launches -- every comparison is torch.equal, never a
tolerance.  That one map is computed correctly is checked against references in tests/test_gpu_ops.py and test_gpu_modules.py.
Needs a real MI355X (pytest -m gpu)."""
import numpy as np
import pytest
import torch

from unseenobjectswithmeanshift_amd import synthetic as syn

pytestmark = pytest.mark.gpu

DEV = "cuda"


def ops():
    from unseenobjectswithmeanshift_amd import ops as _ops
    return _ops


def ms():
    from unseenobjectswithmeanshift_amd import mean_shift as _ms
    return _ms


_MAPS = {}


def maps(M, n, sigma=0.2):
    """(X (M,n,64) on the device, first indices): every map has its own number of clusters, its own points and its own first
    index, so a group that reads a neighbour's rows, keys or exchange slots cannot reproduce the loop."""
    key = (M, n, sigma)
    if key not in _MAPS:
        X = torch.stack([syn.synth_unit_embeddings(n, 64, clusters=5 + 2 * m, sigma=sigma, seed=(n + 31 * m) % 997)[0] for m in range(M)])
        first = [(n // 3 + 997 * m) % n for m in range(M)]
        _MAPS[key] = (X.to(DEV), first)
    return _MAPS[key]


_LOOP_SEEDS = {}


def loop_seeds(M, n, S):
    """The partner: ops.ms_select_seeds per map (computed once per case, with the library's default kernel choice)."""
    key = (M, n, S)
    if key not in _LOOP_SEEDS:
        X, first = maps(M, n)
        pairs = [ops().ms_select_seeds(X[m], S, first[m]) for m in range(M)]
        _LOOP_SEEDS[key] = (torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs]))
    return _LOOP_SEEDS[key]


# (M, n, S): smallest persistent map | n no multiple of 16, 4 workgroups per map | 224 x 224 crops: 33 workgroups per map, seven
# maps per launch -> two launches (7 + 2) | 98 workgroups per map, two maps per launch | one map: the M = 1 launch policy (8
# workgroups of one tile) with a device first index against the same entry point with a host scalar; with one map the
# neighbour half of the give-up check compares empty tensors, only the -1 half says anything
@pytest.mark.parametrize("M,n,S", [(2, 4096, 3), (9, 5003, 40), (9, 50176, 100), (3, 150000, 40), (1, 4096, 3)])
def test_seeding_grouped(M, n, S):
    X, first = maps(M, n)
    seeds_l, sel_l = loop_seeds(M, n, S)
    seeds, sel = ops().ms_select_seeds_batched(X, S, first)
    assert int(sel.min()) >= 0                                        # -1 would mean a group gave up
    assert sel[:, 0].tolist() == first
    assert torch.equal(sel, sel_l) and torch.equal(seeds, seeds_l)
    # the grouped persistent form served this shape: only it reads the give-up flag (the stepwise form would return map 0's indices)
    _, sel_g = ops().ms_select_seeds_batched(X, S, first, _test_give_up=[0])
    assert int(sel_g[0].max()) == -1 and torch.equal(sel_g[1:], sel_l[1:])
    # a device tensor of first indices is taken without a host round trip
    seeds_d, sel_d = ops().ms_select_seeds_batched(X, S, torch.tensor(first, device=DEV))
    assert torch.equal(sel_d, sel_l) and torch.equal(seeds_d, seeds_l)


# (3, 15, 5): fewer rows than the butterfly's 16; (1, 15, 5): the same kernel with a host scalar as first index on the partner's side
@pytest.mark.parametrize("M,n,S", [(3, 15, 5), (3, 1000, 20), (9, 5003, 40), (1, 15, 5)])
def test_seeding_stepwise(M, n, S, lib_option):
    X, first = maps(M, n)
    seeds_l, sel_l = loop_seeds(M, n, S)
    grouped = ops().ms_select_seeds_batched(X, S, first)              # n < 4096 takes the stepwise form by itself
    by_flag = ops().ms_select_seeds_batched(X, S, first, stepwise=True)
    lib_option("MS_NO_PERSISTENT", 1)
    by_option = ops().ms_select_seeds_batched(X, S, first)
    for seeds, sel in (grouped, by_flag, by_option):
        assert torch.equal(sel, sel_l) and torch.equal(seeds, seeds_l)
    assert sel_l[:, 0].tolist() == first and int(sel_l.min()) >= 0


def test_seeding_rejects_bad_first_indices():
    X, first = maps(3, 1000)
    with pytest.raises(RuntimeError):
        ops().ms_select_seeds_batched(X, 20, [0, 1000, 5])
    with pytest.raises(RuntimeError):
        ops().ms_select_seeds_batched(X, 20, first[:2])


def test_give_up_is_per_map_and_falls_back():
    """The simulated give-up flag (as test_mean_shift_seeding_give_up_falls_back uses for one map): the batched op reports -1 for
    the affected maps only; mean_shift_smart_init_batched re-runs those stepwise and returns the clean run's results."""
    M, n, S = 3, 20000, 30
    X, first = maps(M, n, sigma=0.15)
    seeds_c, sel_c = ops().ms_select_seeds_batched(X, S, first)
    _, sel = ops().ms_select_seeds_batched(X, S, first, _test_give_up=[0, 2])
    assert int(sel[0].max()) == -1 and int(sel[2].max()) == -1        # reported, not fabricated
    assert torch.equal(sel[1], sel_c[1]) and int(sel_c.min()) >= 0     # the neighbour in the same launch is untouched
    clean = [ms().mean_shift_smart_init(X[m], kappa=20, num_seeds=S, max_iters=10, first_index=first[m]) for m in range(M)]
    labels, sel = ms().mean_shift_smart_init_batched(X, kappa=20, num_seeds=S, max_iters=10, first_indices=first, _test_give_up=[0, 2])
    for m in range(M):
        assert torch.equal(sel[m], clean[m][1]) and torch.equal(labels[m], clean[m][0])
    assert torch.equal(sel, sel_c)


# 130 seeds are more than 8 x 16 = 128: nine seed blocks, two chunks per iteration; the M = 1 cases walk them with one map's strides
@pytest.mark.parametrize("M,n,S,iters", [(3, 1000, 20, 2), (2, 50176, 100, 10), (5, 5003, 130, 3), (1, 1000, 20, 2), (1, 5003, 130, 1)])
def test_hill_climb(M, n, S, iters):
    X, _ = maps(M, n)
    Z0 = X[:, :: n // S][:, :S].contiguous()
    Z = ops().ms_hill_climb_batched(X, Z0, 20.0, iters)
    for m in range(M):
        assert torch.equal(Z[m], ops().ms_hill_climb(X[m], Z0[m], 20.0, iters))
    assert not torch.equal(Z, Z0)


def test_merge_assign_relabel():
    M, n, S = 4, 5003, 40
    X, first = maps(M, n)
    X = X.clone()
    X[0] = syn.synth_unit_embeddings(n, 64, clusters=1, sigma=0.15, seed=77)[0].to(DEV)     # one blob: every seed merges
    seeds, _ = ops().ms_select_seeds_batched(X, S, first)
    Z = ops().ms_hill_climb_batched(X, seeds, 20.0, 10)
    seed_labels, num = ops().ms_connected_components_batched(Z, 0.04)
    labels, counts = ops().ms_assign_batched(X, Z, seed_labels, S)
    before = labels.clone()
    ops().ms_relabel_largest_zero_batched(labels, counts, num)
    assert int(num[0, 0]) == 1 and int(num[1, 0]) >= 5                 # what the inputs are built for
    for m in range(M):
        sl, nm = ops().ms_connected_components(Z[m], 0.04)
        lab, cnt = ops().ms_assign(X[m], Z[m], sl, S)
        assert torch.equal(seed_labels[m], sl) and torch.equal(num[m], nm)
        assert torch.equal(before[m], lab) and torch.equal(counts[m], cnt)
        assert torch.equal(counts[m], torch.bincount(lab, minlength=S))
        assert torch.equal(labels[m], ops().ms_relabel_largest_zero(lab, cnt, nm))
    # without num_alive every entry of counts takes part, per map
    again = before.clone()
    ops().ms_relabel_largest_zero_batched(again, counts)
    for m in range(M):
        assert torch.equal(again[m], ops().ms_relabel_largest_zero(before[m].clone(), counts[m]))
    # one map may pass the count alone (mean_shift._components_with_count does): element 0 of a map's pair is all that is read
    assert torch.equal(ops().ms_relabel_largest_zero(before[0].clone(), counts[0], num[0, :1]), labels[0])


def _features(M, H, W):
    X, first = maps(M, H * W)
    return X.transpose(1, 2).reshape(M, 64, H, W).contiguous(), first


@pytest.mark.parametrize("M,H,W,S", [(9, 224, 224, 100), (2, 48, 64, 100)])
def test_clustering_features_equals_per_map(M, H, W, S):
    feats, first = _features(M, H, W)
    out, sel = ms().clustering_features(feats, num_seeds=S, first_indices=first)
    assert out.shape == (M, H, W) and out.dtype == torch.float32 and len(sel) == M
    for m in range(M):
        o1, s1 = ms().clustering_features(feats[m:m + 1], num_seeds=S, first_indices=first[m:m + 1])     # B = 1: the per-map path
        assert torch.equal(out[m], o1[0]) and torch.equal(sel[m], s1[0])
    # chunks of map_batch maps change nothing
    out2, sel2 = ms().clustering_features(feats, num_seeds=S, first_indices=first, map_batch=4)
    assert torch.equal(out2, out) and all(torch.equal(a, b) for a, b in zip(sel2, sel))


def test_clustering_features_draws_like_the_loop():
    feats, _ = _features(3, 48, 64)
    np.random.seed(3)
    out, sel = ms().clustering_features(feats)
    np.random.seed(3)
    loop = [ms().clustering_features(feats[m:m + 1]) for m in range(3)]
    for m in range(3):
        assert torch.equal(out[m], loop[m][0][0]) and torch.equal(sel[m], loop[m][1][0])
    # the other plans keep the loop (and its return types)
    np.random.seed(3)
    out_s, sel_s = ms().clustering_features(feats, precision="f32_split")
    assert all(torch.equal(a, b) for a, b in zip(sel_s, sel)) and out_s.shape == out.shape


def test_against_the_goldens(golden):
    """The two 4800-point maps of tests/golden/mean_shift.npz stacked twice with swapped order: both copies give the fixture."""
    g = golden("mean_shift")
    Xa, _ = syn.synth_unit_embeddings(4800, 64, clusters=8, sigma=0.15, seed=18)
    Xn, _ = syn.synth_unit_embeddings(4800, 64, clusters=8, sigma=0.15, seed=33, background_frac=0.02)
    order = ["a", "n", "n", "a"]
    X = torch.stack([Xa if t == "a" else Xn for t in order]).to(DEV)
    first = [int(g[f"{t}_first"]) for t in order]
    labels, sel = ms().mean_shift_smart_init_batched(X, kappa=20, num_seeds=50, max_iters=10, first_indices=first)
    for m, t in enumerate(order):
        assert torch.equal(sel[m].cpu(), torch.from_numpy(g[f"{t}_sel"]))
        assert torch.equal(labels[m].cpu(), torch.from_numpy(g[f"{t}_labels"]).long())
