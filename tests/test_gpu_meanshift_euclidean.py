"""The Euclidean metric of the mean-shift clustering on the HIP path (msm_ms_*_l2, ops.ms_*(metric="euclidean"),
mean_shift.*(metric="euclidean")) against the float64 definitions of tests/ms_euclid_cases.py and the reference's recorded results
(tests/golden/mean_shift_euclidean.npz).  Needs a real MI355X (pytest -m gpu).

Measured on an MI355X: every seeding pick equals the float64 maximum of its step; hill climb max |Z - Z64| 6.3e-8 ... 2.3e-7
against 4.2e-8 ... 1.8e-7 of the reference's direct-difference form in fp32 on the host (test_hill_climb prints the figures per
case; the table is in DESIGN 5p)."""
import numpy as np
import pytest
import torch

import clustering_scene as cs
import ms_euclid_cases as E
from unseenobjectswithmeanshift_amd import synthetic as syn

pytestmark = pytest.mark.gpu

DEV = "cuda"
L2 = "euclidean"
ALL = range(len(E.CASES))


def ops():
    from unseenobjectswithmeanshift_amd import ops as _ops
    return _ops


def ms():
    from unseenobjectswithmeanshift_amd import mean_shift as _ms
    return _ms


_X = {}


def xdev(case):
    if case not in _X:
        _X[case] = E.planted(case)[0].to(DEV)
    return _X[case]


_SEEDS = {}


def gpu_seeds(case):
    """(seeds, indices) of ops.ms_select_seeds(metric="euclidean"), once per case."""
    if case not in _SEEDS:
        _SEEDS[case] = ops().ms_select_seeds(xdev(case), E.CASES[case][3], E.first_index(case), metric=L2)
    return _SEEDS[case]


_CONVERGED = {}


def converged(case):
    """The kernel's seeds after 10 iterations (device), once per case."""
    if case not in _CONVERGED:
        _CONVERGED[case] = ops().ms_hill_climb(xdev(case), gpu_seeds(case)[0], E.KAPPA, E.ITERS, metric=L2)
    return _CONVERGED[case]


# ---- seeding ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.GOLDEN_CASES)
def test_seeding_equals_the_reference(case, golden):
    g = golden("mean_shift_euclidean")
    seeds, idx = gpu_seeds(case)
    assert torch.equal(idx.cpu(), torch.from_numpy(g[f"c{case}_sel"]))
    assert torch.equal(seeds, xdev(case)[idx])


@pytest.mark.parametrize("case", ALL)
def test_seeding_picks_a_maximum(case):
    """Replay in float64 with the kernel's own picks forced: every pick is, to fp32 rounding of 64 non-negative terms and a square
    root (~2e-6 relative), a farthest point of its step."""
    seeds, idx = gpu_seeds(case)
    idx = idx.cpu().numpy()
    assert idx[0] == E.first_index(case) and len(set(idx.tolist())) == len(idx) and idx.min() >= 0
    assert torch.equal(seeds, xdev(case)[torch.from_numpy(idx).to(DEV)])
    r = E.seeding64(E.planted(case)[0], len(idx), int(idx[0]), forced=idx)
    worst = float((r["pick"][1:] / r["top"][1:]).min())
    print(f"case {case}: smallest pick / maximum = 1 - {1 - worst:.2e}")
    assert (r["pick"][1:] >= (1 - 1e-5) * r["top"][1:]).all()


def test_seeding_fewer_rows_than_a_group():
    """n = 15 < the butterfly's 16 rows: the kernel's clamped-row form, one map and two in a batch."""
    X = E.planted(1)[0][:15].contiguous()
    seeds, idx = ops().ms_select_seeds(X.to(DEV), 5, 3, metric=L2)
    want = E.seeding64(X, 5, 3)
    assert float(want["margin"][1:].min()) >= 1e-4                 # the float64 picks are the only legitimate ones
    assert idx.cpu().tolist() == want["idx"].tolist() and torch.equal(seeds.cpu(), X[idx.cpu()])
    both = torch.stack([X, X.flip(0)]).to(DEV)
    _, idx2 = ops().ms_select_seeds_batched(both, 5, [3, 11], metric=L2)
    assert idx2[0].tolist() == want["idx"].tolist() and idx2[1].tolist() == [14 - i for i in want["idx"].tolist()]


def test_seeding_batched_equals_per_map():
    """Three different maps of one n (a golden case and slices of two others) in one call; host and device first indices."""
    n, S = 2000, 20
    maps = [E.planted(0)[0], E.planted(3)[0][:n].contiguous(), E.planted(5)[0][5000:5000 + n].contiguous()]
    first = [E.first_index(0), 11, 1999]
    X = torch.stack(maps).to(DEV)
    seeds, idx = ops().ms_select_seeds_batched(X, S, first, metric=L2)
    for m in range(3):
        s1, i1 = ops().ms_select_seeds(X[m], S, first[m], metric=L2)
        assert torch.equal(idx[m], i1) and torch.equal(seeds[m], s1)
    seeds_d, idx_d = ops().ms_select_seeds_batched(X, S, torch.tensor(first, device=DEV), metric=L2, stepwise=True)
    assert torch.equal(idx_d, idx) and torch.equal(seeds_d, seeds)
    assert torch.equal(idx[0], gpu_seeds(0)[1])


# ---- hill climb ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [2, 10])
@pytest.mark.parametrize("case", ALL)
def test_hill_climb(case, iters):
    """err_gpu <= max(4 x err_cpu32, 5e-7) against the float64 definition; the seeds include one far from every point, whose
    float64 sum of weights is < 0.5 (the clamp(min=1) branch).  4 x: the kernel's expansion ||x||^2 + ||z||^2 - 2 x.z loses
    some accuracy to cancellation (a CPU fp32 expansion form: 0.7-1.9 x of the direct form), times two for the MFMA summation
    order; 5e-7 is two ulps of a coordinate at scale 2."""
    h = E.hill_case(case, iters)
    assert h["far_sum"] < 0.5
    X, Z0 = xdev(case), h["Z0"].to(DEV)
    Z = ops().ms_hill_climb(X, Z0, E.KAPPA, iters, metric=L2)
    err = float((Z.cpu().double() - h["Z64"]).abs().max())
    err_far = float((Z[-1].cpu().double() - h["Z64"][-1]).abs().max())
    print(f"case {case} iters {iters}: err_gpu {err:.3e}  err_cpu32 {h['err32']:.3e}  far seed {err_far:.3e}  "
          f"bound {max(4 * h['err32'], 5e-7):.3e}")
    assert torch.isfinite(Z).all()
    assert err <= max(4 * h["err32"], 5e-7)
    # The far seed's coordinates are ~1e-8 and smaller, far below the bound above, so it gets a relative check of its own: a
    # weight's relative error is kappa x the error of d^2, at most 20 * 2 * 64 * 2^-24 * (|x|^2 + |z|^2) = 6e-4 at scale 2 -> 1e-3.
    # (Dividing by the sum instead of clamp(sum, min=1) would be off by a factor of 1 / sum W > 2.)  Below 1e-30 the weights
    # leave the normal fp32 range (scale 2: e^-80) and only the absolute bound applies.
    far = float(h["Z64"][-1].abs().max())
    if far > 1e-30:
        assert err_far <= 1e-3 * far, (err_far, far)
    assert torch.equal(Z, ops().ms_hill_climb(X, Z0, E.KAPPA, iters, metric=L2))          # two runs, bit for bit
    assert torch.equal(Z0.cpu(), h["Z0"])                                                  # the input is not modified


def test_hill_climb_batched_equals_per_map():
    n = 2000
    maps = [E.planted(0)[0], E.planted(3)[0][:n].contiguous(), E.planted(5)[0][5000:5000 + n].contiguous()]
    X = torch.stack(maps).to(DEV)
    for S, iters in ((21, 3), (130, 2)):                        # two seed blocks | nine: two chunks per iteration
        Z0 = X[:, :: n // S][:, :S].contiguous()
        Z0[:, -1] = E.far_seed(0).to(DEV)
        Z = ops().ms_hill_climb_batched(X, Z0, E.KAPPA, iters, metric=L2)
        for m in range(3):
            assert torch.equal(Z[m], ops().ms_hill_climb(X[m], Z0[m], E.KAPPA, iters, metric=L2))
        assert not torch.equal(Z, Z0)


# ---- connected components --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL)
def test_connected_components(case):
    Z = converged(case)
    labels, num = ops().ms_connected_components(Z, E.EPS, metric=L2)
    want, (alive, created) = E.components64(Z.cpu(), E.EPS)
    assert E.eps_margin(Z.cpu()) >= 1e-4                          # no pair of seeds sits on the threshold
    assert torch.equal(labels.cpu(), want) and num.tolist() == [alive, created]
    assert torch.equal(ms().connected_components(Z, E.EPS, metric=L2), labels)


def test_connected_components_chain():
    Z = E.chain().to(DEV)
    labels, num = ops().ms_connected_components(Z, E.EPS, metric=L2)
    assert labels.tolist() == E.CHAIN_LABELS and num.tolist() == [6, 6]
    both, nums = ops().ms_connected_components_batched(torch.stack([Z, Z.flip(0)]), E.EPS, metric=L2)
    want, (alive, created) = E.components64(E.chain().flip(0), E.EPS)
    assert torch.equal(both[0], labels) and torch.equal(both[1].cpu(), want) and nums[1].tolist() == [alive, created]


# ---- assignment ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL)
def test_assign(case):
    """Every point's label is the label of SOME seed whose float64 d^2 is within 2 * 64 * 2^-24 * (|x|^2 + |z|^2) of the float64
    minimum (the bound on the fp32 dot product's error); no exceptions."""
    X, Z = xdev(case), converged(case)
    S = Z.shape[0]
    seed_labels = torch.arange(S, device=DEV, dtype=torch.int64)               # one label per seed: the argmin itself is visible
    labels, counts = ops().ms_assign(X, Z, seed_labels, S, metric=L2)
    Xc, Zc = X.cpu().double(), Z.cpu().double()
    d2 = E.dist2_64(Xc, Zc)
    bound = 2 * 64 * 2.0 ** -24 * ((Xc * Xc).sum(1)[:, None] + (Zc * Zc).sum(1)[None, :])
    taken = labels.cpu()
    assert int(taken.min()) >= 0 and int(taken.max()) < S
    ok = d2.gather(1, taken[:, None]) <= d2.min(dim=1, keepdim=True).values + bound.gather(1, taken[:, None])
    assert bool(ok.all()), f"{int((~ok).sum())} points took a seed that is not a nearest one"
    assert torch.equal(counts.cpu(), torch.bincount(taken, minlength=S))
    # with the merged labels: the planted clusters, and the histogram of what was written
    merged, num = ops().ms_connected_components(Z, E.EPS, metric=L2)
    lab, cnt = ops().ms_assign(X, Z, merged, S, metric=L2)
    assert torch.equal(cnt.cpu(), torch.bincount(lab.cpu(), minlength=S))
    allowed = d2 <= d2.min(dim=1, keepdim=True).values + bound
    hit = merged.cpu()[None, :] == lab.cpu()[:, None]
    assert bool((allowed & hit).any(dim=1).all())


# ---- end to end ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.GOLDEN_CASES)
def test_smart_init_equals_the_reference(case, golden):
    g = golden("mean_shift_euclidean")
    want = torch.from_numpy(g[f"c{case}_labels"].astype(np.int64))
    X = xdev(case)
    S = E.CASES[case][3]
    labels, sel = ms().mean_shift_smart_init(X, kappa=20, num_seeds=S, max_iters=10, metric=L2, first_index=E.first_index(case))
    assert torch.equal(sel.cpu(), torch.from_numpy(g[f"c{case}_sel"])) and torch.equal(labels.cpu(), want)
    # the public pieces give the same
    seeds, sel2 = ms().select_smart_seeds(X, S, return_selected_indices=True, metric=L2, first_index=E.first_index(case))
    (seeds_only,) = ms().select_smart_seeds(X, S, metric=L2, first_index=E.first_index(case))
    seed_labels, Z = ms().mean_shift_with_seeds(X, seeds, 20, max_iters=10, metric=L2)
    assert torch.equal(sel2, sel) and torch.equal(seeds_only, seeds)
    assert torch.equal(seed_labels.cpu(), torch.from_numpy(g[f"c{case}_seed_labels"]))
    assert float((Z.cpu().double() - torch.from_numpy(g[f"c{case}_Z64"])).abs().max()) <= 5e-7
    W = ms().ball_kernel(seeds, X, 20.0, metric=L2)
    W64 = torch.exp(-20.0 * E.dist2_64(seeds.cpu(), X.cpu()))
    assert float((W.cpu().double() - W64).abs().max()) <= 1e-5 and float(W.max()) <= 1.0


def _feature_maps(case, H, W):
    """Case ``case`` as a (64, H, W) map: n = H * W."""
    return xdev(case).t().reshape(64, H, W).contiguous()


def test_clustering_features_equals_the_reference(golden):
    g = golden("mean_shift_euclidean")
    want = torch.from_numpy(g["c0_labels"].astype(np.int64))
    f0 = _feature_maps(0, 40, 50)
    out, sel = ms().clustering_features(f0[None], num_seeds=20, metric=L2, first_indices=[E.first_index(0)])       # B = 1: the loop
    assert out.dtype == torch.float32 and torch.equal(out[0].long().cpu().reshape(-1), want)
    assert torch.equal(sel[0].cpu(), torch.from_numpy(g["c0_sel"]))
    # B = 3, batched: the golden map between two others of the same size
    other = [E.planted(3)[0][:2000], E.planted(5)[0][7000:9000]]
    feats = torch.stack([other[0].to(DEV).t().reshape(64, 40, 50), f0, other[1].to(DEV).t().reshape(64, 40, 50)]).contiguous()
    first = [5, E.first_index(0), 1234]
    out3, sel3 = ms().clustering_features(feats, num_seeds=20, metric=L2, first_indices=first)
    assert torch.equal(out3[1], out[0]) and torch.equal(sel3[1], sel[0])
    for m in (0, 2):
        o1, s1 = ms().clustering_features(feats[m:m + 1], num_seeds=20, metric=L2, first_indices=first[m:m + 1])
        assert torch.equal(out3[m], o1[0]) and torch.equal(sel3[m], s1[0])
    # case 1 (n = 37) as a 1 x 37 map, twice in a batch
    f1 = xdev(1).t().reshape(1, 64, 1, 37).contiguous()
    out1, sel1 = ms().clustering_features(torch.cat([f1, f1]), num_seeds=5, metric=L2, first_indices=[E.first_index(1)] * 2)
    for m in range(2):
        assert torch.equal(out1[m].long().cpu().reshape(-1), torch.from_numpy(g["c1_labels"].astype(np.int64)))
        assert torch.equal(sel1[m].cpu(), torch.from_numpy(g["c1_sel"]))


def test_smart_init_batched_equals_per_map():
    n, S = 2000, 20
    maps = [E.planted(0)[0], E.planted(3)[0][:n].contiguous(), E.planted(5)[0][5000:5000 + n].contiguous()]
    first = [E.first_index(0), 11, 1999]
    X = torch.stack(maps).to(DEV)
    labels, sel = ms().mean_shift_smart_init_batched(X, kappa=20, num_seeds=S, max_iters=10, first_indices=first, metric=L2)
    for m in range(3):
        l1, s1 = ms().mean_shift_smart_init(X[m], kappa=20, num_seeds=S, max_iters=10, metric=L2, first_index=first[m])
        assert torch.equal(labels[m], l1) and torch.equal(sel[m], s1)
    assert int(sel.min()) >= 0


def test_sample_clustering_euclidean():
    """The planted scene of tests/clustering_scene.py with a network stand-in that returns UN-normalised embeddings (W . image,
    scaled so that two objects are ~1.4 apart and the pixel noise stays within the kernel's reach): the first stage recovers the
    table and the three planted objects."""
    from unseenobjectswithmeanshift_amd import two_stage as ts
    sample, w_net, _, ids = cs.scene()
    sample = {k: v.to(DEV) for k, v in sample.items()}
    wd = (w_net / w_net.norm(dim=0, keepdim=True)).to(DEV) * (1.0 / (2 * 0.4))       # columns of length 1.25: colours differ by 0.8 per channel

    def net(image, label, depth):
        return wd[None, :, 0, None, None] * image[:, 0:1] + wd[None, :, 1, None, None] * image[:, 1:2] + wd[None, :, 2, None, None] * image[:, 2:3]

    feats = net(sample["image_color"], None, None)
    norms = feats.norm(dim=1)
    assert float(norms.max()) < 0.96 and float(norms.max() - norms.min()) > 0.05     # neither unit rows nor of one length
    stages = {}
    out, refined = ts.test_sample_clustering({"image_color": sample["image_color"]}, net, None, num_seeds=20, first_indices=[1000],
                                             stages=stages, metric=L2)
    assert refined is None and out.shape == (1, cs.H, cs.W)
    lab = out[0].long().cpu()
    assert len(torch.unique(lab)) == 4
    for k in range(4):
        region = lab[ids == k]
        assert len(torch.unique(region)) == 1 and cs.iou(lab == region[0], ids == k) == 1.0
    assert int(lab[ids == 0][0]) == 0                              # the table is the largest cluster: label 0
    # the same call through the batch harness
    outb, _, _ = ts.test_batch_clustering([{"image_color": sample["image_color"]}], net, None, num_seeds=20, first_indices=[[1000]],
                                          metric=L2)
    assert torch.equal(outb[0], out[0])


# ---- the cosine entry points are untouched ---------------------------------------------------------------------------------------
def test_cosine_unchanged(golden):
    """A smoke check (the existing suite is the guard): one call each of the four cosine ops on the unit map of
    tests/golden/mean_shift.npz still gives the fixture, and on case 0, normalised, the cosine clustering finds the planted clusters."""
    g = golden("mean_shift")
    Xa, _ = syn.synth_unit_embeddings(4800, 64, clusters=8, sigma=0.15, seed=18)
    Xa = Xa.to(DEV)
    seeds, sel = ops().ms_select_seeds(Xa, 50, int(g["a_first"]))
    assert torch.equal(sel.cpu(), torch.from_numpy(g["a_sel"]))
    Z = ops().ms_hill_climb(Xa, seeds, 20.0, 10)
    seed_labels, num = ops().ms_connected_components(Z, 0.04)
    labels, counts = ops().ms_assign(Xa, Z, seed_labels, 50)
    ops().ms_relabel_largest_zero(labels, counts, num)
    assert torch.equal(labels.cpu(), torch.from_numpy(g["a_labels"]).long())
    Xn = torch.nn.functional.normalize(xdev(0), dim=1).contiguous()
    lab, _ = ms().mean_shift_smart_init(Xn, kappa=20, num_seeds=20, max_iters=10, first_index=E.first_index(0))
    ids = E.planted(0)[1]
    lab = lab.cpu()
    assert len(torch.unique(lab)) == E.CASES[0][1]
    assert all(len(torch.unique(ids[lab == l])) == 1 for l in torch.unique(lab))
