"""Segmentation metrics on the host (unseenobjectswithmeanshift_amd.evaluation, CPU path): the reference's multilabel_metrics
(lib/utils/evaluation.py:109-258) pinned by tests/golden/multilabel_metrics.npz (make_golden_eval.py), bit for bit."""
import numpy as np
import pytest
import torch

from unseenobjectswithmeanshift_amd import evaluation as ev
from unseenobjectswithmeanshift_amd import synthetic as syn
from unseenobjectswithmeanshift_amd import two_stage as ts
from unseenobjectswithmeanshift_amd.meta_arch import Instances

G = np.load(__import__("os").path.join(__import__("os").path.dirname(__file__), "golden", "multilabel_metrics.npz"))
NAMES = [str(n) for n in G["names"]]


def case(name):
    H, W, seed = (int(v) for v in G[f"{name}_recipe"])
    gv, pv = [int(v) for v in G[f"{name}_gt_values"]], [int(v) for v in G[f"{name}_pred_values"]]
    return syn.synth_label_pair(H, W, seed, str(G[f"{name}_kind"]), gt_values=gv, pred_values=pv or None, n_gt=len(gv),
                                n_pred=len(pv) if pv else len(gv))


def same(a, b):
    """== or both nan, value by value"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def as_vec(m):
    assert tuple(m.keys()) == ev.KEYS
    return np.array([float(m[k]) for k in ev.KEYS])


def test_fixture_covers_the_cases():
    assert ev.bound_radius(224, 224) == 1 and ev.bound_radius(480, 640) == 3 and ev.bound_radius(960, 1280) == 5
    assert any(G[f"{n}_labels_gt"].size > 64 for n in NAMES)
    assert any(1023 in G[f"{n}_labels_gt"] and 1023 in G[f"{n}_labels_pred"] for n in NAMES)
    assert sum(np.isnan(G[f"{n}_metrics"]).any() for n in NAMES) >= 2


@pytest.mark.parametrize("name", NAMES)
def test_host_metrics_equal_the_reference_bit_for_bit(name):
    pred, gt = case(name)
    got = ev.multilabel_metrics(pred, gt)
    assert same(as_vec(got), G[f"{name}_metrics"]), (got, G[f"{name}_metrics"])
    # tensors on the CPU take the same path
    assert same(as_vec(ev.multilabel_metrics(torch.from_numpy(pred), torch.from_numpy(gt)[None])), G[f"{name}_metrics"])


@pytest.mark.parametrize("name", [n for n in NAMES if f"{n}_tp" in G])
def test_host_counts_equal_the_reference(name):
    pred, gt = case(name)
    c = ev.host_counts(pred, gt)
    for k in ("labels_gt", "labels_pred", "tp", "fgm", "gtm", "bnd_gt", "bnd_pred"):
        assert np.array_equal(c[k], G[f"{name}_{k}"]), k


@pytest.mark.parametrize("name", [n for n in NAMES if f"{n}_cost" in G])
def test_assignment_equals_the_reference_including_ties(name):
    got = ev.munkres_assignment(G[f"{name}_cost"])
    assert got == [tuple(a) for a in G[f"{name}_assign"].tolist()]


def test_assignment_ties_resolve_as_the_reference():
    """the tie cases of the fixture: two assignments of equal cost, and the reference's choice is the one returned"""
    for name in ("ties_odd", "ties_480"):
        C = G[f"{name}_cost"]
        assert C[0, 0] == C[1, 0] and C[0, 1] == C[1, 1]
        assert ev.munkres_assignment(C) == [tuple(a) for a in G[f"{name}_assign"].tolist()] == [(0, 0), (1, 1)]


def test_assignment_is_optimal_on_random_matrices():
    from itertools import permutations
    rng = np.random.default_rng(0)
    for shape in [(3, 3), (4, 2), (2, 5), (5, 5)]:
        C = np.round(rng.random(shape), 1)                 # many ties
        n = min(shape)
        got = ev.munkres_assignment(C)
        assert len(got) == n and len({i for i, _ in got}) == n and len({j for _, j in got}) == n
        best = min(sum(C[i, j] if C.shape[0] <= C.shape[1] else C[j, i] for i, j in enumerate(p))
                   for p in permutations(range(max(shape)), n))
        assert abs(sum(C[a] for a in got) - best) < 1e-12


def test_average_metrics():
    ms = [dict(zip(ev.KEYS, G[f"{n}_metrics"].tolist())) for n in ("blobs_224", "blobs_odd", "edges_odd")]
    avg = ev.average_metrics(ms)
    assert list(avg.keys()) == list(ev.KEYS)
    for k in ev.KEYS:
        assert avg[k] == ((0 + ms[0][k]) + ms[1][k] + ms[2][k]) / 3
    assert ev.average_metrics([]) == {}


@pytest.mark.parametrize("bad", [-1.0, 1024.0, 2.5, float("nan")])
def test_bad_label_values_raise(bad):
    pred, gt = case("blobs_odd")
    p = pred.copy()
    p[3, 4] = bad
    with pytest.raises(ValueError, match="integers in"):
        ev.multilabel_metrics(p, gt)
    with pytest.raises(ValueError, match="integers in"):
        ev.multilabel_metrics(pred, p)


class _Pred:
    """deterministic stand-in for the network (first and second stage): blobs derived from the image content"""

    def __call__(self, sample):
        img = sample["image"]
        H, W = img.shape[-2:]
        g = torch.Generator().manual_seed(int(float(img.sum()) * 1000) % 100003)
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        masks = torch.zeros(5, H, W)
        for i in range(5):
            cy, cx = torch.rand(1, generator=g).item() * H, torch.rand(1, generator=g).item() * W
            masks[i] = (((yy - cy) / (H / 6)) ** 2 + ((xx - cx) / (W / 6)) ** 2 <= 1).float()
        return {"instances": Instances((H, W), pred_masks=masks, scores=torch.rand(5, generator=g) * 0.6 + 0.35,
                                       pred_classes=torch.ones(5, dtype=torch.long))}

    def batch_call(self, samples):
        return [self(s) for s in samples]


def test_labelled_harness_scores_its_own_label_images():
    """two_stage.test_sample / test_sample_crop / test_dataset(_crop) on the host: the dicts are multilabel_metrics of the
    pipeline's own label images -- the first stage before the depth filter, the refined image (or the filtered first stage)."""
    g = torch.Generator().manual_seed(4)
    H, W = 96, 128
    data = []
    for f in range(3):
        z = 0.4 + torch.rand(1, H, W, generator=g)
        z[:, : H // 3] = 0                                          # the depth filter drops some objects
        gt = torch.from_numpy(syn.synth_label_pair(H, W, 40 + f, "blobs", n_gt=4, n_pred=4)[1])
        data.append({"image_color": torch.rand(3, H, W, generator=g), "depth": torch.cat([torch.rand(2, H, W, generator=g), z]),
                     ("label" if f != 1 else "labels"): gt[None]})
    kw = dict(topk=False, confident_score=0.5)
    pred = _Pred()
    for smp in data:
        gt = ts._sample_gt(smp)
        label, out_label, refined, _, _ = ts._sample_crop(smp, pred, pred, use_depth=True, low_threshold=0.4, num_class=2,
                                                          use_nms=False, depth_threshold=0.5, **kw)
        m, mr = ts.test_sample_crop(smp, pred, pred, **kw)
        assert same(as_vec(m), as_vec(ev.multilabel_metrics(label.numpy(), gt.numpy())))
        ref2 = (refined if refined is not None else out_label)[0]
        assert same(as_vec(mr), as_vec(ev.multilabel_metrics(ref2.numpy(), gt.numpy())))
        m0, mr0 = ts.test_sample_crop(smp, pred, None, **kw)                 # no second stage: the filtered first stage
        assert same(as_vec(m0), as_vec(m)) and same(as_vec(mr0), as_vec(ev.multilabel_metrics(out_label[0].numpy(), gt.numpy())))
        assert same(as_vec(ts.test_sample(smp, pred, **kw)), as_vec(m))
    avg, avg_r = ts.test_dataset_crop(data, pred, pred, **kw)
    pairs = [ts.test_sample_crop(s, pred, pred, **kw) for s in data]
    assert same(as_vec(avg), as_vec(ev.average_metrics([p[0] for p in pairs])))
    assert same(as_vec(avg_r), as_vec(ev.average_metrics([p[1] for p in pairs])))
    assert same(as_vec(ts.test_dataset(data, pred, **kw)), as_vec(ev.average_metrics([ts.test_sample(s, pred, **kw) for s in data])))
