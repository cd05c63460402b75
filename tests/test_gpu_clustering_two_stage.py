"""The UCN two-stage clustering harness on the device (two_stage.test_sample_clustering / test_batch_clustering): the clustering
comes from the HIP kernels, the crops of a whole batch from ONE batched clustering.  Against tests/golden/clustering_two_stage.npz
(the reference's own functions on the planted scene, under the generator's margins), and on the same scene (clustering_scene.py)
at the driver's 100 seeds, where what the harness must return is known from the scene.
Needs a real MI355X (pytest -m gpu)."""
import numpy as np
import pytest
import torch

import clustering_scene as cs

pytestmark = pytest.mark.gpu

DEV = "cuda"
FIRST = [5994, 1688, 31337]          # first stage, then the two crops


def ts():
    from unseenobjectswithmeanshift_amd import two_stage
    return two_stage


def on_device(sample):
    return {k: v.to(DEV) for k, v in sample.items()}


_RUN = {}


def run():
    """The frame and its mirror image through test_sample_clustering, once."""
    if not _RUN:
        sample, w_net, w_crop, ids = cs.scene()
        nets = (cs.network_from(w_net.to(DEV)), cs.network_from(w_crop.to(DEV)))
        first_m = [cs.mirror_index(FIRST[0], cs.W)] + [cs.mirror_index(i, 224) for i in FIRST[1:]]
        plain, mirrored = on_device(sample), on_device(cs.flipped(sample))
        stages = {}
        _RUN.update(sample=plain, mirrored=mirrored, nets=nets, ids=ids.to(DEV), first_m=first_m, stages=stages,
                    single=ts().test_sample_clustering(plain, *nets, first_indices=FIRST, stages=stages),
                    single_m=ts().test_sample_clustering(mirrored, *nets, first_indices=first_m))
    return _RUN


def test_sample_clustering_recovers_the_planted_scene():
    r = run()
    ids, (out_label, refined), stages = r["ids"], r["single"], r["stages"]
    raw = stages["label"][0].long()
    assert raw.unique().numel() == 4 and not bool(raw[ids == 0].any())
    for k in (1, 2, 3):
        assert raw[ids == k].unique().numel() == 1 and int(raw[ids == k][0]) != 0
    assert torch.equal(out_label[0] != 0, (ids == 1) | (ids == 2))                    # the depth filter removes object 3 only
    assert int(stages["selected"][0][0]) == FIRST[0] and [int(s[0]) for s in stages["selected_crop"]] == FIRST[1:]
    assert len(stages["rois"]) == 2
    for lc in stages["labels_crop"]:
        assert float(lc.min()) == -1.0 and float((lc == -1).float().mean()) > 0.4 and float((lc > -1).float().mean()) > 0.3
    ref = refined[0]
    assert set(ref.unique().tolist()) == {0.0, 1.0, 2.0} and not bool(ref[ids == 3].any())
    z = r["sample"]["depth"][0, 2]
    far, near = sorted((1, 2), key=lambda k: -float(z[ids == k].mean()))
    for k, number in ((far, 1.0), (near, 2.0)):                                      # pasted far to near (TD:130-136)
        assert float(ref[ids == k].mode().values) == number and cs.iou(ref == number, ids == k) > 0.9


def test_batch_equals_per_frame_bitwise():
    """Four copies of the frame, frames 1 and 3 mirrored left-right: every frame's results are those of test_sample_clustering on
    that frame alone -- nothing leaks from a neighbour -- and all 8 crops go through one clustering call."""
    from unseenobjectswithmeanshift_amd import mean_shift
    r = run()
    calls = []

    def cluster(features, **kw):
        calls.append(features.shape[0])
        return mean_shift.clustering_features(features, **kw)

    samples = [r["sample"], r["mirrored"], r["sample"], r["mirrored"]]
    firsts = [FIRST, r["first_m"], FIRST, r["first_m"]]
    stages = {}
    out, ref, rows = ts().test_batch_clustering(samples, *r["nets"], first_indices=firsts, cluster=cluster, crop_batch=3, stages=stages)
    assert calls == [4, 8] and [row[0] for row in rows] == [0, 0, 1, 1, 2, 2, 3, 3]
    for f in range(4):
        want = r["single_m"] if f % 2 else r["single"]
        assert torch.equal(out[f], want[0][0]) and torch.equal(ref[f], want[1][0])
    for n in range(8):
        assert int(stages["selected_crop"][n][0]) == firsts[n // 2][1 + n % 2]
    # the default clustering is the same callable
    out_d, ref_d, _ = ts().test_batch_clustering(samples[:2], *r["nets"], first_indices=firsts[:2])
    assert torch.equal(out_d, out[:2]) and torch.equal(ref_d, ref[:2])


def test_mirrored_frames_give_mirrored_first_stage_labels():
    """The first-stage label image of the mirrored frame is the mirror image of the frame's (same clusters, created in the same
    order: the first four seeds fall into the four planted regions).  The refined image keeps the objects and their numbers, but its
    outlines come back from the 224 x 224 crops by nearest sampling, src = floor(dst * 224 / size), which is not mirror symmetric:
    a mirrored outline may land one pixel to the side.  Only outline pixels of the two pasted objects can differ -- at most one per
    row and side and one per column and side, i.e. no more than the two objects' perimeters."""
    r = run()
    assert torch.equal(torch.flip(r["single_m"][0], dims=[-1]), r["single"][0])
    plain, back = r["single"][1][0], torch.flip(r["single_m"][1][0], dims=[-1])
    ids = r["ids"]
    for k in (1, 2):
        assert float(back[ids == k].mode().values) == float(plain[ids == k].mode().values)
    differ = plain != back
    perimeter = 0
    for k in (1, 2):
        m = torch.nn.functional.pad((ids == k).float(), (1, 1, 1, 1)) > 0
        inner = m[1:-1, 1:-1] & m[:-2, 1:-1] & m[2:, 1:-1] & m[1:-1, :-2] & m[1:-1, 2:]
        outline = m[1:-1, 1:-1] & ~inner
        perimeter += int(outline.sum())
        # a differing pixel lies on an outline: in the object's one-pixel band inside or outside
        grown = torch.nn.functional.max_pool2d(outline[None, None].float(), 3, 1, 1)[0, 0] > 0
        differ = differ & ~grown
    assert not bool(differ.any())                                         # nothing differs away from the outlines
    assert int((plain != back).sum()) <= perimeter


def test_random_first_indices_follow_numpy():
    """first_indices=None: np.random.randint draws -- the F first-stage indices, then one per crop in (frame, label) order."""
    r = run()
    np.random.seed(3)
    want = [np.random.randint(0, cs.H * cs.W) for _ in range(2)] + [np.random.randint(0, 224 * 224) for _ in range(4)]
    stages = {}
    np.random.seed(3)
    ts().test_batch_clustering([r["sample"], r["mirrored"]], *r["nets"], stages=stages)
    assert [int(s[0]) for s in stages["selected"]] + [int(s[0]) for s in stages["selected_crop"]] == want


def test_frame_with_every_label_filtered():
    r = run()
    blind = dict(r["sample"], depth=torch.zeros_like(r["sample"]["depth"]))
    out, ref, rows = ts().test_batch_clustering([blind], *r["nets"], first_indices=[FIRST])
    assert rows == [] and not bool(out.any()) and ref.shape == out.shape and not bool(ref.any())
    # next to a frame that keeps its objects: zero rows for the blind frame, a zero refined image, the neighbour untouched
    out, ref, rows = ts().test_batch_clustering([blind, r["sample"]], *r["nets"], first_indices=[FIRST, FIRST])
    assert [row[0] for row in rows] == [1, 1] and not bool(out[0].any()) and not bool(ref[0].any())
    assert torch.equal(out[1], r["single"][0][0]) and torch.equal(ref[1], r["single"][1][0])


# ---- against the reference's functions (tests/golden/clustering_two_stage.npz) ----
def test_against_the_reference(golden):
    from test_clustering_two_stage_cpu import check_against_fixture, fixture_sample
    g = golden("clustering_two_stage")
    sample = on_device(fixture_sample(g))
    nets = (cs.network_from(torch.from_numpy(g["w_net"]).to(DEV)), cs.network_from(torch.from_numpy(g["w_crop"]).to(DEV)))
    S, first = int(g["num_seeds"]), g["first_indices"].tolist()
    stages = {}
    out_label, refined = ts().test_sample_clustering(sample, *nets, num_seeds=S, first_indices=first, stages=stages)
    check_against_fixture(g, out_label, refined, stages)
    # the batch form: the fixture frame four times with the recorded indices
    bst = {}
    out, ref, rows = ts().test_batch_clustering([sample] * 4, *nets, num_seeds=S, first_indices=[first] * 4, stages=bst)
    assert [row[0] for row in rows] == [0, 0, 1, 1, 2, 2, 3, 3]
    for f in range(4):
        per_frame = dict(label=bst["label"][f:f + 1], selected=bst["selected"][f:f + 1], selected_crop=bst["selected_crop"][2 * f:2 * f + 2],
                         rois=torch.tensor([row[2:6] for row in rows[2 * f:2 * f + 2]]), labels_crop=bst["labels_crop"][2 * f:2 * f + 2])
        check_against_fixture(g, out[f:f + 1], ref[f:f + 1], per_frame)
        assert torch.equal(out[f], out_label[0]) and torch.equal(ref[f], refined[0])
    # frames 1 and 3 mirrored: frames 0 and 2 still give the fixture, the mirrored frames the mirrored first-stage labels
    mirrored = {k: torch.flip(v, dims=[-1]).contiguous() for k, v in sample.items()}
    first_m = [cs.mirror_index(first[0], cs.W)] + [cs.mirror_index(i, 224) for i in first[1:]]
    out2, ref2, _ = ts().test_batch_clustering([sample, mirrored, sample, mirrored], *nets, num_seeds=S,
                                               first_indices=[first, first_m, first, first_m])
    for f in (0, 2):
        assert torch.equal(out2[f], out_label[0]) and torch.equal(ref2[f], refined[0])
    tie = torch.from_numpy(g["near_tie_label"]).to(DEV)
    for f in (1, 3):
        assert torch.equal(torch.flip(out2[f], dims=[-1])[~tie], out_label[0][~tie])
