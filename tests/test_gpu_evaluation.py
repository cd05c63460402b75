"""Segmentation metrics on the GPU: msm_eval_counts (csrc/eval_metrics.hip) against the reference's counts of
tests/golden/multilabel_metrics.npz, the batched metrics against the host path bit for bit, and the labelled harness."""
import os

import numpy as np
import pytest
import torch

from unseenobjectswithmeanshift_amd import evaluation as ev
from unseenobjectswithmeanshift_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "multilabel_metrics.npz"))
NAMES = [str(n) for n in G["names"]]


def case(name):
    H, W, seed = (int(v) for v in G[f"{name}_recipe"])
    gv, pv = [int(v) for v in G[f"{name}_gt_values"]], [int(v) for v in G[f"{name}_pred_values"]]
    return syn.synth_label_pair(H, W, seed, str(G[f"{name}_kind"]), gt_values=gv, pred_values=pv or None, n_gt=len(gv),
                                n_pred=len(pv) if pv else len(gv))


def same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def vec(m):
    assert tuple(m.keys()) == ev.KEYS
    return np.array([float(m[k]) for k in ev.KEYS])


@pytest.mark.parametrize("name", NAMES)
def test_device_counts_equal_the_reference(name):
    """every count of the fixture, exactly: > 64 labels on a side (chunk pairs), r = 1 / 3 / 5, odd sizes, edges, 1023"""
    pred, gt = case(name)
    c = ev.device_counts(torch.from_numpy(pred)[None].to(DEV), torch.from_numpy(gt)[None].to(DEV))[0]
    h = ev.host_counts(pred, gt)
    for k in h:
        assert np.array_equal(np.asarray(c[k]), np.asarray(h[k])), k
    if f"{name}_tp" in G:
        for k in ("labels_gt", "labels_pred", "tp", "fgm", "gtm", "bnd_gt", "bnd_pred"):
            assert np.array_equal(c[k], G[f"{name}_{k}"]), k
    assert same(vec(ev.multilabel_metrics(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV))), G[f"{name}_metrics"])


def test_device_counts_at_every_table_capacity():
    """the same counts whatever the label capacity L of the table (one pass at L <= 64, chunk pairs above), and the header"""
    from unseenobjectswithmeanshift_amd import ops
    pred, gt = case("grid_many_gt")
    p, g = torch.from_numpy(pred)[None].to(DEV), torch.from_numpy(gt)[None].to(DEV)
    ref = ev.host_counts(pred, gt)
    for L in (80, 128, 200):
        row = ops.eval_counts(p, g, ev.bound_radius(*pred.shape), L).cpu().numpy()[0]
        assert row[0] == 80 and row[1] == ref["labels_pred"].size and row[2] == row[3] == 0
        assert row[4] == int((gt != 0).sum()) and row[5] == int((pred != 0).sum())
        c = ev._decode_counts(row, L)
        for k in ref:
            assert np.array_equal(np.asarray(c[k]), np.asarray(ref[k])), (L, k)
    row = ops.eval_counts(p, g, ev.bound_radius(*pred.shape), 64).cpu().numpy()[0]      # too small: the header says so
    assert row[0] == 80
    bad = p.clone()
    bad[0, 0, :3] = torch.tensor([-1.0, 1024.0, 2.5])
    row = ops.eval_counts(bad, g, 1, 64).cpu().numpy()[0]
    assert row[3] == 3 and row[2] == 0
    with pytest.raises(ValueError, match="integers in"):
        ev.multilabel_metrics(bad[0], g[0])


def test_batched_metrics_equal_the_host_path():
    """multilabel_metrics_batched on 16 frames of 480x640 (about ten labels a side) == the host path frame by frame"""
    preds, gts = [], []
    for f in range(16):
        p, g = syn.synth_label_pair(480, 640, 100 + f, "blobs", n_gt=10, n_pred=9 + f % 3)
        preds.append(p)
        gts.append(g)
    preds[5], gts[5] = syn.synth_label_pair(480, 640, 7, "full_gt", gt_values=[5], n_gt=1, n_pred=4)
    preds[6][:] = 0
    got = ev.multilabel_metrics_batched(torch.from_numpy(np.stack(preds)).to(DEV), torch.from_numpy(np.stack(gts)).to(DEV))
    assert len(got) == 16
    for f in range(16):
        assert same(vec(got[f]), vec(ev.multilabel_metrics(preds[f], gts[f]))), f


def _model_and_predictor():
    from unseenobjectswithmeanshift_amd.meta_arch import Instances, MeanShiftMaskFormer, build_resnet50_head
    head = build_resnet50_head(num_queries=100, dec_layers=3)
    head.pixel_decoder.load_state_dict(syn.synth_state_dict(syn.pixel_decoder_param_shapes()), strict=True)
    head.predictor.load_state_dict(syn.synth_state_dict(syn.decoder_param_shapes(dec_layers=3)), strict=True)
    model = MeanShiftMaskFormer(backbone=syn.StandInBackbone().to(DEV).eval(), sem_seg_head=head.to(DEV).eval(), num_queries=100)

    class Pred:
        def batch_tensors(self, samples):
            imgs = torch.stack([x["image"] for x in samples])
            inputs = {"image": imgs}
            if samples[0].get("depth") is not None:
                inputs["depth"] = torch.stack([x["depth"] for x in samples])
            with torch.no_grad():
                return model.inference_images(inputs, tuple(int(v) for v in imgs.shape[-2:]))[:3]

        def batch_call(self, samples):
            s, c, m = self.batch_tensors(samples)
            return [{"instances": Instances(tuple(m.shape[-2:]), pred_masks=m[b], scores=s[b], pred_classes=c[b])} for b in range(len(samples))]

        def __call__(self, sample):
            return self.batch_call([sample])[0]

    return model, Pred()


def _samples(n, H, W, seed):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for f in range(n):
        gt = torch.from_numpy(syn.synth_label_pair(H, W, seed * 10 + f, "blobs", n_gt=6, n_pred=6)[1])
        out.append({"image_color": torch.rand(3, H, W, generator=gen).to(DEV), "depth": torch.rand(3, H, W, generator=gen).to(DEV),
                    "label": gt[None]})
    return out


def test_labelled_harness_on_a_random_init_model():
    """test_sample_crop and test_batch_crop score their own label images: each dict equals host multilabel_metrics of the
    image it scores, and the batched form equals test_sample_crop frame by frame"""
    from unseenobjectswithmeanshift_amd import two_stage as ts
    _, pred = _model_and_predictor()
    H, W = 192, 256
    samples = _samples(3, H, W, 6)
    kw = dict(topk=False, confident_score=0.3)
    bm, bmr = ts.test_batch_crop(samples, pred, pred, use_depth=True, **kw)
    for f, smp in enumerate(samples):
        gt = smp["label"][0].numpy()
        label, out_label, refined, _, _ = ts._sample_crop(smp, pred, pred, use_depth=True, low_threshold=0.4, num_class=2, use_nms=False,
                                                          depth_threshold=0.5, **kw)
        m, mr = ts.test_sample_crop(smp, pred, pred, use_depth=True, **kw)
        assert same(vec(m), vec(ev.multilabel_metrics(label.cpu().numpy(), gt)))
        assert same(vec(mr), vec(ev.multilabel_metrics((refined if refined is not None else out_label)[0].cpu().numpy(), gt)))
        assert same(vec(bm[f]), vec(m)) and same(vec(bmr[f]), vec(mr)), f


def test_metrics_accumulator_with_the_pipeline():
    """MetricsAccumulator as BatchedTwoStage.run's consume callback over three batches == the mean of the per-frame host metrics
    of the label images the pipeline handed over"""
    from unseenobjectswithmeanshift_amd import two_stage as ts
    model, _ = _model_and_predictor()
    H, W = 192, 256
    batches = [_samples(3, H, W, 20 + i) for i in range(3)]
    gts = [torch.stack([s["label"][0] for s in b]).to(DEV) for b in batches]
    pipe = ts.BatchedTwoStage(model, 3, (H, W), topk=False, confident_score=0.3)
    acc = ev.MetricsAccumulator(gts, pipe, max_labels=128)
    seen = []

    def consume(i, out_label, refined, rows):
        cropped = {r[0] for r in rows}
        seen.append((i, out_label.clone(), torch.stack([refined[f] if f in cropped else out_label[f] for f in range(3)])))
        acc(i, out_label, refined, rows)

    pipe.run(batches, consume=consume)
    first, second = [], []
    for i, lab, ref in seen:
        for f in range(3):
            gt = gts[i][f].cpu().numpy()
            first.append(ev.multilabel_metrics(lab[f].cpu().numpy(), gt))
            second.append(ev.multilabel_metrics(ref[f].cpu().numpy(), gt))
    per_frame = acc.frames()
    assert len(per_frame) == 9
    for k, (_, _, a, b) in enumerate(per_frame):
        assert same(vec(a), vec(first[k])) and same(vec(b), vec(second[k]))
    m1, m2 = acc.result()
    assert same(vec(m1), vec(ev.average_metrics(first))) and same(vec(m2), vec(ev.average_metrics(second)))
