"""Two-stage (zoom-in refinement) harness around the predictor.

Own counterpart of the reference's host-side harness, same function names / argument meaning /
return values:

  filter_labels_depth       <- lib/fcn/test_dataset.py:183-198
  crop_rois                 <- lib/fcn/test_dataset.py:62-112
  match_label_crop          <- lib/fcn/test_dataset.py:116-179
  nms                       <- lib/fcn/nms.py:3-23
  combine_masks_with_NMS    <- lib/fcn/test_utils.py:55-91
  test_sample_crop_nolabel  <- lib/fcn/test_utils.py:339-421
  test_sample               <- lib/fcn/test_utils.py:169-205   (labelled: scored with evaluation.multilabel_metrics)
  test_sample_crop          <- lib/fcn/test_utils.py:245-336
  test_dataset(_crop)       <- lib/fcn/test_utils.py:424-513   (the printed means, returned)
  test_batch_crop           the labelled form of test_batch_crop_nolabel (one metrics call per batch)
  combine_masks_with_NMS_batched  nms + combine_masks_with_NMS for a batch of images without compaction or host round trip
  test_sample_clustering    <- lib/fcn/test_dataset.py:232-267  (the UCN method: embedding network -> mean-shift clustering, both stages)
  test_batch_clustering     the same for a batch of frames: every second-stage map of the batch clustered in one batched call

These are data-dependent, tiny (<= 20 instances) bookkeeping steps; they run as torch ops on
whatever device the label maps live on (GPU in production, CPU in the unit tests), never through
the oracle.  Differences from the reference, on purpose:
  * the second stage is BATCHED: all crops of an image go through the crop predictor in one call
    (the reference loops batch-1, test_utils.py:396-405);
  * test_sample_crop_nolabel returns (out_label, out_label_refined, out_score, bbox) with None for
    the last two when NMS is off -- the reference raises NameError there (test_utils.py:376,421);
  * test_sample / test_sample_crop read the ground truth from sample["label"], else sample["labels"] -- the reference's
    test_sample_crop tests "label" twice (test_utils.py:252-255), so a sample with "labels" only has no ground truth there
    and multilabel_metrics fails on it;
  * the labelled functions return the metrics (and test_dataset / test_dataset_crop the means) instead of printing them;
  * combine_masks_with_NMS_batched (the batched pipelines with use_nms=True) drops a candidate whose mask is EMPTY before NMS --
    the reference raises on min() of an empty array there (test_utils.py:85-88), and a pipeline captured in a HIP graph cannot
    raise; it also fixes what numpy's default argsort leaves open: equal scores are visited higher index first, equal areas are
    numbered in the order they were kept.
"""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

from .meta_arch import combine_masks_tensor, combine_masks, get_confident_instances

CROP_SIZE = 224          # cfg.TRAIN.SYN_CROP_SIZE, lib/fcn/config.py:130
PADDING_PERCENTAGE = 0.25


LABEL_BINS = 1024      # label images hold 0 and 2..N+1 with N <= detections per image (<= the number of queries)


def mask_to_tight_box(mask):
    """lib/utils/mask.py:179-186: (x_min, y_min, x_max, y_max) of the non-zero pixels."""
    ys, xs = torch.nonzero(mask, as_tuple=True)
    return xs.min(), ys.min(), xs.max(), ys.max()


def label_stats(labels, weight=None):
    """Per-label statistics of integer-valued label images labels (B,H,W) with values in [0, LABEL_BINS):
    (stats (B,k,5) = area, x_min, y_min, x_max, y_max [W, H, -1, -1 when absent]; wsum (B,k) = sum of `weight` over the
    label's pixels; overflow (B,) = number of out-of-range pixels).  One pass replaces the reference's per-label
    unique()/masked reductions (test_dataset.py:62-131, 183-198).  GPU tensors go through the HIP kernel
    (msm_label_stats); CPU tensors -- the host-logic unit tests -- through the same definition in torch ops."""
    k = int(LABEL_BINS)
    B, H, W = labels.shape
    if labels.is_cuda:
        from . import ops
        return ops.label_stats(labels.float().contiguous(), None if weight is None else weight.float().contiguous(), k)
    lab = labels.reshape(B, -1).float()
    idx = lab.to(torch.int64).clamp(0, k - 1)
    overflow = (~(lab >= 0) | (lab.to(torch.int64) >= k)).sum(1).to(torch.int32)
    ys = torch.arange(H).repeat_interleave(W).expand(B, -1)
    xs = torch.arange(W).repeat(H).expand(B, -1)
    area = torch.zeros((B, k), dtype=torch.int64).scatter_add(1, idx, torch.ones_like(idx))
    stats = torch.stack([area,
                         torch.full((B, k), W).scatter_reduce(1, idx, xs, "amin"),
                         torch.full((B, k), H).scatter_reduce(1, idx, ys, "amin"),
                         torch.full((B, k), -1).scatter_reduce(1, idx, xs, "amax"),
                         torch.full((B, k), -1).scatter_reduce(1, idx, ys, "amax")], 2).to(torch.int32)
    wsum = torch.zeros((B, k), dtype=torch.float32)
    if weight is not None:
        wsum.scatter_add_(1, idx, weight.reshape(B, -1).float())
    return stats, wsum, overflow


def filter_labels_depth(labels, depth, threshold):
    """Zero every label whose pixels have valid depth (z > 0) on less than `threshold` of their area.
    labels (B,H,W) with small non-negative integer values, depth (B,3,H,W) xyz.  (lib/fcn/test_dataset.py:183-198; the
    per-label loop of the reference is one statistics pass here: same integer counts, same fp32 division, no host
    syncs.)"""
    stats, good, _ = label_stats(labels, (depth[:, 2] > 0).float())
    area = stats[:, :, 0]
    bad = (good / area.float().clamp_min(1.0) < threshold) & (area > 0)
    bad[:, 0] = False
    idx = labels.reshape(labels.shape[0], -1).to(torch.int64).clamp(0, int(LABEL_BINS) - 1)
    return labels.masked_fill(torch.gather(bad, 1, idx).view_as(labels), 0)


def _label_boxes(label_img):
    """Labels present in an (H,W) label image (0 = background) and their tight boxes, in ascending label order:
    [(label, x_min, y_min, x_max, y_max), ...] -- one statistics pass and ONE device -> host transfer instead of a
    nonzero() + four .item() round trips per label (lib/utils/mask.py:179-186)."""
    stats, _, overflow = label_stats(label_img[None])
    t = torch.cat([stats[0].reshape(-1), overflow]).cpu().numpy()
    if t[-1] != 0:
        raise ValueError(f"label image values must be integers in [0, {LABEL_BINS}) ({t[-1]} pixels are not)")
    t = t[:-1].reshape(-1, 5)
    return [(int(v), int(t[v, 1]), int(t[v, 2]), int(t[v, 3]), int(t[v, 4])) for v in np.nonzero(t[:, 0])[0] if v != 0]


def crop_rois(rgb, initial_masks, depth, crop_size=CROP_SIZE):
    """One padded ROI per label of initial_masks[0], resized to crop_size (bilinear with
    align_corners=True -- F.upsample_bilinear -- for rgb/depth, nearest for the mask).
    Returns (rgb_crops (N,3,S,S), mask_crops (N,S,S), rois (N,4) x0,y0,x1,y1 inclusive, depth_crops)."""
    _, H, W = initial_masks.shape
    dev = rgb.device
    boxes = _label_boxes(initial_masks[0])
    n = len(boxes)
    size = (crop_size, crop_size)
    rois_host, table = [], []
    for mask_id, x0, y0, x1, y1 in boxes:
        # round(): half to even, as the reference's torch.round on the exact product (test_dataset.py:83-84)
        xp, yp = int(round((x1 - x0) * PADDING_PERCENTAGE)), int(round((y1 - y0) * PADDING_PERCENTAGE))
        x0, x1 = max(x0 - xp, 0), min(x1 + xp, W - 1)
        y0, y1 = max(y0 - yp, 0), min(y1 + yp, H - 1)
        rois_host.append([x0, y0, x1, y1])
        table.append([0, int(mask_id), x0, y0, x1, y1, 0, 0])
    rois = torch.tensor(rois_host, dtype=torch.float32).reshape(n, 4).to(dev)
    if rgb.is_cuda and n > 0:
        # device tensors: every crop of the frame in ONE launch of the kernel the batched pipeline uses (msm_crop_resize: bilinear
        # align_corners=True for rgb / depth, nearest for the mask, ATen's index arithmetic -- tests pin it to the loop below)
        from . import ops
        tab = torch.tensor(table, dtype=torch.int32, device=dev)
        rgb_crops, mask_crops, depth_crops = ops.crop_resize(rgb[0:1].float().contiguous(), None if depth is None else depth[0:1].float().contiguous(),
                                                             initial_masks[0:1].float().contiguous(), tab, crop_size)
        return rgb_crops, mask_crops, rois, depth_crops
    # host tensors (unit tests of the harness logic without a GPU): the reference's per-ROI loop
    rgb_crops = torch.zeros((n, 3, crop_size, crop_size), device=dev)
    mask_crops = torch.zeros((n, crop_size, crop_size), device=dev)
    depth_crops = torch.zeros((n, 3, crop_size, crop_size), device=dev) if depth is not None else None
    for k, (mask_id, x0, y0, x1, y1) in enumerate([(t[1], *t[2:6]) for t in table]):
        mask = (initial_masks[0, y0:y1 + 1, x0:x1 + 1] == mask_id).float()
        rgb_crops[k] = F.interpolate(rgb[0:1, :, y0:y1 + 1, x0:x1 + 1], size=size, mode="bilinear", align_corners=True)[0]
        mask_crops[k] = F.interpolate(mask[None, None], size=size, mode="nearest")[0, 0]
        if depth is not None:
            depth_crops[k] = F.interpolate(depth[0:1, :, y0:y1 + 1, x0:x1 + 1], size=size, mode="bilinear",
                                           align_corners=True)[0]
    return rgb_crops, mask_crops, rois, depth_crops


def match_label_crop(initial_masks, labels_crop, out_label_crop, rois, depth_crop):
    """Reject second-stage segments that overlap the first-stage mask by < 50 %, order the crops
    (far-to-near by mean depth, or large-to-small ROI without depth) and paste the renumbered
    segments back at ROI resolution; later crops overwrite earlier ones.
    Returns (refined (1,H,W) float, labels_crop with rejected segments set to -1).

    The reference's per-crop / per-segment loops (test_dataset.py:116-179) are table lookups here: two histograms for
    the overlap test, one (crop, label) -> new number table for the renumbering, and two host transfers in all (the
    sort keys and the ROIs).  The mean depth of a crop is accumulated in fp64 (the reference's fp32 torch.mean can
    order two crops whose mean depths agree to ~1e-7 either way)."""
    num = labels_crop.shape[0]
    dev = labels_crop.device
    refined = torch.zeros_like(initial_masks).float()
    if num == 0:
        return refined, labels_crop
    k = int(LABEL_BINS)
    stats, hit, _ = label_stats(labels_crop, out_label_crop)
    area = stats[:, :, 0].reshape(-1)
    lab = labels_crop.reshape(num, -1).to(torch.int64).clamp(0, k - 1) + torch.arange(num, device=dev)[:, None] * k
    bad = (hit.reshape(-1) / area.float().clamp_min(1.0) < 0.5) & (area > 0)
    labels_crop.masked_fill_(bad[lab].view_as(labels_crop), -1)
    rois_host = [[int(v) for v in r] for r in rois.tolist()]
    if depth_crop is not None:
        sel = (labels_crop > -1).reshape(num, -1)
        z = depth_crop[:, 2].reshape(num, -1)
        use = (sel | ~sel.any(1, keepdim=True)) & (z > 0)
        keys = ((z * use).sum(1, dtype=torch.float64) / use.sum(1)).tolist()            # 0/0 = nan like mean of nothing
    else:
        keys = [float((r[3] - r[1] + 1) * (r[2] - r[0] + 1)) for r in rois_host]
    order = [i for i, _ in sorted(enumerate(keys), key=lambda t: t[1], reverse=True)]
    # new numbers 1.. in (crop order, ascending surviving label) order
    order_t = torch.tensor(order, device=dev)
    alive = ((area > 0) & ~bad).view(num, k)[order_t]
    number = torch.zeros((num, k), dtype=torch.float32, device=dev)
    number[order_t] = (torch.cumsum(alive.reshape(-1), 0).view(num, k) * alive).float()
    renum = number.view(-1)[lab].view(num, 1, *labels_crop.shape[1:])
    for i in order:
        x0, y0, x1, y1 = rois_host[i]
        small = F.interpolate(renum[i:i + 1], size=(y1 - y0 + 1, x1 - x0 + 1), mode="nearest")[0, 0]
        window = refined[0, y0:y1 + 1, x0:x1 + 1]
        window.copy_(torch.where(small != 0, small, window))
    return refined, labels_crop


def nms(masks, scores, thresh):
    """Mask-IoU NMS, kept indices sorted by mask area (lib/fcn/nms.py:3-23).  numpy in / out."""
    flat = masks.reshape(masks.shape[0], -1).astype(np.float32)
    inters = flat @ flat.T
    areas = np.diag(inters)
    order = scores.argsort()[::-1]
    keep = []
    while order.size > 0:
        i = order[0]
        keep.append(i)
        inter = inters[i, order[1:]]
        ovr = inter / (areas[i] + areas[order[1:]] - inter)
        order = order[np.where(ovr <= thresh)[0] + 1]
    return np.array(keep)[np.argsort(areas[keep]).astype(np.int32)]


def combine_masks_with_NMS(instances):
    """Label image (labels from 2), per-pixel int(score*100) image and (N,5) boxes [x1,y1,x2,y2,score]
    after NMS at 0.7 (lib/fcn/test_utils.py:55-91)."""
    mask = instances.get("pred_masks").to("cpu").numpy()
    scores = instances.get("scores").to("cpu").numpy()
    h, w = (mask.shape[1], mask.shape[2]) if mask.ndim == 3 and mask.shape[0] else instances.image_size
    bin_mask, score_mask = np.zeros((h, w)), np.zeros((h, w))
    if len(mask) == 0:
        return bin_mask, score_mask, np.zeros((0, 5), dtype=np.float32)
    keep = nms(mask, scores, thresh=0.7).astype(int)
    mask, scores = mask[keep], scores[keep]
    bbox = np.zeros((len(mask), 5), dtype=np.float32)
    for k, m in enumerate(mask):
        pos = np.nonzero(m)
        bin_mask[pos] = k + 2
        score_mask[pos] = int(scores[k] * 100)
        bbox[k] = [pos[1].min(), pos[0].min(), pos[1].max(), pos[0].max(), scores[k]]
    return bin_mask, score_mask, bbox


def label_image(outputs, topk, confident_score, low_threshold, num_class):
    """combine_masks(get_confident_instances(outputs, ...)) (test_utils.py:35-53, 93-112) without selecting the
    instances first: instance i, if kept, carries label 2 + (number of kept instances before it), and "later
    instances overwrite earlier ones" is the per-pixel maximum of those labels.  Same values as the two reference
    steps, no data-dependent shapes, so no device -> host round trip.  Returns an (H,W) float64 tensor."""
    inst = outputs["instances"]
    masks, scores = inst.get("pred_masks"), inst.get("scores")
    if masks.dim() != 3 or masks.shape[0] == 0:
        h, w = inst.image_size
        return torch.zeros((h, w), dtype=torch.float64, device=scores.device)
    if topk:
        keep = ((inst.get("pred_classes") == 1) & (scores > low_threshold)) if num_class >= 2 else torch.ones_like(scores, dtype=torch.bool)
    else:
        keep = scores > confident_score
    lab = ((torch.cumsum(keep, 0) + 1) * keep).to(torch.int16)
    return ((masks != 0).to(torch.int16) * lab[:, None, None]).amax(0).to(torch.float64)


def _labels_from_outputs(outputs, topk, confident_score, low_threshold, num_class, use_nms):
    if use_nms:
        conf = get_confident_instances(outputs, topk=topk, score=confident_score, num_class=num_class,
                                       low_threshold=low_threshold)
        return combine_masks_with_NMS(conf)
    return label_image(outputs, topk, confident_score, low_threshold, num_class), None, None


def test_sample_crop_nolabel(sample, predictor, predictor_crop=None, *, use_depth=True, topk=False,
                             confident_score=0.7, low_threshold=0.4, num_class=2, use_nms=False,
                             depth_threshold=0.5, crop_batch_builder=None):
    """First-stage prediction -> label image -> depth filter -> ROI crops -> second-stage prediction on
    every crop -> paste back (lib/fcn/test_utils.py:339-421).

    sample: {"image_color" (3,H,W), "depth" (3,H,W) xyz (when use_depth), ...}.  `predictor(sample)`
    returns {"instances": Instances}; `predictor_crop` is called ONCE with a list of crop samples
    (batched) when it exposes ``batch_call``, else once per crop."""
    return _sample_crop(sample, predictor, predictor_crop, use_depth=use_depth, topk=topk, confident_score=confident_score,
                        low_threshold=low_threshold, num_class=num_class, use_nms=use_nms, depth_threshold=depth_threshold)[1:]


def _sample_crop(sample, predictor, predictor_crop, *, use_depth, topk, confident_score, low_threshold, num_class, use_nms,
                 depth_threshold):
    """test_sample_crop_nolabel's steps -> (first-stage label image before the depth filter, out_label, refined, out_score, bbox)."""
    image = sample["image_color"]
    if image.dim() == 4:
        image = image[0]
    sample = dict(sample, image=image, height=image.shape[-2], width=image.shape[-1])
    depth = None
    if use_depth:
        depth = sample["depth"]
        depth = depth[0] if depth.dim() == 4 else depth
    else:
        sample["depth"] = None
    label, score_mask, bbox = _labels_from_outputs(predictor(sample), topk, confident_score, low_threshold, num_class, use_nms)
    dev = image.device
    out_label = torch.as_tensor(label).unsqueeze(0).to(dev)
    out_score = torch.as_tensor(score_mask).unsqueeze(0).to(dev) if score_mask is not None else None
    image4 = image.unsqueeze(0)
    depth4 = depth.unsqueeze(0) if depth is not None else None
    if depth4 is not None:
        thr = 0.8 if "OSD" in str(sample.get("file_name", "")) else depth_threshold      # test_utils.py:384-387
        out_label = filter_labels_depth(out_label, depth4, thr)
    refined = None
    if predictor_crop is not None:
        rgb_crop, out_label_crop, rois, depth_crop = crop_rois(image4, out_label.clone(), depth4)
        n = rgb_crop.shape[0]
        if n > 0:
            crops = [{"image": rgb_crop[i], "height": CROP_SIZE, "width": CROP_SIZE,
                      "depth": depth_crop[i] if depth_crop is not None else None} for i in range(n)]
            outs = predictor_crop.batch_call(crops) if hasattr(predictor_crop, "batch_call") else [predictor_crop(c) for c in crops]
            labels_crop = torch.zeros((n, CROP_SIZE, CROP_SIZE), device=dev)
            for i, o in enumerate(outs):
                lab, _, _ = _labels_from_outputs(o, topk, confident_score, low_threshold, num_class, use_nms)
                labels_crop[i] = torch.as_tensor(lab).to(dev)
            refined, _ = match_label_crop(out_label, labels_crop, out_label_crop, rois, depth_crop)
    return label, out_label, refined, out_score, bbox


# ----------------------------------------------------------------------------------------------------------------------
# The labelled harness (lib/fcn/test_utils.py:169-205, 245-336, 424-513): the same pipelines, scored against the sample's
# ground truth with evaluation.multilabel_metrics.
# ----------------------------------------------------------------------------------------------------------------------
def _sample_gt(sample):
    """The ground-truth label image of a sample: sample["label"], else sample["labels"], squeezed to (H,W)."""
    gt = sample["label"] if "label" in sample else sample["labels"]
    gt = torch.as_tensor(gt)
    return gt.reshape(gt.shape[-2:])


def test_sample(sample, predictor, *, topk=False, confident_score=0.9, low_threshold=0.4, num_class=2, use_nms=False):
    """lib/fcn/test_utils.py:169-205: the first-stage label image of sample["image_color"] scored against the sample's ground
    truth -> the multilabel_metrics dict."""
    from .evaluation import multilabel_metrics
    image = sample["image_color"]
    if image.dim() == 4:
        image = image[0]
    sample = dict(sample, image=image, height=image.shape[-2], width=image.shape[-1])
    sample.setdefault("depth", None)
    label, _, _ = _labels_from_outputs(predictor(sample), topk, confident_score, low_threshold, num_class, use_nms)
    return multilabel_metrics(torch.as_tensor(label).to(image.device), _sample_gt(sample))


def test_sample_crop(sample, predictor, predictor_crop=None, *, use_depth=True, topk=False, confident_score=0.7, low_threshold=0.4,
                     num_class=2, use_nms=False, depth_threshold=0.5):
    """lib/fcn/test_utils.py:245-336: test_sample_crop_nolabel's pipeline scored against the sample's ground truth ->
    (metrics, metrics_refined).  As in the reference:
      * ``metrics`` scores the combined first-stage label image BEFORE the depth filter;
      * ``metrics_refined`` scores the refined label image, or -- no second stage, or no crop -- the depth-filtered
        first-stage image;
      * the ground truth is sample["label"], else sample["labels"] (the reference tests "label" twice and never reads
        "labels", so a sample with "labels" only is scored against None there, test_utils.py:252-255)."""
    from .evaluation import multilabel_metrics
    gt = _sample_gt(sample)
    label, out_label, refined, _, _ = _sample_crop(sample, predictor, predictor_crop, use_depth=use_depth, topk=topk,
                                                   confident_score=confident_score, low_threshold=low_threshold,
                                                   num_class=num_class, use_nms=use_nms, depth_threshold=depth_threshold)
    dev = out_label.device
    metrics = multilabel_metrics(torch.as_tensor(label).to(dev), gt)
    metrics_refined = multilabel_metrics((refined if refined is not None else out_label)[0], gt)
    return metrics, metrics_refined


def test_dataset(dataset, predictor, **kw):
    """lib/fcn/test_utils.py:424-460: test_sample over every sample of ``dataset`` -> the per-key mean (evaluation.average_metrics).
    Keyword arguments as test_sample (the reference's defaults here: topk=False, confident_score=0.7)."""
    from .evaluation import average_metrics
    kw = dict(dict(topk=False, confident_score=0.7, low_threshold=0.4), **kw)
    return average_metrics([test_sample(dataset[i], predictor, **kw) for i in range(len(dataset))])


def test_dataset_crop(dataset, predictor, predictor_crop, **kw):
    """lib/fcn/test_utils.py:462-513: test_sample_crop over every sample -> (mean metrics, mean refined metrics).  Keyword
    arguments as test_sample_crop (the reference's defaults here: topk=True, confident_score=0.9)."""
    from .evaluation import average_metrics
    kw = dict(dict(topk=True, confident_score=0.9, low_threshold=0.4), **kw)
    pairs = [test_sample_crop(dataset[i], predictor, predictor_crop, **kw) for i in range(len(dataset))]
    return average_metrics([p[0] for p in pairs]), average_metrics([p[1] for p in pairs])


# ----------------------------------------------------------------------------------------------------------------------
# The same pipeline for a BATCH of frames (BASELINE configs[3]: batch = 16): lib/fcn/test_utils.py:375-406 is a serial
# loop over frames and, inside it, over crops (batch 1 each).  Nothing couples two frames, so here the first stage runs
# on all frames in one call, every frame's ROIs are cut in one launch (ops.crop_resize), all crops of all frames go
# through the second stage in batches of `crop_batch` (measured at 171 crops: one call 20.8 ms, three calls of <= 64 22.2 ms), and every frame's refined labels are pasted in one launch
# (ops.paste_labels).  Two device -> host transfers per batch in all (the label statistics that define the ROIs, the
# depth keys that order the paste).  Per frame the results are those of test_sample_crop_nolabel; with use_nms=True the label
# images of both stages come from combine_masks_with_NMS_batched (no transfer either).
# ----------------------------------------------------------------------------------------------------------------------
def _raw_batch(samples):
    """True when the samples hold raw camera frames ("color" (H,W,3) uint8, "depth_raw" (H,W) uint16 or float32, "camera_params" --
    frames.ingest's arguments) instead of the finished float tensors ("image_color", "depth"); a batch holds one kind."""
    raw = ["color" in s for s in samples]
    if any(raw) and not all(raw):
        raise ValueError("raw camera frames (\"color\") and float samples (\"image_color\") cannot be mixed in one batch")
    return bool(raw) and raw[0]


def _raw_tensor(a):
    """A raw colour / depth image as a tensor where it lives (numpy -> host tensor); uint16 as int16 holding the same bits (what
    ops.ingest_frames and frames.ingest take: torch has few uint16 kernels)."""
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.view(torch.int16) if t.dtype == torch.uint16 else t


def _raw_arrays(samples, key, dtypes, shape=None):
    """samples[f][key] of a raw batch as tensors (_raw_tensor), checked to be ONE kind: one of ``dtypes``, one shape (``shape`` when
    given), all on the host or all on one device -- a ValueError names the first sample that differs."""
    arrays = [_raw_tensor(s[key]) for s in samples]
    first = arrays[0]
    if first.dtype not in dtypes:
        raise ValueError(f"raw frames: \"{key}\" must be one of {[str(d) for d in dtypes]} (uint16 as such or as int16 bits), got {first.dtype}")
    want = tuple(first.shape) if shape is None else tuple(shape)
    for f, t in enumerate(arrays):
        if tuple(t.shape) != want:
            raise ValueError(f"raw frames: \"{key}\" of sample {f} has shape {tuple(t.shape)}, {want} expected")
        if t.dtype != first.dtype or t.device != first.device:
            raise ValueError(f"raw frames: \"{key}\" of sample {f} is {t.dtype} on {t.device}, sample 0 is {first.dtype} on {first.device}: "
                             "one dtype and one place per batch")
    return arrays


_RAW_COLOR, _RAW_DEPTH = (torch.uint8,), (torch.int16, torch.float32)


def _batch_tensors(predictor, samples):
    """(scores (B,K), classes (B,K), masks (B,K,H,W)) of a list of samples: a predictor that exposes ``batch_tensors`` hands the
    batched tensors of its model over as they are; otherwise the per-sample Instances are stacked (a copy)."""
    if hasattr(predictor, "batch_tensors"):
        return predictor.batch_tensors(samples)
    outs = predictor.batch_call(samples) if hasattr(predictor, "batch_call") else [predictor(s) for s in samples]
    inst = [o["instances"] for o in outs]
    return (torch.stack([i.get("scores") for i in inst]), torch.stack([i.get("pred_classes") for i in inst]),
            torch.stack([i.get("pred_masks") for i in inst]))


def candidate_flags(scores, classes, topk, confident_score, low_threshold, num_class):
    """The get_confident_instances selection (test_utils.py:35-52) as a flag per instance instead of a compaction: scores /
    classes (B,K) -> (B,K) bool.  What instance_labels numbers and combine_masks_with_NMS_batched takes as ``candidate``."""
    if topk:
        return ((classes == 1) & (scores > low_threshold)) if num_class >= 2 else torch.ones_like(scores, dtype=torch.bool)
    return scores > confident_score


def instance_labels(scores, classes, topk, confident_score, low_threshold, num_class):
    """The label each instance carries in the label image (label_image above, batched): 2 + (kept instances before it), 0
    when the instance is dropped (get_confident_instances, test_utils.py:35-52).  scores / classes (B,K) -> (B,K) float."""
    keep = candidate_flags(scores, classes, topk, confident_score, low_threshold, num_class)
    return ((torch.cumsum(keep, 1) + 1) * keep).float()


def _mask_nms_host(masks, scores, candidate, thresh):
    """combine_masks_with_NMS_batched's definition in numpy integer and fp32 operations (host tensors: the CPU tests)."""
    m = masks.numpy() != 0
    s_all = scores.numpy().astype(np.float32)
    c_all = candidate.numpy() != 0
    B, K, H, W = m.shape
    label, score = np.zeros((B, H, W), dtype=np.float32), np.zeros((B, H, W), dtype=np.float32)
    bbox, count = np.zeros((B, K, 5), dtype=np.float32), np.zeros((B,), dtype=np.int32)
    thr = np.float32(thresh)
    for b in range(B):
        s = s_all[b]
        idx = np.nonzero(c_all[b] & ~np.isnan(s))[0]
        flat = m[b, idx].reshape(len(idx), H * W).astype(np.int32)
        inter = flat @ flat.T                                         # exact int32 counts
        area = np.diag(inter)
        pos = np.nonzero(area > 0)[0]                                 # an empty candidate is dropped before NMS
        order = pos[np.argsort(s[idx[pos]], kind="stable")[::-1]]     # descending score, equal scores the higher index first
        alive = np.ones(len(order), dtype=bool)
        keep = []
        for p, i in enumerate(order):
            if not alive[p]:
                continue
            keep.append(i)
            rest = order[p + 1:]
            with np.errstate(divide="ignore", invalid="ignore"):
                iou = inter[i, rest].astype(np.float32) / (area[i] + area[rest] - inter[i, rest]).astype(np.float32)
            alive[p + 1:] &= iou <= thr                               # one fp32 division; a NaN quotient suppresses
        keep = np.array(keep, dtype=np.int64)
        keep = keep[np.argsort(area[keep], kind="stable")]            # area ascending, equal areas in the order kept
        for r, i in enumerate(keep):
            k = idx[i]
            sel = m[b, k]
            label[b][sel] = r + 2                                     # larger masks overwrite smaller ones
            score[b][sel] = np.trunc(np.float32(s[k]) * np.float32(100))
            ys, xs = np.nonzero(sel)
            bbox[b, r] = [xs.min(), ys.min(), xs.max(), ys.max(), s[k]]
        count[b] = len(keep)
    return torch.from_numpy(label), torch.from_numpy(score), torch.from_numpy(bbox), torch.from_numpy(count)


def combine_masks_with_NMS_batched(masks, scores, candidate, thresh=0.7, workspace=None):
    """nms (lib/fcn/nms.py:3-23) + combine_masks_with_NMS (lib/fcn/test_utils.py:55-91) for B images at once, on fixed shapes:
    masks (B,K,H,W) (non-zero = inside), scores (B,K), candidate (B,K) bool -- the get_confident_instances selection as a FLAG
    (candidate_flags), not a compaction -> (label (B,H,W), score (B,H,W), bbox (B,K,5), count (B,) int32), all float32 but count.

    Definition (the same text is in include/msm_hip.h), per image:
      * inter[i][j] = number of pixels inside both masks, area[i] = inter[i][i]: int32, exact.
      * Candidates are visited in descending score order; equal scores the higher index first (a stable ascending argsort,
        reversed).  A NaN score is never a candidate.  A candidate whose mask is empty is dropped before NMS.
      * Greedy suppression: with kept i, candidate j survives iff float32(inter) / float32(area_i + area_j - inter) <=
        float32(thresh) -- one correctly rounded fp32 division; a NaN quotient suppresses.
      * Kept instances are ordered by area ascending, equal areas in the order they were kept; rank r carries label 2 + r.
      * label[y][x] = the largest label among the kept masks covering the pixel (larger masks overwrite smaller ones), else 0;
        score[y][x] = trunc(float32(score_k) * float32(100)) of that same mask, else 0.
      * bbox[r] = (x_min, y_min, x_max, y_max, score) of the WHOLE kept mask of rank r; rows from count on are zero; count =
        number kept.

    Device tensors go through the HIP kernels (ops.mask_nms: bit planes, popcounts, no host synchronisation; ``workspace`` as
    there); host tensors -- the CPU tests -- through the same definition in numpy integer and fp32 operations."""
    B, K, H, W = masks.shape
    if tuple(scores.shape) != (B, K) or tuple(candidate.shape) != (B, K):
        raise ValueError(f"scores / candidate must be (B,K) = ({B},{K}), got {tuple(scores.shape)} / {tuple(candidate.shape)}")
    if B == 0 or K == 0:
        dev = masks.device
        return (torch.zeros((B, H, W), device=dev), torch.zeros((B, H, W), device=dev), torch.zeros((B, K, 5), device=dev),
                torch.zeros((B,), dtype=torch.int32, device=dev))
    if masks.is_cuda:
        from . import ops
        return ops.mask_nms(masks.float().contiguous(), scores.float().contiguous(), (candidate != 0).contiguous(), thresh, workspace)[:4]
    return _mask_nms_host(masks, scores.float(), candidate, thresh)


def roi_table(stats, overflow, H, W):
    """Host side of crop_rois for a batch: stats (F,k,5) / overflow (F,) as numpy (ONE transfer) -> list of rows
    [frame, label, x0, y0, x1, y1, 0, 0] in (frame, ascending label) order, boxes padded by 25 % and clipped
    (test_dataset.py:76-92; round half to even like torch.round)."""
    if overflow.any():
        raise ValueError(f"label image values must be integers in [0, {LABEL_BINS})")
    rows = []
    for f in range(stats.shape[0]):
        t = stats[f]
        for v in np.nonzero(t[:, 0])[0]:
            if v == 0:
                continue
            x0, y0, x1, y1 = (int(t[v, 1]), int(t[v, 2]), int(t[v, 3]), int(t[v, 4]))
            xp, yp = int(round((x1 - x0) * PADDING_PERCENTAGE)), int(round((y1 - y0) * PADDING_PERCENTAGE))
            rows.append([f, int(v), max(x0 - xp, 0), max(y0 - yp, 0), min(x1 + xp, W - 1), min(y1 + yp, H - 1), 0, 0])
    return rows


# GPU tensors go through the HIP kernels; CPU tensors -- the host-logic unit tests -- through the same definitions in torch ops
# (the reference's own per-ROI F.interpolate calls), like label_stats above.
def _label_image_batched(masks, inst_labels):
    if masks.is_cuda:
        from . import ops
        return ops.label_image(masks.float().contiguous(), inst_labels.float().contiguous())
    return ((masks != 0).float() * inst_labels[:, :, None, None].float()).amax(1) if masks.shape[1] else masks.new_zeros((masks.shape[0],) + masks.shape[2:])


def _crop_resize_batched(images, depths, labels, rows, size):
    if images.is_cuda:
        from . import ops
        return ops.crop_resize(images, depths, labels, torch.tensor(rows, dtype=torch.int32, device=images.device), size)
    n = len(rows)
    rgb = torch.zeros((n, 3, size, size))
    msk = torch.zeros((n, size, size))
    dep = torch.zeros((n, 3, size, size)) if depths is not None else None
    for k, (f, lab, x0, y0, x1, y1, _, _) in enumerate(rows):
        rgb[k] = F.interpolate(images[f:f + 1, :, y0:y1 + 1, x0:x1 + 1], size=(size, size), mode="bilinear", align_corners=True)[0]
        msk[k] = F.interpolate((labels[f, y0:y1 + 1, x0:x1 + 1] == lab).float()[None, None], size=(size, size), mode="nearest")[0, 0]
        if depths is not None:
            dep[k] = F.interpolate(depths[f:f + 1, :, y0:y1 + 1, x0:x1 + 1], size=(size, size), mode="bilinear", align_corners=True)[0]
    return rgb, msk, dep


def _paste_batched(renum, rows, order, frame_start, frames, H, W):
    if renum.is_cuda:
        from . import ops
        dev = renum.device
        return ops.paste_labels(renum, torch.tensor(rows, dtype=torch.int32, device=dev), torch.tensor(order, dtype=torch.int32, device=dev),
                                torch.tensor(frame_start, dtype=torch.int32, device=dev), frames, H, W)
    refined = torch.zeros((frames, H, W))
    for f in range(frames):
        for n in order[frame_start[f]:frame_start[f + 1]]:
            _, _, x0, y0, x1, y1, _, _ = rows[n]
            small = F.interpolate(renum[n][None, None], size=(y1 - y0 + 1, x1 - x0 + 1), mode="nearest")[0, 0]
            window = refined[f, y0:y1 + 1, x0:x1 + 1]
            window.copy_(torch.where(small != 0, small, window))
    return refined


def _match_pre(labels_crop, out_label_crop, depth_crop):
    """Device half of match_label_crop_batched, before the paste order is known: the overlap test (second-stage segments that cover
    the first-stage mask by < 50 % are set to -1 in ``labels_crop``, in place) and the crops' sort keys (mean valid depth of the
    surviving segments, fp64; None without depth).  -> (area (N*k,), bad (N*k,), lab (N, S*S) indices into them, keys (N,) or None).
    No host transfer, no data-dependent shape: this half is captured in the second-stage HIP graph of BatchedTwoStage."""
    num = labels_crop.shape[0]
    k = int(LABEL_BINS)
    stats, hit, _ = label_stats(labels_crop, out_label_crop)
    area = stats[:, :, 0].reshape(-1)
    lab = labels_crop.reshape(num, -1).to(torch.int64).clamp(0, k - 1) + torch.arange(num, device=labels_crop.device)[:, None] * k
    bad = (hit.reshape(-1) / area.float().clamp_min(1.0) < 0.5) & (area > 0)
    labels_crop.masked_fill_(bad[lab].view_as(labels_crop), -1)
    keys = None
    if depth_crop is not None:
        sel = (labels_crop > -1).reshape(num, -1)
        z = depth_crop[:, 2].reshape(num, -1)
        use = (sel | ~sel.any(1, keepdim=True)) & (z > 0)
        keys = (z * use).sum(1, dtype=torch.float64) / use.sum(1)                       # 0/0 = nan like mean of nothing
    return area, bad, lab, keys


def _match_post(area, bad, lab, keys, rows, frames, H, W, crop_shape):
    """Host-ordered half: ``keys`` (list of floats, one per crop of ``rows``) -> paste order inside every frame, renumbering, paste.
    area / bad / lab may describe MORE crops than len(rows) (a padded second-stage batch): only the first len(rows) are used."""
    num = len(rows)
    k = int(LABEL_BINS)
    dev = lab.device
    area, bad, lab = area.view(-1, k)[:num].reshape(-1), bad.view(-1, k)[:num].reshape(-1), lab[:num]
    frame_of = [r[0] for r in rows]
    # paste order inside a frame: descending key, ties and NaN exactly as sorted(reverse=True) leaves them in match_label_crop
    order, frame_start = [], [0]
    by_frame = [[] for _ in range(frames)]
    for n, f in enumerate(frame_of):
        by_frame[f].append(n)
    for mine in by_frame:
        order += [mine[i] for i, _ in sorted(enumerate([keys[n] for n in mine]), key=lambda t: t[1], reverse=True)]
        frame_start.append(len(order))
    order_t = torch.tensor(order, device=dev)
    alive = ((area > 0) & ~bad).view(num, k)[order_t]                                    # rows in (frame, paste) order
    c = torch.cumsum(alive.reshape(-1), 0).view(num, k)
    # numbers restart at 1 in every frame: subtract what was counted before the frame's first crop
    before = torch.cat([c.new_zeros(1), c[:, -1]])[torch.tensor([frame_start[frame_of[n]] for n in order], device=dev)]
    number = torch.zeros((num, k), dtype=torch.float32, device=dev)
    number[order_t] = ((c - before[:, None]) * alive).float()
    renum = number.view(-1)[lab].view(num, *crop_shape).contiguous()
    return _paste_batched(renum, rows, order, frame_start, frames, H, W)


def match_label_crop_batched(initial_masks, labels_crop, out_label_crop, rows, depth_crop):
    """match_label_crop for the crops of a whole batch of frames: initial_masks (F,H,W), labels_crop / out_label_crop
    (N,S,S), rows = roi_table(...) (crop n belongs to frame rows[n][0]), depth_crop (N,3,S,S) or None.
    Returns refined (F,H,W).  Same arithmetic per frame as match_label_crop; the renumbering restarts at 1 in every frame."""
    Fr, H, W = initial_masks.shape
    if labels_crop.shape[0] == 0:
        return torch.zeros_like(initial_masks).float()
    area, bad, lab, keys = _match_pre(labels_crop, out_label_crop, depth_crop)
    if keys is not None:
        keys = keys.tolist()                                                             # the batch's second (last) transfer
    else:
        keys = [float((r[5] - r[3] + 1) * (r[4] - r[2] + 1)) for r in rows]
    return _match_post(area, bad, lab, keys, rows, Fr, H, W, tuple(labels_crop.shape[1:]))


def test_batch_crop_nolabel(samples, predictor, predictor_crop=None, *, use_depth=True, topk=False, confident_score=0.7,
                            low_threshold=0.4, num_class=2, depth_threshold=0.5, crop_batch=256, stages=None, order="bgr",
                            depth_scale=1000.0, use_nms=False, nms_thresh=0.7, extras=None):
    """test_sample_crop_nolabel for a list of frames of one size, batched end to end.  ``use_nms``: both stages build their label
    images through combine_masks_with_NMS_batched at ``nms_thresh`` (the reference's configuration for real images, test_utils.py:30,
    376, 396-405) instead of the plain overwrite order, and ``extras`` (a dict) receives the first stage's "out_score" (F,H,W), "bbox"
    (F,K,5) and "count" (F,).
    samples: [{"image_color" (3,H,W), "depth" (3,H,W), ...}, ...] on the GPU -- or raw camera frames [{"color" (H,W,3) uint8,
    "depth_raw" (H,W) uint16 (/ ``depth_scale``) or float32 metres, "camera_params"}, ...] in channel order ``order``, all of one
    dtype and in one place, ingested in one launch (frames.ingest).  Returns (out_label (F,H,W), refined (F,H,W) or
    None, rows) -- frame f's results equal test_sample_crop_nolabel(samples[f], ...)[0][0] / [1][0]; ``rows`` is the ROI table
    (frame, label, x0, y0, x1, y1, 0, 0) of the second stage.  ``stages``: a dict that receives the intermediate tensors
    (crops, second-stage label images) -- for tests."""
    return _batch_crop(samples, predictor, predictor_crop, use_depth=use_depth, topk=topk, confident_score=confident_score,
                       low_threshold=low_threshold, num_class=num_class, depth_threshold=depth_threshold, crop_batch=crop_batch,
                       stages=stages, order=order, depth_scale=depth_scale, use_nms=use_nms, nms_thresh=nms_thresh, extras=extras)[1:]


def _batch_crop(samples, predictor, predictor_crop, *, use_depth, topk, confident_score, low_threshold, num_class, depth_threshold,
                crop_batch, stages, order="bgr", depth_scale=1000.0, use_nms=False, nms_thresh=0.7, extras=None):
    """test_batch_crop_nolabel's steps -> (first-stage label images before the depth filter, out_label, refined, rows)."""
    if _raw_batch(samples):                                  # camera frames: the whole batch ingested at once (one launch on the device)
        from . import frames
        color = torch.stack(_raw_arrays(samples, "color", _RAW_COLOR))
        images, depths = frames.ingest(color, torch.stack(_raw_arrays(samples, "depth_raw", _RAW_DEPTH, color.shape[1:3])) if use_depth else None,
                                       [s["camera_params"] for s in samples] if use_depth else None, order=order, depth_scale=depth_scale)
    else:
        images = torch.stack([s["image_color"][0] if s["image_color"].dim() == 4 else s["image_color"] for s in samples]).float().contiguous()
        depths = None
        if use_depth:
            depths = torch.stack([s["depth"][0] if s["depth"].dim() == 4 else s["depth"] for s in samples]).float().contiguous()
    Fr, _, H, W = images.shape
    first = [{"image": images[f], "depth": depths[f] if depths is not None else None, "height": H, "width": W} for f in range(Fr)]
    kw = dict(topk=topk, confident_score=confident_score, low_threshold=low_threshold, num_class=num_class)
    scores, classes, masks = _batch_tensors(predictor, first)
    if use_nms:
        label, out_score, bbox, count = combine_masks_with_NMS_batched(masks, scores, candidate_flags(scores, classes, **kw), nms_thresh)
        out_label = label
        if extras is not None:
            extras.update(out_score=out_score, bbox=bbox, count=count)
    else:
        label = out_label = _label_image_batched(masks, instance_labels(scores, classes, **kw))
    if depths is not None:
        thr = torch.tensor([0.8 if "OSD" in str(s.get("file_name", "")) else depth_threshold for s in samples],
                           device=images.device, dtype=torch.float32)[:, None]          # test_utils.py:384-387
        out_label = filter_labels_depth(out_label, depths, thr)
    if predictor_crop is None:
        return label, out_label, None, []
    stats, _, overflow = label_stats(out_label)
    packed = torch.cat([stats.reshape(-1), overflow]).cpu().numpy()                      # the batch's first transfer
    rows = roi_table(packed[:-Fr].reshape(Fr, -1, 5), packed[-Fr:], H, W)
    n = len(rows)
    if n == 0:
        return label, out_label, torch.zeros_like(out_label), rows
    rgb_crop, mask_crop, depth_crop = _crop_resize_batched(images, depths, out_label, rows, CROP_SIZE)
    labels_crop = torch.empty((n, CROP_SIZE, CROP_SIZE), device=images.device, dtype=torch.float32)
    for c0 in range(0, n, crop_batch):
        c1 = min(n, c0 + crop_batch)
        crops = [{"image": rgb_crop[i], "height": CROP_SIZE, "width": CROP_SIZE,
                  "depth": depth_crop[i] if depth_crop is not None else None} for i in range(c0, c1)]
        s2, k2, m2 = _batch_tensors(predictor_crop, crops)
        if use_nms:
            labels_crop[c0:c1] = combine_masks_with_NMS_batched(m2, s2, candidate_flags(s2, k2, **kw), nms_thresh)[0]
        else:
            labels_crop[c0:c1] = _label_image_batched(m2, instance_labels(s2, k2, **kw))
    if stages is not None:
        stages.update(rgb_crop=rgb_crop, mask_crop=mask_crop, depth_crop=depth_crop, labels_crop=labels_crop.clone())
    refined = match_label_crop_batched(out_label, labels_crop, mask_crop, rows, depth_crop)
    return label, out_label, refined, rows


def test_batch_crop(samples, predictor, predictor_crop=None, *, use_depth=True, topk=False, confident_score=0.7, low_threshold=0.4,
                    num_class=2, depth_threshold=0.5, crop_batch=256, order="bgr", depth_scale=1000.0, use_nms=False, nms_thresh=0.7):
    """The labelled form of test_batch_crop_nolabel (raw camera frames included): every frame of the batch scored against its sample's ground truth
    ("label", else "labels") -> (metrics, metrics_refined), two lists of per-frame dicts equal to test_sample_crop(samples[f],
    ...): the first-stage label image before the depth filter, and the refined image of a frame that has crops, else its
    depth-filtered first-stage image.  All 2F images are scored by ONE evaluation.multilabel_metrics_batched call."""
    from .evaluation import multilabel_metrics_batched
    label, out_label, refined, rows = _batch_crop(samples, predictor, predictor_crop, use_depth=use_depth, topk=topk,
                                                  confident_score=confident_score, low_threshold=low_threshold, num_class=num_class,
                                                  depth_threshold=depth_threshold, crop_batch=crop_batch, stages=None, order=order,
                                                  depth_scale=depth_scale, use_nms=use_nms, nms_thresh=nms_thresh)
    Fr = label.shape[0]
    dev = label.device
    gt = torch.stack([_sample_gt(s).to(dev).float() for s in samples])
    second = out_label.float()
    if refined is not None:
        cropped = torch.zeros(Fr, dtype=torch.bool)
        cropped[sorted({r[0] for r in rows})] = True
        second = torch.where(cropped.to(dev)[:, None, None], refined.float(), second)
    m = multilabel_metrics_batched(torch.cat([label.float(), second]), torch.cat([gt, gt]))
    return m[:Fr], m[Fr:]


# ----------------------------------------------------------------------------------------------------------------------
# configs[3] as a replayable pipeline: both stages from captured HIP graphs, the two device -> host transfers of a batch
# overlapped with the other batch in flight.
# ----------------------------------------------------------------------------------------------------------------------
class LRUBuckets:
    """A dict in least-recently-used order with a cap: ``put`` of a new key into a full table first evicts the least recently used
    entry and hands it to ``on_evict(key, value)``; ``get`` of a present key makes it the most recent.  ``cap=None`` never evicts.
    Host-only bookkeeping (the crop buckets of a BatchedTwoStage slot: the callback waits for the slot's stream before the entry's
    graph and buffers are dropped)."""

    def __init__(self, cap=None, on_evict=None):
        if cap is not None and int(cap) < 1:
            raise ValueError(f"the cap must be at least 1 (or None for no cap), got {cap}")
        self.cap = None if cap is None else int(cap)
        self.on_evict = on_evict
        self._d = collections.OrderedDict()

    def get(self, key, default=None):
        if key not in self._d:
            return default
        self._d.move_to_end(key)
        return self._d[key]

    def put(self, key, value):
        if key in self._d:
            self._d.move_to_end(key)
        else:
            while self.cap is not None and len(self._d) >= self.cap:
                old, gone = self._d.popitem(last=False)
                if self.on_evict is not None:
                    self.on_evict(old, gone)
                del gone
        self._d[key] = value
        return value

    def keys(self):
        """Least recently used first."""
        return list(self._d)

    def __contains__(self, key):
        return key in self._d

    def __len__(self):
        return len(self._d)


class BatchedTwoStage:
    """test_batch_crop_nolabel (lib/fcn/test_utils.py:339-421 per frame) for batches of ``frames`` frames of one
    size, with the model called directly (``model.inference_images``: backbone + head + post-processing) and both stages replayed
    from HIP graphs:

      graph 1   frames -> model -> label images -> depth filter -> label statistics -> pinned host buffer   (fixed shapes)
      host      ROI table from the statistics (test_dataset.py:76-92), uploaded into the slot's table buffer
      graph 2   (one per crop-count BUCKET: the N crops of a batch are padded to the next multiple of ``bucket`` (16) with copies of
                crop 0, whose results are ignored) every ROI cut and resized -> model -> crop label images -> overlap test ->
                the crops' depth keys -> pinned host buffer
      host      paste order from the keys; renumbering + paste-back launches (eager: their shapes depend on N)

    ``run(batches)`` keeps TWO batches in flight (two slots, one stream each): while the host waits for one slot's statistics
    or keys, the GPU works on the other slot.  ``__call__(samples)`` runs one batch on slot 0.  A batch of raw camera frames
    (samples with "color" / "depth_raw" / "camera_params", see test_batch_crop_nolabel; channel order ``order`` and uint16 depth unit
    ``depth_scale`` are the pipeline's) is uploaded as it is and turned into the slot's input tensors by one eager launch in front
    of graph 1 (_ingest_raw).  Per frame the results are those
    of test_batch_crop_nolabel up to the batch-size dependence of the head's reduction orders (a padded second-stage batch is a
    different batch size: tests hold the pipeline to the same oracle bounds as the eager form).

    ``use_nms=True`` (the reference's configuration for real images, test_utils.py:30): the label images of both stages come from
    combine_masks_with_NMS_batched at ``nms_thresh`` -- fixed shapes, no host synchronisation, so the launches sit inside both graphs,
    each with a workspace of its own (one per slot, one per crop bucket).  The first stage's ``out_score`` (F,H,W), ``bbox`` (F,K,5) and
    ``count`` (F,) are reachable as ``pipeline.extras`` from the moment ``consume`` is called for a batch (tensors owned by the slot,
    valid until its next batch); ``run`` without a consumer clones them, one dict per batch, into ``pipeline.batch_extras``.

    The captured graphs follow the models' execution plans: a plan switch (set_precision, ...) or a parameter update of either model
    re-captures (graphs.StaleCheck, one per model).

    ``model_crop``: the second stage's own network (the reference's predictor_crop, test_utils.py:339-421: the published weights come
    as pairs); None = ``model``.  Both stages apply what their model's own ``forward`` applies in front of ``inference_images``
    (``model.input_spec()``: (x - pixel_mean) / pixel_std, zero padding of image and depth to the size divisibility, ``padded_size``)
    in ONE launch inside the stage's graph (ops.prepare_inputs, _prepared) -- the first stage on the frames, the second on the crops at
    ``crop_size`` -- and nothing at all for a model that neither normalises nor needs padding.  The slot's ``images`` / ``depths``
    stay the unpadded, un-normalised frames: the crops are cut from them (crop_rois, test_dataset.py:62-112), and every result is at
    the frame size.

    ``max_buckets=n``: a slot keeps at most n captured crop buckets; one more evicts the least recently replayed one (graph, table,
    host buffers, outputs, workspaces) after the slot's stream has been synchronised.  ``max_crops=m``: a batch with more than m ROIs
    captures nothing; its second stage runs eagerly on the slot's stream in unpadded chunks of at most m crops (the eager batch's
    ``crop_batch``).  None (the defaults) = no cap."""

    def __init__(self, model, frames, size, *, use_depth=True, topk=False, confident_score=0.7, low_threshold=0.4, num_class=2,
                 depth_threshold=0.5, bucket=16, crop_size=CROP_SIZE, slots=2, graphs=True, order="bgr", depth_scale=1000.0,
                 use_nms=False, nms_thresh=0.7, model_crop=None, max_buckets=None, max_crops=None):
        from .graphs import StaleCheck, _slot_stream
        self.use_nms, self.nms_thresh = bool(use_nms), float(nms_thresh)
        self.extras, self.batch_extras = None, []
        if order not in ("bgr", "rgb"):
            raise ValueError(f"order must be 'bgr' or 'rgb', got {order!r}")
        self.order, self.depth_scale = order, float(depth_scale)
        self.model = model
        self.frames, (self.H, self.W) = int(frames), (int(size[0]), int(size[1]))
        self.use_depth = bool(use_depth)
        self.kw = dict(topk=topk, confident_score=confident_score, low_threshold=low_threshold, num_class=num_class)
        self.depth_threshold = float(depth_threshold)
        self.bucket, self.crop_size, self.use_graphs = int(bucket), int(crop_size), bool(graphs)
        self.model_crop = model if model_crop is None else model_crop
        self._sig = StaleCheck(model)
        self._sig_crop = self._sig if self.model_crop is model else StaleCheck(self.model_crop)
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("BatchedTwoStage needs the model on the GPU (there is no CPU path)")
        if next(self.model_crop.parameters()).device != dev:
            raise ValueError(f"model_crop is on {next(self.model_crop.parameters()).device}, model on {dev}: both stages run on one device")
        if max_buckets is not None and int(max_buckets) < 1 or max_crops is not None and int(max_crops) < 1:
            raise ValueError(f"max_buckets / max_crops must be at least 1 (or None for no cap), got {max_buckets} / {max_crops}")
        self.max_buckets = None if max_buckets is None else int(max_buckets)
        self.max_crops = None if max_crops is None else int(max_crops)
        self.dev = dev
        self._slots = [self._new_slot(_slot_stream(dev, i)) for i in range(max(1, int(slots)))]

    # ---- slot state ----
    def _new_slot(self, stream):
        Fr, H, W, dev = self.frames, self.H, self.W, self.dev
        k = int(LABEL_BINS)
        with torch.cuda.stream(stream):
            st = dict(stream=stream, sig=None, g1=None, label=None, s2=self._new_buckets(stream), cur=None, nms_ws=None, prep=None, extras=None,
                      images=torch.zeros((Fr, 3, H, W), device=dev), depths=torch.zeros((Fr, 3, H, W), device=dev) if self.use_depth else None,
                      thr=torch.full((Fr, 1), self.depth_threshold, device=dev), thr_host=[self.depth_threshold] * Fr,
                      host_stats=torch.zeros(Fr * k * 5 + Fr, dtype=torch.int32).pin_memory(),
                      ev1=torch.cuda.Event(), ev2=torch.cuda.Event(), rows=None, n=0, nb=0)
        return st

    def _new_buckets(self, stream):
        """The crop buckets of a slot: crop count -> dict(g (the graph), refs, table, table_host, host_keys, out, nms_ws, prep).  An
        evicted bucket is dropped only after the slot's stream has run dry: no graph goes while it may still be running."""
        return LRUBuckets(self.max_buckets, lambda nb, b: stream.synchronize())

    def _prepared(self, owner, model, images, depths):
        """What ``model.forward`` applies in front of ``inference_images`` (model.input_spec()) -> (image, depth, image_size,
        padded_size or None).  A model that neither normalises nor needs padding at this size gets the tensors as they are: nothing
        is allocated, nothing is launched.  Otherwise ONE launch (ops.prepare_inputs) writes buffers that live in ``owner`` (the
        slot, or the slot's crop bucket, like nms_ws) so that a captured graph keeps writing the memory it was captured with."""
        spec = getattr(model, "input_spec", None)
        mean, std, div = (None, None, 1) if spec is None else spec()      # (any module with an inference_images of its own: as it is)
        H, W = (int(v) for v in images.shape[-2:])
        frame = (-(-H // div) * div, -(-W // div) * div)
        if mean is None and frame == (H, W):
            return images, depths, (H, W), None
        from . import ops
        bufs = owner.get("prep")
        if bufs is None:
            bufs = owner["prep"] = {}
        key = (tuple(images.shape), None if depths is None else tuple(depths.shape), frame)
        if key not in bufs:
            bufs[key] = tuple(None if t is None else torch.empty(tuple(t.shape[:2]) + frame, device=self.dev) for t in (images, depths))
        image, depth = ops.prepare_inputs(images, depths, mean=mean, std=std, frame=frame, out_image=bufs[key][0], out_depth=bufs[key][1])
        return image, depth, (H, W), frame

    def _predict(self, owner, model, images, depths):
        image, depth, size, padded = self._prepared(owner, model, images, depths)
        inputs = {"image": image}
        if depth is not None:
            inputs["depth"] = depth
        sc, cl, mk = (model.inference_images(inputs, size) if padded is None else model.inference_images(inputs, size, padded))[:3]
        return sc, cl, mk

    def _labels(self, owner, sc, cl, mk):
        """Label images of a stage -> (label, extras or None); with NMS the workspace lives in ``owner`` (the slot, or the slot's
        crop bucket) so that a captured graph keeps writing the memory it was captured with."""
        if not self.use_nms:
            return _label_image_batched(mk, instance_labels(sc, cl, **self.kw)), None
        from . import ops
        need = ops.mask_nms_workspace_bytes(*mk.shape)
        if owner.get("nms_ws") is None or owner["nms_ws"].numel() < need:
            owner["nms_ws"] = torch.empty(need, dtype=torch.uint8, device=self.dev)
        lab, score, bbox, count = combine_masks_with_NMS_batched(mk, sc, candidate_flags(sc, cl, **self.kw), self.nms_thresh, owner["nms_ws"])
        return lab, dict(out_score=score, bbox=bbox, count=count)

    def _stage1(self, st):
        sc, cl, mk = self._predict(st, self.model, st["images"], st["depths"])
        lab, st["extras"] = self._labels(st, sc, cl, mk)
        if st["depths"] is not None:
            lab = filter_labels_depth(lab, st["depths"], st["thr"])
        stats, _, overflow = label_stats(lab)
        st["host_stats"].copy_(torch.cat([stats.reshape(-1), overflow]), non_blocking=True)          # the batch's first transfer
        return lab

    def _stage2(self, st, b, chunk=None):
        """The second stage on the crops of bucket ``b``'s table, as one batch (the captured form) or, eagerly, ``chunk`` crops at a time
        through the network (_batch_crop's loop): everything around the network sees all the crops at once either way."""
        from . import ops
        rgb, msk, dep = ops.crop_resize(st["images"], st["depths"], st["label"], b["table"], self.crop_size)
        if chunk is None:
            sc, cl, mk = self._predict(b, self.model_crop, rgb, dep)
            labels_crop, _ = self._labels(b, sc, cl, mk)
        else:
            labels_crop = torch.empty((rgb.shape[0], self.crop_size, self.crop_size), device=self.dev)
            for c0 in range(0, rgb.shape[0], chunk):
                sc, cl, mk = self._predict(b, self.model_crop, rgb[c0:c0 + chunk], None if dep is None else dep[c0:c0 + chunk])
                labels_crop[c0:c0 + chunk] = self._labels(b, sc, cl, mk)[0]
        raw = labels_crop.clone()
        area, bad, lab, keys = _match_pre(labels_crop, msk, dep)
        if keys is not None:
            b["host_keys"].copy_(keys, non_blocking=True)                                             # the batch's second transfer
        return dict(rgb_crop=rgb, mask_crop=msk, depth_crop=dep, labels_crop=raw, area=area, bad=bad, lab=lab)

    def _capture(self, st, model, fn, *args):
        """Run fn twice (weight caches, MIOpen's solver choices), then capture it on the slot's stream -> (graph, fn's outputs, the
        cache references of ``model``, the one whose stage fn is)."""
        if not self.use_graphs:
            return None, fn(st, *args), None
        for _ in range(2):
            fn(st, *args)
        st["stream"].synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st["stream"]):
            out = fn(st, *args)
        from .graphs import cache_refs
        return g, out, cache_refs(model)                       # the derived tensors the graph reads by address stay alive with it

    def _ingest_raw(self, st, samples):
        """A batch of raw camera frames into the slot's static inputs (on the slot's stream): host frames go through the slot's pinned
        staging buffers and ONE asynchronous copy per array, 5 bytes per pixel instead of the 24 of the float tensors; then one
        eager launch of the ingest kernel writes st["images"] / st["depths"] -- the buffers the graphs read, so the graphs and their
        capture are as they were.  The staging buffers are allocated on the first raw batch (a float-only user never pays for them)."""
        from . import frames, ops
        Fr, H, W, dev = self.frames, self.H, self.W, self.dev
        cols = _raw_arrays(samples, "color", _RAW_COLOR, (H, W, 3))              # the frame size the pipeline was built for
        deps = _raw_arrays(samples, "depth_raw", _RAW_DEPTH, (H, W)) if st["depths"] is not None else None
        ddt = deps[0].dtype if deps else None
        r = st.get("raw")
        if r is None or r["ddt"] != ddt:
            r = dict(ddt=ddt, ev=torch.cuda.Event(), lut=frames._device_lut(dev, frames.PIXEL_MEANS),
                     color=torch.empty((Fr, H, W, 3), dtype=torch.uint8, device=dev),
                     color_host=torch.empty((Fr, H, W, 3), dtype=torch.uint8).pin_memory(), depth=None, depth_host=None, cam=None, cam_host=None)
            if ddt is not None:
                r.update(depth=torch.empty((Fr, H, W), dtype=ddt, device=dev), depth_host=torch.empty((Fr, H, W), dtype=ddt).pin_memory(),
                         cam=torch.empty((Fr, 4), device=dev), cam_host=torch.empty((Fr, 4)).pin_memory())
            st["raw"] = r
        r["ev"].synchronize()                                  # the previous batch's copies out of the pinned buffers are done
        for name, arrays in (("color", cols), ("depth", deps)):
            if arrays is None:
                continue
            if arrays[0].is_cuda:                              # frames that are on the device already: no staging
                torch.stack(arrays, out=r[name])
            else:
                torch.stack(arrays, out=r[name + "_host"])
                r[name].copy_(r[name + "_host"], non_blocking=True)
        if deps is not None:
            r["cam_host"].copy_(frames.camera_table([s["camera_params"] for s in samples], Fr))
            r["cam"].copy_(r["cam_host"], non_blocking=True)
        r["ev"].record(st["stream"])
        ops.ingest_frames(r["color"], r["depth"], r["cam"], r["lut"], depth_div=self.depth_scale, swap_rb=self.order == "rgb",
                          out_image=st["images"], out_depth=st["depths"])

    # ---- the phases of one batch on one slot (all device work on the slot's stream) ----
    @torch.no_grad()
    def _phase1(self, st, samples):
        if len(samples) != self.frames:
            raise ValueError(f"BatchedTwoStage was built for {self.frames} frames, got {len(samples)}")
        raw = _raw_batch(samples)
        sig = self._sig()
        sig = (sig, sig if self._sig_crop is self._sig else self._sig_crop())
        if st["sig"] != sig:                                   # first use, plan switch or parameter update of either model: re-capture everything
            st["stream"].synchronize()
            st.update(sig=sig, g1=None, s2=self._new_buckets(st["stream"]), cur=None, label=None, refs=None, nms_ws=None, prep=None, extras=None)
        with torch.cuda.stream(st["stream"]):
            st["stream"].wait_stream(torch.cuda.current_stream())
            if raw:
                self._ingest_raw(st, samples)
            else:
                torch.stack([s["image_color"][0] if s["image_color"].dim() == 4 else s["image_color"] for s in samples], out=st["images"])
            if st["depths"] is not None:
                if not raw:
                    torch.stack([s["depth"][0] if s["depth"].dim() == 4 else s["depth"] for s in samples], out=st["depths"])
                thr = [0.8 if "OSD" in str(s.get("file_name", "")) else self.depth_threshold for s in samples]      # test_utils.py:384-387
                if thr != st["thr_host"]:
                    st["thr"].copy_(torch.tensor(thr, dtype=torch.float32)[:, None])
                    st["thr_host"] = thr
            if st["label"] is None:
                st["g1"], st["label"], st["refs"] = self._capture(st, self.model, self._stage1)
                if st["g1"] is not None:
                    st["g1"].replay()
            elif st["g1"] is not None:
                st["g1"].replay()
            else:
                st["label"] = self._stage1(st)
            st["ev1"].record(st["stream"])

    @torch.no_grad()
    def _phase2(self, st):
        Fr, k = self.frames, int(LABEL_BINS)
        st["ev1"].synchronize()
        packed = st["host_stats"].numpy()
        rows = roi_table(packed[:Fr * k * 5].reshape(Fr, k, 5), packed[Fr * k * 5:], self.H, self.W)
        st["rows"], st["n"] = rows, len(rows)
        if not rows:
            return
        eager = self.max_crops is not None and len(rows) > self.max_crops
        nb = len(rows) if eager else -(-len(rows) // self.bucket) * self.bucket
        st["nb"] = nb
        with torch.cuda.stream(st["stream"]):
            b = None if eager else st["s2"].get(nb)            # (a hit makes the bucket the most recently replayed one)
            if b is None:
                b = dict(table=torch.zeros((nb, 8), dtype=torch.int32, device=self.dev),
                         table_host=torch.zeros((nb, 8), dtype=torch.int32).pin_memory(),
                         host_keys=torch.zeros(nb, dtype=torch.float64).pin_memory(), out=None, g=None, refs=None)
                if not eager:
                    st["s2"].put(nb, b)                        # one bucket more than max_buckets: the least recently replayed one goes first
            st["cur"] = b
            b["table_host"].copy_(torch.tensor(rows + [rows[0]] * (nb - len(rows)), dtype=torch.int32))
            b["table"].copy_(b["table_host"], non_blocking=True)
            if eager:                                          # more crops than max_crops: no bucket, no graph; chunks of max_crops, unpadded
                b["out"] = self._stage2(st, b, self.max_crops)
            elif b["out"] is None:
                b["g"], b["out"], b["refs"] = self._capture(st, self.model_crop, self._stage2, b)
                if b["g"] is not None:
                    b["g"].replay()
            elif b["g"] is not None:
                b["g"].replay()
            else:
                b["out"] = self._stage2(st, b)
            st["ev2"].record(st["stream"])

    @torch.no_grad()
    def _phase3(self, st, stages=None):
        """-> (out_label (F,H,W), refined (F,H,W), rows): tensors owned by the slot (valid until its next batch)."""
        label, rows, n = st["label"], st["rows"], st["n"]
        self.extras = st["extras"]
        if n == 0:
            return label, torch.zeros_like(label), rows
        st["ev2"].synchronize()
        b = st["cur"]
        o = b["out"]
        if self.use_depth:
            keys = b["host_keys"].numpy()[:n].tolist()
        else:
            keys = [float((r[5] - r[3] + 1) * (r[4] - r[2] + 1)) for r in rows]
        with torch.cuda.stream(st["stream"]):
            refined = _match_post(o["area"], o["bad"], o["lab"], keys, rows, self.frames, self.H, self.W, (self.crop_size, self.crop_size))
        torch.cuda.current_stream().wait_stream(st["stream"])
        if stages is not None:
            stages.update(rgb_crop=o["rgb_crop"][:n], mask_crop=o["mask_crop"][:n], depth_crop=None if o["depth_crop"] is None else o["depth_crop"][:n],
                          labels_crop=o["labels_crop"][:n].clone())
        return label, refined, rows

    def __call__(self, samples, stages=None):
        st = self._slots[0]
        self._phase1(st, samples)
        self._phase2(st)
        return self._phase3(st, stages)

    def run(self, batches, consume=None):
        """Every batch of ``batches`` (lists of ``frames`` samples) through the pipeline with two batches in flight.  ``consume(i,
        out_label, refined, rows)`` is called per batch while the slot still owns the tensors; without it the results are cloned
        into the returned list (and the first stage's NMS outputs, when use_nms, into ``batch_extras``)."""
        S = len(self._slots)
        results = [None] * len(batches)
        self.batch_extras = []

        def finish(i):
            out = self._phase3(self._slots[i % S])
            if consume is not None:
                consume(i, *out)
            else:
                results[i] = (out[0].clone(), out[1].clone(), out[2])
                self.extras = None if self.extras is None else {k: v.clone() for k, v in self.extras.items()}
                self.batch_extras.append(self.extras)

        for i, samples in enumerate(batches):
            if i >= 1:
                self._phase2(self._slots[(i - 1) % S])          # batch i-1's statistics -> its second stage is queued ...
            if i >= S:
                finish(i - S)                                   # ... before the host waits for batch i-S's keys (whose slot batch i reuses)
            self._phase1(self._slots[i % S], samples)
        if batches:
            self._phase2(self._slots[(len(batches) - 1) % S])
        for i in range(max(0, len(batches) - S), len(batches)):
            finish(i)
        return None if consume is not None else results


# ----------------------------------------------------------------------------------------------------------------------
# The UCN two-stage method (lib/fcn/test_dataset.py:232-267): what the seg_resnet34_8s_embedding checkpoints (checkpoint.py ->
# UCNBackbone) are for.  Embedding network -> vMF mean-shift clustering -> depth filter -> ROI crops -> the crop network on the
# 224 x 224 crops -> clustering of every crop -> paste back.  The second stage clusters one small map per object; on the device
# all of them go through ONE batched clustering (mean_shift.clustering_features -> mean_shift_smart_init_batched).
# ----------------------------------------------------------------------------------------------------------------------
def _cluster_fn(cluster, features, metric="cosine"):
    """A caller's ``cluster`` is used as it is; the default is mean_shift.clustering_features with ``metric`` bound."""
    if cluster is not None:
        return cluster
    if not features.is_cuda:
        raise RuntimeError("the clustering has no CPU path in unseenobjectswithmeanshift_amd: pass cluster= (e.g. the oracle's "
                           "clustering_features) for host tensors")
    from . import mean_shift
    if metric == "cosine":
        return mean_shift.clustering_features
    return functools.partial(mean_shift.clustering_features, metric=metric)


def _take_first(first_indices, k, what):
    if k >= len(first_indices):
        raise ValueError(f"first_indices holds {len(first_indices)} indices, {what} needs one more (the first stage's, then one per crop)")
    return int(first_indices[k])


def test_sample_clustering(sample, network, network_crop=None, *, num_seeds=100, depth_threshold=0.8, first_indices=None, cluster=None,
                           stages=None, metric="cosine"):
    """lib/fcn/test_dataset.py:232-267, step for step -> (out_label (1,H,W), out_label_refined (1,H,W) or None).
    sample: {"image_color" (1,3,H,W), "depth" (1,3,H,W) xyz (optional: no depth, no depth filter), "label" (optional)};
    ``network(image, label, depth)`` returns unit-norm embeddings (1,C,H,W), ``network_crop(rgb_crop, mask_crop, depth_crop)``
    (N,C,224,224).  ``first_indices``: the first seed index of the first stage's map, then one per crop in ascending label order,
    in place of the reference's np.random.randint draws (MS:155), which are made here, in that order, when it is None.
    ``cluster``: the clustering_features to use -- default mean_shift.clustering_features on device tensors (the crops in one batched
    call); host tensors (the CPU tests of this logic) must pass one, e.g. the oracle's.  ``stages``: a dict that receives the
    intermediate tensors (selected indices, ROIs, per-crop label images) -- for tests.  ``metric``: "cosine" or "euclidean"
    (cfg.TRAIN.EMBEDDING_METRIC; the networks then return un-normalised embeddings), forwarded to the default clustering; a
    caller's ``cluster`` is called as before."""
    image = sample["image_color"]
    depth = sample.get("depth")
    label = sample.get("label")
    H, W = image.shape[-2:]
    features = network(image, label, depth).detach()                                             # TD:247
    cluster = _cluster_fn(cluster, features, metric)
    first = np.random.randint(0, H * W) if first_indices is None else _take_first(first_indices, 0, "the first stage")
    out_label, selected_pixels = cluster(features, num_seeds=num_seeds, first_indices=[first])   # TD:248
    raw_label = out_label
    if depth is not None:
        out_label = filter_labels_depth(out_label, depth, depth_threshold)                       # TD:252
    out_label_refined = None
    if stages is not None:
        stages.update(label=raw_label, selected=selected_pixels, rois=None, labels_crop=None, selected_crop=[])
    if network_crop is not None:
        rgb_crop, out_label_crop, rois, depth_crop = crop_rois(image, out_label.clone(), depth)  # TD:257
        n = rgb_crop.shape[0]
        if n > 0:
            features_crop = network_crop(rgb_crop, out_label_crop, depth_crop).detach()          # TD:259
            hw = features_crop.shape[-2] * features_crop.shape[-1]
            firsts = [np.random.randint(0, hw) if first_indices is None else _take_first(first_indices, 1 + i, f"crop {i}") for i in range(n)]
            labels_crop, selected_crop = cluster(features_crop, num_seeds=num_seeds, first_indices=firsts)      # TD:260
            labels_crop = labels_crop.to(out_label.device)
            out_label_refined, labels_crop = match_label_crop(out_label, labels_crop, out_label_crop, rois, depth_crop)   # TD:261
            if stages is not None:
                stages.update(rois=rois, labels_crop=labels_crop, selected_crop=selected_crop)      # rejected segments are -1
    return out_label, out_label_refined


def test_batch_clustering(samples, network, network_crop=None, *, num_seeds=100, depth_threshold=0.8, first_indices=None, crop_batch=256,
                          cluster=None, stages=None, metric="cosine"):
    """test_sample_clustering for a list of F frames of one size -> (out_label (F,H,W), refined (F,H,W) or None, rows); frame f's
    results equal test_sample_clustering(samples[f], ...)[0][0] / [1][0] given the same first indices (the reference crops image 0
    of its batch only, so its batch is always 1: the semantics stay per frame).  ``rows`` is the ROI table (frame, label, x0, y0,
    x1, y1, 0, 0) of the second stage.
    The first stage clusters the F maps in one call (at 640 x 480 a map's workgroups fill more than half of the chip, so the
    grouped seeding carries one map per launch); the second stage cuts every ROI of every frame in one launch, runs ``network_crop``
    on ``crop_batch`` crops at a time, clusters ALL N crops of the batch in one batched call and pastes every frame in one launch.
    ``first_indices``: per frame the sequence test_sample_clustering takes (first stage, then the frame's crops); None draws them
    with np.random.randint -- the F first-stage indices, then the crops' in (frame, label) order.  ``metric`` as in
    test_sample_clustering."""
    Fr = len(samples)
    images = torch.stack([s["image_color"][0] if s["image_color"].dim() == 4 else s["image_color"] for s in samples]).float().contiguous()
    with_depth = [s.get("depth") is not None for s in samples]
    if any(with_depth) and not all(with_depth):
        raise ValueError("either every frame of a batch has \"depth\" or none")
    depths = None
    if Fr and with_depth[0]:
        depths = torch.stack([s["depth"][0] if s["depth"].dim() == 4 else s["depth"] for s in samples]).float().contiguous()
    labels = None
    if all("label" in s for s in samples):
        labels = torch.stack([torch.as_tensor(s["label"]).reshape(s["label"].shape[-2:]) for s in samples])
    _, _, H, W = images.shape
    features = network(images, labels, depths).detach()
    cluster = _cluster_fn(cluster, features, metric)
    if first_indices is not None and len(first_indices) != Fr:
        raise ValueError(f"first_indices must hold one sequence per frame ({Fr}), got {len(first_indices)}")
    firsts = [np.random.randint(0, H * W) if first_indices is None else _take_first(first_indices[f], 0, f"frame {f}'s first stage")
              for f in range(Fr)]
    out_label, selected_pixels = cluster(features, num_seeds=num_seeds, first_indices=firsts)
    if stages is not None:
        stages.update(label=out_label, selected=selected_pixels, labels_crop=None, selected_crop=[])
    if depths is not None:
        out_label = filter_labels_depth(out_label, depths, depth_threshold)
    if network_crop is None:
        return out_label, None, []
    stats, _, overflow = label_stats(out_label)
    packed = torch.cat([stats.reshape(-1), overflow]).cpu().numpy()                      # the batch's first transfer
    rows = roi_table(packed[:-Fr].reshape(Fr, -1, 5), packed[-Fr:], H, W)
    n = len(rows)
    if n == 0:
        return out_label, torch.zeros_like(out_label), rows
    rgb_crop, mask_crop, depth_crop = _crop_resize_batched(images, depths, out_label, rows, CROP_SIZE)
    # the N crop embeddings (12.8 MB each at 64 x 224 x 224) are the one buffer of size N: chunks are written into it as they come, and
    # the clustering transposes map_batch maps at a time (mean_shift.clustering_features)
    features_crop = None
    for c0 in range(0, n, crop_batch):
        part = network_crop(rgb_crop[c0:c0 + crop_batch], mask_crop[c0:c0 + crop_batch],
                            None if depth_crop is None else depth_crop[c0:c0 + crop_batch]).detach()
        if features_crop is None:
            features_crop = part if part.shape[0] == n else part.new_empty((n,) + tuple(part.shape[1:]))
        if features_crop is not part:
            features_crop[c0:c0 + part.shape[0]] = part
        del part
    hw = features_crop.shape[-2] * features_crop.shape[-1]
    seen = [0] * Fr
    crop_firsts = []
    for r in rows:                                                                       # (frame, ascending label) order
        seen[r[0]] += 1
        crop_firsts.append(np.random.randint(0, hw) if first_indices is None
                           else _take_first(first_indices[r[0]], seen[r[0]], f"frame {r[0]}'s crop {seen[r[0]] - 1}"))
    labels_crop, selected_crop = cluster(features_crop, num_seeds=num_seeds, first_indices=crop_firsts)      # ONE call for the N crops
    labels_crop = labels_crop.to(out_label.device)
    refined = match_label_crop_batched(out_label, labels_crop, mask_crop, rows, depth_crop)
    if stages is not None:
        stages.update(rgb_crop=rgb_crop, mask_crop=mask_crop, depth_crop=depth_crop, labels_crop=labels_crop, selected_crop=selected_crop)
    return out_label, refined, rows
