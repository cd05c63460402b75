"""Segmentation metrics of the labelled harness: own counterpart of the reference's lib/utils/evaluation.py.

  multilabel_metrics          <- evaluation.py:109-258 (overlap and boundary precision / recall / F-measure, share of objects
                                 found with F > 0.75), same ten keys, same values bit for bit
  munkres_assignment          <- the Munkres algorithm the reference runs on F.max() - F (lib/utils/munkres.py, evaluation.py:219-221)
  average_metrics             <- the per-key dataset mean of lib/fcn/test_utils.py:443-449
  multilabel_metrics_batched  a batch of label-image pairs: one launch sequence, one device -> host copy
  MetricsAccumulator          the same as the ``consume`` callback of two_stage.BatchedTwoStage.run

Every number the reference reports is float64 arithmetic on exact integer counts: label areas, the joint histogram, the
pixel counts of the seg2bmap boundary maps and the two true-positive counts of boundary_overlap per (gt label, predicted
label) pair.  Device tensors get those counts from one kernel pass per image pair (msm_eval_counts); host arrays from the
numpy restatement below (the same definitions, used by the unit tests without a GPU).  The float64 steps that follow run
in the reference's order, so the results equal the reference's exactly, nan included (a label covering the whole image has
no boundary pixel: Boundary Precision / Recall 0 / 0).

Differences on purpose:
  * label values must be integers in [0, 1024) (two_stage.LABEL_BINS); anything else raises ValueError (the reference
    accepts any value);
  * the reference does not run on numpy >= 1.24 (np.bool in seg2bmap) and needs cv2 / skimage; this module needs neither.
"""
import numpy as np
import torch

LABEL_BINS = 1024
BACKGROUND_LABEL = 0
OBJECTS_LABEL = 1
BOUND_TH = 0.003          # boundary_overlap's bound_th (evaluation.py:71)
FAST_LABELS = 64          # label capacity of the one-pass kernel path; more labels take one pass per pair of 64-label chunks

KEYS = ("Objects F-measure", "Objects Precision", "Objects Recall", "Boundary F-measure", "Boundary Precision",
        "Boundary Recall", "obj_detected", "obj_detected_075", "obj_gt", "obj_detected_075_percentage")


def bound_radius(H, W):
    """Disk radius of boundary_overlap: ceil(0.003 * |(H, W)|) -- 1 at 224x224, 3 at 480x640, 5 at 960x1280."""
    return int(np.ceil(BOUND_TH * np.linalg.norm((H, W))))


# ----------------------------------------------------------------------------------------------------------------------
# Munkres (Hungarian) assignment, step for step as the reference runs it, so that ties resolve the same way
# ----------------------------------------------------------------------------------------------------------------------
def munkres_assignment(cost):
    """Minimum-cost assignment of a (rows, cols) float64 cost matrix by the Munkres algorithm in its classic six-step form
    (Munkres 1957; Bourgeois & Lassalle 1971): the matrix is zero-padded to a square, rows are reduced by their minimum,
    zeros are starred greedily in row-major order, and the cover / prime / augmenting-path steps repeat until every row has a
    starred zero.  Zero tests are exact float64 comparisons.  The uncovered zero primed next is the LAST one in the FIRST row
    that has any; stars and primes along a path are found by the first match in their row or column.  Returns the starred
    (row, col) pairs inside the original shape in row-major order -- the assignment, ties included, of the reference's
    munkres.Munkres().compute."""
    cost = np.asarray(cost, dtype=np.float64)
    rows, cols = cost.shape
    n = max(rows, cols)
    C = np.zeros((n, n), dtype=np.float64)
    C[:rows, :cols] = cost
    C -= C.min(axis=1, keepdims=True)
    star = np.zeros((n, n), dtype=bool)
    row_cov = np.zeros(n, dtype=bool)
    col_cov = np.zeros(n, dtype=bool)
    for i, j in zip(*np.nonzero(C == 0)):
        if not row_cov[i] and not col_cov[j]:
            star[i, j] = row_cov[i] = col_cov[j] = True
    while True:
        row_cov[:] = False
        col_cov[:] = star.any(axis=0)
        if int(col_cov.sum()) >= n:
            break
        prime = np.zeros((n, n), dtype=bool)
        while True:
            free = (C == 0) & ~row_cov[:, None] & ~col_cov[None, :]
            hit = np.flatnonzero(free.any(axis=1))
            if hit.size == 0:
                # no uncovered zero: shift the smallest uncovered value (covered rows up, uncovered columns down, in that order)
                m = C[~row_cov][:, ~col_cov].min()
                C[row_cov, :] += m
                C[:, ~col_cov] -= m
                continue
            r = int(hit[0])
            c = int(np.flatnonzero(free[r])[-1])
            prime[r, c] = True
            s = np.flatnonzero(star[r])
            if s.size == 0:
                break
            row_cov[r] = True
            col_cov[s[0]] = False
        # augmenting path from the primed zero (r, c): star in its column, prime in that star's row, ...
        path = [(r, c)]
        while True:
            s = np.flatnonzero(star[:, path[-1][1]])
            if s.size == 0:
                break
            path.append((int(s[0]), path[-1][1]))
            path.append((path[-1][0], int(np.flatnonzero(prime[path[-1][0]])[0])))
        for i, j in path:
            star[i, j] = not star[i, j]
    return [(int(i), int(j)) for i, j in zip(*np.nonzero(star[:rows, :cols]))]


# ----------------------------------------------------------------------------------------------------------------------
# the integer counts: host restatement (numpy) and the device pass (msm_eval_counts)
# ----------------------------------------------------------------------------------------------------------------------
def _check_values(img, what):
    v = np.asarray(img)
    if v.dtype.kind == "f":
        bad = ~((v >= 0) & (v < LABEL_BINS) & (v == np.floor(v)))
    else:
        bad = (v < 0) | (v >= LABEL_BINS)
    nbad = int(bad.sum())
    if nbad:
        raise ValueError(f"{what} label values must be integers in [0, {LABEL_BINS}) ({nbad} pixels are not)")
    return v.astype(np.int64)


def _boundary_pairs(idx):
    """(flat pixel, dense label) pairs of the boundary maps seg2bmap(img == label) of every non-zero label, from the dense
    label index image idx (-1 = background): a pixel lies on the boundary of exactly the distinct labels of its 2x2 block
    (right / lower / lower-right; the last row only right, the last column only lower, the corner nothing) when that block
    is not uniform."""
    e, s, se = idx.copy(), idx.copy(), idx.copy()
    e[:, :-1] = idx[:, 1:]
    s[:-1, :] = idx[1:, :]
    se[:-1, :-1] = idx[1:, 1:]
    pix = np.flatnonzero((idx != e) | (idx != s) | (idx != se))
    members = [m.reshape(-1)[pix] for m in (idx, e, s, se)]
    P, L = [], []
    for k, m in enumerate(members):
        keep = m >= 0
        for prev in members[:k]:
            keep &= m != prev
        P.append(pix[keep])
        L.append(m[keep])
    return np.concatenate(P), np.concatenate(L)


def _disk(r):
    d = np.arange(-r, r + 1)
    dy, dx = np.meshgrid(d, d, indexing="ij")
    keep = dy * dy + dx * dx <= r * r
    return dy[keep], dx[keep]


def _dilated_matches(src_pix, src_lab, n_src, dst_pix, dst_lab, n_dst, H, W, r):
    """[i][j] = boundary pixels of dst label j within disk(r) of a boundary pixel of src label i (cv2.dilate with disk(r);
    pixels outside the image contribute nothing)."""
    out = np.zeros((n_src, n_dst), dtype=np.int64)
    dy, dx = _disk(r)
    for i in range(n_src):
        p = src_pix[src_lab == i]
        if p.size == 0:
            continue
        y = (p // W)[:, None] + dy[None, :]
        x = (p % W)[:, None] + dx[None, :]
        ok = (y >= 0) & (y < H) & (x >= 0) & (x < W)
        dil = np.zeros(H * W, dtype=bool)
        dil[(y * W + x)[ok]] = True
        out[i] = np.bincount(dst_lab[dil[dst_pix]], minlength=n_dst)
    return out


def host_counts(prediction, gt):
    """The integer counts of multilabel_metrics for one (H,W) pair of label images, in numpy: dict with the label values of
    each side (ascending, background excluded), their areas and boundary pixel counts, tp / fgm / gtm [gt label][pred label]
    and the non-zero pixel counts."""
    pred = _check_values(prediction, "prediction")
    g = _check_values(gt, "gt")
    if pred.shape != g.shape or pred.ndim != 2:
        raise ValueError(f"prediction {pred.shape} and gt {g.shape} must be the same (H,W)")
    H, W = g.shape
    r = bound_radius(H, W)
    out = {}
    idx = {}
    for side, img in (("gt", g), ("pred", pred)):
        area = np.bincount(img.reshape(-1), minlength=LABEL_BINS)
        labels = np.flatnonzero(area)
        labels = labels[labels != BACKGROUND_LABEL]
        lut = np.full(LABEL_BINS, -1, dtype=np.int64)
        lut[labels] = np.arange(labels.size)
        idx[side] = lut[img]
        out[f"labels_{side}"] = labels
        out[f"area_{side}"] = area[labels]
        out[f"nz_{side}"] = int(area[1:].sum())
    ng, np_ = out["labels_gt"].size, out["labels_pred"].size
    ig, ip = idx["gt"].reshape(-1), idx["pred"].reshape(-1)
    both = (ig >= 0) & (ip >= 0)
    out["tp"] = np.bincount(ig[both] * np_ + ip[both], minlength=ng * np_).reshape(ng, np_)
    gp, gl = _boundary_pairs(idx["gt"])
    pp, pl = _boundary_pairs(idx["pred"])
    out["bnd_gt"] = np.bincount(gl, minlength=ng)
    out["bnd_pred"] = np.bincount(pl, minlength=np_)
    out["fgm"] = _dilated_matches(gp, gl, ng, pp, pl, np_, H, W, r)
    out["gtm"] = _dilated_matches(pp, pl, np_, gp, gl, ng, H, W, r).T.copy()
    return out


def _decode_counts(row, L):
    """One image's row of msm_eval_counts (include/msm_hip.h) -> the host_counts dict."""
    ng, np_ = int(row[0]), int(row[1])
    if row[2] or row[3]:
        raise ValueError(f"label values must be integers in [0, {LABEL_BINS}) ({int(row[2])} gt and {int(row[3])} predicted pixels are not)")
    t = lambda k, n: row[8 + k * L: 8 + k * L + n].astype(np.int64)
    mat = lambda k: row[8 + 6 * L + k * L * L: 8 + 6 * L + (k + 1) * L * L].reshape(L, L)[:ng, :np_].astype(np.int64)
    return {"labels_gt": t(0, ng), "labels_pred": t(1, np_), "area_gt": t(2, ng), "area_pred": t(3, np_),
            "bnd_gt": t(4, ng), "bnd_pred": t(5, np_), "tp": mat(0), "fgm": mat(1), "gtm": mat(2),
            "nz_gt": int(row[4]), "nz_pred": int(row[5])}


def device_counts(prediction, gt, L=FAST_LABELS):
    """host_counts for (B,H,W) device tensors: one msm_eval_counts pass and ONE device -> host copy; frames with more than L
    labels on a side are counted again with the capacity they need (one pass per pair of 64-label chunks).
    Returns a list of B dicts."""
    from . import ops
    if prediction.dim() != 3 or prediction.shape != gt.shape:
        raise ValueError(f"prediction {tuple(prediction.shape)} and gt {tuple(gt.shape)} must be the same (B,H,W)")
    pred = prediction.float().contiguous()
    g = gt.to(pred.device).float().contiguous()
    B, H, W = pred.shape
    r = bound_radius(H, W)
    host = ops.eval_counts(pred, g, r, L).cpu().numpy()
    out = [None] * B
    for b in range(B):
        if host[b, 2] or host[b, 3]:
            _decode_counts(host[b], L)                                # raises
    need = max([max(int(host[b, 0]), int(host[b, 1])) for b in range(B)] + [0])
    if need > L:
        big = -(-need // 64) * 64
        over = [b for b in range(B) if max(int(host[b, 0]), int(host[b, 1])) > L]
        sel = torch.tensor(over, device=pred.device)
        host2 = ops.eval_counts(pred[sel].contiguous(), g[sel].contiguous(), r, big).cpu().numpy()
        for k, b in enumerate(over):
            out[b] = _decode_counts(host2[k], big)
    for b in range(B):
        if out[b] is None:
            out[b] = _decode_counts(host[b], L)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the reference's float64 arithmetic on the counts
# ----------------------------------------------------------------------------------------------------------------------
def _result(fm, p, r, bfm, bp, br, n_pred, n_det, n_gt, pct):
    return dict(zip(KEYS, (fm, p, r, bfm, bp, br, n_pred, n_det, n_gt, pct)))


def metrics_from_counts(c, obj_detect_threshold=0.75):
    """multilabel_metrics' dict from the integer counts (host_counts / device_counts), float64 steps in the reference's order."""
    num_labels_gt, num_labels_pred = int(c["labels_gt"].size), int(c["labels_pred"].size)
    if num_labels_pred == 0 and num_labels_gt > 0:           # all false negatives
        return _result(0., 1., 0., 0., 1., 0., num_labels_pred, 0., num_labels_gt, 0.)
    if num_labels_pred > 0 and num_labels_gt == 0:           # all false positives
        return _result(0., 0., 1., 0., 0., 1., num_labels_pred, 0., num_labels_gt, 0.)
    if num_labels_pred == 0 and num_labels_gt == 0:          # correctly predicted nothing
        return _result(1., 1., 1., 1., 1., 1., num_labels_pred, 0., num_labels_gt, 1.)
    tp = np.asarray(c["tp"], dtype=np.int64)
    prec = tp / np.asarray(c["area_pred"], dtype=np.int64)[None, :]
    rec = tp / np.asarray(c["area_gt"], dtype=np.int64)[:, None]
    F = np.zeros((num_labels_gt, num_labels_pred))
    pos = prec + rec > 0
    with np.errstate(invalid="ignore"):
        F[pos] = ((2 * prec * rec) / (prec + rec))[pos]
    true_positives = tp.astype(np.float64)
    boundary_stuff = np.stack([np.asarray(c["fgm"]), np.asarray(c["gtm"])], 2).astype(np.float64)
    boundary_prec_denom = 0.
    for v in np.asarray(c["bnd_pred"], dtype=np.int64):
        boundary_prec_denom += v
    boundary_rec_denom = 0.
    for v in np.asarray(c["bnd_gt"], dtype=np.int64):
        boundary_rec_denom += v
    F[np.isnan(F)] = 0
    assignments = munkres_assignment(F.max() - F.copy())
    num_obj_detected = 0
    for a in assignments:
        if F[a] > obj_detect_threshold:
            num_obj_detected += 1
    idx = tuple(np.array(assignments).T)
    with np.errstate(divide="ignore", invalid="ignore"):
        precision = np.sum(true_positives[idx]) / np.int64(c["nz_pred"])
        recall = np.sum(true_positives[idx]) / np.int64(c["nz_gt"])
        F_measure = (2 * precision * recall) / (precision + recall + 1e-10)
        if np.isnan(F_measure):
            F_measure = 0
        boundary_precision = np.sum(boundary_stuff[idx][:, 0]) / boundary_prec_denom
        boundary_recall = np.sum(boundary_stuff[idx][:, 1]) / boundary_rec_denom
        boundary_F_measure = (2 * boundary_precision * boundary_recall) / (boundary_precision + boundary_recall + 1e-10)
        if np.isnan(boundary_F_measure):
            boundary_F_measure = 0
    return _result(F_measure, precision, recall, boundary_F_measure, boundary_precision, boundary_recall,
                   num_labels_pred, num_obj_detected, num_labels_gt, num_obj_detected / num_labels_gt)


def _as_host(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy()
    return np.asarray(x)


def multilabel_metrics(prediction, gt, obj_detect_threshold=0.75):
    """lib/utils/evaluation.py:109-258 for one (H,W) pair of label images (numpy arrays or tensors, CPU or GPU; 0 =
    background, every other value an object).  Returns the reference's dict: Objects / Boundary F-measure, Precision and
    Recall, obj_detected, obj_detected_075, obj_gt, obj_detected_075_percentage.  If either input is a GPU tensor the
    counts come from the kernel pass, else from the host restatement; the values are the same."""
    dev = next((t.device for t in (prediction, gt) if isinstance(t, torch.Tensor) and t.is_cuda), None)
    if dev is not None:
        p = torch.as_tensor(prediction).to(dev)
        g = torch.as_tensor(gt).to(dev)
        if p.dim() != 2 or p.shape != g.shape:
            raise ValueError(f"prediction {tuple(p.shape)} and gt {tuple(g.shape)} must be the same (H,W)")
        c = device_counts(p[None], g[None])[0]
    else:
        c = host_counts(np.squeeze(_as_host(prediction)) if np.ndim(prediction) > 2 else _as_host(prediction),
                        np.squeeze(_as_host(gt)) if np.ndim(gt) > 2 else _as_host(gt))
    return metrics_from_counts(c, obj_detect_threshold)


def multilabel_metrics_batched(prediction, gt, obj_detect_threshold=0.75):
    """multilabel_metrics for every frame of (B,H,W) device tensors: one launch sequence and one device -> host copy of the
    count tables for the batch (a frame with more than 64 labels on a side is counted again with a larger table).
    Returns a list of B dicts."""
    return [metrics_from_counts(c, obj_detect_threshold) for c in device_counts(prediction, gt)]


def average_metrics(metrics_all):
    """The dataset means of lib/fcn/test_utils.py:443-449: per key, the sum over the list in order divided by its length."""
    result = {}
    num = len(metrics_all)
    for metrics in metrics_all:
        for k in metrics.keys():
            result[k] = result.get(k, 0) + metrics[k]
    for k in sorted(result.keys()):
        result[k] /= num
    return result


class MetricsAccumulator:
    """Metrics of the first-stage and the refined label images of every batch of two_stage.BatchedTwoStage.run, as its
    ``consume`` callback: ``run(batches, consume=acc)`` with ``acc = MetricsAccumulator(gts, pipeline)``, gts[i] the (F,H,W)
    ground-truth label images of batch i on the GPU.

    Per batch the two count passes are queued on the slot's stream while the slot still owns its tensors, followed by one
    asynchronous copy into pinned host memory; nothing waits.  The first stage is scored on the label images the pipeline
    hands over (after the depth filter); the second on the refined image of a frame with crops (``rows``), else on its
    first-stage image, as test_sample_crop does.  ``result()`` waits once, does the host step for every frame
    and returns (first_stage_mean, refined_mean) as average_metrics.  ``frames()`` gives the per-frame dicts.  The count
    tables hold ``max_labels`` labels per side (the pipeline's label images hold at most its detections per image); a frame
    with more raises in ``result()``."""

    def __init__(self, gts, pipeline=None, obj_detect_threshold=0.75, max_labels=FAST_LABELS):
        self.gts, self.pipeline = gts, pipeline
        self.thr, self.L = obj_detect_threshold, int(max_labels)
        self._pending = []

    def __call__(self, i, out_label, refined, rows=None):
        from . import ops
        stream = torch.cuda.current_stream(out_label.device)
        if self.pipeline is not None:
            slots = self.pipeline._slots
            stream = slots[i % len(slots)]["stream"]
        Fr, H, W = out_label.shape
        r = bound_radius(H, W)
        with torch.cuda.stream(stream):
            g = self.gts[i].to(out_label.device).float().contiguous()
            c1 = ops.eval_counts(out_label.float().contiguous(), g, r, self.L)
            second = refined.float()
            if rows is not None:
                cropped = torch.zeros(Fr, dtype=torch.bool)
                cropped[sorted({int(row[0]) for row in rows})] = True
                second = torch.where(cropped.to(out_label.device)[:, None, None], second, out_label.float())
            c2 = ops.eval_counts(second.contiguous(), g, r, self.L)
            host = torch.empty((2,) + tuple(c1.shape), dtype=torch.int32, pin_memory=True)
            host[0].copy_(c1, non_blocking=True)
            host[1].copy_(c2, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(stream)
        self._pending.append((i, host, ev))

    def frames(self):
        """[(batch index, frame, first-stage dict, refined dict), ...] in the order the batches were consumed."""
        out = []
        for i, host, ev in self._pending:
            ev.synchronize()
            h = host.numpy()
            for f in range(h.shape[1]):
                for t in (0, 1):
                    if max(int(h[t, f, 0]), int(h[t, f, 1])) > self.L:
                        raise RuntimeError(f"batch {i} frame {f} has more than max_labels={self.L} labels on a side: "
                                           "build the accumulator with a larger max_labels")
                out.append((i, f, metrics_from_counts(_decode_counts(h[0, f], self.L), self.thr),
                            metrics_from_counts(_decode_counts(h[1, f], self.L), self.thr)))
        return out

    def result(self):
        fr = self.frames()
        return average_metrics([m for _, _, m, _ in fr]), average_metrics([m for _, _, _, m in fr])
