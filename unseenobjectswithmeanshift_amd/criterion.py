"""The Mask2Former set criterion the reference fine-tunes with (MSMFormer/meanshiftformer/modeling/criterion.py, matcher.py),
with the point-sampled work on HIP kernels of libmsm_hip.so.

The reference, per prediction (final + every auxiliary one) and per image, samples the masks at random points, builds the
matching cost from about twenty small kernels, blocks on ``C.cpu()`` and solves the assignment; ``loss_masks`` then gathers
the matched masks, picks the most uncertain oversampled points with topk and samples again.  Here one criterion call is:

    1. every random point drawn first, in the reference's order (below)
    2. msm_match_cost: every cost matrix of every prediction, one launch
    3. one pinned device-to-host copy of all of them: the call's only sync
    4. the assignments (scipy.optimize.linear_sum_assignment, as the reference; a numpy solver when scipy is absent)
    5. msm_point_loss_fwd: loss_mask and loss_dice of every prediction (importance sampling included)
    6. loss_ce: torch's weighted cross entropy over the stacked logits (Q x (C+1) values per image: glue)

``loss_mask`` / ``loss_dice`` of all predictions are the outputs of one autograd Function whose backward is
msm_point_loss_bwd.

Random points.  The reference consumes the torch generator, on the predictions' device, in this order: for the final
prediction and then each ``aux_outputs[i]``: the matcher's ``torch.rand(1, P, 2)`` per image, then loss_masks'
``torch.rand(N, int(P * oversample_ratio), 2)`` and ``torch.rand(N, P - k, 2)`` with N = sum_b min(Q, T_b).  N does not
depend on the matching, so all draws are made up front, with the same shapes in the same order (not merged: that would move
the Philox offsets), and the same seed gives the reference's points.  A CPU ``generator`` draws on the CPU and copies.

Deviations: a batch without any target gives loss_mask = loss_dice = 0 with a zero gradient; all target masks of a batch must
share one size (the reference pads them to the largest, which moves the normalised points of the smaller ones);
``num_points <= 0`` raises (the reference computes nan costs).

``solver="device"`` (HungarianMatcher, build_criterion; the default is "host") replaces steps 3 and 4 by msm_lsap_match: the
assignments are solved on the device exactly as ``lsap_numpy`` solves them (scipy's on every matrix whose optimum is
unique), the kernel writes the pair table of step 5 and the target classes of step 6, and the call queues its launches
without ever waiting for the GPU (targets on the device; ``average_num_masks`` of a distributed run aside).  What the host
path raises at once, a nan / -inf or infeasible cost matrix, the device path records in ``last_status`` and reports only
when ``check_matching()`` is called; the losses of such a call are those of the fallback assignment (q = j, target j).
"""
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import ops

try:
    from scipy.optimize import linear_sum_assignment as _scipy_lsa
except ImportError:             # pragma: no cover - scipy is optional
    _scipy_lsa = None


# ----------------------------------------------------------------------------------------------------------------------------
# assignment
def lsap_numpy(cost):
    """Rectangular linear sum assignment by shortest augmenting paths (Crouse 2016, the algorithm behind scipy's
    linear_sum_assignment), iterating over the smaller side.  Returns (rows, cols) int64 arrays sorted by row."""
    cost = np.asarray(cost, dtype=np.float64)
    if cost.ndim != 2:
        raise ValueError("cost must be a matrix")
    if np.isnan(cost).any() or np.isneginf(cost).any():
        raise ValueError("cost matrix contains nan or -inf")
    transpose = cost.shape[1] < cost.shape[0]
    c = cost.T if transpose else cost
    nr, nc = c.shape
    if nr == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    u, v = np.zeros(nr), np.zeros(nc)
    col4row, row4col = np.full(nr, -1, np.int64), np.full(nc, -1, np.int64)
    for cur in range(nr):
        shortest = np.full(nc, np.inf)
        path = np.full(nc, -1, np.int64)
        seen_r, seen_c = np.zeros(nr, bool), np.zeros(nc, bool)
        min_val, i, sink = 0.0, cur, -1
        while sink < 0:
            seen_r[i] = True
            r = min_val + c[i] - u[i] - v
            upd = ~seen_c & (r < shortest)
            path[upd] = i
            shortest[upd] = r[upd]
            cand = np.flatnonzero(~seen_c)
            vals = shortest[cand]
            lowest = vals.min()
            if not np.isfinite(lowest):
                raise ValueError("cost matrix is infeasible")
            ties = cand[vals == lowest]
            free = ties[row4col[ties] < 0]
            j = int(free[0] if free.size else ties[0])
            min_val = lowest
            seen_c[j] = True
            if row4col[j] < 0:
                sink = j
            else:
                i = int(row4col[j])
        u[cur] += min_val
        rows = seen_r.copy()
        rows[cur] = False
        u[rows] += min_val - shortest[col4row[rows]]
        v[seen_c] -= min_val - shortest[seen_c]
        j = sink
        while True:
            i = int(path[j])
            row4col[j] = i
            col4row[i], j = j, int(col4row[i])
            if i == cur:
                break
    if transpose:
        order = np.argsort(col4row)
        return col4row[order].astype(np.int64), order.astype(np.int64)
    return np.arange(nr, dtype=np.int64), col4row.astype(np.int64)


def linear_sum_assignment(cost):
    """scipy.optimize.linear_sum_assignment when scipy imports (what the reference calls), else lsap_numpy."""
    if _scipy_lsa is not None:
        i, j = _scipy_lsa(cost)
        return np.asarray(i, np.int64), np.asarray(j, np.int64)
    return lsap_numpy(cost)


# ----------------------------------------------------------------------------------------------------------------------------
def indices_from_pairs(pairs_host, toff, Q, n_pred):
    """The pair table of one criterion call on the host, (n_pred * N, 4) integer rows (prediction, n, b * Q + q, target row),
    -> HungarianMatcher.solve's structure: per prediction, per image, the (i, j) int64 CPU tensors (queries, targets of the
    image).  N = sum_b min(Q, T_b) with T_b = toff[b + 1] - toff[b]; image b's rows of a prediction are its next min(Q, T_b)."""
    rows = torch.as_tensor(np.asarray(pairs_host), dtype=torch.int64).reshape(-1, 4)
    counts = [min(int(Q), int(b) - int(a)) for a, b in zip(toff, toff[1:])]
    N = sum(counts)
    if rows.shape[0] != n_pred * N:
        raise ValueError(f"indices_from_pairs: {rows.shape[0]} pairs, {n_pred} predictions x {N} expected")
    out = []
    for p in range(n_pred):
        per, at = [], p * N
        for b, n in enumerate(counts):
            part = rows[at:at + n]
            per.append(((part[:, 2] - b * int(Q)).clone(), (part[:, 3] - int(toff[b])).clone()))
            at += n
        out.append(per)
    return out


_STATUS_ERRORS = {1: (ValueError, "cost matrix contains nan or -inf"), 2: (ValueError, "cost matrix is infeasible"),
                  3: (RuntimeError, "msm_lsap_match hit a loop bound (a bug in the solver)")}


def average_num_masks(num_masks, device=None):
    """criterion.py:224-232: the number of target masks, all-reduced and divided by the world size when torch.distributed is
    initialised, clamped to at least 1, as a Python float (computed in float32 like the reference)."""
    import torch.distributed as dist
    n = torch.as_tensor([float(num_masks)], dtype=torch.float)
    world = 1
    if dist.is_available() and dist.is_initialized():
        if dist.get_backend() != "gloo" and device is not None:
            n = n.to(device)
        dist.all_reduce(n)
        world = dist.get_world_size()
    return torch.clamp(n / world, min=1).item()


class _Batch:
    """The targets of one call on the device: masks concatenated to (sum T, Hg, Wg) uint8, labels, per-image offsets."""

    def __init__(self, targets, device):
        self.T = [int(t["labels"].shape[0]) for t in targets]
        self.toff = [0]
        for n in self.T:
            self.toff.append(self.toff[-1] + n)
        sizes = {tuple(t["masks"].shape[-2:]) for t in targets if t["masks"].shape[0] > 0}
        if len(sizes) > 1:
            raise RuntimeError(f"SetCriterion: target masks of one batch must share one size, got {sorted(sizes)}")
        masks = []
        for t, n in zip(targets, self.T):
            m = t["masks"]
            if m.dim() != 3 or m.shape[0] != n:
                raise RuntimeError(f"SetCriterion: masks {tuple(m.shape)} do not match {n} labels")
            if n:
                masks.append(m.to(device=device, dtype=torch.uint8))
        hg, wg = sizes.pop() if sizes else (1, 1)
        self.masks = torch.cat(masks).contiguous() if masks else torch.zeros((0, hg, wg), device=device, dtype=torch.uint8)
        labels = [t["labels"].to(device=device, dtype=torch.int64) for t in targets]
        self.labels = torch.cat(labels) if labels else torch.zeros(0, device=device, dtype=torch.int64)
        self.labels32 = self.labels.to(torch.int32)


def _as_batch(targets, device, B):
    """The targets of one call as the kernels read them: a targets.TargetBatch is used as it is (its concatenated uint8 masks,
    labels and offsets: no torch.cat, no conversion), the reference's list goes through _Batch."""
    if not getattr(targets, "is_target_batch", False):
        return _Batch(targets, device)
    if len(targets.T) != B:
        raise RuntimeError(f"SetCriterion: a TargetBatch of {len(targets.T)} images for predictions of {B}")
    m = targets.masks
    if m.dtype != torch.uint8 or m.dim() != 3 or m.shape[0] != targets.toff[-1] or not m.is_contiguous():
        raise RuntimeError(f"SetCriterion: TargetBatch.masks must be contiguous ({targets.toff[-1]}, Hg, Wg) uint8, got "
                           f"{tuple(m.shape)} {m.dtype}")
    if m.device != torch.device(device) or targets.labels32.device != m.device:
        raise RuntimeError(f"SetCriterion: the TargetBatch lives on {m.device}, the predictions on {device}: build it from device "
                           "label images (there is no copy behind the caller's back)")
    return targets


def _rand_into(out, generator):
    """torch.rand(out.shape) from `generator` (None: the default generator of out's device) into out, as one draw."""
    if generator is None or generator.device == out.device:
        torch.rand(out.shape, generator=generator, out=out)
    else:
        out.copy_(torch.rand(out.shape, generator=generator, device=generator.device))


def _preds(outputs):
    main = {k: v for k, v in outputs.items() if k != "aux_outputs"}
    return [main] + list(outputs.get("aux_outputs", []))


class HungarianMatcher(nn.Module):
    """matcher.py:67-188 on msm_match_cost: the costs of all images (and, inside SetCriterion, all predictions) in one launch,
    one device-to-host copy, then the assignment per image.  solver="device": the assignments by msm_lsap_match, no copy and
    no wait; forward then returns the (i, j) pairs as device tensors (a bad cost matrix gives the fallback pairs, see
    ops.lsap_match; `last_status` holds the statuses)."""

    def __init__(self, cost_class: float = 1, cost_mask: float = 1, cost_dice: float = 1, num_points: int = 0, generator=None,
                 solver: str = "host"):
        super().__init__()
        self.cost_class = cost_class
        self.cost_mask = cost_mask
        self.cost_dice = cost_dice
        assert cost_class != 0 or cost_mask != 0 or cost_dice != 0, "all costs cant be 0"
        self.num_points = num_points
        self.generator = generator
        if solver not in ("host", "device"):
            raise ValueError(f"HungarianMatcher: solver must be 'host' or 'device', got {solver!r}")
        self.solver = solver
        self.last_status = None

    def _check(self):
        if int(self.num_points) <= 0:
            raise ValueError(f"HungarianMatcher: num_points must be positive (got {self.num_points}); the reference gives nan costs")

    def draw_points(self, out):
        """The matcher's draws for one prediction into out (B, P, 2): one torch.rand(1, P, 2) per image (matcher.py:124)."""
        for b in range(out.shape[0]):
            _rand_into(out[b:b + 1], self.generator)

    def costs(self, preds, batch, points):
        """Device cost matrices (n_pred, Q, sum T) of every prediction in `preds` at `points` (n_pred, B, P, 2)."""
        return ops.match_cost([p["pred_logits"].float().contiguous() for p in preds],
                              [p["pred_masks"].float().contiguous() for p in preds], batch.masks, batch.labels32, batch.toff,
                              points, self.cost_class, self.cost_mask, self.cost_dice)

    @staticmethod
    def solve(cost_host, toff):
        """cost_host (n_pred, Q, sum T) on the host -> per prediction the reference's list of (i, j) int64 CPU tensor pairs."""
        c = cost_host.numpy()
        out = []
        for p in range(c.shape[0]):
            per = []
            for b in range(len(toff) - 1):
                i, j = linear_sum_assignment(c[p, :, toff[b]:toff[b + 1]])
                per.append((torch.as_tensor(i, dtype=torch.int64), torch.as_tensor(j, dtype=torch.int64)))
            out.append(per)
        return out

    @staticmethod
    def fetch(cost):
        """The one device-to-host copy (pinned) and its wait."""
        host = torch.empty(cost.shape, dtype=cost.dtype, pin_memory=True)
        host.copy_(cost, non_blocking=True)
        torch.cuda.current_stream(cost.device).synchronize()
        return host

    @staticmethod
    def solve_device(cost, batch, no_object):
        """cost (n_pred, Q, sum T) on the device -> ops.lsap_match's (pairs, target_classes, status); nothing waits."""
        return ops.lsap_match(cost, batch.toff, batch.labels32, no_object)

    @torch.no_grad()
    def memory_efficient_forward(self, outputs, targets):
        self._check()
        dev = outputs["pred_masks"].device
        B, Q = outputs["pred_logits"].shape[:2]
        batch = _as_batch(targets, dev, B)
        pts = torch.empty((1, B, int(self.num_points), 2), device=dev, dtype=torch.float32)
        self.draw_points(pts[0])
        cost = self.costs([outputs], batch, pts)
        if self.solver == "host":
            return self.solve(self.fetch(cost), batch.toff)[0]
        pairs, _, self.last_status = self.solve_device(cost, batch, 0)
        out, at = [], 0
        for b, t in enumerate(batch.T):                 # host-known counts: slices, no sync
            part = pairs[at:at + min(Q, t)].to(torch.int64)
            out.append((part[:, 2] - b * Q, part[:, 3] - batch.toff[b]))
            at += min(Q, t)
        return out

    @torch.no_grad()
    def forward(self, outputs, targets):
        return self.memory_efficient_forward(outputs, targets)

    def __repr__(self, _repr_indent=4):
        head = "Matcher " + self.__class__.__name__
        body = [f"cost_class: {self.cost_class}", f"cost_mask: {self.cost_mask}", f"cost_dice: {self.cost_dice}"]
        return "\n".join([head] + [" " * _repr_indent + line for line in body])


class _PointLosses(torch.autograd.Function):
    """(pred_masks of every prediction) -> (2, n_pred): loss_mask and loss_dice rows.  Forward msm_point_loss_fwd, backward
    msm_point_loss_bwd; `state` carries the targets, pairs, points and num_masks."""

    @staticmethod
    def forward(ctx, state, *masks):
        losses, bits, ws = ops.point_loss_fwd(list(masks), state["tgt"], state["pairs"], state["os"], state["rnd"], state["k"],
                                              state["num_masks"])
        state["sel_bits"] = bits
        ctx.state, ctx.ws = state, ws
        ctx.save_for_backward(*masks)
        return losses

    @staticmethod
    def backward(ctx, g):
        s = ctx.state
        grads = ops.point_loss_bwd(list(ctx.saved_tensors), s["tgt"], s["pairs"], s["os"], s["rnd"], ctx.ws,
                                   g.float().contiguous(), s["k"], s["num_masks"])
        return (None, *grads)


class SetCriterion(nn.Module):
    """criterion.py:90-247: Hungarian matching, then the classification loss and the point-sampled sigmoid-CE and dice mask
    losses for the final prediction and every auxiliary one.  forward(outputs, targets) -> the reference's dict of
    UNWEIGHTED losses (loss_ce, loss_mask, loss_dice, then the same with _i for aux_outputs[i]).  ``targets`` is the reference's
    list of {"labels", "masks"} or a targets.TargetBatch; the latter is read in place (its concatenated uint8 masks, int32 labels
    and offsets: no torch.cat, no conversion), here and in HungarianMatcher.forward.

    After a call, ``last_indices`` holds the assignments per prediction, ``last_points`` the draws (draw_points) and
    ``last_selection`` the importance-sampling selection bitmaps (n_pred * N, ceil(Pos / 32)) int32 (bit i % 32 of word
    i / 32: oversampled point i).

    With a ``solver="device"`` matcher the call waits for nothing: ``last_indices`` is then built on first access (one copy
    of the pair table and one sync, then the same lists of CPU tensor pairs), ``last_status`` is the device tensor
    (n_pred, B) of msm_lsap_match's statuses, and a bad cost matrix is reported only by ``check_matching()``; until then the
    losses of that call are those of the fallback assignment."""

    def __init__(self, num_classes, matcher, weight_dict, eos_coef, losses, num_points, oversample_ratio, importance_sample_ratio,
                 generator=None):
        super().__init__()
        self.num_classes = num_classes
        self.matcher = matcher
        self.weight_dict = weight_dict
        self.eos_coef = eos_coef
        self.losses = losses
        empty_weight = torch.ones(self.num_classes + 1)
        empty_weight[-1] = self.eos_coef
        self.register_buffer("empty_weight", empty_weight)
        self.num_points = num_points
        self.oversample_ratio = oversample_ratio
        self.importance_sample_ratio = importance_sample_ratio
        self.generator = generator
        self.last_indices = None
        self.last_points = None
        self.last_selection = None
        self.last_status = None

    @property
    def last_indices(self):
        if self._last_indices is None and self._last_pairs is not None:
            pairs, toff, Q, n_pred = self._last_pairs
            self._last_indices = indices_from_pairs(pairs.cpu().numpy(), toff, Q, n_pred)      # the copy and its sync
        return self._last_indices

    @last_indices.setter
    def last_indices(self, value):
        self._last_indices, self._last_pairs = value, None

    def check_matching(self):
        """Raise what the host solver would have raised during the last call: ValueError for a cost matrix with nan / -inf or
        an infeasible one, RuntimeError if the device solver hit a loop bound.  Synchronises (it reads ``last_status``);
        a no-op after a host-solver call, which raises at once."""
        if self.last_status is None:
            return
        st = self.last_status.cpu()
        bad = st.nonzero()
        if bad.shape[0]:
            p, b = (int(v) for v in bad[0])
            err, msg = _STATUS_ERRORS.get(int(st[p, b]), (RuntimeError, f"unknown status {int(st[p, b])}"))
            raise err(f"{msg} (prediction {p}, image {b})")

    def point_counts(self):
        """(P, Pos, k): points per mask, oversampled points, importance-sampled points (point_features.py's arithmetic)."""
        assert self.oversample_ratio >= 1
        assert 0 <= self.importance_sample_ratio <= 1
        P = int(self.num_points)
        if P <= 0:
            raise ValueError(f"SetCriterion: num_points must be positive, got {P}")
        return P, int(P * self.oversample_ratio), int(self.importance_sample_ratio * P)

    def draw_points(self, n_pred, B, N, device):
        """Every random draw of one call in the reference's order -> (matcher points (n_pred, B, Pm, 2), oversampled points
        (n_pred, N, Pos, 2) or None, uniform points (n_pred, N, P - k, 2) or None)."""
        self.matcher._check()
        want_masks = "masks" in self.losses
        Pm = int(self.matcher.num_points)
        mp = torch.empty((n_pred, B, Pm, 2), device=device, dtype=torch.float32)
        os_ = rnd = None
        if want_masks:
            P, Pos, k = self.point_counts()
            os_ = torch.empty((n_pred, N, Pos, 2), device=device, dtype=torch.float32)
            rnd = torch.empty((n_pred, N, P - k, 2), device=device, dtype=torch.float32)
        for p in range(n_pred):
            self.matcher.draw_points(mp[p])
            if want_masks:
                _rand_into(os_[p], self.generator)
                if P - k > 0:
                    _rand_into(rnd[p], self.generator)
        return mp, os_, rnd

    def forward(self, outputs, targets):
        for loss in self.losses:
            assert loss in ("labels", "masks"), f"do you really want to compute {loss} loss?"
        preds = _preds(outputs)
        n_pred = len(preds)
        logits0 = preds[0]["pred_logits"]
        dev = preds[0]["pred_masks"].device
        B, Q = logits0.shape[:2]
        batch = _as_batch(targets, dev, B)
        N = sum(min(Q, t) for t in batch.T)
        mp, os_, rnd = self.draw_points(n_pred, B, N, dev)
        self.last_points = (mp, os_, rnd)
        with torch.no_grad():
            cost = self.matcher.costs(preds, batch, mp)
        device_solver = getattr(self.matcher, "solver", "host") == "device"
        if device_solver:
            # pairs and target classes straight from msm_lsap_match: no copy, no wait, no Python lists
            with torch.no_grad():
                pairs_t, target_classes, self.last_status = self.matcher.solve_device(cost, batch, self.num_classes)
            self.last_indices = None
            self._last_pairs = (pairs_t, list(batch.toff), Q, n_pred)
        else:
            indices = self.matcher.solve(self.matcher.fetch(cost), batch.toff)
            self.last_indices = indices
            self.last_status = None
            # the matched pairs (b, q, target row) of each prediction in the reference's order (images in order, q ascending)
            per_pred = [[(b, i, batch.toff[b] + j) for b, (I, J) in enumerate(indices[p]) for i, j in zip(I.tolist(), J.tolist())]
                        for p in range(n_pred)]
        num_masks = average_num_masks(sum(batch.T), dev)

        parts = [dict() for _ in range(n_pred)]
        if "labels" in self.losses:
            if not device_solver:
                flat, tgt = [], []
                for p, rows in enumerate(per_pred):
                    flat += [(p * B + b) * Q + q for b, q, _ in rows]
                    tgt += [t for _, _, t in rows]
                target_classes = torch.full((n_pred * B * Q,), self.num_classes, dtype=torch.int64, device=dev)
                if flat:
                    fi = torch.tensor(flat, dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
                    tj = torch.tensor(tgt, dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
                    target_classes[fi] = batch.labels[tj]
            logits = torch.stack([p["pred_logits"].float() for p in preds])                       # (n_pred, B, Q, C+1)
            C1 = logits.shape[-1]
            w = self.empty_weight.to(dev, non_blocking=True)
            target_classes = target_classes.view(n_pred * B, Q)
            nll = F.cross_entropy(logits.view(n_pred * B, Q, C1).transpose(1, 2), target_classes, w, reduction="none")
            loss_ce = nll.view(n_pred, B * Q).sum(1) / w[target_classes].view(n_pred, B * Q).sum(1)
            for p, v in enumerate(loss_ce.unbind(0)):              # unbind: one stack in the backward, not a copy per loss
                parts[p]["loss_ce"] = v
        if "masks" in self.losses:
            P, Pos, k = self.point_counts()
            if not device_solver:
                pairs = [(p, n, b * Q + q, t) for p, rows in enumerate(per_pred) for n, (b, q, t) in enumerate(rows)]
                pairs_t = torch.tensor(pairs, dtype=torch.int32).reshape(-1, 4).pin_memory().to(dev, non_blocking=True)
            state = {"tgt": batch.masks, "pairs": pairs_t, "os": os_, "rnd": rnd, "k": k, "num_masks": num_masks}
            masks = [p["pred_masks"].float().contiguous() for p in preds]
            lm = _PointLosses.apply(state, *masks)
            self.last_selection = state.get("sel_bits")
            for p, (vm, vd) in enumerate(zip(*(row.unbind(0) for row in lm.unbind(0)))):
                parts[p]["loss_mask"] = vm
                parts[p]["loss_dice"] = vd
        losses = {}
        for p in range(n_pred):
            sfx = "" if p == 0 else f"_{p - 1}"
            for key in ("loss_ce", "loss_mask", "loss_dice"):
                if key in parts[p]:
                    losses[key + sfx] = parts[p][key]
        return losses

    def __repr__(self):
        head = "Criterion " + self.__class__.__name__
        body = [
            "matcher: {}".format(self.matcher.__repr__(_repr_indent=8)),
            f"losses: {self.losses}", f"weight_dict: {self.weight_dict}", f"num_classes: {self.num_classes}",
            f"eos_coef: {self.eos_coef}", f"num_points: {self.num_points}", f"oversample_ratio: {self.oversample_ratio}",
            f"importance_sample_ratio: {self.importance_sample_ratio}",
        ]
        return "\n".join([head] + [" " * 4 + line for line in body])


def build_weight_dict(class_weight, mask_weight, dice_weight, dec_layers, deep_supervision=True):
    """meanshiftformer_model.py:157-164.  dec_layers is the config's DEC_LAYERS (decoder layers + 1): aux keys _0 .. _{DEC_LAYERS-2}."""
    weight_dict = {"loss_ce": class_weight, "loss_mask": mask_weight, "loss_dice": dice_weight}
    if deep_supervision:
        aux = {}
        for i in range(dec_layers - 1):
            aux.update({k + f"_{i}": v for k, v in weight_dict.items()})
        weight_dict.update(aux)
    return weight_dict


def build_criterion(num_classes, *, class_weight, mask_weight, dice_weight, no_object_weight, dec_layers, deep_supervision=True,
                    train_num_points=12544, oversample_ratio=3.0, importance_sample_ratio=0.75, generator=None, solver="host"):
    """SetCriterion as meanshiftformer_model.py:134-176 builds it from the config (MODEL.MASK_FORMER.*).  solver: "host" (the
    assignments by scipy after one device-to-host copy) or "device" (msm_lsap_match, no wait; see SetCriterion)."""
    matcher = HungarianMatcher(cost_class=class_weight, cost_mask=mask_weight, cost_dice=dice_weight, num_points=train_num_points,
                               generator=generator, solver=solver)
    return SetCriterion(num_classes, matcher=matcher,
                        weight_dict=build_weight_dict(class_weight, mask_weight, dice_weight, dec_layers, deep_supervision),
                        eos_coef=no_object_weight, losses=["labels", "masks"], num_points=train_num_points,
                        oversample_ratio=oversample_ratio, importance_sample_ratio=importance_sample_ratio, generator=generator)
