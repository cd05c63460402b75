"""From instance label images to the training targets: the label half of "a batch of raw frames in, a loss dict out".

Own counterpart of what the reference builds per image on the host, same names where it has them:

  process_label_to_annos  <- TableTopDataset.process_label_to_annos, lib/datasets/tabletop_dataset.py:183-216
  process_label           <- TableTopDataset.process_label, :218-232
  sample_pixels           <- TableTopDataset.sample_pixels, :303-316
  instance_targets        <- __getitem__ :330-337,361-362,376-389 (table -> background, the three methods, "category_id": 1),
                             TabletopDatasetMapper.__call__ lib/datasets/tablet_instance_mapper.py:140-175 (masks and classes per
                             image) and prepare_targets / ImageList.from_tensors of the label map,
                             MSMFormer/meanshiftformer/pretrained_meanshiftformer_model.py:319-321,380-395 (zero padding)
  training_batch          <- frames.ingest + instance_targets: the arguments of training.ucn_model_losses; with ``crop=`` the
                             TRAIN.SYN_CROP path of __getitem__ :354-358 in between (crops.py)

Definitions (every value an integer or an exact 0 / 1), per image of ``raw`` (B,H,W) uint8 or int32, ids in [0, 1024):

  1. fold      lab = 0 where raw is one of ``background_ids`` (default (0, 1): the table, id 1, is background,
               tabletop_dataset.py:335), else raw.  Pixels outside [0, 1024) are counted; check() raises on them.
  2. present   the distinct values of lab, ascending (0 included when it occurs): K values.
  3. instances present without a leading 0: T ids.  Instance t has the mask lab == id_t, the tight inclusive box (x_min, y_min,
               x_max, y_max) float32 and the class ``class_id`` (the record's "category_id": 1 is what the mapper turns into
               gt_classes; the clip(1, 2) that process_label_to_annos itself returns is dropped by __getitem__).  Background
               only: T = 0.
  4. dense     dense[y][x] = position of lab[y][x] in present.  Without any background pixel the lowest id gets dense label 0
               and still is instance 0, as in the reference.
  5. sampled   (optional) sample_pixels(dense, num) with caller-drawn int32 ``keys``: per image and dense label with n pixels,
               n <= num keeps all, else the num pixels smallest in the order (key, flat index y W + x) stay and the others
               become -1: a pure function of (dense, keys, num); with independent uniform keys a uniformly random subset,
               which is what the reference's permutation(n)[:num] draws.
  6. padding   masks and label map at (Hp, Wp) = (H, W) rounded up to ``size_divisibility``, zeros at the right / bottom; the
               label map pads with 0, not -1 (the reference pads after sampling with pad_value 0).
  7. layout    masks (TT,Hp,Wp) uint8 with TT = sum T_b, image b at rows toff[b] .. toff[b + 1]: the ``tgt`` operand of
               msm_match_cost / msm_point_loss_*.

Like frames and two_stage, the functions follow their data: device tensors go through the HIP kernels (ops.target_tables,
ops.target_write, ops.sample_labels_: three entry points for a whole batch, 1 byte per pixel uploaded instead of T float masks);
host tensors and numpy arrays -- the unit tests of the logic without a GPU -- through the same definitions in numpy.  There is
no fallback on a device tensor.
"""
import numpy as np
import torch

from . import frames

BACKGROUND_IDS = (0, 1)      # tabletop_dataset.py:335: the table (1) is background
LABEL_BINS = 1024            # ids in [0, 1024): the convention of msm_label_stats / msm_eval_counts
SAMPLE_MAX_LABELS = 256      # dense labels per image the sampler handles


# ----------------------------------------------------------------------------------------------------------------------------
# the definitions in numpy (host tensors / arrays)
def _fold_host(raw, background_ids):
    lab = raw.astype(np.int64)
    bad = ((lab < 0) | (lab >= LABEL_BINS)).reshape(lab.shape[0], -1).sum(1)
    lab[np.isin(lab, np.asarray(background_ids, dtype=np.int64).reshape(-1))] = 0
    return lab, bad


def _image_tables_host(lab):
    """One folded image (out-of-range pixels belong to nothing) -> (present values, instance ids, dense labels)."""
    ok = (lab >= 0) & (lab < LABEL_BINS)
    present = np.unique(lab[ok])
    ids = present[1:] if present.size and present[0] == 0 else present
    dense = np.searchsorted(present, np.where(ok, lab, present[0] if present.size else 0))
    return present, ids, np.where(ok, dense, 0)


def _box_host(mask):
    ys, xs = np.nonzero(mask)
    return xs.min(), ys.min(), xs.max(), ys.max()


def _sample_host(dense, keys, num):
    """dense, keys (B,H,W) -> the sampled labels of definition 5 (int64)."""
    out = np.full(dense.shape, -1, dtype=np.int64)
    B = dense.shape[0]
    flat, kflat, oflat = dense.reshape(B, -1), keys.reshape(B, -1), out.reshape(B, -1)
    for b in range(B):
        for i in np.unique(flat[b]):
            if i < 0:
                continue
            idx = np.flatnonzero(flat[b] == i)
            if idx.size > num:
                idx = idx[np.lexsort((idx, kflat[b][idx]))[:num]]
            oflat[b][idx] = i
    return out


def draw_keys(shape, device="cpu", generator=None):
    """The sampler's keys: int32 uniform on [0, 2^31 - 1) of ``shape`` on ``device`` (from ``generator``; one on another
    device draws there and copies)."""
    dev = torch.device(device)
    if generator is not None and generator.device.type != dev.type:
        return torch.randint(0, 2 ** 31 - 1, tuple(shape), dtype=torch.int32, generator=generator, device=generator.device).to(dev)
    return torch.randint(0, 2 ** 31 - 1, tuple(shape), dtype=torch.int32, generator=generator, device=dev)


# ----------------------------------------------------------------------------------------------------------------------------
def _is_device(x):
    return isinstance(x, torch.Tensor) and x.is_cuda


def _host(x):
    return x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _raw_device(raw):
    """A device label image as the kernels take it: uint8 stays, every other integer type becomes int32."""
    if raw.dtype == torch.uint8:
        return raw.contiguous()
    if raw.dtype.is_floating_point or raw.dtype == torch.bool:
        raise TypeError(f"label images must hold integers, got {raw.dtype}")
    return raw.to(torch.int32).contiguous()


def _check_host_ints(a, who):
    if a.dtype.kind not in "iu":
        raise TypeError(f"{who}: label images must hold integers, got {a.dtype}")


_BG_DEVICE = {}


def _device_background(dev, background_ids):
    ids = tuple(int(v) for v in background_ids)
    if len(ids) > 16:
        raise ValueError("background_ids: at most 16 ids")
    key = (str(dev), ids)
    if key not in _BG_DEVICE:
        _BG_DEVICE[key] = torch.tensor(ids, dtype=torch.int32).to(dev) if ids else None
    return _BG_DEVICE[key]


class TargetBatch:
    """The targets of a batch, in the layout the criterion kernels read:

      masks    (TT,Hp,Wp) uint8 0 / 1, image b at rows toff[b] .. toff[b + 1]      labels   (TT,) int64 classes (labels32: int32)
      boxes    (TT,4) float32 x_min, y_min, x_max, y_max (inclusive)                ids      (TT,) int32 instance ids
      areas    (TT,) int32 pixels per instance                                      label    (B,1,Hp,Wp) dense (or sampled) label map
      counts / T   the host's T_b per image, toff their running sum                targets  the reference's list of {"labels", "masks"}
                                                                                             (bool views of ``masks``, no copy)

    SetCriterion / HungarianMatcher take it in place of ``targets`` and then use masks, labels32 and toff as they are.
    check() raises what the device recorded: ids outside [0, 1024), ``counts=`` that disagree with the images, labels the
    sampler does not handle.  It synchronises; instance_targets itself does not when ``counts`` is given."""

    is_target_batch = True
    crop_boxes = None            # training_batch(..., crop=): the (B, 8) int32 box rows of crops.crop_boxes

    def __init__(self, masks, labels, boxes, ids, areas, label, counts, image_size, status=None, sample_status=None):
        self.masks, self.labels, self.boxes, self.ids, self.areas, self.label = masks, labels, boxes, ids, areas, label
        self.labels32 = labels.to(torch.int32)
        self.counts = [int(c) for c in counts]
        self.T = self.counts
        self.toff = [0]
        for n in self.counts:
            self.toff.append(self.toff[-1] + n)
        self.image_size = tuple(image_size)
        self._status, self._sample_status = status, sample_status
        self._targets = None

    @property
    def targets(self):
        if self._targets is None:
            mb = self.masks.view(torch.bool)
            self._targets = [{"labels": self.labels[a:b], "masks": mb[a:b]} for a, b in zip(self.toff, self.toff[1:])]
        return self._targets

    def __len__(self):
        return len(self.counts)

    def check(self):
        """Raise ValueError for what went wrong on the device side of instance_targets (see the class).  Waits for the GPU."""
        if self._status is not None:
            st = self._status.cpu().numpy() if isinstance(self._status, torch.Tensor) else np.asarray(self._status)
            for b, (bad, T, _, bits) in enumerate(st.tolist()):
                if bad:
                    raise ValueError(f"instance_targets: image {b} has {bad} pixels with ids outside [0, {LABEL_BINS})")
                if bits & 1:
                    raise ValueError(f"instance_targets: counts[{b}] = {self.counts[b]}, but image {b} holds {T} instances")
        if self._sample_status is not None:
            st = self._sample_status.cpu().numpy() if isinstance(self._sample_status, torch.Tensor) else np.asarray(self._sample_status)
            for b, bad in enumerate(st.tolist()):
                if bad:
                    raise ValueError(f"instance_targets: image {b} has {bad} pixels with dense labels outside [0, {SAMPLE_MAX_LABELS}): "
                                     "sample_pixels handles 256 labels per image")
        return self


def _fetch_counts(tables):
    """T_b of every image: the one pinned device-to-host copy and its wait."""
    host = torch.empty((tables.shape[0],), dtype=torch.int32, pin_memory=True)
    host.copy_(tables[:, 1], non_blocking=True)
    torch.cuda.current_stream(tables.device).synchronize()
    return host.tolist()


def _check_counts(counts, B):
    counts = [int(c) for c in counts]
    if len(counts) != B or any(c < 0 or c >= LABEL_BINS for c in counts):
        raise ValueError(f"counts: {B} instance counts in [0, {LABEL_BINS}) expected, got {counts}")
    return counts


def _round_up(v, d):
    return -(-v // d) * d if d > 1 else v


def instance_targets(raw, *, background_ids=BACKGROUND_IDS, class_id=1, size_divisibility=1, counts=None, sample_num=None, keys=None,
                     generator=None, label_dtype=torch.float32):
    """A batch (B,H,W) of instance label images (uint8 or an integer type; one (H,W) image is a batch of one) -> TargetBatch:
    the definitions of this module, on the side the images live on.

    ``counts=None``: the call makes ONE pinned device-to-host copy of the B instance counts and waits for it -- the host needs
    sum T_b to size the mask buffer; this is the call's only wait.  ``counts=[T_0, ...]`` (a loader that knows them): no copy
    and no wait; a count that disagrees with its image never makes the kernel write outside the buffer (rows beyond T_b are
    zero, instances beyond the count are dropped) and is reported by ``check()``, like out-of-range ids.
    ``sample_num``: sample the label map (definition 5) with ``keys`` (B,H,W) int32, or keys drawn from ``generator``.
    ``label_dtype``: float32 (what EmbeddingLoss reads) or int32."""
    if raw.ndim == 2:
        raw = raw[None]
    if raw.ndim != 3:
        raise ValueError(f"raw must be (H, W) or (B, H, W), got {tuple(raw.shape)}")
    if label_dtype not in (torch.float32, torch.int32):
        raise ValueError(f"label_dtype must be torch.float32 or torch.int32, got {label_dtype}")
    B, H, W = raw.shape
    d = int(size_divisibility)
    Hp, Wp = _round_up(H, d), _round_up(W, d)
    if counts is not None:
        counts = _check_counts(counts, B)
    if sample_num is not None and int(sample_num) < 1:
        raise ValueError(f"sample_num must be at least 1, got {sample_num}")
    if keys is not None and tuple(keys.shape) != (B, H, W):
        raise ValueError(f"keys {tuple(keys.shape)} must be {(B, H, W)}")
    if _is_device(raw):
        from . import ops
        dev = raw.device
        rawd = _raw_device(raw)
        tables = ops.target_tables(rawd, _device_background(dev, background_ids))
        if counts is None:
            counts = _fetch_counts(tables)
        toff = [0]
        for n in counts:
            toff.append(toff[-1] + n)
        label, masks, boxes, ids, areas = ops.target_write(rawd, tables, ops._device_table(toff, dev), toff[-1], frame=(Hp, Wp),
                                                           label_dtype=label_dtype)
        sample_status = None
        if sample_num is not None:
            if keys is None:
                keys = draw_keys((B, H, W), dev, generator)
            if not _is_device(keys):
                raise ValueError("keys must live where the label images live")
            sample_status = ops.sample_labels_(label, keys.to(torch.int32).contiguous(), int(sample_num), (H, W))
        labels = torch.full((toff[-1],), int(class_id), dtype=torch.int64, device=dev)
        return TargetBatch(masks, labels, boxes, ids, areas, label[:, None], counts, (H, W), tables[:, :4], sample_status)
    # host: the same definitions in numpy
    r = _host(raw)
    _check_host_ints(r, "instance_targets")
    lab, bad = _fold_host(r, background_ids)
    per = [_image_tables_host(lab[b]) for b in range(B)]
    true_T = [len(p[1]) for p in per]
    if counts is None:
        counts = true_T
    TT = sum(counts)
    masks = np.zeros((TT, Hp, Wp), dtype=np.uint8)
    boxes = np.zeros((TT, 4), dtype=np.float32)
    ids, areas = np.zeros((TT,), dtype=np.int32), np.zeros((TT,), dtype=np.int32)
    dense = np.zeros((B, Hp, Wp), dtype=np.int64)
    status = np.zeros((B, 4), dtype=np.int64)
    row = 0
    for b, (present, inst, dn) in enumerate(per):
        dense[b, :H, :W] = dn
        status[b] = (bad[b], true_T[b], len(present), 0 if counts[b] == true_T[b] else 1)
        for t, i in enumerate(inst[:counts[b]]):
            m = lab[b] == i
            masks[row + t, :H, :W] = m
            boxes[row + t] = _box_host(m)
            ids[row + t], areas[row + t] = i, m.sum()
        row += counts[b]
    sample_status = None
    if sample_num is not None:
        if keys is None:
            keys = draw_keys((B, H, W), "cpu", generator)
        if _is_device(keys):
            raise ValueError("keys must live where the label images live")
        sample_status = (dense[:, :H, :W] >= SAMPLE_MAX_LABELS).reshape(B, -1).sum(1)
        dense[:, :H, :W] = _sample_host(dense[:, :H, :W], _host(keys), int(sample_num))
    np_label = np.float32 if label_dtype == torch.float32 else np.int32
    return TargetBatch(torch.from_numpy(masks), torch.full((TT,), int(class_id), dtype=torch.int64), torch.from_numpy(boxes),
                       torch.from_numpy(ids), torch.from_numpy(areas), torch.from_numpy(dense.astype(np_label))[:, None], counts,
                       (H, W), status, sample_status)


# ----------------------------------------------------------------------------------------------------------------------------
# the reference's three methods by name
def _like(result, given):
    """A numpy result in the container of the input: a tensor for a tensor, an array for an array."""
    return torch.from_numpy(result) if isinstance(given, torch.Tensor) else result


def process_label(labels):
    """process_label: the values of one label image (H,W), or of each image of a batch (B,H,W), mapped to 0 .. K - 1 in ascending
    order (nothing is folded: the reference folds the table before it calls this).  Same container and integer type as the input
    on the host; an int32 map for a device tensor."""
    single = labels.ndim == 2
    x = labels[None] if single else labels
    if _is_device(x):
        from . import ops
        rawd = _raw_device(x)
        out = ops.target_write(rawd, ops.target_tables(rawd), label_dtype=torch.int32)[0]
    else:
        a = _host(x)
        _check_host_ints(a, "process_label")
        out = _like(np.stack([_image_tables_host(a[b].astype(np.int64))[2] for b in range(a.shape[0])]).astype(a.dtype), labels)
    return out[0] if single else out


def process_label_to_annos(labels, class_id=1):
    """process_label_to_annos for one label image (H,W) -> (boxes (T,4) float32, masks (T,H,W) float32, classes (T,) int64), one
    instance per non-zero value in ascending order (every value when 0 does not occur); a batch (B,H,W) gives three lists.
    Every class is ``class_id``: the reference's __getitem__ drops the clip(1, 2) labels this method returns there and records
    "category_id": 1."""
    single = labels.ndim == 2
    tb = instance_targets(labels, background_ids=(), class_id=class_id)
    out = [], [], []
    for a, b in zip(tb.toff, tb.toff[1:]):
        out[0].append(tb.boxes[a:b]), out[1].append(tb.masks[a:b].to(torch.float32)), out[2].append(tb.labels[a:b])
    return tuple(o[0] for o in out) if single else out


def sample_pixels(labels, num=1000, *, keys=None, generator=None):
    """sample_pixels: a copy of the dense label map(s) (H,W) / (B,H,W) in which every label with more than ``num`` pixels keeps
    the ``num`` smallest by (key, flat index) and loses the others to -1 (definition 5).  ``keys``: int32 of the labels' shape,
    default drawn from ``generator``.  Device maps are float32 or int32 (msm_sample_labels, at most 256 labels per image: more
    raise); host maps any signed type."""
    if int(num) < 1:
        raise ValueError(f"sample_pixels: num must be at least 1, got {num}")
    single = labels.ndim == 2
    x = labels[None] if single else labels
    if keys is None:
        keys = draw_keys(x.shape, x.device if _is_device(x) else "cpu", generator)
    elif keys.ndim == 2:
        keys = keys[None]
    if tuple(keys.shape) != tuple(x.shape):
        raise ValueError(f"sample_pixels: keys {tuple(keys.shape)} must have the labels' shape {tuple(x.shape)}")
    if _is_device(x):
        from . import ops
        if not _is_device(keys):
            raise ValueError("sample_pixels: keys must live where the labels live")
        out = x.contiguous().clone()
        status = ops.sample_labels_(out, keys.to(torch.int32).contiguous(), int(num))
        if int(status.sum()):
            raise ValueError(f"sample_pixels: labels must be integers below {SAMPLE_MAX_LABELS}")
    else:
        a = _host(x)
        if a.dtype.kind == "u":
            raise TypeError("sample_pixels: a signed label type is needed to hold -1")
        out = _like(_sample_host(a, _host(keys), int(num)).astype(a.dtype), labels)
    return out[0] if single else out


def training_batch(color, depth, raw, camera_params, *, size_divisibility=1, order="bgr", depth_scale=1000.0, augment=None,
                   crop=None, crop_size=224, **target_args):
    """Raw frames and their label images -> (image, xyz, TargetBatch): frames.ingest and instance_targets padded to the same
    ``size_divisibility``.  ``training.ucn_model_losses(model, image, xyz, batch.targets, criterion, labels=batch.label, ...)``
    (or ``batch`` itself in place of ``batch.targets``) takes them as they are.  ``target_args``: instance_targets' keywords.
    ``augment``: an augment.AugmentParams (augment.draw_params) living where the frames live -- the loader's random
    augmentations in the reference's order: the colour frames (in the order they arrive in; the reference's are BGR), the
    depth (scaled and with ellipses dropped, float32 metres from there on), ingest, then the point-cloud noise on the valid
    corner of xyz.  The label images are not touched, as in the reference.  None: exactly the launches without it.
    ``crop``: a crops.CropParams (crops.draw_crop_params) living where the frames live -- the reference's TRAIN.SYN_CROP path
    that trains the second-stage model, in its order (tabletop_dataset.py:349-367): depth augmentation, ingest at FULL
    resolution for xyz, point-cloud noise, then one object per frame is chosen, its box squared, padded and clamped, colour,
    label image and xyz are cropped there and resized to ``crop_size`` = S (crops.crop_boxes, crops.crop_resize),
    instance_targets runs on the label crops (``sample_num`` and its keys at S x S), the colour augmentation on the S x S colour
    crops, and frames.ingest turns those into the image.  Everything comes back at (B, 3, Sp, Sp), ``batch.image_size == (S, S)``
    and ``batch.crop_boxes`` holds the boxes.  The colour half of ``augment`` is therefore drawn at the crop size
    (``pixel_noise`` (B,S,S): anything else raises ValueError before a launch) and its ``gp_noise`` for the frame size:
    augment.draw_params(B, S, S, ...) for the former and (B, 3, H // 4, W // 4) for the latter.  The only wait remains
    instance_targets' count copy; ``counts=`` cannot be known before the crop is taken -- an object that leaves the crop leaves
    the targets -- so a loader has none to give here.  None: exactly the launches without it."""
    if color.ndim != 4 or raw.ndim != 3 or tuple(raw.shape) != tuple(color.shape[:3]):
        raise ValueError(f"training_batch: colour {tuple(color.shape)} must be (B, H, W, 3) and raw {tuple(raw.shape)} (B, H, W)")
    if _is_device(color) != _is_device(raw):
        raise ValueError("training_batch: frames and label images must live on the same side")
    if crop is not None:
        return _training_batch_crop(color, depth, raw, camera_params, size_divisibility, order, depth_scale, augment, crop,
                                    int(crop_size), target_args)
    if augment is not None:
        from . import augment as aug
        color = aug.augment_color(color, augment)
        if depth is not None:
            depth, depth_scale = aug.augment_depth(depth, augment, depth_scale=depth_scale), 1.0
    image, xyz = frames.ingest(color, depth, camera_params, order=order, depth_scale=depth_scale, size_divisibility=size_divisibility)
    if augment is not None and xyz is not None and augment.gp_noise is not None:
        aug.add_xyz_noise_(xyz, augment, size=tuple(color.shape[1:3]))
    return image, xyz, instance_targets(raw, size_divisibility=size_divisibility, **target_args)


def _training_batch_crop(color, depth, raw, camera_params, size_divisibility, order, depth_scale, augment, crop, S, target_args):
    """training_batch with ``crop=``: the order of its docstring."""
    from . import crops
    B, H, W = raw.shape
    if len(crop) != B:
        raise ValueError(f"training_batch: {len(crop)} crop parameter rows for {B} frames")
    if augment is not None:
        from . import augment as aug
        if augment.pixel_noise is not None and tuple(augment.pixel_noise.shape) != (B, S, S):
            raise ValueError(f"training_batch: with crop= the colour augmentation runs on the {S} x {S} crops: pixel_noise "
                             f"{tuple(augment.pixel_noise.shape)} must be {(B, S, S)} (draw the colour half at the crop size)")
        if depth is not None:
            depth, depth_scale = aug.augment_depth(depth, augment, depth_scale=depth_scale), 1.0
    xyz = None
    if depth is not None:
        xyz = frames.ingest(color, depth, camera_params, order=order, depth_scale=depth_scale)[1]
        if augment is not None and augment.gp_noise is not None:
            aug.add_xyz_noise_(xyz, augment, size=(H, W))
    boxes = crops.crop_boxes(raw, crop, background_ids=target_args.get("background_ids", BACKGROUND_IDS))
    color_crop, raw_crop, xyz_crop = crops.crop_resize(color, raw, xyz, boxes, S, size_divisibility=size_divisibility)
    batch = instance_targets(raw_crop, size_divisibility=size_divisibility, **target_args)
    batch.crop_boxes = boxes
    if augment is not None:
        color_crop = aug.augment_color(color_crop, augment)
    image = frames.ingest(color_crop, None, None, order=order, size_divisibility=size_divisibility)[0]
    if isinstance(xyz_crop, np.ndarray):                   # host arrays: a tensor, as frames.ingest returns its xyz
        xyz_crop = torch.from_numpy(xyz_crop)
    return image, xyz_crop, batch
