"""Classic UCN vMF mean-shift clustering on the HIP kernels.

Mirrors lib/utils/mean_shift.py (and its copy under MSMFormer/.../transformer_decoder/mean_shift.py)
and the driver lib/fcn/test_dataset.py:44-59: same function names, argument meaning and return
values.  The O(n) passes (seeding, hill climbing, assignment, relabel) and the order-dependent
merge of up to 304 seeds (connected_components, mean_shift.py:41-76) run on the GPU; larger seed
sets take a host loop on a (S, 64) copy of the seeds, as the reference does.

Both metrics of the reference are implemented for device tensors: ``metric="cosine"`` (unit
embeddings; every shipped experiment config) and ``metric="euclidean"`` (lib/fcn/config.py:262,
the default TRAIN.EMBEDDING_METRIC; embeddings need not be normalised, e.g.
``UCNBackbone(normalize=False)``): d = ||x - z||_2, W = exp(-kappa d^2),
Z <- W X / clamp(sum W, min=1), merge at d <= epsilon.  The Euclidean metric has the exact fp32 plan
only -- the persistent seeding kernels and the 16-bit plans ("f32_split", "bf16") are cosine-only,
so it seeds with one launch per step and never needs the give-up retry.  Host tensors have no
clustering path in this package: the cosine merge alone runs on them, ``metric="euclidean"``
raises NotImplementedError, an unknown metric ValueError.
"""
import numpy as np
import torch

from . import ops

EMBEDDING_ALPHA = 0.02   # cfg.TRAIN.EMBEDDING_ALPHA, lib/fcn/config.py:255


def _euclidean(metric, *tensors, precision="f32"):
    """True for metric="euclidean" (device tensors and the fp32 plan only), False for "cosine"."""
    if metric not in ops.MS_METRICS:
        raise ValueError(f"metric must be 'cosine' or 'euclidean', not {metric!r}")
    if metric == "cosine":
        return False
    if precision != "f32":
        raise ValueError(f"metric='euclidean' has the exact fp32 plan only, not precision={precision!r}")
    if not all(t.is_cuda for t in tensors):
        raise NotImplementedError("metric='euclidean' is implemented for device tensors only: the clustering has no CPU path")
    return True


def ball_kernel(Z, X, kappa, metric="cosine"):
    """mean_shift.py:11-27.  Materialises the (S, n) kernel matrix -- provided for API parity and
    small problems only; the clustering path below never builds it."""
    Z, X = Z.contiguous(), X.contiguous()
    if _euclidean(metric, Z, X):
        d2 = (Z * Z).sum(dim=1)[:, None] + (X * X).sum(dim=1)[None, :] - 2 * ops.gemm(Z, X)
        return torch.exp(-kappa * d2.clamp_(min=0))
    return torch.exp(kappa * ops.gemm(Z, X))


def get_label_mode(array):
    labels, counts = np.unique(array, return_counts=True)
    return labels[np.argmax(counts)].item()


def connected_components(Z, epsilon, metric="cosine"):
    """mean_shift.py:41-76: sequential, order-dependent merge of the converged seeds.  On the device (one wave,
    ops.ms_connected_components) for up to 304 seeds -- no host synchronisation; larger seed sets take the host loop."""
    l2 = _euclidean(metric, Z)
    if Z.is_cuda and Z.shape[0] <= 304 and Z.shape[1] == 64:
        return ops.ms_connected_components(Z.contiguous(), epsilon, metric)[0]
    return _components_host(Z, epsilon, l2)


def connected_components_host(Z, epsilon):
    """The same merge on the host, on a copy of the seeds (the reference's own form; fallback and test partner)."""
    return _components_host(Z, epsilon, False)


def _components_host(Z, epsilon, l2):
    Zc = Z.detach().to("cpu", torch.float32)
    n = Zc.shape[0]
    K = 0
    labels = np.full((n,), -1, dtype=np.int64)          # bookkeeping in numpy: ~100 seeds, a dozen components
    for i in range(n):
        if labels[i] != -1:
            continue
        if l2:
            comp = (torch.norm(Zc - Zc[i], dim=1) <= epsilon).numpy()     # MS:59-60
        else:
            comp = ((0.5 * (1 - Zc @ Zc[i])) <= epsilon).numpy()     # same fp32 matrix-vector product as the reference
        seen = labels[comp]
        if np.unique(seen).shape[0] > 1:
            label = get_label_mode(seen[seen != -1])
        else:
            label = K
            K += 1
        labels[comp] = label
    return torch.from_numpy(labels)


def seed_hill_climbing_ball(X, Z, kappa, max_iters=10, metric="cosine", precision="f32", xb=None):
    """mean_shift.py:79-109.  ``precision`` (not in the reference): "f32" (fp32 MFMAs), "f32_split" (fp32 results on
    the bf16 matrix pipe) or "bf16" (single bf16 products over a bf16 copy of X, BASELINE configs[4]); ops.ms_hill_climb."""
    _euclidean(metric, X, Z, precision=precision)
    return ops.ms_hill_climb(X.contiguous(), Z.contiguous(), kappa, max_iters, precision=precision, xb=xb, metric=metric)


def mean_shift_with_seeds(X, Z, kappa, max_iters=10, metric="cosine", precision="f32"):
    Z = seed_hill_climbing_ball(X, Z, kappa, max_iters=max_iters, metric=metric, precision=precision)
    return connected_components(Z, 2 * EMBEDDING_ALPHA, metric=metric), Z      # MS:123: the same epsilon for both metrics


def _components_with_count(Z, epsilon, metric="cosine"):
    """(seed_labels, num) with num = len(unique(seed_labels)) as a 1-element int32 device tensor (no host synchronisation on
    the device path): what mean_shift.py:211-216 bounds its per-label counts by."""
    if Z.is_cuda and Z.shape[0] <= 304 and Z.shape[1] == 64:
        labels, num = ops.ms_connected_components(Z.contiguous(), epsilon, metric)
        return labels, num[:1]
    labels = _components_host(Z, epsilon, metric == "euclidean")
    return labels, torch.tensor([int(torch.unique(labels).numel())], dtype=torch.int32, device=Z.device)


def select_smart_seeds(X, num_seeds, return_selected_indices=False, init_seeds=None, num_init_seeds=None,
                       metric="cosine", first_index=None, stepwise=False, xb=None):
    """mean_shift.py:128-189.  The first seed index comes from np.random.randint(0, n) like the
    reference (mean_shift.py:155) unless ``first_index`` is given.  The Euclidean metric always takes one launch per step."""
    l2 = _euclidean(metric, X, precision="f32" if xb is None else "bf16")
    if init_seeds is not None:
        raise NotImplementedError("init_seeds is unused by the inference path")
    if first_index is None:
        first_index = np.random.randint(0, X.shape[0])
    if l2:
        seeds, idx = ops.ms_select_seeds(X.contiguous(), num_seeds, int(first_index), metric=metric)     # never gives up
        return (seeds, idx) if return_selected_indices else (seeds,)
    seeds, idx = ops.ms_select_seeds(X.contiguous(), num_seeds, int(first_index), stepwise=stepwise, xb=xb)
    if not return_selected_indices:
        # the caller cannot see the indices, so the give-up of the persistent kernel (ops.ms_select_seeds) is handled here
        if not stepwise and int(idx.min()) < 0:
            seeds, idx = ops.ms_select_seeds(X.contiguous(), num_seeds, int(first_index), stepwise=True, xb=xb)
        return (seeds,)
    return seeds, idx


def mean_shift_smart_init(X, kappa, num_seeds=100, max_iters=10, metric="cosine", first_index=None, precision="f32"):
    """mean_shift.py:192-229.  Returns (cluster_labels (n,) int64 on X.device, selected_indices (S,)).  ``precision`` "f32" /
    "f32_split": the reference's arithmetic (exact labels); "bf16" (BASELINE configs[4]): seeding and hill climb stream one bf16 copy
    of X -- the same clusters, possibly other member points as seeds and another numbering of the labels.  ``metric`` "euclidean":
    precision "f32" only."""
    l2 = _euclidean(metric, X, precision=precision)
    X = X.contiguous()
    if first_index is None:
        first_index = np.random.randint(0, X.shape[0])                   # MS:155, drawn once: a retry reuses it
    xb = ops.ms_pack_bf16(X) if precision == "bf16" else None
    seeds, selected = select_smart_seeds(X, num_seeds, return_selected_indices=True, metric=metric,
                                         first_index=first_index, xb=xb)
    def rest(seeds):
        Z = seed_hill_climbing_ball(X, seeds, kappa, max_iters=max_iters, metric=metric, precision=precision, xb=xb)
        seed_labels, num = _components_with_count(Z, 2 * EMBEDDING_ALPHA, metric)
        # labels are created in order 0, 1, ...: at most one per seed, so num_seeds bounds the histogram of the assignment; the
        # largest-cluster swap looks at labels 0 .. len(unique(seed_labels)) - 1 only, like the reference (MS:211-222)
        labels, counts = ops.ms_assign(X, Z, seed_labels.to(X.device), seeds.shape[0], metric)
        ops.ms_relabel_largest_zero(labels, counts, num)
        return labels

    labels = rest(seeds)
    if l2:
        return labels, selected          # stepwise seeding: there is no give-up to check, and nothing waits for the host
    # The whole clustering is queued without a host synchronisation (the merge of the seeds runs on the device); the one
    # check that needs the host comes last, when everything is in flight: the give-up flag of the persistent seeding kernel
    # (co-residency lost to other streams / processes).  A give-up re-runs seeding on the one-launch-per-step path
    # (identical results) and everything after it.
    if int(selected.min()) < 0:
        seeds, selected = select_smart_seeds(X, num_seeds, return_selected_indices=True, metric=metric,
                                             first_index=first_index, stepwise=True, xb=xb)
        labels = rest(seeds)
    return labels, selected


def mean_shift_smart_init_batched(X, kappa, num_seeds=100, max_iters=10, first_indices=None, _test_give_up=None, metric="cosine"):
    """mean_shift_smart_init for M maps of one size in one set of launches: X (M,n,64) rows on the device (unit rows for the cosine
    metric) -> (labels (M,n) int64, selected (M,S) int64), each map's equal bit for bit to mean_shift_smart_init(X[m], ...,
    first_index=first_indices[m], metric=metric).  The exact fp32 plan only ("f32_split" / "bf16" stay on the per-map call).
    ``first_indices`` None draws np.random.randint(0, n) once per map, in map order, before anything is queued -- the sequence the
    per-map loop consumes (MS:155).  Everything is queued without a host synchronisation; the one check comes last: maps whose
    seeding group gave up (indices -1, ops.ms_select_seeds_batched) are re-run on the stepwise batched form with their recorded
    first index, the others keep their results (the Euclidean metric seeds stepwise from the start: no check, no synchronisation)."""
    l2 = _euclidean(metric, X)
    X = X.contiguous()
    M, n, _ = X.shape
    if first_indices is None:
        first_indices = [np.random.randint(0, n) for _ in range(M)]
    first = ops._first_indices_device(first_indices, M, n, X.device, "mean_shift_smart_init_batched")

    def chain(Xs, first, stepwise, give_up=None):
        seeds, selected = ops.ms_select_seeds_batched(Xs, num_seeds, first, stepwise=stepwise, _test_give_up=give_up, metric=metric)
        Z = ops.ms_hill_climb_batched(Xs, seeds, kappa, max_iters, metric)
        seed_labels, num = ops.ms_connected_components_batched(Z, 2 * EMBEDDING_ALPHA, metric)
        labels, counts = ops.ms_assign_batched(Xs, Z, seed_labels, num_seeds, metric)      # num_seeds bounds the labels (see mean_shift_smart_init)
        ops.ms_relabel_largest_zero_batched(labels, counts, num)
        return labels, selected

    if l2:
        return chain(X, first, True)
    labels, selected = chain(X, first, False, _test_give_up)
    gave_up = torch.nonzero(selected.min(dim=1).values < 0).flatten()              # the one host synchronisation
    if gave_up.numel():
        l2, s2 = chain(X[gave_up].contiguous(), first[gave_up].contiguous(), True)
        labels[gave_up] = l2
        selected[gave_up] = s2
    return labels, selected


def clustering_features(features, num_seeds=100, metric="cosine", precision="f32", first_indices=None, map_batch=64):
    """lib/fcn/test_dataset.py:44-59: features (B,C,H,W) (unit-norm along C for the cosine metric) -> (out_label (B,H,W) float,
    selected_pixels list of (S,) index tensors).  kappa=20, 10 iterations.  ``first_indices`` (not in the reference): the first
    seed index of every map instead of np.random.randint (MS:155).  B >= 2 maps on the device with
    precision "f32" (either metric) are clustered together (mean_shift_smart_init_batched), ``map_batch`` maps at a time to bound the workspace,
    with results equal to the per-map loop's bit for bit; B = 1, "f32_split" and "bf16" take the loop."""
    B, C, H, W = features.shape
    _euclidean(metric, features, precision=precision)
    out_label = torch.zeros((B, H, W), device=features.device)
    selected_pixels = []
    if B >= 2 and features.is_cuda and precision == "f32":
        if first_indices is None:
            first_indices = [np.random.randint(0, H * W) for _ in range(B)]      # map order, as the loop below would draw them
        first_indices = torch.as_tensor(first_indices, dtype=torch.int64).reshape(-1).cpu()
        for j0 in range(0, B, max(1, int(map_batch))):
            j1 = min(B, j0 + max(1, int(map_batch)))
            X = ops.transpose_last2(features[j0:j1].reshape(j1 - j0, C, H * W).contiguous())      # the copy is bounded by map_batch too
            labels, sel = mean_shift_smart_init_batched(X, kappa=20, num_seeds=num_seeds, max_iters=10,
                                                        first_indices=first_indices[j0:j1], metric=metric)
            out_label[j0:j1] = labels.view(j1 - j0, H, W).float()
            selected_pixels.extend(sel.unbind(0))
        return out_label, selected_pixels
    for j in range(B):
        X = ops.transpose_last2(features[j].reshape(1, C, H * W).contiguous())[0]
        labels, sel = mean_shift_smart_init(X, kappa=20, num_seeds=num_seeds, max_iters=10, metric=metric, precision=precision,
                                            first_index=None if first_indices is None else int(first_indices[j]))
        out_label[j] = labels.view(H, W).float()
        selected_pixels.append(sel)
    return out_label, selected_pixels
