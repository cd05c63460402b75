"""Cases and float64 definitions for the Euclidean metric of the mean-shift clustering (lib/utils/mean_shift.py, the
``metric == 'euclidean'`` branches: MS:21-24, 58-60, 101-105, 159-160, 181-182, 207-209).

Used by tests/golden/make_golden_ms_euclidean.py (which checks these definitions against the reference's own functions),
tests/test_ms_euclid_cases_cpu.py and tests/test_gpu_meanshift_euclidean.py.  Everything here runs on the CPU; the float64
results are computed once per case and shared (callers must not modify them)."""
import functools

import numpy as np
import torch

D = 64
KAPPA = 20.0
ITERS = 10
ALPHA = 0.02                 # cfg.TRAIN.EMBEDDING_ALPHA
EPS = 2 * ALPHA              # MS:123

# (n, clusters, sigma, S, seed, scale): whole 16-point slabs, two seed blocks | three slabs, the last with 5 rows, S < one seed
# block | two slabs, 17 seeds = one block + 1 | a ragged n over several workgroups | S = 300: three chunks of seed blocks per
# iteration, rows of norm 2 | 19200 = 160 x 120, the map of a small frame, more than one pass of a wave over its slabs
CASES = [(2000, 6, .02, 20, 1, 1.0), (37, 3, .02, 5, 3, 1.0), (31, 3, .02, 17, 6, 1.0), (4111, 9, .03, 50, 2, 1.0),
         (5000, 24, .02, 300, 4, 2.0), (19200, 10, .03, 100, 5, 1.0)]
GOLDEN_CASES = (0, 1)        # the reference's own results are stored for these (tests/golden/mean_shift_euclidean.npz)


def first_index(case):
    n = CASES[case][0]
    return (7 * n) // 13


@functools.lru_cache(maxsize=None)
def planted(case):
    """-> (X (n,64) float32, un-normalised; ids (n,) int64): X = C[ids] + sigma * randn, C random directions of length ``scale``.
    Cluster c gets a share of the points proportional to c + 2, so the sizes differ (the largest-cluster swap has one answer)."""
    n, clusters, sigma, _, seed, scale = CASES[case]
    g = torch.Generator().manual_seed(seed)
    C = torch.randn(clusters, D, generator=g, dtype=torch.float64)
    C = C / C.norm(dim=1, keepdim=True) * scale
    w = torch.arange(2, clusters + 2, dtype=torch.float64)
    bounds = torch.round(torch.cumsum(w, 0) / w.sum() * n).long()
    ids = torch.searchsorted(bounds, torch.arange(n), right=True).clamp_(max=clusters - 1)
    ids = ids[torch.randperm(n, generator=g)]
    X = (C[ids] + sigma * torch.randn(n, D, generator=g, dtype=torch.float64)).float().contiguous()
    return X, ids


def checksum(X):
    """float64 sum of X[i, j] * (1 + (i * 64 + j) mod 251): what the goldens record instead of X."""
    w = 1.0 + (torch.arange(X.numel(), dtype=torch.float64) % 251)
    return float((X.double().reshape(-1) * w).sum())


# ---- seeding (MS:155-187) ----------------------------------------------------------------------------------------------
def seeding64(X, S, first, forced=None):
    """Farthest-point seeding in float64.  -> dict(idx (S,), top (S,) the step's maximum of the nearest-seed distance, pick (S,)
    the nearest-seed distance of the index taken, margin (S,) = (top1 - top2) / top1 of the step; entry 0 is unused).
    ``forced``: take these indices instead of the argmax (the replay of a kernel's picks); the statistics stay those of the
    float64 distances."""
    Xd = X.double()
    n = Xd.shape[0]
    idx = np.zeros(S, dtype=np.int64)
    top, pick, margin = np.zeros(S), np.zeros(S), np.ones(S)
    idx[0] = first
    nearest = torch.full((n,), float("inf"), dtype=torch.float64)
    for i in range(1, S):
        nearest = torch.minimum(nearest, (Xd - Xd[idx[i - 1]]).norm(dim=1))
        best = int(torch.argmax(nearest))                       # first maximum, like torch.argmax in the reference
        top[i] = float(nearest[best])
        if n > 1:
            second = float(torch.cat([nearest[:best], nearest[best + 1:]]).max())
            margin[i] = (top[i] - second) / top[i] if top[i] > 0 else 0.0
        idx[i] = best if forced is None else int(forced[i])
        pick[i] = float(nearest[idx[i]])
    return dict(idx=idx, top=top, pick=pick, margin=margin)


# ---- hill climb (MS:90-105) --------------------------------------------------------------------------------------------
def _hill(X, Z, kappa, iters):
    """The reference's direct-difference form in the dtype of X: d = ||z - x|| from the differences, W = exp(-kappa d^2),
    Z = W X / clamp(sum W, min=1).  -> (Z, sum W of the LAST iteration)."""
    sw = None
    for _ in range(iters):
        d = torch.cdist(Z, X, compute_mode="donot_use_mm_for_euclid_dist")
        W = torch.exp(-kappa * d.pow(2))
        sw = W.sum(dim=1)
        Z = (W @ X) / sw.clamp(min=1.0).unsqueeze(1)
    return Z, sw


def hill64(X, Z, kappa=KAPPA, iters=ITERS):
    return _hill(X.double(), Z.double(), kappa, iters)


def hill32(X, Z, kappa=KAPPA, iters=ITERS):
    """The same form in plain fp32 on the CPU: the yardstick of what fp32 arithmetic costs on these inputs."""
    return _hill(X.float(), Z.float(), kappa, iters)


def far_seed(case):
    """A seed that is no data point and far from all of them: next to the origin, at distance ~ scale from every point, so every
    weight is tiny (e^-20 at scale 1, e^-80 at scale 2: still normal fp32 numbers, not flushed to zero) and sum W < 1 (the
    clamp(min=1) branch)."""
    scale = CASES[case][5]
    g = torch.Generator().manual_seed(1000 + case)
    u = torch.randn(D, generator=g, dtype=torch.float64)
    return (0.05 * scale * u / u.norm()).float()


@functools.lru_cache(maxsize=None)
def hill_case(case, iters):
    """-> dict(Z0 (S+1,64) fp32: the float64 seeding's seeds plus far_seed, Z64, Z32, err32 = max |Z32 - Z64|, far_sum = float64
    sum W of the far seed in the first iteration)."""
    X, _ = planted(case)
    S = CASES[case][3]
    sel = seeding64(X, S, first_index(case))["idx"]
    Z0 = torch.cat([X[torch.from_numpy(sel)], far_seed(case)[None]]).contiguous()
    Z64, _ = hill64(X, Z0, KAPPA, iters)
    Z32, _ = hill32(X, Z0, KAPPA, iters)
    _, sw1 = hill64(X, Z0[-1:], KAPPA, 1)
    return dict(Z0=Z0, Z64=Z64, Z32=Z32, err32=float((Z32.double() - Z64).abs().max()), far_sum=float(sw1[0]))


# ---- connected components (MS:41-76) -----------------------------------------------------------------------------------
def components64(Z, eps=EPS):
    """MS:41-76 with the Euclidean membership test in float64 -> (labels (S,) int64, (alive, created))."""
    Zd = Z.double()
    S = Zd.shape[0]
    labels = np.full(S, -1, dtype=np.int64)
    K = 0
    for i in range(S):
        if labels[i] != -1:
            continue
        comp = ((Zd - Zd[i]).norm(dim=1) <= eps).numpy()
        seen = labels[comp]
        if np.unique(seen).shape[0] > 1:                         # MS:66-69: the mode of the labels already there
            vals, counts = np.unique(seen[seen != -1], return_counts=True)
            label = int(vals[np.argmax(counts)])
        else:
            label = K
            K += 1
        labels[comp] = label
    return torch.from_numpy(labels), (int(np.unique(labels).shape[0]), K)


def eps_margin(Z, eps=EPS):
    """min over seed pairs of | ||z_i - z_j|| - eps |: how far the merge is from depending on rounding."""
    d = torch.cdist(Z.double(), Z.double(), compute_mode="donot_use_mm_for_euclid_dist")
    return float((d - eps).abs().min())


CHAIN_ORDER = [0, 4, 1, 2, 3, 5, 8, 14, 11, 9, 17, 12, 10, 15, 13, 18, 16, 19]
# By hand, eps = 0.04, seeds at 0.03 * CHAIN_ORDER[i] on a line (a seed reaches its direct neighbours only):
#   i0 (0) takes i2 (1) -> 0; i1 (4) takes i4 (3), i5 (5) -> 1; i3 (2) meets i2 (label 0) and i4 (label 1): a tie, the smaller
#   label wins and i4 is overwritten -> 0.  Second run: i6 (8), i9 (9) -> 2; i7 (14), i14 (13), i13 (15) -> 3; i8 (11), i12 (10),
#   i11 (12) -> 4; i10 (17), i16 (16), i15 (18) -> 5; i17 (19) meets i15 (label 5) alone -> 5.
CHAIN_LABELS = [0, 1, 0, 0, 0, 1, 2, 3, 4, 2, 5, 4, 4, 3, 3, 5, 5, 5]


def chain(step=0.03):
    """Seeds ``step`` apart on a line in two runs, visited in an order that makes the merge order dependent: later seeds meet
    labels made earlier (the mode branch, once with a tie) and overwrite a neighbour's label.  In line order every run would
    collapse into one label."""
    Z = torch.zeros(len(CHAIN_ORDER), D)
    Z[:, 0] = 0.5
    Z[:, 1] = torch.tensor([step * o for o in CHAIN_ORDER])
    return Z.contiguous()


# ---- assignment and the whole clustering (MS:192-229) ------------------------------------------------------------------
def dist2_64(X, Z):
    return torch.cdist(X.double(), Z.double(), compute_mode="donot_use_mm_for_euclid_dist").pow(2)


def relabel_largest_zero(labels, seed_labels):
    """MS:217-227 on a copy."""
    labels = labels.clone()
    num = len(torch.unique(seed_labels))
    count = torch.tensor([int((labels == i).sum()) for i in range(num)])
    lmax = int(torch.argmax(count))
    if lmax != 0:
        i1, i2 = labels == 0, labels == lmax
        labels[i1] = lmax
        labels[i2] = 0
    return labels


@functools.lru_cache(maxsize=None)
def smart_init64(case):
    """mean_shift_smart_init(metric='euclidean') in float64 -> dict(sel, Z, seed_labels, labels, seeding)."""
    X, _ = planted(case)
    S = CASES[case][3]
    seeding = seeding64(X, S, first_index(case))
    sel = torch.from_numpy(seeding["idx"])
    Z, _ = hill64(X, X[sel], KAPPA, ITERS)
    seed_labels, _ = components64(Z, EPS)
    labels = seed_labels[torch.argmin(dist2_64(X, Z), dim=1)]
    return dict(sel=sel, Z=Z, seed_labels=seed_labels, labels=relabel_largest_zero(labels, seed_labels), seeding=seeding)
