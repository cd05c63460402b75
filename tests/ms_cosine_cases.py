"""Cases and float64 definitions for the cosine (vMF) metric of the mean-shift clustering (lib/utils/mean_shift.py: MS:26, 90-107,
155-187, 192-229): seeding with d = 0.5 (1 - x.s), Z = normalize(exp(kappa Z X^T) X), first-argmin assignment.

Used by tests/test_ms_cosine_cases_cpu.py (which checks these definitions against oracle/msm_oracle.py and
tests/golden/mean_shift.npz, and the properties of the inputs that the GPU tests rely on) and tests/test_gpu_meanshift_cosine.py.
Everything here runs on the CPU; the float64 results are computed once per case and shared (callers must not modify them).

Measured on an MI355X (test_gpu_meanshift_cosine.py::test_hill_climb prints the figures per case), err_gpu = max |Z - Z64| of
ops.ms_hill_climb(precision="f32") over err32 = the same figure of hill32 below, over all cases and iters in {1, 10}:
    err_gpu / err32 = 0.37 ... 1.36   (err_gpu 2.4e-8 ... 8.6e-8, err32 on that host 2.4e-8 ... 1.8e-7; the far seed's row after one
    iteration 2.1e-8 ... 4.0e-8 against 2.6e-8 ... 9.9e-8; MS_CHUNK = 1 .. 8 and NSB = 1 .. 8 bit-equal, both metrics)
so the factor 4 of hill_bound is never approached: neither v_exp_f32 nor the MFMA summation order costs more than the CPU's fp32.
Every seeding pick of every form was the float64 argmax itself, also at the steps whose margin is below 2 E."""
import functools

import numpy as np
import torch

from unseenobjectswithmeanshift_amd import synthetic as syn

D = 64
KAPPA = 20.0
ITERS = 10
EPS = 2 * 0.02               # MS:123: 2 * cfg.TRAIN.EMBEDDING_ALPHA
U = 2.0 ** -24               # unit roundoff of fp32

# (n, clusters, sigma, S, seed): whole 16-row groups, two seed blocks | n < 16: the SMALL seeding step, one partial slab | exactly
# one slab, exactly one seed block | one seed | one seed block + 1, a tail slab of 15 rows | persistent seeding, ragged n, four seed
# blocks in one launch | eight seed blocks in one launch, one assignment chunk exactly full | the hill climb's grid at its cap of 512
# workgroups (two waves walk a second slab, one of them the 5-row tail), nine seed blocks = launches of 5 + 4, the last block with one
# seed, two assignment chunks | the S limit: launches of 7 + 7 + 5 seed blocks, three assignment chunks | three seed blocks in one launch
CASES = [(2000, 6, .15, 20, 1), (15, 2, .10, 5, 2), (16, 2, .10, 16, 3), (37, 3, .15, 1, 4), (31, 3, .15, 17, 5),
         (4111, 9, .20, 50, 6), (4096, 5, .15, 128, 9), (32789, 10, .20, 129, 8), (5003, 24, .15, 304, 7), (4111, 9, .20, 48, 6)]
ALL = range(len(CASES))
MULTI = [c for c in ALL if CASES[c][3] > 1]          # the cases with more than one seed
EXACT_SEEDING = (1, 2)       # n = 15, 16: every float64 step margin is far above the fp32 error, the picks are unique
LIMIT = 8                    # the S = 304 case
# Seeding only, S = 12: the smallest ragged n that the host sends to 2 and to 3 tiles per lane group of the single-map persistent
# kernel (ng = cdiv(n, 131072)), and one map just above the fp32 persistent limit of 393 216 rows, for the bf16 forms.
SEED_MAPS = {"ng2": (131075, 10, .20, 12, 11), "ng3": (262147, 10, .20, 12, 12), "bf16": (393217 + 22, 10, .20, 12, 13)}


def _spec(case):
    return SEED_MAPS[case] if isinstance(case, str) else CASES[case]


def first_index(case):
    return (7 * _spec(case)[0]) // 13


@functools.lru_cache(maxsize=None)
def planted(case):
    """-> (X (n,64) fp32 unit rows, ids (n,) int64): synthetic.synth_unit_embeddings of the case."""
    n, clusters, sigma, _, seed = _spec(case)
    return syn.synth_unit_embeddings(n, D, clusters=clusters, sigma=sigma, seed=seed)


@functools.lru_cache(maxsize=None)
def planted_bf16(case):
    """The points as the bf16 forms see them: every coordinate rounded to bf16 (rows no longer exactly of unit length)."""
    return planted(case)[0].to(torch.bfloat16).float().contiguous()


def bound(xn=1.0, zn=1.0):
    """E: the worst-case error of a cosine distance 0.5 (1 - x.z) computed in fp32 -- a dot product of 64 terms in any summation
    order (64 u |x||z|), halved by the distance, plus one rounding of the result (|d| <= 1).  Two computed distances are compared
    by every "is a maximum / is a minimum" rule, hence 2 E there."""
    return D * U * 0.5 * xn * zn + U


E = bound()


def dist64(X, Z):
    return 0.5 * (1.0 - X.double() @ Z.double().t())


# ---- seeding (MS:155-187) ----------------------------------------------------------------------------------------------
def seeding64(X, S, first, forced=None):
    """Farthest-point seeding in float64, d = 0.5 (1 - x.s).  -> dict(idx (S,), best (S,) the float64 first argmax of the step, top
    (S,) the step's maximum of the nearest-seed distance, pick (S,) the nearest-seed distance of the index taken, margin (S,) = top1 -
    top2 of the step; entry 0 is unused).  ``forced``: take these indices instead of the argmax (the replay of a kernel's picks); the
    statistics stay those of the float64 distances."""
    Xd = X.double()
    n = Xd.shape[0]
    idx, best = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64)
    top, pick, margin = np.zeros(S), np.zeros(S), np.full(S, np.inf)
    idx[0] = best[0] = first
    nearest = torch.full((n,), float("inf"), dtype=torch.float64)
    for i in range(1, S):
        nearest = torch.minimum(nearest, 0.5 * (1.0 - Xd @ Xd[idx[i - 1]]))
        b = int(torch.argmax(nearest))                          # first maximum, like torch.argmax in the reference
        best[i], top[i] = b, float(nearest[b])
        if n > 1:
            two = torch.topk(nearest, 2).values
            margin[i] = float(two[0] - two[1])
        idx[i] = b if forced is None else int(forced[i])
        pick[i] = float(nearest[idx[i]])
    return dict(idx=idx, best=best, top=top, pick=pick, margin=margin)


@functools.lru_cache(maxsize=None)
def seeds64(case):
    """The float64 seeding of the case from its first index (cached)."""
    return seeding64(planted(case)[0], _spec(case)[3], first_index(case))


# ---- hill climb (MS:26, 90-107) ----------------------------------------------------------------------------------------
def _hill(X, Z, kappa, iters):
    for _ in range(iters):
        Z = torch.nn.functional.normalize(torch.exp(kappa * (Z @ X.t())) @ X, dim=1)
    return Z


def hill64(X, Z, kappa=KAPPA, iters=ITERS):
    return _hill(X.double(), Z.double(), kappa, iters)


def hill32(X, Z, kappa=KAPPA, iters=ITERS):
    """The same definition in plain fp32 on the CPU: the yardstick of what fp32 arithmetic costs on these inputs."""
    return _hill(X.float(), Z.float(), kappa, iters)


def far_seed(X):
    """-normalize(mean(X)): no data point, and on the far side of all of them (dots -0.9 ... 0.07), so every weight of this seed is
    far below the other seeds' weights."""
    return torch.nn.functional.normalize(-X.double().mean(dim=0), dim=0).float()


@functools.lru_cache(maxsize=None)
def hill_case(case, iters):
    """-> dict(Z0 (S,64) fp32: the float64 seeding's seeds, the last replaced by far_seed when S > 1; Z64; Z32; err32 = max
    |Z32 - Z64|; err32_far: the same of the far seed's row (0.0 when S = 1))."""
    X, _ = planted(case)
    S = CASES[case][3]
    Z0 = X[torch.from_numpy(seeds64(case)["idx"])].clone()
    if S > 1:
        Z0[-1] = far_seed(X)
    Z0 = Z0.contiguous()
    Z64, Z32 = hill64(X, Z0, KAPPA, iters), hill32(X, Z0, KAPPA, iters)
    d = (Z32.double() - Z64).abs()
    return dict(Z0=Z0, Z64=Z64, Z32=Z32, err32=float(d.max()), err32_far=float(d[-1].max()) if S > 1 else 0.0)


def hill_bound(err32):
    """max(4 err32, 2^-22): four times what the definition costs in fp32 on the CPU (the factor of the Euclidean test: two for the
    kernel's other summation order, two for v_exp_f32 against expf), never below two ulps of a coordinate of magnitude 1."""
    return max(4.0 * err32, 2.0 ** -22)


@functools.lru_cache(maxsize=None)
def hill_case_bf16(case, iters):
    """float64 on the bf16-ROUNDED points (what the "bf16" climb is given), from the Z0 of hill_case -> Z64."""
    return hill64(planted_bf16(case), hill_case(case, iters)["Z0"], KAPPA, iters)


def launch_widths(S, cap=8):
    """Seed blocks per hill-climb launch for S seeds, the host's rule (equal chunks of at most ``cap`` blocks)."""
    nsb = -(-S // 16)
    ch = -(-nsb // -(-nsb // cap))
    return [min(ch, nsb - b) for b in range(0, nsb, ch)]


EUCLID_LIMIT = 4             # the case of ms_euclid_cases that the walk over the seed-block counts extends to S = 304


@functools.lru_cache(maxsize=None)
def euclid_limit_case():
    """Case EUCLID_LIMIT of ms_euclid_cases (n = 5000, rows of norm 2) with 304 seeds, the last one that module's far seed, one
    iteration -> dict(X, Z0, Z64, err32) by that module's float64 and fp32 definitions."""
    import ms_euclid_cases as L2
    X, _ = L2.planted(EUCLID_LIMIT)
    sel = L2.seeding64(X, 304, L2.first_index(EUCLID_LIMIT))["idx"]
    Z0 = X[torch.from_numpy(sel)].clone()
    Z0[-1] = L2.far_seed(EUCLID_LIMIT)
    Z0 = Z0.contiguous()
    Z64, _ = L2.hill64(X, Z0, L2.KAPPA, 1)
    Z32, _ = L2.hill32(X, Z0, L2.KAPPA, 1)
    return dict(X=X, Z0=Z0, Z64=Z64, err32=float((Z32.double() - Z64).abs().max()))


# ---- merge, assignment, the whole clustering (MS:41-76, 192-229) -------------------------------------------------------
def eps_margin(Z, eps=EPS):
    """min over seed pairs of |0.5 (1 - z_i.z_j) - eps|: how far the merge is from depending on rounding."""
    return float((dist64(Z, Z) - eps).abs().min())


def relabel_largest_zero(labels, num):
    """MS:211-227 on a copy: label 0 <-> the first-argmax label among 0 .. num - 1."""
    labels = labels.clone()
    count = torch.bincount(labels, minlength=num)[:num]
    lmax = int(torch.argmax(count))
    if lmax != 0:
        a, b = labels == 0, labels == lmax
        labels[a] = lmax
        labels[b] = 0
    return labels


def same_partition(labels, ids):
    """labels and ids split the points into the same sets (the names of the sets are free)."""
    labels, ids = torch.as_tensor(labels).long().reshape(-1), torch.as_tensor(ids).long().reshape(-1)
    pairs = torch.unique(torch.stack([labels, ids]), dim=1)
    return pairs.shape[1] == torch.unique(labels).numel() == torch.unique(ids).numel()


@functools.lru_cache(maxsize=None)
def smart_init64(case):
    """mean_shift_smart_init in float64 -> dict(sel, Z, seed_labels, labels)."""
    from oracle import msm_oracle as O
    X, _ = planted(case)
    sel = torch.from_numpy(seeds64(case)["idx"])
    Z = hill64(X, X[sel], KAPPA, ITERS)
    seed_labels = O.connected_components(Z, EPS)
    labels = seed_labels[torch.argmin(dist64(X, Z), dim=1)]
    return dict(sel=sel, Z=Z, seed_labels=seed_labels, labels=relabel_largest_zero(labels, len(torch.unique(seed_labels))))


def assign_check(X, Z, taken, xn=1.0):
    """The float64 view of an assignment ``taken`` (n,) of seed indices: -> dict(admissible: every taken seed is within 2 E of the
    float64 minimum; exact: wherever the float64 runner-up is more than 2 E away the taken seed is the float64 argmin; ambiguous: the
    share of points whose runner-up is within 2 E)."""
    d = dist64(X, Z)
    tol = 2 * bound(xn, xn)
    taken = torch.as_tensor(taken).long().reshape(-1, 1)
    two = torch.topk(d, min(2, d.shape[1]), dim=1, largest=False).values
    clear = (two[:, 1] - two[:, 0] > tol) if d.shape[1] > 1 else torch.ones(d.shape[0], dtype=torch.bool)
    admissible = d.gather(1, taken)[:, 0] <= two[:, 0] + tol
    exact = taken[:, 0][clear] == torch.argmin(d, dim=1)[clear]
    return dict(admissible=bool(admissible.all()), exact=bool(exact.all()), ambiguous=float((~clear).float().mean()),
                bad=int((~admissible).sum()) + int((~exact).sum()))


# Copies of seed rows on later rows of the S = 304 case: (2 -> 5) the same seed block, another lane; (3 -> 19) the same lane, the
# next seed block; (7 -> 135) the same lane and block position, the next chunk of eight blocks.
TIES = ((2, 5), (3, 19), (7, 135))


@functools.lru_cache(maxsize=None)
def tie_seeds():
    """-> Z (304,64): the raw seeds of the S = 304 case with the rows of TIES copied bit for bit."""
    X, _ = planted(LIMIT)
    Z = X[torch.from_numpy(seeds64(LIMIT)["idx"])].clone()
    for src, dst in TIES:
        Z[dst] = Z[src]
    return Z.contiguous()


@functools.lru_cache(maxsize=None)
def behind_seeds(case):
    """-> Z (S,64): distinct seeds that most points have BEHIND them (x.z < 0, distance above 0.5): normalize(0.2 x_s - m), m the
    mean direction of the map.  The kernel pads its seed tile with zero rows, whose distance would be exactly 0.5: for these seeds a
    padding row wins unless it is masked out by its index."""
    X, _ = planted(case)
    m = -far_seed(X).double()
    Z = torch.nn.functional.normalize(0.2 * X[torch.from_numpy(seeds64(case)["idx"])].double() - m, dim=1)
    return Z.float().contiguous()
