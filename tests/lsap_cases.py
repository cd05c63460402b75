"""The assignment problems that the CPU guard (test_lsap_cases_cpu.py) and the GPU test (test_gpu_lsap.py) share.  Problems are
grouped by Q, because one msm_lsap_match launch shares Q; every group runs with n_pred = 2 (a seed per prediction).

The groups cover T < Q, T = Q, T > Q, T = 0, T = 1, the 64-lane edge of the kernel's scan on both sides (63 / 64 / 65 columns or
rows), more than one 64-column chunk (100, 129, 300) and the 300-query configuration."""
import numpy as np

GROUPS = [
    (100, (8, 1, 0, 17, 100, 64, 3)),
    (5, (9, 5, 1, 0, 4)),
    (64, (64, 63, 65)),
    (65, (3, 64)),
    (1, (1, 3)),
    (129, (17,)),
    (300, (40, 1)),
]
KINDS = ("normal", "ties", "inf")
N_PRED = 2


def toff_of(T):
    return [0] + np.cumsum(T).astype(int).tolist()


def make_cost(Q, T, kind, seed):
    """(N_PRED, Q, sum T) float32: image b's matrix is columns toff[b] .. toff[b + 1].
    normal: 3 randn rounded to fp32; ties: integers in {0, 1, 2}; inf: normal with about 5 % of every matrix at +inf, one
    finite band kept (entry (q, t) with t = q mod T_b ... q = t mod Q), so that every assignment problem stays feasible."""
    rng = np.random.default_rng(seed)
    TT = int(sum(T))
    if kind == "ties":
        return rng.integers(0, 3, size=(N_PRED, Q, TT)).astype(np.float32)
    cost = (3.0 * rng.standard_normal((N_PRED, Q, TT))).astype(np.float32)
    if kind == "inf":
        toff = toff_of(T)
        for b, t in enumerate(T):
            if t == 0:
                continue
            hole = rng.random((N_PRED, Q, t)) < 0.05
            q, j = np.arange(Q)[:, None], np.arange(t)[None, :]
            keep = (q % t == j) | (j % Q == q)          # a perfect matching of the smaller side stays finite
            hole &= ~keep[None]
            block = cost[:, :, toff[b]:toff[b + 1]]
            block[hole] = np.inf
    return cost


def cases():
    """(Q, T, kind, seed) of every launch."""
    out = []
    for g, (Q, T) in enumerate(GROUPS):
        for k, kind in enumerate(KINDS):
            out.append((Q, T, kind, 1000 + 10 * g + k))
    return out


def case_id(case):
    Q, T, kind, _ = case
    return f"Q{Q}-{kind}"


def labels_of(T, seed):
    """(sum T,) int32 classes in [0, 7)."""
    return np.random.default_rng(seed + 5).integers(0, 7, size=int(sum(T))).astype(np.int32)


def reference(cost, T, Q, labels, no_object, solver):
    """What msm_lsap_match must write for `cost` when every problem is solved by `solver` (a function cost matrix -> (rows,
    cols)): pairs (N_PRED * N, 4) int32 and target_classes (N_PRED, B, Q) int64."""
    toff = toff_of(T)
    n_pred, B = cost.shape[0], len(T)
    N = sum(min(Q, t) for t in T)
    pairs = np.zeros((n_pred * N, 4), np.int32)
    tc = np.full((n_pred, B, Q), no_object, np.int64)
    for p in range(n_pred):
        n = 0
        for b in range(B):
            i, j = solver(cost[p, :, toff[b]:toff[b + 1]])
            assert len(i) == min(Q, T[b]) and (np.diff(i) > 0).all()
            for q, t in zip(i.tolist(), j.tolist()):
                pairs[p * N + n] = (p, n, b * Q + q, toff[b] + t)
                tc[p, b, q] = labels[toff[b] + t]
                n += 1
        assert n == N
    return pairs, tc
