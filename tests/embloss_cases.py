"""Cases, seeded inputs and the float64 definition of EmbeddingLoss (lib/networks/embedding.py:57-133; the restatement on
per-(image, cluster) sums that include/msm_hip.h documents for msm_embloss_fwd / _bwd).

Used by tests/golden/make_golden_embedding_loss.py (which runs the reference's own module on these inputs),
tests/test_embloss_cases_cpu.py and tests/test_gpu_embedding_loss.py.  Everything here runs on the CPU; the float64 results are
computed once per case and shared (callers must not modify them).

Inputs are planted: a unit prototype per cluster plus sigma * N(0, I) / sqrt(C) noise, renormalised where ``normalize``, on label
maps made of 4 x 4 blocks; about 10 % of the pixels are unlabelled (-1).  Every labelled pixel keeps |d_p - alpha| >= MARGIN (a
pixel that does not is re-labelled -1), so the hard-negative counts N_bk are the same in fp32 and in float64."""
import collections
import functools

import torch

ALPHA = 0.02                 # cfg.TRAIN.EMBEDDING_ALPHA
DELTA = 0.5                  # cfg.TRAIN.EMBEDDING_DELTA
LAMBDA_INTRA = 1.0
LAMBDA_INTER = 2.0           # not the reference's 1.0: a weight of 1 would hide a missing factor
MARGIN = 1e-4
GRAD_WEIGHTS = (2.0, 3.0, -1.0)      # the gradient under test is that of 2 loss + 3 intra - inter

Case = collections.namedtuple("Case", "B C H W K metric normalize delta sigma seed special")
# name -> case.  What each one reaches:
#   0   ragged H W (943: no multiple of 64 or 4), cluster 1 empty in every image, N_bk above and below 50
#   1   K = 1 (no inter term), odd C, less than one workgroup
#   2   un-normalised centres, Euclidean
#   3   Euclidean inter term > 0 (delta = 1.5; at 0.5 unit centres are never that close)
#   4   the table at the LDS limit (64 x 256), every N_bk < 50
#   5   several workgroups and several rounds per workgroup; image 1 entirely -1; image 2 holds label 0 only
#   6   sigma = 0: no pixel beyond alpha, the zero-intra branch, gradient from the inter term alone; 6k1: K = 1, everything 0
#   7i  case 0 with int64 labels; 7s: case 0 with a 3 x 3 patch of label 2.5 (labelled pixels of no cluster)
CASES = collections.OrderedDict([
    ("0", Case(2, 64, 23, 41, 5, "cosine", True, DELTA, 0.30, 11, "empty1")),
    ("1", Case(1, 7, 9, 13, 1, "cosine", True, DELTA, 0.30, 12, "")),
    ("2", Case(2, 16, 20, 20, 4, "euclidean", False, DELTA, 0.30, 13, "")),
    ("3", Case(2, 64, 23, 41, 5, "euclidean", True, 1.5, 0.30, 14, "empty1")),
    ("4", Case(1, 256, 32, 32, 64, "cosine", True, DELTA, 0.30, 15, "one_block_each")),
    ("5", Case(3, 64, 120, 160, 12, "cosine", True, DELTA, 0.60, 16, "image1_unlabelled,image2_label0")),
    ("6", Case(2, 64, 24, 40, 5, "cosine", True, DELTA, 0.0, 17, "")),
    ("6k1", Case(2, 64, 24, 40, 1, "cosine", True, DELTA, 0.0, 18, "")),
    ("7i", Case(2, 64, 23, 41, 5, "cosine", True, DELTA, 0.30, 11, "empty1,int64")),
    ("7s", Case(2, 64, 23, 41, 5, "cosine", True, DELTA, 0.30, 11, "empty1,stray")),
])
GOLDEN_CASES = ("0", "1", "2", "3", "6", "6k1", "7i", "7s")      # the reference's own results are stored for these
GRAD_SAMPLE = 4096


def checksum(X):
    """float64 sum of X.flat[i] * (1 + i mod 251): what the goldens record instead of X (as ms_euclid_cases.checksum)."""
    w = 1.0 + (torch.arange(X.numel(), dtype=torch.float64) % 251)
    return float((X.double().reshape(-1) * w).sum())


def grad_sample_index(numel):
    """The strided sample of a gradient the goldens store: GRAD_SAMPLE indices spread over the whole tensor."""
    step = max(1, numel // GRAD_SAMPLE)
    return torch.arange(0, numel, step)[:GRAD_SAMPLE]


def definition64(x, labels, case, weights=GRAD_WEIGHTS):
    """The definition in float64 -> dict(loss, intra, inter: floats; grad (B,C,H,W) float64 of weights . (loss, intra, inter);
    K; n, N (B,K) int64; d (B,HW) float64 distances; labelled, stray (B,HW) bool)."""
    B, C, H, W = x.shape
    xf = x.double().reshape(B, C, H * W).clone().requires_grad_(True)
    l = labels.reshape(B, H * W).double()
    K = int(l.max()) + 1
    M = (l[:, None, :] == torch.arange(K, dtype=torch.float64)[None, :, None]).double()          # (B,K,HW)
    n = M.sum(2)
    m = torch.einsum("bkp,bcp->bkc", M, xf) / (n + 1e-10)[..., None]
    mu = m / m.norm(dim=2, keepdim=True).clamp_min(1e-12) if case.normalize else m
    centre = torch.einsum("bkp,bkc->bcp", M, mu)
    labelled = l >= 0
    if case.metric == "cosine":
        d = labelled * (0.5 * (1 - (xf * centre).sum(1)))
        d2 = d ** 2
    else:
        d2 = labelled * ((xf - centre) ** 2).sum(1)          # smooth at d = 0: the gradient is 2 (x - mu), not a quotient
        d = d2.detach().sqrt()
    hard = d.detach() > ALPHA
    N = torch.einsum("bkp,bp->bk", M, hard.double())
    stray = labelled & (M.sum(1) == 0)
    if bool(hard.any()):
        w = torch.einsum("bkp,bk->bp", M, 1.0 / (K * N.clamp_min(50.0))) + stray.double() / (50.0 * K)
        intra = LAMBDA_INTRA / B * (d2 * w).sum()
    else:
        intra = xf.sum() * 0.0
    if K > 1:
        if case.metric == "cosine":
            dist = 0.5 * (1 - torch.einsum("bic,bjc->bij", mu, mu))
        else:
            sq = ((mu[:, :, None, :] - mu[:, None, :, :]) ** 2).sum(-1)
            pos = sq > 0
            dist = torch.where(pos, torch.where(pos, sq, torch.ones_like(sq)).sqrt(), torch.zeros_like(sq))
        h = (case.delta - dist).clamp_min(0.0) * (1 - torch.eye(K, dtype=torch.float64))
        inter = LAMBDA_INTER * (h ** 2).sum() / (K * (K - 1) / 2 * B)
    else:
        inter = xf.sum() * 0.0
    loss = intra + inter
    (grad,) = torch.autograd.grad(weights[0] * loss + weights[1] * intra + weights[2] * inter, xf)
    return dict(loss=float(loss.detach()), intra=float(intra.detach()), inter=float(inter.detach()), grad=grad.reshape(B, C, H, W),
                K=K, n=n.long(), N=N.long(), d=d.detach(), labelled=labelled, stray=stray)


def _label_map(case, g):
    B, H, W, K = case.B, case.H, case.W, case.K
    hb, wb = (H + 3) // 4, (W + 3) // 4
    weights = torch.ones(K)
    if K > 1:
        weights[K - 1] = 0.12                              # a small cluster: N_bk below 50 next to clusters above it
    coarse = torch.multinomial(weights, B * hb * wb, replacement=True, generator=g).reshape(B, hb, wb)
    if "one_block_each" in case.special:                   # 4 x 4 blocks of 16 pixels, cluster k in the k-th block
        coarse = torch.arange(B * hb * wb).reshape(B, hb, wb) % K
    lab = coarse.repeat_interleave(4, 1).repeat_interleave(4, 2)[:, :H, :W].clone().double()
    if "empty1" in case.special:
        lab[lab == 1] = 3
    if "image2_label0" in case.special:
        lab[2] = 0
    lab[torch.rand(B, H, W, generator=g) < 0.10] = -1
    if "image1_unlabelled" in case.special:
        lab[1] = -1
    if "stray" in case.special:
        lab[0, 5:8, 9:12] = 2.5
    return lab.reshape(B, 1, H, W)


@functools.lru_cache(maxsize=None)
def planted(name):
    """-> (x (B,C,H,W) float32, labels (B,1,H,W) float32, or int64 where the case says so)."""
    case = CASES[name]
    B, C, H, W, K = case.B, case.C, case.H, case.W, case.K
    g = torch.Generator().manual_seed(case.seed)
    P = torch.randn(K + 1, C, generator=g, dtype=torch.float64)
    P = P / P.norm(dim=1, keepdim=True)                    # row K: what unlabelled and stray pixels sit around
    lab = _label_map(case, g)
    idx = lab.reshape(B, H, W)
    idx = torch.where((idx >= 0) & (idx == idx.floor()), idx, torch.full_like(idx, K)).long()
    x = P[idx] + case.sigma * torch.randn(B, H, W, C, generator=g, dtype=torch.float64) / C ** 0.5
    if case.normalize:
        x = x / x.norm(dim=3, keepdim=True)
    x = x.permute(0, 3, 1, 2).float().contiguous()
    for _ in range(20):                                    # re-label the pixels whose distance sits at the threshold
        r = definition64(x, lab, case)
        near = r["labelled"] & ((r["d"] - ALPHA).abs() < MARGIN) & ~r["stray"]
        if not bool(near.any()):
            break
        lab = torch.where(near.reshape(lab.shape), torch.full_like(lab, -1.0), lab)
    else:
        raise AssertionError(f"case {name}: the threshold margin did not settle")
    labels = lab.long() if "int64" in case.special else lab.float()
    return x, labels.contiguous()


@functools.lru_cache(maxsize=None)
def reference64(name):
    """definition64 of the case's inputs (shared: do not modify)."""
    x, labels = planted(name)
    return definition64(x, labels, CASES[name])
