"""EmbeddingLoss: the clustering loss of the UCN embedding network (lib/networks/embedding.py:57-133, byte-identical in
MSMFormer/meanshiftformer/embedding.py) on the fused HIP kernels of csrc/embedding_loss.hip.

The reference loops over the K clusters four times with full (B,C,H,W) temporaries that autograd keeps, and reads K back with
``.item()``.  Here the arithmetic is collapsed to per-(image, cluster) sums (the definition is in include/msm_hip.h): the forward
reads x twice, the backward reads it once and writes grad_x once, and nothing waits for the GPU -- K is found on the device.
What the reference would silently compute with any number of clusters, the kernels compute with a table of ``max_clusters``
rows in LDS: a label beyond it is treated as a pixel of no cluster and recorded in ``last_status``; ``check()`` reads that word
(the only synchronisation) and raises, like ``SetCriterion.check_matching()``.

No CPU path and no fallback: x must be float32 on the GPU.
"""
import torch
from torch import nn

from . import ops


class _EmbeddingLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, labels, alpha, delta, lambda_intra, lambda_inter, metric, normalize, max_clusters, workspace):
        losses, info, workspace = ops.embloss_fwd(x, labels, alpha, delta, lambda_intra, lambda_inter, metric, normalize,
                                                  max_clusters, workspace)
        ctx.save_for_backward(x, labels, workspace)
        ctx.metric, ctx.max_clusters = metric, max_clusters
        ctx.mark_non_differentiable(info)
        return losses, info

    @staticmethod
    def backward(ctx, g_losses, _g_info):
        x, labels, workspace = ctx.saved_tensors
        grad_x = ops.embloss_bwd(x, labels, g_losses.to(torch.float32).contiguous(), workspace, ctx.metric, ctx.max_clusters)
        return (grad_x,) + (None,) * 9


class EmbeddingLoss(nn.Module):
    """``EmbeddingLoss(alpha, delta, lambda_intra, lambda_inter, metric='cosine', normalize=True)`` as in the reference, plus
    ``max_clusters`` (keyword only; default min(64, 16384 // C)): the rows of the cluster table, ``max_clusters * C <= 16384``.

    ``forward(x, cluster_masks) -> (loss, intra_cluster_loss, inter_cluster_loss)``, 0-d tensors; any combination of the three
    may be backpropagated.  x (B,C,H,W) float32 on the GPU (made contiguous when it is not), cluster_masks (B,1,H,W) float or
    integer, -1 = unlabelled.  ``workspace``: a uint8 tensor of ``ops.embloss_workspace_bytes`` bytes that a caller capturing the
    step in a HIP graph owns; the backward reads it, so it serves one forward / backward pair at a time.
    ``last_status`` is the device status word of the last call (0-d int32), ``last_info`` the device counts (K, n, N)."""

    def __init__(self, alpha, delta, lambda_intra, lambda_inter, metric='cosine', normalize=True, *, max_clusters=None):
        super().__init__()
        if metric not in ops.EMBLOSS_METRICS:
            raise ValueError(f"EmbeddingLoss: metric must be 'cosine' or 'euclidean', got {metric!r}")
        self.alpha = alpha
        self.delta = delta
        self.lambda_intra = lambda_intra
        self.lambda_inter = lambda_inter
        self.metric = metric
        self.normalize = normalize
        self.max_clusters = max_clusters
        self.last_status = None
        self.last_info = None

    def forward(self, x, cluster_masks, workspace=None):
        if x.dim() != 4:
            raise RuntimeError(f"EmbeddingLoss: x must be (B,C,H,W), got {tuple(x.shape)}")
        max_clusters = ops.embloss_max_clusters(x.shape[1], self.max_clusters)
        if x.dtype != torch.float32:
            raise RuntimeError(f"EmbeddingLoss: x must be torch.float32, got {x.dtype}")
        if not x.is_cuda or not cluster_masks.is_cuda:
            raise RuntimeError("EmbeddingLoss: x and cluster_masks must be on the GPU (there is no CPU path)")
        labels = cluster_masks.detach().to(torch.float32).contiguous()
        losses, info = _EmbeddingLossFn.apply(x.contiguous(), labels, self.alpha, self.delta, self.lambda_intra,
                                              self.lambda_inter, self.metric, self.normalize, max_clusters, workspace)
        self.last_info = ops.embloss_info(info, x.shape[0])
        self.last_status = self.last_info["status"]
        return losses[0], losses[1], losses[2]      # autograd sums whatever is backpropagated into the (3,) gradient

    def check(self):
        """Raise ValueError if the last call met a label the cluster table could not hold (its pixels were treated as pixels of
        no cluster, so the losses of that call are not the reference's).  Synchronises: it reads ``last_status``."""
        if self.last_status is None:
            return
        if int(self.last_status.cpu()) & 1:
            raise ValueError(f"EmbeddingLoss: a label >= max_clusters = {self.last_info['n'].shape[1]} was met; "
                             "construct the loss with a larger max_clusters (max_clusters * C <= 16384)")
