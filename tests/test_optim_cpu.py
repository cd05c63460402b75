"""optim.build_param_groups restates the reference's rule (MSMFormer/tabletop_train_net_pretrained.py:113-159): one group per
trainable tensor in traversal order, lr and weight decay by the owning module.  Host only; the constructor's refusals too."""
import pytest
import torch
from torch import nn

from unseenobjectswithmeanshift_amd.optim import FullModelClipAdamW, build_optimizer, build_param_groups


class Backbone(nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = nn.Linear(3, 4)
        self.bn = nn.BatchNorm2d(4)


class Toy(nn.Module):
    def __init__(self):
        super().__init__()
        self.backbone = Backbone()
        self.ln = nn.LayerNorm(4)
        self.gn = nn.GroupNorm(2, 4)
        self.emb = nn.Embedding(5, 4)
        self.head = nn.Linear(4, 2)
        self.tied = nn.Linear(4, 2, bias=False)
        self.tied.weight = self.head.weight                    # one parameter shared by two modules
        self.frozen = nn.Linear(2, 2, bias=False)
        self.frozen.weight.requires_grad_(False)
        self.absolute_pos_embed = nn.Parameter(torch.zeros(1, 4))          # a parameter the reference exempts by name


def test_toy_module_groups_follow_the_reference_rule():
    m = Toy()
    groups = build_param_groups(m, 1e-2, weight_decay=0.05, weight_decay_norm=0.01, weight_decay_embed=0.02, backbone_multiplier=0.1)
    assert all(set(g) == {"params", "lr", "weight_decay"} and len(g["params"]) == 1 for g in groups)
    expected = [                                               # named_modules() order: the root's own parameters first
        (m.absolute_pos_embed, 1e-2, 0.0),
        (m.backbone.fc.weight, 1e-3, 0.05), (m.backbone.fc.bias, 1e-3, 0.05),
        (m.backbone.bn.weight, 1e-3, 0.01), (m.backbone.bn.bias, 1e-3, 0.01),
        (m.ln.weight, 1e-2, 0.01), (m.ln.bias, 1e-2, 0.01),
        (m.gn.weight, 1e-2, 0.01), (m.gn.bias, 1e-2, 0.01),
        (m.emb.weight, 1e-2, 0.02),
        (m.head.weight, 1e-2, 0.05), (m.head.bias, 1e-2, 0.05),
    ]
    assert len(groups) == len(expected)
    for g, (p, lr, wd) in zip(groups, expected):
        assert g["params"][0] is p
        assert g["lr"] == pytest.approx(lr, rel=1e-12) and g["weight_decay"] == wd
    got = [g["params"][0] for g in groups]
    assert sum(p is m.head.weight for p in got) == 1           # shared: once
    assert not any(p is m.frozen.weight for p in got)          # frozen: absent


def test_resnet50_head_has_298_groups_and_decays_all_but_norms_and_embeddings():
    from unseenobjectswithmeanshift_amd.meta_arch import build_resnet50_head
    head = build_resnet50_head()
    groups = build_param_groups(head, 1e-4)
    assert len(groups) == 298
    assert sum(g["params"][0].numel() for g in groups) == sum(p.numel() for p in head.parameters() if p.requires_grad)
    no_decay = set()
    for mod in head.modules():
        if isinstance(mod, (nn.GroupNorm, nn.LayerNorm, nn.BatchNorm2d, nn.Embedding)):
            no_decay.update(id(p) for p in mod.parameters(recurse=False))
    assert no_decay
    assert {id(g["params"][0]) for g in groups if g["weight_decay"] == 0.0} == no_decay
    assert all(g["weight_decay"] == 0.05 for g in groups if id(g["params"][0]) not in no_decay)
    assert all(g["lr"] == 1e-4 for g in groups)                # the head has no backbone


def test_build_optimizer_is_the_two_together():
    m = Toy()
    opt = build_optimizer(m, base_lr=2e-3, max_norm=0.5)
    assert isinstance(opt, FullModelClipAdamW) and isinstance(opt, torch.optim.Optimizer)
    assert opt.max_norm == 0.5 and len(opt.param_groups) == 12
    ref = build_param_groups(m, 2e-3)
    assert [(g["lr"], g["weight_decay"]) for g in opt.param_groups] == [(g["lr"], g["weight_decay"]) for g in ref]
    torch_keys = set(torch.optim.AdamW([nn.Parameter(torch.zeros(1))]).param_groups[0])
    assert set(opt.param_groups[0]) == torch_keys             # a state dict of either loads into the other
    assert opt.param_groups[0]["betas"] == (0.9, 0.999) and opt.param_groups[0]["eps"] == 1e-8


def test_a_scheduler_drives_the_learning_rate():
    opt = FullModelClipAdamW([nn.Parameter(torch.zeros(3))], lr=1.0)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda epoch: 0.5)
    assert opt.param_groups[0]["lr"] == 0.5 and sched.get_last_lr() == [0.5]


@pytest.mark.parametrize("kwargs, offender", [({"amsgrad": True}, "amsgrad"), ({"maximize": True}, "maximize")])
def test_unsupported_variants_raise_and_are_named(kwargs, offender):
    with pytest.raises(NotImplementedError, match=offender):
        FullModelClipAdamW([nn.Parameter(torch.zeros(3))], **kwargs)


@pytest.mark.parametrize("dtype", [torch.float64, torch.bfloat16, torch.float16])
def test_a_parameter_that_is_not_float32_raises(dtype):
    with pytest.raises(NotImplementedError, match=str(dtype).replace(".", r"\.")):
        FullModelClipAdamW([nn.Parameter(torch.zeros(3)), nn.Parameter(torch.zeros(2, 2, dtype=dtype))])


def test_a_parameter_that_is_not_contiguous_raises():
    with pytest.raises(RuntimeError, match="contiguous"):
        FullModelClipAdamW([nn.Parameter(torch.zeros(4, 3).t())])


def test_a_host_tensor_raises_the_gpu_error_at_step():
    p = nn.Parameter(torch.zeros(3))
    opt = FullModelClipAdamW([p], lr=1e-2)
    p.grad = torch.ones(3)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        opt.step()
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        opt.zero_grad(set_to_none=False)
    assert torch.equal(p.detach(), torch.zeros(3)) and p not in opt.state


def test_a_closure_raises():
    opt = FullModelClipAdamW([nn.Parameter(torch.zeros(3))])
    with pytest.raises(NotImplementedError, match="closure"):
        opt.step(lambda: 0.0)
