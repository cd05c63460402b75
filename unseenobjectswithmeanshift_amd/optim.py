"""The reference's optimizer (Trainer.build_optimizer, MSMFormer/tabletop_train_net_pretrained.py:113-191) on the HIP kernels of
csrc/optimizer.hip: AdamW with one param group per tensor behind ``clip_grad_norm_`` over the whole model.

The reference decides lr and weight decay per module, so every parameter tensor is a group of its own (298 for the ResNet-50 head,
125 for the RGB-D head), and every ``step()`` first clips the gradient of the whole model to ``CLIP_VALUE`` 0.01.  torch runs that as
a dozen small launches per tensor (a launch per group even with ``fused=True``).  Here a step is two launches over a device-resident
table, whatever the number of tensors: the squared norm of every chunk of every gradient, then the clip coefficient and the AdamW
update per chunk (the definition is in include/msm_hip.h).  Nothing in ``step()`` waits for the GPU.

    optimizer = build_optimizer(model.sem_seg_head, base_lr=1e-4)       # = FullModelClipAdamW(build_param_groups(...), ...)
    sum(losses.values()).backward(); optimizer.step(); optimizer.zero_grad()

No CPU path and no fallback: parameters and gradients are contiguous float32 tensors on one GPU.
"""
import operator

import numpy as np
import torch
from torch import nn

from . import ops

NORM_MODULE_TYPES = (                      # tabletop_train_net_pretrained.py:121-133
    nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d, nn.SyncBatchNorm, nn.GroupNorm, nn.InstanceNorm1d, nn.InstanceNorm2d,
    nn.InstanceNorm3d, nn.LayerNorm, nn.LocalResponseNorm)


def build_param_groups(model, base_lr, weight_decay=0.05, weight_decay_norm=0.0, weight_decay_embed=0.0, backbone_multiplier=0.1):
    """The reference's param groups (:135-159): one ``{"params": [tensor], "lr", "weight_decay"}`` per trainable parameter tensor, in
    the order of ``named_modules()`` / ``named_parameters(recurse=False)``, a shared parameter once.  A module whose name holds
    "backbone" trains at ``base_lr * backbone_multiplier``; ``relative_position_bias_table`` / ``absolute_pos_embed`` parameters get
    weight decay 0, the parameters of normalisation modules ``weight_decay_norm``, those of ``nn.Embedding`` ``weight_decay_embed``
    (the later rule wins, as in the reference).  Defaults: SOLVER.WEIGHT_DECAY 0.05, WEIGHT_DECAY_NORM 0.0, WEIGHT_DECAY_EMBED 0.0,
    BACKBONE_MULTIPLIER 0.1 of every shipped config.  Host only."""
    groups, memo = [], set()
    for module_name, module in model.named_modules():
        for param_name, value in module.named_parameters(recurse=False):
            if not value.requires_grad or value in memo:
                continue
            memo.add(value)
            lr, wd = base_lr, weight_decay
            if "backbone" in module_name:
                lr = lr * backbone_multiplier
            if "relative_position_bias_table" in param_name or "absolute_pos_embed" in param_name:
                wd = 0.0
            if isinstance(module, NORM_MODULE_TYPES):
                wd = weight_decay_norm
            if isinstance(module, nn.Embedding):
                wd = weight_decay_embed
            groups.append({"params": [value], "lr": lr, "weight_decay": wd})
    return groups


_HYPER = operator.itemgetter("lr", "weight_decay", "betas", "eps", "amsgrad", "maximize")
_DATA_PTR = torch.Tensor.data_ptr


class _Slot:
    """One pinned staging buffer and the event behind its last copy."""

    def __init__(self, words):
        self.buf = torch.empty(words, dtype=torch.int64).pin_memory()
        self.i64 = self.buf.numpy()
        self.f64 = self.i64.view(np.float64)
        self.event = None


class FullModelClipAdamW(torch.optim.Optimizer):
    """``torch.optim.AdamW`` behind ``torch.nn.utils.clip_grad_norm_(all parameters, max_norm)``, two launches per ``step()``.

    ``params``, ``lr``, ``betas``, ``eps``, ``weight_decay`` and ``param_groups`` are torch's: a scheduler that writes
    ``group["lr"]`` works unchanged, and ``state_dict()`` / ``load_state_dict()`` are interchangeable with ``torch.optim.AdamW`` over
    the same groups (per parameter ``step``, ``exp_avg``, ``exp_avg_sq``).  ``max_norm <= 0`` turns the clipping off.  A parameter
    whose ``.grad`` is None is left out of the step as torch leaves it out: no norm contribution, no state change, no step count.

    The host keeps what it last uploaded -- the hyper-parameters of every group and the addresses of every parameter and
    gradient -- and uploads again, in one asynchronous copy from pinned staging, only when one of them changed: a scheduler's lr
    (the 64-byte rows alone), a gradient reallocated after ``zero_grad(set_to_none=True)`` or a parameter without a gradient (the
    whole table).  ``uploads`` counts the copies.  ``step()`` copies nothing back, never synchronises and allocates nothing after
    the first call with a given set of gradients; ``zero_grad(set_to_none=False)`` is one launch over the same table.
    ``last_grad_norm`` / ``last_clip_coef``: 0-d float32 device tensors (views of the kernels' state block) of the last step, the
    norm before clipping; None before the first step, and with ``max_norm <= 0`` the norm is not computed and reads 0.
    Everything is issued on the stream that is current when ``step()`` is called; use one stream for the steps of one optimizer.

    Not supported (NotImplementedError): ``amsgrad``, ``maximize``, a ``closure``, parameters other than float32;
    RuntimeError: host tensors, non-contiguous parameters or gradients, parameters on several devices."""

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 max_norm=0.01):
        if amsgrad:
            raise NotImplementedError("FullModelClipAdamW: amsgrad=True is not supported")
        if maximize:
            raise NotImplementedError("FullModelClipAdamW: maximize=True is not supported")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid betas: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        # the keys of torch.optim.AdamW's own groups, so that a state dict of either loads into the other and then steps
        defaults = dict(torch.optim.AdamW([torch.zeros(1)]).defaults)
        defaults.update(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False)
        self.max_norm = float(max_norm)
        self.uploads = 0
        self.last_grad_norm = None
        self.last_clip_coef = None
        self._calls = 0                 # value of the device call counter once everything issued has run
        self._params = None             # flat parameter list; everything below is built from it at the first step
        super().__init__(params, defaults)

    # ---- layout: what depends on the parameter list alone ----
    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        for p in self.param_groups[-1]["params"]:
            if p.dtype != torch.float32:
                raise NotImplementedError(f"FullModelClipAdamW: parameter of shape {tuple(p.shape)} is {p.dtype}; only torch.float32 "
                                          "parameters are supported")
            if not p.is_contiguous():
                raise RuntimeError(f"FullModelClipAdamW: parameter of shape {tuple(p.shape)} is not contiguous")
        if getattr(self, "_params", None) is not None:
            self._layout(keep_offsets=True)

    def _layout(self, keep_offsets=False):
        old = dict(zip(map(id, self._params), self._off)) if keep_offsets else {}
        params = [p for g in self.param_groups for p in g["params"]]
        for p in params:
            if not p.is_cuda:
                raise RuntimeError(f"FullModelClipAdamW: parameter of shape {tuple(p.shape)} must be on the GPU (no CPU path in "
                                   "unseenobjectswithmeanshift_amd)")
            if p.device != params[0].device:
                raise RuntimeError(f"FullModelClipAdamW: parameters on {params[0].device} and {p.device}; one optimizer serves one GPU")
            if p.numel() == 0:
                raise RuntimeError("FullModelClipAdamW: a parameter without elements")
        self._params = params
        self._off = [old.get(id(p), self._calls) for p in params]           # step of parameter i = calls - off[i]
        self._group_of = [gi for gi, g in enumerate(self.param_groups) for _ in g["params"]]
        chunk = self.chunk = ops.optim_chunk()
        self._chunk_offsets = [np.arange(0, p.numel(), chunk, dtype=np.int64) for p in params]
        T, C = len(params), sum(len(o) for o in self._chunk_offsets)
        dev = params[0].device
        self._device = dev
        self._hyp0, self._rec0, self._chk0 = 0, T * ops.OPTIM_HYP, T * ops.OPTIM_HYP + T * ops.OPTIM_REC
        self._words = self._chk0 + 2 * C
        self._table = torch.zeros(self._words, dtype=torch.int64, device=dev)
        self._hyper_dev = self._table[:self._rec0].view(torch.float64)
        self._rec_dev = self._table[self._rec0:self._chk0]
        self._chk_dev = self._table[self._chk0:]
        self._partials = torch.zeros(C, dtype=torch.float64, device=dev)
        if getattr(self, "_state_dev", None) is None or self._state_dev.device != dev:
            self._state_dev = torch.zeros(2, dtype=torch.int64, device=dev)
            self._state_dev[0] = self._calls
            f = self._state_dev.view(torch.float32)
            self.last_grad_norm, self.last_clip_coef = f[2], f[3]
        self._slots = [_Slot(self._words), _Slot(self._words)]
        self._hyper_key = self._table_key = None
        self._present, self._absent = [], []
        self._n_tensors = self._n_chunks = 0

    # ---- host mirror and upload ----
    def _free_slot(self):
        for s in self._slots:
            if s.event is None or s.event.query():
                return s
        s = _Slot(self._words)              # every copy is still in flight: the host runs that far ahead of the GPU
        self._slots.append(s)
        return s

    def _upload(self, slot, words):
        self._table[:words].copy_(slot.buf[:words], non_blocking=True)
        if slot.event is None:
            slot.event = torch.cuda.Event()
        slot.event.record()
        self.uploads += 1

    def _hyper_rows(self, key):
        for gi, (lr, wd, betas, eps, amsgrad, maximize) in enumerate(key):
            if amsgrad or maximize:
                raise NotImplementedError(f"FullModelClipAdamW: param group {gi} sets {'amsgrad' if amsgrad else 'maximize'}")
            if isinstance(lr, torch.Tensor) or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
                raise ValueError(f"FullModelClipAdamW: param group {gi}: lr must be a Python float and betas in [0, 1), got "
                                 f"{type(lr).__name__}, {betas}")
        per_group = np.array([(lr, wd, betas[0], betas[1], eps) for lr, wd, betas, eps, _, _ in key], dtype=np.float64)
        rows = np.zeros((len(self._params), ops.OPTIM_HYP), dtype=np.float64)
        rows[:, :5] = per_group[self._group_of]
        rows[:, 5] = self._off
        return rows.ravel()

    def _records(self, gptrs):
        """The tensor records and the chunk list of the parameters that have a gradient; creates their state."""
        present = [i for i, g in enumerate(gptrs) if g]
        rec = np.zeros((len(present), ops.OPTIM_REC), dtype=np.int64)
        for t, i in enumerate(present):
            p = self._params[i]
            g = p.grad
            if not g.is_cuda or g.device != self._device:
                raise RuntimeError(f"FullModelClipAdamW: the gradient of parameter {i} must be on the GPU ({self._device}), got {g.device}")
            if g.dtype != torch.float32 or g.is_sparse:
                raise NotImplementedError(f"FullModelClipAdamW: the gradient of parameter {i} is {g.dtype}"
                                          f"{' (sparse)' if g.is_sparse else ''}; only dense torch.float32 is supported")
            if not p.is_contiguous() or not g.is_contiguous():
                raise RuntimeError(f"FullModelClipAdamW: parameter {i} of shape {tuple(p.shape)} or its gradient is not contiguous")
            st = self.state[p]
            if "exp_avg" not in st:
                st["step"] = torch.tensor(0.0)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                self._off[i] = self._calls
            m, v = st["exp_avg"], st["exp_avg_sq"]
            for name, s in (("exp_avg", m), ("exp_avg_sq", v)):
                if s.dtype != torch.float32 or s.device != self._device or s.shape != p.shape or not s.is_contiguous():
                    raise RuntimeError(f"FullModelClipAdamW: state {name} of parameter {i} must be a contiguous float32 tensor of shape "
                                       f"{tuple(p.shape)} on {self._device}")
            ptrs = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr())
            flags = (ops.OPTIM_ALIGNED if all(a % 16 == 0 for a in ptrs) else 0) | (ops.OPTIM_ALIGNED_G if ptrs[1] % 16 == 0 else 0)
            rec[t] = (*ptrs, p.numel(), i, flags, 0)
        chunks = np.empty((sum(len(self._chunk_offsets[i]) for i in present), 2), dtype=np.int64)
        at = 0
        for t, i in enumerate(present):
            o = self._chunk_offsets[i]
            chunks[at:at + len(o), 0] = t
            chunks[at:at + len(o), 1] = o
            at += len(o)
        return present, rec, chunks

    def _prepare(self):
        """Bring the device table up to date with the param groups, the parameters and their gradients: at most one upload."""
        if self._params is None:
            self._layout()
        params = self._params
        hyper_key = list(map(_HYPER, self.param_groups))                # ~0.1 ms of Python per step for 298 groups: no
        gptrs = [0 if g is None else g.data_ptr() for g in [p.grad for p in params]]      # per-group work beyond these lines
        table_key = (gptrs, list(map(_DATA_PTR, params)))
        if table_key != self._table_key:
            present, rec, chunks = self._records(gptrs)
            seen = set(present)
            slot = self._free_slot()
            slot.f64[:self._rec0] = self._hyper_rows(hyper_key)
            slot.i64[self._rec0:self._rec0 + rec.size] = rec.ravel()
            slot.i64[self._chk0:self._chk0 + chunks.size] = chunks.ravel()
            self._present, self._absent = present, [i for i in range(len(params)) if i not in seen]
            self._n_tensors, self._n_chunks = len(present), len(chunks)
            if present:
                self._upload(slot, self._chk0 + chunks.size)
            self._table_key, self._hyper_key = table_key, hyper_key
        elif hyper_key != self._hyper_key:
            slot = self._free_slot()
            slot.f64[:self._rec0] = self._hyper_rows(hyper_key)
            if self._n_tensors:
                self._upload(slot, self._rec0)
            self._hyper_key = hyper_key

    # ---- torch.optim.Optimizer ----
    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise NotImplementedError("FullModelClipAdamW: a closure is not supported; compute the loss before step()")
        with torch.cuda.device(self._device if self._params is not None else self._first_device()):
            self._prepare()
            if not self._n_tensors:
                return None
            n, c = self._n_tensors, self._n_chunks
            if self.max_norm > 0:
                ops.optim_grad_norm(self._rec_dev, self._chk_dev, self._partials, self._state_dev, n, c)
            ops.optim_adamw_step(self._rec_dev, self._chk_dev, self._hyper_dev, self._partials, self._state_dev, n, c,
                                 len(self._params), self.max_norm)
        self._calls += 1
        for i in self._absent:              # the counter moved, their step did not
            self._off[i] += 1
        return None

    def _first_device(self):
        for g in self.param_groups:
            for p in g["params"]:
                if not p.is_cuda:
                    raise RuntimeError(f"FullModelClipAdamW: parameter of shape {tuple(p.shape)} must be on the GPU (no CPU path in "
                                       "unseenobjectswithmeanshift_amd)")
                return p.device
        raise RuntimeError("FullModelClipAdamW: no parameters")

    def zero_grad(self, set_to_none=True):
        """``set_to_none=True`` (torch's default) drops the gradients as torch does; ``False`` zeroes every gradient in place in one
        launch over the optimizer's table instead of one memset per tensor (addresses stay, so the next step uploads nothing)."""
        if set_to_none:
            return super().zero_grad(set_to_none=True)
        with torch.cuda.device(self._device if self._params is not None else self._first_device()):
            self._prepare()
            if self._n_tensors:
                ops.optim_zero(self._rec_dev, self._chk_dev, self._n_tensors, self._n_chunks)

    def state_dict(self):
        """torch's layout; ``step`` of every parameter is materialised here from the call count (a float32 scalar, as torch keeps it)."""
        if self._params is not None:
            for i, p in enumerate(self._params):
                if p in self.state and "exp_avg" in self.state[p]:
                    self.state[p]["step"] = torch.tensor(float(self._calls - self._off[i]))
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        if self._params is None:
            with torch.cuda.device(self._first_device()):
                self._layout()
        for i, p in enumerate(self._params):
            st = self.state.get(p)
            self._off[i] = self._calls - (int(st["step"]) if st and "step" in st else 0)
        self._hyper_key = self._table_key = None         # new state tensors, new offsets: the next step uploads the table


def build_optimizer(model, base_lr=1e-4, weight_decay=0.05, weight_decay_norm=0.0, weight_decay_embed=0.0, backbone_multiplier=0.1,
                    betas=(0.9, 0.999), eps=1e-8, max_norm=0.01):
    """The optimizer every shipped config trains with (OPTIMIZER "ADAMW", CLIP_TYPE "full_model", CLIP_VALUE 0.01):
    ``FullModelClipAdamW(build_param_groups(model, ...), lr=base_lr, max_norm=max_norm)``."""
    groups = build_param_groups(model, base_lr, weight_decay, weight_decay_norm, weight_decay_embed, backbone_multiplier)
    return FullModelClipAdamW(groups, lr=base_lr, betas=betas, eps=eps, max_norm=max_norm)
