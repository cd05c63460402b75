"""The reference's optimizer (Trainer.build_optimizer, MSMFormer/tabletop_train_net_pretrained.py:113-191) on the HIP kernels of
csrc/optimizer.hip: AdamW with one param group per tensor behind ``clip_grad_norm_`` over the whole model.

The reference decides lr and weight decay per module, so every parameter tensor is a group of its own (298 for the ResNet-50 head,
125 for the RGB-D head), and every ``step()`` first clips the gradient of the whole model to ``CLIP_VALUE`` 0.01.  torch runs that as
a dozen small launches per tensor (a launch per group even with ``fused=True``).  Here a step is two launches over a device-resident
table, whatever the number of tensors: the squared norm of every chunk of every gradient, then the clip coefficient and the AdamW
update per chunk (the definition is in include/msm_hip.h).  Nothing in ``step()`` waits for the GPU.

    optimizer = build_optimizer(model.sem_seg_head, base_lr=1e-4)       # = FullModelClipAdamW(build_param_groups(...), ...)
    sum(losses.values()).backward(); optimizer.step(); optimizer.zero_grad()

``SGD`` and ``Adam`` are the optimizers of the UCN embedding network (tools/train_net.py:130-142: two param groups, biases then
weights; ``build_ucn_optimizer``) on the same table, chunk list, uploads and launches (msm_optim_count_norm / msm_optim_update,
one rule per optimizer), which keep the step count of every tensor on the device.  All three classes follow
GradScaler's protocol for fused optimizers (``_step_supports_amp_scaling``: the scaler sets ``grad_scale`` and ``found_inf``, the
kernels unscale and skip), so the reference's ``grad_scaler.step(optimizer)`` (AMPTrainer.run_step, :209-246) does not wait either:

    scaler.scale(losses).backward(); scaler.step(optimizer); scaler.update()

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
_SGD_HYPER = operator.itemgetter("lr", "weight_decay", "momentum", "dampening", "nesterov", "maximize")
_DATA_PTR = torch.Tensor.data_ptr


class _Slot:
    """One pinned staging buffer and the event behind its last copy."""

    def __init__(self, words):
        self.buf = torch.empty(words, dtype=torch.int64).pin_memory()
        self.i64 = self.buf.numpy()
        self.f64 = self.i64.view(np.float64)
        self.event = None


class _TableOptimizer(torch.optim.Optimizer):
    """What the three optimizers share: the device table (hyper rows, tensor records, chunk list), its host mirror and uploads, the
    launches of a step, ``zero_grad`` in one launch, the state dicts.  A subclass names its rule, the hyper-parameters of a group
    (``_hyper_of``, ``_group_rows``) and its per-parameter state (``_state_of``, ``_write_counts``, ``_loaded_counts``).

    Step counts live in ``_steps_dev`` (int64 per parameter), advanced by the launches for the tensors that take a step -- a step
    that GradScaler's ``found_inf`` skips is decided there, where no host counter could follow."""

    _NAME = None
    _RULE = None
    _hyper_of = None
    _step_supports_amp_scaling = True       # torch/amp/grad_scaler.py:403-454: the scaler sets grad_scale / found_inf and calls step()

    def _setup(self, max_norm):
        self.max_norm = float(max_norm)
        self.uploads = 0
        self.last_grad_norm = None
        self.last_clip_coef = None
        self._params = None             # flat parameter list; everything below is built from it at the first step
        self._seen = set()              # indices of the parameters that an earlier table held (their device counts may have moved)

    # ---- layout: what depends on the parameter list alone ----
    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        for p in self.param_groups[-1]["params"]:
            if p.dtype != torch.float32:
                raise NotImplementedError(f"{self._NAME}: parameter of shape {tuple(p.shape)} is {p.dtype}; only torch.float32 "
                                          "parameters are supported")
            if not p.is_contiguous():
                raise RuntimeError(f"{self._NAME}: parameter of shape {tuple(p.shape)} is not contiguous")
        if getattr(self, "_params", None) is not None:
            self._layout(keep_counts=True)

    def _layout(self, keep_counts=False):
        params = [p for g in self.param_groups for p in g["params"]]
        for p in params:
            if not p.is_cuda:
                raise RuntimeError(f"{self._NAME}: parameter of shape {tuple(p.shape)} must be on the GPU (no CPU path in "
                                   "unseenobjectswithmeanshift_amd)")
            if p.device != params[0].device:
                raise RuntimeError(f"{self._NAME}: parameters on {params[0].device} and {p.device}; one optimizer serves one GPU")
            if p.numel() == 0:
                raise RuntimeError(f"{self._NAME}: a parameter without elements")
        self._params = params
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
            f = self._state_dev.view(torch.float32)
            self.last_grad_norm, self.last_clip_coef = f[2], f[3]
        steps = torch.zeros(T, dtype=torch.int64, device=dev)
        if keep_counts:                    # a parameter group added later: the counts of the parameters before it stay
            steps[:self._steps_dev.numel()].copy_(self._steps_dev)
        self._steps_dev = steps
        self._slots = [_Slot(self._words), _Slot(self._words)]
        self._hyper_key = self._table_key = None
        self._n_tensors = self._n_chunks = self._n_states = 0

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
        rows = np.zeros((len(self._params), ops.OPTIM_HYP), dtype=np.float64)
        rows[:] = self._group_rows(key)[self._group_of]
        return rows.ravel()

    def _table_extra(self):
        """What besides the addresses decides the records (SGD: which groups keep a momentum buffer)."""
        return ()

    def _check_state(self, i, p, tensors):
        for name, s in tensors:
            if s.dtype != torch.float32 or s.device != self._device or s.shape != p.shape or not s.is_contiguous():
                raise RuntimeError(f"{self._NAME}: state {name} of parameter {i} must be a contiguous float32 tensor of shape "
                                   f"{tuple(p.shape)} on {self._device}")

    def _records(self, gptrs):
        """The tensor records and the chunk list of the parameters that have a gradient; creates their state."""
        present = [i for i, g in enumerate(gptrs) if g]
        rec = np.zeros((len(present), ops.OPTIM_REC), dtype=np.int64)
        for t, i in enumerate(present):
            p = self._params[i]
            g = p.grad
            if not g.is_cuda or g.device != self._device:
                raise RuntimeError(f"{self._NAME}: the gradient of parameter {i} must be on the GPU ({self._device}), got {g.device}")
            if g.dtype != torch.float32 or g.is_sparse:
                raise NotImplementedError(f"{self._NAME}: the gradient of parameter {i} is {g.dtype}"
                                          f"{' (sparse)' if g.is_sparse else ''}; only dense torch.float32 is supported")
            if not p.is_contiguous() or not g.is_contiguous():
                raise RuntimeError(f"{self._NAME}: parameter {i} of shape {tuple(p.shape)} or its gradient is not contiguous")
            m, v = self._state_of(i, p)
            ptrs = (p.data_ptr(), g.data_ptr(), 0 if m is None else m.data_ptr(), 0 if v is None else v.data_ptr())
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
        hyper_key = list(map(self._hyper_of, self.param_groups))        # ~0.1 ms of Python per step for 298 groups: no
        gptrs = [0 if g is None else g.data_ptr() for g in [p.grad for p in params]]      # per-group work beyond these lines
        table_key = (gptrs, list(map(_DATA_PTR, params)), self._table_extra())
        # a state that the user dropped (del optimizer.state[p]) took its tensors with it: new state, new records
        if table_key != self._table_key or len(self.state) != self._n_states:
            present, rec, chunks = self._records(gptrs)
            slot = self._free_slot()
            slot.f64[:self._rec0] = self._hyper_rows(hyper_key)
            slot.i64[self._rec0:self._rec0 + rec.size] = rec.ravel()
            slot.i64[self._chk0:self._chk0 + chunks.size] = chunks.ravel()
            self._seen.update(present)
            self._n_tensors, self._n_chunks, self._n_states = len(present), len(chunks), len(self.state)
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
            raise NotImplementedError(f"{self._NAME}: a closure is not supported; compute the loss before step()")
        # GradScaler.step sets these around the call (0-d float32 device tensors; grad_scale None after scaler.unscale_(optimizer)).
        # Only their addresses are used: the kernels read the values.
        grad_scale, found_inf = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)
        with torch.cuda.device(self._device if self._params is not None else self._first_device()):
            self._prepare()
            if not self._n_tensors:
                return None
            n, c, rows = self._n_tensors, self._n_chunks, len(self._params)
            if self.max_norm > 0:
                ops.optim_count_norm(self._rec_dev, self._chk_dev, self._partials, self._steps_dev, n, c, rows, grad_scale, found_inf)
            ops.optim_update(self._RULE, self._rec_dev, self._chk_dev, self._hyper_dev, self._partials, self._state_dev,
                             self._steps_dev, n, c, rows, self.max_norm, grad_scale, found_inf)
        return None

    def _first_device(self):
        for g in self.param_groups:
            for p in g["params"]:
                if not p.is_cuda:
                    raise RuntimeError(f"{self._NAME}: parameter of shape {tuple(p.shape)} must be on the GPU (no CPU path in "
                                       "unseenobjectswithmeanshift_amd)")
                return p.device
        raise RuntimeError(f"{self._NAME}: no parameters")

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
        """torch's layout; the step counts are read back from the device and materialised here (``step`` a float32 scalar, as torch
        keeps it): a wait, which state_dict() may and step() may not.  A parameter that has not stepped -- every step since its
        state was made was skipped -- is written out as torch would have it: without state."""
        if self._params is None:
            return super().state_dict()
        counts = self._steps_dev.cpu().tolist()
        self._write_counts(counts)
        sd = super().state_dict()
        for i, n in enumerate(counts):
            if n == 0:
                sd["state"].pop(i, None)
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        if self._params is None:
            with torch.cuda.device(self._first_device()):
                self._layout()
        # the loaded step counts to the device: one asynchronous copy
        staged = torch.tensor(self._loaded_counts(), dtype=torch.int64).pin_memory()
        self._steps_dev = staged.to(self._device, non_blocking=True)
        self._hyper_key = self._table_key = None         # new state tensors: the next step uploads the table


class _AdamFamily(_TableOptimizer):
    """State ``step``, ``exp_avg``, ``exp_avg_sq`` per parameter and the hyper-parameters of torch.optim.Adam / AdamW."""

    _hyper_of = staticmethod(_HYPER)

    def _check_args(self, lr, betas, eps, weight_decay, amsgrad, maximize):
        if amsgrad:
            raise NotImplementedError(f"{self._NAME}: amsgrad=True is not supported")
        if maximize:
            raise NotImplementedError(f"{self._NAME}: maximize=True is not supported")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid betas: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")

    def _group_rows(self, key):
        for gi, (lr, wd, betas, eps, amsgrad, maximize) in enumerate(key):
            if amsgrad or maximize:
                raise NotImplementedError(f"{self._NAME}: param group {gi} sets {'amsgrad' if amsgrad else 'maximize'}")
            if isinstance(lr, torch.Tensor) or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
                raise ValueError(f"{self._NAME}: param group {gi}: lr must be a Python float and betas in [0, 1), got "
                                 f"{type(lr).__name__}, {betas}")
        return np.array([(lr, wd, betas[0], betas[1], eps, 0.0, 0.0, 0.0) for lr, wd, betas, eps, _, _ in key], dtype=np.float64)

    def _state_of(self, i, p):
        st = self.state[p]
        if "exp_avg" not in st:
            st["step"] = torch.tensor(0.0)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            if i in self._seen:         # its state was dropped after it had stepped: it starts again at step 1, as in torch
                self._steps_dev[i:i + 1].fill_(0)
        m, v = st["exp_avg"], st["exp_avg_sq"]
        self._check_state(i, p, (("exp_avg", m), ("exp_avg_sq", v)))
        return m, v

    def _write_counts(self, counts):
        for p, n in zip(self._params, counts):
            if p in self.state and "exp_avg" in self.state[p]:
                self.state[p]["step"] = torch.tensor(float(n))

    def _loaded_counts(self):
        states = [self.state.get(p) for p in self._params]
        return [int(st["step"]) if st and "step" in st else 0 for st in states]


class FullModelClipAdamW(_AdamFamily):
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

    Under a ``torch.amp.GradScaler`` (``scaler.step(optimizer)``) the kernels unscale the gradients and skip the step when the
    scaler found an inf: no parameter, state or step count changes, ``last_grad_norm`` / ``last_clip_coef`` keep the last taken
    step's values, and ``.grad`` stays scaled (the reference's ``unscale_`` has divided it by then; nothing reads it before
    ``zero_grad``).  After a taken step ``.grad`` holds the unscaled, clipped gradient.

    The step count of every tensor lives on the device, where a skipped step is decided: ``state_dict()`` reads the counts back and
    may wait; ``step()`` and ``zero_grad()`` never do.  A parameter whose state was dropped (``del optimizer.state[p]``) gets fresh
    state at the next step and counts from 1 again, as in torch.

    Not supported (NotImplementedError): ``amsgrad``, ``maximize``, a ``closure``, parameters other than float32;
    RuntimeError: host tensors, non-contiguous parameters or gradients, parameters on several devices."""

    _NAME = "FullModelClipAdamW"
    _RULE = "adamw"

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 max_norm=0.01):
        self._check_args(lr, betas, eps, weight_decay, amsgrad, maximize)
        # the keys of torch.optim.AdamW's own groups, so that a state dict of either loads into the other and then steps
        defaults = dict(torch.optim.AdamW([torch.zeros(1)]).defaults)
        defaults.update(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False)
        self._setup(max_norm)
        super().__init__(params, defaults)


class Adam(_AdamFamily):
    """``torch.optim.Adam`` (no amsgrad: weight decay added to the gradient, bias-corrected moments) in two launches per ``step()``,
    behind ``clip_grad_norm_`` over all parameters when ``max_norm > 0`` (off by default, as in tools/train_net.py:136-138).

    Param groups of any number of tensors; everything else as ``FullModelClipAdamW``: torch's ``param_groups``, schedulers write
    ``group["lr"]``, ``state_dict()`` / ``load_state_dict()`` interchangeable with ``torch.optim.Adam`` (``step``, ``exp_avg``,
    ``exp_avg_sq``; ``state_dict()`` reads the step counts from the device and may wait, ``step()`` never does), ``uploads``,
    ``last_grad_norm`` / ``last_clip_coef``, ``zero_grad(set_to_none=False)`` in one launch, GradScaler's fused protocol.

    Not supported (NotImplementedError): ``amsgrad``, ``maximize``, a ``closure``, parameters other than float32;
    RuntimeError: host tensors, non-contiguous parameters or gradients, parameters on several devices."""

    _NAME = "Adam"
    _RULE = "adam"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False, max_norm=0.0):
        self._check_args(lr, betas, eps, weight_decay, amsgrad, maximize)
        defaults = dict(torch.optim.Adam([torch.zeros(1)]).defaults)
        defaults.update(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False)
        self._setup(max_norm)
        super().__init__(params, defaults)


class SGD(_TableOptimizer):
    """``torch.optim.SGD`` (momentum, dampening, nesterov, weight decay added to the gradient) in two launches per ``step()``, behind
    ``clip_grad_norm_`` over all parameters when ``max_norm > 0`` (the "SGD" branch of Trainer.build_optimizer clips, the UCN
    trainer does not).

    State per parameter is ``momentum_buffer`` alone, as in torch, and only with momentum != 0; whether a tensor has stepped -- its
    first step sets the buffer to the gradient, undampened -- is counted on the device.  ``state_dict()`` / ``load_state_dict()``
    are interchangeable with ``torch.optim.SGD``: a loaded buffer means "has stepped", a tensor that has not stepped is written out
    without one.  A group whose momentum goes from 0 to non-zero in mid-run gets fresh buffers, and its tensors count from there.  Everything else as ``FullModelClipAdamW``: param groups of any number of tensors, schedulers write
    ``group["lr"]``, ``uploads``, ``last_grad_norm`` / ``last_clip_coef``, ``zero_grad(set_to_none=False)`` in one launch,
    GradScaler's fused protocol; ``step()`` never waits, ``state_dict()`` may.

    Not supported (NotImplementedError): ``maximize``, a ``closure``, parameters other than float32;
    RuntimeError: host tensors, non-contiguous parameters or gradients, parameters on several devices."""

    _NAME = "SGD"
    _RULE = "sgd"
    _hyper_of = staticmethod(_SGD_HYPER)

    def __init__(self, params, lr, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False, max_norm=0.0):
        if maximize:
            raise NotImplementedError("SGD: maximize=True is not supported")
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        defaults = dict(torch.optim.SGD([torch.zeros(1)], lr=1e-3).defaults)
        defaults.update(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, maximize=False)
        self._setup(max_norm)
        super().__init__(params, defaults)

    def _group_rows(self, key):
        for gi, (lr, wd, momentum, dampening, nesterov, maximize) in enumerate(key):
            if maximize:
                raise NotImplementedError(f"SGD: param group {gi} sets maximize")
            if isinstance(lr, torch.Tensor) or momentum < 0.0:
                raise ValueError(f"SGD: param group {gi}: lr must be a Python float and momentum >= 0, got {type(lr).__name__}, "
                                 f"{momentum}")
            if nesterov and (momentum <= 0 or dampening != 0):
                raise ValueError(f"SGD: param group {gi}: Nesterov momentum requires a momentum and zero dampening")
        return np.array([(lr, wd, 0.0, 0.0, 0.0, momentum, dampening, 1.0 if nesterov else 0.0) for lr, wd, momentum, dampening,
                         nesterov, _ in key], dtype=np.float64)

    def _table_extra(self):
        return tuple(g["momentum"] != 0 for g in self.param_groups)      # a group that starts to keep a buffer: new records

    def _state_of(self, i, p):
        if self.param_groups[self._group_of[i]]["momentum"] == 0:
            return None, None
        st = self.state[p]
        if st.get("momentum_buffer") is None:
            st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            if i in self._seen:         # stepped without a buffer (its group's momentum was 0 until now): torch's buffer is None
                self._steps_dev[i:i + 1].fill_(0)       # there, so the next step is its first -- buf = d, undampened
        buf = st["momentum_buffer"]
        self._check_state(i, p, (("momentum_buffer", buf),))
        return buf, None

    def _write_counts(self, counts):
        pass                                # no step key in torch.optim.SGD's state

    def _loaded_counts(self):
        states = [self.state.get(p) for p in self._params]
        return [1 if st and st.get("momentum_buffer") is not None else 0 for st in states]


def build_ucn_param_groups(network, weight_decay=1e-4):
    """The two param groups of the UCN embedding network's trainer (tools/train_net.py:133-134 over SEGNET.bias_parameters() /
    weight_parameters(), lib/networks/SEG.py:122-126): every parameter whose name holds 'bias', then every one whose name holds
    'weight', in the order of ``named_parameters()``, both at TRAIN.WEIGHT_DECAY (1e-4, lib/fcn/config.py).  Host only."""
    named = list(network.named_parameters())
    return [{"params": [p for n, p in named if "bias" in n], "weight_decay": weight_decay},
            {"params": [p for n, p in named if "weight" in n], "weight_decay": weight_decay}]


def build_ucn_optimizer(network, solver="sgd", lr=1e-4, momentum=0.9, beta=0.999, weight_decay=1e-4):
    """The optimizer tools/train_net.py:130-142 builds over ``build_ucn_param_groups(network)``: ``solver`` "sgd" (its default:
    ``SGD(momentum=TRAIN.MOMENTUM)``, driven by a MultiStepLR) or "adam" (``Adam(betas=(TRAIN.MOMENTUM, TRAIN.BETA))``); defaults
    TRAIN.LEARNING_RATE 1e-4, MOMENTUM 0.9, BETA 0.999, WEIGHT_DECAY 1e-4.  Neither clips."""
    if solver not in ("sgd", "adam"):
        raise ValueError(f"build_ucn_optimizer: solver must be 'sgd' or 'adam', got {solver!r}")
    groups = build_ucn_param_groups(network, weight_decay)
    if solver == "sgd":
        return SGD(groups, lr, momentum=momentum)
    return Adam(groups, lr, betas=(momentum, beta))


def build_optimizer(model, base_lr=1e-4, weight_decay=0.05, weight_decay_norm=0.0, weight_decay_embed=0.0, backbone_multiplier=0.1,
                    betas=(0.9, 0.999), eps=1e-8, max_norm=0.01, optimizer="ADAMW", momentum=0.9):
    """The optimizer every shipped config trains with (OPTIMIZER "ADAMW", CLIP_TYPE "full_model", CLIP_VALUE 0.01):
    ``FullModelClipAdamW(build_param_groups(model, ...), lr=base_lr, max_norm=max_norm)``.  ``optimizer="SGD"`` is the reference's
    other branch (:179-182): ``SGD(the same groups, lr=base_lr, momentum=momentum)`` (SOLVER.MOMENTUM 0.9) behind the same
    clipping.  Anything else raises NotImplementedError, as the reference does."""
    groups = build_param_groups(model, base_lr, weight_decay, weight_decay_norm, weight_decay_embed, backbone_multiplier)
    if optimizer == "SGD":
        return SGD(groups, lr=base_lr, momentum=momentum, max_norm=max_norm)
    if optimizer != "ADAMW":
        raise NotImplementedError(f"no optimizer type {optimizer}")
    return FullModelClipAdamW(groups, lr=base_lr, betas=betas, eps=eps, max_norm=max_norm)
