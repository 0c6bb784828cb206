"""Optimizer / schedule of the training-step contract (reference solver/__init__.py:10-92, engine/trainer.py:109-126).

AdamW(lr 3e-4, betas (0.9, 0.99), weight decay 1e-5); parameters whose name contains "bias" run at
BASE_LR * BIAS_LR_FACTOR.  The reference builds one param-group per parameter (280 groups -> 280 separate foreach
launches); groups with equal hyper-parameters are arithmetically identical when merged, so two groups are built
(weights / biases), which lets torch run one fused multi-tensor AdamW kernel per group.

SOLVER.OPTIMIZER 'adam_onecycle' (solver/__init__.py:45-58) is the reference's fastai wrapper with its one-cycle schedule: `OptimWrapper`, `OneCycle`
and the driver of its one-launch update, `MultiTensorAdamTrueWD`, below."""
import math
import warnings

import torch


class CosineWarmupLR(torch.optim.lr_scheduler.LRScheduler):
    """The reference's warm-up schedule (solver/learning_schedules_fastai.py:82-91): RISES from `eta_min` at step 0 to each group's
    base learning rate at step T_max along (1 - cos)/2.  (torch's CosineAnnealingLR is the falling half and is not this.)"""

    def __init__(self, optimizer, T_max, eta_min=0.0, last_epoch=-1):
        self.T_max, self.eta_min = T_max, eta_min
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        f = (1.0 - math.cos(math.pi * self.last_epoch / self.T_max)) / 2.0
        return [self.eta_min + (base_lr - self.eta_min) * f for base_lr in self.base_lrs]


def step_scheduler(scheduler, iteration):
    """`scheduler.step(iteration)` as the reference's loop calls it (engine/trainer.py:123-126): the schedule position is SET to the
    iteration just finished (so a resumed run, or the hand-over from the warm-up schedule, lands on the right value) instead of
    advanced by one.  torch keeps that call form but warns about it."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        scheduler.step(iteration)


def get_model_params(model, cfg, per_parameter_groups=False, tensor_lr_device=None):
    base_lr = cfg.SOLVER.BASE_LR
    bias_lr = max(base_lr, base_lr * cfg.SOLVER.BIAS_LR_FACTOR)
    if tensor_lr_device is not None:
        # a captured optimizer step bakes a Python-float lr into the hipGraph; a device scalar is read at replay time, so schedulers
        # (which fill_ it) keep working under GraphedTrainStep
        mk = lambda v: torch.tensor(float(v), dtype=torch.float32, device=tensor_lr_device)      # noqa: E731
    else:
        mk = float
    if per_parameter_groups:                                         # the reference's literal layout
        return [{"params": [p], "lr": mk(bias_lr if "bias" in k else base_lr)} for k, p in model.named_parameters() if p.requires_grad]
    w = [p for k, p in model.named_parameters() if p.requires_grad and "bias" not in k]
    b = [p for k, p in model.named_parameters() if p.requires_grad and "bias" in k]
    return [{"params": w, "lr": mk(base_lr)}, {"params": b, "lr": mk(bias_lr)}]


def build_optimizer(model, cfg, per_parameter_groups=False, capturable=None):
    """`capturable=None`: capturable (device-side step counters and learning rates) whenever the model lives on a GPU, so that the
    training loop can replay the step from hipGraphs (engine/trainer.do_train); the arithmetic is AdamW's / Adam's either way.
    'adam' is the reference's optim.Adam(betas=(0.9, 0.99)) with L2 weight decay (solver/__init__.py:33-34); on the CPU it is built as a plain
    torch.optim.Adam with float learning rates.  'sgd' stays eager: the reference's own sgd branch reads a MOMENTUM key its config does not define.
    'adam_onecycle' returns an `OptimWrapper` (the reference's fastai wrapper around optim.Adam, two param groups of its own: `onecycle_param_groups`);
    `per_parameter_groups` does not apply to it."""
    s = cfg.SOLVER
    dev = next((p.device for p in model.parameters() if p.is_cuda), None)
    if s.OPTIMIZER == "adam_onecycle":
        return OptimWrapper.for_model(model, s.BASE_LR, wd=s.WEIGHT_DECAY, capturable=(dev is not None) if capturable is None else bool(capturable))
    adam_family = s.OPTIMIZER in ("adamw", "adam")
    if capturable is None:
        capturable = dev is not None and adam_family
    tensor_lr = capturable and dev is not None and adam_family
    params = get_model_params(model, cfg, per_parameter_groups, tensor_lr_device=dev if tensor_lr else None)
    on_gpu = dev is not None
    if s.OPTIMIZER == "adamw":
        lr = torch.tensor(float(s.BASE_LR), dtype=torch.float32, device=dev) if tensor_lr else s.BASE_LR
        return torch.optim.AdamW(params, lr=lr, weight_decay=s.WEIGHT_DECAY, betas=(0.9, 0.99), fused=on_gpu or None,
                                 capturable=capturable)
    if s.OPTIMIZER == "adam":
        if not capturable:                                                # the CPU (or an explicit capturable=False): as before
            return torch.optim.Adam(params, lr=s.BASE_LR, weight_decay=s.WEIGHT_DECAY, betas=(0.9, 0.99), fused=on_gpu or None)
        lr = torch.tensor(float(s.BASE_LR), dtype=torch.float32, device=dev) if tensor_lr else s.BASE_LR
        return torch.optim.Adam(params, lr=lr, weight_decay=s.WEIGHT_DECAY, betas=(0.9, 0.99), fused=on_gpu or None, capturable=True)
    if s.OPTIMIZER == "sgd":
        return torch.optim.SGD(params, lr=s.BASE_LR, weight_decay=s.WEIGHT_DECAY, momentum=s.get("MOMENTUM", 0.9))
    raise NotImplementedError("SOLVER.OPTIMIZER %r is not a name the reference knows: adamw, adam, sgd and adam_onecycle are all served" % s.OPTIMIZER)


BN_TYPES = (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d, torch.nn.BatchNorm3d, torch.nn.SyncBatchNorm)      # fastai_optim.bn_types (InPlaceABN is not one)


def onecycle_param_groups(model):
    """-> ([non-BN parameters, BN parameters], trainable parameters in neither): the reference's layout for 'adam_onecycle' (solver/__init__.py:45-58,
    fastai_optim.split_bn_bias).  `flatten_model` collects the LEAF modules -- modules without children -- depth first, and the two groups are the
    trainable parameters of the leaves that are not / are BatchNorm, in that order, each parameter once.  A parameter owned directly by a module that
    also HAS children belongs to no leaf and so to no group: DCN.weight / DCN.bias of every DCNv2 layer (DCN holds the child `conv_offset_mask`).
    Such parameters receive gradients, are counted by the gradient clip, and are never updated."""
    def leaves(m):
        kids = list(m.children())
        return [m] if not kids else sum((leaves(k) for k in kids), [])
    groups, seen = ([], []), set()
    for leaf in leaves(model):
        for p in leaf.parameters():
            if p.requires_grad and id(p) not in seen:
                seen.add(id(p))
                groups[isinstance(leaf, BN_TYPES)].append(p)
    left = [p for p in model.parameters() if p.requires_grad and id(p) not in seen]
    return list(groups), left


class OptimWrapper:
    """SOLVER.OPTIMIZER 'adam_onecycle': the reference's fastai wrapper (solver/fastai_optim.py OptimWrapper, built with true_wd=True, bn_wd=True) around a
    real torch.optim.Adam(betas=(0.9, 0.99)) -- `self.opt` -- with the reference's two param groups (`onecycle_param_groups`), so state_dict() is the inner
    Adam's and loads into the reference's wrapper, and the reverse.  What the reference's loop, scheduler and checkpointer touch is here: step / zero_grad,
    param_groups / state / state_dict / load_state_dict, and lr / mom / wd / beta as properties.

    step(): every held parameter is multiplied by 1 - wd * lr (a Python double, rounded to fp32 by `mul_`: decay outside the optimizer), then Adam steps
    with weight_decay 0 and betas = (mom, beta).  BIAS_LR_FACTOR plays no part: both groups share lr, mom and wd.

    On a GPU (`capturable`) the inner Adam is capturable and every group carries a device-scalar `lr` and a device-scalar `mom`, which the setters
    `fill_`: the OneCycle schedule moves both every iteration, and the one-launch update (MultiTensorAdamTrueWD, csrc/adamw.hip mfx_optim_multi_sched)
    reads both from the device, so a captured step follows the schedule.  `betas` in the groups stays a float pair (torch's bookkeeping, state_dict).
    `step()` here is the eager form -- the reference's arithmetic in torch operations, the form the CPU runs; `optimizer_step` takes the HIP launch.
    `norm_only_params`: the trainable parameters the groups leave out; SOLVER.GRAD_NORM_CLIP's norm covers their gradients (the reference clips over
    model.parameters()) and zero_grad clears them."""

    def __init__(self, opt, wd, true_wd=False, bn_wd=True, norm_only_params=()):
        self.opt, self.true_wd, self.bn_wd = opt, bool(true_wd), bool(bn_wd)
        self.norm_only_params = list(norm_only_params)
        self._wd = float(wd)
        for g in opt.param_groups:
            if "mom" not in g:
                g["mom"] = torch.tensor(float(g["betas"][0]), dtype=torch.float32, device=g["lr"].device) if torch.is_tensor(g["lr"]) else float(g["betas"][0])
        if not self.true_wd:
            self.wd = wd

    @classmethod
    def for_model(cls, model, lr, wd, capturable=False):
        groups, left = onecycle_param_groups(model)
        dev = next((p.device for p in model.parameters() if p.is_cuda), None)
        if capturable and dev is not None:
            mk = lambda v: torch.tensor(float(v), dtype=torch.float32, device=dev)      # noqa: E731
            opt = torch.optim.Adam([{"params": g, "lr": mk(lr), "mom": mk(0.9)} for g in groups], lr=mk(lr), betas=(0.9, 0.99), fused=True, capturable=True)
        else:
            opt = torch.optim.Adam([{"params": g, "lr": float(lr), "mom": 0.9} for g in groups], lr=float(lr), betas=(0.9, 0.99))
        return cls(opt, wd=wd, true_wd=True, bn_wd=True, norm_only_params=left)

    def __repr__(self):
        return "OptimWrapper over %r.\nTrue weight decay: %s" % (self.opt, self.true_wd)

    # ---- what torch optimizers offer, handed to the inner one ----
    param_groups = property(lambda self: self.opt.param_groups)
    state = property(lambda self: self.opt.state)

    def state_dict(self):
        return self.opt.state_dict()

    def load_state_dict(self, sd):
        """The inner Adam's load; device-scalar lr / mom stay the same tensor objects (a captured step reads them), filled with the loaded values."""
        keep = [(g["lr"], g.get("mom")) for g in self.opt.param_groups]
        self.opt.load_state_dict(sd)
        for g, (lr, mom) in zip(self.opt.param_groups, keep):
            new_mom = g.get("mom", g["betas"][0])
            for key, old, new in (("lr", lr, g["lr"]), ("mom", mom, new_mom)):
                if torch.is_tensor(old):
                    old.fill_(float(new))
                    g[key] = old
                else:
                    g[key] = float(new)
            g["betas"] = (float(new_mom), float(g["betas"][1]))

    def zero_grad(self, set_to_none=True):
        self.opt.zero_grad(set_to_none=set_to_none)
        for p in self.norm_only_params:
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.detach_().zero_()

    def __getattr__(self, k):                               # (the reference's passthrough: anything else is the inner optimizer's, or None)
        if k == "opt":
            raise AttributeError(k)
        return getattr(self.opt, k, None)

    def _decay_groups(self):
        return [g for i, g in enumerate(self.opt.param_groups) if i % 2 == 0 or self.bn_wd]

    @torch.no_grad()
    def step(self):
        """The eager form.  `found_inf` (the fp16 loss scaler's flag, set on this object): read on the host here -- a set flag skips the whole step."""
        found = self.__dict__.get("found_inf")
        if found is not None and float(found) != 0.0:
            return
        if self.true_wd:
            for g in self._decay_groups():
                factor = 1 - self._wd * float(g["lr"])
                for p in g["params"]:
                    if p.requires_grad:
                        p.data.mul_(factor)
            for g in self.opt.param_groups:
                g["weight_decay"] = 0
        for g in self.opt.param_groups:                      # betas = (mom, beta): the floats torch's Adam reads
            g["betas"] = (float(g["mom"]), float(g["betas"][1]))
        self.opt.step()

    # ---- hyper-parameters as properties (fastai_optim.py:166-209) ----
    def _set(self, key, val):
        for g in self.opt.param_groups:
            if torch.is_tensor(g.get(key)):
                g[key].fill_(float(val))
            else:
                g[key] = float(val)

    @property
    def lr(self):
        return float(self.opt.param_groups[0]["lr"])

    @lr.setter
    def lr(self, val):
        self._set("lr", val)

    @property
    def mom(self):
        return float(self.opt.param_groups[0]["mom"])

    @mom.setter
    def mom(self, val):
        self._set("mom", val)
        for g in self.opt.param_groups:
            g["betas"] = (float(val), float(g["betas"][1]))

    @property
    def beta(self):
        return float(self.opt.param_groups[0]["betas"][1])

    @beta.setter
    def beta(self, val):
        if val is None:
            return
        for g in self.opt.param_groups:
            g["betas"] = (float(g["betas"][0]), float(val))

    @property
    def wd(self):
        return self._wd

    @wd.setter
    def wd(self, val):
        if not self.true_wd:
            for i, g in enumerate(self.opt.param_groups):
                if i % 2 == 0 or self.bn_wd:
                    g["weight_decay"] = float(val)
        self._wd = float(val)


def _annealing_cos(start, end, pct):
    import numpy as np
    cos_out = np.cos(np.pi * pct) + 1                        # (np.cos, as the reference: learning_schedules_fastai.py:53-57)
    return end + (start - end) / 2 * cos_out


class OneCycle:
    """The reference's one-cycle schedule (solver/learning_schedules_fastai.py OneCycle / LRSchedulerStep) over an OptimWrapper: with
    a1 = int(total_step * pct_start) and low_lr = lr_max / div_factor, lr anneals by cosine from low_lr to lr_max over [0, a1) and from lr_max to
    low_lr / 1e4 over [a1, total_step); mom from moms[0] to moms[1] and back.  The constructor sets (low_lr, moms[0]); `step(k)` SETS the values of
    iteration k + 1 -- the trainer calls it after the optimizer step of iteration k (engine/trainer.py:121-126), so iteration 0 runs at the
    constructor's values.  A pure function of the iteration: no state_dict (the reference's checkpointer skips it for that reason).
    `last_epoch = k >= 0` (a resumed run whose last finished iteration was k) positions the schedule at the values of step(k)."""

    def __init__(self, fai_optimizer, total_step, lr_max, moms, div_factor, pct_start, last_epoch=-1):
        self.optimizer, self.total_step = fai_optimizer, total_step
        self.lr_max, self.moms, self.div_factor, self.pct_start = lr_max, list(moms), div_factor, pct_start
        a1 = int(total_step * pct_start)
        low_lr = lr_max / div_factor
        self.lr_phases = [(0, a1, (low_lr, lr_max)), (a1, total_step, (lr_max, low_lr / 1e4))]
        self.mom_phases = [(0, a1, tuple(self.moms)), (a1, total_step, tuple(self.moms[::-1]))]
        assert 0 < a1 < total_step, "OneCycle: int(total_step * pct_start) must lie inside (0, total_step)"
        fai_optimizer.lr, fai_optimizer.mom = low_lr, self.moms[0]
        if last_epoch >= 0:
            self.step(last_epoch)

    def values(self, step):
        """(lr, mom) that `step(step)` sets."""
        out = []
        for phases in (self.lr_phases, self.mom_phases):
            val = None
            for start, end, (a, b) in phases:
                if step >= start:
                    val = _annealing_cos(a, b, (step - start) / (end - start))
            out.append(float(val))
        return tuple(out)

    def step(self, step):
        self.optimizer.lr, self.optimizer.mom = self.values(step)


def build_scheduler(optimizer, cfg=None, iters_per_epoch=1, last_epoch=-1, total_iters_each_epoch=None, optim_cfg=None):
    """Step decay by LR_DECAY (solver/__init__.py:64-92), stepped per iteration.

    Two call forms: this build's `build_scheduler(optimizer, cfg, iters_per_epoch)` -> LambdaLR decaying at
    DECAY_EPOCH_STEPS * iters_per_epoch; and the reference's `build_scheduler(optimizer, total_iters_each_epoch=...,
    optim_cfg=cfg.SOLVER)` -> `(scheduler, warmup_scheduler)` decaying at optim_cfg.STEPS (iterations, set by the entry
    script from the epochs), clipped at LR_CLIP / BASE_LR, with the cosine warm-up when LR_WARMUP is on.
    An OPTIMIZER name containing 'onecycle' gets the OneCycle schedule over MAX_ITERATION instead (solver/__init__.py:78-82) and no warm-up
    schedule; LR_WARMUP True is refused (the reference's loop asserts that the warm-up scheduler exists, engine/trainer.py:82-83)."""
    s_cfg = optim_cfg if optim_cfg is not None else cfg.SOLVER
    if str(s_cfg.OPTIMIZER).find("onecycle") >= 0:
        if s_cfg.LR_WARMUP:
            raise ValueError("SOLVER.LR_WARMUP True with SOLVER.OPTIMIZER %r: build_scheduler returns no warm-up scheduler for the one-cycle schedule, and "
                             "the reference's loop stops on it (engine/trainer.py:82-83 `assert warmup_scheduler is not None`); set LR_WARMUP False"
                             % s_cfg.OPTIMIZER)
        one = OneCycle(optimizer, s_cfg.MAX_ITERATION, s_cfg.BASE_LR, list(s_cfg.MOMS), s_cfg.DIV_FACTOR, s_cfg.PCT_START, last_epoch=last_epoch)
        return (one, None) if optim_cfg is not None else one
    if optim_cfg is not None:
        steps, decay = list(optim_cfg.STEPS), optim_cfg.LR_DECAY
        floor = optim_cfg.LR_CLIP / optim_cfg.BASE_LR

        def lr_lbmd(it):
            f = 1.0
            for s in steps:
                if it >= s:
                    f *= decay
            return max(f, floor)
        sched = torch.optim.lr_scheduler.LambdaLR(optimizer, lr_lbmd, last_epoch=last_epoch)
        warm = None
        if optim_cfg.LR_WARMUP:
            warm = CosineWarmupLR(optimizer, T_max=optim_cfg.WARMUP_STEPS, eta_min=optim_cfg.BASE_LR / optim_cfg.DIV_FACTOR)
        return sched, warm
    steps = [e * iters_per_epoch for e in cfg.SOLVER.DECAY_EPOCH_STEPS]
    decay = cfg.SOLVER.LR_DECAY

    def factor(it):
        f = 1.0
        for s in steps:
            if it >= s:
                f *= decay
        return f
    return torch.optim.lr_scheduler.LambdaLR(optimizer, factor, last_epoch=last_epoch)


class MultiTensorAdamW:
    """`optimizer.step()` of a torch.optim.AdamW (fused, capturable, device-scalar learning rates: what `build_optimizer` makes on a GPU) as ONE HIP launch
    over all parameter tensors (csrc/adamw.hip) instead of torch's chunked multi-tensor kernels (25 launches / 345 us of the B = 8 training step).
    The optimizer object stays the owner of everything -- param_groups, `state[p] = {step, exp_avg, exp_avg_sq}` in torch's own layout -- so
    state_dict() / load_state_dict() / LR schedulers / the loss scaler's `found_inf` hook work unchanged; only the arithmetic runs elsewhere.

    The kernel reads a pointer table on the device.  Eagerly the table is rebuilt and uploaded every call (gradients are fresh tensors each step).
    Inside a stream capture the addresses of the step's gradients are known once backward has been captured, but a host-to-device copy cannot be:
    the launch is recorded against tables of its own (allocated by the preceding eager step -- NOT inside the capture: see step() -- and never
    reused by eager steps) and `finish_capture()` fills them once the capture has ended (before the first replay).

    `step(max_norm)` with max_norm > 0 is the CLIPPED update (reference engine/trainer.py:119 clip_grad_norm_, then step): two launches over the same
    tables leave [total_norm, coef] in a device pair (`self.grad_norm`: mfx_grad_norm_multi, fixed-order sums, no atomics) and the update multiplies
    every gradient element by coef as it reads it.  The gradients themselves are not written: p.grad keeps the UNCLIPPED values.
    `MultiTensorAdam` below is the same driver for torch.optim.Adam with L2 weight decay (SOLVER.OPTIMIZER 'adam')."""
    optimizer_type = torch.optim.AdamW
    rule = 0                      # lib.OPTIM_ADAMW
    group_extra_bytes = 0         # per group, behind the mfx_adamw_group records in the group table (MultiTensorAdamTrueWD: the beta1 pointers)

    def __init__(self, optimizer):
        import weakref
        self._opt = weakref.ref(optimizer)     # (the optimizer holds this object: no reference cycle, or its parameters outlive their last user until a GC pass)
        self.tables = {}          # device -> (descs tensor, prefix tensor, groups tensor, capacity)
        self.pending = []
        self.captured = []
        self.spare = {}           # device -> a table set allocated by the last eager step for the next captured launch
        self.grad_norm = None     # [total_norm, coef] of the last clipped step (device fp32 pair; a captured step keeps its own)

    @classmethod
    def eligible(cls, optimizer):
        if type(optimizer) is not cls.optimizer_type:
            return False
        for g in optimizer.param_groups:
            if bool(g.get("decoupled_weight_decay", cls.rule == 0)) != (cls.rule == 0):      # (torch.optim.Adam can be asked for AdamW's rule)
                return False
            if not g.get("capturable") or g.get("amsgrad") or g.get("maximize") or not torch.is_tensor(g["lr"]) or not g["lr"].is_cuda \
                    or g["lr"].dtype != torch.float32 or g.get("differentiable"):
                return False
            for p in g["params"]:
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous() or p.is_sparse:
                    return False
        return True

    def _norm_only(self, opt):
        """Parameters whose gradients the clipped step's norm covers although `opt` does not hold them (none under AdamW / Adam)."""
        return []

    def _group_bytes(self):
        from . import lib as L
        return ctypes_sizeof(L.AdamWGroup) + self.group_extra_bytes

    def _new_tables(self, dev, n, ngroups):
        from . import lib as L
        rows = [p for g in self._opt().param_groups for p in g["params"]] + list(self._norm_only(self._opt()))
        cap = max(n, len(rows))
        chunk = L.load().mfx_adamw_chunk_elems()
        nchunk = sum((p.numel() + chunk - 1) // chunk for p in rows)
        # ... + the gradient norm's partial sums (one float per chunk) and its [total_norm, coef] pair: written and read by the launches themselves
        return (torch.zeros(cap * ctypes_sizeof(L.AdamWDesc), dtype=torch.uint8, device=dev), torch.zeros(cap + 1, dtype=torch.int64, device=dev),
                torch.zeros(max(ngroups, len(self._opt().param_groups)) * self._group_bytes(), dtype=torch.uint8, device=dev), cap,
                torch.zeros(int(L.load().mfx_grad_norm_workspace_bytes(nchunk)), dtype=torch.uint8, device=dev),
                torch.ones(2, dtype=torch.float32, device=dev))

    def _tables(self, dev, n, ngroups):
        t = self.tables.get(dev)
        if t is None or t[3] < n or t[2].numel() < ngroups * self._group_bytes():
            t = self.tables[dev] = self._new_tables(dev, n, ngroups)
        return t

    @torch.no_grad()
    def step(self, max_norm=-1.0):
        import numpy as np
        from . import lib as L
        opt = self._opt()
        chunk = L.load().mfx_adamw_chunk_elems()
        by_dev = {}
        clip = max_norm is not None and float(max_norm) > 0

        def dense(gr):
            if gr.dtype != torch.float32 or not gr.is_contiguous() or gr.is_sparse:
                raise RuntimeError("MultiTensorAdamW: dense contiguous fp32 gradients only")
            return gr
        for gi, g in enumerate(opt.param_groups):
            for p in g["params"]:
                if p.grad is None:
                    if self._decay_only(p):
                        by_dev.setdefault(p.device, []).append((gi, p, None, None))
                    continue
                st = opt.state[p]
                if len(st) == 0:                                       # torch's lazy state initialisation (adamw.py `_init_group`)
                    st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                by_dev.setdefault(p.device, []).append((gi, p, dense(p.grad), st))
        if clip:
            for p in self._norm_only(opt):
                if p.grad is not None:
                    by_dev.setdefault(p.device, []).append((-1, p, dense(p.grad), None))
        found_inf = getattr(opt, "found_inf", None)
        opt._opt_called = True                                         # (what torch's wrapped step() tells the LR schedulers)
        capturing = torch.cuda.is_current_stream_capturing()
        if clip and len(by_dev) > 1:
            raise RuntimeError("MultiTensorAdamW: the clipped update takes the norm over ONE device's gradients")
        for dev, items in by_dev.items():
            n = len(items)
            descs = (L.AdamWDesc * n)()
            prefix = np.zeros(n + 1, dtype=np.int64)
            for i, (gi, p, gr, st) in enumerate(items):
                d = descs[i]
                if gi < 0:                                             # norm-only: the update returns for this row
                    d.g = gr.data_ptr()
                elif gr is None:                                       # decay-only: shrunk, no Adam step
                    d.p = p.data_ptr()
                else:
                    d.p, d.g, d.m, d.v, d.step = p.data_ptr(), gr.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), st["step"].data_ptr()
                d.numel, d.group = p.numel(), gi
                prefix[i + 1] = prefix[i] + (p.numel() + chunk - 1) // chunk
            groups = (L.AdamWGroup * len(opt.param_groups))()
            for gi, g in enumerate(opt.param_groups):
                groups[gi].lr = g["lr"].data_ptr()
                groups[gi].beta1, groups[gi].beta2 = float(g["betas"][0]), float(g["betas"][1])
                groups[gi].eps, groups[gi].weight_decay = float(g["eps"]), float(self._group_wd(opt, gi, g))
            host = (torch.from_numpy(np.frombuffer(bytes(descs), dtype=np.uint8).copy()), torch.from_numpy(prefix),
                    torch.from_numpy(np.frombuffer(bytes(groups) + self._group_extra(opt), dtype=np.uint8).copy()))
            if capturing:
                # tables of their own for a captured launch: an eager step of the same optimizer later must not overwrite what the replays read.  They
                # were allocated by the last EAGER step (`spare`), outside the graph's memory pool -- a block of that pool is reused by other captured
                # temporaries, whose kernels would overwrite the table at every replay before this launch reads it
                sp = self.spare.pop(dev, None)
                if sp is None or sp[3] < n:
                    raise RuntimeError("MultiTensorAdamW: run one eager optimizer step before capturing one (it allocates the captured launch's tables)")
                dt, pt, gt, _, ws, out2 = sp
                self.captured.append(sp)
                self.pending.append((dt, pt, gt, host))
            else:
                dt, pt, gt, _, ws, out2 = self._tables(dev, n, len(opt.param_groups))
                self._upload(dt, pt, gt, host)
                if dev not in self.spare:
                    self.spare[dev] = self._new_tables(dev, n, len(opt.param_groups))
            fi = ctypes_ptr(found_inf) if found_inf is not None else None
            with torch.cuda.device(dev):
                coef = None
                if clip:
                    L.check(L.load().mfx_grad_norm_multi(ctypes_ptr(dt), ctypes_ptr(pt), n, int(prefix[n]), float(max_norm), ctypes_ptr(ws), ws.numel(),
                                                         ctypes_ptr(out2), fi, ctypes_stream()), "mfx_grad_norm_multi")
                    self.grad_norm = out2
                    coef = ctypes_ptr(out2[1:])
                self._launch(dt, pt, n, int(prefix[n]), gt, len(opt.param_groups), coef, fi)

    def _decay_only(self, p):
        """Whether a held parameter WITHOUT a gradient still takes part in the step (the true-weight-decay rule shrinks it)."""
        return False

    def _group_wd(self, opt, gi, g):
        return g["weight_decay"]

    def _group_extra(self, opt):
        return b""

    def _launch(self, dt, pt, n, nchunk, gt, ngroups, coef, fi):
        from . import lib as L
        if self.rule == L.OPTIM_ADAMW and coef is None:                # the plain AdamW step: the launch it has always been
            L.check(L.load().mfx_adamw_multi(ctypes_ptr(dt), ctypes_ptr(pt), n, nchunk, ctypes_ptr(gt), fi, ctypes_stream()), "mfx_adamw_multi")
        else:
            L.check(L.load().mfx_optim_multi(ctypes_ptr(dt), ctypes_ptr(pt), n, nchunk, ctypes_ptr(gt), self.rule, coef, fi, ctypes_stream()), "mfx_optim_multi")

    @staticmethod
    def _upload(dt, pt, gt, host):
        dt[:host[0].numel()].copy_(host[0])
        pt[:host[1].numel()].copy_(host[1])
        gt[:host[2].numel()].copy_(host[2])

    def finish_capture(self):
        """Fill the tables of the launches recorded during a capture (call after the capture has ended, before the first replay)."""
        for dt, pt, gt, host in self.pending:
            self._upload(dt, pt, gt, host)
        self.pending = []
        if torch.cuda.is_available():
            torch.cuda.synchronize()


class MultiTensorAdam(MultiTensorAdamW):
    """The same driver for torch.optim.Adam (fused, capturable, device-scalar learning rates: `build_optimizer` with SOLVER.OPTIMIZER 'adam' on a GPU):
    L2 weight decay, g' = g + wd p, the arithmetic of torch's capturable `_fused_adam_` (mfx_optim_multi, rule MFX_OPTIM_ADAM_L2).  The state is torch's
    own {step, exp_avg, exp_avg_sq}, so state_dict() loads into a plain torch.optim.Adam."""
    optimizer_type = torch.optim.Adam
    rule = 1                      # lib.OPTIM_ADAM_L2


class MultiTensorAdamTrueWD(MultiTensorAdamW):
    """The same driver for an OptimWrapper (SOLVER.OPTIMIZER 'adam_onecycle' on a GPU): mfx_optim_multi_sched with rule MFX_OPTIM_ADAM_TRUE_WD.  `self._opt()`
    is the wrapper; param_groups and state are its inner Adam's.  Beside the learning rate the launch reads every group's `mom` device scalar as Adam's
    beta1 (a table of pointers behind the group records), so replays follow the OneCycle schedule; the wrapper's `wd` travels in the group record.
    A held parameter without a gradient becomes a decay-only row (the wrapper shrinks it, Adam skips it); with max_norm > 0 the gradients of the wrapper's
    `norm_only_params` join the tables as norm-only rows, so the norm is the one over model.parameters() while the update leaves them alone."""
    optimizer_type = OptimWrapper
    rule = 2                      # lib.OPTIM_ADAM_TRUE_WD
    group_extra_bytes = 8

    @classmethod
    def eligible(cls, optimizer):
        if not isinstance(optimizer, OptimWrapper) or type(optimizer.opt) is not torch.optim.Adam or not optimizer.true_wd:
            return False
        for g in optimizer.param_groups:
            if not g.get("capturable") or g.get("amsgrad") or g.get("maximize") or g.get("differentiable") or g.get("decoupled_weight_decay"):
                return False
            for s in (g["lr"], g.get("mom")):
                if not torch.is_tensor(s) or not s.is_cuda or s.dtype != torch.float32:
                    return False
            for p in g["params"]:
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous() or p.is_sparse:
                    return False
        return all(p.is_cuda and p.dtype == torch.float32 for p in optimizer.norm_only_params)

    def _norm_only(self, opt):
        return opt.norm_only_params

    def _decay_only(self, p):
        return p.requires_grad

    def _group_wd(self, opt, gi, g):
        return opt.wd if (gi % 2 == 0 or opt.bn_wd) else 0.0

    def _group_extra(self, opt):
        import numpy as np
        return np.asarray([g["mom"].data_ptr() for g in opt.param_groups], dtype=np.uint64).tobytes()

    def _launch(self, dt, pt, n, nchunk, gt, ngroups, coef, fi):
        import ctypes
        from . import lib as L
        beta1 = ctypes.c_void_p(gt.data_ptr() + ngroups * ctypes_sizeof(L.AdamWGroup))           # (8-byte aligned: the record is 24 bytes)
        L.check(L.load().mfx_optim_multi_sched(ctypes_ptr(dt), ctypes_ptr(pt), n, nchunk, ctypes_ptr(gt), beta1, self.rule, coef, fi, ctypes_stream()),
                "mfx_optim_multi_sched")


def multi_tensor_driver(optimizer):
    """The one-launch driver of `optimizer` (created on first use and kept on it), or None: not a GPU AdamW / Adam / OptimWrapper of `build_optimizer`'s
    making, or MFX_HIP_ADAMW=0 (torch's own kernels; for the wrapper its eager form)."""
    if not HIP_ADAMW[0]:
        return None
    mt = getattr(optimizer, "_mfx_multi", None)
    if mt is None:
        for cls in (MultiTensorAdamW, MultiTensorAdam, MultiTensorAdamTrueWD):
            if cls.eligible(optimizer):
                mt = optimizer._mfx_multi = cls(optimizer)
                break
    return mt


def ctypes_sizeof(t):
    import ctypes
    return ctypes.sizeof(t)


def ctypes_ptr(t):
    import ctypes
    return ctypes.c_void_p(t.data_ptr())


def ctypes_stream():
    import ctypes
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


HIP_ADAMW = [__import__("os").environ.get("MFX_HIP_ADAMW", "1") != "0"]      # MFX_HIP_ADAMW=0: torch's own fused AdamW step (A/B)


def optimizer_step(optimizer, max_norm=-1.0):
    """`optimizer.step()`; a GPU AdamW / Adam / OptimWrapper built by `build_optimizer` takes the one-launch HIP form (MultiTensorAdamW / MultiTensorAdam /
    MultiTensorAdamTrueWD) -- eagerly and
    inside captures alike, so a replayed step and an eager step stay the same arithmetic.  `max_norm` > 0: the clipped update (gradient norm + coefficient
    as part of that form); a caller whose optimizer has no such driver (`multi_tensor_driver` is None) clips with torch's function first and passes nothing."""
    mt = multi_tensor_driver(optimizer)
    if mt is None:
        if max_norm is not None and float(max_norm) > 0:
            raise ValueError("optimizer_step: max_norm needs the one-launch driver; clip with torch.nn.utils.clip_grad_norm_ first (engine/trainer.py)")
        return optimizer.step()
    return mt.step(max_norm)


def finish_capture(optimizer):
    mt = getattr(optimizer, "_mfx_multi", None)
    if mt is not None:
        mt.finish_capture()
