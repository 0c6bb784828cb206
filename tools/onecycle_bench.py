"""Timing of the optimizer step of SOLVER.OPTIMIZER 'adam_onecycle' over the real parameter set of the B = 8 model (runs/monoflex.yaml KeypointDetector,
about 20 M fp32 parameters), three ways on the same tensors and gradients:
  hip_sched     the one-launch update reading lr and beta1 from the device (mfx_optim_multi_sched, rule MFX_OPTIM_ADAM_TRUE_WD; solver.optimizer_step)
  eager_wrapper the wrapper's eager form (solver.OptimWrapper.step: one mul_ per parameter, then torch's fused Adam; the lr / mom reads synchronise)
  adamw_multi   mfx_adamw_multi through its driver over the SAME tensors (a capturable AdamW built on the wrapper's two groups; the DCN layers' own
                weights, which the wrapper does not hold, are left out here too): the yardstick -- the same traffic (read p, g, m, v; write p, m, v)
20 warm-up steps each, then REPS windows of ITERS steps between two device events, the three taking turns inside a repetition; the median window and the
spread are printed as one JSON line.  Back-to-back steps on ~495 MB of traffic (17.7 M held parameters x 28 bytes): the figure is the update kernel's time plus the step-counter launch and
the host's table upload.  Carries no threshold.      python tools/onecycle_bench.py [--iters N] [--reps R]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from monoflex_amd.config import get_cfg                         # noqa: E402
from monoflex_amd.model.detector import KeypointDetector        # noqa: E402
from monoflex_amd.solver import MultiTensorAdamTrueWD, MultiTensorAdamW, build_optimizer, build_scheduler, multi_tensor_driver, optimizer_step   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()
WARM = 20
if not torch.cuda.is_available():
    raise SystemExit("onecycle_bench: needs a GPU (a timing taken elsewhere says nothing)")


def cfg_for(optimizer):
    cfg = get_cfg(os.path.join(ROOT, "runs", "monoflex.yaml"), ["SOLVER.OPTIMIZER", optimizer, "SOLVER.LR_WARMUP", False])
    cfg.MODEL.PRETRAIN = False
    return cfg


torch.manual_seed(0)
model = KeypointDetector(cfg_for("adamw")).cuda().train()
gen = torch.Generator(device="cuda").manual_seed(1)
for p in model.parameters():
    if p.requires_grad:
        p.grad = torch.randn(p.shape, generator=gen, device="cuda") * 1e-3
one_hip, one_eager = build_optimizer(model, cfg_for("adam_onecycle")), build_optimizer(model, cfg_for("adam_onecycle"))
lr = lambda: torch.tensor(3e-4, dtype=torch.float32, device="cuda")      # noqa: E731
adamw = torch.optim.AdamW([{"params": g["params"], "lr": lr()} for g in one_hip.param_groups], lr=lr(), weight_decay=1e-5, betas=(0.9, 0.99), fused=True, capturable=True)
for o in (one_hip, one_eager):
    build_scheduler(o, total_iters_each_epoch=1, optim_cfg=cfg_for("adam_onecycle").SOLVER, last_epoch=1000)       # a position inside the cycle
assert type(multi_tensor_driver(one_hip)) is MultiTensorAdamTrueWD and type(multi_tensor_driver(adamw)) is MultiTensorAdamW
entries = {"hip_sched": lambda: optimizer_step(one_hip), "eager_wrapper": one_eager.step, "adamw_multi": lambda: optimizer_step(adamw)}


def window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n                                    # milliseconds per step


for fn in entries.values():
    window(fn, WARM)
samples = {n: [] for n in entries}
for _ in range(args.reps):
    for n, fn in entries.items():
        samples[n].append(window(fn, args.iters))
held = sum(p.numel() for g in one_hip.param_groups for p in g["params"])
res = {"what": "optimizer step over the B = 8 model's parameters: adam_onecycle by the one-launch HIP update, by the wrapper's eager form, and mfx_adamw_multi",
       "parameters": {"model": sum(p.numel() for p in model.parameters() if p.requires_grad), "held_by_the_wrapper": held,
                      "tensors_held": sum(len(g["params"]) for g in one_hip.param_groups), "norm_only_tensors": len(one_hip.norm_only_params)},
       "warmup": WARM, "steps_per_window": args.iters, "windows": args.reps,
       "ms_per_step": {n: {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for n, v in samples.items()}}
print(json.dumps(res))
