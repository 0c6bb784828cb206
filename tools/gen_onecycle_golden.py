#!/usr/bin/env python
"""Recorder of tests/golden/onecycle.npz: the reference's own SOLVER.OPTIMIZER 'adam_onecycle' -- its fastai OptimWrapper over optim.Adam and its
OneCycle schedule -- driven as its training loop drives them (engine/trainer.py:116-126: zero_grad, backward, step, `scheduler.step(iteration)`).

Sibling of oracle/gen_lr_golden.py, through which it imports: the same route (the reference checkout that script names, read-only) and the same
in-process patch (`collections.Iterable`, removed in Python 3.10; the reference's fastai_optim imports it).  Data only.  Run from the repository root:

    python tools/gen_onecycle_golden.py

Stored:
  trace_40_04 / trace_37_03   (lr, mom) BEFORE every iteration for (MAX_ITERATION 40, PCT_START 0.4) and (37, 0.3), where int() truncates the
                              phase boundary (int(37 * 0.3) = 11)
  held_0 / held_1 / left_out  names of the stand-in tree's parameters in the two param groups (in group order) and of the trainable ones in neither
  init/<name>                 initial values of every parameter of the tree
  grad/<it>/<name>            the gradients of iteration it = 0..7 (seeded, scaled by 10 ** (it - 3)), stored so that no test depends on a generator
  p|m|v/<step>/<name>         every parameter and both Adam moments of the held ones after steps 1, 4 and 8 of the 40-iteration case
  param_groups                the inner optimizer's state_dict()["param_groups"] after step 8, as JSON
  teeth_wd0 / teeth_mom       max |difference| / max |value| of the same run with wd = 0, and with mom frozen at 0.95, against the recorded one
The stand-in tree (tests/onecycle_cases.py `Tree`): a leaf conv, a leaf BatchNorm2d, a module that owns a Parameter AND has a child conv (the shape of DCN: its own
parameter is in no group), a leaf holding one frozen parameter, and parameters of 2 * 4096 + 5 and of 7 elements.
Settings: BASE_LR 3e-3, MOMS [0.95, 0.85], DIV_FACTOR 10, WEIGHT_DECAY 0.01 (at the shipped 1e-5 the factor 1 - 3e-8 rounds to 1.0f: the decay
could not be seen)."""
import json
import os
import sys

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(REPO)
from oracle import gen_lr_golden as _route                      # noqa: E402,F401  (names the reference checkout, patches collections.Iterable, imports ITS solver)
import numpy as np                                              # noqa: E402
import torch                                                    # noqa: E402
from solver import build_optimizer, build_scheduler             # noqa: E402  (the reference's: already imported by that route)

sys.path.insert(0, os.path.join(REPO, "tests"))
from monoflex_amd.config import get_cfg                         # noqa: E402
from onecycle_cases import make_tree                            # noqa: E402  (the stand-in tree, shared with the tests)

STEPS_KEPT = (1, 4, 8)
TOL = 1e-7                                                      # the tolerance the teeth are counted in: the bound of tests/test_onecycle_cpu.py's trajectory test


def cfg_for(total, pct, wd):
    cfg = get_cfg(os.path.join(REPO, "runs", "monoflex.yaml"))
    s = cfg.SOLVER
    s.OPTIMIZER, s.BASE_LR, s.MOMS, s.DIV_FACTOR, s.PCT_START, s.WEIGHT_DECAY = "adam_onecycle", 3e-3, [0.95, 0.85], 10.0, pct, wd
    s.MAX_ITERATION, s.LR_WARMUP, s.STEPS = total, False, [total]
    return cfg


def make_grads(m, iters=8, seed=23):
    g = torch.Generator().manual_seed(seed)
    return [{n: torch.randn(p.shape, generator=g) * (10.0 ** (it - 3)) for n, p in m.named_parameters() if p.requires_grad} for it in range(iters)]


def run(total, pct, wd=0.01, grads=None, freeze_mom=False, iters=None):
    """-> (trace, model, optimizer, snapshots) of the reference's loop."""
    cfg = cfg_for(total, pct, wd)
    m = make_tree()
    opt = build_optimizer(m, cfg)
    sched, warm = build_scheduler(opt, total_iters_each_epoch=10, optim_cfg=cfg.SOLVER)
    assert warm is None
    names = {id(p): n for n, p in m.named_parameters()}
    trace, snaps = [], {}
    for it in range(total if iters is None else iters):
        trace.append([float(opt.lr), float(opt.mom)])
        opt.zero_grad()
        for n, p in m.named_parameters():
            if p.requires_grad:
                p.grad = (grads[it][n].clone() if grads is not None and it < len(grads) else torch.zeros_like(p))
        opt.step()
        sched.step(it)
        if freeze_mom:
            opt.mom = 0.95
        if it + 1 in STEPS_KEPT:
            snaps[it + 1] = {"p": {n: p.detach().clone() for n, p in m.named_parameters()},
                             "m": {names[id(p)]: st["exp_avg"].clone() for p, st in opt.opt.state.items()},
                             "v": {names[id(p)]: st["exp_avg_sq"].clone() for p, st in opt.opt.state.items()}}
    return trace, m, opt, snaps


def rel(a, b):
    return max(float((a[n] - b[n]).abs().max() / a[n].abs().max().clamp(min=1e-30)) for n in a)


if __name__ == "__main__":
    out = {}
    out["trace_40_04"] = np.asarray(run(40, 0.4)[0], dtype=np.float64)
    out["trace_37_03"] = np.asarray(run(37, 0.3)[0], dtype=np.float64)
    grads = make_grads(make_tree())
    _, m, opt, snaps = run(40, 0.4, grads=grads, iters=8)
    names = {id(p): n for n, p in m.named_parameters()}
    held = [[names[id(p)] for p in g["params"]] for g in opt.opt.param_groups]
    assert len(held) == 2
    left = [n for n, p in m.named_parameters() if p.requires_grad and n not in held[0] + held[1]]
    assert left == ["dcn.weight"] and "dcn.conv_offset_mask.weight" in held[0] and held[1] == ["bn.weight", "bn.bias"] and "frozen.value" not in held[0]
    out["held_0"], out["held_1"], out["left_out"] = np.asarray(held[0]), np.asarray(held[1]), np.asarray(left)
    for n, p in make_tree().named_parameters():
        out["init/" + n] = p.detach().numpy()
    for it, gd in enumerate(grads):
        for n, v in gd.items():
            out["grad/%d/%s" % (it, n)] = v.numpy()
    for k, sn in snaps.items():
        for kind in ("p", "m", "v"):
            for n, v in sn[kind].items():
                out["%s/%d/%s" % (kind, k, n)] = v.numpy()
    assert torch.equal(snaps[8]["p"]["dcn.weight"], make_tree().dcn.weight) and torch.equal(snaps[8]["p"]["frozen.value"], make_tree().frozen.value)
    out["param_groups"] = np.asarray(json.dumps(opt.opt.state_dict()["param_groups"]))
    # teeth: without the decay, and with beta1 frozen at its first value, the same run ends more than 100 tolerances away
    held_names = held[0] + held[1]
    want = {n: snaps[8]["p"][n] for n in held_names}
    for key, kw in (("teeth_wd0", dict(wd=0.0)), ("teeth_mom", dict(freeze_mom=True))):
        other = run(40, 0.4, grads=grads, iters=8, **kw)[3][8]["p"]
        d = rel(want, {n: other[n] for n in held_names})
        assert d > 100 * TOL, (key, d)
        out[key] = np.asarray(d)
    out["meta"] = np.asarray("reference solver.build_optimizer / build_scheduler with SOLVER.OPTIMIZER adam_onecycle, driven as engine/trainer.py:116-126; "
                             "BASE_LR 3e-3, MOMS [0.95, 0.85], DIV_FACTOR 10, WEIGHT_DECAY 0.01; traces are [lr, mom] before each iteration")
    path = os.path.join(REPO, "tests", "golden", "onecycle.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; teeth wd0 %.3e mom %.3e" % (float(out["teeth_wd0"]), float(out["teeth_mom"])))
