"""SOLVER.OPTIMIZER 'adam_onecycle' on the device: the one-launch update that reads beta1 from the device (csrc/adamw.hip mfx_optim_multi_sched, rule
MFX_OPTIM_ADAM_TRUE_WD; monoflex_amd/solver.MultiTensorAdamTrueWD) against the wrapper's eager form (solver.OptimWrapper.step: the reference's
arithmetic in torch operations, pinned to the reference by tests/test_onecycle_cpu.py), against the reference's recorded trajectory
(tests/golden/onecycle.npz), replayed from a graph while the schedule moves lr and mom, with norm-only rows under the gradient clip, and as the
optimizer of a whole GraphedTrainStep.  Tensor shapes: tests/test_gpu_optim.py `_params` (ragged sizes, more than one chunk, a storage that is not
16-byte aligned) and the golden's stand-in tree (tests/onecycle_cases.py).

Bounds.  Parameters and moments against the eager form: tests/test_gpu_optim.py's 2e-6 (max |difference| / max |value|).  total_norm and coef: the
bounds derived in tests/test_gpu_optim_recipes.py (2e-6 relative against the float64 norm; 2 * 2^-24 on torch's rule evaluated on the kernel's norm)."""
import os

import pytest
import torch

from onecycle_cases import SETTINGS, STEPS_KEPT, golden_tree, load_golden, rel, set_grads
from test_gpu_optim import DEV, _params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _s(v):
    return torch.tensor(float(v), dtype=torch.float32, device=DEV)


def _wrap(ps, wd=1e-2, norm_only=()):
    from monoflex_amd.solver import OptimWrapper
    groups = [{"params": ps[::2], "lr": _s(3e-3), "mom": _s(0.95)}, {"params": ps[1::2], "lr": _s(3e-3), "mom": _s(0.95)}]
    inner = torch.optim.Adam(groups, lr=_s(3e-3), betas=(0.95, 0.99), fused=True, capturable=True)
    return OptimWrapper(inner, wd=wd, true_wd=True, bn_wd=True, norm_only_params=norm_only)


def _counters():
    from monoflex_amd import lib as L
    return {k: L.load().mfx_get_counter(k.encode()) for k in ("adamw_multi", "optim_multi", "optim_multi_sched", "grad_norm_multi")}


def _rel(x, y):
    return float((x.detach() - y.detach()).abs().max() / x.detach().abs().max().clamp(min=1e-30))


def test_hip_update_follows_the_eager_wrapper():
    """Six steps, lr and mom rewritten between steps (for both groups, then for one), a found_inf skip at step 3, weight decay 1e-2; parameter 1 never
    gets a gradient (the wrapper shrinks it all the same: a decay-only row).  Both sides read the same fp32 scalars."""
    from monoflex_amd.solver import MultiTensorAdam, MultiTensorAdamTrueWD, MultiTensorAdamW, multi_tensor_driver, optimizer_step
    a, b = _params(1), _params(1)
    oa, ob = _wrap(a), _wrap(b)
    assert MultiTensorAdamTrueWD.eligible(ob) and not MultiTensorAdam.eligible(ob) and not MultiTensorAdamW.eligible(ob)
    assert type(multi_tensor_driver(ob)) is MultiTensorAdamTrueWD
    found = torch.zeros((), dtype=torch.float32, device=DEV)
    oa.found_inf = ob.found_inf = found
    g = torch.Generator().manual_seed(9)
    c0 = _counters()
    worst = 0.0
    for it in range(6):
        skip = it == 3                                                      # a skipped step: nothing may move, counters and the shrink included
        found.fill_(1.0 if skip else 0.0)
        before = [p.detach().clone() for p in b]
        for i, (pa, pb) in enumerate(zip(a, b)):
            gr = torch.randn(pa.shape, generator=g).to(DEV) * (10.0 ** (it - 3))
            pa.grad, pb.grad = (None, None) if i == 1 else (gr.clone(), gr.clone())
        for o in (oa, ob):
            o.lr, o.mom = 3e-3 * (1 + it) / 6, 0.95 - 0.02 * it             # the schedule writes the device scalars between steps
            if it == 4:
                o.param_groups[1]["lr"].fill_(1e-3)
                o.param_groups[1]["mom"].fill_(0.9)
        assert torch.equal(oa.param_groups[0]["mom"], ob.param_groups[0]["mom"]) and torch.equal(oa.param_groups[1]["lr"], ob.param_groups[1]["lr"])
        oa.step()
        optimizer_step(ob)
        torch.cuda.synchronize()
        for i, (pa, pb) in enumerate(zip(a, b)):
            assert _rel(pa, pb) < 2e-6, (it, i, "param", _rel(pa, pb))
            worst = max(worst, _rel(pa, pb))
            assert torch.equal(pb, before[i]) == skip, (it, i)                # (the decay-only parameter moves too: shrunk)
            if i == 1:
                assert pb not in ob.state and pa not in oa.state
                continue
            sa, sb = oa.state[pa], ob.state[pb]
            assert float(sa["step"]) == float(sb["step"]) == (it + 1 - (1 if it >= 3 else 0)), (it, i)
            for x, y, name in ((sa["exp_avg"], sb["exp_avg"], "exp_avg"), (sa["exp_avg_sq"], sb["exp_avg_sq"], "exp_avg_sq")):
                assert _rel(x, y) < 2e-6, (it, i, name, _rel(x, y))
                worst = max(worst, _rel(x, y))
    print("HIP against the eager wrapper: max rel %.3e" % worst)
    c1 = _counters()
    assert c1["optim_multi_sched"] == c0["optim_multi_sched"] + 6
    assert all(c1[k] == c0[k] for k in ("adamw_multi", "optim_multi", "grad_norm_multi"))


def test_hip_update_follows_the_reference_trajectory():
    """Eight steps on the recorded tree and gradients under the recorded schedule, against the reference's parameters and moments after steps 1, 4, 8.
    The CPU form measures 0.0 against the golden (tests/test_onecycle_cpu.py); the device form adds the fp32 rounding of lr and mom -- mom enters through
    w1 = 1 - b1 >= 0.05, up to 2^-24 / 0.05 = 1.2e-6 relative per step -- and fp32 evaluation order.
    Measured on an MI355X: max |difference| / max |value| = 1.021e-6 over every tensor and kept step (MEASURED_REL); the bound is 4 x that, 4.1e-6, and
    stays below the recorder's teeth (dropping the decay moves the end point by 4.6e-5, freezing mom by 8.7e-5)."""
    from monoflex_amd.config import get_cfg
    from monoflex_amd.solver import build_optimizer, build_scheduler, optimizer_step
    golden = load_golden()
    bound = 4 * MEASURED_REL
    assert bound < float(golden["teeth_wd0"]) and bound < float(golden["teeth_mom"])
    cfg = get_cfg(os.path.join(ROOT, "runs", "monoflex.yaml"), ["SOLVER.OPTIMIZER", "adam_onecycle"])
    s = cfg.SOLVER
    s.BASE_LR, s.MOMS, s.DIV_FACTOR, s.WEIGHT_DECAY = SETTINGS["BASE_LR"], SETTINGS["MOMS"], SETTINGS["DIV_FACTOR"], SETTINGS["WEIGHT_DECAY"]
    s.PCT_START, s.MAX_ITERATION, s.LR_WARMUP = 0.4, 40, False
    m = golden_tree(golden, DEV)
    opt = build_optimizer(m, cfg)
    assert all(g["capturable"] and torch.is_tensor(g["lr"]) and torch.is_tensor(g["mom"]) and g["mom"].is_cuda for g in opt.param_groups)
    sched, _ = build_scheduler(opt, total_iters_each_epoch=10, optim_cfg=s)
    names = {id(p): n for n, p in m.named_parameters()}
    c0 = _counters()
    worst = 0.0
    for it in range(8):
        opt.zero_grad()
        set_grads(m, golden, it)
        optimizer_step(opt)
        sched.step(it)
        if it + 1 in STEPS_KEPT:
            for n, p in m.named_parameters():
                worst = max(worst, rel(p, golden["p/%d/%s" % (it + 1, n)]))
            for p, st in opt.state.items():
                worst = max(worst, rel(st["exp_avg"], golden["m/%d/%s" % (it + 1, names[id(p)])]), rel(st["exp_avg_sq"], golden["v/%d/%s" % (it + 1, names[id(p)])]))
    print("HIP against the golden: max rel %.3e (bound %.3e)" % (worst, bound))
    assert _counters()["optim_multi_sched"] == c0["optim_multi_sched"] + 8
    assert worst <= bound, worst
    assert torch.equal(m.dcn.weight.cpu(), torch.from_numpy(golden["init/dcn.weight"]))


MEASURED_REL = 1.021e-6


@pytest.mark.parametrize("clip", [-1.0, 10.0])
def test_update_replays_from_a_graph_while_the_schedule_moves(clip):
    """One captured step replayed three times with lr.fill_ / mom.fill_ between replays, next to an eager HIP optimizer on the same inputs: bit-equal
    parameters, moments and step counters (and [total_norm, coef] with the clip, whose norm covers a norm-only tensor).  A beta1 baked into the
    captured launch fails here."""
    from monoflex_amd.solver import finish_capture, optimizer_step
    a, b = _params(2), _params(2)
    xa, xb = (torch.nn.Parameter(torch.randn(5000, generator=torch.Generator().manual_seed(4)).to(DEV)) for _ in range(2))
    oa, ob = _wrap(a, norm_only=[xa]), _wrap(b, norm_only=[xb])
    g = torch.Generator().manual_seed(3)
    for pa, pb in zip(a + [xa], b + [xb]):
        gr = torch.randn(pa.shape, generator=g).to(DEV)
        pa.grad, pb.grad = gr.clone(), gr.clone()
    optimizer_step(ob, clip)                                                 # eager first step: state and tables exist
    optimizer_step(oa, clip)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            optimizer_step(ob, clip)
    finish_capture(ob)
    x0 = xb.detach().clone()
    for it in range(3):
        for pa, pb in zip(a + [xa], b + [xb]):
            gr = torch.randn(pa.shape, generator=g).to(DEV) * (1e-3 if it == 1 else 1.0)
            pa.grad.copy_(gr)
            pb.grad.copy_(gr)
        for o in (oa, ob):
            o.lr, o.mom = 1e-3 * (it + 1), 0.93 - 0.04 * it
        moved = [p.detach().clone() for p in b]
        optimizer_step(oa, clip)
        graph.replay()
        torch.cuda.synchronize()
        for pa, pb, pm in zip(a, b, moved):
            assert torch.equal(pa, pb) and not torch.equal(pb, pm) and float(oa.state[pa]["step"]) == float(ob.state[pb]["step"]) == it + 2
            assert torch.equal(oa.state[pa]["exp_avg"], ob.state[pb]["exp_avg"]) and torch.equal(oa.state[pa]["exp_avg_sq"], ob.state[pb]["exp_avg_sq"])
        assert torch.equal(xb, x0) and xb not in ob.state
        if clip > 0:
            assert torch.equal(oa._mfx_multi.grad_norm, ob._mfx_multi.grad_norm)
            assert (float(ob._mfx_multi.grad_norm[1]) == 1.0) == (it == 1)


def test_norm_only_rows_join_the_norm_and_nothing_else():
    from monoflex_amd.solver import optimizer_step
    max_norm = 10.0
    b, u = _params(5), _params(5)
    gen = torch.Generator().manual_seed(12)
    extra = [torch.nn.Parameter(torch.randn(s, generator=gen).to(DEV)) for s in ((4096 + 3,), (6, 4, 3, 3))]
    ob, ou = _wrap(b, norm_only=extra), _wrap(u)
    g = torch.Generator().manual_seed(6)
    for p, q in zip(b + extra, u + [None, None]):
        p.grad = torch.randn(p.shape, generator=g).to(DEV)
        if q is not None:
            q.grad = p.grad.clone()
    grads = [p.grad.clone() for p in b + extra]
    want_norm = float(torch.sqrt(sum((gr.double() ** 2).sum() for gr in grads)))
    held_norm = float(torch.sqrt(sum((gr.double() ** 2).sum() for gr in grads[:len(b)])))
    before = [p.detach().clone() for p in extra]
    c0 = _counters()
    optimizer_step(ob, max_norm)
    optimizer_step(ou, max_norm)                                             # the same step without the extra rows: another norm, another coef
    torch.cuda.synchronize()
    c1 = _counters()
    assert c1["grad_norm_multi"] == c0["grad_norm_multi"] + 2 and c1["optim_multi_sched"] == c0["optim_multi_sched"] + 2 and c1["optim_multi"] == c0["optim_multi"]
    total, coef = (float(x) for x in ob._mfx_multi.grad_norm)
    print("total_norm %.9g (float64 %.9g, rel %.2e; held only %.9g) coef %.9g" % (total, want_norm, abs(total - want_norm) / want_norm, held_norm, coef))
    assert abs(total - want_norm) <= 2e-6 * want_norm and abs(total - held_norm) > 1e-3 * want_norm
    assert abs(float(ou._mfx_multi.grad_norm[0]) - held_norm) <= 2e-6 * held_norm
    want_coef = float(torch.clamp(max_norm / (torch.tensor(total, dtype=torch.float32) + 1e-6), max=1.0))     # torch's rule on the kernel's own norm
    assert abs(coef - want_coef) <= 2 * 2.0 ** -24 * want_coef and coef < 1.0
    for p, q, gr in zip(extra, before, grads[len(b):]):
        assert torch.equal(p, q) and torch.equal(p.grad, gr) and p not in ob.state
    assert len(ob.state) == len(b) and all(float(ob.state[p]["step"]) == 1.0 for p in b)
    assert any(not torch.equal(p, q) for p, q in zip(b, u))                  # the larger norm scaled the held gradients further down


def test_whole_step_graphed_equals_eager_pieces():
    """GraphedTrainStep with the wrapper on the smallest model and batch of tests/test_gpu_train_recipes.py (B = 2 at 128 x 384, fp32, GRAD_NORM_CLIP 10,
    deterministic reductions), SOLVER.OPTIMIZER adam_onecycle, MAX_ITERATION 6: three replays with the schedule advanced between them against the
    use_graphs=False loop -- equal losses, parameters, buffers and moments, bit for bit as that file asks for `adam`; DCN weights never move."""
    import copy
    from monoflex_amd import lib as L
    from monoflex_amd.engine.trainer import GraphedTrainStep, advance_schedule
    from monoflex_amd.solver import MultiTensorAdamTrueWD, OptimWrapper, build_optimizer, build_scheduler, multi_tensor_driver
    from test_gpu_train_recipes import _batch, _cfg, _model
    L.set_deterministic(True)
    try:
        cfg = _cfg("fp32", ["SOLVER.OPTIMIZER", "adam_onecycle", "SOLVER.MAX_ITERATION", 6, "SOLVER.LR_WARMUP", False])
        clip = cfg.SOLVER.GRAD_NORM_CLIP
        assert clip == 10.0
        b = _model("fp32")
        imgs, tg = _batch(b)
        opt_b = build_optimizer(b, cfg)
        assert type(opt_b) is OptimWrapper and type(multi_tensor_driver(opt_b)) is MultiTensorAdamTrueWD and len(opt_b.norm_only_params) >= 12
        sched_b, _ = build_scheduler(opt_b, total_iters_each_epoch=1, optim_cfg=cfg.SOLVER)
        c0 = _counters()
        step = GraphedTrainStep(b, opt_b, imgs, tg, warmup=2, grad_norm_clip=clip)
        assert step.use_graphs and len(step.graphs) == 1
        torch.cuda.synchronize()
        c1 = _counters()
        assert c1["optim_multi_sched"] > c0["optim_multi_sched"] and c1["grad_norm_multi"] > c0["grad_norm_multi"]
        assert c1["optim_multi"] == c0["optim_multi"] and c1["adamw_multi"] == c0["adamw_multi"]
        model_sd = {k: v.detach().clone() for k, v in b.state_dict().items()}
        a = _model("fp32", seed=5)
        a.load_state_dict(model_sd)
        opt_a = build_optimizer(a, cfg)
        opt_a.load_state_dict(copy.deepcopy(opt_b.state_dict()))
        sched_a, _ = build_scheduler(opt_a, total_iters_each_epoch=1, optim_cfg=cfg.SOLVER)
        eager = GraphedTrainStep(a, opt_a, imgs, tg, use_graphs=False, grad_norm_clip=clip)
        seen = set()
        for it in range(3):
            assert torch.equal(opt_a.param_groups[0]["lr"], opt_b.param_groups[0]["lr"]) and torch.equal(opt_a.param_groups[1]["mom"], opt_b.param_groups[1]["mom"])
            seen.add((opt_b.lr, opt_b.mom))
            loss_b = step().clone()
            loss_a = eager().clone()
            torch.cuda.synchronize()
            assert bool(torch.isfinite(loss_a)) and torch.equal(loss_a, loss_b), (it, float(loss_a), float(loss_b))
            sa, sb = a.state_dict(), b.state_dict()
            diff = [k for k in sa if not torch.equal(sa[k], sb[k])]
            assert not diff, (it, diff[:8])
            n_state = 0
            for ga, gb in zip(opt_a.param_groups, opt_b.param_groups):
                for x, y in zip(ga["params"], gb["params"]):
                    if x in opt_a.state:
                        n_state += 1
                        for key in ("exp_avg", "exp_avg_sq", "step"):
                            assert torch.equal(opt_a.state[x][key], opt_b.state[y][key]), (it, key)
                        assert float(opt_b.state[y]["step"]) == it + 1
            assert n_state > 200
            na, nb = opt_a._mfx_multi.grad_norm, opt_b._mfx_multi.grad_norm
            assert torch.equal(na, nb) and 0.0 < float(nb[0]) < float("inf") and 0.0 < float(nb[1]) <= 1.0
            for sched in (sched_a, sched_b):
                advance_schedule(it, -1, sched, None)
        assert len(seen) == 2                                                # iterations 0 and 1 share the constructor's values; iteration 2 has moved on
        own = [n + "." + k for n, mod in b.named_modules() if type(mod).__name__ == "DCN" for k, _ in mod.named_parameters(recurse=False)]
        assert len(own) >= 12 and all(torch.equal(b.state_dict()[k], model_sd[k]) for k in own)
        moved = [n for n, p in b.named_parameters() if not torch.equal(p, model_sd[n])]
        assert len(moved) > 200 and not (set(moved) & set(own))
    finally:
        L.set_deterministic(False)
