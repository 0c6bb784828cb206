"""SOLVER.OPTIMIZER 'adam_onecycle' on the CPU: solver.OptimWrapper (the reference's fastai wrapper, solver/fastai_optim.py, true weight decay around
optim.Adam) and solver.OneCycle (solver/learning_schedules_fastai.py) against tests/golden/onecycle.npz, which tools/gen_onecycle_golden.py recorded
from the reference's own build_optimizer / build_scheduler driven as its loop drives them (engine/trainer.py:116-126).  The wrapper's eager form
tested here is also the form tests/test_gpu_onecycle.py compares the one-launch HIP update with."""
import copy
import os

import numpy as np
import pytest
import torch

from onecycle_cases import SETTINGS, STEPS_KEPT, golden_tree, load_golden, rel, set_grads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACES = {"trace_40_04": (40, 0.4), "trace_37_03": (37, 0.3)}


@pytest.fixture(scope="module")
def golden():
    return load_golden()


def _cfg(total=40, pct=0.4, warmup=False):
    from monoflex_amd.config import get_cfg
    cfg = get_cfg(os.path.join(ROOT, "runs", "monoflex.yaml"), ["SOLVER.OPTIMIZER", "adam_onecycle"])
    s = cfg.SOLVER
    s.BASE_LR, s.MOMS, s.DIV_FACTOR, s.WEIGHT_DECAY = SETTINGS["BASE_LR"], SETTINGS["MOMS"], SETTINGS["DIV_FACTOR"], SETTINGS["WEIGHT_DECAY"]
    s.PCT_START, s.MAX_ITERATION, s.LR_WARMUP, s.WARMUP_STEPS, s.STEPS = pct, total, warmup, 5, [total]
    return cfg


def _built(golden, total=40, pct=0.4, last_epoch=-1):
    from monoflex_amd.solver import build_optimizer, build_scheduler
    cfg = _cfg(total, pct)
    m = golden_tree(golden)
    opt = build_optimizer(m, cfg)
    sched, warm = build_scheduler(opt, total_iters_each_epoch=10, optim_cfg=cfg.SOLVER, last_epoch=last_epoch)
    assert warm is None
    return m, opt, sched


@pytest.mark.parametrize("name", sorted(TRACES))
def test_schedule_reproduces_the_recorded_trace(golden, name):
    """(lr, mom) before every iteration, driven by engine.trainer.advance_schedule after a (zero-gradient) optimizer step, to 1e-12 relative: the same
    four double operations and np.cos.  Also: the boundary iteration a1 = int(total * pct) starts the second phase at (lr_max, moms[1]); the last
    iteration; `last_epoch = k` gives row k + 1; the group values are what the properties report."""
    from monoflex_amd.engine.trainer import advance_schedule
    from monoflex_amd.solver import OneCycle
    total, pct = TRACES[name]
    want = golden[name]
    assert want.shape == (total, 2)
    m, opt, sched = _built(golden, total, pct)
    assert type(sched) is OneCycle
    for it in range(total):
        got = (opt.lr, opt.mom)
        assert all(g["lr"] == got[0] and g["mom"] == got[1] and g["betas"] == (got[1], 0.99) for g in opt.param_groups)
        np.testing.assert_allclose(got, want[it], rtol=1e-12, atol=0, err_msg="iteration %d" % it)
        for p in m.parameters():
            p.grad = torch.zeros_like(p) if p.requires_grad else None
        opt.step()
        advance_schedule(it, -1, sched, None)
    a1 = int(total * pct)
    assert a1 == {40: 16, 37: 11}[total]
    np.testing.assert_allclose(want[a1 + 1], [SETTINGS["BASE_LR"], SETTINGS["MOMS"][1]], rtol=1e-12)     # step(a1): pct 0 of the second phase
    np.testing.assert_allclose(sched.values(a1), want[a1 + 1], rtol=1e-12)
    np.testing.assert_allclose(sched.values(total - 2), want[total - 1], rtol=1e-12)
    assert want[a1, 0] < SETTINGS["BASE_LR"] and want[total - 1, 0] < want[total - 2, 0] and want[total - 1, 1] > want[total - 2, 1]
    for k in (0, a1 - 1, a1, total - 2):
        _, opt_k, _ = _built(golden, total, pct, last_epoch=k)
        np.testing.assert_allclose((opt_k.lr, opt_k.mom), want[k + 1], rtol=1e-12, err_msg="last_epoch %d" % k)


def test_lr_warmup_is_refused(golden):
    from monoflex_amd.solver import build_optimizer, build_scheduler
    cfg = _cfg(warmup=True)
    opt = build_optimizer(golden_tree(golden), cfg)
    with pytest.raises(ValueError, match="assert warmup_scheduler is not None"):
        build_scheduler(opt, total_iters_each_epoch=10, optim_cfg=cfg.SOLVER)


def test_unknown_optimizer_names_what_is_served():
    from monoflex_amd.solver import build_optimizer
    cfg = _cfg()
    cfg.SOLVER.OPTIMIZER = "lamb"
    with pytest.raises(NotImplementedError, match="adamw, adam, sgd and adam_onecycle are all served"):
        build_optimizer(torch.nn.Linear(2, 2), cfg)


def test_group_layout_on_the_stand_in(golden):
    from monoflex_amd.solver import OptimWrapper
    m, opt, _ = _built(golden)
    assert type(opt) is OptimWrapper and type(opt.opt) is torch.optim.Adam and opt.true_wd and opt.bn_wd and opt.wd == SETTINGS["WEIGHT_DECAY"]
    names = {id(p): n for n, p in m.named_parameters()}
    held = [[names[id(p)] for p in g["params"]] for g in opt.param_groups]
    assert held == [list(golden["held_0"]), list(golden["held_1"])]
    assert [names[id(p)] for p in opt.norm_only_params] == list(golden["left_out"]) == ["dcn.weight"]
    assert "frozen.value" not in held[0] + held[1]


def test_group_layout_on_the_detector():
    """Every DCN module's own weight / bias is trainable, in `norm_only_params` and in no group; its conv_offset_mask.* is held; BatchNorm leaves make
    up group 1 (InPlaceABN is not a BatchNorm type: group 0); both groups share lr, mom and wd (no BIAS_LR_FACTOR)."""
    from monoflex_amd.config import get_cfg
    from monoflex_amd.model.detector import KeypointDetector
    from monoflex_amd.solver import BN_TYPES, build_optimizer
    cfg = get_cfg(os.path.join(ROOT, "runs", "monoflex.yaml"), ["SOLVER.OPTIMIZER", "adam_onecycle"])
    cfg.MODEL.PRETRAIN = False
    m = KeypointDetector(cfg)
    opt = build_optimizer(m, cfg)
    names = {id(p): n for n, p in m.named_parameters()}
    g0, g1 = ({names[id(p)] for p in g["params"]} for g in opt.param_groups)
    left = {names[id(p)] for p in opt.norm_only_params}
    dcn = [(n, mod) for n, mod in m.named_modules() if type(mod).__name__ == "DCN"]
    assert len(dcn) >= 6
    own = {n + "." + k for n, mod in dcn for k, _ in mod.named_parameters(recurse=False)}
    assert own and all(k.endswith((".weight", ".bias")) for k in own)
    assert left == own and not (own & (g0 | g1))
    assert all(n + ".conv_offset_mask.weight" in g0 and n + ".conv_offset_mask.bias" in g0 for n, _ in dcn)
    bn = {n + "." + k for n, mod in m.named_modules() if isinstance(mod, BN_TYPES) and not list(mod.children()) for k, _ in mod.named_parameters(recurse=False)}
    assert bn and g1 == bn
    assert g0 | g1 | left == {n for n, p in m.named_parameters() if p.requires_grad} and not (g0 & g1)
    assert len({(g["lr"], g["mom"], g["weight_decay"]) for g in opt.param_groups}) == 1 and opt.param_groups[0]["weight_decay"] == 0


def test_eager_trajectory_follows_the_reference(golden):
    """Eight steps of the wrapper's CPU form on the stored gradients against the stored parameters and moments (steps 1, 4 and 8).
    Measured: max |difference| / max |value| = 0.0 over every tensor and step (the same torch operations in the same order as the reference's
    wrapper).  Bound: 10 x measured with the floor 1e-7 -> 1e-7; the recorder asserted that dropping the decay (4.6e-5) or freezing mom (8.7e-5)
    moves the end point by more than 100 x 1e-7."""
    bound = 1e-7
    assert float(golden["teeth_wd0"]) > 100 * bound and float(golden["teeth_mom"]) > 100 * bound
    m, opt, sched = _built(golden)
    names = {id(p): n for n, p in m.named_parameters()}
    worst = 0.0
    for it in range(8):
        opt.zero_grad()
        set_grads(m, golden, it)
        opt.step()
        sched.step(it)
        if it + 1 in STEPS_KEPT:
            for n, p in m.named_parameters():
                worst = max(worst, rel(p, golden["p/%d/%s" % (it + 1, n)]))
            assert len(opt.state) == len(golden["held_0"]) + len(golden["held_1"])
            for p, st in opt.state.items():
                worst = max(worst, rel(st["exp_avg"], golden["m/%d/%s" % (it + 1, names[id(p)])]), rel(st["exp_avg_sq"], golden["v/%d/%s" % (it + 1, names[id(p)])]))
                assert float(st["step"]) == it + 1
    print("eager CPU form against the golden: max rel %.3e" % worst)
    assert worst <= bound, worst
    assert torch.equal(m.dcn.weight, torch.from_numpy(golden["init/dcn.weight"])) and torch.equal(m.frozen.value, torch.from_numpy(golden["init/frozen.value"]))
    assert m.dcn.weight.grad is not None                                     # it received a gradient; zero_grad clears it with the held ones
    opt.zero_grad()
    assert m.dcn.weight.grad is None and m.conv.weight.grad is None
    for got, want in zip(opt.state_dict()["param_groups"], golden["param_groups"]):
        assert got["params"] == want["params"] and got["weight_decay"] == want["weight_decay"] == 0 and got["eps"] == want["eps"]
        np.testing.assert_allclose([got["lr"], *got["betas"]], [want["lr"], *want["betas"]], rtol=1e-12)


def test_state_dict_loads_into_plain_adam_and_round_trips_through_the_checkpointer(golden, tmp_path):
    from monoflex_amd.utils.check_point import Checkpointer
    m, opt, sched = _built(golden)
    for it in range(3):
        opt.zero_grad()
        set_grads(m, golden, it)
        opt.step()
        sched.step(it)
    # a plain torch Adam with the golden's group layout takes the state
    m2 = golden_tree(golden)
    by_name = dict(m2.named_parameters())
    plain = torch.optim.Adam([{"params": [by_name[n] for n in golden[k]]} for k in ("held_0", "held_1")], lr=1e-3)
    plain.load_state_dict(copy.deepcopy(opt.state_dict()))
    for go, gp in zip(opt.param_groups, plain.param_groups):
        assert gp["lr"] == go["lr"] and tuple(gp["betas"]) == tuple(go["betas"])
        for x, y in zip(go["params"], gp["params"]):
            assert torch.equal(opt.state[x]["exp_avg"], plain.state[y]["exp_avg"]) and torch.equal(opt.state[x]["exp_avg_sq"], plain.state[y]["exp_avg_sq"])
    # through utils/check_point.py: plain numbers in the file, the same values (and objects) back
    lr, mom = opt.lr, opt.mom
    assert lr != SETTINGS["BASE_LR"] / SETTINGS["DIV_FACTOR"] and mom != SETTINGS["MOMS"][0]
    Checkpointer(m, opt, sched, save_dir=str(tmp_path)).save("ck", iteration=3)
    saved = torch.load(str(tmp_path / "ck.pth"), map_location="cpu")
    assert "scheduler" not in saved and len(saved["optimizer"]["param_groups"]) == 2
    for g in saved["optimizer"]["param_groups"]:
        assert type(g["lr"]) is float and type(g["mom"]) is float and g["lr"] == lr and g["mom"] == mom and tuple(g["betas"]) == (mom, 0.99)
    m3, opt3, sched3 = _built(golden)
    keep = [(g["lr"], g["mom"]) for g in opt3.param_groups]
    rest = Checkpointer(m3, opt3, sched3, save_dir=str(tmp_path)).load()
    assert rest == {"iteration": 3}
    assert (opt3.lr, opt3.mom) == (lr, mom) and all(tuple(g["betas"]) == (mom, 0.99) for g in opt3.param_groups)
    for g, (l0, m0) in zip(opt3.param_groups, keep):
        if torch.is_tensor(l0):
            assert g["lr"] is l0 and g["mom"] is m0
    for x, y in zip(opt.param_groups[0]["params"], opt3.param_groups[0]["params"]):
        assert torch.equal(opt.state[x]["exp_avg"], opt3.state[y]["exp_avg"]) and torch.equal(x, y)
