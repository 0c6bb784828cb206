"""The reference's other training recipes on the captured step: MODEL.HEAD.LOSS_TYPE smooth_l1 / log, SOLVER.OPTIMIZER adam and
SOLVER.GRAD_NORM_CLIP 10 together.  One step, B = 2 at 128 x 384 (as tests/test_gpu_head_sets_model.py): with fixed-order reductions the
GraphedTrainStep replay equals the eager train_step in the loss, every parameter, every buffer and both moments; and do_train takes the
captured step for `adam` exactly as for `adamw`."""
import copy
import logging
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
OUT_W, OUT_H = 96, 32                                                   # a 128 x 384 input
RECIPE = ["MODEL.HEAD.LOSS_TYPE", ["Penalty_Reduced_FocalLoss", "smooth_l1", "giou", "log"], "SOLVER.OPTIMIZER", "adam", "SOLVER.GRAD_NORM_CLIP", 10.0]


def _cfg(dtype, extra=()):
    from monoflex_amd.config import get_cfg
    cfg = get_cfg(os.path.join(ROOT, "runs", "monoflex.yaml"), RECIPE + ["INPUT.WIDTH_TRAIN", OUT_W * 4, "INPUT.HEIGHT_TRAIN", OUT_H * 4] + list(extra))
    cfg.MODEL.PRETRAIN = False
    cfg.MODEL.COMPUTE_DTYPE = dtype
    return cfg


def _model(dtype, seed=3):
    from monoflex_amd import synthetic as S
    from monoflex_amd.model.detector import KeypointDetector
    m = KeypointDetector(_cfg(dtype))
    m.load_state_dict(S.synthetic_state_dict(m.state_dict(), seed=seed, cls_bias=-1.0))
    m = m.to(DEV).train()
    m.heads.loss_evaluator.log_as_float = False
    return m


def _batch(m, B=2, seed0=20):
    from monoflex_amd import synthetic as S
    from monoflex_amd.engine.trainer import prepare_targets
    from monoflex_amd.structures.params_3d import make_train_target
    tg = [make_train_target(S.synthetic_train_target(seed0 + i, out_w=OUT_W, out_h=OUT_H, n_obj=3 + i)).to(DEV) for i in range(B)]
    return S.synthetic_images(B, OUT_H * 4, OUT_W * 4, seed=seed0).to(DEV), prepare_targets(m, tg, DEV)


@pytest.fixture
def deterministic():
    from monoflex_amd import lib as L
    L.set_deterministic(True)
    yield
    L.set_deterministic(False)


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_recipe_step_graphed_equals_eager(dtype, deterministic):
    """fp16 runs both sides under the loss scaler (unscale -> fused norm -> clipped Adam reading found_inf)."""
    from monoflex_amd import lib as L
    from monoflex_amd.engine.trainer import GraphedTrainStep, LossScaler, train_step
    from monoflex_amd.solver import MultiTensorAdam, build_optimizer, multi_tensor_driver
    cfg = _cfg(dtype)
    clip = cfg.SOLVER.GRAD_NORM_CLIP
    b = _model(dtype)
    ev = b.heads.loss_evaluator
    assert (ev.reg_loss, ev.depth_loss) == ("smooth_l1", "log") and ev.object_loss_kinds() == (1, 1)
    imgs, tg = _batch(b)
    opt_b = build_optimizer(b, cfg)
    assert type(opt_b) is torch.optim.Adam and all(g["capturable"] and torch.is_tensor(g["lr"]) for g in opt_b.param_groups)
    assert type(multi_tensor_driver(opt_b)) is MultiTensorAdam
    cnt = lambda: {k: L.load().mfx_get_counter(k.encode()) for k in ("adamw_multi", "optim_multi", "grad_norm_multi")}      # noqa: E731
    c0 = cnt()
    step = GraphedTrainStep(b, opt_b, imgs, tg, warmup=2, grad_norm_clip=clip)
    assert step.use_graphs and len(step.graphs) == 1
    torch.cuda.synchronize()
    c1 = cnt()
    assert c1["optim_multi"] > c0["optim_multi"] and c1["grad_norm_multi"] > c0["grad_norm_multi"] and c1["adamw_multi"] == c0["adamw_multi"]
    model_sd = {k: v.detach().clone() for k, v in b.state_dict().items()}
    opt_sd = copy.deepcopy(opt_b.state_dict())
    a = _model(dtype, seed=5)
    a.load_state_dict(model_sd)
    opt_a = build_optimizer(a, cfg)
    opt_a.load_state_dict(opt_sd)
    sc_a = LossScaler.for_model(a)
    assert (sc_a is not None) == (dtype == "fp16") == (step.scaler is not None)
    if sc_a is not None:
        sc_a.attach(opt_a).load_state_dict(step.scaler.state_dict())
    applied = 0
    for it in range(2):
        loss_b = step().clone()
        loss_a, loss_dict, _ = train_step(a, opt_a, imgs, tg, grad_norm_clip=clip, scaler=sc_a)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss_a)) and torch.equal(loss_a, loss_b), (it, float(loss_a), float(loss_b))
        if sc_a is not None:
            assert sc_a.state_dict() == step.scaler.state_dict() and torch.equal(sc_a.found_inf, step.scaler.found_inf)
        sa, sb = a.state_dict(), b.state_dict()                              # every parameter and every buffer
        diff = [k for k in sa if not torch.equal(sa[k], sb[k])]
        assert not diff, (it, diff[:8])
        n_state = 0
        for ga, gb in zip(opt_a.param_groups, opt_b.param_groups):
            for x, y in zip(ga["params"], gb["params"]):
                if x in opt_a.state:
                    n_state += 1
                    for key in ("exp_avg", "exp_avg_sq", "step"):
                        assert torch.equal(opt_a.state[x][key], opt_b.state[y][key]), (it, key)
        assert n_state > 200
        na, nb = opt_a._mfx_multi.grad_norm, opt_b._mfx_multi.grad_norm     # [total_norm, coef]; a skipped fp16 step has a non-finite norm and coef 1
        assert torch.equal(na.view(torch.int32), nb.view(torch.int32))
        skipped = sc_a is not None and float(sc_a.found_inf) != 0.0
        applied += not skipped
        assert float(nb[1]) == 1.0 if skipped else (0.0 < float(nb[0]) < float("inf") and 0.0 < float(nb[1]) <= 1.0), (it, nb)
    moved = [n for n, p in b.named_parameters() if not torch.equal(p, model_sd[n])]
    assert len(moved) > 200 or applied == 0
    assert applied > 0 or dtype == "fp16"


def test_do_train_captures_the_step_for_adam(tmp_path, caplog):
    """engine.trainer.do_train over DeviceLoader batches with the recipe: three iterations, "captured as hipGraphs" in the log."""
    from PIL import Image
    from monoflex_amd import synthetic as S
    from monoflex_amd.config import get_cfg
    from monoflex_amd.data import DeviceLoader, KITTIDataset
    from monoflex_amd.engine import trainer as TR
    from monoflex_amd.model.detector import KeypointDetector
    from monoflex_amd.solver import build_optimizer, build_scheduler
    for d in ("image_2", "label_2", "calib", "ImageSets"):
        (tmp_path / d).mkdir()
    P = np.asarray(S.KITTI_P2).reshape(-1)
    for i, (w, h) in enumerate([(1242, 375), (1224, 370), (1238, 374), (1242, 375)]):
        Image.fromarray(np.random.RandomState(i).randint(0, 256, (h, w, 3)).astype(np.uint8)).save(tmp_path / "image_2" / ("%06d.png" % i))
        (tmp_path / "label_2" / ("%06d.txt" % i)).write_text("".join(l + "\n" for l in S.synthetic_kitti_labels(60 + i, w, h, 5 + i)))
        (tmp_path / "calib" / ("%06d.txt" % i)).write_text("P2: " + " ".join("%.12e" % v for v in P) + "\nP3: " + " ".join("%.12e" % v for v in P) + "\n")
    (tmp_path / "ImageSets" / "train.txt").write_text("000000\n000001\n000002\n000003\n")
    cfg = get_cfg(os.path.join(ROOT, "runs", "monoflex.yaml"), RECIPE)
    cfg.MODEL.PRETRAIN = False
    cfg.MODEL.COMPUTE_DTYPE = "bf16"
    cfg.SOLVER.MAX_ITERATION, cfg.SOLVER.LR_WARMUP, cfg.SOLVER.WARMUP_STEPS, cfg.SOLVER.STEPS = 3, False, -1, [2]
    cfg.SOLVER.SAVE_CHECKPOINT_INTERVAL, cfg.SOLVER.EVAL_INTERVAL = 1000, 0
    ds = KITTIDataset(cfg, str(tmp_path), is_train=True, augment=False)
    batches = (list(DeviceLoader(ds, batch_size=2)) * 2)[:3]
    torch.manual_seed(0)
    model = KeypointDetector(cfg).cuda().train()
    opt = build_optimizer(model, cfg)
    sched, warm = build_scheduler(opt, total_iters_each_epoch=2, optim_cfg=cfg.SOLVER)
    w0 = model.backbone.base.level2.tree1.conv1.weight.detach().clone()
    args = {"iteration": 0}
    with caplog.at_level(logging.INFO, logger="monoflex.trainer"):
        loss = TR.do_train(cfg, False, model, batches, None, opt, sched, warm, None, "cuda", args)
    assert args["iteration"] == 3 and np.isfinite(loss)
    assert any("captured as hipGraphs" in r.getMessage() for r in caplog.records), [r.getMessage() for r in caplog.records]
    assert type(opt) is torch.optim.Adam and not torch.equal(w0, model.backbone.base.level2.tree1.conv1.weight)
    assert float(opt._mfx_multi.captured[0][5][0]) > 0                       # the captured launch's [total_norm, coef] pair was written
