"""The reduced head sets through the model on the device: predictor, training step, captured step, checkpoint.

Sets s000 (no optional head, the depth branch first: 26 channels) and s011 (keypoints with their uncertainties, no depth uncertainty,
the uncertainties ahead of the keypoints: 49 channels) of tests/head_sets_ref.py.

* Predictor, B = 2 on a 24 x 80 map: the inference head map against the same layers in fp32 torch (F.conv2d, eval-mode BN, leaky ReLU,
  the edge fusion's Conv1d chain) with the bound of tests/test_gpu_ops.py test_heads_fused_vs_torch (1e-4 fp32, 5e-2 bf16, of the
  largest reference value); forward_train in its dense, sparse and Gram forms agrees with itself as
  tests/test_gpu_train_step.py test_gram_heads_step_equals_the_dense_heads_step requires of the full set (outputs tol, gradients
  norm-relative 10 tol in fp32 and 0.35 in bf16; tol = 2e-3 / 8e-2).
* One training step, B = 2 at 128 x 384: the loss dict has the reference's keys; with fixed-order reductions the GraphedTrainStep replay
  EQUALS the eager train_step -- the loss and every parameter, buffer and AdamW moment, as
  test_graphed_train_step_equals_the_eager_step_bitwise requires of the full set -- so the parameter checksums are equal.
* Checkpoint save -> load into a fresh model -> bit-identical decode.
"""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import head_sets_cases as HC
from tests import head_sets_ref as HS

pytestmark = pytest.mark.gpu
DEV = "cuda"
SETS = ["s000", "s011"]
MAP_W, MAP_H = 80, 24
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _predictor(name, seed=3):
    from monoflex_amd import synthetic as S
    from monoflex_amd.model.head.detector_predictor import _predictor as Predictor
    cfg = HC.model_cfg(name, extra=["INPUT.WIDTH_TRAIN", MAP_W * 4, "INPUT.HEIGHT_TRAIN", MAP_H * 4])
    m = Predictor(cfg, 64)
    m.load_state_dict(S.synthetic_state_dict(m.state_dict(), seed=seed, cls_bias=-1.0))
    return cfg, m


def _targets(B=2, seed0=40):
    from monoflex_amd import synthetic as S
    from monoflex_amd.structures.params_3d import make_train_target
    return [make_train_target(S.synthetic_train_target(seed0 + i, out_w=MAP_W, out_h=MAP_H, n_obj=4 + i)) for i in range(B)]


def _torch_heads(m, x, ei, el):
    """The predictor's eval forward in fp32 torch on the CPU: x (B, 64, H, W) -> class logits (B, ncls, H, W), regression (B, R, H, W)."""
    def trunk(seq):
        conv, abn = seq[0], seq[1]
        y = F.conv2d(x, conv.weight, None, padding=1)
        y = F.batch_norm(y, abn.running_mean, abn.running_var, abn.weight, abn.bias, False, 0.0, abn.eps)
        return F.leaky_relu(y, 0.01)
    f_cls = trunk(m.class_head)
    cls = F.conv2d(f_cls, m.class_head[2].weight, m.class_head[2].bias)
    regs, f_off = [], None
    for i, (feat, heads) in enumerate(zip(m.reg_features, m.reg_heads)):
        f = trunk(feat)
        if i == m.offset_index[0]:
            f_off = f
        regs.append(torch.cat([F.conv2d(f, h.weight, h.bias) for h in heads], dim=1))
    if m.enable_edge_fusion:                                            # detector_predictor.py:140-169 of the reference
        oi, oj = m.offset_index
        lo = sum(m.regression_channel_cfg[oi][:oj])
        for b in range(x.shape[0]):
            n = int(el[b])
            xs, ys = ei[b, :, 0].long(), ei[b, :, 1].long()
            for f, seq, base, c0 in ((f_cls, m.trunc_heatmap_conv, cls, 0), (f_off, m.trunc_offset_conv, regs[oi], lo)):
                o = seq.eval()(f[b][:, ys, xs].unsqueeze(0))[0]        # (cout, L): Conv1d k3 (replicate) -> BN1d -> [ReLU] -> Conv1d 1x1
                base[b, c0:c0 + o.shape[0], ys[:n], xs[:n]] += o[:, :n]
    return cls, torch.cat(regs, dim=1)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", SETS)
def test_inference_head_map_vs_torch(name, dtype):
    from monoflex_amd.model.head.detector_predictor import REG_OFF, stack_edge_fields
    cfg, m = _predictor(name)
    m.eval()
    tg = _targets()
    ei, el = stack_edge_fields(tg, "cpu")
    x = torch.randn(2, 64, MAP_H, MAP_W, generator=torch.Generator().manual_seed(9)).relu()
    if dtype == "bf16":
        x = x.bfloat16().float()
    with torch.no_grad():
        want_cls, want_reg = _torch_heads(m, x, ei, el)
    R = HS.WIDTHS[name]
    assert want_reg.shape[1] == R == m.reg_width
    m.to(DEV)
    hm = m.forward_nhwc(x.permute(0, 2, 3, 1).contiguous().to(DEV, DT[dtype]), ei.to(DEV), el.to(DEV)).float().cpu()
    tol = 1e-4 if dtype == "fp32" else 5e-2
    got_cls, got_reg = hm[..., :3].permute(0, 3, 1, 2), hm[..., REG_OFF:REG_OFF + R].permute(0, 3, 1, 2)
    e_cls = float((got_cls - want_cls).abs().max())                     # absolute, as test_heads_fused_vs_torch bounds the class logits
    e_reg = float((got_reg - want_reg).abs().max()) / max(1.0, float(want_reg.abs().max()))
    print("%s %s: head map error cls %.2e reg %.2e (bound %.0e)" % (name, dtype, e_cls, e_reg, tol))
    assert e_cls < tol and e_reg < tol
    out = m(x.to(DEV, DT[dtype]), tg)                                  # the reference surface: 'reg' is the R-channel view
    assert out['reg'].shape == (2, R, MAP_H, MAP_W) and torch.equal(out['reg'].float().cpu(), got_reg)


@pytest.fixture
def deterministic():
    from monoflex_amd import lib as L
    L.set_deterministic(True)
    yield
    L.set_deterministic(False)


def _train_forms(name, dtype):
    """forward_train of one predictor state in its three forms -> {form: (cls, table (n valid rows, R), gradients {param: tensor}, d features)}."""
    from monoflex_amd.model.head import detector_predictor as DP
    from monoflex_amd.model.head.detector_loss import Loss_Computation
    cfg, m0 = _predictor(name)
    tg = [t.to(DEV) for t in _targets()]
    ei, el = DP.stack_edge_fields(tg, DEV)
    rows = Loss_Computation(cfg).prepare_targets(tg, DEV)[1]["object_rows"]
    valid = torch.nonzero(rows[:, 0] != 0).flatten()
    B, R = 2, HS.WIDTHS[name]
    x0 = torch.randn(B, MAP_H, MAP_W, 64, generator=torch.Generator().manual_seed(11)).relu()
    g = torch.Generator().manual_seed(12)
    w_cls, w_tab = torch.randn(B, MAP_H, MAP_W, 3, generator=g).to(DEV), torch.randn(int(valid.numel()), R, generator=g).to(DEV)
    bidx, cx, cy = rows[:, 57].long(), rows[:, 2].long(), rows[:, 3].long()
    out = {}
    for form in ("dense", "sparse", "gram"):
        m = copy.deepcopy(m0).to(DEV).train()
        x = x0.to(DEV, DT[dtype]).requires_grad_()
        DP.GRAM_HEADS[0] = form == "gram"
        try:
            if form == "dense":
                cls, reg = m.forward_train(x, ei, el)
                assert reg.shape == (B, MAP_H, MAP_W, R)
                table = reg[bidx, cy, cx]
            else:
                cls, table = m.forward_train(x, ei, el, rows)
                assert table.shape == (rows.shape[0], R)
        finally:
            DP.GRAM_HEADS[0] = True
        table = table.float()[valid]
        ((cls.float() * w_cls).sum() + (table * w_tab).sum()).backward()
        torch.cuda.synchronize()
        out[form] = (cls.detach().float().cpu(), table.detach().cpu(), {n: p.grad.detach().float().cpu() for n, p in m.named_parameters() if p.grad is not None},
                     x.grad.detach().float().cpu())
    return out


@pytest.mark.parametrize("dtype,tol", [("fp32", 2e-3), ("bf16", 8e-2)])
@pytest.mark.parametrize("name", SETS)
def test_forward_train_forms_agree(name, dtype, tol, deterministic):
    out = _train_forms(name, dtype)
    cls_d, tab_d, g_d, dx_d = out["dense"]
    assert len(g_d) >= 4 * (1 + len(HS.SETS[name]))
    for form in ("sparse", "gram"):
        cls, tab, g, dx = out[form]
        assert set(g) == set(g_d)
        e_cls = float((cls - cls_d).abs().max()) / max(1.0, float(cls_d.abs().max()))
        e_tab = float((tab - tab_d).abs().max()) / max(1.0, float(tab_d.abs().max()))
        gmax = max(float(v.norm()) for v in g_d.values())
        floor = (1e-5 if dtype == "fp32" else 2e-3) * gmax
        worst = max((float((g[n] - g_d[n]).norm()) / max(float(g_d[n].norm()), floor), n) for n in g_d)
        e_dx = float((dx - dx_d).norm()) / float(dx_d.norm())
        print("%s %s %s vs dense: cls %.2e table %.2e worst parameter gradient %.2e (%s) d features %.2e" % (name, dtype, form, e_cls, e_tab, worst[0], worst[1], e_dx))
        assert e_cls <= tol and e_tab <= tol
        assert worst[0] < (10 * tol if dtype == "fp32" else 0.35), worst
        assert e_dx < (10 * tol if dtype == "fp32" else 0.35)


@pytest.mark.parametrize("name", SETS)
def test_gram_hip_node_runs_a_reduced_set(name):
    """Without fixed-order reductions the 16-bit Gram form is the HIP node (csrc/gram_heads.hip), what a training run uses: its table and
    gradients against the dense form, bf16 bounds as above."""
    out = _train_forms(name, "bf16")
    (cls_d, tab_d, g_d, dx_d), (cls, tab, g, dx) = out["dense"], out["gram"]
    assert float((tab - tab_d).abs().max()) <= 8e-2 * max(1.0, float(tab_d.abs().max()))
    gmax = max(float(v.norm()) for v in g_d.values())
    worst = max((float((g[n] - g_d[n]).norm()) / max(float(g_d[n].norm()), 2e-3 * gmax), n) for n in g_d)
    assert worst[0] < 0.35, worst


# ---- the whole model -----------------------------------------------------------------------------------------------------------------------
OUT_W, OUT_H = 96, 32                                                   # a 128 x 384 input


def _cfg(name, dtype):
    cfg = HC.model_cfg(name, extra=["INPUT.WIDTH_TRAIN", OUT_W * 4, "INPUT.HEIGHT_TRAIN", OUT_H * 4])
    cfg.MODEL.PRETRAIN = False
    cfg.MODEL.COMPUTE_DTYPE = dtype
    return cfg


def _model(name, dtype, seed=3):
    from monoflex_amd import synthetic as S
    from monoflex_amd.model.detector import KeypointDetector
    m = KeypointDetector(_cfg(name, dtype))
    m.load_state_dict(S.synthetic_state_dict(m.state_dict(), seed=seed, cls_bias=-1.0))
    m = m.to(DEV).train()
    m.heads.loss_evaluator.log_as_float = False
    return m


def _batch(m, B=2, seed0=20):
    from monoflex_amd import synthetic as S
    from monoflex_amd.engine.trainer import prepare_targets
    from monoflex_amd.structures.params_3d import make_train_target
    tg = [make_train_target(S.synthetic_train_target(seed0 + i, out_w=OUT_W, out_h=OUT_H, n_obj=3 + i)).to(DEV) for i in range(B)]
    imgs = S.synthetic_images(B, OUT_H * 4, OUT_W * 4, seed=seed0).to(DEV)
    return imgs, tg, prepare_targets(m, tg, DEV)


def _checksum(m):
    return sum(float(p.detach().double().sum()) for p in m.parameters())


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", SETS)
def test_training_step_graphed_equals_eager(name, dtype, deterministic):
    from monoflex_amd.engine.trainer import GraphedTrainStep, train_step
    from monoflex_amd.solver import build_optimizer
    cfg = _cfg(name, dtype)
    b = _model(name, dtype)
    imgs, _, tg = _batch(b)
    names, _ = HS.loss_names(name)
    opt_b = build_optimizer(b, cfg, capturable=True)
    step = GraphedTrainStep(b, opt_b, imgs, tg, warmup=2)
    torch.cuda.synchronize()
    model_sd = {k: v.detach().clone() for k, v in b.state_dict().items()}
    opt_sd = copy.deepcopy(opt_b.state_dict())
    a = _model(name, dtype, seed=5)
    a.load_state_dict(model_sd)
    opt_a = build_optimizer(a, cfg, capturable=True)
    opt_a.load_state_dict(opt_sd)
    before = _checksum(b)
    loss_b = step().clone()
    loss_a, loss_dict, logs = train_step(a, opt_a, imgs, tg)
    torch.cuda.synchronize()
    assert set(loss_dict) == HS.expected_loss_keys(name, names) and set(logs) == HS.expected_log_keys(name, names)      # the reference's dict keys
    assert all(bool(torch.isfinite(v)) for v in loss_dict.values())
    assert abs(float(sum(v.detach() for v in loss_dict.values())) - float(loss_a)) <= 1e-5 * abs(float(loss_a))                             # the total is the sum of the named terms
    assert bool(torch.isfinite(loss_a)) and torch.equal(loss_a, loss_b), (float(loss_a), float(loss_b))
    sa, sb = a.state_dict(), b.state_dict()
    diff = [k for k in sa if not torch.equal(sa[k], sb[k])]
    assert not diff, diff[:8]
    assert _checksum(a) == _checksum(b) != before                       # AdamW moved the parameters, to the same place
    moved = [n for n, p in b.named_parameters() if n.startswith("heads.predictor.reg_heads") and not torch.equal(p, model_sd[n])]
    assert len(moved) == 2 * sum(len(g) for g in HS.SETS[name])         # every configured regression head trains (weight and bias)


@pytest.mark.parametrize("name", SETS)
def test_checkpoint_round_trip_gives_the_same_detections(name, tmp_path):
    from monoflex_amd.model.detector import KeypointDetector
    from monoflex_amd.utils.check_point import DetectronCheckpointer
    m = _model(name, "fp32").eval()
    imgs, tg, _ = _batch(m)
    want = m(imgs, tg)
    DetectronCheckpointer(m.cfg if hasattr(m, "cfg") else _cfg(name, "fp32"), m, save_dir=str(tmp_path)).save("head_set")
    other = KeypointDetector(_cfg(name, "fp32")).to(DEV).eval()
    DetectronCheckpointer(_cfg(name, "fp32"), other, save_dir=str(tmp_path)).load(os.path.join(str(tmp_path), "head_set.pth"), use_latest=False)
    got = other(imgs, tg)
    torch.cuda.synchronize()
    rows_w, rows_g = want[0], got[0]
    rows_w, rows_g = (rows_w if isinstance(rows_w, (list, tuple)) else [rows_w]), (rows_g if isinstance(rows_g, (list, tuple)) else [rows_g])
    assert len(rows_w) == len(rows_g) and all(torch.equal(x, y) for x, y in zip(rows_w, rows_g))
    assert torch.equal(want[1]['det_all'], got[1]['det_all']) and bool(torch.isfinite(want[1]['det_all']).all())
    report = HS.has_depth_error(name, "soft" if HS.flags(name)[2] else "direct")
    assert (want[1]['estimated_depth_error'] is not None) == report == (want[1]['uncertainty_conf'] is not None)
