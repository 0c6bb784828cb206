"""MODEL.INPLACE_ABN False (conv3x3 -> BatchNorm2d -> ReLU head trunks) on the device, against tests/head_act_ref.py (the float64 statement
that tests/test_head_act_cpu.py pins to the reference's own results, tests/golden/head_act.npz).

Inputs: the seeded state / feature map / edge sequences of tests/head_act_ref.py (B = 2, 24 x 40) -- a state on which the ReLU and the leaky
form differ by more than ten times any bound below, and a quarter of the trunk channels are dead (test_head_act_cpu.py checks both).

Bounds, all taken from the tests of the ABN form:
  eval        tests/test_gpu_ops.py test_heads_fused_vs_torch: 1e-4 (fp32), 5e-2 (bf16), absolute on the class logits and of max(1, largest
              reference value) on the regression maps; split precision (fp16x2) the fp32 bound, as tests/test_gpu_split_precision.py; fp16 has
              three more mantissa bits than bf16 (unit roundoff 2^-11 against 2^-8): 5e-2 / 8
  32x32 form  test_heads_fused_mfma_32x32x16_form_equals_the_16x16x32_form: 2e-2 (bf16) of max(1, largest value), 2e-4 on average
  training    tests/test_gpu_head_sets_model.py test_forward_train_forms_agree: outputs 2e-3 (fp32) / 8e-2 (bf16), gradients norm-relative
              10 x that in fp32 and 0.35 in bf16 (floor 1e-5 / 2e-3 of the largest gradient norm)
  step        test_training_step_graphed_equals_eager: the replayed step EQUALS the eager one under fixed-order reductions
  two ranks   tests/test_gpu_train_step.py test_sync_bn_two_ranks_equal_one_process_on_the_whole_batch: 2e-5 / 1e-4 of max(1, largest value)
"""
import copy
import ctypes
import os
import socket

import numpy as np
import pytest
import torch

from tests import head_act_ref as HA

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16, "fp16x2": torch.float32}
EVAL_TOL = {"fp32": 1e-4, "bf16": 5e-2, "fp16": 5e-2 / 8, "fp16x2": 1e-4}


def _predictor(inplace_abn=False, extra=()):
    from monoflex_amd.model.head.detector_predictor import _predictor as Predictor
    cfg = HA.make_cfg(inplace_abn=inplace_abn, extra=extra)
    m = Predictor(cfg, 64)
    m.load_state_dict(HA.synthetic_state(m.state_dict()))
    return cfg, m


def _round(x, dtype):
    return x.to(DT[dtype]).float()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "head_act.npz"))


@pytest.fixture(scope="module")
def eval_refs():
    """The statement's eval maps per input rounding (fp32 / bf16 / fp16), computed once and left unchanged."""
    cfg, m = _predictor()
    _, ei, el = HA.edge_targets()
    out = {}
    for key in ("fp32", "bf16", "fp16"):
        with torch.no_grad():
            out[key] = HA.HeadActRef(m.state_dict(), cfg).forward(_round(HA.features(), key), ei, el, train=False)
    return out


@pytest.fixture
def deterministic():
    from monoflex_amd import lib as L
    L.set_deterministic(True)
    yield
    L.set_deterministic(False)


def _written(pk):
    w = torch.zeros(pk.ld_out, dtype=torch.bool)
    for o, c in zip(pk.ch_off, pk.c_out):
        w[o:o + c] = True
    return w.to(DEV)


# ---- 1. eval against the statement (and, in fp32, the reference's own maps) -----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16", "fp16x2"])
def test_eval_head_map_vs_reference(dtype, eval_refs, gold):
    from monoflex_amd import lib as L, ops
    from monoflex_amd.model.head.detector_predictor import REG_OFF
    cfg, m = _predictor()
    m.eval().to(DEV)
    if dtype == "fp16x2":
        for mod in m.modules():
            mod.__dict__["_mfx_split"] = True
    _, ei, el = HA.edge_targets()
    want_cls, want_reg = eval_refs["fp32" if dtype == "fp16x2" else dtype]
    x = _round(HA.features(), dtype).permute(0, 2, 3, 1).contiguous().to(DEV, DT[dtype])
    c0 = L.load().mfx_get_counter(b"edge_chain")
    hm = m.forward_nhwc(x, ei.to(DEV, torch.int32), el.to(DEV, torch.int32)).float().cpu()
    assert L.load().mfx_get_counter(b"edge_chain") == c0 + (1 if dtype in ("bf16", "fp16") else 0)     # 16-bit: the one-kernel edge chain
    pk = m._pack(ops.compute_tag(m, x.dtype))
    assert pk.act == L.ACT_RELU and pk.edge_trunk.act == L.ACT_RELU and pk.split == (dtype == "fp16x2")
    assert torch.equal(m.last_cls_planar.cpu().view(HA.B, 3, HA.H, HA.W), hm[..., :3].permute(0, 3, 1, 2))
    got_cls, got_reg = hm[..., :3].permute(0, 3, 1, 2).double(), hm[..., REG_OFF:REG_OFF + 50].permute(0, 3, 1, 2).double()
    tol = EVAL_TOL[dtype]
    e_cls = float((got_cls - want_cls).abs().max())
    e_reg = float((got_reg - want_reg).abs().max()) / max(1.0, float(want_reg.abs().max()))
    print("%s: class logits %.3e regression %.3e (bound %.2e)" % (dtype, e_cls, e_reg, tol))
    assert e_cls < tol and e_reg < tol
    if dtype == "fp32":                                                  # the reference's own output
        g_cls, g_reg = torch.from_numpy(gold["eval_cls"]).double(), torch.from_numpy(gold["eval_reg"]).double()
        assert float((HA.HeadActRef.sigmoid_hm(got_cls) - g_cls).abs().max()) < tol
        assert float((got_reg - g_reg).abs().max()) < tol * max(1.0, float(g_reg.abs().max()))
        out = m(HA.features().to(DEV), [_Target(ei[b], el[b]) for b in range(HA.B)])        # the reference surface
        assert float((out["cls"].double().cpu() - g_cls).abs().max()) < tol and torch.equal(out["reg"].cpu().double(), got_reg)


class _Target:
    def __init__(self, ei, el):
        self.f = {"edge_indices": ei, "edge_len": el}

    def get_field(self, k):
        return self.f[k]


# ---- 2. kernel variants of the ReLU form on a ragged map ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_relu_kernel_variants_on_a_ragged_map(dtype):
    from monoflex_amd import lib as L, ops
    lib_ = L.load()
    cfg, m = _predictor()
    m.eval().to(DEV)
    pk = m._pack(DT[dtype])
    assert pk.act == L.ACT_RELU and (pk.w1_32 is not None) == (dtype != "fp32")
    written = _written(pk)
    x0 = _round(HA.features(3, 21, 37, seed=4), dtype)                    # partial tiles: 3 x 3 tiles per image, 243 units
    x = x0.permute(0, 2, 3, 1).contiguous().to(DEV, DT[dtype])
    outs = {}
    for persist in (0, 7):
        for m32 in ((0, 1) if dtype != "fp32" else (0,)):
            for planes in ((0, 1) if dtype != "fp16" else (0,)):
                L.set_options({"heads_persist": persist, "heads_mfma32": m32, "heads_planes": planes})
                hm, planar = ops.heads_fused(x, pk, planar_classes=3)
                torch.cuda.synchronize()
                outs[(persist, m32, planes)] = (hm[..., written].float().cpu(), planar.float().cpu())
    lib_.mfx_reset_options()
    ref = outs[(0, 0, 0)]
    scale = float(ref[0].abs().max())
    for (persist, m32, planes), (hm, planar) in outs.items():
        assert bool(torch.isfinite(hm).all())
        assert torch.equal(hm, outs[(0, m32, planes)][0]) and torch.equal(planar, outs[(0, m32, planes)][1]), (persist, m32, planes)     # persistent == per tile
        if m32 == 0 or planes == 1:                                       # (the planes layout applies to the 16x16x32 form: heads_mfma32 is not taken then)
            assert torch.equal(hm, ref[0]) and torch.equal(planar, ref[1]), (persist, m32, planes)
        else:
            bound = (2e-2 if dtype == "bf16" else 3e-3) * max(1.0, scale)
            assert float((hm - ref[0]).abs().max()) <= bound and float((planar - ref[1]).abs().max()) <= bound, (persist, m32, planes)
            assert float((hm - ref[0]).abs().mean()) <= 2e-4 * max(1.0, scale)
    # ... and it is the ReLU form: the statement without edge fusion on the same map
    st = HA.HeadActRef(m.state_dict(), cfg)
    st.edge_fusion = False
    with torch.no_grad():
        w_cls, w_reg = st.forward(x0, train=False)
    want = torch.cat((w_cls, w_reg), 1).permute(0, 2, 3, 1)
    got = torch.cat((ref[0][..., :3], ref[0][..., 3:]), -1).double()
    tol = EVAL_TOL[dtype]
    assert float((got[..., :3] - want[..., :3]).abs().max()) < tol
    assert float((got[..., 3:] - want[..., 3:]).abs().max()) < tol * max(1.0, float(want[..., 3:].abs().max()))


# ---- 3. edge fusion: one kernel == five launches ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_edge_chain_kernel_equals_the_five_launches_with_a_relu_trunk(dtype, relu):
    from monoflex_amd import lib as L, ops
    lib_ = L.load()
    cfg, m = _predictor(extra=["MODEL.HEAD.EDGE_FUSION_RELU", relu])
    m.eval().to(DEV)
    assert isinstance(m.trunc_heatmap_conv[2], torch.nn.ReLU) == relu
    _, ei, el = HA.edge_targets()
    ei32, el32 = ei.to(DEV, torch.int32), el.to(DEV, torch.int32)
    x = HA.features().permute(0, 2, 3, 1).contiguous().to(DEV, DT[dtype])
    pk = m._pack(DT[dtype])
    assert pk.edge_chain is not None and pk.edge_chain.act_trunk == L.ACT_RELU and pk.edge_chain.relu == relu
    c0 = lib_.mfx_get_counter(b"edge_chain")
    hm = m.forward_nhwc(x, ei32, el32).clone()
    planar = m.last_cls_planar.clone()
    assert lib_.mfx_get_counter(b"edge_chain") == c0 + 1
    L.set_options({"edge_chain": 0})
    hm0 = m.forward_nhwc(x, ei32, el32).clone()
    planar0 = m.last_cls_planar.clone()
    assert lib_.mfx_get_counter(b"edge_chain") == c0 + 1                  # not at all with the switch off
    lib_.mfx_reset_options()
    w = _written(pk)
    assert torch.equal(hm[..., w], hm0[..., w]) and torch.equal(planar, planar0)
    # the fusion did something
    plain, _ = ops.heads_fused(x, pk, planar_classes=3)
    assert float((hm[..., :3] - plain[..., :3]).abs().max()) > 1e-3


# ---- 4. training forms ----------------------------------------------------------------------------------------------------------------------
N_PER_IMAGE = 40                                                         # MAX_OBJECTS: the table has 2 x MAX_OBJECTS rows


def _train_reference(dtype):
    """The statement's training step on the rounded input under the loss sum(cls * w_cls) + sum(table[valid] * w_tab)."""
    cfg, m = _predictor()
    _, ei, el = HA.edge_targets()
    rows = HA.object_rows(ei, el, N_PER_IMAGE)
    valid = torch.nonzero(rows[:, 0] != 0).flatten()
    g = torch.Generator().manual_seed(12)
    w_cls, w_tab = torch.randn(HA.B, HA.H, HA.W, 3, generator=g), torch.randn(int(valid.numel()), 50, generator=g)
    st = HA.HeadActRef(m.state_dict(), cfg, requires_grad=True)
    x = _round(HA.features(), dtype).double().requires_grad_()
    cls, reg = st.forward(x, ei, el, train=True)
    bidx, cx, cy = rows[:, 57].long(), rows[:, 2].long(), rows[:, 3].long()
    table = reg.permute(0, 2, 3, 1)[bidx, cy, cx][valid]
    cls = cls.permute(0, 2, 3, 1)
    ((cls * w_cls).sum() + (table * w_tab).sum()).backward()
    return dict(cls=cls.detach(), table=table.detach(), grads=st.grads(), dx=x.grad.permute(0, 2, 3, 1), running=st.running,
                rows=rows, valid=valid, w_cls=w_cls, w_tab=w_tab, ei=ei, el=el)


@pytest.fixture(scope="module")
def train_refs():
    return {dtype: _train_reference(dtype) for dtype in ("fp32", "bf16")}


def _train_forms(dtype, ref, forms=("dense", "sparse", "gram"), mark_sync=False):
    from monoflex_amd.model.head import detector_predictor as DP
    _, m0 = _predictor()
    if mark_sync:
        for t in [m0.class_head[1]] + [f[1] for f in m0.reg_features]:
            t.sync_bn = True
    ei, el, rows = ref["ei"].to(DEV, torch.int32), ref["el"].to(DEV, torch.int32), ref["rows"].to(DEV)
    valid, w_cls, w_tab = ref["valid"].to(DEV), ref["w_cls"].to(DEV), ref["w_tab"].to(DEV)
    bidx, cx, cy = rows[:, 57].long(), rows[:, 2].long(), rows[:, 3].long()
    out = {}
    for form in forms:
        m = copy.deepcopy(m0).to(DEV).train()
        x = HA.features().permute(0, 2, 3, 1).contiguous().to(DEV, DT[dtype]).requires_grad_()
        DP.GRAM_HEADS[0] = form == "gram"
        try:
            if form == "dense":
                cls, reg = m.forward_train(x, ei, el)
                table = reg[bidx, cy, cx]
            else:
                cls, table = m.forward_train(x, ei, el, rows)
                assert table.shape == (rows.shape[0], 50)
                assert form == "sparse" or float(table.detach()[rows[:, 0] == 0].abs().max()) == 0.0      # (the sparse form's 3d_offset columns come from the dense map)
        finally:
            DP.GRAM_HEADS[0] = True
        table = table.float()[valid]
        ((cls.float() * w_cls).sum() + (table * w_tab).sum()).backward()
        torch.cuda.synchronize()
        out[form] = dict(cls=cls.detach().double().cpu(), table=table.detach().double().cpu(), dx=x.grad.detach().double().cpu(),
                         grads={n: p.grad.detach().double().cpu() for n, p in m.named_parameters() if p.grad is not None},
                         state={k: v.detach().clone().cpu() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k})
    return out


def _check_against(got, want, dtype, tol, what):
    e_cls = float((got["cls"] - want["cls"]).abs().max()) / max(1.0, float(want["cls"].abs().max()))
    e_tab = float((got["table"] - want["table"]).abs().max()) / max(1.0, float(want["table"].abs().max()))
    gw = want["grads"]
    assert set(got["grads"]) == set(gw) and len(gw) == 59, set(got["grads"]) ^ set(gw)
    gmax = max(float(v.norm()) for v in gw.values())
    floor = (1e-5 if dtype == "fp32" else 2e-3) * gmax
    worst = max((float((got["grads"][n] - gw[n]).norm()) / max(float(gw[n].norm()), floor), n) for n in gw)
    e_dx = float((got["dx"] - want["dx"]).norm()) / float(want["dx"].norm())
    print("%s %s: cls %.2e table %.2e worst parameter gradient %.2e (%s) d features %.2e" % (what, dtype, e_cls, e_tab, worst[0], worst[1], e_dx))
    assert e_cls <= tol and e_tab <= tol
    assert worst[0] < (10 * tol if dtype == "fp32" else 0.35), worst
    assert e_dx < (10 * tol if dtype == "fp32" else 0.35)


@pytest.mark.parametrize("dtype,tol", [("fp32", 2e-3), ("bf16", 8e-2)])
def test_forward_train_forms_agree_with_each_other_and_the_reference(dtype, tol, deterministic, train_refs, gold):
    ref = train_refs[dtype]
    assert ref["rows"].shape[0] == 2 * N_PER_IMAGE and int((ref["rows"][:, 0] == 0).sum()) > 20
    out = _train_forms(dtype, ref)
    for form in ("dense", "sparse", "gram"):
        _check_against(out[form], ref, dtype, tol, form + " vs reference")
        if form != "dense":
            _check_against(out[form], out["dense"], dtype, tol, form + " vs dense")
        st = out[form]["state"]
        for k, v in ref["running"].items():                              # every norm's running statistics after the step
            assert float((st[k].double() - v).abs().max()) <= (1e-4 if dtype == "fp32" else 1e-3) * max(1.0, float(v.abs().max())), (form, k)
        assert all(int(v) == 1 for k, v in st.items() if "num_batches" in k)
        if dtype == "fp32":                                              # ... and the reference's own, for the two trunks the golden holds
            for n in HA.STAT_TRUNKS:
                for s_ in ("running_mean", "running_var"):
                    want = torch.from_numpy(gold["train_%s.%s" % (n, s_)])
                    assert float((st["%s.%s" % (n, s_)] - want).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max())), (form, n, s_)


def test_gram_hip_node_serves_the_relu_trunks(train_refs):
    """Without fixed-order reductions the 16-bit Gram form is the HIP node (csrc/gram_heads.hip), what a training run uses."""
    from monoflex_amd import lib as L
    ref = train_refs["bf16"]
    c0 = L.load().mfx_get_counter(b"gram")
    out = _train_forms("bf16", ref, forms=("gram",))
    assert L.load().mfx_get_counter(b"gram") >= c0 + 8                   # the eight phases
    _check_against(out["gram"], ref, "bf16", 8e-2, "gram (HIP node) vs reference")


# ---- 5. the whole training step -------------------------------------------------------------------------------------------------------------
OUT_W, OUT_H = 96, 32


def _model_cfg(dtype, inplace_abn=False):
    cfg = HA.make_cfg(inplace_abn=inplace_abn, extra=["INPUT.WIDTH_TRAIN", OUT_W * 4, "INPUT.HEIGHT_TRAIN", OUT_H * 4])
    cfg.MODEL.COMPUTE_DTYPE = dtype
    return cfg


def _model(dtype, seed=3):
    from monoflex_amd import synthetic as S
    from monoflex_amd.model.detector import KeypointDetector
    m = KeypointDetector(_model_cfg(dtype))
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


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_captured_training_step_of_the_whole_detector(dtype, deterministic):
    from monoflex_amd.engine.trainer import GraphedTrainStep, train_step
    from monoflex_amd.solver import build_optimizer
    cfg = _model_cfg(dtype)
    b = _model(dtype)
    assert "heads.predictor.class_head.3.bias" in b.state_dict() and isinstance(b.heads.predictor.class_head[1], torch.nn.BatchNorm2d)
    imgs, tg = _batch(b)
    opt_b = build_optimizer(b, cfg, capturable=True)
    step = GraphedTrainStep(b, opt_b, imgs, tg, warmup=2)
    torch.cuda.synchronize()
    a = _model(dtype, seed=5)
    a.load_state_dict({k: v.detach().clone() for k, v in b.state_dict().items()})
    opt_a = build_optimizer(a, cfg, capturable=True)
    opt_a.load_state_dict(copy.deepcopy(opt_b.state_dict()))
    head0 = {n: p.detach().clone() for n, p in b.named_parameters() if n.startswith("heads.predictor.")}
    for it in range(2):
        loss_b = step().clone()
        loss_a, loss_dict, _ = train_step(a, opt_a, imgs, tg)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss_a)) and all(bool(torch.isfinite(v)) for v in loss_dict.values())
        assert torch.equal(loss_a, loss_b), (it, float(loss_a), float(loss_b))
    sa, sb = a.state_dict(), b.state_dict()
    diff = [k for k in sa if not torch.equal(sa[k], sb[k])]
    assert not diff, diff[:8]
    moved = [n for n, p in b.named_parameters() if n in head0 and not torch.equal(p, head0[n])]
    assert "heads.predictor.class_head.3.weight" in moved and "heads.predictor.reg_features.4.1.weight" in moved and len(moved) >= 50
    assert int(sb["heads.predictor.class_head.1.num_batches_tracked"]) >= 2


# ---- 6. the leaky form is what it was -------------------------------------------------------------------------------------------------------
def _heads_desc(x, p, out, planar):
    from monoflex_amd import lib as L, ops
    d = L.HeadsDesc()
    B, H, W, _ = x.shape
    d.planar, d.planar_c = planar.data_ptr(), planar.shape[1]
    d.x, d.w1, d.scale1, d.shift1 = x.data_ptr(), p.w1.data_ptr(), p.scale1.data_ptr(), p.shift1.data_ptr()
    d.w2, d.bias2, d.out = p.w2.data_ptr(), p.bias2.data_ptr(), out.data_ptr()
    d.w1_32 = p.w1_32.data_ptr() if p.w1_32 is not None else None
    d.w2_32 = p.w2_32.data_ptr() if p.w2_32 is not None else None
    d.B, d.H, d.W, d.nbranch, d.K_pad, d.ld_out = B, H, W, len(p.c_out), p.K_pad, p.ld_out
    d.dtype = ops._dt(x.dtype)
    for i, (o, c) in enumerate(zip(p.ch_off, p.c_out)):
        d.ch_off[i], d.c_out[i], d.w2_scale[i] = o, c, 1.0
    return d


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_leaky_entry_points_are_bit_identical_to_their_act_forms(dtype):
    from monoflex_amd import lib as L, ops
    lib_ = L.load()
    _, m = _predictor(inplace_abn=True)
    m.eval().to(DEV)
    pk = m._pack(DT[dtype])
    assert pk.act == L.ACT_LEAKY
    x = HA.features(3, 21, 37, seed=4).permute(0, 2, 3, 1).contiguous().to(DEV, DT[dtype])
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = []
    for call in ("old", "act"):
        out = torch.zeros((3, 21, 37, pk.ld_out), dtype=torch.float32, device=DEV)
        planar = torch.zeros((3, 3, 21 * 37), dtype=torch.float32, device=DEV)
        d = _heads_desc(x, pk, out, planar)
        if call == "old":
            L.check(lib_.mfx_heads_fused(ctypes.byref(d), st), "mfx_heads_fused")
        else:
            L.check(lib_.mfx_heads_fused_act(ctypes.byref(d), L.ACT_LEAKY, st), "mfx_heads_fused_act")
        torch.cuda.synchronize()
        res.append((out, planar))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and float(res[0][0].abs().max()) > 0.1
    out = torch.zeros_like(res[0][0]); planar = torch.zeros_like(res[0][1])
    L.check(lib_.mfx_heads_fused_act(ctypes.byref(_heads_desc(x, pk, out, planar)), L.ACT_RELU, st), "mfx_heads_fused_act")
    torch.cuda.synchronize()
    assert not torch.equal(out, res[0][0])                               # and the activation does travel
    if dtype == "fp32":
        return
    # mfx_edge_chain and its _act form
    _, ei, _ = HA.edge_targets(37, 21, ((37 * 4 - 4, 21 * 4 - 2),) * 3)
    ei32 = ei.to(DEV, torch.int32).contiguous()
    p = pk.edge_chain
    assert p is not None and p.act_trunk == L.ACT_LEAKY
    res = []
    for act in (None, L.ACT_LEAKY, L.ACT_RELU):
        d = L.EdgeChainDesc()
        d.x, d.edge_xy = x.data_ptr(), ei32.data_ptr()
        d.w_trunk, d.scale_trunk, d.shift_trunk = p.w_trunk.data_ptr(), p.scale_trunk.data_ptr(), p.shift_trunk.data_ptr()
        d.w_conv, d.scale_conv, d.shift_conv = p.w_conv.data_ptr(), p.scale_conv.data_ptr(), p.shift_conv.data_ptr()
        d.w_out, d.bias_out = p.w_out.data_ptr(), p.bias_out.data_ptr()
        d.B, d.H, d.W, d.C, d.L, d.head_conv, d.ksize, d.relu, d.dtype = 3, 21, 37, 64, ei32.shape[1], 256, 3, int(p.relu), ops._dt(x.dtype)
        o = torch.zeros((2, 3, ei32.shape[1], 4), dtype=torch.float32, device=DEV)
        d.out = o.data_ptr()
        if act is None:
            L.check(lib_.mfx_edge_chain(ctypes.byref(d), st), "mfx_edge_chain")
        else:
            L.check(lib_.mfx_edge_chain_act(ctypes.byref(d), act, st), "mfx_edge_chain_act")
        torch.cuda.synchronize()
        res.append(o)
    assert torch.equal(res[0], res[1]) and not torch.equal(res[0], res[2]) and float(res[0].abs().max()) > 1e-3


# ---- 7. SyncBN ------------------------------------------------------------------------------------------------------------------------------
def test_sync_flag_without_a_process_group_changes_nothing(deterministic, train_refs):
    ref = train_refs["bf16"]
    plain = _train_forms("bf16", ref)
    marked = _train_forms("bf16", ref, mark_sync=True)
    for form in plain:
        a, b = plain[form], marked[form]
        assert torch.equal(a["cls"], b["cls"]) and torch.equal(a["table"], b["table"]) and torch.equal(a["dx"], b["dx"]), form
        assert all(torch.equal(a["grads"][n], b["grads"][n]) for n in a["grads"]) and all(torch.equal(a["state"][k], b["state"][k]) for k in a["state"]), form


def test_synchronised_head_norms_do_not_take_the_rank_local_sparse_form(train_refs):
    """SparseRegHeadsFn's batch statistics are rank-local (mfx_bn_train_stats).  With a process group in force and the head norms marked,
    forward_train must not route them through it even where the Gram form is switched off: it takes the Gram form, whose node all-reduces
    its sums.  (One rank: the collectives are forced, as tests/test_gpu_train_step.py does for its captured-collective coverage.)"""
    import torch.distributed as dist
    from monoflex_amd import autograd as AG
    ref = train_refs["bf16"]
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)
    calls = []
    real = AG.SparseRegHeadsFn.apply
    AG._SYNC_BN_FORCE[0] = True
    AG.SparseRegHeadsFn.apply = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        out = _train_forms("bf16", ref, forms=("sparse",), mark_sync=True)       # GRAM_HEADS off
        assert not calls
        _check_against(out["sparse"], ref, "bf16", 8e-2, "synchronised norms, Gram form switched off")
        from monoflex_amd.model.head.detector_predictor import InPlaceABN
        h = InPlaceABN(256).to(DEV)
        h.sync_bn = True
        with pytest.raises(NotImplementedError, match="rank-local"):
            real(ref["rows"].to(DEV), (h,), (0,), 50, (False,), torch.zeros(2, 4, 4, 256, device=DEV), h.weight, h.bias,
                 torch.zeros(2, 256, device=DEV), torch.zeros(2, device=DEV))
    finally:
        AG.SparseRegHeadsFn.apply = real
        AG._SYNC_BN_FORCE[0] = False
        dist.destroy_process_group()


def _two_rank_worker(rank, world, port, out):
    import torch.distributed as dist
    torch.cuda.set_device(rank if world > 1 else 0)
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    from monoflex_amd import lib as L
    from monoflex_amd.engine.trainer import convert_sync_batchnorm
    L.set_deterministic(True)
    dev = "cuda:%d" % (rank if world > 1 else 0)
    _, m = _predictor()
    assert convert_sync_batchnorm(m) == 11
    m.to(dev).train()
    Bt = 4
    _, ei, el = HA.edge_targets(orig_sizes=HA.ORIG_SIZES * 2)
    rows = HA.object_rows(ei, el, 10, batch=Bt)
    x = HA.features(Bt).permute(0, 2, 3, 1).contiguous()
    g = torch.Generator().manual_seed(12)
    w_cls, w_tab = torch.randn(Bt, HA.H, HA.W, 3, generator=g), torch.randn(rows.shape[0], 50, generator=g)
    sl = slice(2 * rank, 2 * rank + 2) if world > 1 else slice(0, Bt)
    rsl = slice(20 * rank, 20 * rank + 20) if world > 1 else slice(0, 40)
    r = rows[rsl].clone()
    r[:, 57] -= sl.start
    xs = x[sl].to(dev).requires_grad_()
    cls, table = m.forward_train(xs, ei[sl].to(dev, torch.int32), el[sl].to(dev, torch.int32), r.to(dev))
    ((cls.float() * w_cls[sl].to(dev)).sum() + (table.float() * w_tab[rsl].to(dev)).sum()).backward()
    torch.cuda.synchronize()
    norms = [("class_head.1", m.class_head[1])] + [("reg_features.%d.1" % i, f[1]) for i, f in enumerate(m.reg_features)]
    res = {}
    for n, t in norms:
        res[n] = tuple(v.detach().float().cpu().numpy() for v in (t.running_mean, t.running_var, t.weight.grad, t.bias.grad))
    out.put((rank, res))
    dist.destroy_process_group()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_two_ranks_on_half_batches_give_the_whole_batch_head_statistics():
    """Data parallel with USE_SYNC_BN: the nine head norms are real BatchNorm2d modules now, so the conversion reaches them and they take
    global-batch statistics -- two ranks x B = 2 give the running statistics of one process on B = 4, and their rank-local dgamma / dbeta
    sum to the whole-batch ones."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    res = {}
    for world in (2, 1):
        s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
        q = ctx.Queue()
        ps = [ctx.Process(target=_two_rank_worker, args=(r, world, port, q)) for r in range(world)]
        [p.start() for p in ps]
        got = sorted((q.get(timeout=300) for _ in ps), key=lambda v: v[0])
        [p.join(timeout=60) for p in ps]
        assert all(p.exitcode == 0 for p in ps)
        res[world] = [g[1] for g in got]
    close = lambda u, v, tol=2e-5: float(np.abs(u - v).max()) <= tol * max(1.0, float(np.abs(v).max()))      # noqa: E731
    for n, (rm, rv, dg, db) in res[1][0].items():
        (rm0, rv0, dg0, db0), (rm1, rv1, dg1, db1) = res[2][0][n], res[2][1][n]
        assert close(rm0, rm) and close(rm1, rm) and close(rv0, rv) and close(rv1, rv), n
        assert close(dg0 + dg1, dg, 1e-4) and close(db0 + db1, db, 1e-4), n
