"""The edge fusion's other settings on the device -- MODEL.HEAD.EDGE_FUSION_KERNEL_SIZE k in {1, 3, 5, 7}, EDGE_FUSION_NORM 'BN' or none (Conv1d with its
bias), EDGE_FUSION_RELU, both trunk forms -- against tests/edge_fusion_ref.py, the float64 statement that tests/test_edge_fusion_settings_cpu.py pins to
the reference's own results (tests/golden/edge_fusion_settings.npz).  k = 3 with the BatchNorm1d is runs/monoflex.yaml's setting and stays with
tests/test_gpu_edge_chain.py / tests/test_gpu_head_act.py; k = 3 WITHOUT the norm is new ground (the old entries, scale = 1) and is walked here.

Eval, 16-bit: the one kernel (csrc/edge_chain.hip, instantiated per window; mfx_edge_chain_ks) against
  * the five mfx_conv2d_nhwc launches (option edge_chain = 0), asserted BIT-IDENTICAL: both forms issue the same v_mfma_f32_16x16x32 per 32 elements of
    ascending K (K = 256 k: one workgroup sums all of it in both forms, the library's split-K is opt-in) and round at the same three places; without a
    norm both multiply by the same 1.0;
  * the float64 statement within tests/test_gpu_edge_chain.py's derived bound: 1.01 x (what rounding the two intermediates to the activation type can
    move an output by, edge_fusion_ref.edge_chain_ref's `bound`) + 1e-5 x the output's scale (fp32 accumulation and folding).
A workgroup writes SEG = 64 - (k - 1) positions and recomputes k // 2 halo rows on either side: sequence lengths around the halo and around one and two
segments are where clamped halos and ragged last segments go wrong.

fp32 and split precision keep the five launches (their only form); bound: tests/test_gpu_head_act.py's EVAL_TOL for the same maps.

Training (dense, sparse and Gram forms, fused_edge_nodes on and off) against float64 autograd of the statement; bounds: those of
tests/test_gpu_head_act.py (test_forward_train_forms_agree_with_each_other_and_the_reference) for the same quantities at k = 3 -- outputs 2e-3 (fp32) /
8e-2 (bf16) of max(1, largest value), gradients norm-relative 10 x that in fp32 and 0.35 in bf16 -- with the output bound and the fp32 gradient bound
multiplied by K / 768 = k / 3 where the Conv1d's K = 256 k exceeds k = 3's 768 (the sums they bound grow with the number of products; `_kf`)."""
import copy
import os

import numpy as np
import pytest
import torch

import edge_fusion_ref as EF
from tests import head_act_ref as HA

pytestmark = pytest.mark.gpu
DEV = "cuda"
D64 = torch.float64
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16, "fp16x2": torch.float32}
EVAL_TOL = {"fp32": 1e-4, "fp16x2": 1e-4}                       # tests/test_gpu_head_act.py EVAL_TOL
_cache = {}


def _seg(k):
    return 64 - (k - 1)


def _kf(k):
    """K of the Conv1d against k = 3's: 256 k / 768"""
    return max(1.0, k / 3.0)


def _lib():
    from monoflex_amd import lib as L, ops
    return ops, L, L.load()


def _model(k, norm, relu, abn):
    """(the predictor on the device in eval mode, a host copy for the statement's operands); one per setting, shared by every test"""
    key = ("model", k, norm, relu, abn)
    if key not in _cache:
        from monoflex_amd.model.head.detector_predictor import _predictor
        cfg = HA.make_cfg(inplace_abn=abn, extra=EF.setting_opts(k, norm, relu))
        m = _predictor(cfg, 64).eval()
        m.load_state_dict(HA.synthetic_state(m.state_dict(), seed=3))
        assert isinstance(m.trunc_heatmap_conv[2], torch.nn.ReLU) == bool(relu) and isinstance(m.trunc_offset_conv[1], torch.nn.BatchNorm1d) == (norm == "BN")
        _cache[key] = (copy.deepcopy(m).to(DEV), m, cfg)
    return _cache[key]


def _features(B, H, W, dtype, seed=9):
    x = torch.randn(B, 64, H, W, generator=torch.Generator().manual_seed(seed)).relu().to(dtype)
    return x.permute(0, 2, 3, 1).contiguous().to(DEV), x.to(D64)


def _edge_indices(H, W, B, full=False):
    """as tests/test_gpu_edge_chain.py: (B, L, 2) int64 border points; `full`: the padding rows replaced by distinct interior pixels"""
    from monoflex_amd import synthetic as S
    tgt = S.synthetic_target(W, H)
    ei, n = tgt["edge_indices"].clone(), tgt["edge_len"]
    if full:
        q = ei.shape[0] - n
        ei[n:, 0], ei[n:, 1] = torch.arange(5, 5 + q), H // 2
        assert len({(int(a), int(b)) for a, b in ei}) == ei.shape[0]
    return torch.stack([ei] * B), tgt["edge_len"]


def _five_launches(ops, m, p, feats, ei32):
    """The chain as forward_nhwc runs it with option edge_chain = 0 -> fp32 (2, B, L, 4)"""
    from monoflex_amd.model.head.detector_predictor import make_edge_rowmap
    B, H, W, _ = feats.shape
    Lm, h = ei32.shape[1], m.edge_halo
    trunk = ops.conv2d(feats, p.edge_trunk, rowmap=make_edge_rowmap(ei32, H, W, h)).view(B, 1, Lm + 2 * h, 512)
    outs = []
    for bi, (pk1, pk2, _, _) in enumerate(p.edge_branches):
        outs.append(ops.conv2d(ops.conv2d(trunk, pk1, x_ch_off=bi * 256), pk2, out_dtype=torch.float32).view(B, Lm, 4))
    return torch.stack(outs)


def _judge(got, x64, ei, mcpu, dtype, what):
    """got fp32 (2, B, L, 4) against the float64 statement within the rounding bound of the intermediates"""
    ref = EF.edge_chain_ref(x64, ei, EF.chain_operands(mcpu, dtype), U[dtype])
    for bi, (o, bound) in enumerate(ref):
        o, bound = o.permute(0, 2, 1), bound.permute(0, 2, 1)                      # (B, L, c)
        c = o.shape[-1]
        g = got[bi].to(D64).cpu()
        err = (g[..., :c] - o).abs()
        scale = max(1.0, float(o.abs().max()))
        tol = 1.01 * bound + 1e-5 * scale
        print("%s branch %d: max err %.3e mean err %.3e (max |ref| %.3f, largest bound %.3e, worst err / tol %.3f)"
              % (what, bi, float(err.max()), float(err.mean()), float(o.abs().max()), float(tol.max()), float((err / tol).max())))
        assert bool((err <= tol).all()), (what, bi, float((err / tol).max()))
        assert float(g[..., c:].abs().max()) == 0.0                               # the padded channels: zero weights, zero bias


def _written(t):
    from monoflex_amd.model.head.detector_predictor import REG_OFF
    return torch.cat((t[..., :3], t[..., REG_OFF:REG_OFF + 50]), -1)


OPERATOR_CASES = [(k, norm) for k in (1, 5, 7) for norm in ("BN", "none")] + [(3, "none")]


# ---- 1. the operator ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("k,norm", OPERATOR_CASES)
def test_operator_equals_the_five_launches_and_meets_the_statement(k, norm, dtype):
    """ReLU on and off; B = 1 with the InPlaceABN trunks, B = 3 with the BatchNorm2d + ReLU trunks; every image's sequence rolled differently."""
    ops, L, lib = _lib()
    for relu in (True, False):
        for (B, H, W), abn in (((1, 24, 40), True), ((3, 24, 40), False)):
            m, mcpu, _ = _model(k, norm, relu, abn)
            p = m._pack(dtype)
            c = p.edge_chain
            assert c is not None and c.ksize == k and c.relu == bool(relu) and c.act_trunk == (L.ACT_LEAKY if abn else L.ACT_RELU)
            assert (norm == "BN") != bool(torch.equal(c.scale_conv, torch.ones_like(c.scale_conv)))
            feats, x64 = _features(B, H, W, dtype)
            ei, _ = _edge_indices(H, W, B)
            for b in range(B):                                 # every image its own sequence: rolled, so that the replicate-padded ends differ too
                ei[b] = torch.roll(ei[b], 7 * b + 3, 0)
            ei32 = ei.to(DEV, torch.int32).contiguous()
            c0 = lib.mfx_get_counter(b"edge_chain")
            got = ops.edge_chain(feats, ei32, c)
            assert got is not None and got.shape == (2, B, ei.shape[1], 4) and lib.mfx_get_counter(b"edge_chain") == c0 + 1
            old = _five_launches(ops, m, p, feats, ei32)
            torch.cuda.synchronize()
            assert torch.equal(got, old), (relu, B, float((got - old).abs().max()))
            _judge(got, x64, ei, mcpu, dtype, "k=%d %s %s relu=%s B=%d" % (k, norm, dtype, relu, B))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("k", [1, 5, 7])
def test_sequence_lengths_around_the_halo_and_the_segment_length(k, dtype):
    """L = 1, 2, HALO, HALO + 1 (every halo row a clamped copy; L <= HALO: several taps on one position) and one below / at / one above one and two
    segments (a last segment of 1 .. SEG positions).  Pixels anywhere in the map, the corners among them (taps outside the image)."""
    ops, L, lib = _lib()
    halo, SEG = k // 2, _seg(k)
    H, W = 24, 40
    m, mcpu, _ = _model(k, "none" if k == 5 else "BN", True, k == 7)
    p = m._pack(dtype)
    feats, x64 = _features(2, H, W, dtype)
    g = torch.Generator().manual_seed(k)
    n = 2 * SEG + 1
    ei = torch.stack((torch.randint(0, W, (2, n), generator=g), torch.randint(0, H, (2, n), generator=g)), -1)
    ei[0, 0], ei[0, 1], ei[1, 0], ei[1, SEG - 1] = torch.tensor([0, 0]), torch.tensor([W - 1, H - 1]), torch.tensor([W - 1, 0]), torch.tensor([0, H - 1])
    for Lm in sorted({v for v in (1, 2, halo, halo + 1, SEG - 1, SEG, SEG + 1, 2 * SEG - 1, 2 * SEG, 2 * SEG + 1) if v >= 1}):
        e = ei[:, :Lm].contiguous()
        e32 = e.to(DEV, torch.int32).contiguous()
        got = ops.edge_chain(feats, e32, p.edge_chain)
        old = _five_launches(ops, m, p, feats, e32)
        torch.cuda.synchronize()
        assert got.shape == (2, 2, Lm, 4) and torch.equal(got, old), Lm
        _judge(got, x64, e, mcpu, dtype, "k=%d %s L=%d" % (k, dtype, Lm))


def test_ks_entry_launches_the_old_entries_kernel_at_k3():
    """mfx_edge_chain_ks with ksize = 3 against mfx_edge_chain_act: the same instantiation, the same bits; both move the one counter."""
    import ctypes
    ops, L, lib = _lib()
    m, _, _ = _model(3, "none", True, True)
    p = m._pack(torch.bfloat16).edge_chain
    feats, _ = _features(2, 24, 40, torch.bfloat16)
    ei, _ = _edge_indices(24, 40, 2)
    ei32 = ei.to(DEV, torch.int32).contiguous()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = []
    c0 = lib.mfx_get_counter(b"edge_chain")
    for fn in (lib.mfx_edge_chain_act, lib.mfx_edge_chain_ks):
        d = L.EdgeChainDesc()
        d.x, d.edge_xy = feats.data_ptr(), ei32.data_ptr()
        d.w_trunk, d.scale_trunk, d.shift_trunk = p.w_trunk.data_ptr(), p.scale_trunk.data_ptr(), p.shift_trunk.data_ptr()
        d.w_conv, d.scale_conv, d.shift_conv = p.w_conv.data_ptr(), p.scale_conv.data_ptr(), p.shift_conv.data_ptr()
        d.w_out, d.bias_out = p.w_out.data_ptr(), p.bias_out.data_ptr()
        d.B, d.H, d.W, d.C, d.L, d.head_conv, d.ksize, d.relu, d.dtype = 2, 24, 40, 64, ei32.shape[1], 256, 3, 1, ops._dt(feats.dtype)
        o = torch.zeros((2, 2, ei32.shape[1], 4), dtype=torch.float32, device=DEV)
        d.out = o.data_ptr()
        L.check(fn(ctypes.byref(d), p.act_trunk, st), "edge chain")
        torch.cuda.synchronize()
        res.append(o)
    assert torch.equal(res[0], res[1]) and float(res[0].abs().max()) > 1e-3 and lib.mfx_get_counter(b"edge_chain") == c0 + 2


# ---- 2. the whole predictor, eval -----------------------------------------------------------------------------------------------------------
FORWARD_SETTING = {1: ("BN", False), 3: ("none", True), 5: ("none", True), 7: ("BN", True)}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("k", [1, 3, 5, 7])
def test_forward_nhwc_equals_the_five_launch_form(k, dtype):
    """Images with different edge_len: 0, 1, L - 1, L (no padding rows) and one below / above the segment length.  The head map and the planar class copy
    are bit-identical to the five-launch form's, what the fusion added is the statement's output at the first edge_len points and nothing elsewhere, and
    the dispatch counter tells which form ran."""
    ops, L, lib = _lib()
    from monoflex_amd.model.head.detector_predictor import REG_OFF
    norm, relu = FORWARD_SETTING[k]
    m, mcpu, _ = _model(k, norm, relu, k in (1, 5))
    H, W, SEG = 24, 40, _seg(k)
    for lens in ([0, 1, 127], [128, SEG - 1, SEG + 1]):
        B = len(lens)
        feats, x64 = _features(B, H, W, dtype, seed=11)
        ei, _ = _edge_indices(H, W, B, full=True)
        assert ei.shape[1] == 128
        ei32, el = ei.to(DEV, torch.int32).contiguous(), torch.tensor(lens, dtype=torch.int32, device=DEV)
        c0 = lib.mfx_get_counter(b"edge_chain")
        hm = m.forward_nhwc(feats, ei32, el)
        planar = m.last_cls_planar
        assert lib.mfx_get_counter(b"edge_chain") == c0 + 1
        L.set_options({"edge_chain": 0})
        try:
            k0 = lib.mfx_get_counter(b"conv_igemm")
            hm0 = m.forward_nhwc(feats, ei32, el)
            planar0 = m.last_cls_planar
            assert lib.mfx_get_counter(b"edge_chain") == c0 + 1 and lib.mfx_get_counter(b"conv_igemm") == k0 + 5      # not at all with the switch off
        finally:
            L.set_options({"edge_chain": 1})
        base, _ = ops.heads_fused(feats, m._pack(dtype), planar_classes=3)
        torch.cuda.synchronize()
        assert torch.equal(_written(hm), _written(hm0)) and torch.equal(planar, planar0)
        assert torch.equal(planar.view(B, 3, H, W), hm[..., :3].permute(0, 3, 1, 2))
        ref = EF.edge_chain_ref(x64, ei, EF.chain_operands(mcpu, dtype), U[dtype])
        added = (hm.to(D64) - base.to(D64)).cpu()
        added[..., 3:REG_OFF], added[..., REG_OFF + 50:] = 0.0, 0.0                 # (channels nobody writes)
        hm_abs = hm.to(D64).abs().cpu()
        hm_abs[..., 3:REG_OFF], hm_abs[..., REG_OFF + 50:] = 0.0, 0.0
        p = m._pack(dtype)
        want, tol, touched = torch.zeros_like(added), torch.zeros_like(added), torch.zeros_like(added, dtype=torch.bool)
        for (o, bound), (_, _, cout, choff) in zip(ref, p.edge_branches):
            for b, n in enumerate(lens):
                xs, ys = ei[b, :n, 0], ei[b, :n, 1]
                want[b, ys, xs, choff:choff + cout] = o[b, :, :n].t()
                tol[b, ys, xs, choff:choff + cout] = 1.01 * bound[b, :, :n].t() + 1e-5 * max(1.0, float(o.abs().max()))
                touched[b, ys, xs, choff:choff + cout] = True
        tol = tol + 2.0 ** -22 * hm_abs.clamp(min=1.0)           # the fp32 add into the head map, and its difference taken here
        err = (added - want).abs()
        print("k=%d %s lens=%s: fusion max err %.3e, worst err / tol %.3f" % (k, dtype, lens, float(err.max()), float((err / tol).max())))
        assert bool((err <= tol).all())
        assert touched.sum() == 5 * sum(lens) and float(added[~touched].abs().max()) == 0.0      # pixels and channels the fusion does not touch


@pytest.mark.parametrize("dtype", ["fp32", "fp16x2"])
@pytest.mark.parametrize("k,norm,relu", [(5, "none", True), (7, "BN", False), (1, "none", False)])
def test_fp32_and_split_precision_keep_the_five_launches(k, norm, relu, dtype):
    ops, L, lib = _lib()
    from monoflex_amd.model.head.detector_predictor import REG_OFF
    m0, _, cfg = _model(k, norm, relu, False)
    m = copy.deepcopy(m0)
    if dtype == "fp16x2":
        for mod in m.modules():
            mod.__dict__["_mfx_split"] = True
    assert m._pack(ops.compute_tag(m, torch.float32)).edge_chain is None
    _, ei, el = HA.edge_targets()
    x0 = HA.features()
    with torch.no_grad():
        want_cls, want_reg = EF.EdgeFusionRef(m0.state_dict(), cfg).forward(x0, ei, el, train=False)
    x = x0.permute(0, 2, 3, 1).contiguous().to(DEV)
    c0, k0 = lib.mfx_get_counter(b"edge_chain"), lib.mfx_get_counter(b"conv_igemm")
    hm = m.forward_nhwc(x, ei.to(DEV, torch.int32), el.to(DEV, torch.int32)).float().cpu()
    assert lib.mfx_get_counter(b"edge_chain") == c0 and lib.mfx_get_counter(b"conv_igemm") == k0 + 5
    got_cls, got_reg = hm[..., :3].permute(0, 3, 1, 2).double(), hm[..., REG_OFF:REG_OFF + 50].permute(0, 3, 1, 2).double()
    tol = EVAL_TOL[dtype]
    e_cls = float((got_cls - want_cls).abs().max())
    e_reg = float((got_reg - want_reg).abs().max()) / max(1.0, float(want_reg.abs().max()))
    print("k=%d %s relu=%s %s: class logits %.3e regression %.3e (bound %.2e)" % (k, norm, relu, dtype, e_cls, e_reg, tol))
    assert e_cls < tol and e_reg < tol


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_two_graph_replays_give_equal_head_maps_at_k5(dtype):
    ops, L, lib = _lib()
    m, _, _ = _model(5, "none", True, True)
    feats, _ = _features(2, 24, 40, dtype, seed=5)
    ei, n = _edge_indices(24, 40, 2)
    ei32, el = ei.to(DEV, torch.int32).contiguous(), torch.tensor([n, n - 3], dtype=torch.int32, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eager = m.forward_nhwc(feats, ei32, el).clone()                             # (first launch outside the capture: kernel attributes are set here)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    c0 = lib.mfx_get_counter(b"edge_chain")
    with torch.cuda.graph(g):
        hm = m.forward_nhwc(feats, ei32, el)
    assert lib.mfx_get_counter(b"edge_chain") == c0 + 1
    g.replay()
    first = hm.clone()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(first, hm) and torch.equal(_written(first), _written(eager))


def test_detector_prepares_the_row_map_with_the_predictors_halo():
    """fp32 (five launches) through the whole detector at k = 5: device_targets' row map has L + 4 positions per image, and the head map equals the one
    computed from a row map made inside the step."""
    from monoflex_amd import synthetic as S
    from monoflex_amd.model.detector import KeypointDetector
    from monoflex_amd.structures.params_3d import make_test_target
    ow, oh = 48, 24
    cfg = HA.make_cfg(inplace_abn=True, extra=EF.setting_opts(5, "none", True) + ["INPUT.WIDTH_TRAIN", ow * 4, "INPUT.HEIGHT_TRAIN", oh * 4])
    cfg.DATASETS.TEST_SPLIT = "test"
    m = KeypointDetector(cfg).eval()
    m.load_state_dict(S.synthetic_state_dict(m.state_dict(), seed=0, cls_bias=-1.0))
    m.to(DEV)
    imgs = S.synthetic_images(2, oh * 4, ow * 4, seed=1000).to(DEV)
    tg = m.device_targets([make_test_target(S.synthetic_target(ow, oh))] * 2, DEV)
    ei, rowmap = tg[0], tg[5]
    assert rowmap.numel() == 2 * (ei.shape[1] + 4) and rowmap.tolist() == EF.rowmap_loop(ei.cpu(), oh, ow, 2)
    with torch.no_grad():
        hm = m.detect_device(imgs, *tg)[3].clone()
        hm0 = m.detect_device(imgs, *tg[:5])[3]
    torch.cuda.synchronize()
    assert torch.equal(_written(hm), _written(hm0)) and bool(torch.isfinite(_written(hm)).all())


# ---- 3. training forms ----------------------------------------------------------------------------------------------------------------------
N_PER_IMAGE = 40
TRAIN_SETTINGS = [(1, "BN", False), (5, "BN", False), (5, "none", True), (7, "none", False)]


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "edge_fusion_settings.npz"))


@pytest.fixture
def deterministic():
    from monoflex_amd import lib as L
    L.set_deterministic(True)
    yield
    L.set_deterministic(False)


def _train_predictor(k, norm, relu):
    from monoflex_amd.model.head.detector_predictor import _predictor as Predictor
    cfg = HA.make_cfg(inplace_abn=False, extra=EF.setting_opts(k, norm, relu))
    m = Predictor(cfg, 64)
    m.load_state_dict(HA.synthetic_state(m.state_dict()))
    return cfg, m


def _train_reference(setting, dtype):
    """The statement's training step on the rounded input under the loss sum(cls * w_cls) + sum(table[valid] * w_tab); computed once per (setting, type)"""
    key = ("train", setting, dtype)
    if key in _cache:
        return _cache[key]
    cfg, m = _train_predictor(*setting)
    _, ei, el = HA.edge_targets()
    rows = HA.object_rows(ei, el, N_PER_IMAGE)
    valid = torch.nonzero(rows[:, 0] != 0).flatten()
    g = torch.Generator().manual_seed(12)
    w_cls, w_tab = torch.randn(HA.B, HA.H, HA.W, 3, generator=g), torch.randn(int(valid.numel()), 50, generator=g)
    st = EF.EdgeFusionRef(m.state_dict(), cfg, requires_grad=True)
    x = HA.features().to(DT[dtype]).double().requires_grad_()
    cls, reg = st.forward(x, ei, el, train=True)
    bidx, cx, cy = rows[:, 57].long(), rows[:, 2].long(), rows[:, 3].long()
    table = reg.permute(0, 2, 3, 1)[bidx, cy, cx][valid]
    cls = cls.permute(0, 2, 3, 1)
    ((cls * w_cls).sum() + (table * w_tab).sum()).backward()
    _cache[key] = dict(cls=cls.detach(), table=table.detach(), grads=st.grads(), dx=x.grad.permute(0, 2, 3, 1), running=st.running,
                       rows=rows, valid=valid, w_cls=w_cls, w_tab=w_tab, ei=ei, el=el)
    return _cache[key]


def _train_forms(setting, dtype, ref, fused):
    from monoflex_amd.model.head import detector_predictor as DP
    _, m0 = _train_predictor(*setting)
    ei, el, rows = ref["ei"].to(DEV, torch.int32), ref["el"].to(DEV, torch.int32), ref["rows"].to(DEV)
    valid, w_cls, w_tab = ref["valid"].to(DEV), ref["w_cls"].to(DEV), ref["w_tab"].to(DEV)
    bidx, cx, cy = rows[:, 57].long(), rows[:, 2].long(), rows[:, 3].long()
    out = {}
    for form in ("dense", "sparse", "gram"):
        m = copy.deepcopy(m0).to(DEV).train()
        m.fused_edge_nodes = fused
        x = HA.features().permute(0, 2, 3, 1).contiguous().to(DEV, DT[dtype]).requires_grad_()
        DP.GRAM_HEADS[0] = form == "gram"
        try:
            if form == "dense":
                cls, reg = m.forward_train(x, ei, el)
                table = reg[bidx, cy, cx]
            else:
                cls, table = m.forward_train(x, ei, el, rows)
                assert table.shape == (rows.shape[0], 50)
        finally:
            DP.GRAM_HEADS[0] = True
        table = table.float()[valid]
        ((cls.float() * w_cls).sum() + (table * w_tab).sum()).backward()
        torch.cuda.synchronize()
        out[form] = dict(cls=cls.detach().double().cpu(), table=table.detach().double().cpu(), dx=x.grad.detach().double().cpu(),
                         grads={n: p.grad.detach().double().cpu() for n, p in m.named_parameters() if p.grad is not None},
                         state={k: v.detach().clone().cpu() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k})
    return out


def _check_against(got, want, dtype, tol, kf, what):
    """tests/test_gpu_head_act.py _check_against, the output bound and the fp32 gradient bound times kf = K / 768 (module docstring)"""
    e_cls = float((got["cls"] - want["cls"]).abs().max()) / max(1.0, float(want["cls"].abs().max()))
    e_tab = float((got["table"] - want["table"]).abs().max()) / max(1.0, float(want["table"].abs().max()))
    gw = want["grads"]
    assert set(got["grads"]) == set(gw), set(got["grads"]) ^ set(gw)
    gmax = max(float(v.norm()) for v in gw.values())
    floor = (1e-5 if dtype == "fp32" else 2e-3) * gmax
    worst = max((float((got["grads"][n] - gw[n]).norm()) / max(float(gw[n].norm()), floor), n) for n in gw)
    fusion = max((float((got["grads"][n] - gw[n]).norm()) / max(float(gw[n].norm()), floor), n) for n in gw if n.startswith("trunc_"))
    e_dx = float((got["dx"] - want["dx"]).norm()) / float(want["dx"].norm())
    print("%s %s: cls %.2e table %.2e worst parameter gradient %.2e (%s), of the fusion's %.2e (%s), d features %.2e"
          % (what, dtype, e_cls, e_tab, worst[0], worst[1], fusion[0], fusion[1], e_dx))
    assert e_cls <= tol * kf and e_tab <= tol * kf
    assert worst[0] < (10 * tol * kf if dtype == "fp32" else 0.35), worst
    assert e_dx < (10 * tol * kf if dtype == "fp32" else 0.35)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("dtype,tol", [("fp32", 2e-3), ("bf16", 8e-2)])
@pytest.mark.parametrize("k,norm,relu", TRAIN_SETTINGS)
def test_forward_train_forms_agree_with_each_other_and_the_statement(k, norm, relu, dtype, tol, fused, deterministic, gold):
    setting = (k, norm, relu)
    ref = _train_reference(setting, dtype)
    names = set(ref["grads"])
    assert {"trunc_heatmap_conv.0.weight", "trunc_heatmap_conv.0.bias", "trunc_offset_conv.3.weight", "trunc_offset_conv.3.bias"} <= names
    assert ("trunc_offset_conv.1.weight" in names) == (norm == "BN") and ref["grads"]["trunc_offset_conv.0.weight"].shape == (256, 256, k)
    out = _train_forms(setting, dtype, ref, fused)
    name = EF.setting_name(*setting)
    for form in ("dense", "sparse", "gram"):
        _check_against(out[form], ref, dtype, tol, _kf(k), "%s fused=%s %s vs statement" % (name, fused, form))
        if form != "dense":
            _check_against(out[form], out["dense"], dtype, tol, _kf(k), "%s fused=%s %s vs dense" % (name, fused, form))
        st = out[form]["state"]
        assert ("trunc_heatmap_conv.1.running_mean" in st) == (norm == "BN")
        for q, v in ref["running"].items():                              # every norm's running statistics after the step
            assert float((st[q].double() - v).abs().max()) <= (1e-4 if dtype == "fp32" else 1e-3) * max(1.0, float(v.abs().max())), (form, q)
        assert all(int(v) == 1 for q, v in st.items() if "num_batches" in q)
        if dtype == "fp32" and norm == "BN":                             # ... and the reference's own, for the two BatchNorm1d
            for f in ("trunc_heatmap_conv", "trunc_offset_conv"):
                for s_ in ("running_mean", "running_var"):
                    want = torch.from_numpy(gold["%s/train_%s.1.%s" % (name, f, s_)])
                    assert float((st["%s.1.%s" % (f, s_)] - want).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max())), (form, f, s_)


# ---- 4. the whole training step -------------------------------------------------------------------------------------------------------------
OUT_W, OUT_H = 40, 24


def _detector(dtype, cfg, seed=3):
    from monoflex_amd import synthetic as S
    from monoflex_amd.model.detector import KeypointDetector
    m = KeypointDetector(cfg)
    m.load_state_dict(S.synthetic_state_dict(m.state_dict(), seed=seed, cls_bias=-1.0))
    m = m.to(DEV).train()
    m.heads.loss_evaluator.log_as_float = False
    return m


def test_captured_training_step_at_k5_without_a_norm(deterministic):
    """The trainer's graph path at B = 2 on a 24 x 40 map, k = 5, no norm, ReLU: it captures, replays, gives a finite loss and equals the eager step."""
    from monoflex_amd import synthetic as S
    from monoflex_amd.engine.trainer import GraphedTrainStep, prepare_targets, train_step
    from monoflex_amd.solver import build_optimizer
    from monoflex_amd.structures.params_3d import make_train_target
    cfg = HA.make_cfg(inplace_abn=True, extra=EF.setting_opts(5, "none", True) + ["INPUT.WIDTH_TRAIN", OUT_W * 4, "INPUT.HEIGHT_TRAIN", OUT_H * 4])
    cfg.MODEL.COMPUTE_DTYPE = "bf16"
    b = _detector("bf16", cfg)
    pr = b.heads.predictor
    assert pr.edge_halo == 2 and isinstance(pr.trunc_offset_conv[1], torch.nn.Identity) and "heads.predictor.trunc_offset_conv.1.weight" not in b.state_dict()
    tg = [make_train_target(S.synthetic_train_target(20 + i, out_w=OUT_W, out_h=OUT_H, n_obj=3 + i)).to(DEV) for i in range(2)]
    imgs, tg = S.synthetic_images(2, OUT_H * 4, OUT_W * 4, seed=20).to(DEV), prepare_targets(b, tg, DEV)
    opt_b = build_optimizer(b, cfg, capturable=True)
    step = GraphedTrainStep(b, opt_b, imgs, tg, warmup=2)
    torch.cuda.synchronize()
    a = _detector("bf16", cfg, seed=5)
    a.load_state_dict({q: v.detach().clone() for q, v in b.state_dict().items()})
    opt_a = build_optimizer(a, cfg, capturable=True)
    opt_a.load_state_dict(copy.deepcopy(opt_b.state_dict()))
    w0 = pr.trunc_heatmap_conv[0].weight.detach().clone()         # (the class fusion: the dense focal loss reaches it at every border pixel)
    for it in range(2):
        loss_b = step().clone()
        loss_a, loss_dict, _ = train_step(a, opt_a, imgs, tg)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss_a)) and all(bool(torch.isfinite(v)) for v in loss_dict.values())
        assert torch.equal(loss_a, loss_b), (it, float(loss_a), float(loss_b))
    sa, sb = a.state_dict(), b.state_dict()
    diff = [q for q in sa if not torch.equal(sa[q], sb[q])]
    assert not diff, diff[:8]
    assert w0.shape == (256, 256, 5) and not torch.equal(pr.trunc_heatmap_conv[0].weight.detach(), w0)         # the k = 5 Conv1d trains
