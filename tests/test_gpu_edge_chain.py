"""The edge fusion's conv chain as one kernel (csrc/edge_chain.hip, ops.edge_chain, option / counter "edge_chain") against

  * the five mfx_conv2d_nhwc launches it replaces (option edge_chain = 0): the kernel issues the same MFMAs in the same K order and rounds at the same
    three places, so the results are asserted BIT-IDENTICAL (torch.equal) -- no factor between the two forms' errors is needed;
  * tests/edge_chain_ref.py, the float64 reference pinned to the oracle Predictor by tests/test_edge_chain_ref_cpu.py: operands rounded to the 16-bit
    type, no intermediate rounding.  The bound is not fitted: per output element it is what rounding the two intermediates to the activation type can
    move it by at most (edge_chain_ref's `bound`, unit roundoff 2^-8 bfloat16 / 2^-11 half), times 1.01 for the second-order terms, plus 1e-5 of the
    output's scale for the fp32 accumulation and the fp32 (against float64) folding of the normalisations.

    That bound is a worst case (every rounding error at its largest and of the sign that hurts): on the MI355X the errors measured were about 1 % of it
    -- B = 3, 24 x 40: max 5.6e-3 / mean 1.2e-3 in bfloat16, 7.3e-4 / 1.5e-4 in half (ReLU on; 9.7e-3 / 1.8e-3 and 1.1e-3 / 2.2e-4 with it off), outputs
    up to 3.0 -- and, being bit-identical, the same for both forms.  What catches a wrong kernel here is the equality with the five launches; the
    reference keeps that pair of forms from being wrong together.

A segment of the kernel is 62 sequence positions (+ 2 halo rows): the operator is run at sequence lengths around one and two segments, and the 24 x 40 and
16 x 48 maps (L = 128) have two full segments and a ragged third."""
import copy
import os

import pytest
import torch

from edge_chain_ref import D64, chain_operands, edge_chain_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SEG = 62
_cache = {}


def _lib():
    from monoflex_amd import lib as L, ops
    return ops, L, L.load()


def _model(relu):
    """The product predictor with synthetic weights (one per ReLU setting, shared by every test)."""
    if ("model", relu) not in _cache:
        from monoflex_amd import synthetic as S
        from monoflex_amd.config import get_cfg
        from monoflex_amd.model.head.detector_predictor import _predictor
        cfg = get_cfg(os.path.join(ROOT, "runs", "monoflex.yaml"), ["MODEL.HEAD.EDGE_FUSION_RELU", relu])
        m = _predictor(cfg, 64).eval()
        sd = S.synthetic_state_dict({"heads.predictor." + k: v for k, v in m.state_dict().items()}, seed=3)
        m.load_state_dict({k[len("heads.predictor."):]: v for k, v in sd.items()})
        assert isinstance(m.trunc_heatmap_conv[2], torch.nn.ReLU) == bool(relu)
        _cache[("model", relu)] = m.to(DEV)
    return _cache[("model", relu)]


def _features(B, H, W, dtype, seed=9):
    """(NHWC device tensor of `dtype`, the same values as float64 NCHW on the host)"""
    x = torch.randn(B, 64, H, W, generator=torch.Generator().manual_seed(seed)).relu().to(dtype)
    return x.permute(0, 2, 3, 1).contiguous().to(DEV), x.to(D64)


def _edge_indices(H, W, B, full=False):
    """(B, L, 2) int64 border points of an H x W map; `full`: the padding rows replaced by distinct interior pixels, so that an edge_len of L scatters
    to L different pixels (the padding rows all list pixel (0, 0))."""
    from monoflex_amd import synthetic as S
    tgt = S.synthetic_target(W, H)
    ei, n = tgt["edge_indices"].clone(), tgt["edge_len"]                  # (the point after the first edge_len closes the loop: a repeat)
    if full:
        k = ei.shape[0] - n
        ei[n:, 0], ei[n:, 1] = torch.arange(5, 5 + k), H // 2
        assert len({(int(a), int(b)) for a, b in ei}) == ei.shape[0]
    return torch.stack([ei] * B), tgt["edge_len"]


def _five_launches(ops, m, p, feats, ei32):
    """The chain as forward_nhwc runs it with option edge_chain = 0 -> fp32 (2, B, L, 4)"""
    from monoflex_amd.model.head.detector_predictor import make_edge_rowmap
    B, H, W, _ = feats.shape
    Lm = ei32.shape[1]
    trunk = ops.conv2d(feats, p.edge_trunk, rowmap=make_edge_rowmap(ei32, H, W)).view(B, 1, Lm + 2, 512)
    outs = []
    for bi, (pk1, pk2, _, _) in enumerate(p.edge_branches):
        outs.append(ops.conv2d(ops.conv2d(trunk, pk1, x_ch_off=bi * 256), pk2, out_dtype=torch.float32).view(B, Lm, 4))
    return torch.stack(outs)


def _judge(got, x64, ei, m, dtype, what):
    """got fp32 (2, B, L, 4) against the float64 reference within the rounding bound of the intermediates; returns (max, mean) error / max |ref|"""
    ref = edge_chain_ref(x64, ei, chain_operands(m, dtype), U[dtype])
    worst, mean = 0.0, 0.0
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
        worst, mean = max(worst, float(err.max()) / scale), max(mean, float(err.mean()) / scale)
    return worst, mean


def _written(t):
    """The channels of a head map the kernels write -- [0:3] class logits, [REG_OFF:REG_OFF + 50] regression; the rest of the 64 is never initialised."""
    from monoflex_amd.model.head.detector_predictor import REG_OFF
    return torch.cat((t[..., :3], t[..., REG_OFF:REG_OFF + 50]), -1)


def _cpu(relu):
    """the same predictor on the host, for chain_operands"""
    if ("cpu", relu) not in _cache:
        _cache[("cpu", relu)] = copy.deepcopy(_model(relu)).cpu()
    return _cache[("cpu", relu)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("B,H,W", [(1, 24, 40), (3, 24, 40), (2, 16, 48)])
def test_operator_equals_the_five_launches_and_meets_the_reference(dtype, relu, B, H, W):
    ops, L, lib = _lib()
    m = _model(relu)
    p = m._pack(dtype)
    assert p.edge_chain is not None and p.edge_chain.relu == bool(relu)
    feats, x64 = _features(B, H, W, dtype)
    ei, _ = _edge_indices(H, W, B)
    for b in range(1, B):                                  # every image its own sequence: rolled, so that the replicate-padded ends differ too
        ei[b] = torch.roll(ei[b], 7 * b, 0)
    ei32 = ei.to(DEV, torch.int32).contiguous()
    c0 = lib.mfx_get_counter(b"edge_chain")
    got = ops.edge_chain(feats, ei32, p.edge_chain)
    assert got is not None and got.shape == (2, B, ei.shape[1], 4) and lib.mfx_get_counter(b"edge_chain") == c0 + 1
    old = _five_launches(ops, m, p, feats, ei32)
    torch.cuda.synchronize()
    assert torch.equal(got, old), float((got - old).abs().max())
    _judge(got, x64, ei, _cpu(relu), dtype, "%s relu=%s %dx%dx%d" % (dtype, relu, B, H, W))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_sequence_lengths_around_the_segment_length(dtype):
    """L = 1, 2 and one below / at / one above one and two segments: halo rows that are clamped copies, a last segment of 1 .. 62 positions."""
    ops, L, lib = _lib()
    m = _model(True)
    p = m._pack(dtype)
    mcpu = _cpu(True)
    feats, x64 = _features(2, 24, 40, dtype)
    ei, _ = _edge_indices(24, 40, 2, full=True)
    ei[1] = torch.roll(ei[1], 31, 0)
    for Lm in (1, 2, SEG - 1, SEG, SEG + 1, 2 * SEG - 1, 2 * SEG, 2 * SEG + 1):
        e = ei[:, :Lm].contiguous()
        e32 = e.to(DEV, torch.int32).contiguous()
        got = ops.edge_chain(feats, e32, p.edge_chain)
        old = _five_launches(ops, m, p, feats, e32)
        torch.cuda.synchronize()
        assert got.shape == (2, 2, Lm, 4) and torch.equal(got, old), Lm
        _judge(got, x64, e, mcpu, dtype, "%s L=%d" % (dtype, Lm))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("relu", [True, False])
def test_forward_nhwc_equals_the_five_launch_form(dtype, relu):
    """The whole predictor, images with different edge_len: 0, 1, L - 1, L (no padding rows) and one below / above the segment length.  The head map and
    the planar class copy are bit-identical to the five-launch form's, the planar copy equals hm[..., :3], what the fusion added is the reference's
    output at the first edge_len points and nothing elsewhere, and the dispatch counter tells which form ran."""
    ops, L, lib = _lib()
    m = _model(relu)
    mcpu = _cpu(relu)
    H, W = 24, 40
    for lens in ([0, 1, 127], [128, SEG - 1, SEG + 1]):
        B = len(lens)
        feats, x64 = _features(B, H, W, dtype, seed=11)
        ei, _ = _edge_indices(H, W, B, full=True)
        Lm = ei.shape[1]
        assert Lm == 128
        ei32, el = ei.to(DEV, torch.int32).contiguous(), torch.tensor(lens, dtype=torch.int32, device=DEV)
        c0 = lib.mfx_get_counter(b"edge_chain")
        hm = m.forward_nhwc(feats, ei32, el)
        planar = m.last_cls_planar
        assert lib.mfx_get_counter(b"edge_chain") == c0 + 1
        L.set_options({"edge_chain": 0})
        hm0 = m.forward_nhwc(feats, ei32, el)
        planar0 = m.last_cls_planar
        assert lib.mfx_get_counter(b"edge_chain") == c0 + 1                  # not at all with the switch off
        L.set_options({"edge_chain": 1})
        base, _ = ops.heads_fused(feats, m._pack(dtype), planar_classes=3)
        torch.cuda.synchronize()
        assert torch.equal(_written(hm), _written(hm0)) and torch.equal(planar, planar0)
        assert torch.equal(planar.view(B, 3, H, W), hm[..., :3].permute(0, 3, 1, 2))
        # what the fusion added, against the reference
        ref = edge_chain_ref(x64, ei, chain_operands(mcpu, dtype), U[dtype])
        from monoflex_amd.model.head.detector_predictor import REG_OFF
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
        print("%s relu=%s lens=%s: fusion max err %.3e, worst err / tol %.3f" % (dtype, relu, lens, float(err.max()), float((err / tol).max())))
        assert bool((err <= tol).all())
        assert touched.sum() == 5 * sum(lens) and float(added[~touched].abs().max()) == 0.0      # pixels and channels the fusion does not touch


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_two_graph_replays_give_equal_head_maps(dtype):
    ops, L, lib = _lib()
    m = _model(True)
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


def test_fp32_input_keeps_the_five_launches():
    ops, L, lib = _lib()
    m = _model(True)
    assert m._pack(torch.float32).edge_chain is None
    feats, x64 = _features(1, 24, 40, torch.float32)
    ei, n = _edge_indices(24, 40, 1)
    c0, k0 = lib.mfx_get_counter(b"edge_chain"), lib.mfx_get_counter(b"conv_igemm")
    hm = m.forward_nhwc(feats, ei.to(DEV, torch.int32).contiguous(), torch.tensor([n], dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert lib.mfx_get_counter(b"edge_chain") == c0 and lib.mfx_get_counter(b"conv_igemm") == k0 + 5
    assert bool(torch.isfinite(hm[..., :3]).all())


def test_operator_declines_what_the_kernel_is_not_built_for():
    ops, L, lib = _lib()
    m = _model(True)
    p = m._pack(torch.bfloat16)
    feats, _ = _features(1, 24, 40, torch.bfloat16)
    ei, _ = _edge_indices(24, 40, 1)
    c0 = lib.mfx_get_counter(b"edge_chain")
    assert ops.edge_chain(feats, ei.to(DEV), p.edge_chain) is None                  # int64 coordinates
    assert ops.edge_chain(feats.half(), ei.to(DEV, torch.int32), p.edge_chain) is None      # activations of another type than the pack
    L.set_options({"edge_chain": 0})
    assert ops.edge_chain(feats, ei.to(DEV, torch.int32), p.edge_chain) is None
    assert lib.mfx_get_counter(b"edge_chain") == c0
