"""The bf16-only kernels of the benchmarked mode, each checked DIRECTLY against the CPU oracle (oracle/dcn_v2_ref.c for the
deformable conv, torch fp32 convolution for the rest) on bf16-representable inputs and on the real layer shapes of the
1280x384 network -- not against another HIP kernel.

Error model of a bf16 layer whose inputs are exact in bf16: fp32 accumulation (error ~1e-6 relative), then ONE rounding of
the output to bf16 (2^-9 = 1.95e-3 relative).  The DCN LDS-patch kernel additionally blends the four corners in packed fp16
(2^-11 per operation, weights carry the mask) before its fp16 MFMA.  Bounds below are ~2x the values observed on MI355X
(printed by the tests; recorded in profiles/r02_bf16_kernel_parity.json)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBSERVED = {}


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _bf(t):
    return t.bfloat16().float()


# the two 16-bit activation types of the inference path: bf16 (benchmarked mode; also training) and IEEE fp16 (inference mode "fp16":
# same kernels instantiated for half_t).  `tight` scales the bf16 bounds: one output rounding is 2^-9 in bf16, 2^-11 in fp16.
DTYPES = {"bf16": (torch.bfloat16, 1.0, 1.0), "fp16": (torch.float16, 0.125, 0.22)}     # (torch dtype, conv/stem bound scale, DCN bound scale)
# (fp16 observed on MI355X: conv / stem 3.7e-4 max, 1.8e-4 mean; DCN 8.5e-4 max, 4.9e-4 mean -- the scales keep the bounds at ~2x)


def _record(name, **kv):
    OBSERVED[name] = {k: float(v) for k, v in kv.items()}
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    with open(os.path.join(ROOT, "gpurun_out", "bf16_kernel_parity.json"), "w") as f:
        json.dump(OBSERVED, f, indent=1, sort_keys=True)


def _errs(got, want):
    d = (got - want).abs()
    return float(d.max() / want.abs().max().clamp(min=1.0)), float(d.mean() / want.abs().mean().clamp(min=1e-6))


# (B, Cin, Cout, H, W, offset std, patch variants that must be exercised)
DCN_REAL_SHAPES = [
    (1, 64, 64, 96, 320, 1.5, (2, 3, 4, 5, 6, 7, 8)),          # dla_up.ida_2.node_*, ida_up.node_* (5 of the 16 layers)
    (1, 128, 64, 48, 160, 1.5, (2, 3, 4, 5, 6, 7, 8)),         # dla_up.ida_2.proj_*, ida_up.proj_1
    (2, 64, 64, 96, 320, 5.0, (5, 8)),                        # offsets of several pixels: many samples leave the +-7 patch
]


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("B,C,Co,H,W,std,variants", DCN_REAL_SHAPES)
def test_dcn_patch_kernel_vs_c_oracle_real_shapes(B, C, Co, H, W, std, variants, dt):
    """dcn_patch_kernel (every tile height / margin variant, plus the automatic dispatch) against oracle/dcn_v2_ref.c:
    the reference's im2col + GEMM arithmetic in fp32 (src/cuda/dcn_v2_im2col_cuda.cu:125-195)."""
    from monoflex_amd import lib as L, ops
    from oracle import dcn_ref
    tdt, _, ds = DTYPES[dt]
    _bf = lambda t: t.to(tdt).float()                       # noqa: E731  (round to the mode's activation type)
    if dt == "fp16":
        variants = tuple(v for v in variants if v == 8)      # fp16 maps: the production variant (padded +-7 px patch) only
    g = _g(101)
    x = _bf(torch.randn(B, C, H, W, generator=g).relu())
    off = torch.randn(B, 18, H, W, generator=g) * std
    msk = torch.sigmoid(torch.randn(B, 9, H, W, generator=g))
    off[0, :, 0, 0] = 40.0                                  # far outside the map
    off[0, 0::2, 1, 1] = -1.0                               # exactly on the -1 boundary (excluded: h > -1)
    w = _bf(torch.randn(Co, C, 3, 3, generator=g) / (3 * C ** 0.5))
    b = torch.randn(Co, generator=g) * 0.1
    want = dcn_ref.dcn_v2_forward(x, w, b, off, msk, 3, 3, 1, 1, 1, 1, 1, 1, 1)        # (B,Co,H,W) fp32, CPU
    om = torch.zeros(B, H, W, 32)
    om[..., :18] = off.permute(0, 2, 3, 1)
    om[..., 18:27] = msk.permute(0, 2, 3, 1)
    xd = x.permute(0, 2, 3, 1).contiguous().to(tdt).to(DEV)
    p = ops.pack_conv(w.to(DEV), tdt, None, b.to(DEV), stride=1, pad=1, act=L.ACT_NONE)
    ops.add_f16_fragments(p, w.to(DEV))
    lib_ = L.load()
    worst = (0.0, 0.0)
    try:
        for v in (1,) + tuple(variants):
            L.check(lib_.mfx_set_option(b"dcn_patch", v), "opt")
            got = ops.dcn(xd, om.to(DEV), p).float().cpu().permute(0, 3, 1, 2)
            emax, emean = _errs(got, want)
            worst = (max(worst[0], emax), max(worst[1], emean))
            assert emax <= 7.5e-3 * ds and emean <= 4.5e-3 * ds, (v, emax, emean)        # observed (bf16) 3.5e-3 / 2.2e-3
    finally:
        L.check(lib_.mfx_set_option(b"dcn_patch", 1), "opt")
    print("dcn_patch %s %d->%d@%dx%d std %.1f: worst max-rel %.2e mean-rel %.2e" % (dt, C, Co, H, W, std, *worst))
    _record("dcn_patch_%s_%d_%d_%dx%d_std%.1f" % (dt, C, Co, H, W, std), max_rel=worst[0], mean_rel=worst[1])


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("B,C,Co,H,W", [(1, 512, 256, 12, 40), (1, 256, 128, 24, 80), (1, 128, 128, 48, 160)])
def test_dcn_generic_and_wave_kernels_vs_c_oracle_real_shapes(B, C, Co, H, W, dt):
    """The other bf16 DCN kernels of the step (first-generation gather igemm with split-K, wave-private variant) on the
    remaining distinct layer shapes, automatic dispatch, against the C oracle."""
    from monoflex_amd import lib as L, ops
    from oracle import dcn_ref
    tdt, _, ds = DTYPES[dt]
    _bf = lambda t: t.to(tdt).float()                       # noqa: E731
    g = _g(102)
    x = _bf(torch.randn(B, C, H, W, generator=g).relu())
    off = torch.randn(B, 18, H, W, generator=g) * 2.0
    msk = torch.sigmoid(torch.randn(B, 9, H, W, generator=g))
    w = _bf(torch.randn(Co, C, 3, 3, generator=g) / (3 * C ** 0.5))
    b = torch.randn(Co, generator=g) * 0.1
    want = dcn_ref.dcn_v2_forward(x, w, b, off, msk, 3, 3, 1, 1, 1, 1, 1, 1, 1)
    om = torch.zeros(B, H, W, 32)
    om[..., :18] = off.permute(0, 2, 3, 1)
    om[..., 18:27] = msk.permute(0, 2, 3, 1)
    p = ops.pack_conv(w.to(DEV), tdt, None, b.to(DEV), stride=1, pad=1, act=L.ACT_NONE)
    ops.add_f16_fragments(p, w.to(DEV))
    got = ops.dcn(x.permute(0, 2, 3, 1).contiguous().to(tdt).to(DEV), om.to(DEV), p).float().cpu().permute(0, 3, 1, 2)
    emax, emean = _errs(got, want)
    print("dcn %s %d->%d@%dx%d: max-rel %.2e mean-rel %.2e" % (dt, C, Co, H, W, emax, emean))
    _record("dcn_auto_%s_%d_%d_%dx%d" % (dt, C, Co, H, W), max_rel=emax, mean_rel=emean)
    assert emax <= 7.5e-3 * ds and emean <= 4.5e-3 * ds        # observed (bf16) <= 3.6e-3 / 2.2e-3


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_stem_kernel_vs_torch_full_resolution(dt):
    """stem_conv7x7_kernel (reads the fp32 NCHW planes, rounds them to bf16 itself) at 384x1280 against F.conv2d on the
    bf16-rounded image and weights + folded BN + ReLU (dla_dcn.py:268-272)."""
    from monoflex_amd import lib as L, ops
    tdt, cs, _ = DTYPES[dt]
    _bf = lambda t: t.to(tdt).float()                       # noqa: E731
    g = _g(103)
    img = torch.randn(1, 3, 384, 1280, generator=g)
    w = torch.randn(16, 3, 7, 7, generator=g) * (2.0 / 147) ** 0.5
    scale, shift = torch.rand(16, generator=g) * 0.4 + 0.8, torch.randn(16, generator=g) * 0.1
    ref = torch.relu(F.conv2d(_bf(img), _bf(w), padding=3) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
    p = ops.pack_stem(w.to(DEV), tdt, scale.to(DEV), shift.to(DEV), act=L.ACT_RELU)
    got = ops.stem_conv(img.to(DEV), p).float().cpu().permute(0, 3, 1, 2)
    emax, emean = _errs(got, ref)
    print("stem %s 384x1280: max-rel %.2e mean-rel %.2e" % (dt, emax, emean))
    _record("stem_%s_384x1280" % dt, max_rel=emax, mean_rel=emean)
    assert emax <= 4e-3 * cs and emean <= 2.9e-3 * cs          # observed (bf16) 2.0e-3 / 1.4e-3


CONV_VARIANT_CASES = [
    # name, (B,H,W,Cin,Cout), option, values, out fp32?, epilogue
    ("offset_conv_k_split_waves", (1, 96, 320, 64, 27), b"halo", (1, 9, 10, 11), True, "offmask"),
    ("offset_conv_k_split_waves_c512", (2, 12, 40, 512, 27), b"halo", (1, 9, 10, 11), True, "offmask"),
    ("halo_wide_c64", (1, 96, 320, 64, 64), b"halo", (1, 7, 13, 14), False, "bn_res_relu"),
    ("halo_wide_c128", (1, 48, 160, 128, 128), b"halo", (1, 8, 12, 15), False, "bn_res_relu"),
    ("halo_wide_c256", (2, 24, 80, 256, 256), b"halo", (1, 6, 12), False, "bn_res_relu"),
    ("halo_wide_c512", (2, 12, 40, 512, 512), b"halo", (1, 12), False, "bn_res_relu"),
    ("generic_split_k_c512", (2, 12, 40, 512, 512), b"ksplit", (1, 2, 3, 8), False, "bn_res_relu"),
]


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("name,shape,opt,values,f32out,epi", CONV_VARIANT_CASES)
def test_conv3x3_kernel_variants_vs_torch_real_shapes(name, shape, opt, values, f32out, epi, dt):
    """Every 3x3/s1 kernel variant the bf16 step can dispatch to (LDS-halo tiles with and without K-split waves, narrow
    fp32-out offset/mask conv with its sigmoid epilogue, cross-workgroup split-K) forced one by one on the layer shapes it
    serves, against F.conv2d in fp32 on the bf16-rounded operands."""
    from monoflex_amd import lib as L, ops
    B, H, W, Ci, Co = shape
    tdt, cs, _ = DTYPES[dt]
    _bf = lambda t: t.to(tdt).float()                       # noqa: E731
    g = _g(104)
    x = _bf(torch.randn(B, Ci, H, W, generator=g).relu())
    w = _bf(torch.randn(Co, Ci, 3, 3, generator=g) / (3 * Ci ** 0.5))
    ref = F.conv2d(x, w, padding=1)
    xd = x.permute(0, 2, 3, 1).contiguous().to(tdt).to(DEV)
    if epi == "offmask":
        bias = torch.randn(Co, generator=g)
        ref = ref + bias.view(1, -1, 1, 1)
        ref[:, 18:27] = torch.sigmoid(ref[:, 18:27])
        p = ops.pack_conv(w.to(DEV), tdt, None, bias.to(DEV), stride=1, pad=1, act=L.ACT_DCN_OFFMASK, cout=32)
        res_d = None
    else:
        scale, shift = torch.rand(Co, generator=g) * 0.4 + 0.3, torch.randn(Co, generator=g) * 0.1
        res = _bf(torch.randn(B, Co, H, W, generator=g))
        ref = torch.relu(ref * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1) + res)
        p = ops.pack_conv(w.to(DEV), tdt, scale.to(DEV), shift.to(DEV), stride=1, pad=1, act=L.ACT_RELU)
        res_d = res.permute(0, 2, 3, 1).contiguous().to(tdt).to(DEV)
    if opt == b"ksplit":
        p.w_frag = None                                      # keep the layer on the generic implicit-GEMM kernel
    lib_ = L.load()
    worst = (0.0, 0.0)
    try:
        for v in values:
            L.check(lib_.mfx_set_option(opt, v), "opt")
            y = ops.conv2d(xd, p, res=res_d, out_dtype=torch.float32 if f32out else None)
            got = y.float().cpu().permute(0, 3, 1, 2)[:, :Co]
            emax, emean = _errs(got, ref)
            worst = (max(worst[0], emax), max(worst[1], emean))
            bound = (2e-6, 5e-7) if f32out else (6e-3 * cs, 2.9e-3 * cs)          # observed (bf16) 3.9e-7 / 1.1e-7 (fp32 out: accumulation order only) and 3.0e-3 / 1.4e-3
            assert emax <= bound[0] and emean <= bound[1], (name, v, emax, emean)
    finally:
        L.check(lib_.mfx_set_option(opt, 1 if opt == b"halo" else 0), "opt")
    print("%s %s: worst max-rel %.2e mean-rel %.2e" % (name, dt, *worst))
    _record(name + "_" + dt, max_rel=worst[0], mean_rel=worst[1])


# ---- the production shapes of the B = 8 step (batch > 1 at 96x320: the LDS-patch kernels' image boundaries; the dispatch counters
# (mfx_get_counter) pin which kernel family ran)

def _om_nhwc(off, msk):
    B, _, H, W = off.shape
    om = torch.zeros(B, H, W, 32)
    om[..., :18] = off.permute(0, 2, 3, 1)
    om[..., 18:27] = msk.permute(0, 2, 3, 1)
    return om


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("std", [1.5, 5.0])
def test_dcn_lds_kernel_vs_c_oracle_batched_production_shape(std, dt):
    """dcn_lds_kernel (the 64 -> 64 layers at B * H * W >= 65536, automatic dispatch) at B = 3, 96x320 against oracle/dcn_v2_ref.c; std 5.0
    sends many samples beyond the +-7 px patch (the far pass); plus samples far outside the map and exactly on the -1 boundary, in the last image."""
    from monoflex_amd import lib as L, ops
    from oracle import dcn_ref
    tdt, _, ds = DTYPES[dt]
    rnd = lambda t: t.to(tdt).float()                       # noqa: E731
    B, C, Co, H, W = 3, 64, 64, 96, 320
    g = _g(105)
    x = rnd(torch.randn(B, C, H, W, generator=g).relu())
    off = torch.randn(B, 18, H, W, generator=g) * std
    msk = torch.sigmoid(torch.randn(B, 9, H, W, generator=g))
    off[B - 1, :, 0, 0] = 40.0
    off[B - 1, :, H - 1, W - 1] = -40.0
    off[B - 1, 0::2, 1, 1] = -1.0
    off[B - 1, 1::2, 2, 5] = -1.0
    w = rnd(torch.randn(Co, C, 3, 3, generator=g) / (3 * C ** 0.5))
    b = torch.randn(Co, generator=g) * 0.1
    want = dcn_ref.dcn_v2_forward(x, w, b, off, msk, 3, 3, 1, 1, 1, 1, 1, 1, 1)
    p = ops.pack_conv(w.to(DEV), tdt, None, b.to(DEV), stride=1, pad=1, act=L.ACT_NONE)
    ops.add_f16_fragments(p, w.to(DEV))
    lib_ = L.load()
    n0 = lib_.mfx_get_counter(b"dcn_lds")
    got = ops.dcn(x.permute(0, 2, 3, 1).contiguous().to(tdt).to(DEV), _om_nhwc(off, msk).to(DEV), p).float().cpu().permute(0, 3, 1, 2)
    torch.cuda.synchronize()
    assert lib_.mfx_get_counter(b"dcn_lds") == n0 + 1                     # the LDS kernel took it
    emax, emean = _errs(got, want)
    print("dcn_lds %s B=%d std %.1f: max-rel %.2e mean-rel %.2e" % (dt, B, std, emax, emean))
    _record("dcn_lds_%s_b%d_std%.1f" % (dt, B, std), max_rel=emax, mean_rel=emean)
    for i in range(B):                                                    # every image on its own (an image-boundary slip stays visible)
        ei = _errs(got[i:i + 1], want[i:i + 1])
        assert ei[0] <= 7.5e-3 * ds and ei[1] <= 4.5e-3 * ds, (i, ei)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_dcn_lds_fused_offset_conv_vs_c_oracle_b8(dt):
    """The OF path of dcn_lds_kernel (offset/mask conv computed inside, ops.dcn_module) at B = 8, 96x320: the returned offset map against a
    float64 offset conv + sigmoid, and the output against oracle/dcn_v2_ref.c fed with the kernel's own offsets; `need_offmask` must not change y."""
    from monoflex_amd import lib as L, ops
    from oracle import dcn_ref
    tdt, _, ds = DTYPES[dt]
    rnd = lambda t: t.to(tdt).float().half().float()       # noqa: E731  (exact in the map type AND in the kernel's fp16 operands)
    B, C, Co, H, W = 8, 64, 64, 96, 320
    g = _g(106)
    x = rnd(torch.randn(B, C, H, W, generator=g).relu())
    wo = rnd(torch.randn(27, C, 3, 3, generator=g) * 0.09)                # offsets of std ~1.5 px
    bo = torch.randn(27, generator=g) * 0.5
    w = rnd(torch.randn(Co, C, 3, 3, generator=g) / (3 * C ** 0.5))
    b = torch.randn(Co, generator=g) * 0.1
    p_off = ops.add_f16_fragments(ops.pack_conv(wo.to(DEV), tdt, None, bo.to(DEV), stride=1, pad=1, act=L.ACT_DCN_OFFMASK, cout=32), wo.to(DEV))
    p = ops.add_f16_fragments(ops.pack_conv(w.to(DEV), tdt, None, b.to(DEV), stride=1, pad=1, act=L.ACT_NONE), w.to(DEV))
    xd = x.permute(0, 2, 3, 1).contiguous().to(tdt).to(DEV)
    lib_ = L.load()
    n0 = lib_.mfx_get_counter(b"dcn_lds_of")
    y, om = ops.dcn_module(xd, p_off, p, need_offmask=True)
    y1, om1 = ops.dcn_module(xd, p_off, p)
    torch.cuda.synchronize()
    assert lib_.mfx_get_counter(b"dcn_lds_of") == n0 + 2 and om1 is None
    assert torch.equal(y, y1)
    om = om.cpu()
    ref = F.conv2d(x.double(), wo.double(), bo.double(), 1, 1)
    off_r, msk_r = ref[:, :18], torch.sigmoid(ref[:, 18:27])
    off_k, msk_k = om[..., :18].permute(0, 3, 1, 2).double(), om[..., 18:27].permute(0, 3, 1, 2).double()
    e_off = float(((off_k - off_r).abs() / off_r.abs().clamp(min=1.0)).max())
    e_msk = float((msk_k - msk_r).abs().max())
    want = dcn_ref.dcn_v2_forward(x, w, b, off_k.float(), msk_k.float(), 3, 3, 1, 1, 1, 1, 1, 1, 1)
    got = y.float().cpu().permute(0, 3, 1, 2)
    emax, emean = _errs(got, want)
    print("dcn_lds OF %s B=8: offsets %.2e mask %.2e (std %.2f) | max-rel %.2e mean-rel %.2e" % (dt, e_off, e_msk, float(off_r.std()), emax, emean))
    _record("dcn_lds_of_%s_b8" % dt, off_rel=e_off, mask_abs=e_msk, max_rel=emax, mean_rel=emean)
    assert e_off <= 5e-6 and e_msk <= 1e-6            # observed 1.7e-6 / 4.0e-7: exact operands, fp32 sums (the table's 2e-3 covers rounded weights)
    for i in range(B):
        ei = _errs(got[i:i + 1], want[i:i + 1])
        assert ei[0] <= 7.5e-3 * ds and ei[1] <= 4.5e-3 * ds, (i, ei)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("B,C,Co,H,W", [(8, 512, 256, 12, 40), (8, 256, 64, 24, 80)])
def test_dcn_project_then_sample_vs_c_oracle(B, C, Co, H, W, dt):
    """ops.dcn_ps (1x1 projection on gemm_as_kernel or the implicit-GEMM kernel, then dcn_sample_kernel) on the two layers of the step that take
    it, against oracle/dcn_v2_ref.c."""
    from monoflex_amd import lib as L, ops
    from oracle import dcn_ref
    tdt, _, ds = DTYPES[dt]
    rnd = lambda t: t.to(tdt).float()                       # noqa: E731
    g = _g(107)
    x = rnd(torch.randn(B, C, H, W, generator=g).relu())
    off = torch.randn(B, 18, H, W, generator=g) * 2.0
    msk = torch.sigmoid(torch.randn(B, 9, H, W, generator=g))
    off[B - 1, :, 0, 0] = 30.0
    off[B - 1, 0::2, 1, 1] = -1.0
    w = rnd(torch.randn(Co, C, 3, 3, generator=g) / (3 * C ** 0.5))
    b = torch.randn(Co, generator=g) * 0.1
    scale, shift = torch.rand(Co, generator=g) * 0.4 + 0.8, torch.randn(Co, generator=g) * 0.1
    want = torch.relu(dcn_ref.dcn_v2_forward(x, w, b, off, msk, 3, 3, 1, 1, 1, 1, 1, 1, 1) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
    p = ops.pack_conv(w.to(DEV), tdt, scale.to(DEV), (shift + b * scale).to(DEV), stride=1, pad=1, act=L.ACT_RELU)
    xd = x.permute(0, 2, 3, 1).contiguous().to(tdt).to(DEV)
    assert ops.dcn_ps_applies(xd, p)
    got = ops.dcn_ps(xd, _om_nhwc(off, msk).to(DEV), p).float().cpu().permute(0, 3, 1, 2)
    emax, emean = _errs(got, want)
    print("dcn_ps %s %d->%d@%dx%d B=%d: max-rel %.2e mean-rel %.2e" % (dt, C, Co, H, W, B, emax, emean))
    _record("dcn_ps_%s_%d_%d_%dx%d_b%d" % (dt, C, Co, H, W, B), max_rel=emax, mean_rel=emean)
    for i in range(B):
        ei = _errs(got[i:i + 1], want[i:i + 1])
        assert ei[0] <= 7.5e-3 * ds and ei[1] <= 4.5e-3 * ds, (i, ei)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_heads_fused_vs_float64_convs_b8(dt):
    """heads_fused_kernel (every branch: 3x3 64 -> 256 + BN + leaky ReLU, 1x1 -> the branch's heads) at B = 8, 96x320 against float64 torch
    convolutions (on the device) of the reference Predictor's branches, on 16-bit-exact features."""
    from monoflex_amd import ops
    from monoflex_amd.config import get_cfg
    from monoflex_amd.model.head.detector_predictor import _predictor, REG_OFF
    from monoflex_amd import synthetic as S
    from oracle import monoflex_ref as R
    tdt, _, _ = DTYPES[dt]
    cfg = get_cfg(os.path.join(ROOT, "runs", "monoflex.yaml"))
    ref = R.Predictor().eval()
    sd = S.synthetic_state_dict({"heads.predictor." + k: v for k, v in ref.state_dict().items()}, seed=3)
    ref.load_state_dict({k[len("heads.predictor."):]: v for k, v in sd.items()})
    m = _predictor(cfg, 64).eval()
    m.load_state_dict(ref.state_dict())
    m.to(DEV)
    ref = ref.to(DEV, torch.float64)
    x = torch.randn(8, 64, 96, 320, generator=_g(108)).relu().to(tdt).float()
    hm, _ = ops.heads_fused(x.permute(0, 2, 3, 1).contiguous().to(tdt).to(DEV), m._pack(tdt))
    with torch.no_grad():
        x64 = x.to(DEV, torch.float64)
        outs = [ref.class_head[-1](ref.class_head[:-1](x64))]
        for i, feat in enumerate(ref.reg_features):
            f = feat(x64)
            outs += [h(f) for h in ref.reg_heads[i]]
        want = torch.cat(outs, 1)
    got = torch.cat((hm[..., :3], hm[..., REG_OFF:REG_OFF + 50]), -1).permute(0, 3, 1, 2).double()
    worst = (0.0, 0.0)
    for i in range(8):
        ei = _errs(got[i:i + 1], want[i:i + 1])
        worst = (max(worst[0], ei[0]), max(worst[1], ei[1]))
    print("heads_fused %s B=8 96x320: max-rel %.2e mean-rel %.2e" % (dt, *worst))
    _record("heads_fused_%s_b8" % dt, max_rel=worst[0], mean_rel=worst[1])
    bound = (8e-3, 6e-3) if dt == "bf16" else (8e-4, 7e-4)    # observed bf16 3.9e-3 / 2.8e-3, fp16 3.8e-4 / 3.3e-4 (test_heads_fused_vs_torch: 5e-2)
    assert worst[0] <= bound[0] and worst[1] <= bound[1], worst
