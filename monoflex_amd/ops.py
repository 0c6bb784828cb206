"""Tensor-level wrappers over the C ABI (include/monoflex_hip.h).

Activations are torch CUDA tensors in physical NHWC layout, shape (B, H, W, C), dtype float32
(parity mode) or bfloat16 (perf mode).  torch is used for device memory and the current HIP stream
only; every arithmetic op below runs in libmonoflex_hip.so.  The weight layouts these operators
read are defined in packing.py; its names are re-exported here.
"""
import ctypes
import os
from typing import Optional

import torch

from . import lib as L
from .packing import (F16X2, STEM_PAD_H, STEM_PAD_WL, STEM_PAD_WR, PackedCat, PackedConv, PackedEdgeChain, PackedHeads, _elems, _pad_rows_cols, _pow2,       # noqa: F401
                      _round_up, add_f16_fragments, cast_operand, compute_tag, cout_pad, dcn_pair_fragments, dcn_ps_pack, fold_bn, fragment_major,
                      pack_cat, pack_conv, pack_edge_chain, pack_heads, pack_stem, pack_upsample, pair_steps, split_chunks, split_halves, split_weight_scale,
                      storage_dtype)


def _stream():
    """The current HIP stream of the CURRENT device: every entry point below runs under `on_tensor_device`, which makes the
    operands' device current first, so a model on cuda:N launches on cuda:N's stream whatever the caller's current device is."""
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _first_cuda_device(args):
    for a in args:
        if torch.is_tensor(a):
            if a.is_cuda:
                return a.device
        elif isinstance(a, (list, tuple)):
            d = _first_cuda_device(a)
            if d is not None:
                return d
    return None


def on_tensor_device(fn):
    """Run `fn` with the device of its first CUDA tensor argument current (kernels, streams and scratch buffers are all
    looked up through the current device); other CUDA operands must live on the same device."""
    import functools

    @functools.wraps(fn)
    def run(*args, **kwargs):
        dev = _first_cuda_device(args) or _first_cuda_device(tuple(kwargs.values()))
        if dev is None or dev.index == torch.cuda.current_device():
            return fn(*args, **kwargs)
        with torch.cuda.device(dev):
            return fn(*args, **kwargs)
    return run


def _dt(dtype):
    if dtype == torch.float32:
        return L.MFX_F32
    if dtype == torch.bfloat16:
        return L.MFX_BF16
    if dtype == torch.float16:
        return L.MFX_F16
    raise TypeError("MonoFlex HIP kernels take float32, bfloat16 or float16, got %s" % dtype)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _need_cuda(*ts):
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("MonoFlex HIP operator called with a CPU tensor: the product path has no CPU "
                               "fallback (the CPU oracle lives in oracle/ and is test-only)")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError("MonoFlex HIP operator: operands on different devices (%s and %s)" % (dev, t.device))


# --------------------------------------------------------------------------------------------
# operators
# --------------------------------------------------------------------------------------------
@on_tensor_device
def conv2d(x, p: PackedConv, res=None, out_dtype=None, rowmap=None, x_channels=None, x_ch_off=0,
           out_hw=None, in_hw=None, stats=None):
    """y = act(conv(x)*scale + shift (+res)).  x: (B,H,W,Cx) NHWC.  With `rowmap` (int32 [M], pixel
    indices into the (B,Ho,Wo) grid, -1 = zero row) the output is the dense (M, Cout) row list."""
    _need_cuda(x, res, rowmap)
    B, H, W, Cx = x.shape
    if in_hw is not None:
        H, W = in_hw
    out_dtype = out_dtype or x.dtype
    if out_hw is None:
        Ho = (H + 2 * p.pad_h - ((p.kh - 1) + 1)) // p.stride + 1
        Wo = (W + 2 * p.pad_w - (p.dil_w * (p.kw - 1) + 1)) // p.stride + 1
    else:
        Ho, Wo = out_hw
    M = B * Ho * Wo if rowmap is None else rowmap.numel()
    y = torch.empty((B, Ho, Wo, p.Cout) if rowmap is None else (M, p.Cout), dtype=out_dtype, device=x.device)
    d = L.ConvDesc()
    d.x = x.data_ptr() + x_ch_off * x.element_size()
    d.w, d.scale, d.shift = p.w.data_ptr(), (p.scale.data_ptr() if p.scale is not None else None), \
        (p.shift.data_ptr() if p.shift is not None else None)
    d.w_frag = p.w_frag.data_ptr() if p.w_frag is not None else None
    d.w_frag_pair = p.w_frag_pair.data_ptr() if p.w_frag_pair is not None else None
    d.res = res.data_ptr() if res is not None else None
    d.y = y.data_ptr()
    d.rowmap = rowmap.data_ptr() if rowmap is not None else None
    d.B, d.H, d.W, d.x_pixstride, d.Ck = B, H, W, Cx, p.Ck
    d.kh, d.kw, d.stride, d.pad_h, d.pad_w, d.dil_w = p.kh, p.kw, p.stride, p.pad_h, p.pad_w, p.dil_w
    d.Ho, d.Wo, d.M, d.Cout, d.Cout_pad, d.K_pad = Ho, Wo, M, p.Cout, p.Cout_pad, p.K_pad
    d.ldy, d.ldres = p.Cout, (res.shape[-1] if res is not None else 0)
    d.act, d.dtype, d.out_dtype = p.act, (L.MFX_F16X2 if p.split else _dt(x.dtype)), _dt(out_dtype)
    if rowmap is None and M * p.Cout_pad <= SPLITK_MAX_ELEMS and p.K_pad * x.element_size() >= 2048:
        ws = _splitk_workspace(x.device)                      # small-M / long-K layers: lets the library split K
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    if stats is not None:
        # train-mode BN statistics of y accumulated by the conv's epilogue into the BN layer's scratch (where the kernel that
        # runs supports it: conv2d.last_stats_done tells the caller whether a statistics pass is still needed)
        done = ctypes.c_int(0)
        d.stats, d.stats_ncopy, d.stats_done = stats.data_ptr(), L.load().mfx_bn_ncopy(p.Cout), ctypes.pointer(done)
        L.check(L.load().mfx_conv2d_nhwc(ctypes.byref(d), _stream()), "mfx_conv2d_nhwc")
        conv2d.last_stats_done = bool(done.value)
        return y
    L.check(L.load().mfx_conv2d_nhwc(ctypes.byref(d), _stream()), "mfx_conv2d_nhwc")
    return y


conv2d.last_stats_done = False


@on_tensor_device
def cat_conv1x1(srcs, p: PackedCat):
    """Root: 1x1 conv over the virtual concat of `srcs` (list of (B,H,W,Ci) tensors)."""
    _need_cuda(*srcs)
    B, H, W, _ = srcs[0].shape
    y = torch.empty((B, H, W, p.Cout), dtype=srcs[0].dtype, device=srcs[0].device)
    d = L.CatDesc()
    n = 0
    for s in srcs:
        C = s.shape[3]
        for part in range(C // p.Cseg):
            d.src[n], d.stride[n], d.off[n] = s.data_ptr(), C, part * p.Cseg
            n += 1
    d.nseg, d.Cseg = n, p.Cseg
    d.w, d.res, d.y = p.w.data_ptr(), None, y.data_ptr()
    d.scale = p.scale.data_ptr() if p.scale is not None else None
    d.shift = p.shift.data_ptr() if p.shift is not None else None
    d.M, d.Cout, d.Cout_pad, d.K_pad, d.ldy, d.ldres, d.act = B * H * W, p.Cout, p.Cout_pad, p.K_pad, p.Cout, 0, p.act
    d.dtype = L.MFX_F16X2 if p.split else _dt(y.dtype)
    L.check(L.load().mfx_cat_conv1x1_nhwc(ctypes.byref(d), _stream()), "mfx_cat_conv1x1_nhwc")
    return y


def _dcn_desc(x, offmask, p: PackedConv, y, off: Optional[PackedConv] = None, offmask_out=None):
    B, H, W, C = x.shape
    Ho, Wo = y.shape[1], y.shape[2]
    d = L.DcnDesc()
    d.x, d.w, d.y = x.data_ptr(), p.w.data_ptr(), y.data_ptr()
    d.offmask = offmask.data_ptr() if offmask is not None else None
    d.w_frag = p.w_frag.data_ptr() if p.w_frag is not None else None
    d.w_frag_f16 = p.w_frag_f16.data_ptr() if p.w_frag_f16 is not None else None
    d.w_pair_f16 = p.w_pair_f16.data_ptr() if p.w_pair_f16 is not None else None
    d.scale = p.scale.data_ptr() if p.scale is not None else None
    d.shift = p.shift.data_ptr() if p.shift is not None else None
    d.B, d.H, d.W, d.C = B, H, W, C
    d.kh, d.kw, d.stride, d.pad, d.dil = p.kh, p.kw, p.stride, p.pad_h, p.dil_w
    d.Ho, d.Wo, d.Cout, d.Cout_pad, d.K_pad, d.ldy, d.act = Ho, Wo, p.Cout, p.Cout_pad, p.K_pad, p.Cout, p.act
    d.dtype = L.MFX_F16X2 if p.split else _dt(x.dtype)
    if off is not None and off.w_frag_f16 is not None and off.shift is not None and off.Cout_pad == 32 and off.K_pad == 9 * C:
        d.off_w_frag_f16, d.off_shift = off.w_frag_f16.data_ptr(), off.shift.data_ptr()
        d.offmask_out = offmask_out.data_ptr() if offmask_out is not None else None
    return d


@on_tensor_device
def dcn(x, offmask, p: PackedConv):
    """Fused DCNv2 + scale/shift + act.  x (B,H,W,C) NHWC, offmask fp32 (B,Ho,Wo,32)."""
    _need_cuda(x, offmask)
    B = x.shape[0]
    Ho, Wo = offmask.shape[1], offmask.shape[2]
    y = torch.empty((B, Ho, Wo, p.Cout), dtype=x.dtype, device=x.device)
    d = _dcn_desc(x, offmask, p, y)
    if B * Ho * Wo * p.Cout_pad <= SPLITK_MAX_ELEMS:           # small maps: lets the library split K over workgroups
        ws = _splitk_workspace(x.device)
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    L.check(L.load().mfx_dcn_nhwc(ctypes.byref(d), _stream()), "mfx_dcn_nhwc")
    return y


# DCN as "project, then sample" (csrc/dcn_ps.hip): which layers take it.  The projected map holds 9 * Cout values per pixel and is written and read back;
# measured at B = 8 (profiles/r06_dcn_ps.md): it beats the fused gather kernels where that map is <= 18 MB (512 -> 256 @ 12 x 40: 49 -> 39 us,
# 256 -> 64 @ 24 x 80: 30 -> 24 us) and loses from 35 MB up (the projection GEMM is bound by writing the map: 70.8 MB take 33-47 us with this library's
# 1x1 kernel AND with the vendor's GEMM), so the byte limit below keeps it to the two small-map channel-reducing modules.
DCN_PS = [os.environ.get("MFX_DCN_PS", "1") != "0"]      # MFX_DCN_PS=0: every layer on the fused gather kernels (A/B)
DCN_PS_MAX_BYTES = [int(os.environ.get("MFX_DCN_PS_MAX_MB", "24")) << 20]
PROJECT_AS = [os.environ.get("MFX_PROJECT_AS", "1") != "0"]      # the projection on csrc/gemm_as.hip (0: mfx_conv2d_nhwc's 1x1 kernel)


def dcn_ps_applies(x, p: PackedConv):
    B, H, W, C = x.shape
    if p.transient:                                            # training: the projection operand would be re-packed (six launches) every step
        return False
    return (DCN_PS[0] and x.dtype in (torch.bfloat16, torch.float16) and not p.split and p.kh == 3 and p.kw == 3 and p.stride == 1 and p.pad_h == 1
            and p.dil_w == 1 and p.K_pad == 9 * C and C >= 128 and p.Cout == p.Cout_pad and p.Cout in (64, 128, 256)
            and B * H * W * 9 * p.Cout * 2 <= DCN_PS_MAX_BYTES[0])


@on_tensor_device
def dcn_ps(x, offmask, p: PackedConv):
    """DCNv2 + scale/shift + act as two launches: the 1x1 projection of the whole map (dense GEMM), then the bilinear sampling of the projected map."""
    _need_cuda(x, offmask)
    B, H, W, C = x.shape
    pp = dcn_ps_pack(p)
    # measured (profiles/r06_dcn_ps.md, B = 8): the activation-stationary kernel wins where the map is store-bound or wide -- K = 128 (35.9 -> 23.0 us,
    # 63.3 -> 35.1), K = 512 (29.7 -> 26.5), K = 256 with 2304 outputs (47.4 -> 35.0) -- and loses on 256 -> 576 / 1152 (16.6 -> 20.4, 27.4 -> 25.8: a tie)
    if PROJECT_AS[0] and pp.K_pad == C and (C in (128, 512) or (C == 256 and 9 * p.Cout >= 2304)):
        proj = torch.empty((B, H, W, 9 * p.Cout), dtype=x.dtype, device=x.device)      # rows [(tap, n)]
        L.check(L.load().mfx_project_nhwc(_ptr(x), _ptr(pp.w), _ptr(proj), B * H * W, C, 9 * p.Cout, C, 9 * p.Cout, _dt(x.dtype), _stream()), "mfx_project_nhwc")
    else:
        proj = conv2d(x, pp)                                    # the tiled implicit-GEMM kernel
    y = torch.empty((B, H, W, p.Cout), dtype=x.dtype, device=x.device)
    L.check(L.load().mfx_dcn_sample_nhwc(_ptr(proj), _ptr(offmask), _ptr(p.scale), _ptr(p.shift), _ptr(y), B, H, W, p.Cout, p.Cout, p.act,
                                         _dt(x.dtype), _stream()), "mfx_dcn_sample_nhwc")
    return y


@on_tensor_device
def dcn_module(x, p_off: PackedConv, p: PackedConv, need_offmask=False, done=None):
    """The DCN module of the reference (dcn_v2.py:118-128): offset/mask conv (27 -> 32 channels, fp32 out, sigmoid on the mask channels)
    followed by the fused DCNv2.  Where the library's LDS-patch kernel takes the layer (mfx_dcn_fuses_offset_conv: 64 -> 64 on large
    16-bit maps) the offset conv runs INSIDE it -- one launch, the (B,H,W,32) offset map exists only if `need_offmask` (training: the
    backward pass reads it).  -> (y, offmask or None)
    `done`: this module's (y, offmask) where `dcn_module_group` has computed it already with other modules of its shape -- returned as it is,
    nothing is launched: the module is still entered through this function, so whoever wraps it (hooks, the layer-by-layer oracle walk of the
    tests) sees every module's input, output and offset map."""
    _need_cuda(x)
    if done is not None:
        return done
    B, H, W, C = x.shape
    if p.stride == 1 and p.pad_h == 1 and p.kh == 3 and p.kw == 3:
        y = torch.empty((B, H, W, p.Cout), dtype=x.dtype, device=x.device)
        om = torch.empty((B, H, W, 32), dtype=torch.float32, device=x.device) if need_offmask else None
        d = _dcn_desc(x, None, p, y, off=p_off, offmask_out=om)
        if d.off_w_frag_f16 and L.load().mfx_dcn_fuses_offset_conv(ctypes.byref(d)):
            L.check(L.load().mfx_dcn_nhwc(ctypes.byref(d), _stream()), "mfx_dcn_nhwc")
            return y, om
    om = conv2d(x, p_off, out_dtype=torch.float32)
    if dcn_ps_applies(x, p):
        return dcn_ps(x, om, p), om
    return dcn(x, om, p), om


@on_tensor_device
def dcn_module_group(xs, p_offs, ps):
    """The DCN modules (xs[i], p_offs[i], ps[i]) -- independent of each other -- as one grouped offset/mask conv launch and one grouped gather launch
    where the library takes them (mfx_dcn_module_group: 2..4 modules of identical shape on the 16-bit gather kernel; bit-identical to separate
    launches), module by module through `dcn_module` otherwise.  -> ([y_i], [offmask_i or None])"""
    _need_cuda(*xs)
    n = len(xs)
    x0, p0 = xs[0], ps[0]

    def same(a, b):
        return all(getattr(a, f) == getattr(b, f) for f in ("kh", "kw", "stride", "pad_h", "pad_w", "dil_w", "Ck", "Cout", "Cout_pad", "K_pad", "act", "split"))
    ok = (1 <= n <= 4 and x0.dtype in (torch.bfloat16, torch.float16) and not p0.split and p0.stride == 1 and p0.pad_h == 1 and p0.kh == 3 and p0.kw == 3
          and all(x.shape == x0.shape and x.dtype == x0.dtype and x.is_contiguous() for x in xs)
          and all(same(p, p0) for p in ps) and all(same(q, p_offs[0]) for q in p_offs)
          and all(q.w_frag is not None and q.Cout_pad == 32 for q in p_offs)
          and not any(dcn_ps_applies(x, p) for x, p in zip(xs, ps)))          # project-then-sample layers are routed here, not in the library
    if ok:
        B, H, W, C = x0.shape
        offs, dcns = (L.ConvDesc * n)(), (L.DcnDesc * n)()
        ys = [torch.empty((B, H, W, p0.Cout), dtype=x0.dtype, device=x0.device) for _ in range(n)]
        oms = [torch.empty((B, H, W, 32), dtype=torch.float32, device=x0.device) for _ in range(n)]
        for i, (x, q, p) in enumerate(zip(xs, p_offs, ps)):
            d = offs[i]
            d.x, d.w, d.w_frag, d.y = x.data_ptr(), q.w.data_ptr(), q.w_frag.data_ptr(), oms[i].data_ptr()
            d.scale = q.scale.data_ptr() if q.scale is not None else None
            d.shift = q.shift.data_ptr() if q.shift is not None else None
            d.B, d.H, d.W, d.x_pixstride, d.Ck = B, H, W, C, q.Ck
            d.kh, d.kw, d.stride, d.pad_h, d.pad_w, d.dil_w = q.kh, q.kw, q.stride, q.pad_h, q.pad_w, q.dil_w
            d.Ho, d.Wo, d.M, d.Cout, d.Cout_pad, d.K_pad = H, W, B * H * W, q.Cout, q.Cout_pad, q.K_pad
            d.ldy, d.ldres, d.act, d.dtype, d.out_dtype = q.Cout, 0, q.act, _dt(x.dtype), L.MFX_F32
            dd = _dcn_desc(x, oms[i], p, ys[i])
            if B * H * W * p.Cout_pad <= SPLITK_MAX_ELEMS:       # as `dcn` does: a module that would run split-K alone is not grouped
                ws = _splitk_workspace(x.device)
                dd.workspace, dd.workspace_bytes = ws.data_ptr(), ws.numel() * 4
            ctypes.memmove(ctypes.byref(dcns[i]), ctypes.byref(dd), ctypes.sizeof(L.DcnDesc))
        rc = L.load().mfx_dcn_module_group(offs, dcns, n, _stream())
        if rc == 0:
            return ys, oms
        if rc < 0:
            L.check(rc, "mfx_dcn_module_group")
    outs = [dcn_module(x, q, p) for x, q, p in zip(xs, p_offs, ps)]             # not applicable (rc == 1): nothing was launched
    return [o[0] for o in outs], [o[1] for o in outs]


@on_tensor_device
def maxpool2x2(x):
    _need_cuda(x)
    B, H, W, C = x.shape
    y = torch.empty((B, H // 2, W // 2, C), dtype=x.dtype, device=x.device)
    L.check(L.load().mfx_maxpool2x2_nhwc(_ptr(x), _ptr(y), B, H, W, C, _dt(x.dtype), _stream()), "mfx_maxpool2x2_nhwc")
    return y


@on_tensor_device
def upsample_add(x, w_taps, f, skip=None):
    _need_cuda(x, w_taps, skip)
    B, H, W, C = x.shape
    y = torch.empty((B, H * f, W * f, C), dtype=x.dtype, device=x.device)
    L.check(L.load().mfx_upsample_add_nhwc(_ptr(x), _ptr(w_taps), _ptr(skip), _ptr(y), B, H, W, C, f, _dt(x.dtype), _stream()),
            "mfx_upsample_add_nhwc")
    return y


@on_tensor_device
def nchw_to_nhwc(x, dtype, channels=None):
    """fp32 NCHW -> NHWC of `dtype`, channel axis zero-padded to `channels`."""
    _need_cuda(x)
    x = x.float().contiguous()
    B, C, H, W = x.shape
    ld = channels or C
    y = torch.empty((B, H, W, ld), dtype=dtype, device=x.device)
    L.check(L.load().mfx_nchw_to_nhwc(_ptr(x), _ptr(y), B, C, H, W, ld, _dt(dtype), _stream()), "mfx_nchw_to_nhwc")
    return y


@on_tensor_device
def nhwc_to_nchw(x, channels=None):
    _need_cuda(x)
    B, H, W, ld = x.shape
    C = channels or ld
    y = torch.empty((B, C, H, W), dtype=torch.float32, device=x.device)
    L.check(L.load().mfx_nhwc_to_nchw(_ptr(x), _ptr(y), B, C, H, W, ld, _dt(x.dtype), _stream()), "mfx_nhwc_to_nchw")
    return y


@on_tensor_device
def pack_image(images, dtype):
    """(B,3,H,W) fp32 NCHW -> zero-padded NHWC4 (B, H+6, W+8, 4) for the stem conv."""
    _need_cuda(images)
    images = images.float().contiguous()
    dtype = storage_dtype(dtype)
    B, C, H, W = images.shape
    assert C == 3
    y = torch.empty((B, H + 2 * STEM_PAD_H, W + STEM_PAD_WL + STEM_PAD_WR, 4), dtype=dtype, device=images.device)
    L.check(L.load().mfx_pack_image_nhwc4(_ptr(images), _ptr(y), B, H, W, STEM_PAD_H, STEM_PAD_WL, STEM_PAD_WR,
                                          _dt(dtype), _stream()), "mfx_pack_image_nhwc4")
    return y


@on_tensor_device
def stem_conv(images, p: PackedConv):
    """bf16 stem: (B,3,H,W) fp32 NCHW -> (B,H,W,16) bf16 NHWC, conv7x7 + scale/shift + act in one kernel."""
    _need_cuda(images)
    images = images.float().contiguous()
    B, C, H, W = images.shape
    assert C == 3 and p.w.dtype in (torch.bfloat16, torch.float16) and p.Cout == 16
    y = torch.empty((B, H, W, 16), dtype=torch.float32 if p.split else p.w.dtype, device=images.device)
    L.check(L.load().mfx_stem_conv7x7_nchw(_ptr(images), _ptr(p.w), _ptr(p.scale), _ptr(p.shift), _ptr(y), B, H, W, 16, p.K_pad, p.act,
                                           L.MFX_F16X2 if p.split else _dt(p.w.dtype), _stream()), "mfx_stem_conv7x7_nchw")
    return y


@on_tensor_device
def f1_fused(images, p_stem: PackedConv, p_l0: PackedConv, p_l1: PackedConv):
    """(B,3,H,W) fp32 NCHW -> level1 map (B,H/2,W/2,32): stem + level0 + level1 (each conv + folded BN + ReLU) in one kernel (csrc/f1_fused.hip);
    the packs are the ones the three separate launches use (pack_stem, pack_conv)."""
    _need_cuda(images)
    images = images.float().contiguous()
    B, C, H, W = images.shape
    split = p_stem.split                                            # split precision: fp32 map out, (hi, lo) fp16 operand pairs
    dt = torch.float32 if split else p_stem.w.dtype
    assert C == 3 and (split or dt in (torch.bfloat16, torch.float16)) and p_stem.Cout == 16 and p_l0.Cout == 16 and p_l1.Cout == 32 and p_l1.stride == 2
    assert p_l0.split == split and p_l1.split == split
    for p in (p_l0, p_l1):                                          # [Cout][160] slice of the K-padded (tap, channel) matrix, cached on the pack
        if p.f1_w160 is None:
            assert p.K_pad >= 160 and p.Ck == 16
            p.f1_w160 = p.w[:, :160].contiguous()
    y = torch.empty((B, H // 2, W // 2, 32), dtype=dt, device=images.device)
    L.check(L.load().mfx_f1_fused(_ptr(images), _ptr(p_stem.w), _ptr(p_stem.scale), _ptr(p_stem.shift),
                                  _ptr(p_l0.f1_w160), _ptr(p_l0.scale), _ptr(p_l0.shift),
                                  _ptr(p_l1.f1_w160), _ptr(p_l1.scale), _ptr(p_l1.shift),
                                  _ptr(y), B, H, W, p_stem.K_pad, L.MFX_F16X2 if split else _dt(dt), _stream()), "mfx_f1_fused")
    return y


@on_tensor_device
def heads_fused(x, p: PackedHeads, planar_classes=0):
    """-> (head map fp32 (B,H,W,ld_out), class-planar logits (B,planar_classes,H*W) or None)."""
    _need_cuda(x)
    B, H, W, C = x.shape
    assert C == 64
    out = torch.empty((B, H, W, p.ld_out), dtype=torch.float32, device=x.device)
    planar = torch.empty((B, planar_classes, H * W), dtype=torch.float32, device=x.device) if planar_classes else None
    d = L.HeadsDesc()
    d.planar, d.planar_c = (planar.data_ptr() if planar is not None else None), planar_classes
    d.x, d.w1, d.scale1, d.shift1 = x.data_ptr(), p.w1.data_ptr(), p.scale1.data_ptr(), p.shift1.data_ptr()
    d.w2, d.bias2, d.out = p.w2.data_ptr(), p.bias2.data_ptr(), out.data_ptr()
    d.w1_32 = p.w1_32.data_ptr() if p.w1_32 is not None else None
    d.w2_32 = p.w2_32.data_ptr() if p.w2_32 is not None else None
    d.B, d.H, d.W, d.nbranch, d.K_pad, d.ld_out = B, H, W, len(p.c_out), p.K_pad, p.ld_out
    d.dtype = L.MFX_F16X2 if p.split else _dt(x.dtype)
    for i, (o, c) in enumerate(zip(p.ch_off, p.c_out)):
        d.ch_off[i], d.c_out[i] = o, c
        d.w2_scale[i] = p.w2_scale[i] if p.w2_scale is not None else 1.0
    L.check(L.load().mfx_heads_fused_act(ctypes.byref(d), p.act, _stream()), "mfx_heads_fused_act")
    return out, planar


@on_tensor_device
def edge_chain(x, edge_xy, p: PackedEdgeChain):
    """The edge fusion's conv chain in one kernel: x (B,H,W,64) 16-bit, edge_xy int32 (B,L,2) -> fp32 (2,B,L,4), [0] the class branch's and [1]
    the 3d_offset branch's Conv1d output at every sequence position (what edge_scatter_add adds to the head map).  None where the library keeps
    the five conv launches (option "edge_chain" off, or not a 16-bit map): the caller runs those.  A k = 3 pack goes through mfx_edge_chain_applies /
    mfx_edge_chain_act, the other windows (p.ksize 1, 5, 7) through mfx_edge_chain_ks_applies / mfx_edge_chain_ks."""
    _need_cuda(x, edge_xy)
    B, H, W, C = x.shape
    Lmax = edge_xy.shape[1]
    if edge_xy.dtype != torch.int32 or not edge_xy.is_contiguous() or not x.is_contiguous() or x.dtype != p.w_trunk.dtype:
        return None
    d = L.EdgeChainDesc()
    d.x, d.edge_xy = x.data_ptr(), edge_xy.data_ptr()
    d.w_trunk, d.scale_trunk, d.shift_trunk = p.w_trunk.data_ptr(), p.scale_trunk.data_ptr(), p.shift_trunk.data_ptr()
    d.w_conv, d.scale_conv, d.shift_conv = p.w_conv.data_ptr(), p.scale_conv.data_ptr(), p.shift_conv.data_ptr()
    d.w_out, d.bias_out = p.w_out.data_ptr(), p.bias_out.data_ptr()
    d.B, d.H, d.W, d.C, d.L, d.head_conv, d.ksize, d.relu, d.dtype = B, H, W, C, Lmax, 256, p.ksize, int(p.relu), _dt(x.dtype)
    lib = L.load()
    applies, run, name = (lib.mfx_edge_chain_applies, lib.mfx_edge_chain_act, "mfx_edge_chain_act") if p.ksize == 3 else \
        (lib.mfx_edge_chain_ks_applies, lib.mfx_edge_chain_ks, "mfx_edge_chain_ks")
    if not applies(ctypes.byref(d)):
        return None
    out = torch.empty((2, B, Lmax, 4), dtype=torch.float32, device=x.device)
    d.out = out.data_ptr()
    L.check(run(ctypes.byref(d), p.act_trunk, _stream()), name)
    return out


@on_tensor_device
def edge_scatter_add(out, ch_off, C, v, edge_xy, edge_len, planar=None):
    _need_cuda(out, v, edge_xy, edge_len, planar)
    B, H, W, ld = out.shape
    Lmax = edge_xy.shape[1]
    L.check(L.load().mfx_edge_scatter_add(_ptr(out), ld, ch_off, C, _ptr(v), v.shape[-1], _ptr(edge_xy), _ptr(edge_len),
                                          B, Lmax, H, W, _ptr(planar), _stream()), "mfx_edge_scatter_add")


@on_tensor_device
def decode_topk(hmap, ch_off, ncls, K, planar=None):
    """Per-(image,class) NMS + top-K.  Reads the class-planar logits when given (coalesced), else the NHWC map."""
    _need_cuda(hmap, planar)
    B, H, W, ld = hmap.shape
    scores = torch.empty((B, ncls, K), dtype=torch.float32, device=hmap.device)
    index = torch.empty((B, ncls, K), dtype=torch.int32, device=hmap.device)
    if planar is not None:
        src, bs, cs, ps = planar.data_ptr(), ncls * H * W, H * W, 1
    else:
        src, bs, cs, ps = hmap.data_ptr() + 4 * ch_off, H * W * ld, 1, ld
    lib = L.load()
    ws = torch.empty(int(lib.mfx_decode_topk_workspace_bytes(ncls, B, K)), dtype=torch.uint8, device=hmap.device)
    L.check(lib.mfx_decode_topk(ctypes.c_void_p(src), bs, cs, ps, ncls, B, H, W, K, _ptr(scores), _ptr(index), _ptr(ws), ws.numel(),
                                _stream()), "mfx_decode_topk")
    return scores, index


@on_tensor_device
def decode_boxes(hmap, reg_off, scores, index, calib, pad, img_size, threshold, depth_mode="soft", cfg=None, return_unc=False, heads=None):
    """`depth_mode`: the reference's `output_depth` name (lib.DEPTH_MODES; 'oracle' needs ground truth and is not a decode mode).
    `cfg`: a lib.DecodeCfg (lib.decode_cfg) with the head settings the model was trained with; None is the runs/monoflex.yaml decode
    (mfx_decode_boxes_mode).  `depth_mode` overrides the cfg's own output_depth.  `return_unc` (needs a cfg) appends
    unc (B,K,2) = [estimated_depth_error, uncertainty_conf], zeros when the cfg's uncertainty_as_conf is off.
    `heads` (needs a cfg): a lib.HeadLayout (lib.HeadSet.layout()) for a head set other than the nine-key one of runs/monoflex.yaml
    (mfx_decode_boxes_heads); unc is zero too where the set has no uncertainty head for the chosen depth."""
    _need_cuda(hmap, scores, index, calib, pad, img_size)
    if depth_mode not in L.DEPTH_MODES:
        raise ValueError("decode_boxes: output_depth %r is not one of %s" % (depth_mode, sorted(L.DEPTH_MODES)))
    if (return_unc or heads is not None) and cfg is None:
        raise ValueError("decode_boxes: return_unc / heads need a cfg (lib.decode_cfg)")
    B, H, W, ld = hmap.shape
    ncls, K = scores.shape[1], scores.shape[2]
    det = torch.empty((B, K, 14), dtype=torch.float32, device=hmap.device)
    topk = torch.empty((B, K, 5), dtype=torch.float32, device=hmap.device)
    valid = torch.empty((B, K), dtype=torch.int32, device=hmap.device)
    if cfg is None:
        L.check(L.load().mfx_decode_boxes_mode(_ptr(hmap), ld, reg_off, _ptr(scores), _ptr(index), ncls, B, H, W, K, _ptr(calib),
                                               _ptr(pad), _ptr(img_size), ctypes.c_float(threshold), L.DEPTH_MODES[depth_mode], _ptr(det), _ptr(topk),
                                               _ptr(valid), _stream()), "mfx_decode_boxes_mode")
        return det, topk, valid
    c = L.DecodeCfg.from_buffer_copy(cfg)                       # (the caller's struct keeps its own output_depth)
    c.output_depth = L.DEPTH_MODES[depth_mode]
    unc = torch.empty((B, K, 2), dtype=torch.float32, device=hmap.device) if return_unc else None
    if heads is not None:
        L.check(L.load().mfx_decode_boxes_heads(_ptr(hmap), ld, reg_off, _ptr(scores), _ptr(index), ncls, B, H, W, K, _ptr(calib),
                                                _ptr(pad), _ptr(img_size), ctypes.c_float(threshold), ctypes.byref(c), ctypes.byref(heads),
                                                _ptr(det), _ptr(topk), _ptr(valid), _ptr(unc), _stream()), "mfx_decode_boxes_heads")
        return (det, topk, valid, unc) if return_unc else (det, topk, valid)
    L.check(L.load().mfx_decode_boxes_cfg(_ptr(hmap), ld, reg_off, _ptr(scores), _ptr(index), ncls, B, H, W, K, _ptr(calib),
                                          _ptr(pad), _ptr(img_size), ctypes.c_float(threshold), ctypes.byref(c), _ptr(det), _ptr(topk),
                                          _ptr(valid), _ptr(unc), _stream()), "mfx_decode_boxes_cfg")
    return (det, topk, valid, unc) if return_unc else (det, topk, valid)


ORACLE_GT_FIELDS = ("reg_mask", "cls_ids", "gt_bboxes", "locations")
ORACLE_GT_ROW = 8


def oracle_gt_rows(source, device):
    """The ground-truth table OUTPUT_DEPTH 'oracle' matches against (mfx_decode_boxes_multi), fp32 (B, M, 8) on `device`: reg_mask, cls_id,
    2D box x1, y1, x2, y2, depth (locations[..., 2]), one spare.  `source`: the loader's batch-stacked `fields` dict, or the per-image
    ParamsLists (stacked here).  Targets without the ground-truth fields (the `test` split) raise ValueError."""
    if isinstance(source, dict):
        missing = [k for k in ORACLE_GT_FIELDS if k not in source]
        get = lambda k: torch.as_tensor(source[k])
    else:
        source = list(source)
        missing = [k for k in ORACLE_GT_FIELDS if not all(t.has_field(k) for t in source)]
        get = lambda k: torch.stack([torch.as_tensor(t.get_field(k)) for t in source])
    if missing:
        raise ValueError("OUTPUT_DEPTH 'oracle' reads the ground truth of every image, and these targets have no %s "
                         "(the `test` split has no labels: evaluate a split that has)" % ", ".join(missing))
    mask = get("reg_mask")
    B, M = mask.shape[:2]
    f = lambda k, w: get(k).to(device=device, dtype=torch.float32).reshape(B, M, w)
    rows = torch.zeros((B, M, ORACLE_GT_ROW), dtype=torch.float32, device=device)
    rows[:, :, 0:1] = f("reg_mask", 1)
    rows[:, :, 1:2] = f("cls_ids", 1)
    rows[:, :, 2:6] = f("gt_bboxes", 4)
    rows[:, :, 6] = f("locations", 3)[:, :, 2]
    return rows


@on_tensor_device
def decode_boxes_multi(hmap, reg_off, scores, index, calib, pad, img_size, threshold, modes, cfg, heads=None, gt_rows=None, return_unc=False):
    """Several depth modes of decode_boxes, and the reference's 'oracle', from ONE launch on one top-K (mfx_decode_boxes_multi).
    `modes`: a sequence of distinct names from lib.DEPTH_MODES plus 'oracle'; `cfg`: a lib.DecodeCfg (its own output_depth is not read);
    `heads`: a lib.HeadLayout, None = the nine-key layout of runs/monoflex.yaml; `gt_rows` (B, M, 8) fp32 (oracle_gt_rows): required with
    'oracle', M <= 128.  -> (det (B, NM, K, 14), topk (B, K, 5), valid (B, K), unc (B, NM, K, 2) or None, choice (B, K) int32 or None):
    slice i is `modes[i]`, bit for bit the row decode_boxes(depth_mode=modes[i]) writes; an oracle row is the row of the single-estimate mode
    the detection took, or the 'mean' row; choice = -1 (kept the mean) or the column 0..3 (0 = direct), only with 'oracle'.
    No host synchronisation."""
    _need_cuda(hmap, scores, index, calib, pad, img_size, gt_rows)
    modes = list(modes)
    bad = [m for m in modes if m not in L.DEPTH_MODES and m != 'oracle']
    if bad or len(set(modes)) != len(modes):
        raise ValueError("decode_boxes_multi: modes %r must be distinct names of %s or 'oracle'" % (modes, sorted(L.DEPTH_MODES)))
    if cfg is None:
        raise ValueError("decode_boxes_multi: needs a cfg (lib.decode_cfg)")
    if heads is None:
        heads = L.HeadSet([L.HEAD_KEYS], [[L.HEAD_WIDTHS[k] for k in L.HEAD_KEYS]]).layout()
    bit = lambda m: L.DEPTH_ORACLE if m == 'oracle' else L.DEPTH_MODES[m]
    mask = 0
    for m in modes:
        mask |= 1 << bit(m)
    B, H, W, ld = hmap.shape
    ncls, K = scores.shape[1], scores.shape[2]
    NM = len(modes)
    oracle = 'oracle' in modes
    M = 0
    if gt_rows is not None:
        if gt_rows.dtype != torch.float32 or gt_rows.dim() != 3 or gt_rows.shape[0] != B or gt_rows.shape[2] != ORACLE_GT_ROW or not gt_rows.is_contiguous():
            raise RuntimeError("decode_boxes_multi: gt_rows is a contiguous float32 (B, M, 8) table (oracle_gt_rows), got %s %s"
                               % (gt_rows.dtype, tuple(gt_rows.shape)))
        M = gt_rows.shape[1]
    dev = hmap.device
    det = torch.empty((B, NM, K, 14), dtype=torch.float32, device=dev)
    topk = torch.empty((B, K, 5), dtype=torch.float32, device=dev)
    valid = torch.empty((B, K), dtype=torch.int32, device=dev)
    unc = torch.empty((B, NM, K, 2), dtype=torch.float32, device=dev) if return_unc else None
    choice = torch.empty((B, K), dtype=torch.int32, device=dev) if oracle else None
    L.check(L.load().mfx_decode_boxes_multi(_ptr(hmap), ld, reg_off, _ptr(scores), _ptr(index), ncls, B, H, W, K, _ptr(calib), _ptr(pad),
                                            _ptr(img_size), ctypes.c_float(threshold), ctypes.byref(cfg), ctypes.byref(heads), mask,
                                            _ptr(gt_rows) if oracle else None, M, _ptr(det), _ptr(topk), _ptr(valid), _ptr(unc), _ptr(choice),
                                            _stream()), "mfx_decode_boxes_multi")
    # the kernel writes the slices in ascending bit order: hand them back in the order asked for
    order = sorted(range(NM), key=lambda i: bit(modes[i]))                 # order[s] = position in `modes` of slice s
    if order != list(range(NM)):
        where = {i: s for s, i in enumerate(order)}                        # where[i] = slice of modes[i]
        pick = lambda t: torch.stack([t[:, where[i]] for i in range(NM)], dim=1)       # (one device copy, no index tensor from the host)
        det, unc = pick(det), None if unc is None else pick(unc)
    return det, topk, valid, unc, choice


# ---- reference `_ext` boundary (NCHW fp32) ---------------------------------------------------------
_ws_cache = {}


SPLITK_MAX_ELEMS = 4 * 1024 * 1024          # output elements (M * Cout_pad) up to which split-K is offered
_splitk_ws = {}


def _splitk_workspace(device):
    """One persistent fp32 scratch per device (9 splits x SPLITK_MAX_ELEMS): stable address, so captured graphs stay valid;
    launches on one stream are ordered, so consecutive layers can share it."""
    if torch.cuda.is_current_stream_capturing():
        # inside a hipGraph capture the scratch must come from THAT graph's memory pool and live exactly as long as the ops
        # that use it (an entry cached from an earlier capture would belong to another graph's pool): allocate per call, the
        # pool reuses the block for the next layer in stream order, which replays faithfully
        return torch.empty(9 * SPLITK_MAX_ELEMS, dtype=torch.float32, device=device)
    key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream)      # concurrent streams must not share it
    if key not in _splitk_ws:
        _splitk_ws[key] = torch.empty(9 * SPLITK_MAX_ELEMS, dtype=torch.float32, device=device)
    return _splitk_ws[key]


def _workspace(nbytes, device):
    if torch.cuda.is_current_stream_capturing():                # see _splitk_workspace
        return torch.empty(int(nbytes), dtype=torch.uint8, device=device)
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        _ws_cache[key] = ws
    return ws


def _ext_check(x, w, off, msk, kh, kw, dg):
    """The reference's argument checks (src/cuda/dcn_v2_cuda.cu:60-84, dcn_v2.py:84-87) with its messages, as RuntimeError."""
    C = x.shape[1]
    if w.shape[2] != kh or w.shape[3] != kw:
        raise RuntimeError("Input shape and kernel shape wont match: (%d x %d vs %d x %d)." % (kh, kw, w.shape[2], w.shape[3]))
    if w.shape[1] != C:
        raise RuntimeError("Input shape and kernel channels wont match: (%d vs %d)." % (C, w.shape[1]))
    if dg < 1 or C % dg != 0:
        raise RuntimeError("dcn_v2: %d input channels cannot be split into %d deformable groups" % (C, dg))
    if off.shape[1] != 2 * dg * kh * kw or msk.shape[1] != dg * kh * kw:
        raise RuntimeError("dcn_v2: offset / mask must have 2*dg*kh*kw = %d / dg*kh*kw = %d channels (got %d / %d)"
                           % (2 * dg * kh * kw, dg * kh * kw, off.shape[1], msk.shape[1]))


@on_tensor_device
def ext_dcn_v2_forward(input, weight, bias, offset, mask, kh, kw, sh, sw, ph, pw, dh, dw, dg):
    """`_ext.dcn_v2_forward` (src/dcn_v2.h:9-23): NCHW fp32 in and out; ONE call of the C entry, which is as general as the reference's:
    deformable groups (its own example uses 2, testcuda.py:169-180) are looped inside `mfx_dcn_v2_forward` (group g = channel slice g with its
    own 2*kh*kw offset and kh*kw mask channels, dcn_v2_im2col_cuda.cu:147-156), stride / padding / dilation are per axis."""
    _need_cuda(input, weight, bias, offset, mask)
    ts = [t.float().contiguous() for t in (input, weight, bias, offset, mask)]
    x, w, b, off, msk = ts
    _ext_check(x, w, off, msk, kh, kw, dg)
    B, C, H, W = x.shape
    Cout = w.shape[0]
    Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1
    Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
    lib_ = L.load()
    nbytes = lib_.mfx_dcn_v2_workspace_bytes_g(B, C, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, dg, 0)
    ws = _workspace(nbytes, x.device)
    out = torch.empty((B, Cout, Ho, Wo), dtype=torch.float32, device=x.device)
    L.check(lib_.mfx_dcn_v2_forward(_ptr(x), _ptr(w), _ptr(b), _ptr(off), _ptr(msk), _ptr(out), B, C, H, W, Cout, kh, kw,
                                    sh, sw, ph, pw, dh, dw, dg, _ptr(ws), ws.numel(), _stream()), "mfx_dcn_v2_forward")
    return out


@on_tensor_device
def ext_dcn_v2_backward(input, weight, bias, offset, mask, grad_output, kh, kw, sh, sw, ph, pw, dh, dw, dg):
    """`_ext.dcn_v2_backward` (src/dcn_v2.h:48-59) -> [grad_input, grad_offset, grad_mask, grad_weight, grad_bias]; deformable
    groups and per-axis geometry inside the C entry, as in the forward."""
    _need_cuda(input, weight, bias, offset, mask, grad_output)
    x, w, b, off, msk, go = [t.float().contiguous() for t in (input, weight, bias, offset, mask, grad_output)]
    _ext_check(x, w, off, msk, kh, kw, dg)
    B, C, H, W = x.shape
    Cout = w.shape[0]
    lib_ = L.load()
    nbytes = lib_.mfx_dcn_v2_workspace_bytes_g(B, C, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, dg, 1)
    ws = _workspace(nbytes, x.device)
    gi, gw, gb = torch.empty_like(x), torch.empty_like(w), torch.empty_like(b)
    goff, gm = torch.empty_like(off), torch.empty_like(msk)
    L.check(lib_.mfx_dcn_v2_backward(_ptr(x), _ptr(w), _ptr(b), _ptr(off), _ptr(msk), _ptr(go), _ptr(gi), _ptr(goff), _ptr(gm),
                                     _ptr(gw), _ptr(gb), B, C, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, dg,
                                     _ptr(ws), ws.numel(), _stream()), "mfx_dcn_v2_backward")
    return [gi, goff, gm, gw, gb]


def _psroi_operands(input, rois, offset, no_trans, output_dim, part_size):
    """Contiguous fp32 operands and the sizes both pooling entries take; `offset` may be an empty tensor when `no_trans` (dcn_v2.py:211)."""
    _need_cuda(input, rois, offset)
    x, r = input.float().contiguous(), rois.float().contiguous()
    if x.dim() != 4:
        raise RuntimeError("dcn_v2_psroi_pooling: input must be (B, C, H, W), got %s" % (tuple(x.shape),))
    if r.dim() != 2 or r.shape[1] != 5:
        raise RuntimeError("dcn_v2_psroi_pooling: rois must be (N, 5) rows of (batch_index, x1, y1, x2, y2), got %s" % (tuple(r.shape),))
    if x.shape[1] != output_dim:
        raise RuntimeError("dcn_v2_psroi_pooling: input channels and output channels must equal (got %d channels, output_dim %d)"
                           % (x.shape[1], output_dim))
    if no_trans:
        return x, r, None, 0, 2
    t = offset.float().contiguous()
    if t.dim() != 4 or t.shape[0] < r.shape[0] or t.shape[1] < 2 or t.shape[1] % 2 or t.shape[2] != part_size or t.shape[3] != part_size:
        raise RuntimeError("dcn_v2_psroi_pooling: offset must be (>= %d rois, 2 * num_classes, part_size = %d, part_size), got %s"
                           % (r.shape[0], part_size, tuple(t.shape)))
    return x, r, t, t.shape[0], t.shape[1]


@on_tensor_device
def ext_dcn_v2_psroi_pooling_forward(input, rois, offset, no_trans, spatial_scale, output_dim, group_size, pooled_size, part_size,
                                     sample_per_part, trans_std):
    """`_ext.dcn_v2_psroi_pooling_forward` (src/dcn_v2.h:94-138) -> (output, output_count), both (N, output_dim, pooled, pooled) fp32."""
    no_trans = int(no_trans)
    x, r, t, trans_rois, trans_ch = _psroi_operands(input, rois, offset, no_trans, output_dim, part_size)
    B, C, H, W = x.shape
    N = r.shape[0]
    out = torch.empty((N, output_dim, pooled_size, pooled_size), dtype=torch.float32, device=x.device)
    count = torch.empty_like(out)
    L.check(L.load().mfx_dcn_v2_psroi_pooling_forward(_ptr(x), _ptr(r), _ptr(t), _ptr(out), _ptr(count), B, C, H, W, N, trans_rois, trans_ch,
                                                      no_trans, spatial_scale, output_dim, group_size, pooled_size, part_size,
                                                      sample_per_part, trans_std, _stream()), "mfx_dcn_v2_psroi_pooling_forward")
    return out, count


@on_tensor_device
def ext_dcn_v2_psroi_pooling_backward(grad_output, input, rois, offset, output_count, no_trans, spatial_scale, output_dim, group_size,
                                      pooled_size, part_size, sample_per_part, trans_std):
    """`_ext.dcn_v2_psroi_pooling_backward` (src/dcn_v2.h:140-190) -> (grad_input, grad_offset); grad_offset has the shape of `offset`
    (the empty tensor's when `no_trans`)."""
    no_trans = int(no_trans)
    _need_cuda(grad_output, output_count)
    x, r, t, trans_rois, trans_ch = _psroi_operands(input, rois, offset, no_trans, output_dim, part_size)
    B, C, H, W = x.shape
    N = r.shape[0]
    go, cnt = grad_output.float().contiguous(), output_count.float().contiguous()
    want = (N, output_dim, pooled_size, pooled_size)
    if tuple(go.shape) != want or tuple(cnt.shape) != want:
        raise RuntimeError("dcn_v2_psroi_pooling_backward: grad_output / output_count must be %s, got %s / %s"
                           % (want, tuple(go.shape), tuple(cnt.shape)))
    gi = torch.empty_like(x)
    goff = torch.empty_like(t) if t is not None else torch.zeros_like(offset, dtype=torch.float32)
    L.check(L.load().mfx_dcn_v2_psroi_pooling_backward(_ptr(go), _ptr(x), _ptr(r), _ptr(t), _ptr(cnt), _ptr(gi), _ptr(goff) if t is not None else None,
                                                       B, C, H, W, N, trans_rois, trans_ch, no_trans, spatial_scale, output_dim, group_size,
                                                       pooled_size, part_size, sample_per_part, trans_std, _stream()),
            "mfx_dcn_v2_psroi_pooling_backward")
    return gi, goff


@on_tensor_device
def box3d_iou(a, b):
    """Rotated 3D box IoU of N matched pairs (mfx_box3d_iou_pairs; reference get_iou_3d, model/layers/iou_loss.py:99-136) -> (N,) fp32.
    `a`, `b`: both (N, 7) rows (x, y, z, l, h, w, ry) with y the box centre, or both (N, 8, 3) corner tables in encode_box3d order.
    One launch on the current stream, no host synchronisation."""
    _need_cuda(a, b)
    if a.shape != b.shape or not ((a.dim() == 2 and a.shape[1] == 7) or (a.dim() == 3 and tuple(a.shape[1:]) == (8, 3))):
        raise RuntimeError("box3d_iou: both operands must be (N, 7) box rows or (N, 8, 3) corner tables, got %s and %s"
                           % (tuple(a.shape), tuple(b.shape)))
    x, y = a.detach().float().contiguous(), b.detach().float().contiguous()
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    L.check(L.load().mfx_box3d_iou_pairs(_ptr(x), _ptr(y), x.shape[0], 0 if x.dim() == 2 else 1, _ptr(out), _stream()), "mfx_box3d_iou_pairs")
    return out


@on_tensor_device
def box_nms(det, valid, kind, thresh, class_agnostic=False):
    """Greedy suppression of duplicate detections per image (mfx_box_nms; TEST.USE_NMS '2d' / '3d', which the reference declares and never
    reads: the semantics are in INTEGRATION.md).  det (B, K, 14) fp32 rows of decode_boxes, valid (B, K) int32, kind '2d' | '3d',
    thresh in [0, 1) -> valid_out (B, K) int32 = valid & kept; det is not touched.  Rows are ranked by score (column 13) descending, ties to
    the lower slot; a row is kept unless an already kept row (of its class, unless class_agnostic) overlaps it with IoU > thresh.
    CUDA tensors: one launch on the current stream, no host synchronisation, K <= 128.  CPU tensors: a float64 restatement on the host."""
    if kind not in L.NMS_KINDS:
        raise ValueError("box_nms: kind %r is not one of %s" % (kind, sorted(L.NMS_KINDS)))
    if not 0.0 <= float(thresh) < 1.0:
        raise ValueError("box_nms: thresh %r is outside [0, 1)" % (thresh,))
    if det.dim() != 3 or det.shape[2] != 14 or tuple(valid.shape) != tuple(det.shape[:2]):
        raise RuntimeError("box_nms: det (B, K, 14) and valid (B, K), got %s and %s" % (tuple(det.shape), tuple(valid.shape)))
    if det.dtype != torch.float32 or valid.dtype != torch.int32:
        raise TypeError("box_nms: det is float32 and valid is int32")
    if not det.is_cuda and not valid.is_cuda:
        return _box_nms_host(det, valid, kind, float(thresh), bool(class_agnostic))
    _need_cuda(det, valid)
    B, K = valid.shape
    x, v = det.detach().contiguous(), valid.contiguous()
    out = torch.empty_like(v)
    L.check(L.load().mfx_box_nms(_ptr(x), _ptr(v), B, K, L.NMS_KINDS[kind], ctypes.c_float(float(thresh)), int(bool(class_agnostic)), _ptr(out),
                                 _stream()), "mfx_box_nms")
    return out


def _box_nms_host(det, valid, kind, thresh, class_agnostic):
    """box_nms on CPU tensors: the pairwise IoU matrix of an image in float64 (2D: vectorised; 3D: the host form of get_iou_3d on corner
    tables, kept in float64), the ranking by a stable sort, the walk over it."""
    import numpy as np
    from .model.layers.iou_loss import _iou_3d_host
    B, K = valid.shape
    d = det.detach().double()
    out = torch.zeros_like(valid)
    for b in range(B):
        idx = torch.nonzero(valid[b] != 0).flatten()
        n = idx.numel()
        if n == 0:
            continue
        r = d[b, idx]
        if kind == '2d':
            x1, y1, x2, y2 = (r[:, c] for c in (2, 3, 4, 5))
            iw = (torch.minimum(x2[:, None], x2[None]) - torch.maximum(x1[:, None], x1[None])).clamp(min=0)
            ih = (torch.minimum(y2[:, None], y2[None]) - torch.maximum(y1[:, None], y1[None])).clamp(min=0)
            area = (x2 - x1) * (y2 - y1)
            iou = iw * ih / (area[:, None] + area[None] - iw * ih)                       # 0 / 0 = NaN: not > thresh
        else:
            i, j = torch.triu_indices(n, n, 1)
            # only pairs that can meet are evaluated: rectangles whose circumscribed circles do not touch share no area (IoU 0)
            reach = 0.5 * torch.hypot(r[:, 8], r[:, 7])
            can = torch.hypot(r[i, 9] - r[j, 9], r[i, 11] - r[j, 11]) <= reach[i] + reach[j]
            can |= ~torch.isfinite(r[i].sum(1) + r[j].sum(1))
            if not class_agnostic:
                can &= r[i, 0] == r[j, 0]
            i, j = i[can], j[can]
            iou = torch.zeros((n, n), dtype=torch.float64)
            if i.numel():
                corners = _corner_tables(r)
                iou[i, j] = torch.from_numpy(_iou_3d_host(corners[i].numpy(), corners[j].numpy()))
                iou = iou + iou.T
        over = (iou > thresh).numpy()
        if not class_agnostic:
            over &= (r[:, 0][:, None] == r[:, 0][None]).numpy()
        score = r[:, 13].numpy()
        order = np.argsort(-np.where(np.isnan(score), -np.inf, score), kind="stable")    # ties: the lower slot (idx ascends)
        kept = np.zeros(n, dtype=bool)
        for c in order:
            if not (over[c] & kept).any():
                kept[c] = True
        out[b, idx[torch.from_numpy(kept)]] = 1
    return out


def _corner_tables(rows):
    """det rows (n, 14) float64 -> (n, 8, 3) corner tables in encode_box3d order of the boxes (x, y - h / 2, z, l, h, w, ry)."""
    sx = rows.new_tensor([-1, -1, 1, 1, -1, -1, 1, 1]) * 0.5
    sy = rows.new_tensor([1, 1, 1, 1, -1, -1, -1, -1]) * 0.5
    sz = rows.new_tensor([-1, 1, 1, -1, -1, 1, 1, -1]) * 0.5
    h, w, l, x, y, z, ry = (rows[:, c:c + 1] for c in (6, 7, 8, 9, 10, 11, 12))
    c, s = torch.cos(ry), torch.sin(ry)
    px, py, pz = l * sx, h * sy, w * sz
    return torch.stack((c * px + s * pz + x, py + (y - h / 2), -s * px + c * pz + z), dim=2)


# ---- validation diagnostics at the ground-truth centres (TEST.EVAL_DEPTH / TEST.EVAL_DIS_IOUS) ------------------------------------------
EVAL_DEPTH_KEYS = ("direct", "direct_sigma", "keypoint_center", "keypoint_02", "keypoint_13", "keypoint_center_sigma", "keypoint_02_sigma",
                   "keypoint_13_sigma", "sigma_min", "sigma_weighted", "mean", "min", "target")       # detector_infer.py:341-357, mfx_eval_diagnostics' columns
EVAL_IOU_KEYS = ("pred_IoU", "offset_IoU", "depth_IoU", "dims_IoU", "orien_IoU")                       # detector_infer.py:450
EVAL_GT_FIELDS = ("reg_mask", "cls_ids", "target_centers", "offset_3D", "locations", "dimensions", "rotys")
EVAL_GT_ROW = 16


def eval_diag_rows(source, device):
    """The ground-truth table of mfx_eval_diagnostics, fp32 (B, M, 16) on `device`: reg_mask, cls_id, cx, cy, offset_3D x, y, location X, Y, Z,
    dimensions l, h, w, roty, three spare.  `source`: the loader's batch-stacked `fields` dict, or the per-image ParamsLists (stacked here).
    Targets without the ground-truth fields (the `test` split) raise ValueError."""
    if isinstance(source, dict):
        missing = [k for k in EVAL_GT_FIELDS if k not in source]
        get = lambda k: torch.as_tensor(source[k])
    else:
        source = list(source)
        missing = [k for k in EVAL_GT_FIELDS if not all(t.has_field(k) for t in source)]
        get = lambda k: torch.stack([torch.as_tensor(t.get_field(k)) for t in source])
    if missing:
        raise ValueError("TEST.EVAL_DEPTH / TEST.EVAL_DIS_IOUS read the ground truth of every image, and these targets have no %s "
                         "(the `test` split has no labels: evaluate a split that has)" % ", ".join(missing))
    mask = get("reg_mask")
    B, M = mask.shape[:2]
    f = lambda k, w: get(k).to(device=device, dtype=torch.float32).reshape(B, M, w)
    rows = torch.zeros((B, M, EVAL_GT_ROW), dtype=torch.float32, device=device)
    col = 0
    for k, w in (("reg_mask", 1), ("cls_ids", 1), ("target_centers", 2), ("offset_3D", 2), ("locations", 3), ("dimensions", 3), ("rotys", 1)):
        rows[:, :, col:col + w] = f(k, w)
        col += w
    return rows


@on_tensor_device
def eval_diagnostics(hmap, reg_off, gt_rows, calib, pad, cfg, heads, want=3, return_boxes=False):
    """mfx_eval_diagnostics: the reference's evaluate_3D_depths / evaluate_3D_detection at every object slot of `gt_rows` (eval_diag_rows).
    hmap fp32 (B, H, W, ld); cfg / heads: lib.DecodeCfg (its output_depth decides the predicted depth of the boxes) / lib.HeadLayout.
    -> (depth_err (B, M, 13) or None, iou (B, M, 5) or None[, boxes (B, M, 6, 7)]), columns EVAL_DEPTH_KEYS / EVAL_IOU_KEYS, zeros in the
    slots whose reg_mask is 0.  One launch on the current stream, no host synchronisation, fixed shapes."""
    _need_cuda(hmap, gt_rows, calib, pad)
    if hmap.dtype != torch.float32 or gt_rows.dtype != torch.float32 or calib.dtype != torch.float32 or pad.dtype != torch.int32:
        raise TypeError("eval_diagnostics: hmap, gt_rows and calib are float32, pad is int32")
    B, H, W, ld = hmap.shape
    if gt_rows.dim() != 3 or gt_rows.shape[0] != B or gt_rows.shape[2] != EVAL_GT_ROW or tuple(calib.shape) != (B, 6) or tuple(pad.shape) != (B, 2):
        raise RuntimeError("eval_diagnostics: gt_rows (B, M, 16), calib (B, 6), pad (B, 2) for hmap (B, H, W, ld); got %s, %s, %s, %s"
                           % (tuple(gt_rows.shape), tuple(calib.shape), tuple(pad.shape), tuple(hmap.shape)))
    if not (hmap.is_contiguous() and gt_rows.is_contiguous() and calib.is_contiguous() and pad.is_contiguous()):
        raise RuntimeError("eval_diagnostics: operands must be contiguous")
    if return_boxes and not want & 2:
        raise ValueError("eval_diagnostics: the boxes come with the IoUs (want bit 1)")
    M = gt_rows.shape[1]
    dev = hmap.device
    depth_err = torch.empty((B, M, len(EVAL_DEPTH_KEYS)), dtype=torch.float32, device=dev) if want & 1 else None
    iou = torch.empty((B, M, len(EVAL_IOU_KEYS)), dtype=torch.float32, device=dev) if want & 2 else None
    boxes = torch.empty((B, M, 6, 7), dtype=torch.float32, device=dev) if return_boxes else None
    L.check(L.load().mfx_eval_diagnostics(_ptr(hmap), ld, reg_off, _ptr(gt_rows), B, M, H, W, _ptr(calib), _ptr(pad), ctypes.byref(cfg),
                                          ctypes.byref(heads), int(want), _ptr(depth_err), _ptr(iou), _ptr(boxes), _stream()),
            "mfx_eval_diagnostics")
    return (depth_err, iou, boxes) if return_boxes else (depth_err, iou)
