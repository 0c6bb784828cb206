#!/usr/bin/env python
"""SHA-256 of every output tensor of every DCN kernel family on seeded inputs, one line per case, with the dispatch-counter deltas that
say which kernel ran.  For A/B of two BUILDS of the library that must agree to the bit (a refactor of the kernels' shared arithmetic):

    python tools/dcn_bits.py > a.txt ; MFX_LIB_PATH=/path/to/other/libmonoflex_hip.so python tools/dcn_bits.py > b.txt ; diff a.txt b.txt

Two fresh processes; only the public ops / autograd / _ext API.  Offsets: sigma 2 px, 2 % of the samples planted in each border band
((-1, 0) and (H-1, H) of either axis) and 2 % thrown 12..20 px away (beyond the LDS patch margin and the tile window: the far passes).
No wild or non-finite offsets.  Every backward case runs with option deterministic = 1 (the atomics forms are not repeatable)."""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from monoflex_amd import autograd as AG, lib as L, ops                       # noqa: E402
from monoflex_amd.model.backbone.DCNv2 import _ext                           # noqa: E402
from monoflex_amd.model.backbone.DCNv2.dcn_v2 import DCN                     # noqa: E402

DEV = "cuda"
COUNTERS = ("dcn_lds", "dcn_lds_of", "dcn_lds_split", "dcn_patch", "dcn_wave", "dcn_gather", "conv_splitk",
            "dcn_bt_fly", "dcn_bt_fused", "dcn_bt_tile", "dcn_bt_sample", "dcn_bt_far")


def sha(t):
    t = t.detach().contiguous().cpu()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()[:24]


def offsets(g, B, Ho, Wo, H, W, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, kh=3, kw=3):
    """(B, Ho, Wo, 18) offsets [2k] = dh, [2k + 1] = dw as described in the module docstring."""
    off = torch.randn(B, Ho, Wo, kh * kw, 2, generator=g) * 2.0
    oy = torch.arange(Ho).view(1, Ho, 1, 1) * sh - ph + (torch.arange(kh * kw) // kw).view(1, 1, 1, -1) * dh
    ox = torch.arange(Wo).view(1, 1, Wo, 1) * sw - pw + (torch.arange(kh * kw) % kw).view(1, 1, 1, -1) * dw
    base = torch.stack([oy.expand(B, Ho, Wo, kh * kw), ox.expand(B, Ho, Wo, kh * kw)], -1).float()
    pick = torch.rand(B, Ho, Wo, kh * kw, generator=g)
    frac = torch.rand(B, Ho, Wo, kh * kw, generator=g) * 0.9 + 0.05
    size = torch.tensor([H, W]).float()
    for axis in (0, 1):
        lo = (pick >= 0.02 * (2 * axis)) & (pick < 0.02 * (2 * axis + 1))                 # band (-1, 0)
        hi = (pick >= 0.02 * (2 * axis + 1)) & (pick < 0.02 * (2 * axis + 2))             # band (H-1, H)
        off[..., axis][lo] = (-frac - base[..., axis])[lo]
        off[..., axis][hi] = (size[axis] - 1 + frac - base[..., axis])[hi]
    far = (pick >= 0.08) & (pick < 0.10)
    sign = torch.where(torch.rand(B, Ho, Wo, kh * kw, 2, generator=g) < 0.5, -1.0, 1.0)
    off[far] = (sign * (12.0 + 8.0 * torch.rand(B, Ho, Wo, kh * kw, 2, generator=g)))[far]
    return off.reshape(B, Ho, Wo, 2 * kh * kw)


def offmask_rows(g, B, H, W):
    om = torch.zeros(B, H, W, 32)
    om[..., :18] = offsets(g, B, H, W, H, W)
    om[..., 18:27] = torch.sigmoid(torch.randn(B, H, W, 9, generator=g))
    return om


def module(g, cin, cout, dt):
    m = DCN(cin, cout, kernel_size=(3, 3), stride=1, padding=1, dilation=1, deformable_groups=1)
    with torch.no_grad():
        m.weight.copy_((torch.randn(m.weight.shape, generator=g) * 0.05).to(dt).float())
        m.bias.copy_(torch.randn(cout, generator=g) * 0.1)
        m.conv_offset_mask.weight.copy_((torch.randn(m.conv_offset_mask.weight.shape, generator=g) * (0.3 / (9 * cin) ** 0.5)).to(dt).float())
        b = torch.randn(27, generator=g) * 2.0
        b[18:] = torch.randn(9, generator=g)
        m.conv_offset_mask.bias.copy_(b)
    return m.to(DEV)


def run(name, opts, fn):
    lib_ = L.load()
    L.check(lib_.mfx_reset_options(), "reset")
    try:
        L.set_options(opts)
        before = {c: lib_.mfx_get_counter(c.encode()) for c in COUNTERS}
        outs = fn()
        torch.cuda.synchronize()
        delta = " ".join("%s+%d" % (c, lib_.mfx_get_counter(c.encode()) - before[c]) for c in COUNTERS if lib_.mfx_get_counter(c.encode()) != before[c])
        print("%-34s %s | %s" % (name, " ".join(sha(t) for t in outs), delta or "-"), flush=True)
    except RuntimeError as e:
        msg = str(e).replace("\n", " ")[:160]
        print("%-34s NOT RUN: %s" % (name, msg), flush=True)
        if "hip" in msg.lower() or "illegal" in msg.lower() or "memory access" in msg.lower():
            sys.exit(3)                                     # a device error: nothing more runs in this process
    finally:
        lib_.mfx_reset_options()


def forward_cases():
    B, H, W = 2, 24, 40
    for half, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        g = torch.Generator().manual_seed(11)
        m = module(g, 64, 64, dt)
        x = torch.randn(B, H, W, 64, generator=g).to(dt).to(DEV)
        om = offmask_rows(g, B, H, W).to(DEV)
        p, po = m.packed_main(dt), m.packed_offset(dt)
        run("fwd dcn_lds %s" % half, {"dcn_lds": 2}, lambda: [ops.dcn(x, om, p)])
        run("fwd dcn_lds %s +offset conv" % half, {"dcn_lds": 2}, lambda: list(ops.dcn_module(x, po, p, need_offmask=True)))
        run("fwd dcn_patch %s" % half, {"dcn_lds": 0, "dcn_patch": 2}, lambda: [ops.dcn(x, om, p)])
        run("fwd dcn_patch %s +offset conv" % half, {"dcn_lds": 0, "dcn_patch": 2}, lambda: list(ops.dcn_module(x, po, p, need_offmask=True)))
    g = torch.Generator().manual_seed(12)
    m = module(g, 64, 64, torch.float16)
    xs = torch.randn(B, H, W, 64, generator=g).to(DEV)
    om = offmask_rows(g, B, H, W).to(DEV)
    ps = m.packed_main(ops.F16X2)
    run("fwd dcn_lds split", {"dcn_lds": 2}, lambda: [ops.dcn(xs, om, ps)])
    g = torch.Generator().manual_seed(13)
    m = module(g, 128, 128, torch.bfloat16)
    x = torch.randn(B, H, W, 128, generator=g).bfloat16().to(DEV)
    om = offmask_rows(g, B, H, W).to(DEV)
    p = m.packed_main(torch.bfloat16)
    run("fwd dcn_wave 128->128 bf16", {}, lambda: [ops.dcn(x, om, p)])
    g = torch.Generator().manual_seed(14)
    m = module(g, 128, 64, torch.bfloat16)
    for half, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        x = torch.randn(B, H, W, 128, generator=torch.Generator().manual_seed(15)).to(dt).to(DEV)
        p = m.packed_main(dt)
        run("fwd dcn_gather 128->64 %s" % half, {"dcn_wave": 0, "dcn_patch": 0, "dcn_lds": 0, "dcn_ksplit": 1}, lambda: [ops.dcn(x, om, p)])
    run("fwd dcn_gather 128->64 bf16 split-K", {"dcn_wave": 0, "dcn_patch": 0, "dcn_lds": 0, "dcn_ksplit": 2}, lambda: [ops.dcn(x, om, p)])
    g = torch.Generator().manual_seed(16)
    m = module(g, 256, 64, torch.bfloat16)
    x = torch.randn(B, H, W, 256, generator=g).bfloat16().to(DEV)
    p = m.packed_main(torch.bfloat16)
    run("fwd dcn_ps 256->64 bf16", {}, lambda: [ops.dcn_ps(x, om, p)])


def ext_cases():
    B, C, Co, H, W, dg = 2, 8, 8, 12, 20, 2
    for tag, (sh, sw, ph, pw, dh, dw) in (("s1 p1 d1", (1, 1, 1, 1, 1, 1)), ("s2/1 p0/2 d1/2", (2, 1, 0, 2, 1, 2)), ("s1/2 p2/0 d2/1", (1, 2, 2, 0, 2, 1))):
        g = torch.Generator().manual_seed(21)
        Ho, Wo = (H + 2 * ph - (dh * 2 + 1)) // sh + 1, (W + 2 * pw - (dw * 2 + 1)) // sw + 1
        x = torch.randn(B, C, H, W, generator=g)
        w = torch.randn(Co, C, 3, 3, generator=g) / (C * 9) ** 0.5
        b = torch.randn(Co, generator=g)
        off = torch.cat([offsets(g, B, Ho, Wo, H, W, sh, sw, ph, pw, dh, dw) for _ in range(dg)], -1).permute(0, 3, 1, 2).contiguous()
        msk = torch.sigmoid(torch.randn(B, 9 * dg, Ho, Wo, generator=g))
        go = torch.randn(B, Co, Ho, Wo, generator=g)
        a = [t.to(DEV) for t in (x, w, b, off, msk)]
        geo = (3, 3, sh, sw, ph, pw, dh, dw, dg)
        run("_ext forward dg2 %s" % tag, {}, lambda: [_ext.dcn_v2_forward(*a, *geo)])
        for fast in (1, 0):
            run("_ext backward dg2 %s fast=%d" % (tag, fast), {"ext_bwd_fast": fast, "deterministic": 1},
                lambda: list(_ext.dcn_v2_backward(*a, go.to(DEV), *geo)))
    # the model's own geometry at 64 channels: the fast route of the boundary takes the tile-owned kernels
    g = torch.Generator().manual_seed(22)
    B, C, Co = 2, 64, 64
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(Co, C, 3, 3, generator=g) / (C * 9) ** 0.5
    b = torch.randn(Co, generator=g)
    off = offsets(g, B, H, W, H, W).permute(0, 3, 1, 2).contiguous()
    msk = torch.sigmoid(torch.randn(B, 9, H, W, generator=g))
    go = torch.randn(B, Co, H, W, generator=g)
    a = [t.to(DEV) for t in (x, w, b, off, msk)]
    geo = (3, 3, 1, 1, 1, 1, 1, 1, 1)
    run("_ext forward 64->64", {}, lambda: [_ext.dcn_v2_forward(*a, *geo)])
    for fast in (1, 0):
        run("_ext backward 64->64 fast=%d" % fast, {"ext_bwd_fast": fast, "deterministic": 1}, lambda: list(_ext.dcn_v2_backward(*a, go.to(DEV), *geo)))


def train_cases():
    forms = (("fly2", {"dcn_bt_fly": 2, "dcn_bt_fuse_wgrad": 1}), ("fly", {"dcn_bt_fly": 1, "dcn_bt_fuse_wgrad": 1}),
             ("fused", {"dcn_bt_fly": 0, "dcn_bt_fuse_wgrad": 1}), ("unfused", {"dcn_bt_fly": 0, "dcn_bt_fuse_wgrad": 0}))
    for half, dt, C, Co, H, W in (("bf16", torch.bfloat16, 64, 64, 24, 64), ("fp16", torch.float16, 64, 64, 24, 64),
                                  ("bf16", torch.bfloat16, 64, 64, 24, 40), ("bf16", torch.bfloat16, 128, 64, 24, 40),
                                  ("fp32", torch.float32, 64, 64, 24, 40)):
        g = torch.Generator().manual_seed(31)
        B = 2
        x = torch.randn(B, H, W, C, generator=g).to(dt)
        om = offmask_rows(g, B, H, W)
        w = (torch.randn(Co, C, 3, 3, generator=g) * 0.05).to(dt).float()
        b = torch.randn(Co, generator=g) * 0.1
        r = torch.randn(B, H, W, Co, generator=g)

        def step():
            xd = x.to(DEV).requires_grad_()
            omd, wd, bd = om.to(DEV).requires_grad_(), w.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
            y = AG.DCNFn.apply(xd, omd, wd, bd, 1, 1, 1, True)
            (y.float() * r.to(DEV)).sum().backward()
            return [y, xd.grad, omd.grad, wd.grad, bd.grad]
        for fname, fo in forms:
            o = dict(fo, deterministic=1, dcn_bt_fuse_min_chunks=1)
            run("train bwd %s %d->%d %dx%d %s" % (half, C, Co, H, W, fname), o, step)


if __name__ == "__main__":
    print("library:", L.LIB_PATH, flush=True)
    which = sys.argv[1:] or ["forward", "ext", "train"]
    if "forward" in which:
        forward_cases()
    if "ext" in which:
        ext_cases()
    if "train" in which:
        train_cases()
