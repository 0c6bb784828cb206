"""Case tables, input generators and float64 references for the convolution weight gradient (conv_wgrad_impl in csrc/train_kernels.hip,
the kernels of csrc/wgrad_tr.hip, the stem's own kernel) and the convolution data gradient (autograd._conv_backward).

Shared by tests/test_wgrad_cases_cpu.py (proves the preconditions on the references alone) and tests/test_gpu_wgrad_exact.py (compares the
kernels with them).  CPU torch only: nothing here touches a GPU.

Exactness.  Activations, output gradients, residuals and weights are drawn from +-{1/4, 1/2, 3/4, 1}: bf16, fp16 and fp32 numbers, never 0.
A product of two of them is a multiple of 1/16 with magnitude <= 1, so a sum of n products is an integer number of sixteenths below 16 n.
exact_terms_bound() demands 16 n <= 2^20 -- four bits below fp32's 2^24, room for however the matrix cores align products before they
add -- and then every partial sum, in any order, over any split into slabs, through atomics or the reduce pass, is an fp32 number: the
kernel's result is the mathematical one and `torch.equal` with the float64 reference is the comparison.  Because no operand is zero every
(pixel, tap) pair contributes non-zero products to a whole (Cout, Ck) slice of dW; a dropped, doubled or misplaced pair changes that slice
(CPU test: test_a_dropped_pixel_fails_the_comparison).
    dW   n = M = B * Ho * Wo accumulated terms               (<= 65536 pixels; every case here is below 10^4)
    dx   n = kh * kw * Cp products, + 1 for the residual

Routes.  plan() restates the dispatch of conv_wgrad_impl / try_conv_wgrad_patch / conv_wgrad_tr_t as read from the source; every row of the
tables names the route it must take, the CPU test asserts plan(row) agrees and the GPU test asserts the library's dispatch counters agree.
"""
import os
import re
from functools import lru_cache

import torch
import torch.nn.functional as F

from helper_kernels_cases import CANARY, CSRC, DTYPES, GUARD, TORCH_DTYPE          # noqa: F401  (re-exported for the two test modules)

HALVES = ("bf16", "fp16")
WS_FLOATS = 1 << 22                                       # the GPU test's own workspace: 16 MiB of fp32, canary-filled before every call
COUNTERS = ("wgrad_patch", "wgrad_tr", "wgrad_mfma", "wgrad_valu", "wgrad_reduce", "stem_wgrad")
ROUTE_COUNTER = {"patch": "wgrad_patch", "tr": "wgrad_tr", "mfma": "wgrad_mfma", "valu": "wgrad_valu", "stem": "stem_wgrad"}

# the options the dispatch reads, with the defaults of csrc/options.h (test_wgrad_cases_cpu.py compares them with the header)
DEFAULTS = dict(wgrad_mfma=1, wgrad_blocks=600, wgrad_ws=1, wgrad_ws_blocks=1200, wgrad_min_m=128, wgrad_tr=1, wgrad_tr_blocks=512,
                wgrad_patch=1, wgrad_patch_blocks=256, wgrad_patch_waves=12, deterministic=0)


def option_defaults():
    """{name: default} of the options above, parsed from the X(name, default, ...) table of csrc/options.h."""
    with open(os.path.join(CSRC, "options.h")) as f:
        src = f.read()
    out = {}
    for name in DEFAULTS:
        m = re.search(r"X\(%s,\s*(-?\d+)," % name, src)
        assert m, "option %s is not in options.h" % name
        out[name] = int(m.group(1))
    return out


# ---- the grid ----------------------------------------------------------------------------------------------------------------------------

def grid(shape, seed):
    """float64 values of +-{1/4, 1/2, 3/4, 1}, never 0."""
    r = torch.randint(0, 8, tuple(shape), generator=torch.Generator().manual_seed(seed))
    return ((r % 4 + 1).double() / 4) * (1 - 2 * (r // 4)).double()


def exact_terms_bound(n_terms):
    """16 * (number of accumulated terms): the largest magnitude, in sixteenths, any partial sum can have.  Must be <= 2^20."""
    return 16 * n_terms


BOUND_CAP = 2 ** 20


# ---- a weight-gradient row --------------------------------------------------------------------------------------------------------------

class WCase:
    """One call of a C entry.  entry: 'oihw' (mfx_conv_wgrad_oihw: workspace, (Cout_real, Cin_real, kh, kw) result), 'nhwc' (mfx_conv_wgrad_nhwc:
    no workspace, [Cout][tap][Ck]) or 'dil' (mfx_conv_wgrad_nhwc_dil).  ws: floats of workspace handed to the oihw entry.  same: x is both operands."""

    def __init__(self, name, route, B, H, W, Ck, Cout, k=3, s=1, dts=HALVES, entry="oihw", opts=None, ws=WS_FLOATS, kh=None, kw=None, pad=None,
                 dil_w=1, xps=None, ldy=None, Cout_real=None, Cin_real=None, Ho=None, Wo=None, same=False, expect=None):
        self.name, self.route, self.dts, self.entry, self.opts, self.ws, self.same = name, route, tuple(dts), entry, dict(opts or {}), ws, same
        self.B, self.H, self.W, self.Ck, self.Cout, self.stride, self.dil_w = B, H, W, Ck, Cout, s, dil_w
        self.kh, self.kw = kh or k, kw or k
        self.pad_h, self.pad_w = pad if pad is not None else (self.kh // 2, self.kw // 2)
        self.xps, self.ldy = xps or Ck, ldy or Cout
        self.Cout_real, self.Cin_real = Cout_real or Cout, Cin_real or Ck
        self.Ho = Ho if Ho is not None else (H + 2 * self.pad_h - self.kh) // s + 1
        self.Wo = Wo if Wo is not None else (W + 2 * self.pad_w - dil_w * (self.kw - 1) - 1) // s + 1
        self.M, self.K = B * self.Ho * self.Wo, self.kh * self.kw * Ck
        self.expect = dict(expect or {})                  # entries of plan() the row exists for (asserted by the CPU test)
        assert not same or (self.ldy == self.xps and Cout <= self.xps and self.Ho == H and self.Wo == W)

    def __repr__(self):
        return self.name

    def dw_numel(self):
        return self.Cout_real * self.Cin_real * self.kh * self.kw if self.entry == "oihw" else self.Cout * self.K


def cdiv(a, b):
    return (a + b - 1) // b


def plan(c, dt):
    """The dispatch of conv_wgrad_impl for row `c` in dtype `dt`, restated:
    -> dict(route, reduce (wgrad_reduce_kernel runs), ws_used (floats of the workspace the kernels may write), + the slab arithmetic of the route)."""
    o = dict(DEFAULTS)
    o.update(c.opts)
    is16 = dt != "fp32"
    has_ws = c.entry == "oihw"                            # the other two entries pass no workspace
    ws_floats = c.ws if has_ws else 0
    M, K = c.M, c.K
    if is16 and o["wgrad_mfma"]:
        # try_conv_wgrad_patch
        if (o["wgrad_patch"] and has_ws and (c.kh, c.kw, c.stride, c.pad_h, c.pad_w, c.dil_w) == (3, 3, 1, 1, 1, 1) and c.Ho == c.H and c.Wo == c.W
                and (c.Ck % 64 == 0 or c.Ck in (16, 32)) and c.xps == c.Ck and c.ldy % 8 == 0 and c.Cout % 8 == 0 and M >= 2048
                and not (c.Ck < 64 and c.Cout > 32)):
            ntiles = cdiv(c.W, 32) * cdiv(c.H, 4) * c.B
            xs = 4 if c.Ck >= 64 else c.Ck // 16
            os_ = 4 if c.Cout > 32 else (2 if (c.Cout > 16 or xs == 4) else 1)
            otiles, slices = cdiv(c.Cout, 16 * os_), c.Ck // (16 * xs)
            ws_slab = c.Cout * K
            nslab = max(1, (8 if xs < 4 else 1) * o["wgrad_patch_blocks"] // (otiles * slices))
            nslab = min(nslab, ws_floats // ws_slab)
            nslab = min(nslab, max(1, ntiles // 4))
            if nslab >= 1:
                tps = cdiv(ntiles, nslab)
                nslab = cdiv(ntiles, tps)
                return dict(route="patch", reduce=True, ws_used=nslab * ws_slab, nslab=nslab, tiles_per_slab=tps, ntiles=ntiles,
                            last_slab_tiles=ntiles - (nslab - 1) * tps, xs=xs, os=os_, waves=(12 if o["wgrad_patch_waves"] == 12 else 6) if xs == 4 and os_ == 4
                            else (3 if xs == 1 else 6))
        # conv_wgrad_tr_t
        if (o["wgrad_tr"] and has_ws and (c.Cout % 128 == 0 or o["wgrad_tr"] == 2) and K % 192 == 0 and c.Cout % 64 == 0 and c.Ck % 8 == 0
                and c.xps % 8 == 0 and c.ldy % 8 == 0 and M >= 4096):
            bo = 128 if c.Cout % 128 == 0 else 64
            tiles = (K // 192) * (c.Cout // bo)
            ws_slab = c.Cout * K
            slabs = min(max(1, o["wgrad_tr_blocks"] // tiles), ws_floats // ws_slab)
            if slabs >= 1:
                mpb = max(512, cdiv(M // slabs, 32) * 32)
                nslab = cdiv(M, mpb)
                return dict(route="tr", reduce=True, ws_used=nslab * ws_slab, nslab=nslab, m_per_block=mpb, bo=bo, last_slab_m=M - (nslab - 1) * mpb)
    if is16 and c.Ck % 8 == 0 and c.xps % 2 == 0 and c.ldy % 8 == 0 and o["wgrad_mfma"]:
        bt = 128 if (c.Cout >= 128 and K >= 128 and o["wgrad_mfma"] == 3) else 64
        tiles = cdiv(K, bt) * cdiv(c.Cout, bt)
        ws_ld = cdiv(K, bt) * bt
        ws_slab = cdiv(c.Cout, bt) * bt * ws_ld
        use_ws = has_ws and bool(o["wgrad_ws"])
        slabs = max(1, (o["wgrad_ws_blocks"] if use_ws else o["wgrad_blocks"]) // tiles)
        if use_ws:
            slabs = max(1, min(slabs, ws_floats // ws_slab))
        mpb = max(max(32, o["wgrad_min_m"] // 32 * 32), cdiv(M // slabs, 32) * 32)
        nslab = cdiv(M, mpb)
        ws_ok = use_ws and nslab * ws_slab <= ws_floats
        if not ws_ok and o["deterministic"]:
            mpb = cdiv(M, 32) * 32
        nslab = cdiv(M, mpb)
        return dict(route="mfma", reduce=ws_ok, ws_used=nslab * ws_slab if ws_ok else 0, nslab=nslab, m_per_block=mpb, bt=bt, ws_ok=ws_ok,
                    last_slab_m=M - (nslab - 1) * mpb)
    mpb = M if o["deterministic"] else 2048
    return dict(route="valu", reduce=False, ws_used=0, nslab=cdiv(M, mpb), m_per_block=mpb)


# ---- operands and references -------------------------------------------------------------------------------------------------------------

def wgrad_inputs(c, seed=7):
    """float64 (x (B, H, W, xps), dy (B, Ho, Wo, ldy)) on the grid -- padding channels included, so a kernel that reads them fails the comparison."""
    x = grid((c.B, c.H, c.W, c.xps), seed)
    dy = x if c.same else grid((c.B, c.Ho, c.Wo, c.ldy), seed + 1)
    return x, dy


def wgrad_windows(x, Ck, kh, kw, stride, pad_h, pad_w, dil_w, Ho, Wo):
    """x (B, H, W, x_pixstride) -> (kh * kw, B, Ho, Wo, Ck): the operand of every tap, x[b, oh s - pad_h + i, ow s - pad_w + j dil_w, c] with
    out-of-range pixels read as zero.  c runs over Ck CONSECUTIVE elements of memory from the pixel's first one (Ck > x_pixstride: the stem's
    super-taps run into the next pixel of the row)."""
    B, H, W, xps = x.shape
    flat = torch.cat([x.reshape(B, -1), torch.zeros((B, Ck), dtype=x.dtype)], 1)
    xe = flat.as_strided((B, H, W, Ck), (flat.stride(0), W * xps, xps, 1))
    top, left = max(pad_h, 0), max(pad_w, 0)
    bottom = max(0, (Ho - 1) * stride - pad_h + kh - 1 - (H - 1))
    right = max(0, (Wo - 1) * stride - pad_w + (kw - 1) * dil_w - (W - 1))
    xp = torch.zeros((B, top + H + bottom, left + W + right, Ck), dtype=x.dtype)
    xp[:, top:top + H, left:left + W] = xe
    taps = []
    for i in range(kh):
        for j in range(kw):
            h0, w0 = top - pad_h + i, left - pad_w + j * dil_w
            taps.append(xp[:, h0:h0 + (Ho - 1) * stride + 1:stride, w0:w0 + (Wo - 1) * stride + 1:stride])
    return torch.stack(taps)


def wgrad_ref(x, dy, Ck, kh, kw, stride, pad_h, pad_w, dil_w, Ho, Wo, Cout, shuffle=None, drop=None):
    """dW[o, i kw + j, c] = sum_{b, oh, ow} x[b, oh s - pad_h + i, ow s - pad_w + j dil_w, c] dy[b, oh, ow, o] in the dtype of the operands,
    (Cout, kh kw, Ck).  shuffle = seed: the pixels are summed in a random order, 61 at a time, one running sum.  drop = a flat pixel index
    (b, oh, ow) whose contribution is left out of every tap."""
    taps = wgrad_windows(x, Ck, kh, kw, stride, pad_h, pad_w, dil_w, Ho, Wo)
    T, M = kh * kw, dy.shape[0] * Ho * Wo
    a = taps.reshape(T, M, Ck)
    g = dy[..., :Cout].reshape(M, Cout)
    if drop is not None:
        keep = torch.ones(M, dtype=torch.bool)
        keep[drop] = False
        a, g = a[:, keep], g[keep]
    if shuffle is None:
        return torch.einsum("tmc,mo->otc", a, g)
    perm = torch.randperm(g.shape[0], generator=torch.Generator().manual_seed(shuffle))
    a, g = a[:, perm], g[perm]
    acc = torch.zeros((Cout, T, Ck), dtype=x.dtype)
    for m0 in range(0, g.shape[0], 61):
        acc = acc + torch.einsum("tmc,mo->otc", a[:, m0:m0 + 61], g[m0:m0 + 61])
    return acc


def as_oihw(dw, kh, kw, Cout_real, Cin_real):
    """(Cout, kh kw, Ck) -> the (Cout_real, Cin_real, kh, kw) layout of mfx_conv_wgrad_oihw (padded channels dropped)."""
    return dw[:Cout_real, :, :Cin_real].permute(0, 2, 1).reshape(Cout_real, Cin_real, kh, kw).contiguous()


def case_ref(c, x, dy, **kw):
    """The reference of a row in the layout its entry writes."""
    dw = wgrad_ref(x, dy, c.Ck, c.kh, c.kw, c.stride, c.pad_h, c.pad_w, c.dil_w, c.Ho, c.Wo, c.Cout, **kw)
    return as_oihw(dw, c.kh, c.kw, c.Cout_real, c.Cin_real) if c.entry == "oihw" else dw


@lru_cache(maxsize=4)
def case_data(c):
    """(x, dy, float64 reference) of a row, computed once and shared by the dtypes of the row (do not modify)."""
    x, dy = wgrad_inputs(c)
    return x, dy, case_ref(c, x, dy)


def is_standard(c):
    """A row F.conv2d autograd can state: square dilation-free taps over dense channels."""
    return c.dil_w == 1 and c.xps == c.Ck and c.Ho == (c.H + 2 * c.pad_h - c.kh) // c.stride + 1 and c.Wo == (c.W + 2 * c.pad_w - c.kw) // c.stride + 1


def conv2d_wgrad_ref(x, dy, c):
    """float64 F.conv2d autograd of a standard row: (Cout, Ck, kh, kw)."""
    w = torch.zeros((c.Cout, c.Ck, c.kh, c.kw), dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x[..., :c.Ck].permute(0, 3, 1, 2), w, None, stride=c.stride, padding=(c.pad_h, c.pad_w))
    assert y.shape[2:] == (c.Ho, c.Wo), (y.shape, c.Ho, c.Wo)
    y.backward(dy[..., :c.Cout].permute(0, 3, 1, 2))
    return w.grad


# ---- the route tables --------------------------------------------------------------------------------------------------------------------------
# patch: 3x3 / s1 / p1, Ck % 64 == 0 or Ck in {16, 32} with Cout <= 32, Cout % 8 == 0, M >= 2048, workspace.  4 x 32 pixel tiles:
#   2 x 23 x 45   M 2070: 6 x 2 tiles per image, the last tile row holds 3 of 4 rows, the last tile column 13 of 32 pixels
#   3 x 8 x 96    M 2304: tiles fit exactly (2 x 3 per image)
#   1 x 65 x 33   M 2145: one pixel over a tile in both directions (17 x 2 tiles)
# slabs: nslab <= ntiles / 4 ("at least four tiles per slab"), so with the default 256 target blocks the 24 tiles of 2 x 23 x 45 already make 6
# slabs of 4 tiles; a slab of a SINGLE tile cannot be reached at any option value (M >= 2048 means ntiles >= 16): the row with
# wgrad_patch_blocks = 4096 pins that floor instead.  wgrad_patch_blocks = 5 -> ceil(24 / 5) = 5 tiles per slab, the last slab holds 4.
_PATCH_GEOMS = [("2x23x45_64_64", 2, 23, 45, 64, 64, {}), ("2x23x45_16_16", 2, 23, 45, 16, 16, {}), ("2x23x45_32_32", 2, 23, 45, 32, 32, {}),
                ("2x23x45_128_24", 2, 23, 45, 128, 24, {}), ("2x23x45_64_27of32", 2, 23, 45, 64, 32, dict(Cout_real=27)),
                ("3x8x96_64_64", 3, 8, 96, 64, 64, {}), ("1x65x33_64_64", 1, 65, 33, 64, 64, {}),
                ("2x23x45_64_64_ldy72", 2, 23, 45, 64, 64, dict(ldy=72)), ("2x23x45_32_16", 2, 23, 45, 32, 16, {})]
PATCH_CASES = [WCase("patch_%s_w%d" % (n, wv), "patch", B, H, W, ck, co, opts=dict(wgrad_patch_waves=wv), **kw)
               for (n, B, H, W, ck, co, kw) in _PATCH_GEOMS for wv in (12, 6)]
PATCH_CASES += [
    WCase("patch_2x23x45_64_64_blocks1", "patch", 2, 23, 45, 64, 64, opts=dict(wgrad_patch_blocks=1), expect=dict(nslab=1, tiles_per_slab=24)),
    WCase("patch_2x23x45_64_64_blocks5", "patch", 2, 23, 45, 64, 64, opts=dict(wgrad_patch_blocks=5), expect=dict(nslab=5, tiles_per_slab=5, last_slab_tiles=4)),
    WCase("patch_2x23x45_64_64_blocks4096", "patch", 2, 23, 45, 64, 64, opts=dict(wgrad_patch_blocks=4096), expect=dict(nslab=6, tiles_per_slab=4)),
]

# tr: K % 192 == 0, Cout % 128 == 0 (% 64 under wgrad_tr = 2), M >= 4096, workspace; the patch form is switched off.
#   2 x 41 x 51   M 4182 = 8 * 512 + 86: not a multiple of 32 or 512.  m_per_block = max(512, ..): with the default 512 target blocks the slabs
#                 already sit at the 512 floor (9 slabs, the last one 86 pixels = 2 steps of 32 + 22); wgrad_tr_blocks = 4096 keeps them there,
#                 = 6 makes 2 slabs of 2112 / 2070 pixels, = 3 a single slab of 4182.
#   2 x 91 x 91   stride 2 -> 46 x 46, M 4232: the largest case of the suite
_TR = dict(wgrad_patch=0)
TR_CASES = [
    WCase("tr_2x41x51_64_128", "tr", 2, 41, 51, 64, 128, opts=_TR, expect=dict(m_per_block=512, nslab=9, last_slab_m=86, bo=128)),
    WCase("tr_2x41x51_64_64_tr2", "tr", 2, 41, 51, 64, 64, opts=dict(_TR, wgrad_tr=2), expect=dict(m_per_block=512, bo=64)),
    WCase("tr_2x91x91_s2_64_128", "tr", 2, 91, 91, 64, 128, s=2, opts=_TR, expect=dict(m_per_block=512, nslab=9)),
    WCase("tr_2x41x51_1x1_192_128", "tr", 2, 41, 51, 192, 128, k=1, opts=_TR),
    WCase("tr_2x41x51_64_128_blocks4096", "tr", 2, 41, 51, 64, 128, opts=dict(_TR, wgrad_tr_blocks=4096), expect=dict(m_per_block=512, nslab=9)),
    WCase("tr_2x41x51_64_128_blocks6", "tr", 2, 41, 51, 64, 128, opts=dict(_TR, wgrad_tr_blocks=6), expect=dict(m_per_block=2112, nslab=2, last_slab_m=2070)),
    WCase("tr_2x41x51_64_128_blocks3", "tr", 2, 41, 51, 64, 128, opts=dict(_TR, wgrad_tr_blocks=3), expect=dict(m_per_block=4192, nslab=1)),
    WCase("tr_2x41x51_64_128_ldy136", "tr", 2, 41, 51, 64, 128, opts=_TR, ldy=136),
    WCase("tr_2x41x51_64_128_xps72", "tr", 2, 41, 51, 64, 128, opts=_TR, xps=72),
]

# mfma: first-generation slab kernel, 64- or 128-wide tiles; patch and tr switched off.
#   2 x 13 x 37   M 962 (s1) / 266 (s2, 7 x 19): 128-pixel slabs (wgrad_min_m) cut rows of 37 and the batch boundary at pixel 481
#   3 x 20 x 36   M 2160 / 540
# forms: workspace + wgrad_reduce_kernel (default), fp32 atomics (wgrad_ws = 0), atomics with a single slab (deterministic = 1)
_MF = dict(wgrad_tr=0, wgrad_patch=0)
_MF_SHAPES = [("2x13x37", 2, 13, 37), ("3x20x36", 3, 20, 36)]
_MF_KINDS = [("3x3", 3, 1), ("3x3s2", 3, 2), ("1x1", 1, 1)]
_MF_CHANS = [("64_64", 64, 64, {}), ("128_128", 128, 128, {}), ("256_64", 256, 64, {}), ("64_27of32", 64, 32, dict(Cout_real=27))]
_MF_FORMS = [("ws", {}, dict(ws_ok=True)), ("atomic", dict(wgrad_ws=0), dict(ws_ok=False)),
             ("atomic_det", dict(wgrad_ws=0, deterministic=1), dict(ws_ok=False, nslab=1))]
MFMA_CASES = [WCase("mfma_%s_%s_%s_%s" % (sn, kn, cn, fn), "mfma", B, H, W, ck, co, k=k, s=s, opts=dict(_MF, **fo), expect=dict(fe, bt=64), **kw)
              for (sn, B, H, W) in _MF_SHAPES for (kn, k, s) in _MF_KINDS for (cn, ck, co, kw) in _MF_CHANS for (fn, fo, fe) in _MF_FORMS]
MFMA_CASES += [WCase("mfma_%s_%s_128_128_bt128_%s" % (sn, kn, fn), "mfma", B, H, W, 128, 128, k=k, s=s, opts=dict(_MF, wgrad_mfma=3, **fo),
                     expect=dict(fe, bt=128))
               for (sn, B, H, W) in _MF_SHAPES for (kn, k, s) in _MF_KINDS for (fn, fo, fe) in _MF_FORMS[:2]]
MFMA_CASES += [
    # 32-pixel slabs: 31 of them over 962 pixels; rows of 37 and the batch boundary (481 = 15 * 32 + 1) fall inside slabs, the last slab holds 2 pixels
    WCase("mfma_2x13x37_3x3_64_64_slab32", "mfma", 2, 13, 37, 64, 64, opts=dict(_MF, wgrad_min_m=32, wgrad_ws_blocks=9 * 64),
          expect=dict(m_per_block=32, nslab=31, last_slab_m=2, ws_ok=True)),
    # a workspace smaller than one slab: ws_ok is false, the tiles are accumulated with atomics and the workspace is not written
    WCase("mfma_2x13x37_3x3_64_64_small_ws", "mfma", 2, 13, 37, 64, 64, opts=_MF, ws=1000, expect=dict(ws_ok=False)),
    # mfx_conv_wgrad_nhwc: no workspace, [Cout][tap][Ck] result -- CatConv1x1Fn's call (1x1), and a 3x3 for the tap axis of that layout
    WCase("mfma_3x20x36_1x1_64_64_nhwc", "mfma", 3, 20, 36, 64, 64, k=1, entry="nhwc", opts=_MF, expect=dict(ws_ok=False)),
    WCase("mfma_2x13x37_3x3_64_128_nhwc", "mfma", 2, 13, 37, 64, 128, entry="nhwc", opts=_MF, expect=dict(ws_ok=False)),
]

# valu: fp32, 16-bit under wgrad_mfma = 0, 16-bit with Ck % 8 != 0.  2048-pixel slabs, atomics: 3 x 20 x 36 s1 makes two slabs (2048 + 112).
VALU_CASES = [WCase("valu_%s_%s_%s_fp32" % (sn, kn, cn), "valu", B, H, W, ck, co, k=k, s=s, dts=("fp32",), **kw)
              for (sn, B, H, W) in _MF_SHAPES for (kn, k, s) in _MF_KINDS for (cn, ck, co, kw) in (_MF_CHANS[0], _MF_CHANS[3])]
VALU_CASES += [
    WCase("valu_3x20x36_3x3_64_64_mfma0", "valu", 3, 20, 36, 64, 64, opts=dict(wgrad_mfma=0), expect=dict(nslab=2)),
    WCase("valu_3x20x36_3x3_4_8", "valu", 3, 20, 36, 4, 8, expect=dict(nslab=2)),
    WCase("valu_3x20x36_3x3_64_64_fp32_det", "valu", 3, 20, 36, 64, 64, dts=("fp32",), opts=dict(deterministic=1), expect=dict(nslab=1)),
    WCase("valu_3x20x36_1x1_64_64_fp32_nhwc", "valu", 3, 20, 36, 64, 64, k=1, dts=("fp32",), entry="nhwc"),
]

# the geometries the gram heads (gram_heads.py) and the stem (StemConvFn) pass, at the C boundary, default options.
#   gram 5x5 / 3x5    x is both operands (C = 64), pad (2, 2), Ho = H, Wo = W (the 3x5 form reads rows oh - 2 .. oh)
#                     (a 5x5 row on the tr route does not exist: K = 25 * 64 = 1600 is not a multiple of 192, so M >= 4096 would still run mfma)
#   matrix            _dense_wgrad: B = 1, H = 1, W = R rows of a (R, Kc) x (R, Co) product; R = 4100 >= 4096 stays on mfma because K = 64 is not a multiple of 192
#   stem              7 x 4 super-taps of two 4-channel pixels, dilation 2, over the packed (B, H + 6, W + 8, 4) image: Ck = 8 > x_pixstride = 4
_ALL = DTYPES
CALLER_CASES = [
    WCase("gram5x5_2x12x40_64", None, 2, 12, 40, 64, 64, k=5, pad=(2, 2), same=True, dts=_ALL),
    WCase("gram3x5_2x12x40_64", None, 2, 12, 40, 64, 64, kh=3, kw=5, pad=(2, 2), Ho=12, Wo=40, same=True, dts=_ALL),
    WCase("matrix_R130_64_128", None, 1, 1, 130, 64, 128, k=1, dts=_ALL),
    WCase("matrix_R4100_64_128", None, 1, 1, 4100, 64, 128, k=1, dts=_ALL),
    WCase("stemform_2x9x36", None, 2, 9 + 6, 36 + 8, 8, 16, kh=7, kw=4, pad=(0, 0), dil_w=2, xps=4, Ho=9, Wo=36, entry="dil", dts=_ALL),
    WCase("ldy96_2x13x37_64_64", None, 2, 13, 37, 64, 64, ldy=96, dts=_ALL),
    WCase("xps96_2x13x37_64_64", None, 2, 13, 37, 64, 64, xps=96, dts=_ALL),
]


def caller_route(dt):
    return "valu" if dt == "fp32" else "mfma"


WGRAD_TABLES = dict(patch=PATCH_CASES, tr=TR_CASES, mfma=MFMA_CASES, valu=VALU_CASES, caller=CALLER_CASES)
ALL_WCASES = [c for t in WGRAD_TABLES.values() for c in t]


def rows(table):
    """[(case, dtype)] of a table, for parametrize."""
    return [(c, dt) for c in table for dt in c.dts]


def row_id(v):
    return v if isinstance(v, str) else repr(v)


def row_route(c, dt):
    return c.route or caller_route(dt)


# ---- the stem, through StemConvFn: (B, H, W) ----------------------------------------------------------------------------------------------
# 8 x 32 output tiles of the stem's kernel: one tile exactly, (37, 70) ragged in both directions (5 x 3 tiles), (32, 64) whole tiles
STEM_CASES = [(1, 8, 32), (3, 37, 70), (2, 32, 64)]
STEM_COUT = 16


def stem_inputs(B, H, W, seed=21):
    """float64 (images (B, 3, H, W), weight (16, 3, 7, 7), dy NHWC (B, H, W, 16))."""
    return grid((B, 3, H, W), seed), grid((STEM_COUT, 3, 7, 7), seed + 1), grid((B, H, W, STEM_COUT), seed + 2)


def stem_wgrad_ref(images, dy):
    """float64 F.conv2d autograd: dW (16, 3, 7, 7) of the 7x7 / s1 / p3 stem."""
    w = torch.zeros((STEM_COUT, 3, 7, 7), dtype=images.dtype, requires_grad=True)
    F.conv2d(images, w, None, stride=1, padding=3).backward(dy.permute(0, 3, 1, 2))
    return w.grad


def stem_general_ref(images, dy):
    """The same gradient through the general reference, in the 16-bit path's own geometry: the packed image (zero border, zero fourth channel),
    7 x 4 super-taps of 8 elements at dilation 2, then StemConvFn's reshuffle to (16, 3, 7, 7)."""
    from monoflex_amd.packing import STEM_PAD_H, STEM_PAD_WL, STEM_PAD_WR
    B, _, H, W = images.shape
    xp = torch.zeros((B, H + 2 * STEM_PAD_H, W + STEM_PAD_WL + STEM_PAD_WR, 4), dtype=images.dtype)
    xp[:, STEM_PAD_H:STEM_PAD_H + H, STEM_PAD_WL:STEM_PAD_WL + W, :3] = images.permute(0, 2, 3, 1)
    dws = wgrad_ref(xp, dy, 8, 7, 4, 1, 0, 0, 2, H, W, STEM_COUT)
    return dws.view(STEM_COUT, 7, 4, 2, 4).reshape(STEM_COUT, 7, 8, 4)[:, :, :7, :3].permute(0, 3, 1, 2).contiguous()


# ---- the data gradient, through autograd._conv_backward -------------------------------------------------------------------------------------
# (k, stride, H, W): stride 2 over even / odd maps (H = 2 Ho and H = 2 Ho - 1, the same for W: the last inserted row / column is the last one of the map)
DGRAD_GEOMS = [(3, 2, 20, 36), (3, 2, 21, 36), (3, 2, 20, 37), (3, 2, 21, 37), (3, 1, 13, 37), (1, 1, 13, 37)]
# (Cin, Cout): 27 is padded to 32 channels of dy; Cin = 20 is padded to 32 rows of the operand, so dx is sliced and `res` takes the padded branch
DGRAD_CHANS = [(32, 64), (64, 128), (16, 27), (20, 64)]
DGRAD_B = 2


def pad_channels(n, dt):
    """packing._pad_channels, restated (the CPU test compares the two)."""
    return (n + 63) // 64 * 64 if n >= 64 else max(4 if dt == "fp32" else 8, 1 << (n - 1).bit_length())


def dgrad_cases():
    return [(k, s, H, W, cin, cout) for (k, s, H, W) in DGRAD_GEOMS for (cin, cout) in DGRAD_CHANS]


def dgrad_inputs(k, s, H, W, cin, cout, dt, seed=33):
    """float64 (weight (Cout, Cin, k, k), dy NHWC (B, Ho, Wo, Cp), res NHWC (B, H, W, Cin)); the padded channels of dy hold grid values too: the
    data-gradient operand has zero weights there, so they must not reach dx."""
    Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
    return grid((cout, cin, k, k), seed), grid((DGRAD_B, Ho, Wo, pad_channels(cout, dt)), seed + 1), grid((DGRAD_B, H, W, cin), seed + 2)


def dgrad_terms(k, cout, dt):
    return k * k * pad_channels(cout, dt) + 1


def dgrad_ref(w, dy, res, k, s, H, W):
    """float64 F.conv2d autograd: dx NHWC (B, H, W, Cin) (+ res)."""
    cout, cin = w.shape[0], w.shape[1]
    x = torch.zeros((dy.shape[0], cin, H, W), dtype=w.dtype, requires_grad=True)
    F.conv2d(x, w, None, stride=s, padding=k // 2).backward(dy[..., :cout].permute(0, 3, 1, 2))
    dx = x.grad.permute(0, 2, 3, 1)
    return (dx + res if res is not None else dx).contiguous()


def dgrad_general(w, dy, res, k, s, H, W, shuffle=None):
    """The same, written out: dx[b, oh s - p + i, ow s - p + j, c] += dy[b, oh, ow, o] w[o, c, i, j], taps in a shuffled order with `shuffle` = seed,
    the residual first."""
    cout, cin = w.shape[0], w.shape[1]
    B, Ho, Wo, _ = dy.shape
    p = k // 2
    buf = torch.zeros((B, H + 2 * p + s, W + 2 * p + s, cin), dtype=w.dtype)
    if res is not None:
        buf[:, p:p + H, p:p + W] = res
    order = list(range(k * k))
    if shuffle is not None:
        order = torch.randperm(k * k, generator=torch.Generator().manual_seed(shuffle)).tolist()
    g = dy[..., :cout]
    for t in order:
        i, j = t // k, t % k
        buf[:, i:i + (Ho - 1) * s + 1:s, j:j + (Wo - 1) * s + 1:s] += torch.einsum("bhwo,oc->bhwc", g, w[:, :, i, j])
    return buf[:, p:p + H, p:p + W].contiguous()
