"""Case tables, input generators and float64 references for the memory-bound helper kernels
(csrc/misc_kernels.hip and the pooling / upsample / column-sum part of csrc/train_kernels.hip).

Shared by tests/test_helper_kernels_cases_cpu.py (proves the preconditions on the references alone) and
tests/test_gpu_helper_kernels.py (compares the kernels with them).  CPU torch only: nothing here touches a GPU.

Exactness.  Every operand of an "exact" case sits on a dyadic grid so small that every partial sum of the operation,
in any order, with or without fused multiply-add, is an fp32 number; the inputs are bf16 and fp16 numbers as well:
    activations and gradients   multiples of 1/8,  |v| <= 4     (6 significant bits)
    upsample tap weights        multiples of 1/16, in [0, 1]
    column-sum operands         multiples of 1/8,  |v| <= 2,  M <= 2^18 + 5   ->  |sum| * 8 <= 2^22 + 80 < 2^24
    upsample forward            <= 4 products (multiples of 1/128, |.| <= 4) + skip      ->  |y| * 128  <= 2^12
    upsample dx                 <= (2f)^2 <= 256 such products                           ->  |dx| * 128 <= 2^17
    upsample dw                 B*H*W <= 1024 products x*dy (multiples of 1/64, <= 16)   ->  |dw| * 64  <= 2^20
The kernel's fp32 result is then the mathematical result and a 16-bit output is that result rounded once, so the
comparison with the float64 reference (`.to(dtype)`) is `torch.equal`.  exact_terms_bound() states the bounds; the
CPU test asserts them, and that the fp32 evaluation of every reference equals the float64 one.
"""
import os
import re

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "monoflex_amd", "csrc")

DTYPES = ("fp32", "bf16", "fp16")
TORCH_DTYPE = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
CHUNK = {"fp32": 4, "bf16": 8, "fp16": 8}               # elements of one 16-byte chunk
UNIT_ROUNDOFF = {"fp32": 0.0, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}     # one output rounding, with room for a boundary flip
ABS_FLOOR = {"fp32": 0.0, "bf16": 0.0, "fp16": 2.0 ** -24}               # fp16 subnormal spacing
CANARY = -24576.0                                        # -3 * 2^13: a bf16, fp16 and fp32 number far outside every exact result that is compared with it
GUARD = 256                                              # canary elements kept after the end of every test-owned output


def chunk_of(c, dt):
    """'chunk' in a case table is one 16-byte chunk of the dtype; 'chunk3' three of them."""
    if c == "chunk":
        return CHUNK[dt]
    if c == "chunk3":
        return 3 * CHUNK[dt]
    return c


# ---- the grid cap, read from the source ---------------------------------------------------------------------------------

def grid_caps():
    """{macro: (workgroup cap, threads per workgroup)} of the grid-stride launches, parsed from the two macros that set them."""
    out = {}
    for fn, macro in (("misc_kernels.hip", "MFX_GRID"), ("train_kernels.hip", "TR_GRID")):
        with open(os.path.join(CSRC, fn)) as f:
            src = f.read()
        m = re.search(r"#define\s+%s\(([^)]*)\)\s+dim3\(\(unsigned\)\((\w+)\(\(total\),\s*(\(threads\)|\d+)\)\s*<\s*(\d+)\s*\?[^:]*:\s*(\d+)\)\)" % macro, src)
        assert m, "cannot find the definition of %s in %s" % (macro, fn)
        assert m.group(4) == m.group(5), (macro, m.groups())
        if m.group(3) == "(threads)":                    # MFX_GRID(total, threads): every user passes the same literal
            uses = set(re.findall(r"%s\(total,\s*(\d+)\)" % macro, src))
            assert len(uses) == 1, (macro, uses)
            threads = int(uses.pop())
        else:
            threads = int(m.group(3))
        out[macro] = (int(m.group(4)), threads)
    return out


# ---- generators ------------------------------------------------------------------------------------------------------------

def _gen(seed):
    return torch.Generator().manual_seed(seed)


def dyadic(shape, seed, step=0.125, bound=4.0, nonzero=False):
    """float64 multiples of `step` in [-bound, bound]."""
    n = int(round(bound / step))
    v = torch.randint(-n, n + 1, tuple(shape), generator=_gen(seed)).double()
    if nonzero:
        v[v == 0] = 1.0
    return v * step


def tap_weights(C, f, seed):
    """(C, 1, 2f, 2f) float64 multiples of 1/16 in [0, 1]."""
    return torch.randint(0, 17, (C, 1, 2 * f, 2 * f), generator=_gen(seed)).double() / 16


def pool_input(B, C, H, W, seed):
    """(B, C, H, W) float64 multiples of 1/2 in [-2, 2], drawn so that most 2x2 windows have more than one maximum (each value is the
    largest of eight uniform draws: the top of the range is crowded; with one uniform draw only a fifth of the windows would tie at their
    maximum), plus a few +-inf: a window with two +inf, an all -inf window where the map is large enough, single infinities."""
    g = _gen(seed)
    v = torch.randint(0, 9, (8, B, C, H, W), generator=g).max(0).values.double() * 0.5 - 2.0
    v[0, 0, 0, 0] = float("inf")
    v[0, 0, 1, 1] = float("inf")                          # the same window: the first +inf takes the gradient
    v[-1, -1, -1, -1] = float("-inf")
    if H >= 6 and W >= 2:
        v[0, 1, 2:4, 0:2] = float("-inf")                 # a window of four -inf: its first element takes the gradient
        v[-1, 0, 4, 1] = float("inf")
    return v


def tie_share(x):
    """Share of the 2x2 windows (per channel) of a (B, C, H, W) map whose maximum occurs more than once."""
    w = pool_windows(x)
    return float(((w == w.max(-1, keepdim=True).values).sum(-1) > 1).double().mean())


def pool_windows(x):
    """(B, C, H, W) -> (B, C, H/2, W/2, 4), the window in row-major order."""
    B, C, H, W = x.shape
    return x.reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)


def pool_first_max_grad(x, dy):
    """The rule itself, without autograd: dy goes to the first maximum of each window in row-major order, exact zeros elsewhere."""
    B, C, H, W = x.shape
    w = pool_windows(x)
    eq = w == w.max(-1, keepdim=True).values
    first = eq & (eq.cumsum(-1) == 1)
    g = torch.where(first, dy.unsqueeze(-1).expand_as(w), torch.zeros((), dtype=dy.dtype))
    return g.reshape(B, C, H // 2, W // 2, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H, W)


# ---- references (float64 unless a dtype is given: the CPU test evaluates them in float32 as well) --------------------------

def pool_ref(x, dy):
    """-> (y, dx) of F.max_pool2d(x, 2, 2) and its autograd."""
    xr = x.clone().requires_grad_()
    y = F.max_pool2d(xr, 2, 2)
    y.backward(dy)
    return y.detach(), xr.grad


def upsample_ref(x, w, skip, f, dy=None):
    """Depthwise ConvTranspose2d(k = 2f, stride f, pad f/2) + skip, NCHW.  -> y, or (y, dx, dw) with `dy` (the skip gradient is dy itself)."""
    C = x.shape[1]
    if dy is None:
        y = F.conv_transpose2d(x, w, stride=f, padding=f // 2, groups=C)
        return y if skip is None else y + skip
    xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
    y = F.conv_transpose2d(xr, wr, stride=f, padding=f // 2, groups=C)
    if skip is not None:
        y = y + skip
    y.backward(dy)
    return y.detach(), xr.grad, wr.grad


def zero_insert_ref(dy, H, W):
    """(B, Ho, Wo, C) -> (B, H, W, C): dy at the even (h, w), zeros elsewhere."""
    B, Ho, Wo, C = dy.shape
    up = torch.zeros((B, H, W, C), dtype=dy.dtype)
    up[:, 0:2 * Ho:2, 0:2 * Wo:2] = dy[:, :(H + 1) // 2, :(W + 1) // 2]
    return up


def edge_scatter_ref(out, ch_off, C, v, edge_xy, edge_len, planar):
    """fp32 in, fp32 out: (map, planar) after adding v[b, j, :C] at pixel edge_xy[b, j] for j < edge_len[b]."""
    out = out.clone()
    planar = planar.clone() if planar is not None else None
    W = out.shape[2]
    for b in range(out.shape[0]):
        for j in range(int(edge_len[b])):
            x, y = int(edge_xy[b, j, 0]), int(edge_xy[b, j, 1])
            out[b, y, x, ch_off:ch_off + C] += v[b, j, :C]
            if planar is not None:
                planar[b, :, y * W + x] += v[b, j, :C]
    return out, planar


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


# ---- 1. layout transforms --------------------------------------------------------------------------------------------------
# (B, C, H, W, ld).  32x32 tiles over (pixel, channel): partial tiles in both axes, ld > C inside the last channel tile (zero fill / ignored padding),
# ld a whole tile past C (2, 33, 32, 32, 72: channel tiles 0..2, the third holds padding only; HW = 1024 = 32 tiles exactly), one element.
LAYOUT_CASES = [(2, 3, 5, 7, 4), (1, 27, 9, 13, 32), (2, 45, 33, 31, 48), (1, 64, 4, 40, 64), (2, 33, 32, 32, 72), (1, 1, 1, 1, 8)]

SPECIALS = [0.0, -0.0, float("inf"), float("-inf"), float("nan"),
            65504.0, 65519.0, 65520.0, -65504.0, -65519.0, -65520.0,              # fp16: largest finite, last value rounding to it, first rounding to inf
            1e-6, 6e-8, -1e-6, -6e-8,                                             # fp16 subnormals
            1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11,   # round-to-even ties of bf16 (2^-8) and fp16 (2^-11): down, up
            -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), -(1 + 2.0 ** -11), -(1 + 3 * 2.0 ** -11), 1.0]


def specials_nchw():
    """(1, 3, 2, 4) fp32 NCHW holding SPECIALS."""
    assert len(SPECIALS) == 24
    return torch.tensor(SPECIALS, dtype=torch.float32).reshape(1, 3, 2, 4)


# ---- 2. stem image packing ---------------------------------------------------------------------------------------------------
PACK_CASES = [(1, 1, 1), (2, 5, 7), (1, 37, 70)]
PACK_GRID_STRIDE_CASE = (1, 2050, 2050)                   # fp32 only: (2050 + 6) * (2050 + 8) = 4231248 pixels > 16384 * 256 = 4194304


def pack_ref(img, dt):
    """(B, 3, H, W) -> (B, H + 2 ph, W + pwl + pwr, 4) of the dtype: interior = cast image, border and fourth channel zero."""
    from monoflex_amd.packing import STEM_PAD_H, STEM_PAD_WL, STEM_PAD_WR
    B, _, H, W = img.shape
    y = torch.zeros((B, H + 2 * STEM_PAD_H, W + STEM_PAD_WL + STEM_PAD_WR, 4), dtype=TORCH_DTYPE[dt])
    y[:, STEM_PAD_H:STEM_PAD_H + H, STEM_PAD_WL:STEM_PAD_WL + W, :3] = img.permute(0, 2, 3, 1).to(TORCH_DTYPE[dt])
    return y


# ---- 3. max-pool ---------------------------------------------------------------------------------------------------------------
POOL_C = ("chunk", 24, 64)
POOL_HW = [(2, 2), (2, 6), (6, 2), (10, 14)]
POOL_B = (1, 3)


def pool_cases(dt):
    return [(B, chunk_of(C, dt), H, W) for C in POOL_C for (H, W) in POOL_HW for B in POOL_B]


# ---- 4. upsample forward: (B, f, C, H, W, skip) ---------------------------------------------------------------------------------
# every f (8 = the runtime-stride instantiation), every C, every (H, W), with and without skip, in each dtype
UPSAMPLE_FWD_CASES = [
    (1, 2, "chunk", 1, 1, True), (2, 2, 64, 1, 5, False), (1, 2, 128, 5, 1, True), (1, 2, 256, 3, 7, True), (2, 2, 64, 6, 10, True),
    (1, 4, "chunk", 6, 10, False), (2, 4, 64, 3, 7, True), (1, 4, 128, 1, 1, False), (1, 4, 256, 5, 1, True),
    (1, 8, "chunk", 5, 1, True), (1, 8, 64, 6, 10, True), (1, 8, 128, 3, 7, False), (1, 8, 256, 1, 5, False), (2, 8, 64, 1, 1, True),
]
UPSAMPLE_FWD_RANDN = (2, 4, 64, 6, 10, True)

# ---- 5. upsample backward: name -> (B, C, f, H, W) -----------------------------------------------------------------------------
# The arithmetic of upsample_bwd_dw_kernel for each case is restated by dw_plan() and asserted by the CPU test; in short
# (items = (2f)^2 * C / chunk, S = 1024 / items column groups, the 4x-unrolled column loop runs where iw_lo + grp + 3 S <= iw_hi):
#   unrolled_w19   fp32: items 256, S 4, 3 S = 12 <= 18    16-bit: items 128, S 8, 3 S = 24 > 18: tail loop only
#   unrolled_w35   fp32: S 4, two unrolled rounds for grp 0..2 + tail       16-bit: S 8, 3 S = 24 <= 34: unrolled, then a tail
#   tail_only      W = 3 < S in every dtype: groups grp >= 3 own no column
#   items_1024     fp32: items = 64 * 16 = 1024 exactly, S = 1, no LDS fold      16-bit: items 512, S 2
#   multi_pass     fp32: items = 256 * 16 = 4096 -> 4 passes of 1024 items       16-bit: 2048 -> 2 passes
#   c128 / c256    fp32: items 512 (S 2) / 1024 (S 1)                            16-bit: 256 (S 4) / 512 (S 2)
#   ragged_rows    B * H = 301 input rows: with the workspace rows_per_block = ceil(301 / 256) = 2, 151 workgroups, the last one holds a single row;
#                  W = 3 < S as well
UPSAMPLE_BWD_CASES = {
    "unrolled_w19": (2, 64, 2, 3, 19),
    "unrolled_w35": (2, 64, 2, 3, 35),
    "tail_only": (1, 64, 2, 2, 3),
    "items_1024": (1, 64, 4, 3, 5),
    "multi_pass": (1, 64, 8, 2, 3),
    "c128": (1, 128, 2, 3, 7),
    "c256": (1, 256, 2, 3, 7),
    "ragged_rows": (7, 64, 2, 43, 3),
}
UPSAMPLE_BWD_RANDN = (2, 64, 2, 6, 10)
UPSAMPLE_BWD_BAD_ITEMS = ("fp32", 1, 24, 2, 3, 5)         # 16 taps x 6 chunks = 96: not a power of two -> argument error, nothing launched


def dw_plan(dt, B, C, f, H, W, workspace, deterministic=False):
    """The launch arithmetic of upsample_bwd_impl / upsample_bwd_dw_kernel (csrc/train_kernels.hip), restated."""
    E = CHUNK[dt]
    k, p = 2 * f, f // 2
    taps, CG = k * k, C // E
    items = taps * CG
    S = 1 if items >= 1024 else 1024 // items
    nrows = B * H
    rpb = (nrows + 255) // 256 if workspace else (nrows if deterministic else (2 if nrows >= 1024 else 1))
    blocks = (nrows + rpb - 1) // rpb
    unrolled = tail = idle = 0                            # (kw, column group) pairs that run the unrolled loop / reach the tail loop / own no column
    for kw in range(k):
        iw_lo, iw_hi = max(0, (p - kw + f - 1) // f), min(W - 1, (W * f - 1 + p - kw) // f)
        for grp in range(S):
            iw = iw_lo + grp
            if iw > iw_hi:
                idle += 1
                continue
            n4 = 0
            while iw + 3 * S <= iw_hi:
                iw += 4 * S
                n4 += 1
            unrolled += n4 > 0
            tail += iw <= iw_hi
    return dict(items=items, S=S, passes=max(1, items // 1024), pow2=items & (items - 1) == 0, rows_per_block=rpb, blocks=blocks,
                last_block_rows=nrows - (blocks - 1) * rpb, unrolled=unrolled, tail=tail, idle=idle)


def upsample_bwd_inputs(dt, B, C, f, H, W, seed, randn=False):
    """NCHW float64 (x, w, skip, dy); the activations are numbers of the dtype."""
    if randn:
        g = _gen(seed)
        td = TORCH_DTYPE[dt]
        x = torch.randn(B, C, H, W, generator=g).to(td).double()
        w = torch.rand(C, 1, 2 * f, 2 * f, generator=g).double()
        skip = torch.randn(B, C, H * f, W * f, generator=g).to(td).double()
        dy = torch.randn(B, C, H * f, W * f, generator=g).to(td).double()
        return x, w, skip, dy
    return (dyadic((B, C, H, W), seed), tap_weights(C, f, seed + 1), dyadic((B, C, H * f, W * f), seed + 2),
            dyadic((B, C, H * f, W * f), seed + 3, nonzero=True))


# ---- 6. zero insertion: (B, Ho, Wo, C, H, W) -----------------------------------------------------------------------------------
# H = 2 Ho and H = 2 Ho - 1 (the stride-2 conv of an even / odd map), the same for W
ZERO_INSERT_CASES = [(2, 3, 4, "chunk", 6, 8), (1, 19, 35, 64, 37, 69), (1, 18, 35, 32, 36, 70)]

# ---- 7. column sums: (M, C, ld, dtypes) ------------------------------------------------------------------------------------------
# chunk route (colsum_chunk_kernel): C a power-of-two number of chunks and ld a multiple of the chunk; generic route (colsum_kernel) otherwise:
#   (500, 27)  odd C            (129, 3)  M just over one 128-row workgroup       (777, 24)  6 chunks in fp32
#   (300, 96)  24 / 12 chunks, C > 64: two channel blocks, the second half empty
#   (2^18 + 5, 3 chunks)  M >= 2^18: 1024 rows per workgroup, ragged last one
COLSUM_CHUNK_CASES = [(1, 64, 64, DTYPES), (1000, 64, 64, DTYPES), (4097, 256, 256, DTYPES), (333, 32, 64, DTYPES)]
COLSUM_GENERIC_CASES = [(500, 27, 27, ("fp32",)), (129, 3, 3, ("fp32",)), (777, 24, 24, ("fp32",)), (300, 96, 96, DTYPES),
                        ((1 << 18) + 5, "chunk3", "chunk3", DTYPES)]
COLSUM_DETERMINISTIC_CASES = [(1000, 64, 64, DTYPES), (300, 96, 96, DTYPES)]
COLSUM_RANDN = (1000, 64, 64)


def colsum_route(dt, C, ld):
    E = CHUNK[dt]
    return "chunk" if C % E == 0 and ld % E == 0 and C // E <= 256 and 256 % (C // E) == 0 else "generic"


def colsum_input(M, C, ld, seed):
    """(M, ld) float64: multiples of 1/8 with |v| <= 2 in the first C columns, 1024 in the padding columns [C, ld) (never summed)."""
    x = torch.full((M, ld), 1024.0, dtype=torch.float64)
    x[:, :C] = dyadic((M, C), seed, bound=2.0)
    return x


# ---- 8. edge scatter-add ---------------------------------------------------------------------------------------------------------
EDGE = dict(B=3, L=16, H=6, W=10, ld_out=64, ldv=4, edge_len=[0, 16, 7], canary_pixel=(9, 5))
EDGE_CASES = [(0, 3, False), (0, 3, True), (5, 2, False), (5, 2, True)]          # (ch_off, C, planar)


def edge_inputs(seed):
    """-> out (B, H, W, ld_out) fp32, v (B, L, ldv) fp32, edge_xy (B, L, 2) int32 (x, y), edge_len (B,) int32.  Inside each image's prefix the points
    are distinct and avoid the canary pixel; every ignored point (j >= edge_len[b]) IS the canary pixel -- in range, so a kernel that forgets
    edge_len fails the comparison instead of faulting."""
    e = EDGE
    g = _gen(seed)
    out = dyadic((e["B"], e["H"], e["W"], e["ld_out"]), seed + 1).float()
    v = dyadic((e["B"], e["L"], e["ldv"]), seed + 2, nonzero=True).float()
    cx, cy = e["canary_pixel"]
    xy = torch.empty((e["B"], e["L"], 2), dtype=torch.int32)
    xy[..., 0], xy[..., 1] = cx, cy
    for b, n in enumerate(e["edge_len"]):
        pix = [i for i in torch.randperm(e["H"] * e["W"], generator=g).tolist() if i != cy * e["W"] + cx][:n]
        for j, i in enumerate(pix):
            xy[b, j, 0], xy[b, j, 1] = i % e["W"], i // e["W"]
    return out, v, xy, torch.tensor(e["edge_len"], dtype=torch.int32)


# ---- bounds ------------------------------------------------------------------------------------------------------------------------

def exact_terms_bound(n_terms, term_max, term_step):
    """True if every partial sum of n_terms numbers that are multiples of term_step with |t| <= term_max is an fp32 number (< 2^24 steps)."""
    return n_terms * term_max / term_step < 2 ** 24


def randn_bound(ref, abs_sum, n_terms, dt):
    """Per-element bound of a `randn` case: one rounding of the output (u |ref|, + the fp16 subnormal spacing) and an fp32 sum of n_terms products in any
    order ((n + 1) 2^-24 S, S = the float64 sum of the absolute values of the element's terms)."""
    return UNIT_ROUNDOFF[dt] * ref.abs() + (n_terms + 1) * 2.0 ** -24 * abs_sum + ABS_FLOOR[dt]
