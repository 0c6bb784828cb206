"""Engineered inputs for the tile-owned DCN backward (tests/test_dcn_bwd_ref_cpu.py, tests/test_gpu_dcn_bwd_edges.py): offset fields that put
every sample exactly where a limit of dcn_bwd_tile.hip is -- the near / far seam of the 8-pixel ring, the capacity of a pixel's LDS list, the
capacity of a workgroup's far stage, the border band and the exact coordinates -1 / H -- instead of drawing them.

All offsets and masks are multiples of 1/4, so the kernel's fp32 coordinates are exact.  x and dy are integers / 8 in [-3/8, 1], w integers / 16 in
[-3/16, 1/2]: exact in bf16, fp16 and fp32 alike, so the operands are the same numbers in every type.  The values lean positive on purpose: the sums
do not cancel to nothing, so the magnitude map M of the error model stays within a small factor of |reference| and a pair that is dropped or counted
twice moves an element by a visible share of its bound.

A case is (name, B, C, Cout, H, W, om); `inputs(case)` adds x, w, dy.  Nothing here is random at test time: torch.Generator with fixed seeds."""
import functools
from collections import namedtuple

import torch

Case = namedtuple("Case", "name B C Cout H W om")

ROW_SHIFTS = (7.5, 8.0, 8.25, 9.0, -8.0, -9.0)                    # each with 0.25 on the columns
COL_SHIFTS = (8.0, 8.5, 9.0, 16.25, 24.0, -8.0, -9.0, -17.5)      # each with 0.5 on the rows
# On the 16 x 32 map every row lies within 8 pixels of both tile rows, so the row shifts above move corners across a tile edge but can never make a
# pair "far" there; the tall map (32 x 32: four tile rows) is where a row shift walks the near / far seam, and 17 rows is the row shift that
# overflows a workgroup's far stage (a 9-row shift reaches at most 3 of a tile's 8 rows x 16 columns x 3 taps x 2 corners = 288 far pairs).
TALL_ROW_SHIFTS = ROW_SHIFTS + (17.0,)
BORDER_MASKS = (0.0, 0.25, 0.5, 1.0)


def _mask_field(B, H, W):
    b, y, x, k = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(W), torch.arange(9), indexing="ij")
    return 0.25 * (1 + (b + y + 2 * x + k) % 4).float()


def translate_field(B, H, W, s_h, s_w):
    """Every tap of every pixel shifted by (s_h, s_w); masks 1/4 .. 1."""
    om = torch.zeros(B, H, W, 32)
    om[..., 0:18:2] = s_h
    om[..., 1:18:2] = s_w
    om[..., 18:27] = _mask_field(B, H, W)
    return om


def _tap_pos(H, W):
    y, x, k = torch.meshgrid(torch.arange(H), torch.arange(W), torch.arange(9), indexing="ij")
    return (y - 1 + k // 3).float(), (x - 1 + k % 3).float()


def focus_field(B, H, W, y_star, x_star, block):
    """All nine taps of the block x block pixels whose top-left pixel is (y_star - (block - 1) // 2, x_star - (block - 1) // 2) aim at
    (y_star + 0.5, x_star + 0.5) with mask 1: 9 block^2 pairs of weight 1/4 on each of the four pixels around the point.  Elsewhere: a quarter-pixel
    row offset and no column offset (two corners per sample, 18 pairs per pixel), masks 1/4 .. 1."""
    om = torch.zeros(B, H, W, 32)
    b, y, x, k = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(W), torch.arange(9), indexing="ij")
    om[..., 0:18:2] = 0.25 * (1 + (y + x + k + b) % 3).float()
    om[..., 18:27] = _mask_field(B, H, W)
    py, px = _tap_pos(H, W)
    y0, x0 = y_star - (block - 1) // 2, x_star - (block - 1) // 2
    assert y0 >= 0 and x0 >= 0 and y0 + block <= H and x0 + block <= W
    sl = (slice(None), slice(y0, y0 + block), slice(x0, x0 + block))
    om[sl + (slice(0, 18, 2),)] = (y_star + 0.5) - py[y0:y0 + block, x0:x0 + block]
    om[sl + (slice(1, 18, 2),)] = (x_star + 0.5) - px[y0:y0 + block, x0:x0 + block]
    om[sl + (slice(18, 27),)] = 1.0
    return om


def border_targets(n):
    """Coordinates along an axis of length n: the eight border values and two interior ones (integral: two corners of weight zero; half-way)."""
    return (-1.0, -0.75, -0.25, 0.0, 3.0, 4.5, n - 1.0, n - 0.75, n - 0.25, float(n))


def border_field(B, H, W):
    """Sample number i = (pixel, tap) goes to row target i % 10 and column target (i // 10) % 10 with mask (i // 100) % 4 of BORDER_MASKS: every
    (row target, column target, mask) triple occurs in every 400 consecutive samples; images start at different i."""
    om = torch.zeros(B, H, W, 32)
    py, px = _tap_pos(H, W)
    rows, cols, masks = torch.tensor(border_targets(H)), torch.tensor(border_targets(W)), torch.tensor(BORDER_MASKS)
    i0 = torch.arange(H * W * 9).view(H, W, 9)
    for b in range(B):
        i = i0 + 137 * b
        om[b, :, :, 0:18:2] = rows[i % 10] - py
        om[b, :, :, 1:18:2] = cols[(i // 10) % 10] - px
        om[b, :, :, 18:27] = masks[(i // 100) % 4]
    return om


def _fmt(v):
    return ("%g" % v).replace("-", "m").replace(".", "p")


@functools.lru_cache(maxsize=None)
def all_cases():
    c = []
    for s in ROW_SHIFTS:
        c.append(Case("translate_rows_%s" % _fmt(s), 2, 64, 64, 16, 32, translate_field(2, 16, 32, s, 0.25)))
    for s in COL_SHIFTS:
        c.append(Case("translate_cols_%s" % _fmt(s), 2, 64, 64, 16, 32, translate_field(2, 16, 32, 0.5, s)))
    for s in TALL_ROW_SHIFTS:
        c.append(Case("translate_tall_rows_%s" % _fmt(s), 2, 64, 64, 32, 32, translate_field(2, 32, 32, s, 0.25)))
    c.append(Case("focus16_mid", 2, 64, 64, 16, 32, focus_field(2, 16, 32, 3, 7, 3)))
    c.append(Case("focus16_corner", 2, 64, 64, 16, 32, focus_field(2, 16, 32, 7, 15, 3)))
    c.append(Case("focus32_mid", 2, 64, 64, 16, 32, focus_field(2, 16, 32, 3, 7, 8)))
    c.append(Case("focus32_corner", 2, 64, 64, 16, 32, focus_field(2, 16, 32, 7, 15, 8)))
    c.append(Case("border_9x17", 2, 64, 64, 9, 17, border_field(2, 9, 17)))
    c.append(Case("border_9x32", 2, 64, 64, 9, 32, border_field(2, 9, 32)))
    for C, Cout, H, W in ((128, 64, 9, 32), (256, 128, 9, 20)):
        tag = "wide%d_%dx%d" % (C, H, W)
        c.append(Case("%s_translate_cols_9" % tag, 2, C, Cout, H, W, translate_field(2, H, W, 0.5, 9.0)))
        c.append(Case("%s_translate_cols_16p25" % tag, 2, C, Cout, H, W, translate_field(2, H, W, 0.5, 16.25)))
        c.append(Case("%s_border" % tag, 2, C, Cout, H, W, border_field(2, H, W)))
    return {k.name: k for k in c}


def case(name):
    return all_cases()[name]


def names(prefix):
    return [n for n in all_cases() if n.startswith(prefix)]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """x (B,H,W,C), om, w (Cout,C,3,3), dy (B,H,W,Cout) as float32 tensors whose values are exact in bf16 and fp16."""
    k = case(name)
    g = torch.Generator().manual_seed(1000 + sorted(all_cases()).index(name))
    x = torch.randint(-3, 9, (k.B, k.H, k.W, k.C), generator=g).float() / 8
    dy = torch.randint(-3, 9, (k.B, k.H, k.W, k.Cout), generator=g).float() / 8
    w = torch.randint(-3, 9, (k.Cout, k.C, 3, 3), generator=g).float() / 16
    if name.startswith("focus16"):
        # no negative values: |reference| = M at every element.  With 20 to 30 of a focus pixel's ~90 pairs arriving through packed 16-bit atomics the
        # bound is dominated by n_atomic u_out M, and a reference without those pairs stays 2x beyond it only if the sum does not cancel
        x, w, dy = x.abs(), w.abs(), dy.abs()
    return x, k.om, w, dy
