"""Explicit float64 restatement of the DCNv2 backward that monoflex_amd/csrc/dcn_bwd_tile.hip computes (3x3 / stride 1 / pad 1 / dilation 1, one
deformable group), and a census of the routes a (sample, corner) pair can take through dcn_bwd_tile_kernel.  TEST INFRASTRUCTURE: plain torch float64
on the CPU, no autograd -- every gradient is written out, because the error model of tests/test_gpu_dcn_bwd_edges.py needs the SAME sums with every
factor replaced by its absolute value (the magnitude maps M).

Layout, as the kernel consumes it: x (B,H,W,C), om (B,H,W,32) = [2k] dh, [2k+1] dw of tap k, [18+k] the post-sigmoid mask, 27..31 padding,
w (Cout,C,3,3), dy (B,H,W,Cout).  Outputs dx (B,H,W,C), d_raw (B,H,W,32), dw (Cout,C,3,3), db (Cout).

The rule (monoflex_amd/csrc/dcn_sample_math.h; the reference's modulated_deformable_col2im / _col2im_coord):
  * coordinate: the kernel's fp32 value (float)(o - 1 + t) + d, widened to float64 -- the corner pair and the one-sided derivative depend on it;
  * inside is strict on both sides: a sample at exactly h = -1 or h = H adds nothing to ANY gradient, its own offset gradient included (zero-padded
    bilinear interpolation has a non-zero d/dh there: that shortcut is not this rule);
  * the corner pair is floor() of the coordinate itself; at an integral coordinate the derivative is the one-sided one of that pair;
  * a corner outside the map adds nothing;
  * d_raw[0:18] = offset gradient with the mask folded in, d_raw[18:27] = gradient of the mask LOGIT = d mask * m (1 - m), d_raw[27:32] = 0.

`strict_inside=False` is the deliberately wrong rule of a tooth (h >= -1, h <= H): never a reference.

Census (`census`): a property of the INPUTS, restating the binning rule of dcn_bwd_tile_kernel phase 1 in integer arithmetic -- 8 x 16 tiles, ring D;
the pair (sample m, corner pixel p) is "near" iff m lies in tile(p) grown by D pixels, and then goes to p's LDS list (route 1) while the list has
room; a far pair is reported by the workgroup of m's own tile into its stage of BT_FCAP entries (route 2) or, once that is full, one by one
(route 3); a near pair beyond the list's capacity takes the same stage.  Pairs of weight zero and samples of mask zero are skipped by the kernel
and are not counted.  The census says nothing about what the kernel did."""
import os
import re

import torch

D64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "monoflex_amd", "csrc", "dcn_bwd_tile.hip")
TILE_H, TILE_W = 8, 16


def kernel_constants(path=SOURCE):
    """The five limits of dcn_bwd_tile.hip, from its source text: ring, stage capacity, list capacities (16-bit, gcol-free 16-bit, fp32)."""
    with open(path) as f:
        src = f.read()

    def one(pattern):
        found = re.findall(pattern, src, flags=re.M | re.S)
        assert len(found) == 1, "dcn_bwd_tile.hip: %d matches of %r" % (len(found), pattern)
        return int(found[0])

    c = dict(BT_D_VAL=one(r"^#define\s+BT_D_VAL\s+(\d+)"), BT_FCAP=one(r"constexpr\s+int\s+BT_FCAP\s*=\s*(\d+)\s*;"),
             BT_LCAP_BF16=one(r"^#define\s+BT_LCAP_BF16\s+(\d+)"), FZ_LCAP=one(r"constexpr\s+int\s+FZ_LCAP\s*=\s*(\d+)\s*;"),
             LCAP_F32=one(r"struct\s+BtEntry<float>\s*\{.*?static\s+constexpr\s+int\s+LCAP\s*=\s*(\d+)\s*;"))
    th, tw = one(r"constexpr\s+int\s+BT_TH\s*=\s*(\d+)\s*,"), one(r"BT_TW\s*=\s*(\d+)\s*,")
    assert (th, tw) == (TILE_H, TILE_W), "the census assumes 8 x 16 tiles"
    return c


def geometry(om, H, W, strict_inside=True):
    """Per (b, y, x, tap): the fp32 coordinate widened to float64, inside, mask; per corner q = 0..3 (row q >> 1, column q & 1): pixel, unmodulated
    weight, coefficient of d/dh and d/dw (dcns::coord_weights), and whether the corner exists."""
    B = om.shape[0]
    om32 = om.to(torch.float32)
    ys = torch.arange(H, dtype=torch.float32).view(1, H, 1, 1)
    xs = torch.arange(W, dtype=torch.float32).view(1, 1, W, 1)
    th = torch.tensor([k // 3 for k in range(9)], dtype=torch.float32).view(1, 1, 1, 9)
    tw = torch.tensor([k % 3 for k in range(9)], dtype=torch.float32).view(1, 1, 1, 9)
    h = ((ys - 1 + th) + om32[..., 0:18:2]).to(D64)                      # fp32 sum, as dcns::pos3x3
    w = ((xs - 1 + tw) + om32[..., 1:18:2]).to(D64)
    h, w = h.expand(B, H, W, 9), w.expand(B, H, W, 9)
    mask = om[..., 18:27].to(D64)
    if strict_inside:
        inside = (h > -1) & (w > -1) & (h < H) & (w < W)
    else:
        inside = (h >= -1) & (w >= -1) & (h <= H) & (w <= W)
    h0, w0 = torch.floor(h), torch.floor(w)
    lh, lw = h - h0, w - w0
    hh, hw = 1 - lh, 1 - lw
    hc = torch.stack((h0, h0, h0 + 1, h0 + 1), -1).long()
    wc = torch.stack((w0, w0 + 1, w0, w0 + 1), -1).long()
    wt = torch.stack((hh * hw, hh * lw, lh * hw, lh * lw), -1)
    ch = torch.stack((-hw, -lw, hw, lw), -1)
    cw = torch.stack((-hh, hh, -lh, lh), -1)
    exists = inside.unsqueeze(-1) & (hc >= 0) & (hc < H) & (wc >= 0) & (wc < W)
    return dict(h=h, w=w, inside=inside, mask=mask, hc=hc, wc=wc, wt=wt, ch=ch, cw=cw, exists=exists)


def _pixel_index(g, B, H, W):
    b = torch.arange(B).view(B, 1, 1, 1, 1)
    return (b * H * W + g["hc"].clamp(0, H - 1) * W + g["wc"].clamp(0, W - 1)).expand(B, H, W, 9, 4)


def scatter_pairs(g, gcol, select=None):
    """sum over the (sample, tap, corner) pairs in `select` (B,H,W,9,4 bool; None = every existing pair) of weight * mask * gcol[sample, tap, :],
    added at the corner's pixel: grad_input, or the part of it a set of pairs carries."""
    B, H, W = gcol.shape[:3]
    C = gcol.shape[-1]
    coef = g["wt"] * g["mask"].unsqueeze(-1) * g["exists"].to(D64)
    if select is not None:
        coef = coef * select.to(D64)
    idx = _pixel_index(g, B, H, W)
    out = torch.zeros(B * H * W, C, dtype=D64)
    for k in range(9):
        for q in range(4):
            out.index_add_(0, idx[:, :, :, k, q].reshape(-1), (coef[:, :, :, k, q].unsqueeze(-1) * gcol[:, :, :, k, :]).reshape(-1, C))
    return out.view(B, H, W, C)


def census(om, H, W, consts=None):
    """Counts from the inputs alone (see the module docstring).  Returns
         pairs   (B,H,W,9,4) bool: the pairs the kernel does not skip (corner exists, weight and mask non-zero)
         near    (B,H,W,9,4) bool: of them, those whose sample lies in the corner's tile grown by D
         near_pp (B,H,W) int: per TARGET pixel, the pairs that aim at it from the near window  (route 1 while <= the list capacity)
         far_pp  (B,H,W) int: per target pixel, the far pairs that aim at it                    (routes 2 / 3)
         far_pt  (B,ty,tx) int: per tile, the far pairs of its own samples                      (what its stage must take, list overflow aside)
         ring    (B,H,W,9,4) int: Chebyshev distance in pixels from the sample to the corner's tile (0 = inside it)"""
    c = consts or kernel_constants()
    D = c["BT_D_VAL"]
    B = om.shape[0]
    g = geometry(om, H, W)
    pairs = g["exists"] & (g["wt"] != 0) & (g["mask"] != 0).unsqueeze(-1)
    ty0, tx0 = (g["hc"].clamp(0, H - 1) // TILE_H) * TILE_H, (g["wc"].clamp(0, W - 1) // TILE_W) * TILE_W
    my = torch.arange(H).view(1, H, 1, 1, 1)
    mx = torch.arange(W).view(1, 1, W, 1, 1)
    dist_y = torch.maximum(torch.maximum(ty0 - my, my - (ty0 + TILE_H - 1)), torch.zeros((), dtype=torch.long))
    dist_x = torch.maximum(torch.maximum(tx0 - mx, mx - (tx0 + TILE_W - 1)), torch.zeros((), dtype=torch.long))
    ring = torch.maximum(dist_y, dist_x)
    near = pairs & (ring <= D)
    far = pairs & (ring > D)
    idx = _pixel_index(g, B, H, W).reshape(-1)
    near_pp = torch.zeros(B * H * W, dtype=torch.long).index_add_(0, idx, near.reshape(-1).long()).view(B, H, W)
    far_pp = torch.zeros(B * H * W, dtype=torch.long).index_add_(0, idx, far.reshape(-1).long()).view(B, H, W)
    nty, ntx = (H + TILE_H - 1) // TILE_H, (W + TILE_W - 1) // TILE_W
    b = torch.arange(B).view(B, 1, 1, 1, 1)
    tidx = ((b * nty + my // TILE_H) * ntx + mx // TILE_W).expand(B, H, W, 9, 4).reshape(-1)
    far_pt = torch.zeros(B * nty * ntx, dtype=torch.long).index_add_(0, tidx, far.reshape(-1).long()).view(B, nty, ntx)
    return dict(pairs=pairs, near=near, far=far, near_pp=near_pp, far_pp=far_pp, far_pt=far_pt, ring=ring, geometry=g)


def n_atomic(cen, lcap):
    """Contributions that reach a pixel of grad_input through atomics: its far pairs and the near pairs beyond its list's capacity."""
    return cen["far_pp"] + (cen["near_pp"] - lcap).clamp(min=0)


def stage_load(cen, lcap):
    """Per tile: what its workgroup hands to_far() -- the far pairs of its own samples plus the pairs beyond the capacity of its pixels' lists."""
    B, H, W = cen["near_pp"].shape
    over = (cen["near_pp"] - lcap).clamp(min=0)
    nty, ntx = cen["far_pt"].shape[1:]
    pad = torch.zeros(B, nty * TILE_H, ntx * TILE_W, dtype=torch.long)
    pad[:, :H, :W] = over
    return cen["far_pt"] + pad.view(B, nty, TILE_H, ntx, TILE_W).sum(dim=(2, 4))


def ragged_own(cen, H, W):
    """Pairs of a sample that land in its OWN tile where that tile hangs over the map's edge (the part of an edge tile that exists)."""
    g = cen["geometry"]
    my, mx = torch.arange(H).view(1, H, 1, 1, 1), torch.arange(W).view(1, 1, W, 1, 1)
    own = (g["hc"] // TILE_H == my // TILE_H) & (g["wc"] // TILE_W == mx // TILE_W)
    ragged = ((g["hc"] // TILE_H + 1) * TILE_H > H) | ((g["wc"] // TILE_W + 1) * TILE_W > W)
    return cen["pairs"] & own & ragged


def beyond_capacity(cen, lcap):
    """One choice of the pairs a list of `lcap` entries cannot hold: per over-full pixel, its near pairs after the first `lcap` in sample order (the
    kernel's choice depends on arrival order; any choice is the same NUMBER of pairs)."""
    B, H, W = cen["near_pp"].shape
    g = cen["geometry"]
    idx = _pixel_index(g, B, H, W)
    sel = torch.zeros_like(cen["near"])
    flat = sel.view(-1)
    for p in torch.nonzero(cen["near_pp"].view(-1) > lcap).view(-1).tolist():
        members = torch.nonzero((cen["near"] & (idx == p)).view(-1)).view(-1)
        flat[members[lcap:]] = True
    return sel


def backward(x, om, w, dy, strict_inside=True):
    """The four gradients in float64 and, next to each, its magnitude map M (the same sum over absolute values).  Also returns the geometry and
    d(columns) so that a caller can take the part of dx a set of pairs carries (scatter_pairs)."""
    x, om, w, dy = x.to(D64), om.to(D64), w.to(D64), dy.to(D64)
    B, H, W, C = x.shape
    Cout = w.shape[0]
    g = geometry(om, H, W, strict_inside)
    wk = w.reshape(Cout, C, 9)
    gcol = torch.einsum("bhwo,ock->bhwkc", dy, wk)                        # d(columns)[m][tap][c]
    gcol_a = torch.einsum("bhwo,ock->bhwkc", dy.abs(), wk.abs())
    xf, xa = x.reshape(B * H * W, C), x.abs().reshape(B * H * W, C)
    idx = _pixel_index(g, B, H, W)
    ex = g["exists"].to(D64)
    mask = g["mask"]
    val = torch.zeros(B, H, W, 9, C, dtype=D64)
    val_a, bh, bh_a, bw, bw_a = (torch.zeros_like(val) for _ in range(5))
    for q in range(4):
        xq = xf[idx[..., q].reshape(-1)].view(B, H, W, 9, C) * ex[..., q].unsqueeze(-1)
        xqa = xa[idx[..., q].reshape(-1)].view(B, H, W, 9, C) * ex[..., q].unsqueeze(-1)
        val += g["wt"][..., q].unsqueeze(-1) * xq
        val_a += g["wt"][..., q].unsqueeze(-1) * xqa
        bh += g["ch"][..., q].unsqueeze(-1) * xq
        bh_a += g["ch"][..., q].abs().unsqueeze(-1) * xqa
        bw += g["cw"][..., q].unsqueeze(-1) * xq
        bw_a += g["cw"][..., q].abs().unsqueeze(-1) * xqa
    ins = g["inside"].to(D64)
    d_raw = torch.zeros(B, H, W, 32, dtype=D64)
    m_raw = torch.zeros_like(d_raw)
    d_raw[..., 0:18:2] = mask * ins * (gcol * bh).sum(-1)
    m_raw[..., 0:18:2] = mask * ins * (gcol_a * bh_a).sum(-1)
    d_raw[..., 1:18:2] = mask * ins * (gcol * bw).sum(-1)
    m_raw[..., 1:18:2] = mask * ins * (gcol_a * bw_a).sum(-1)
    sig = mask * (1 - mask)
    d_raw[..., 18:27] = sig * ins * (gcol * val).sum(-1)
    m_raw[..., 18:27] = sig.abs() * ins * (gcol_a * val_a).sum(-1)
    col, col_a = mask.unsqueeze(-1) * val, mask.unsqueeze(-1) * val_a        # modulated columns
    dw = torch.einsum("bhwo,bhwkc->ock", dy, col).reshape(Cout, C, 3, 3)
    m_dw = torch.einsum("bhwo,bhwkc->ock", dy.abs(), col_a).reshape(Cout, C, 3, 3)
    db, m_db = dy.sum(dim=(0, 1, 2)), dy.abs().sum(dim=(0, 1, 2))
    dx, m_dx = scatter_pairs(g, gcol), scatter_pairs(g, gcol_a)
    return dict(dx=dx, d_raw=d_raw, dw=dw, db=db, M=dict(dx=m_dx, d_raw=m_raw, dw=m_dw, db=m_db), geometry=g, gcol=gcol, gcol_abs=gcol_a)
