// The bilinear sampling rule of the modulated deformable convolution (DCNv2): the geometry of ONE (output pixel, tap) sample.
//
// Reference: dmcn_im2col_bilinear and the `inside` test of modulated_deformable_im2col (src/cuda/dcn_v2_im2col_cuda.cu:25-54,
// 178-189), dmcn_get_coordinate_weight (:82-122); restated for the CPU by oracle/dcn_v2_ref.c.  The rule:
//   position   h = (o_h * stride_h - pad_h + t_h * dil_h) + dh,  w likewise            (integer tap position + learned offset)
//   inside     h > -1 && w > -1 && h < H && w < W                                       (strict on both sides)
//   corners    (h0, w0) = floor(h, w), (h0, w0 + 1), (h0 + 1, w0), (h0 + 1, w0 + 1) -- order q = 0..3: row q >> 1, column q & 1
//   a corner exists iff the sample is inside and the corner lies in [0, H-1] x [0, W-1]; a corner that does not exist adds nothing
//   weights    hh * hw, hh * lw, lh * hw, lh * lw   with lh = h - h0, lw = w - w0, hh = 1 - lh, hw = 1 - lw
// The DCN kernels (forward: dcn_ps / dcn_patch / dcn_lds; backward: dcn_bwd / dcn_bwd_tile) take these
// steps from here and keeps only what is its own: the mask, the packing of the weights, addresses, the blend.  This header stops at
// geometry: every product below feeds a product at the site (`hh * hw * mask` is `(hh * hw) * mask` everywhere), never an add, so
// there is nothing here that could be contracted into an FMA differently from site to site.
//
// Float -> int conversion of the floor.  ONE way: clamp, then convert (`sample`).  A NaN or huge offset would otherwise overflow the
// conversion (undefined behaviour); fmaxf(NaN, lo) = lo.  The bounds LO = -24, HI = 30000 can be reached only by a sample that is
// not inside -- floor(h) < -1 or floor(h) >= H -- and such a sample has inside == false, no corner and weight zero at every site:
//   * dcn_ps, dcn_patch, dcn_lds (both forms), dcn_bwd_tile: 3x3 / stride 1 training and inference maps; dcn_bwd_tile refuses
//     H, W >= 4096 at launch, the forward maps are far below 30000 rows / columns (the bound these kernels have always had);
//   * dcn_patch and dcn_lds store the corner as (h0 + 32) | ((w0 + 32) << 16): needs -32 <= h0, w0 and w0 + 32 < 2^15 -- LO, HI fit;
//   * dcn_bwd_tile keeps window coordinates in 5 + 5 bits, but only of corners that passed the bounds test against H, W;
//   * LO <= -2 makes both rows (columns) of a clamped sample fail `0 <= h0 + 1`.
// dcn_bwd (the `_ext` boundary: any geometry, any map whose tensor is below 4 GB, so a row count above 30000 is legal) instantiates
// sample<kClampLo, kClampHiWide>: 2^30, because H * W * C * sizeof < 2^32 with C * sizeof >= 4 gives H, W < 2^30, and h0 + 1 cannot
// overflow.  It converted unclamped before.
// NOT moved: the two gather A-loaders, DcnALoader::tap_setup (conv_kernels.hip) and the geom lambda of dcn_wave_kernel, keep their own
// text (the same rule, unclamped conversion guarded by the later index clamp).  On this header they missed the resource gates:
// dcn_igemm_kernel<bf16 / fp16, 64, 128, 2, 2, 4> went from 96 / 94 to 98 VGPRs (4 -> 3 waves per SIMD), and the dcn_wave_kernel
// instantiations that already sit at 256 VGPRs gained 4..112 bytes of scratch (profiles/dcn_sample_math.md).
// `sample_inside` converts without the clamp; its precondition is that the caller has tested inside(h, w, H, W) first.
//
// Not taken from here, on purpose: the d/dh, d/dw blend of dcn_bwd_tile.hip (finish / the fused forms), which factors the corner
// differences (d10, d32) instead of using the four coefficients of coord_weights -- another order of additions, so moving it
// would change bits; it is a blend and stays at the site.
// box3d_iou_math.h-style: plain functions; tests/shim/dcn_sample_host.cpp compiles them for the host (tests/test_dcn_sample_math_cpu.py).
#pragma once
#include <cmath>

#include "hd.h"

namespace mfx {
namespace dcns {

// ---- the offset / mask row of one output pixel: 32 floats, [2k] = dh, [2k + 1] = dw of tap k (0..8), [18 + k] = mask, 27..31 padding
constexpr int kRow = 32, kMaskBase = 18;
MFX_HD constexpr int off_h(int k) { return 2 * k; }
MFX_HD constexpr int off_w(int k) { return 2 * k + 1; }
MFX_HD constexpr int mask_at(int k) { return kMaskBase + k; }

constexpr int kClampLo = -24, kClampHi = 30000, kClampHiWide = 1 << 30;

// ---- tap index -> (row, column)
struct Tap { int th, tw; };
MFX_HD Tap tap3x3(int tap) {                                       // 3x3: (tap * 11) >> 5 == tap / 3 for 0 <= tap <= 12
    const int th = (tap * 11) >> 5;
    return Tap{th, tap - th * 3};
}
MFX_HD Tap tap_of(int tap, int kw) {                               // general kernel width
    const int th = tap / kw;
    return Tap{th, tap - th * kw};
}

// ---- sample position along one axis: integer tap position (output index o, tap row / column t) + the learned offset
MFX_HD float pos(int o, int stride, int pad, int t, int dil, float d) { return (float)(o * stride - pad + t * dil) + d; }
MFX_HD float pos3x3(int o, int t, float d) { return (float)(o - 1 + t) + d; }      // stride 1, pad 1, dilation 1

MFX_HD bool inside(float h, float w, int H, int W) { return h > -1.f && w > -1.f && h < (float)H && w < (float)W; }

// ---- floor, fractions, integer top-left corner
struct Sample { float lh, lw, hh, hw; int h0, w0; };

template <int LO = kClampLo, int HI = kClampHi>
MFX_HD Sample sample(float h, float w) {
    const float hf = floorf(h), wf = floorf(w);
    Sample s;
    s.lh = h - hf; s.lw = w - wf; s.hh = 1.f - s.lh; s.hw = 1.f - s.lw;
    s.h0 = (int)fminf(fmaxf(hf, (float)LO), (float)HI);
    s.w0 = (int)fminf(fmaxf(wf, (float)LO), (float)HI);
    return s;
}
// precondition: inside(h, w, H, W) held, so -1 <= floor(h) < H and -1 <= floor(w) < W: the conversion cannot overflow
MFX_HD Sample sample_inside(float h, float w) {
    const float hf = floorf(h), wf = floorf(w);
    Sample s;
    s.lh = h - hf; s.lw = w - wf; s.hh = 1.f - s.lh; s.hw = 1.f - s.lw;
    s.h0 = (int)hf; s.w0 = (int)wf;
    return s;
}

// ---- the four corners, q = 0..3
MFX_HD int corner_h(const Sample& s, int q) { return s.h0 + (q >> 1); }
MFX_HD int corner_w(const Sample& s, int q) { return s.w0 + (q & 1); }
// a corner exists iff the sample is inside and the corner lies in the map.  An inside sample has -1 <= h0 <= H - 1, so the top row
// can only miss on the low side and the bottom row only on the high side (likewise the columns): the reference's own four tests
MFX_HD bool corner_valid(const Sample& s, bool inside_, int q, int H, int W) {
    const bool row = (q >> 1) ? s.h0 + 1 <= H - 1 : s.h0 >= 0;
    const bool col = (q & 1) ? s.w0 + 1 <= W - 1 : s.w0 >= 0;
    return inside_ && row && col;
}
// the full bounds test of a corner (hc, wc), for sites that walk corners of samples already known to be inside
MFX_HD bool in_map(int hc, int wc, int H, int W) { return hc >= 0 && hc < H && wc >= 0 && wc < W; }
// clamped indices: always addressable, whatever the sample
MFX_HD int clamp_idx(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }
// unmodulated weight of corner q
MFX_HD float corner_weight(const Sample& s, int q) { return ((q >> 1) ? s.lh : s.hh) * ((q & 1) ? s.lw : s.hw); }

// ---- backward: d(sample) / dh = sum_q ch[q] * v[q], d(sample) / dw = sum_q cw[q] * v[q]   (dmcn_get_coordinate_weight,
// dcn_v2_im2col_cuda.cu:82-122; v[q] = 0 for a corner that does not exist)
struct CoordWeights { float ch[4], cw[4]; };
MFX_HD CoordWeights coord_weights(const Sample& s) {
    return CoordWeights{{-s.hw, -s.lw, s.hw, s.lw}, {-s.hh, s.hh, -s.lh, s.lh}};
}

}  // namespace dcns
}  // namespace mfx
