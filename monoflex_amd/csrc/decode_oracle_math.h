// `output_depth = 'oracle'`: which depth estimate a detection takes, given its image's ground truth.  The only statement of the rule
// (reference get_oracle_depths, model/head/detector_infer.py:239-278; box_iou, engine/visualize_infer.py:23-27), exactly as
// PostProcessor.decode_oracle serves it on the host.  decode_multi.hip runs choose() per detection on a table staged in LDS;
// tests/shim/decode_oracle_host.cpp compiles it for the host.  float32 throughout, plain functions of one detection and one table, no
// HIP-only constructs.
//
// The distance, IoU and depth-difference expressions are evaluated WITHOUT fused multiply-add contraction (the pragma below, in each
// function): they then have the float32 values torch and numpy produce on the host, whatever flags the translation unit is compiled with.
#pragma once
#include <cmath>
#include <cstddef>

#include "hd.h"

#if defined(__clang__)
#define MFX_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define MFX_NO_CONTRACT                                            // (the host shim is compiled with -ffp-contract=off)
#endif

namespace mfx {
namespace dorc {

// one ground-truth slot: fp32 [8] = reg_mask, cls_id, x1, y1, x2, y2, depth, 0.  Slots with reg_mask != 0 take part, in slot order (the
// order of the reference's masked tensors).
enum { G_MASK = 0, G_CLS = 1, G_BOX = 2, G_DEPTH = 6, GT_ROW = 8 };
constexpr int MAX_GT = 128;                                        // slots per image the kernel stages (DATASETS.MAX_OBJECTS is 40)
constexpr float OTHER_CLASS_DIS = 9999.f;                          // the reference's literal: `dis[target_clses != pred_cls] = 9999`
constexpr float MATCH_IOU = 0.5f;

// box_iou (visualize_infer.py:23-27) in float32: max(x, 0) as Python evaluates it (a NaN stays a NaN), no +1, 0 / 0 = NaN
MFX_HD float iou_2d(const float* a, const float* b) {
    MFX_NO_CONTRACT
    const float dw = fminf(a[2], b[2]) - fmaxf(a[0], b[0]), dh = fminf(a[3], b[3]) - fmaxf(a[1], b[1]);
    const float inter = (0.f > dw ? 0.f : dw) * (0.f > dh ? 0.f : dh);
    const float area_a = (a[2] - a[0]) * (a[3] - a[1]), area_b = (b[2] - b[0]) * (b[3] - b[1]);
    return inter / ((area_a + area_b) - inter);
}

// squared distance of the box centres (x1 + x2) / 2, (y1 + y2) / 2 (:256-259)
MFX_HD float centre_dis(const float* a, const float* b) {
    MFX_NO_CONTRACT
    const float dx = (a[0] + a[2]) / 2.f - (b[0] + b[2]) / 2.f, dy = (a[1] + a[3]) / 2.f - (b[1] + b[3]) / 2.f;
    const float dx2 = dx * dx, dy2 = dy * dy;
    return dx2 + dy2;
}

// The slot a detection is tested against: the first minimum, over the valid slots in slot order, of the centre distance -- REPLACED by
// 9999 where the slot's class differs (:260-261).  So with no object of the class the first valid slot is "nearest", and a same-class
// object farther than sqrt(9999) px loses to an earlier other-class slot.  -1: the table has no valid slot.
MFX_HD int nearest_slot(const float* box, int cls, const float* gt, int M) {
    int near = -1;
    float best = 0.f;
    for (int g = 0; g < M; ++g) {
        const float* t = gt + (size_t)g * GT_ROW;
        if (t[G_MASK] == 0.f) continue;
        const float dis = (int)t[G_CLS] != cls ? OTHER_CLASS_DIS : centre_dis(box, t + G_BOX);
        if (near < 0 || dis < best) { near = g; best = dis; }
    }
    return near;
}

// first minimum of |d[c] - target| over the columns c = first .. 3 (:272-273)
MFX_HD int closest_column(const float* d, int first, float target) {
    MFX_NO_CONTRACT
    int col = -1;
    float best = 0.f;
    for (int c = 0; c < 4; ++c) {                                  // (fixed trip count: d[] stays in registers on the device)
        const float v = fabsf(d[c] - target);
        if (c >= first && (col < 0 || v < best)) { best = v; col = c; }
    }
    return col;
}

// One detection (2D box x1, y1, x2, y2, class, score; d[4] = its direct, keypoint-centre, 02, 13 depths) against one image's table of M
// slots.  -> -1: the detection keeps the 'mean' row (score below the threshold, no valid slot, or unmatched: IoU with the nearest slot
// < 0.5 -- a NaN IoU is not, :268-270); else the column 0..3 whose single-estimate row it takes (0 = direct, offered only with
// depth_uncertainty: the reference's pred_combined_depths has three columns without it, :177-182).
MFX_HD int choose(const float* box, int cls, float score, float threshold, const float* d, bool has_direct, const float* gt, int M) {
    if (!(score >= threshold)) return -1;
    const int near = nearest_slot(box, cls, gt, M);
    if (near < 0) return -1;
    const float* t = gt + (size_t)near * GT_ROW;
    if (iou_2d(box, t + G_BOX) < MATCH_IOU) return -1;
    return closest_column(d, has_direct ? 0 : 1, t[G_DEPTH]);
}

}  // namespace dorc
}  // namespace mfx
