// Validation diagnostics of one labelled object -- C ABI mfx_eval_diagnostics (eval_diag.hip maps one lane onto one object slot).
//
// Reference: PostProcessor.evaluate_3D_depths (model/head/detector_infer.py:280-359, TEST.EVAL_DEPTH) and evaluate_3D_detection (:361-452,
// TEST.EVAL_DIS_IOUS).  Both read the regression row at the object's TARGET centre and decode it with the TARGET class:
//   depth errors  the four depth estimates (direct, keypoint centre / 02 / 13) and their sigmas, the estimate of the smallest sigma, the
//                 1/sigma-weighted one, their mean and the best of the four, each as |estimate - Z_target| (13 values, DE_* below)
//   boxes         six rows (x, y, z, l, h, w, ry), y = the box centre: the predicted box, the target box, and four boxes in which ONE
//                 component (offset, depth, dimensions, orientation) is predicted and the rest is ground truth (BOX_* below)
//   IoUs          biou::iou_rows of boxes 0, 2, 3, 4, 5 with box 1 (pred_IoU, offset_IoU, depth_IoU, dims_IoU, orien_IoU)
// The decode is box_decode_math.h's (anno_encoder.py:124-295), the functions decode.hip `decode_boxes_kernel` runs; the tests pin the predicted
// box to that kernel's row of the same pixel and class.  The reference's evaluate_3D_detection only knows output_depth 'direct' (its other
// branches raise); for the other seven modes the predicted depth is bdec::combine's, as in that kernel.  Its get_iou3d never ran (NameError):
// the IoU is this library's own operator.
// float32 throughout.  box3d_iou_math.h-style: plain functions of one object; tests/shim compiles them for the host.
#pragma once
#include <cmath>

#include "../../include/monoflex_hip.h"
#include "box3d_iou_math.h"
#include "box_decode_math.h"

namespace mfx {
namespace ediag {
using namespace bdec;

constexpr int GT_ROW = MFX_EVAL_GT_ROW, NDEPTH = MFX_EVAL_DEPTH_KEYS, NIOU = MFX_EVAL_IOU_KEYS, NBOX = MFX_EVAL_BOXES;
// gt_rows columns
enum { G_MASK = 0, G_CLS, G_CX, G_CY, G_OFFX, G_OFFY, G_X, G_Y, G_Z, G_L, G_H, G_W, G_RY };
// depth_err columns, in the order of the reference's dict (detector_infer.py:341-357)
enum { DE_DIRECT = 0, DE_DIRECT_SIGMA, DE_KPT_CENTER, DE_KPT_02, DE_KPT_13, DE_KPT_CENTER_SIGMA, DE_KPT_02_SIGMA, DE_KPT_13_SIGMA,
       DE_SIGMA_MIN, DE_SIGMA_WEIGHTED, DE_MEAN, DE_MIN, DE_TARGET };
enum { BOX_PRED = 0, BOX_TARGET, BOX_OFFSET, BOX_DEPTH, BOX_DIMS, BOX_ORIEN };

// evaluate_3D_depths (detector_infer.py:314-357): needs all four estimates and sigmas
MFX_HD void depth_errors(const Estimates& e, float zt, float* out) {
    const float *d = e.d, *u = e.u;
    int amin = 0;                                                     // argmin of sigma, first of equals
    for (int i = 1; i < 4; ++i)
        if (u[i] < u[amin]) amin = i;
    float w[4];
    for (int i = 0; i < 4; ++i) w[i] = 1.f / u[i];
    const float ws = ((w[0] + w[1]) + w[2]) + w[3];
    float soft = 0.f, emin = 0.f;
    for (int i = 0; i < 4; ++i) {
        soft += d[i] * (w[i] / ws);
        const float err = fabsf(d[i] - zt);
        emin = i == 0 ? err : fminf(emin, err);
    }
    const float mean = (((d[0] + d[1]) + d[2]) + d[3]) / 4.f;
    out[DE_DIRECT] = fabsf(d[0] - zt); out[DE_DIRECT_SIGMA] = u[0];
    out[DE_KPT_CENTER] = fabsf(d[1] - zt); out[DE_KPT_02] = fabsf(d[2] - zt); out[DE_KPT_13] = fabsf(d[3] - zt);
    out[DE_KPT_CENTER_SIGMA] = u[1]; out[DE_KPT_02_SIGMA] = u[2]; out[DE_KPT_13_SIGMA] = u[3];
    out[DE_SIGMA_MIN] = fabsf(d[amin] - zt);
    out[DE_SIGMA_WEIGHTED] = fabsf(soft - zt);
    out[DE_MEAN] = fabsf(mean - zt);
    out[DE_MIN] = emin;
    out[DE_TARGET] = zt;
}

MFX_HD void put_box(float* o, const float* loc, const float* dims, float ry) {
    o[0] = loc[0]; o[1] = loc[1]; o[2] = loc[2]; o[3] = dims[0]; o[4] = dims[1]; o[5] = dims[2]; o[6] = ry;
}

// evaluate_3D_detection (detector_infer.py:377-442): the six boxes [6][7]
MFX_HD void build_boxes(const float* r, const float* g, const float* pdims, float pdepth, const Camera& c, const mfx_decode_cfg& dc,
                        const mfx_head_layout& hl, float* boxes) {
    const float px = (float)(int)g[G_CX], py = (float)(int)g[G_CY];
    const float pox = r[hl.ch[HK_OFF3D]], poy = r[hl.ch[HK_OFF3D] + 1];
    const float *tloc = g + G_X, *tdims = g + G_L;
    const float try_ = g[G_RY], alpha = decode_alpha(r, hl);
    float loc[3];
    decode_location(px, py, pox, poy, pdepth, c, dc.down_ratio, loc);
    put_box(boxes + 7 * BOX_PRED, loc, pdims, roty_of(alpha, loc[0], loc[2]));
    put_box(boxes + 7 * BOX_TARGET, tloc, tdims, try_);
    decode_location(px, py, pox, poy, g[G_Z], c, dc.down_ratio, loc);
    put_box(boxes + 7 * BOX_OFFSET, loc, tdims, try_);
    decode_location(px, py, g[G_OFFX], g[G_OFFY], pdepth, c, dc.down_ratio, loc);
    put_box(boxes + 7 * BOX_DEPTH, loc, tdims, try_);
    put_box(boxes + 7 * BOX_DIMS, tloc, pdims, try_);
    put_box(boxes + 7 * BOX_ORIEN, tloc, tdims, roty_of(alpha, tloc[0], tloc[2]));
}

// Whether a valid row can be evaluated: its centre inside the map and its class one of the three rows of dim_mean / dim_std
MFX_HD bool row_in_range(const float* g, int H, int W) {
    return g[G_CX] >= 0.f && g[G_CX] < (float)W && g[G_CY] >= 0.f && g[G_CY] < (float)H && g[G_CLS] >= 0.f && g[G_CLS] < 3.f;
}

// One object slot.  `map` = the regression channels of image b ([H][W] rows of ld floats, already offset by reg_off), g = its gt row.
// reg_mask == 0: zeros everywhere, the map is not read.  A valid row whose centre or class is out of range reads nothing either and
// writes NaN (the table is then visibly wrong instead of a read outside the map).  Outputs not wanted may be null.
MFX_HD void eval_object(const float* map, int ld, int H, int W, const float* g, const float* calib6, float padx, float pady,
                        const mfx_decode_cfg& dc, const mfx_head_layout& hl, int want, float* depth_err, float* iou, float* boxes) {
    const bool valid = g[G_MASK] != 0.f, ok = valid && row_in_range(g, H, W);
    if (!ok) {
        const float fill = valid ? __builtin_nanf("") : 0.f;
        if ((want & 1) && depth_err) for (int i = 0; i < NDEPTH; ++i) depth_err[i] = fill;
        if ((want & 2) && iou) for (int i = 0; i < NIOU; ++i) iou[i] = fill;
        if ((want & 2) && boxes) for (int i = 0; i < NBOX * 7; ++i) boxes[i] = fill;
        return;
    }
    const int cx = (int)g[G_CX], cy = (int)g[G_CY], cls = (int)g[G_CLS];
    const float* r = map + ((size_t)cy * W + cx) * ld;
    const Camera c = {calib6[0], calib6[1], calib6[2], calib6[3], calib6[4], calib6[5], padx, pady};
    float dims[3];
    decode_dims(r, dc, hl, cls, dims);
    Estimates e;
    decode_estimates(r, dc, hl, c.fu, dims[1], e);
    if ((want & 1) && depth_err) depth_errors(e, g[G_Z], depth_err);
    if (want & 2) {
        float bx[NBOX * 7];
        build_boxes(r, g, dims, combine(e, dc.output_depth, hl.ch[HK_DEPTH_UNC] >= 0, hl.ch[HK_KPT_UNC] >= 0).depth, c, dc, hl, bx);
        if (boxes) for (int i = 0; i < NBOX * 7; ++i) boxes[i] = bx[i];
        if (iou) {
            const int which[NIOU] = {BOX_PRED, BOX_OFFSET, BOX_DEPTH, BOX_DIMS, BOX_ORIEN};
            for (int k = 0; k < NIOU; ++k) iou[k] = biou::iou_rows(bx + 7 * which[k], bx + 7 * BOX_TARGET);
        }
    }
}

// Argument check shared by the entry point and the host shim: null when (cfg, heads, want) can be served, else the message
inline const char* config_error(const mfx_decode_cfg& dc, const mfx_head_layout& hl, int want) {
    if (want < 1 || want > 3) return "want must be 1 (depth errors), 2 (IoUs) or 3 (both)";
    if (const char* e = decode_cfg_error(dc)) return e;
    if (const char* e = head_layout_error(hl.ch, hl.reg_width)) return e;
    if ((want & 1) && !(hl.ch[HK_KPT] >= 0 && hl.ch[HK_KPT_UNC] >= 0 && hl.ch[HK_DEPTH_UNC] >= 0))
        return "the depth errors need depth_uncertainty, corner_offset and corner_uncertainty";
    return (want & 2) ? output_depth_error(dc.output_depth, hl) : nullptr;     // HeadSet.check_output_depth (detector_infer.py:148-204)
}

}  // namespace ediag
}  // namespace mfx
