// Validation diagnostics of one labelled object -- C ABI mfx_eval_diagnostics (eval_diag.hip maps one lane onto one object slot).
//
// Reference: PostProcessor.evaluate_3D_depths (model/head/detector_infer.py:280-359, TEST.EVAL_DEPTH) and evaluate_3D_detection (:361-452,
// TEST.EVAL_DIS_IOUS).  Both read the regression row at the object's TARGET centre and decode it with the TARGET class:
//   depth errors  the four depth estimates (direct, keypoint centre / 02 / 13) and their sigmas, the estimate of the smallest sigma, the
//                 1/sigma-weighted one, their mean and the best of the four, each as |estimate - Z_target| (13 values, DE_* below)
//   boxes         six rows (x, y, z, l, h, w, ry), y = the box centre: the predicted box, the target box, and four boxes in which ONE
//                 component (offset, depth, dimensions, orientation) is predicted and the rest is ground truth (BOX_* below)
//   IoUs          biou::iou_rows of boxes 0, 2, 3, 4, 5 with box 1 (pred_IoU, offset_IoU, depth_IoU, dims_IoU, orien_IoU)
// The decode formulas are those of decode.hip `decode_boxes_kernel` (anno_encoder.py:124-295), restated here per object; the tests pin the
// predicted box to that kernel's row of the same pixel and class.  The reference's evaluate_3D_detection only knows output_depth 'direct'
// (its other branches raise); for the other seven modes the predicted depth is the one decode_boxes_kernel produces, same combination and
// head-set rule.  Its get_iou3d never ran (NameError): the IoU is this library's own operator.
// float32 throughout.  box3d_iou_math.h-style: plain functions of one object; tests/shim compiles them for the host.
#pragma once
#include <cmath>

#include "../../include/monoflex_hip.h"
#include "box3d_iou_math.h"

namespace mfx {
namespace ediag {

constexpr float kPi = 3.14159265358979323846f;
constexpr int GT_ROW = MFX_EVAL_GT_ROW, NDEPTH = MFX_EVAL_DEPTH_KEYS, NIOU = MFX_EVAL_IOU_KEYS, NBOX = MFX_EVAL_BOXES;
// gt_rows columns
enum { G_MASK = 0, G_CLS, G_CX, G_CY, G_OFFX, G_OFFY, G_X, G_Y, G_Z, G_L, G_H, G_W, G_RY };
// depth_err columns, in the order of the reference's dict (detector_infer.py:341-357)
enum { DE_DIRECT = 0, DE_DIRECT_SIGMA, DE_KPT_CENTER, DE_KPT_02, DE_KPT_13, DE_KPT_CENTER_SIGMA, DE_KPT_02_SIGMA, DE_KPT_13_SIGMA,
       DE_SIGMA_MIN, DE_SIGMA_WEIGHTED, DE_MEAN, DE_MIN, DE_TARGET };
enum { BOX_PRED = 0, BOX_TARGET, BOX_OFFSET, BOX_DEPTH, BOX_DIMS, BOX_ORIEN };
// mfx_head_layout.ch[] order
enum { HK_2D = 0, HK_OFF3D, HK_KPT, HK_KPT_UNC, HK_DIM3D, HK_ORI_CLS, HK_ORI_OFF, HK_DEPTH, HK_DEPTH_UNC };

struct Camera { float fu, fv, cu, cv, bx, by, padx, pady; };

// the four depth estimates d[] = direct, keypoint centre, 02, 13 (clamped to the depth range) and their sigmas u[] (1 where the set has
// no such head), from the decoded height dh
struct Estimates { float d[4], u[4]; };

MFX_HD float clampf(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }

// decode_dimension (anno_encoder.py:221-243), order (l, h, w)
MFX_HD void decode_dims(const float* r, const mfx_decode_cfg& dc, const mfx_head_layout& hl, int cls, float* dims) {
    for (int i = 0; i < 3; ++i) {
        const float x = r[hl.ch[HK_DIM3D] + i];
        const float off = dc.dim_exp ? expf(x) : x;
        dims[i] = dc.dim_use_std ? off * dc.dim_std[cls * 3 + i] + dc.dim_mean[cls * 3 + i] : off * dc.dim_mean[cls * 3 + i];
    }
}

// decode_depth (anno_encoder.py:124-140) and decode_depth_from_keypoints_batch (:187-219) with the image's own f_u
MFX_HD void decode_estimates(const float* r, const mfx_decode_cfg& dc, const mfx_head_layout& hl, float fu, float dh, Estimates& e) {
    const float lo = dc.depth_range[0], hi = dc.depth_range[1];
    const float x = r[hl.ch[HK_DEPTH]];
    float d0;
    if (dc.depth_decode == 0) d0 = expf(x);
    else if (dc.depth_decode == 1) d0 = x * dc.depth_ref[1] + dc.depth_ref[0];
    else d0 = 1.f / (1.f / (1.f + expf(-x))) - 1.f;
    e.d[0] = clampf(d0, lo, hi);
    const int kp = hl.ch[HK_KPT], cu = kp >= 0 ? hl.ch[HK_KPT_UNC] : -1, du = hl.ch[HK_DEPTH_UNC];
    e.u[0] = du >= 0 ? expf(r[du]) : 1.f;
    // keypoint k = (r[kp + 2 k], r[kp + 2 k + 1]); only the y values enter
    float t[5];
    const int top[5] = {8, 0, 2, 1, 3}, bottom[5] = {9, 4, 6, 5, 7};
    for (int i = 0; i < 5; ++i) {
        const float dy = kp >= 0 ? r[kp + 2 * top[i] + 1] - r[kp + 2 * bottom[i] + 1] : 0.f;
        t[i] = fu * dh / (fmaxf(dy, 0.f) * dc.down_ratio + dc.eps);
    }
    e.d[1] = clampf(t[0], lo, hi);
    e.d[2] = clampf((t[1] + t[2]) / 2.f, lo, hi);
    e.d[3] = clampf((t[3] + t[4]) / 2.f, lo, hi);
    for (int i = 0; i < 3; ++i) e.u[1 + i] = cu >= 0 ? expf(r[cu + i]) : 1.f;
}

// the depth decode_boxes_kernel gives the box under cfg.output_depth (detector_infer.py:149-198); without depth_uncertainty soft / hard /
// mean combine the three keypoint depths alone
MFX_HD float output_depth(const Estimates& e, int mode, bool has_du) {
    const float *d = e.d, *u = e.u;
    if (mode <= MFX_DEPTH_MEAN && !has_du) {
        if (mode == MFX_DEPTH_SOFT) {
            float w1 = 1.f / u[1], w2 = 1.f / u[2], w3 = 1.f / u[3];
            const float ws = (w1 + w2) + w3;
            w1 /= ws; w2 /= ws; w3 /= ws;
            return (d[1] * w1 + d[2] * w2) + d[3] * w3;
        }
        if (mode == MFX_DEPTH_HARD) {
            const float w1 = 1.f / u[1], w2 = 1.f / u[2], w3 = 1.f / u[3];
            float depth = d[1], wb = w1;
            if (w2 > wb) { wb = w2; depth = d[2]; }
            if (w3 > wb) { wb = w3; depth = d[3]; }
            return depth;
        }
        return ((d[1] + d[2]) + d[3]) / 3.f;
    }
    if (mode == MFX_DEPTH_SOFT) {
        float w0 = 1.f / u[0], w1 = 1.f / u[1], w2 = 1.f / u[2], w3 = 1.f / u[3];
        const float ws = ((w0 + w1) + w2) + w3;
        w0 /= ws; w1 /= ws; w2 /= ws; w3 /= ws;
        return ((d[0] * w0 + d[1] * w1) + d[2] * w2) + d[3] * w3;
    }
    if (mode == MFX_DEPTH_HARD) {                                    // the estimate of the largest weight 1 / u, first of equals
        float depth = d[0], wb = 1.f / u[0];
        for (int i = 1; i < 4; ++i) {
            const float w = 1.f / u[i];
            if (w > wb) { wb = w; depth = d[i]; }
        }
        return depth;
    }
    if (mode == MFX_DEPTH_MEAN) return (((d[0] + d[1]) + d[2]) + d[3]) / 4.f;
    if (mode == MFX_DEPTH_DIRECT) return d[0];
    if (mode == MFX_DEPTH_KEYPOINTS_AVG) return ((d[1] + d[2]) + d[3]) / 3.f;
    return d[mode - MFX_DEPTH_KEYPOINTS_CENTER + 1];
}

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

// decode_location_flatten (anno_encoder.py:142-155) + project_image_to_rect (kitti_utils.py:350-369) at the cell (px, py)
MFX_HD void decode_location(float px, float py, float offx, float offy, float depth, const Camera& c, float down_ratio, float* loc) {
    const float u = (px + offx) * down_ratio - c.padx;
    const float v = (py + offy) * down_ratio - c.pady;
    loc[0] = ((u - c.cu) * depth) / c.fu + c.bx;
    loc[1] = ((v - c.cv) * depth) / c.fv + c.by;
    loc[2] = depth;
}

// decode_axes_orientation, multi-bin (anno_encoder.py:245-295) -> the local angle before any wrap
MFX_HD float decode_alpha(const float* r, const mfx_head_layout& hl) {
    const int oc = hl.ch[HK_ORI_CLS], oo = hl.ch[HK_ORI_OFF];
    int best = 0; float bestp = -1.f;
    for (int i = 0; i < 4; ++i) {
        const float a = r[oc + 2 * i], c = r[oc + 2 * i + 1];
        const float m = fmaxf(a, c), e0 = expf(a - m), e1 = expf(c - m);
        const float p1 = e1 / (e0 + e1);
        if (p1 > bestp) { bestp = p1; best = i; }
    }
    const float centers[4] = {0.f, kPi / 2.f, kPi, -kPi / 2.f};
    return atan2f(r[oo + 2 * best], r[oo + 2 * best + 1]) + centers[best];
}

MFX_HD float roty_of(float alpha, float X, float Z) {
    float ry = alpha + atan2f(X, Z);
    if (ry > kPi) ry -= 2.f * kPi;
    if (ry < -kPi) ry += 2.f * kPi;
    return ry;
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
        build_boxes(r, g, dims, output_depth(e, dc.output_depth, hl.ch[HK_DEPTH_UNC] >= 0), c, dc, hl, bx);
        if (boxes) for (int i = 0; i < NBOX * 7; ++i) boxes[i] = bx[i];
        if (iou) {
            const int which[NIOU] = {BOX_PRED, BOX_OFFSET, BOX_DEPTH, BOX_DIMS, BOX_ORIEN};
            for (int k = 0; k < NIOU; ++k) iou[k] = biou::iou_rows(bx + 7 * which[k], bx + 7 * BOX_TARGET);
        }
    }
}

// Argument check shared by the entry point and the host shim: null when (cfg, heads, want) can be served, else the message
inline const char* config_error(const mfx_decode_cfg& dc, const mfx_head_layout& hl, int want) {
    if (want < 1 || want > 3) return "eval_diagnostics: want must be 1 (depth errors), 2 (IoUs) or 3 (both)";
    if (dc.depth_decode < 0 || dc.depth_decode > 2) return "eval_diagnostics: depth_decode must be 0 (exp), 1 (linear) or 2 (inv_sigmoid)";
    if (dc.output_depth < MFX_DEPTH_SOFT || dc.output_depth > MFX_DEPTH_KEYPOINTS_13) return "eval_diagnostics: output_depth must be one of MFX_DEPTH_*";
    if (!std::isfinite(dc.depth_range[0]) || !std::isfinite(dc.depth_range[1]) || dc.depth_range[0] > dc.depth_range[1])
        return "eval_diagnostics: depth_range must be finite with depth_range[0] <= depth_range[1]";
    const int R = hl.reg_width;
    if (R < 1 || R > 50) return "eval_diagnostics: reg_width must be 1..50";
    const int width[9] = {4, 2, 20, 3, 3, 8, 8, 1, 1};
    for (int i = 0; i < 9; ++i) {
        const bool optional = i == HK_KPT || i == HK_KPT_UNC || i == HK_DEPTH_UNC;
        if (hl.ch[i] < 0 && !(optional && hl.ch[i] == -1)) return "eval_diagnostics: a required regression key is absent";
        if (hl.ch[i] >= 0 && hl.ch[i] + width[i] > R) return "eval_diagnostics: a regression key's channels reach past reg_width";
    }
    const bool kp = hl.ch[HK_KPT] >= 0, cu = hl.ch[HK_KPT_UNC] >= 0, du = hl.ch[HK_DEPTH_UNC] >= 0;
    if (cu && !kp) return "eval_diagnostics: corner_uncertainty without corner_offset";
    if ((want & 1) && !(kp && cu && du))
        return "eval_diagnostics: the depth errors need depth_uncertainty, corner_offset and corner_uncertainty";
    if (want & 2) {                                                   // HeadSet.check_output_depth (detector_infer.py:148-204)
        if (dc.output_depth >= MFX_DEPTH_KEYPOINTS_AVG && !kp) return "eval_diagnostics: output_depth keypoints_* needs corner_offset";
        if (dc.output_depth <= MFX_DEPTH_MEAN && !(kp && cu)) return "eval_diagnostics: output_depth soft / hard / mean needs corner_offset and corner_uncertainty";
    }
    return nullptr;
}

}  // namespace ediag
}  // namespace mfx
