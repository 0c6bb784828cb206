// From one regression row to one 3D box: the only statement of the decode rule (reference Anno_Encoder.decode_*, model/anno_encoder.py:69-295,
// and the `output_depth` combination, model/head/detector_infer.py:148-229) and of the head layout it reads.  decode.hip runs decode_row on
// the K best pixels of an image, eval_diag_math.h runs the same pieces at the labelled centres, object_loss_math.h takes the key order and
// the layout check (its own decode carries tangents and stays there).  float32 throughout; plain functions of one row, no HIP-only
// constructs: tests/shim/decode_row_host.cpp compiles them for the host.
#pragma once
#include <cmath>

#include "../../include/monoflex_hip.h"
#include "hd.h"

namespace mfx {
namespace bdec {

constexpr float kPi = 3.14159265358979323846f;
// mfx_head_layout.ch[] order (= mfx_object_loss_cfg.ch[]) and the channels each key takes
enum { HK_2D = 0, HK_OFF3D, HK_KPT, HK_KPT_UNC, HK_DIM3D, HK_ORI_CLS, HK_ORI_OFF, HK_DEPTH, HK_DEPTH_UNC };
constexpr int kHeadWidth[9] = {4, 2, 20, 3, 3, 8, 8, 1, 1};
// key2channel offsets of runs/monoflex.yaml:27-28, the full layout
enum { R_2D = 0, R_OFF3D = 4, R_KPT = 6, R_KPT_UNC = 26, R_DIM3D = 29, R_ORI_CLS = 32, R_ORI_OFF = 40, R_DEPTH = 48, R_DEPTH_UNC = 49, R_TOTAL = 50 };

// ---- what can be served: the message, or nullptr (the entry points prefix their own name) ------------------------------------------------
// The head set: three of the nine keys are optional (corner_offset, corner_uncertainty -- only with corner_offset --, depth_uncertainty);
// ch[i] == -1 marks an absent one, every present key lies inside the reg_width channels of the row.
inline const char* head_layout_error(const int* ch, int reg_width) {
    if (reg_width < 1 || reg_width > R_TOTAL) return "reg_width must be 1..50";
    for (int i = 0; i < 9; ++i) {
        const bool optional = i == HK_KPT || i == HK_KPT_UNC || i == HK_DEPTH_UNC;
        if (ch[i] < 0 && !(optional && ch[i] == -1)) return "a required regression key is absent";
        if (ch[i] >= 0 && ch[i] + kHeadWidth[i] > reg_width) return "a regression key's channels reach past reg_width";
    }
    if (ch[HK_KPT_UNC] >= 0 && ch[HK_KPT] < 0) return "corner_uncertainty without corner_offset";
    return nullptr;
}

inline const char* decode_cfg_error(const mfx_decode_cfg& dc) {
    if (dc.depth_decode < 0 || dc.depth_decode > 2) return "depth_decode must be 0 (exp), 1 (linear) or 2 (inv_sigmoid)";
    if (dc.output_depth < MFX_DEPTH_SOFT || dc.output_depth > MFX_DEPTH_KEYPOINTS_13) return "output_depth must be one of MFX_DEPTH_*";
    if (!std::isfinite(dc.depth_range[0]) || !std::isfinite(dc.depth_range[1]) || dc.depth_range[0] > dc.depth_range[1])
        return "depth_range must be finite with depth_range[0] <= depth_range[1]";
    return nullptr;
}

// detector_infer.py:148-204: keypoints_* read the keypoint depths; soft / hard / mean read them and their uncertainties
inline const char* output_depth_error(int mode, const mfx_head_layout& hl) {
    const bool kp = hl.ch[HK_KPT] >= 0, cu = hl.ch[HK_KPT_UNC] >= 0;
    if (mode >= MFX_DEPTH_KEYPOINTS_AVG && !kp) return "output_depth keypoints_* needs corner_offset";
    if (mode <= MFX_DEPTH_MEAN && !(kp && cu)) return "output_depth soft / hard / mean needs corner_offset and corner_uncertainty";
    return nullptr;
}

// ---- the row decodes -------------------------------------------------------------------------------------------------------------------------
struct Camera { float fu, fv, cu, cv, bx, by, padx, pady; };       // calib [6] and pad [2] of the row's image

// the four depth estimates d[] = direct, keypoint centre, 02, 13 (clamped to the depth range) and their sigmas u[] (1 where the set has
// no such head)
struct Estimates { float d[4], u[4]; };

MFX_HD float clampf(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }
MFX_HD float wrap_pi(float a) {
    if (a > kPi) a -= 2.f * kPi;
    if (a < -kPi) a += 2.f * kPi;
    return a;
}

// decode_box2d_fcos (anno_encoder.py:69-86) at the cell (px, py) -> x1, y1, x2, y2 clamped to [0, wmax] x [0, hmax]
MFX_HD void decode_box2d(const float* r, const mfx_head_layout& hl, float px, float py, const Camera& c, float down_ratio, float wmax, float hmax,
                         float* box) {
    const float* e = r + hl.ch[HK_2D];
    const float x1 = (px - fmaxf(e[0], 0.f)) * down_ratio - c.padx, y1 = (py - fmaxf(e[1], 0.f)) * down_ratio - c.pady;
    const float x2 = (px + fmaxf(e[2], 0.f)) * down_ratio - c.padx, y2 = (py + fmaxf(e[3], 0.f)) * down_ratio - c.pady;
    box[0] = clampf(x1, 0.f, wmax); box[1] = clampf(y1, 0.f, hmax); box[2] = clampf(x2, 0.f, wmax); box[3] = clampf(y2, 0.f, hmax);
}

// decode_dimension (anno_encoder.py:221-243), order (l, h, w): exp(offset) or the offset, then * std[cls] + mean[cls] or * mean[cls]
MFX_HD void decode_dims(const float* r, const mfx_decode_cfg& dc, const mfx_head_layout& hl, int cls, float* dims) {
    for (int i = 0; i < 3; ++i) {
        const float x = r[hl.ch[HK_DIM3D] + i];
        const float off = dc.dim_exp ? expf(x) : x;
        dims[i] = dc.dim_use_std ? off * dc.dim_std[cls * 3 + i] + dc.dim_mean[cls * 3 + i] : off * dc.dim_mean[cls * 3 + i];
    }
}

// decode_depth (anno_encoder.py:124-140: exp / linear around DEPTH_REFERENCE / inv_sigmoid) and decode_depth_from_keypoints_batch
// (:187-219) with the image's own f_u and the decoded height dh; an absent key is never read
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

// Which depth leaves the four estimates and the uncertainty that goes with it (detector_infer.py:149-198 `output_depth`).  Without
// depth_uncertainty soft / hard / mean combine the three keypoint depths alone (:177-182).  has_err: whether the reference has an
// estimated_depth_error for this mode at all -- the chosen estimate's own uncertainty head must exist (:148-170).
struct Combined { float depth, sigma; bool has_err; };

MFX_HD Combined combine(const Estimates& e, int mode, bool has_du, bool has_cu) {
    const float d0 = e.d[0], d1 = e.d[1], d2 = e.d[2], d3 = e.d[3], u0 = e.u[0], u1 = e.u[1], u2 = e.u[2], u3 = e.u[3];
    float depth, sigma;
    bool has_err = true;
    if (mode <= MFX_DEPTH_MEAN && !has_du) {
        if (mode == MFX_DEPTH_SOFT) {
            float w1 = 1.f / u1, w2 = 1.f / u2, w3 = 1.f / u3;
            const float ws = (w1 + w2) + w3;
            w1 /= ws; w2 /= ws; w3 /= ws;
            depth = (d1 * w1 + d2 * w2) + d3 * w3;
            sigma = (w1 * u1 + w2 * u2) + w3 * u3;
        } else if (mode == MFX_DEPTH_HARD) {
            const float w1 = 1.f / u1, w2 = 1.f / u2, w3 = 1.f / u3;
            depth = d1; float wb = w1;
            if (w2 > wb) { wb = w2; depth = d2; }
            if (w3 > wb) { wb = w3; depth = d3; }
            sigma = fminf(u1, fminf(u2, u3));
        } else {
            depth = ((d1 + d2) + d3) / 3.f; sigma = ((u1 + u2) + u3) / 3.f;
        }
    } else if (mode == MFX_DEPTH_SOFT) {                        // 'soft' (:186-192; runs/monoflex.yaml)
        float w0 = 1.f / u0, w1 = 1.f / u1, w2 = 1.f / u2, w3 = 1.f / u3;
        const float ws = ((w0 + w1) + w2) + w3;
        w0 /= ws; w1 /= ws; w2 /= ws; w3 /= ws;
        depth = ((d0 * w0 + d1 * w1) + d2 * w2) + d3 * w3;
        sigma = ((w0 * u0 + w1 * u1) + w2 * u2) + w3 * u3;
    } else if (mode == MFX_DEPTH_HARD) {                        // 'hard' (:180-184): the estimate of the largest weight 1 / u (first of equals, as argmax)
        const float w0 = 1.f / u0, w1 = 1.f / u1, w2 = 1.f / u2, w3 = 1.f / u3;
        depth = d0; float wb = w0;
        if (w1 > wb) { wb = w1; depth = d1; }
        if (w2 > wb) { wb = w2; depth = d2; }
        if (w3 > wb) { wb = w3; depth = d3; }
        sigma = fminf(fminf(u0, u1), fminf(u2, u3));
    } else if (mode == MFX_DEPTH_MEAN) {                        // 'mean' (:194-198)
        depth = (((d0 + d1) + d2) + d3) / 4.f; sigma = (((u0 + u1) + u2) + u3) / 4.f;
    } else if (mode == MFX_DEPTH_DIRECT) {                      // 'direct' (:149-152)
        depth = d0; sigma = u0; has_err = has_du;
    } else if (mode == MFX_DEPTH_KEYPOINTS_AVG) {               // 'keypoints_avg' (:155-157)
        depth = ((d1 + d2) + d3) / 3.f; sigma = ((u1 + u2) + u3) / 3.f; has_err = has_cu;
    } else if (mode == MFX_DEPTH_KEYPOINTS_CENTER) { depth = d1; sigma = u1; has_err = has_cu; }   // (:159-161)
    else if (mode == MFX_DEPTH_KEYPOINTS_02) { depth = d2; sigma = u2; has_err = has_cu; }          // (:163-165)
    else { depth = d3; sigma = u3; has_err = has_cu; }                                              // 'keypoints_13' (:167-169)
    return Combined{depth, sigma, has_err};
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

MFX_HD float roty_of(float alpha, float X, float Z) { return wrap_pi(alpha + atan2f(X, Z)); }

// One detection: det = [cls, alpha, x1, y1, x2, y2, h, w, l, X, Y, Z, ry, score] (Y = the bottom centre), the chosen depth's sigma,
// conf = 1 - clamp(sigma, 0.01, 1), and whether conf scaled the score (TEST.UNCERTAINTY_AS_CONFIDENCE, detector_infer.py:223-229: only where
// the reference has an estimated_depth_error; otherwise the raw score, and no uncertainty is reported).
struct Row { float det[14], sigma, conf; bool as_conf; };

// r = the regression row of the cell (px, py), decoded under class cls; (wmax, hmax) = the 2D box clamp (image 0's padded size - 1)
MFX_HD Row decode_row(const float* r, float px, float py, int cls, float score, const Camera& c, float wmax, float hmax,
                      const mfx_decode_cfg& dc, const mfx_head_layout& hl) {
    Row o;
    float dims[3], loc[3];
    Estimates e;
    decode_box2d(r, hl, px, py, c, dc.down_ratio, wmax, hmax, o.det + 2);
    decode_dims(r, dc, hl, cls, dims);
    decode_estimates(r, dc, hl, c.fu, dims[1], e);
    const bool has_kp = hl.ch[HK_KPT] >= 0;
    const Combined z = combine(e, dc.output_depth, hl.ch[HK_DEPTH_UNC] >= 0, has_kp && hl.ch[HK_KPT_UNC] >= 0);
    decode_location(px, py, r[hl.ch[HK_OFF3D]], r[hl.ch[HK_OFF3D] + 1], z.depth, c, dc.down_ratio, loc);
    const float alpha = decode_alpha(r, hl);
    o.det[0] = (float)cls; o.det[1] = wrap_pi(alpha);
    o.det[6] = dims[1]; o.det[7] = dims[2]; o.det[8] = dims[0];                  // roll(-1): (l,h,w) -> (h,w,l)
    o.det[9] = loc[0]; o.det[10] = loc[1] + dims[1] / 2.f; o.det[11] = loc[2];   // detector_infer.py:215
    o.det[12] = roty_of(alpha, loc[0], loc[2]);
    o.sigma = z.sigma;
    o.conf = 1.f - clampf(z.sigma, 0.01f, 1.f);
    o.as_conf = dc.uncertainty_as_conf && z.has_err;
    o.det[13] = o.as_conf ? score * o.conf : score;
    return o;
}

// ---- decode_row in two parts (decode_multi.hip: several depth modes of one detection) -------------------------------------------------------
// What no depth mode changes: the 2D box, the dimensions (l, h, w), the local angle before any wrap, the 3D offset and the four estimates.
// finish_row(shared_part(...), ..., combine(estimates, mode, ...)) is decode_row under that mode, expression for expression.
struct Shared { float box[4], dims[3], alpha, offx, offy; Estimates e; };

MFX_HD void shared_part(const float* r, float px, float py, int cls, const Camera& c, float wmax, float hmax, const mfx_decode_cfg& dc,
                        const mfx_head_layout& hl, Shared& s) {
    decode_box2d(r, hl, px, py, c, dc.down_ratio, wmax, hmax, s.box);
    decode_dims(r, dc, hl, cls, s.dims);
    decode_estimates(r, dc, hl, c.fu, s.dims[1], s.e);
    s.offx = r[hl.ch[HK_OFF3D]]; s.offy = r[hl.ch[HK_OFF3D] + 1];
    s.alpha = decode_alpha(r, hl);
}

// the row from a depth, its sigma and has_err (a Combined)
MFX_HD Row finish_row(const Shared& s, float px, float py, int cls, float score, const Camera& c, const mfx_decode_cfg& dc, const Combined& z) {
    Row o;
    float loc[3];
    decode_location(px, py, s.offx, s.offy, z.depth, c, dc.down_ratio, loc);
    o.det[0] = (float)cls; o.det[1] = wrap_pi(s.alpha);
    for (int i = 0; i < 4; ++i) o.det[2 + i] = s.box[i];
    o.det[6] = s.dims[1]; o.det[7] = s.dims[2]; o.det[8] = s.dims[0];
    o.det[9] = loc[0]; o.det[10] = loc[1] + s.dims[1] / 2.f; o.det[11] = loc[2];
    o.det[12] = roty_of(s.alpha, loc[0], loc[2]);
    o.sigma = z.sigma;
    o.conf = 1.f - clampf(z.sigma, 0.01f, 1.f);
    o.as_conf = dc.uncertainty_as_conf && z.has_err;
    o.det[13] = o.as_conf ? score * o.conf : score;
    return o;
}

}  // namespace bdec
}  // namespace mfx
