// Per-object regression losses of the detection head and their gradient, as one function of (the R <= 50 regression channels at
// the object's centre pixel, the object's target row) -- C ABI mfx_object_loss / mfx_object_loss_backward.
//
// Reference: model/head/detector_loss.py:116-482 (prepare_predictions + the nine regression terms + the logged MAEs) with
// the decoders of model/anno_encoder.py:88-295, model/layers/iou_loss.py:7-49 and data/datasets/kitti_utils.py:350-369.  The
// reference evaluates them as ~300 small tensor ops forward and ~600 backward per step; every one of them is per-object, so
// here one wavefront owns one object: lane c carries the forward-mode tangent d/d(channel c) through the whole expression
// (Dual below), which gives the exact gradient row of every loss term in the same pass -- no hand-derived backward to keep
// in sync.  Non-differentiable selections (arg max of the orientation bins, `.detach()`ed operands) simply carry a zero tangent.
// kitti_eval_math.h-style: plain functions, loss_kernels.hip maps lanes onto them, tests/shim compiles them for the host.
//
// Head sets (the reference's ablation ladder): three of the nine keys are optional -- depth_uncertainty, corner_offset and
// corner_uncertainty (only with corner_offset); cfg.ch[i] == -1 marks an absent one.  Its channels are never read, the terms and
// logged values that need it come out 0, and the rest follows the reference's `if self.depth_with_uncertainty` /
// `compute_keypoint_corner` / `corner_with_uncertainty` branches (head_set_error below lists what each set can serve).
//
// Loss types (MODEL.HEAD.LOSS_TYPE entries 1 and 3; C ABI mfx_object_loss_types): the regular regression loss is L1 or smooth-L1
// (reg_loss below: the offset coordinates, the dimensions, the corner coordinates, the keypoint depths, the combined depth), the
// direct-depth loss is L1, log-L1 or the reference's `inv_sig` (depth_loss below).  Both kinds are template parameters of
// object_terms_t: <REG_L1, DEP_L1> compiles to the expressions that were here before them (mfx_object_loss: same bits).
#pragma once
#include <cmath>

#include "../../include/monoflex_hip.h"
#include "box3d_iou_math.h"
#include "box_decode_math.h"

namespace mfx {
namespace oloss {

constexpr int ROW = MFX_OBJ_ROW, NTERM = MFX_OBJ_TERMS, NVAL = MFX_OBJ_VALUES, NNORM = 8;
// target row fields (float32 each; written by Loss_Computation.pack_objects)
enum { R_VALID = 0, R_CLS, R_CX, R_CY, R_BOX = 4, R_KP = 8, R_KDM = 38, R_DIMS = 41, R_DEPTH = 44, R_ROTY, R_ORI = 46, R_OFF = 54,
       R_TRUNC = 56, R_B, R_CAL = 58, R_PAD = 64, R_FU_RANK = 66 };
// loss terms (the reference's names), then the logged values (V_IOU3D = slot 21: the first of the three spare slots)
enum { T_BBOX = 0, T_DEPTH, T_OFFSET, T_TRUNC_OFFSET, T_ORIEN, T_DIMS, T_CORNER, T_KEYPOINT, T_KEYPOINT_DEPTH, T_SOFT_DEPTH,
       V_IOU2D = 10, V_REAL_DEPTH, V_VALID_KD, V_DEPTH_MAE, V_CENTER_MAE, V_02_MAE, V_13_MAE, V_LOWER_MAE, V_HARD_MAE, V_SOFT_MAE,
       V_MEAN_MAE, V_IOU3D };
static_assert(V_IOU3D == 21 && V_IOU3D < NVAL, "the logged 3D IoU is value slot 21");
enum { N_V = 0, N_V2D, N_V_INSIDE, N_TRUNC, N_KMASK, N_KD_VALID, N_KD_INVALID, N_ORI };
// cfg.ch[] is in bdec's key order
using bdec::HK_2D; using bdec::HK_OFF3D; using bdec::HK_KPT; using bdec::HK_KPT_UNC; using bdec::HK_DIM3D; using bdec::HK_ORI_CLS;
using bdec::HK_ORI_OFF; using bdec::HK_DEPTH; using bdec::HK_DEPTH_UNC;
constexpr int MAX_REG = 50;                                        // the full head set's width; a reduced set is 26..49 wide

// regression width the caller states (cfg.reg_width; 0 = the full 50)
MFX_HD int reg_width(const mfx_object_loss_cfg& c) { return c.reg_width == 0 ? MAX_REG : c.reg_width; }
// What is wrong with a head set / corner depth mode, or nullptr: the required keys present and inside the row, corner_uncertainty only
// next to corner_offset, keypoint_mean only with keypoints, soft / hard combine only with all four depth estimates and their uncertainties.
inline const char* head_set_error(const mfx_object_loss_cfg& c) {
    if (const char* e = bdec::head_layout_error(c.ch, reg_width(c))) return e;
    if (c.corner_depth_mode < 0 || c.corner_depth_mode > 3) return "corner_depth_mode outside 0..3";
    if (c.corner_depth_mode == 1 && c.ch[HK_KPT] < 0) return "corner_depth_mode keypoint_mean needs corner_offset";
    if (c.corner_depth_mode >= 2 && (c.ch[HK_KPT] < 0 || c.ch[HK_KPT_UNC] < 0 || c.ch[HK_DEPTH_UNC] < 0))
        return "corner_depth_mode soft_combine / hard_combine needs corner_offset, corner_uncertainty and depth_uncertainty";
    return nullptr;
}

// ---- forward-mode value/tangent pair ------------------------------------------------------------------------------------------
struct Dual { float v, d; };
MFX_HD Dual K(float c) { return Dual{c, 0.f}; }
MFX_HD Dual detach(Dual a) { return Dual{a.v, 0.f}; }
MFX_HD Dual operator+(Dual a, Dual b) { return Dual{a.v + b.v, a.d + b.d}; }
MFX_HD Dual operator-(Dual a, Dual b) { return Dual{a.v - b.v, a.d - b.d}; }
MFX_HD Dual operator-(Dual a) { return Dual{-a.v, -a.d}; }
MFX_HD Dual operator*(Dual a, Dual b) { return Dual{a.v * b.v, a.d * b.v + a.v * b.d}; }
MFX_HD Dual operator/(Dual a, Dual b) { const float q = a.v / b.v; return Dual{q, (a.d - q * b.d) / b.v}; }
MFX_HD Dual operator+(Dual a, float b) { return Dual{a.v + b, a.d}; }
MFX_HD Dual operator-(Dual a, float b) { return Dual{a.v - b, a.d}; }
MFX_HD Dual operator*(Dual a, float b) { return Dual{a.v * b, a.d * b}; }
MFX_HD Dual operator/(Dual a, float b) { return Dual{a.v / b, a.d / b}; }
MFX_HD Dual dexp(Dual a) { const float e = expf(a.v); return Dual{e, e * a.d}; }
MFX_HD Dual dlog(Dual a) { return Dual{logf(a.v), a.d / a.v}; }
MFX_HD Dual dabs(Dual a) { return Dual{fabsf(a.v), a.v > 0.f ? a.d : (a.v < 0.f ? -a.d : 0.f)}; }          // sign(0) = 0 as torch
MFX_HD Dual drelu(Dual a) { return a.v > 0.f ? a : Dual{0.f, 0.f}; }
MFX_HD Dual dclamp(Dual a, float lo, float hi) {                                                            // gradient passes on [lo, hi]
    return a.v < lo ? Dual{lo, 0.f} : (a.v > hi ? Dual{hi, 0.f} : a);
}
MFX_HD Dual dmin(Dual a, Dual b) { return a.v < b.v ? a : (b.v < a.v ? b : Dual{a.v, 0.5f * (a.d + b.d)}); }
MFX_HD Dual dmax(Dual a, Dual b) { return a.v > b.v ? a : (b.v > a.v ? b : Dual{a.v, 0.5f * (a.d + b.d)}); }
MFX_HD Dual dsin(Dual a) { return Dual{sinf(a.v), cosf(a.v) * a.d}; }
MFX_HD Dual dcos(Dual a) { return Dual{cosf(a.v), -sinf(a.v) * a.d}; }
MFX_HD Dual datan2(Dual y, Dual x) {
    const float r2 = x.v * x.v + y.v * y.v;
    return Dual{atan2f(y.v, x.v), r2 > 0.f ? (y.d * x.v - x.d * y.v) / r2 : 0.f};
}
MFX_HD Dual dsqrt(Dual a) { const float s = sqrtf(a.v); return Dual{s, s > 0.f ? 0.5f * a.d / s : 0.f}; }
MFX_HD Dual dsigmoid(Dual a) { const float s = 1.f / (1.f + expf(-a.v)); return Dual{s, s * (1.f - s) * a.d}; }

// F.smooth_l1_loss at its default beta = 1 (value 0.5 and slope +-1 from both sides at |d| = 1: C1)
MFX_HD Dual dsmooth_l1(Dual a) {
    const float m = fabsf(a.v);
    return m < 1.f ? Dual{0.5f * a.v * a.v, a.v * a.d} : Dual{m - 0.5f, a.v > 0.f ? a.d : -a.d};
}

// MODEL.HEAD.LOSS_TYPE[1]: 'L1', or any other string = F.smooth_l1_loss (detector_loss.py:53); LOSS_TYPE[3]: 'L1', 'log', 'inv_sig'
// (detector_loss.py:45-49; 'berhu' cannot run in the reference and is refused by Loss_Computation)
enum { REG_L1 = 0, REG_SMOOTH_L1, NUM_REG_LOSS };
enum { DEP_L1 = 0, DEP_LOG, DEP_INV_SIG, NUM_DEPTH_LOSS };
MFX_HD bool loss_kinds_ok(int reg, int dep) { return reg >= 0 && reg < NUM_REG_LOSS && dep >= 0 && dep < NUM_DEPTH_LOSS; }
// the regular regression loss of a difference d (self.reg_loss_fnc, reduction 'none')
template <int REG> MFX_HD Dual reg_loss(Dual d) { return REG == REG_L1 ? dabs(d) : dsmooth_l1(d); }
// the direct-depth loss of (decoded, clamped prediction p; target t).  DEP_LOG: |log p - log t| (depth_losses.py Log_L1_Loss).
// DEP_INV_SIG: what Inverse_Sigmoid_Loss.forward computes, |1/sigmoid(t) - 1 - t| -- a function of the TARGET alone (the reference
// transforms `target`, not `prediction`): the depth channel gets a zero gradient, the depth uncertainty still gets its own.
template <int DEP> MFX_HD Dual depth_loss(Dual p, float t) {
    if (DEP == DEP_LOG) return dabs(dlog(p) - logf(t));
    if (DEP == DEP_INV_SIG) return K(fabsf(1.f / (1.f / (1.f + expf(-t))) - 1.f - t));
    return dabs(p - t);
}

struct Vec3 { Dual x, y, z; };

// anno_encoder.py:124-140
MFX_HD Dual decode_depth(Dual off, const mfx_object_loss_cfg& c) {
    Dual d = c.depth_mode == 0 ? dexp(off) : (c.depth_mode == 1 ? off * c.depth_ref[1] + c.depth_ref[0] : K(1.f) / dsigmoid(off) - 1.f);
    return c.has_depth_range ? dclamp(d, c.depth_range[0], c.depth_range[1]) : d;
}
// anno_encoder.py:142-156 with kitti_utils.py:350-369 (project_image_to_rect, one point)
MFX_HD Vec3 decode_location(float px, float py, Dual ox, Dual oy, Dual depth, const float* cal, const float* pad, float down) {
    const Dual u = (ox + px) * down - pad[0], v = (oy + py) * down - pad[1];
    return Vec3{(u - cal[2]) * depth / cal[0] + cal[4], (v - cal[3]) * depth / cal[1] + cal[5], depth};
}
// anno_encoder.py:88-122: corner k of the box (rotation about Y, centre at half height as the reference builds it)
MFX_HD Vec3 box_corner(int k, Dual cs, Dual sn, const Dual* dims, const Vec3& loc) {
    const float sx = (k & 2) ? 1.f : -1.f;                         // -1 -1 1 1 -1 -1 1 1
    const float sy = k < 4 ? 1.f : -1.f;                           //  1  1 1 1 -1 -1 -1 -1
    const float sz = ((k + 1) & 2) ? 1.f : -1.f;                   // -1  1 1 -1 -1 1 1 -1
    const Dual x = dims[0] * (0.5f * sx), y = dims[1] * (0.5f * sy), z = dims[2] * (0.5f * sz);
    return Vec3{cs * x + sn * z + loc.x, y + loc.y, -(sn * x) + cs * z + loc.z};
}

// One object.  X(ch) returns channel `ch` of the regression channels at the object's pixel as a Dual seeded for this lane;
// `t` is the target row, `nrm` the eight batch-wide selection counts.  out[NVAL] ACCUMULATES nothing: it is overwritten with this
// object's contribution to each loss term (already weighted and divided by its count) and to each logged mean.
template <int REG, int DEP, typename Reader>
MFX_HD void object_terms_t(const Reader& X, const float* t, const mfx_object_loss_cfg& c, const float* nrm, Dual* out) {
    for (int i = 0; i < NVAL; ++i) out[i] = K(0.f);
    if (t[R_VALID] == 0.f) return;
    const float PI = 3.14159265358979323846f;
    auto cnt = [&](int i) { return fmaxf(nrm[i], 1.f); };
    const int cls = t[R_CLS] > 0.f ? (int)t[R_CLS] : 0;
    const float px = t[R_CX], py = t[R_CY];
    const float* box = t + R_BOX;
    const float* cal = t + R_CAL;
    const float* pad = t + R_PAD;
    const float t_depth = t[R_DEPTH];
    const float inv_v = 1.f / cnt(N_V);
    const bool has_du = c.ch[HK_DEPTH_UNC] >= 0, has_kp = c.ch[HK_KPT] >= 0, has_cu = has_kp && c.ch[HK_KPT_UNC] >= 0;

    // ---- 2D box: GIoU / IoU of the four ReLU'ed side distances (iou_loss.py:12-49) ---------------------------------------------
    if (box[3] - box[1] > 0.f && box[2] - box[0] > 0.f) {
        const Dual pl = drelu(X(c.ch[HK_2D])), pt = drelu(X(c.ch[HK_2D] + 1)), pr = drelu(X(c.ch[HK_2D] + 2)), pb = drelu(X(c.ch[HK_2D] + 3));
        const Dual tl = K(px - box[0]), tt = K(py - box[1]), tr = K(box[2] - px), tb = K(box[3] - py);
        const Dual t_area = (tl + tr) * (tt + tb), p_area = (pl + pr) * (pt + pb);
        const Dual w_i = dmin(pl, tl) + dmin(pr, tr), h_i = dmin(pb, tb) + dmin(pt, tt);
        const Dual g_w = dmax(pl, tl) + dmax(pr, tr), g_h = dmax(pb, tb) + dmax(pt, tt);
        const Dual ac = g_w * g_h + 1e-7f, inter = w_i * h_i, uni = t_area + p_area - inter;
        const Dual iou = (inter + 1.0f) / (uni + 1.0f);
        const Dual l = c.iou_type == 1 ? -dlog(iou) : (c.iou_type == 2 ? K(1.f) - iou : K(1.f) - (iou - (ac - uni) / ac));
        out[T_BBOX] = l * (c.w[T_BBOX] / cnt(N_V2D));
        out[V_IOU2D] = K(iou.v / cnt(N_V2D));
    }

    // ---- decoded predictions ---------------------------------------------------------------------------------------------------
    const Dual p_depth = decode_depth(X(c.ch[HK_DEPTH]), c);
    const Dual d_unc = has_du ? dclamp(X(c.ch[HK_DEPTH_UNC]), c.unc_lo, c.unc_hi) : K(0.f);
    Dual p_dims[3];
    for (int k = 0; k < 3; ++k) {                                   // anno_encoder.py:217-239
        Dual o = X(c.ch[HK_DIM3D] + k);
        if (c.dim_exp) o = dexp(o);
        p_dims[k] = c.dim_use_std ? o * c.dim_std[cls * 3 + k] + c.dim_mean[cls * 3 + k] : o * c.dim_mean[cls * 3 + k];
    }
    Dual kx[10], ky[10];
    for (int j = 0; j < 10; ++j) {
        kx[j] = has_kp ? X(c.ch[HK_KPT] + 2 * j) : K(0.f);
        ky[j] = has_kp ? X(c.ch[HK_KPT] + 2 * j + 1) : K(0.f);
    }
    // depths from the three keypoint groups (anno_encoder.py:185-215); the focal length is the reference's rank-indexed one
    Dual kd[3] = {K(0.f), K(0.f), K(0.f)};
    if (has_kp) {
        const Dual fh = p_dims[1] * t[R_FU_RANK];
        auto solve = [&](Dual dh) { return fh / (drelu(dh) * c.down_ratio + c.eps); };
        kd[0] = solve(ky[8] - ky[9]);
        kd[1] = (solve(ky[0] - ky[4]) + solve(ky[2] - ky[6])) * 0.5f;
        kd[2] = (solve(ky[1] - ky[5]) + solve(ky[3] - ky[7])) * 0.5f;
        for (int g = 0; g < 3; ++g) kd[g] = dclamp(kd[g], c.depth_range[0], c.depth_range[1]);
    }
    Dual c_unc[3];
    for (int g = 0; g < 3; ++g) c_unc[g] = has_cu ? dclamp(X(c.ch[HK_KPT_UNC] + g), c.unc_lo, c.unc_hi) : K(0.f);
    // uncertainty-weighted combination of the depth estimates: all four, or (no depth_uncertainty) the three keypoint depths alone
    // (detector_loss.py:396-403); without corner_uncertainty there is no combination and `soft` stays 0
    const Dual comb_depth[4] = {p_depth, kd[0], kd[1], kd[2]};
    const Dual comb_unc[4] = {dexp(d_unc), dexp(c_unc[0]), dexp(c_unc[1]), dexp(c_unc[2])};
    const int c0 = has_du ? 0 : 1;                                   // first column of the combination
    Dual wsum = K(0.f), soft = K(0.f);
    int amin = c0;
    if (has_cu) {
        for (int i = c0; i < 4; ++i) wsum = wsum + K(1.f) / comb_unc[i];
        for (int i = c0; i < 4; ++i) soft = soft + comb_depth[i] * ((K(1.f) / comb_unc[i]) / wsum);
        for (int i = c0 + 1; i < 4; ++i) if (comb_unc[i].v < comb_unc[amin].v) amin = i;
    }
    Dual corner_depth = p_depth;                                     // CORNER_LOSS_DEPTH: direct
    if (c.corner_depth_mode == 1) corner_depth = (kd[0] + kd[1] + kd[2]) / 3.f;
    else if (c.corner_depth_mode == 2) corner_depth = soft;
    else if (c.corner_depth_mode == 3) corner_depth = comb_depth[amin];
    const Dual ox = X(c.ch[HK_OFF3D]), oy = X(c.ch[HK_OFF3D] + 1);
    const Vec3 p_loc = decode_location(px, py, ox, oy, corner_depth, cal, pad, c.down_ratio);
    // multi-bin yaw (anno_encoder.py:241-295): the most confident bin's residual + its centre, + the viewing-ray angle
    Dual p_roty;
    {
        int best = 0; float bconf = -1.f;
        for (int i = 0; i < 4; ++i) {
            const float a = X(c.ch[HK_ORI_CLS] + 2 * i).v, b = X(c.ch[HK_ORI_CLS] + 2 * i + 1).v;
            const float m = fmaxf(a, b), conf = expf(b - m) / (expf(a - m) + expf(b - m));
            if (conf > bconf) { bconf = conf; best = i; }
        }
        const float centers[4] = {0.f, PI / 2, PI, -PI / 2};
        const Dual alpha = datan2(X(c.ch[HK_ORI_OFF] + 2 * best), X(c.ch[HK_ORI_OFF] + 2 * best + 1)) + centers[best];
        p_roty = alpha + datan2(p_loc.x, p_loc.z);
        if (p_roty.v > PI) p_roty = p_roty - 2 * PI;
        if (p_roty.v < -PI) p_roty = p_roty + 2 * PI;
    }

    // ---- depth with aleatoric uncertainty (detector_loss.py:302-314) -----------------------------------------------------------
    {
        const Dual l1 = depth_loss<DEP>(p_depth, t_depth) * c.w[T_DEPTH];
        out[T_DEPTH] = (has_du ? l1 * dexp(-d_unc) + d_unc * c.w[T_DEPTH] : l1) * inv_v;
        out[V_REAL_DEPTH] = K(l1.v * inv_v);
    }
    // ---- projected-centre offset; truncated objects optionally in their own (log) term -----------------------------------------
    {
        const Dual l1 = reg_loss<REG>(ox - t[R_OFF]) + reg_loss<REG>(oy - t[R_OFF + 1]);
        const bool trunc = t[R_TRUNC] != 0.f;
        if (c.separate_trunc) {
            if (trunc) out[T_TRUNC_OFFSET] = (c.trunc_log ? dlog(l1 + 1.f) : l1) * (c.w[T_TRUNC_OFFSET] / cnt(N_TRUNC));
            else out[T_OFFSET] = l1 * (c.w[T_OFFSET] / cnt(N_V_INSIDE));
        } else {
            out[T_OFFSET] = l1 * (c.w[T_OFFSET] * inv_v);
        }
    }
    // ---- multi-bin orientation (detector_loss.py:495-517) ----------------------------------------------------------------------
    {
        Dual ce = K(0.f), rg = K(0.f);
        for (int i = 0; i < 4; ++i) {
            const Dual a = X(c.ch[HK_ORI_CLS] + 2 * i), b = X(c.ch[HK_ORI_CLS] + 2 * i + 1);
            const float m = fmaxf(a.v, b.v);
            const Dual lse = dlog(dexp(a - m) + dexp(b - m)) + m;
            const bool is_bin = t[R_ORI + i] == 1.f;
            ce = ce + (lse - ((int)t[R_ORI + i] == 1 ? b : a));
            if (is_bin) {
                const Dual s = X(c.ch[HK_ORI_OFF] + 2 * i), q = X(c.ch[HK_ORI_OFF] + 2 * i + 1);
                const Dual nr = dsqrt(s * s + q * q);
                const Dual dn = nr.v > 1e-12f ? nr : K(1e-12f);        // F.normalize: x / max(||x||, 1e-12)
                rg = rg + dabs(s / dn - sinf(t[R_ORI + 4 + i])) + dabs(q / dn - cosf(t[R_ORI + 4 + i]));
            }
        }
        out[T_ORIEN] = (ce * (inv_v / 4.f) + rg / cnt(N_ORI)) * c.w[T_ORIEN];
    }
    // ---- dimensions ------------------------------------------------------------------------------------------------------------
    {
        Dual l = K(0.f);
        for (int k = 0; k < 3; ++k) l = l + reg_loss<REG>(p_dims[k] - t[R_DIMS + k]) * c.dim_weight[k];
        out[T_DIMS] = l * (c.w[T_DIMS] * inv_v);
    }
    // ---- eight box corners, L1 per coordinate, mean over corners (detector_loss.py:338-339) -------------------------------------
    {
        const Vec3 t_loc = decode_location(px, py, K(t[R_OFF]), K(t[R_OFF + 1]), K(t_depth), cal, pad, c.down_ratio);
        const Dual t_dims[3] = {K(t[R_DIMS]), K(t[R_DIMS + 1]), K(t[R_DIMS + 2])};
        const Dual pc = dcos(p_roty), ps = dsin(p_roty), tc = K(cosf(t[R_ROTY])), ts = K(sinf(t[R_ROTY]));
        Dual l = K(0.f);
        for (int k = 0; k < 8; ++k) {
            const Vec3 a = box_corner(k, pc, ps, p_dims, p_loc), b = box_corner(k, tc, ts, t_dims, t_loc);
            l = l + reg_loss<REG>(a.x - b.x) + reg_loss<REG>(a.y - b.y) + reg_loss<REG>(a.z - b.z);
        }
        out[T_CORNER] = l * (c.w[T_CORNER] * inv_v / 8.f);
        // the logged 3D IoU of the same two boxes (detector_loss.py:333,436 get_iou_3d): values only, no tangent
        const float pl[3] = {p_loc.x.v, p_loc.y.v, p_loc.z.v}, pd[3] = {p_dims[0].v, p_dims[1].v, p_dims[2].v};
        const float tl[3] = {t_loc.x.v, t_loc.y.v, t_loc.z.v};
        out[V_IOU3D] = K(biou::iou_parts(pl, pd, pc.v, ps.v, tl, t + R_DIMS, tc.v, ts.v) * inv_v);
    }
    // ---- keypoints (visible ones) ----------------------------------------------------------------------------------------------
    if (has_kp) {
        Dual l = K(0.f);
        for (int j = 0; j < 10; ++j)
            l = l + (dabs(kx[j] - t[R_KP + 3 * j]) + dabs(ky[j] - t[R_KP + 3 * j + 1])) * t[R_KP + 3 * j + 2];
        out[T_KEYPOINT] = l * (c.w[T_KEYPOINT] / cnt(N_KMASK));
    }
    // ---- keypoint depths with their uncertainties; invalid groups only train the uncertainty (detector_loss.py:341-371); without
    // corner_uncertainty the valid ones are plain L1 and the invalid ones a detached constant (value, no gradient) ------------------
    if (has_kp) {
        Dual l = K(0.f);
        float lg = 0.f;
        for (int g = 0; g < 3; ++g) {
            const float wk = c.w[T_KEYPOINT_DEPTH];
            if (t[R_KDM + g] != 0.f) {
                const Dual l1 = reg_loss<REG>(kd[g] - t_depth) * wk;
                l = l + (has_cu ? l1 * dexp(-c_unc[g]) + c_unc[g] * wk : l1) / cnt(N_KD_VALID);
                lg += l1.v / cnt(N_KD_VALID);
            } else if (c.modify_invalid) {
                const Dual l1 = reg_loss<REG>(detach(kd[g]) - t_depth) * wk;
                l = l + (has_cu ? l1 * dexp(-c_unc[g]) : l1) / cnt(N_KD_INVALID);
            }
        }
        out[T_KEYPOINT_DEPTH] = l;
        out[V_VALID_KD] = K(lg);
    }
    // ---- the combined depth ----------------------------------------------------------------------------------------------------
    if (has_cu) out[T_SOFT_DEPTH] = reg_loss<REG>(soft - t_depth) * (c.w[T_SOFT_DEPTH] * inv_v);
    // ---- logged relative depth errors (detector_loss.py:396-482) ---------------------------------------------------------------
    {
        const float mae[4] = {fabsf(p_depth.v - t_depth) / t_depth, fabsf(kd[0].v - t_depth) / t_depth, fabsf(kd[1].v - t_depth) / t_depth,
                              fabsf(kd[2].v - t_depth) / t_depth};
        out[V_DEPTH_MAE] = K(mae[0] * inv_v);
        if (has_kp) { out[V_CENTER_MAE] = K(mae[1] * inv_v); out[V_02_MAE] = K(mae[2] * inv_v); out[V_13_MAE] = K(mae[3] * inv_v); }
        if (has_cu) {
            const float lower3 = fminf(mae[1], fminf(mae[2], mae[3]));
            const float mean = has_du ? 0.25f * (comb_depth[0].v + comb_depth[1].v + comb_depth[2].v + comb_depth[3].v)
                                      : (comb_depth[1].v + comb_depth[2].v + comb_depth[3].v) / 3.f;
            out[V_LOWER_MAE] = K((has_du ? fminf(fminf(mae[0], mae[1]), fminf(mae[2], mae[3])) : lower3) * inv_v);
            out[V_HARD_MAE] = K(mae[amin] * inv_v);
            out[V_SOFT_MAE] = K(fabsf(soft.v - t_depth) / t_depth * inv_v);
            out[V_MEAN_MAE] = K(fabsf(mean - t_depth) / t_depth * inv_v);
        }
    }
}

// L1 + L1 (LOSS_TYPE of runs/monoflex.yaml): mfx_object_loss
template <typename Reader>
MFX_HD void object_terms(const Reader& X, const float* t, const mfx_object_loss_cfg& c, const float* nrm, Dual* out) {
    object_terms_t<REG_L1, DEP_L1>(X, t, c, nrm, out);
}

// MFX_LOSS_KINDS(reg, dep, CALL): CALL(REG, DEP) with the two run-time kinds as compile-time constants (loss_kinds_ok checked by the caller)
#define MFX_LOSS_KINDS(reg, dep, CALL)                                                                                      \
    switch ((reg) * mfx::oloss::NUM_DEPTH_LOSS + (dep)) {                                                                   \
        case 0: CALL(0, 0); break; case 1: CALL(0, 1); break; case 2: CALL(0, 2); break;                                    \
        case 3: CALL(1, 0); break; case 4: CALL(1, 1); break; default: CALL(1, 2); break;                                   \
    }

// the eight batch-wide selection counts, accumulated row by row (callers reduce over rows)
MFX_HD void row_counts(const float* t, float* n) {
    for (int i = 0; i < NNORM; ++i) n[i] = 0.f;
    if (t[R_VALID] == 0.f) return;
    const float* box = t + R_BOX;
    n[N_V] = 1.f;
    n[N_V2D] = (box[3] - box[1] > 0.f && box[2] - box[0] > 0.f) ? 1.f : 0.f;
    n[N_TRUNC] = t[R_TRUNC] != 0.f ? 1.f : 0.f;
    n[N_V_INSIDE] = 1.f - n[N_TRUNC];
    for (int j = 0; j < 10; ++j) n[N_KMASK] += t[R_KP + 3 * j + 2];
    for (int g = 0; g < 3; ++g) { n[N_KD_VALID] += t[R_KDM + g] != 0.f ? 1.f : 0.f; n[N_KD_INVALID] += t[R_KDM + g] != 0.f ? 0.f : 1.f; }
    for (int i = 0; i < 4; ++i) n[N_ORI] += t[R_ORI + i] == 1.f ? 1.f : 0.f;
}

}  // namespace oloss
}  // namespace mfx
