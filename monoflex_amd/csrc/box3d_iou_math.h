// Rotated 3D box IoU of one matched (predicted, target) pair -- C ABI mfx_box3d_iou_pairs, and value slot V_IOU3D of mfx_object_loss.
//
// Reference: get_iou_3d of model/layers/iou_loss.py:99-136 (the logged `3D_IoU`, model/head/detector_loss.py:333,436), which builds one
// shapely Polygon per box on the host.  By its definition, for upright boxes rotated about Y:
//   height overlap  = overlap of the intervals [-(y + h/2), -(y - h/2)]   (y = box centre, Y points down)
//   bottom overlap  = area of the intersection of the two x-z rectangles (corners 0..3 of encode_box3d, ring order)
//   IoU             = bottom * height / (area_a * h_a + area_b * h_b - bottom * height), each box with its OWN height.
// The intersection is a Sutherland-Hodgman clip of one convex quad by the four edge half-planes of the other, then a shoelace sum:
// every output vertex lies on a segment of the polygon being clipped, so coincident and collinear edges (identical boxes, boxes that
// differ in one parameter) cost at most a sliver of rounding-sized area -- there is no vertex ordering step that could fail on them.
// float32 throughout; both rectangles are translated to the target's centre first, so the coordinates that meet in the cross products
// are box-sized (metres), not scene-sized (tens of metres): area error ~ perimeter * 2^-24 * |coordinate|, far below 1e-4 of a union.
// kitti_eval_math.h-style: plain functions of one pair; box3d_iou.hip maps lanes onto them, object_loss_math.h calls them per object,
// tests/shim compiles them for the host.
#pragma once
#include <cmath>

#include "hd.h"

namespace mfx {
namespace biou {

constexpr int MAXV = 8;                                            // a quad clipped by four half-planes has at most eight vertices

// twice the signed area of a polygon of n vertices p[2 i], p[2 i + 1]
MFX_HD float shoelace2(const float* p, int n) {
    float s = 0.f;
    for (int i = 0; i < n; ++i) {
        const int j = i + 1 < n ? i + 1 : 0;
        s += p[2 * i] * p[2 * j + 1] - p[2 * j] * p[2 * i + 1];
    }
    return s;
}

// Area of the intersection of two convex quads a, b (4 x [x, z], ring order, either orientation).
MFX_HD float quad_intersection(const float* a, const float* b) {
    const float orient = shoelace2(b, 4) < 0.f ? -1.f : 1.f;      // inside = left of every edge of a counter-clockwise b
    float buf[2][2 * MAXV];
    int n = 4, cur = 0;
    for (int i = 0; i < 8; ++i) buf[0][i] = a[i];
    for (int e = 0; e < 4 && n > 0; ++e) {
        const float ex = b[2 * e], ez = b[2 * e + 1];
        const float dx = (b[2 * ((e + 1) & 3)] - ex) * orient, dz = (b[2 * ((e + 1) & 3) + 1] - ez) * orient;
        const float* in = buf[cur];
        float* out = buf[cur ^ 1];
        int m = 0;
        float px = in[2 * (n - 1)], pz = in[2 * (n - 1) + 1];
        float pd = dx * (pz - ez) - dz * (px - ex);                // > 0: strictly inside this edge's half-plane
        for (int i = 0; i < n; ++i) {
            const float qx = in[2 * i], qz = in[2 * i + 1];
            const float qd = dx * (qz - ez) - dz * (qx - ex);
            if ((pd >= 0.f) != (qd >= 0.f)) {                      // the segment crosses the edge's line: pd - qd != 0 and t in [0, 1]
                const float t = pd / (pd - qd);
                if (m < MAXV) { out[2 * m] = px + t * (qx - px); out[2 * m + 1] = pz + t * (qz - pz); ++m; }
            }
            if (qd >= 0.f && m < MAXV) { out[2 * m] = qx; out[2 * m + 1] = qz; ++m; }
            px = qx; pz = qz; pd = qd;
        }
        n = m;
        cur ^= 1;
    }
    return n < 3 ? 0.f : 0.5f * fabsf(shoelace2(buf[cur], n));
}

// IoU from the two bottom quads (already translated to a common nearby origin) and the two height intervals [lo, hi]
MFX_HD float iou_of(const float* qa, const float* qb, float lo_a, float hi_a, float lo_b, float hi_b) {
    const float h_ov = fmaxf(0.f, fminf(hi_a, hi_b) - fmaxf(lo_a, lo_b));
    const float area_a = 0.5f * fabsf(shoelace2(qa, 4)), area_b = 0.5f * fabsf(shoelace2(qb, 4));
    const float ov = h_ov > 0.f ? quad_intersection(qa, qb) * h_ov : 0.f;
    const float uni = area_a * (hi_a - lo_a) + area_b * (hi_b - lo_b) - ov;
    const float r = ov / uni;
    return (uni > 0.f && r >= 0.f && r <= 3.4e38f) ? r : 0.f;       // union <= 0 or anything not finite: 0, never NaN
}

// corners 0..3 of encode_box3d (anno_encoder.py:88-122; object_loss_math.h box_corner) in the x-z plane, the centre at (cx, cz)
MFX_HD void bottom_quad(float l, float w, float cs, float sn, float cx, float cz, float* q) {
    const float sx[4] = {-1.f, -1.f, 1.f, 1.f}, sz[4] = {-1.f, 1.f, 1.f, -1.f};
    for (int k = 0; k < 4; ++k) {
        const float x = 0.5f * l * sx[k], z = 0.5f * w * sz[k];
        q[2 * k] = cs * x + sn * z + cx;
        q[2 * k + 1] = -(sn * x) + cs * z + cz;
    }
}

// boxes as decoded parts: centre, (l, h, w), cos / sin of the yaw -- what the fused object loss holds.  b is the target: the origin.
MFX_HD float iou_parts(const float* loc_a, const float* dims_a, float cs_a, float sn_a,
                       const float* loc_b, const float* dims_b, float cs_b, float sn_b) {
    float qa[8], qb[8];
    bottom_quad(dims_a[0], dims_a[2], cs_a, sn_a, loc_a[0] - loc_b[0], loc_a[2] - loc_b[2], qa);
    bottom_quad(dims_b[0], dims_b[2], cs_b, sn_b, 0.f, 0.f, qb);
    const float ya = loc_a[1] - loc_b[1];
    return iou_of(qa, qb, -(ya + 0.5f * dims_a[1]), -(ya - 0.5f * dims_a[1]), -(0.5f * dims_b[1]), 0.5f * dims_b[1]);
}

// form 0: rows (x, y, z, l, h, w, ry), y = the box centre
MFX_HD float iou_rows(const float* a, const float* b) {
    return iou_parts(a, a + 3, cosf(a[6]), sinf(a[6]), b, b + 3, cosf(b[6]), sinf(b[6]));
}

// form 1: (8, 3) corner tables in encode_box3d order, as get_iou_3d receives them: heights from the mean y of corners 0..3 and 4..7,
// bottom polygon from corners 0..3 [x, z]
MFX_HD float iou_corners(const float* A, const float* B) {
    float ox = 0.f, oy = 0.f, oz = 0.f;
    for (int k = 0; k < 4; ++k) { ox += B[3 * k]; oz += B[3 * k + 2]; }
    for (int k = 0; k < 8; ++k) oy += B[3 * k + 1];
    ox *= 0.25f; oz *= 0.25f; oy *= 0.125f;
    float qa[8], qb[8], ya[2] = {0.f, 0.f}, yb[2] = {0.f, 0.f};
    for (int k = 0; k < 4; ++k) {
        qa[2 * k] = A[3 * k] - ox; qa[2 * k + 1] = A[3 * k + 2] - oz;
        qb[2 * k] = B[3 * k] - ox; qb[2 * k + 1] = B[3 * k + 2] - oz;
    }
    for (int k = 0; k < 8; ++k) { ya[k >> 2] += A[3 * k + 1] - oy; yb[k >> 2] += B[3 * k + 1] - oy; }
    return iou_of(qa, qb, -0.25f * ya[0], -0.25f * ya[1], -0.25f * yb[0], -0.25f * yb[1]);
}

// ---- the same arithmetic with the clip's two vertex rings in the CALLER's memory ------------------------------------------------------
// quad_intersection keeps its rings in a private array that is indexed at run time: a lane's 16 + 16 floats go to scratch memory (or to
// LDS the compiler sets aside).  A kernel whose workgroup holds a table in LDS with the lane as the fastest index (box_nms.hip) passes
// one column of it instead: 2 * 2 * MAXV floats, element k at buf[k * stride].  Statement for statement the functions above -- a host
// build gives bit-identical results (tests/test_box_nms_cpu.py compares them) -- kept beside them so that the units that call the private
// forms compile to the code they always did.
MFX_HD float quad_intersection_in(const float* a, const float* b, float* buf, int stride) {
    const float orient = shoelace2(b, 4) < 0.f ? -1.f : 1.f;
    int n = 4, cur = 0;
    for (int i = 0; i < 8; ++i) buf[i * stride] = a[i];
    for (int e = 0; e < 4 && n > 0; ++e) {
        const float ex = b[2 * e], ez = b[2 * e + 1];
        const float dx = (b[2 * ((e + 1) & 3)] - ex) * orient, dz = (b[2 * ((e + 1) & 3) + 1] - ez) * orient;
        const float* in = buf + cur * (2 * MAXV) * stride;
        float* out = buf + (cur ^ 1) * (2 * MAXV) * stride;
        int m = 0;
        float px = in[2 * (n - 1) * stride], pz = in[(2 * (n - 1) + 1) * stride];
        float pd = dx * (pz - ez) - dz * (px - ex);
        for (int i = 0; i < n; ++i) {
            const float qx = in[2 * i * stride], qz = in[(2 * i + 1) * stride];
            const float qd = dx * (qz - ez) - dz * (qx - ex);
            if ((pd >= 0.f) != (qd >= 0.f)) {
                const float t = pd / (pd - qd);
                if (m < MAXV) { out[2 * m * stride] = px + t * (qx - px); out[(2 * m + 1) * stride] = pz + t * (qz - pz); ++m; }
            }
            if (qd >= 0.f && m < MAXV) { out[2 * m * stride] = qx; out[(2 * m + 1) * stride] = qz; ++m; }
            px = qx; pz = qz; pd = qd;
        }
        n = m;
        cur ^= 1;
    }
    if (n < 3) return 0.f;
    const float* p = buf + cur * (2 * MAXV) * stride;
    float s = 0.f;                                                 // shoelace2 of the surviving ring
    for (int i = 0; i < n; ++i) {
        const int j = i + 1 < n ? i + 1 : 0;
        s += p[2 * i * stride] * p[(2 * j + 1) * stride] - p[2 * j * stride] * p[(2 * i + 1) * stride];
    }
    return 0.5f * fabsf(s);
}

MFX_HD float iou_of_in(const float* qa, const float* qb, float lo_a, float hi_a, float lo_b, float hi_b, float* buf, int stride) {
    const float h_ov = fmaxf(0.f, fminf(hi_a, hi_b) - fmaxf(lo_a, lo_b));
    const float area_a = 0.5f * fabsf(shoelace2(qa, 4)), area_b = 0.5f * fabsf(shoelace2(qb, 4));
    const float ov = h_ov > 0.f ? quad_intersection_in(qa, qb, buf, stride) * h_ov : 0.f;
    const float uni = area_a * (hi_a - lo_a) + area_b * (hi_b - lo_b) - ov;
    const float r = ov / uni;
    return (uni > 0.f && r >= 0.f && r <= 3.4e38f) ? r : 0.f;
}

// iou_parts; iou_rows(a, b) is this with cosf / sinf of the two yaws
MFX_HD float iou_parts_in(const float* loc_a, const float* dims_a, float cs_a, float sn_a,
                          const float* loc_b, const float* dims_b, float cs_b, float sn_b, float* buf, int stride) {
    float qa[8], qb[8];
    bottom_quad(dims_a[0], dims_a[2], cs_a, sn_a, loc_a[0] - loc_b[0], loc_a[2] - loc_b[2], qa);
    bottom_quad(dims_b[0], dims_b[2], cs_b, sn_b, 0.f, 0.f, qb);
    const float ya = loc_a[1] - loc_b[1];
    return iou_of_in(qa, qb, -(ya + 0.5f * dims_a[1]), -(ya - 0.5f * dims_a[1]), -(0.5f * dims_b[1]), 0.5f * dims_b[1], buf, stride);
}

}  // namespace biou
}  // namespace mfx
