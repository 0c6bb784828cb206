// Greedy suppression of duplicate detections of one image (C ABI mfx_box_nms; TEST.USE_NMS '2d' / '3d', TEST.NMS_THRESH,
// TEST.NMS_CLASS_AGNOSTIC).  The reference declares these keys (config/defaults.py) and reads them nowhere: the semantics are this
// project's, stated in INTEGRATION.md and restated in float64 by tests/box_nms_ref.py:
//   input   the decode's rows det[k][0:14] = cls, alpha, x1, y1, x2, y2, h, w, l, x, y (bottom centre), z, ry, score and valid[k]
//   order   valid rows by score (column 13) descending, ties to the lower slot k
//   walk    a row is kept unless an already KEPT row overlaps it with IoU > thresh (strict); a suppressed row suppresses nothing
//   class   unless class-agnostic, only rows of equal class id (column 0) meet
//   '2d'    axis-aligned IoU of columns 2:6 as _box_iou (model/head/detector_infer.py): no +1; 0 / 0 = NaN is not > thresh
//   '3d'    biou::iou_rows of the rows (x, y - h / 2, z, l, h, w, ry); the pair (i, j), i < j, is evaluated once, with j as the origin
//   output  valid_out[k] = valid[k] & kept[k]; invalid rows take no part
// Plain functions of one pair and PHASES of one image.  A phase does the work items `lane, lane + nlanes, ...`; every item writes
// memory no other item of the phase writes or reads, so the phases need a barrier between them and nothing else: box_nms.hip runs them
// with a workgroup's lanes and the working set in LDS, nms_image() below -- what tests/shim compiles for the host -- with one lane.
#pragma once
#include <cmath>
#include <cstddef>

#include "box3d_iou_math.h"
#include "hd.h"

namespace mfx {
namespace bnms {

constexpr int MAXK = 128;                                          // rows per image
constexpr int WORDS = MAXK / 64;                                   // 64-bit words per bit row
constexpr int ROWB = WORDS * 8;                                    // bytes per bit row
constexpr int KIND_2D = 1, KIND_3D = 2;                            // MFX_NMS_2D / MFX_NMS_3D
constexpr int CLIP = 2 * 2 * biou::MAXV;                           // floats of one lane's clip rings (biou::quad_intersection_in)
// a row of the working table
enum { C_CLS = 0, C_BOX = 1 /* x1, y1, x2, y2 */, C_LOC = 5 /* x, y centre, z */, C_DIM = 8 /* l, h, w */, C_CS = 11, C_SN = 12, C_KEY = 13, BOXW = 14 };

struct Image {                                                     // the working set of one image
    float box[MAXK][BOXW];
    int valid[MAXK];
    int order[MAXK];                                               // order[r] = slot of rank r among the valid rows, -1 past the last
    unsigned char hit[MAXK][MAXK];                                 // hit[i][j], i < j: the pair meets and overlaps above the threshold (one owner each)
    unsigned long long bits[MAXK][WORDS];                          // the K x ceil(K / 64) bit matrix, rows in RANK order: bit j of row r = slot
                                                                   // order[r] and slot j overlap (hit mirrored below the diagonal)
    unsigned long long kept[WORDS];
};

// _box_iou in float32: max(x, 0) as Python evaluates it (a NaN stays a NaN), no +1, 0 / 0 = NaN
MFX_HD float iou_2d(const float* a, const float* b) {
    const float dw = fminf(a[2], b[2]) - fmaxf(a[0], b[0]), dh = fminf(a[3], b[3]) - fmaxf(a[1], b[1]);
    const float inter = (0.f > dw ? 0.f : dw) * (0.f > dh ? 0.f : dh);
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter);
}

// one det row -> one row of the working table.  A NaN score ranks last.  (KIND_2D never reads cos / sin; it still gets them: one code path)
MFX_HD void load_row(const float* d, float* r) {
    r[C_CLS] = d[0];
    for (int i = 0; i < 4; ++i) r[C_BOX + i] = d[2 + i];
    r[C_LOC] = d[9]; r[C_LOC + 1] = d[10] - d[6] / 2.f; r[C_LOC + 2] = d[11];
    r[C_DIM] = d[8]; r[C_DIM + 1] = d[6]; r[C_DIM + 2] = d[7];
    r[C_CS] = cosf(d[12]); r[C_SN] = sinf(d[12]);
    r[C_KEY] = d[13] == d[13] ? d[13] : -INFINITY;
}

// Conservative early-out of '3d': the circles around the two bottom rectangles are apart by more than 4.8 % of the sum of their radii
// (d^2 > 1.1 * 2 (ra^2 + rb^2) >= 1.1 (ra + rb)^2, r^2 = (l^2 + w^2) / 4).  Every vertex the clip would meet is then outside one of its
// half-planes by that distance, far beyond float32 rounding: the clip returns exactly 0, the IoU is 0 and not > thresh.  Anything not
// finite compares false here and takes the full evaluation.
MFX_HD bool far_apart(const float* a, const float* b) {
    const float dx = a[C_LOC] - b[C_LOC], dz = a[C_LOC + 2] - b[C_LOC + 2];
    return dx * dx + dz * dz > 0.55f * (a[C_DIM] * a[C_DIM] + a[C_DIM + 2] * a[C_DIM + 2] + b[C_DIM] * b[C_DIM] + b[C_DIM + 2] * b[C_DIM + 2]);
}

MFX_HD float iou_3d(const float* a, const float* b, float* clip, int clip_stride) {
    return biou::iou_parts_in(a + C_LOC, a + C_DIM, a[C_CS], a[C_SN], b + C_LOC, b + C_DIM, b[C_CS], b[C_SN], clip, clip_stride);
}

// rows a, b of the working table, slot of a < slot of b
MFX_HD bool pair_overlaps(const float* a, const float* b, int kind, float thresh, int early_out, float* clip, int clip_stride) {
    if (kind == KIND_2D) return iou_2d(a + C_BOX, b + C_BOX) > thresh;
    if (early_out && far_apart(a, b)) return false;
    return iou_3d(a, b, clip, clip_stride) > thresh;
}

// does row (key a, slot ia) rank before row (key b, slot ib)
MFX_HD bool ranks_before(float a, int ia, float b, int ib) { return a > b || (a == b && ia < ib); }

// ---- phases ----------------------------------------------------------------------------------------------------------------------------
// item = row: the working table's row, its validity, order[] reset
MFX_HD void phase_load(Image& w, const float* det, const int* valid_in, int K, int lane, int nlanes) {
    for (int i = lane; i < K; i += nlanes) {
        load_row(det + (size_t)i * 14, w.box[i]);
        w.valid[i] = valid_in[i] != 0 ? 1 : 0;
        w.order[i] = -1;
    }
}

// item = row: its rank among the valid rows (a count: K <= 128 needs no sort); item = pair (i, j), i < j: hit[i][j].  Pairs with an invalid
// row or, unless class-agnostic, of different classes are dropped before any IoU.  clip: this lane's column of the clip table.
MFX_HD void phase_pairs(Image& w, int K, int kind, float thresh, int class_agnostic, int early_out, float* clip, int clip_stride,
                        int lane, int nlanes) {
    for (int i = lane; i < K; i += nlanes) {
        if (!w.valid[i]) continue;
        int rank = 0;
        for (int j = 0; j < K; ++j) rank += (w.valid[j] && ranks_before(w.box[j][C_KEY], j, w.box[i][C_KEY], i)) ? 1 : 0;
        w.order[rank] = i;
    }
    for (int u = lane; u < K * K; u += nlanes) {
        const int i = u / K, j = u - i * K;
        if (j <= i) continue;
        bool over = w.valid[i] && w.valid[j] && (class_agnostic || w.box[i][C_CLS] == w.box[j][C_CLS]);
        if (over) over = pair_overlaps(w.box[i], w.box[j], kind, thresh, early_out, clip, clip_stride);
        w.hit[i][j] = over ? 1 : 0;
    }
}

// item = (rank r, byte q of its bit row): eight pairs of the slot of that rank, read from either side of the diagonal
MFX_HD void phase_bits(Image& w, int K, int lane, int nlanes) {
    for (int u = lane; u < K * ROWB; u += nlanes) {
        const int r = u / ROWB, q = u - r * ROWB, i = w.order[r];
        unsigned bits = 0;
        if (i >= 0)
            for (int jj = 0; jj < 8; ++jj) {
                const int j = 8 * q + jj;
                if (j >= K || j == i) continue;
                bits |= (unsigned)(j < i ? w.hit[j][i] : w.hit[i][j]) << jj;
            }
        reinterpret_cast<unsigned char*>(w.bits[r])[q] = (unsigned char)bits;
    }
}

// ONE lane: the greedy walk over the ranking.  No load depends on `kept`: the K rows stream in while the chain of decisions runs.
MFX_HD void phase_walk(Image& w, int K) {
    unsigned long long kept[WORDS];
    for (int v = 0; v < WORDS; ++v) kept[v] = 0ull;
    for (int r = 0; r < K; ++r) {
        const int c = w.order[r];
        unsigned long long hit = 0ull;
        for (int v = 0; v < WORDS; ++v) hit |= w.bits[r][v] & kept[v];
        if (c >= 0 && !hit) kept[c >> 6] |= 1ull << (c & 63);
    }
    for (int v = 0; v < WORDS; ++v) w.kept[v] = kept[v];
}

// item = row
MFX_HD void phase_store(const Image& w, int K, int* valid_out, int lane, int nlanes) {
    for (int i = lane; i < K; i += nlanes) valid_out[i] = (w.valid[i] && ((w.kept[i >> 6] >> (i & 63)) & 1ull)) ? 1 : 0;
}

// The image as one lane runs it.  valid_out may alias valid_in: phase_load has read every valid_in before phase_store writes.
MFX_HD void nms_image(Image& w, const float* det, const int* valid_in, int K, int kind, float thresh, int class_agnostic, int early_out,
                      int* valid_out) {
    float clip[CLIP];
    phase_load(w, det, valid_in, K, 0, 1);
    phase_pairs(w, K, kind, thresh, class_agnostic, early_out, clip, 1, 0, 1);
    phase_bits(w, K, 0, 1);
    phase_walk(w, K);
    phase_store(w, K, valid_out, 0, 1);
}

}  // namespace bnms
}  // namespace mfx
