// TEST-ONLY host build of monoflex_amd/csrc/box_nms_math.h: the per-image function the kernel's workgroup runs phase by phase, run here by
// one lane, so the CPU suite can check the ranking, the bit matrix and the walk against the float64 restatement without a GPU.  Not loaded
// by the product.
#include <cstddef>

#include "../../monoflex_amd/csrc/box_nms_math.h"

using namespace mfx;

extern "C" void shim_box_nms(const float* det, const int* valid_in, int B, int K, int kind, float thresh, int class_agnostic, int early_out,
                             int* valid_out) {
    static bnms::Image w;
    for (int b = 0; b < B; ++b)
        bnms::nms_image(w, det + (size_t)b * K * 14, valid_in + (size_t)b * K, K, kind, thresh, class_agnostic, early_out, valid_out + (size_t)b * K);
}

// One pair of det rows: out[0] = the IoU as the kernel evaluates it (working-table rows, caller-owned clip rings at `stride`), out[1] =
// biou::iou_rows of the converted 7-float rows (the definition), out[2] = far_apart.
extern "C" void shim_box_nms_pair(const float* da, const float* db, int stride, float* out) {
    float a[bnms::BOXW], b[bnms::BOXW], clip[bnms::CLIP * 8];
    bnms::load_row(da, a);
    bnms::load_row(db, b);
    out[0] = bnms::iou_3d(a, b, clip, stride);
    const float ra[7] = {a[bnms::C_LOC], a[bnms::C_LOC + 1], a[bnms::C_LOC + 2], a[bnms::C_DIM], a[bnms::C_DIM + 1], a[bnms::C_DIM + 2], da[12]};
    const float rb[7] = {b[bnms::C_LOC], b[bnms::C_LOC + 1], b[bnms::C_LOC + 2], b[bnms::C_DIM], b[bnms::C_DIM + 1], b[bnms::C_DIM + 2], db[12]};
    out[1] = biou::iou_rows(ra, rb);
    out[2] = bnms::far_apart(a, b) ? 1.f : 0.f;
}

extern "C" float shim_box_nms_iou_2d(const float* a, const float* b) { return bnms::iou_2d(a, b); }
