// TEST-ONLY host build of monoflex_amd/csrc/box3d_iou_math.h: the one-lane-per-pair kernel as a plain loop over the pairs, so the CPU
// suite can check the float32 clip against the float64 reference without a GPU.  Not loaded by the product.
#include <cstddef>

#include "../../monoflex_amd/csrc/box3d_iou_math.h"

extern "C" void shim_box3d_iou_pairs(const float* a, const float* b, int N, int form, float* iou) {
    for (int n = 0; n < N; ++n)
        iou[n] = form == 0 ? mfx::biou::iou_rows(a + (size_t)n * 7, b + (size_t)n * 7)
                           : mfx::biou::iou_corners(a + (size_t)n * 24, b + (size_t)n * 24);
}
