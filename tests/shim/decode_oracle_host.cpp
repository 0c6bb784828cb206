// TEST-ONLY host build of monoflex_amd/csrc/decode_oracle_math.h: the function every lane of decode_boxes_multi_kernel asks which row its
// detection takes under OUTPUT_DEPTH 'oracle', run here over a list of detections against one image's ground-truth table, so the CPU suite
// can check the rule against the float32 restatement without a GPU.  Not loaded by the product.
#include <cstddef>

#include "../../monoflex_amd/csrc/decode_oracle_math.h"

using namespace mfx;

// boxes (N, 4), cls (N), score (N), d (N, 4) = direct, keypoint centre, 02, 13; gt (M, 8) -> choice (N): -1 or the column 0..3
extern "C" void shim_oracle_choose(const float* boxes, const int* cls, const float* score, float threshold, const float* d, int has_direct,
                                   const float* gt, int M, int N, int* choice) {
    for (int i = 0; i < N; ++i)
        choice[i] = dorc::choose(boxes + (size_t)i * 4, cls[i], score[i], threshold, d + (size_t)i * 4, has_direct != 0, gt, M);
}

extern "C" int shim_oracle_nearest(const float* box, int cls, const float* gt, int M) { return dorc::nearest_slot(box, cls, gt, M); }
extern "C" float shim_oracle_iou_2d(const float* a, const float* b) { return dorc::iou_2d(a, b); }
extern "C" float shim_oracle_centre_dis(const float* a, const float* b) { return dorc::centre_dis(a, b); }
extern "C" int shim_oracle_max_gt() { return dorc::MAX_GT; }
