// Rotated 3D box IoU of matched box pairs (C ABI mfx_box3d_iou_pairs).  Reference: get_iou_3d, model/layers/iou_loss.py:99-136,
// which loops over the pairs on the host with one shapely Polygon each.  The arithmetic is in box3d_iou_math.h; here one lane owns
// one pair: its two rows (7 or 24 floats) are read straight from global memory, the clip runs in the lane's own registers / private
// memory, and the result leaves through one vector store.  N is a few hundred at most (B * MAX_OBJECTS), so the launch is latency,
// not throughput: 64-lane workgroups, no LDS, no atomics, nothing allocated, nothing synchronised -- capturable in a hipGraph.
#include <hip/hip_runtime.h>

#include "../../include/monoflex_hip.h"
#include "box3d_iou_math.h"
#include "err.h"

namespace mfx {

__global__ __launch_bounds__(64) void box3d_iou_pairs_kernel(const float* __restrict__ a, const float* __restrict__ b, int N, int form,
                                                             float* __restrict__ iou) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    iou[n] = form == 0 ? biou::iou_rows(a + (size_t)n * 7, b + (size_t)n * 7) : biou::iou_corners(a + (size_t)n * 24, b + (size_t)n * 24);
}

}  // namespace mfx

extern "C" int mfx_box3d_iou_pairs(const float* boxes_a, const float* boxes_b, int N, int form, float* iou, void* stream) {
    if (N < 0) return mfx_fail(MFX_ERR_ARG, "box3d_iou_pairs: negative pair count");
    if (form != 0 && form != 1) return mfx_fail(MFX_ERR_ARG, "box3d_iou_pairs: form must be 0 (7-float rows) or 1 ((8, 3) corner tables)");
    if (N == 0) return MFX_OK;
    if (!boxes_a || !boxes_b || !iou) return mfx_fail(MFX_ERR_ARG, "box3d_iou_pairs: null pointer");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(mfx::box3d_iou_pairs_kernel, dim3((unsigned)(((long)N + 63) / 64)), dim3(64), 0, st, boxes_a, boxes_b, N, form, iou);
    MFX_HIP_CHECK(hipGetLastError());
    return MFX_OK;
}
