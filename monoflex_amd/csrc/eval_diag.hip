// Validation diagnostics at the ground-truth centres (C ABI mfx_eval_diagnostics): the reference's TEST.EVAL_DEPTH / TEST.EVAL_DIS_IOUS
// tables (model/head/detector_infer.py:280-452), which it computes with tensor ops on the masked rows of one image.  The arithmetic is in
// eval_diag_math.h; here one lane owns one (image, object slot): it reads its gt row (16 floats) and its one contiguous NHWC regression row
// straight from global memory with scalar loads (no alignment assumed on ld / reg_off), decodes in registers / private memory and stores
// its 13 + 5 (+ 42) results.  B * M is a few hundred at most, so the launch is latency, not throughput: 64-lane workgroups, no LDS, no
// atomics, nothing allocated, nothing synchronised -- capturable in a hipGraph.  Fixed-shape outputs: empty slots are written as zeros.
#include <hip/hip_runtime.h>

#include "../../include/monoflex_hip.h"
#include "err.h"
#include "eval_diag_math.h"

namespace mfx {

__global__ __launch_bounds__(64) void eval_diagnostics_kernel(const float* __restrict__ hmap, int ld, int reg_off, const float* __restrict__ gt_rows,
                                                              int B, int M, int H, int W, const float* __restrict__ calib,
                                                              const int* __restrict__ pad, mfx_decode_cfg dc, mfx_head_layout hl, int want,
                                                              float* __restrict__ depth_err, float* __restrict__ iou, float* __restrict__ boxes) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= B * M) return;
    const int b = n / M;
    ediag::eval_object(hmap + (size_t)b * H * W * ld + reg_off, ld, H, W, gt_rows + (size_t)n * ediag::GT_ROW, calib + b * 6,
                       (float)pad[b * 2], (float)pad[b * 2 + 1], dc, hl, want,
                       depth_err ? depth_err + (size_t)n * ediag::NDEPTH : nullptr, iou ? iou + (size_t)n * ediag::NIOU : nullptr,
                       boxes ? boxes + (size_t)n * ediag::NBOX * 7 : nullptr);
}

}  // namespace mfx

extern "C" int mfx_eval_diagnostics(const float* hmap, int ld, int reg_off, const float* gt_rows, int B, int M, int H, int W,
                                    const float* calib, const int32_t* pad, const mfx_decode_cfg* cfg, const mfx_head_layout* heads,
                                    int want, float* depth_err, float* iou, float* boxes, void* stream) {
    if (!cfg) return mfx_fail(MFX_ERR_ARG, "eval_diagnostics: null cfg");
    if (!heads) return mfx_fail(MFX_ERR_ARG, "eval_diagnostics: null heads");
    if (const char* e = mfx::ediag::config_error(*cfg, *heads, want)) return mfx_fail_in(MFX_ERR_ARG, "eval_diagnostics", e);
    if (B < 0 || M < 0 || H < 1 || W < 1 || (long)B * M > 0x7fffffffL / 64 || reg_off < 0 || ld < heads->reg_width || reg_off + heads->reg_width > ld)
        return mfx_fail(MFX_ERR_ARG, "eval_diagnostics: need B, M >= 0, H, W >= 1 and the regression channels inside a row (reg_off + reg_width <= ld)");
    if (boxes && !(want & 2)) return mfx_fail(MFX_ERR_ARG, "eval_diagnostics: boxes given without want bit 1");
    if (B * M == 0) return MFX_OK;
    if (!hmap || !gt_rows || !calib || !pad || ((want & 1) && !depth_err) || ((want & 2) && !iou))
        return mfx_fail(MFX_ERR_ARG, "eval_diagnostics: null pointer");
    // an output that is not wanted is never written, whatever the caller passed
    hipLaunchKernelGGL(mfx::eval_diagnostics_kernel, dim3((unsigned)((B * M + 63) / 64)), dim3(64), 0, reinterpret_cast<hipStream_t>(stream),
                       hmap, ld, reg_off, gt_rows, B, M, H, W, calib, pad, *cfg, *heads, want, (want & 1) ? depth_err : nullptr,
                       (want & 2) ? iou : nullptr, boxes);
    MFX_HIP_CHECK(hipGetLastError());
    return MFX_OK;
}
