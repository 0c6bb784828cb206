// Greedy suppression of duplicate detections on the device (C ABI mfx_box_nms; TEST.USE_NMS '2d' / '3d').  The semantics and the
// arithmetic are in box_nms_math.h; here one workgroup owns one image and runs that header's phases with its 256 lanes:
//   load         lane = row: the decode's row becomes a row of the LDS table (3D box with y at the centre, cos / sin of the yaw)
//   pairs        lane = row: its rank among the valid rows, by counting; then the lanes share the K (K - 1) / 2 pairs, one pair to a work
//                item, its answer one byte of an LDS table written by its one owner with a plain store
//   bits         the K x ceil(K / 64)-word bit matrix in LDS, rows in rank order: a work item packs one byte of it from the table
//   walk         one lane: K steps over the ranking, two 64-bit words per step, no load depending on a decision
//   store        lane = row: valid_out = valid_in & kept
// K <= 128 is a few thousand pairs at most: the launch is latency, not throughput.  No atomics, no global scratch, no workspace, nothing
// allocated, nothing synchronised -- capturable in a hipGraph.  The Sutherland-Hodgman rings of the rotated IoU (2 x 16 floats per lane,
// indexed at run time) would go to scratch memory as a private array; they are one column per lane of a [32][256] LDS table instead, the
// lane the fastest index, so a wavefront's accesses fall on 64 consecutive banks.  LDS: 58 KB per workgroup.
#include <hip/hip_runtime.h>

#include "../../include/monoflex_hip.h"
#include "box_nms_math.h"
#include "err.h"

namespace mfx {

constexpr int kNmsThreads = 256;

__global__ __launch_bounds__(kNmsThreads) void box_nms_kernel(const float* __restrict__ det, const int* valid_in, int K, int kind, float thresh,
                                                              int class_agnostic, int* valid_out) {
    __shared__ bnms::Image w;
    __shared__ float clip[bnms::CLIP * kNmsThreads];
    const int b = blockIdx.x, tid = threadIdx.x;
    bnms::phase_load(w, det + (size_t)b * K * 14, valid_in + (size_t)b * K, K, tid, kNmsThreads);
    __syncthreads();
    bnms::phase_pairs(w, K, kind, thresh, class_agnostic, 1, clip + tid, kNmsThreads, tid, kNmsThreads);
    __syncthreads();
    bnms::phase_bits(w, K, tid, kNmsThreads);
    __syncthreads();
    if (tid == 0) bnms::phase_walk(w, K);
    __syncthreads();
    bnms::phase_store(w, K, valid_out + (size_t)b * K, tid, kNmsThreads);
}

}  // namespace mfx

extern "C" int mfx_box_nms(const float* det, const int32_t* valid_in, int B, int K, int kind, float thresh, int class_agnostic,
                           int32_t* valid_out, void* stream) {
    if (B < 0 || K < 0) return mfx_fail(MFX_ERR_ARG, "box_nms: negative B or K");
    if (kind != MFX_NMS_2D && kind != MFX_NMS_3D) return mfx_fail(MFX_ERR_ARG, "box_nms: kind must be MFX_NMS_2D or MFX_NMS_3D");
    if (!(thresh >= 0.f && thresh < 1.f)) return mfx_fail(MFX_ERR_ARG, "box_nms: thresh must be in [0, 1)");
    if (K > mfx::bnms::MAXK) return mfx_fail(MFX_ERR_UNSUPPORTED, "box_nms: K <= 128 (one image's bit matrix and ranking live in one workgroup's LDS)");
    if (B == 0 || K == 0) return MFX_OK;
    if (!det || !valid_in || !valid_out) return mfx_fail(MFX_ERR_ARG, "box_nms: null pointer");
    hipLaunchKernelGGL(mfx::box_nms_kernel, dim3((unsigned)B), dim3(mfx::kNmsThreads), 0, reinterpret_cast<hipStream_t>(stream),
                       det, valid_in, K, kind, thresh, class_agnostic != 0 ? 1 : 0, valid_out);
    MFX_HIP_CHECK(hipGetLastError());
    ++g_cnt_box_nms;
    return MFX_OK;
}
