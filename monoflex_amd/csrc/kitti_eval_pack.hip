// Detections of a pass -> the evaluator's record table on the device (mfx_kitti_eval_pack_*, C ABI group 5).
// The record rule is kitti_eval_pack_math.h; this file maps one wave onto one image: lane k looks at slot k of (image, method),
// a ballot of the validity flags gives the image's detection count and, below each lane, its place among the valid slots -- the
// line the slot would have had in the image's result file.  The two scans between the launches are the caller's.
#include <hip/hip_runtime.h>

#include "err.h"
#include "kitti_eval_pack_math.h"

namespace mfx {

constexpr int PACK_WAVES = 4;                              // images per workgroup

// The validity ballot of image i, method m; `slot` is this lane's flag offset.  Every lane of a wave gets the same i.
__device__ __forceinline__ unsigned long long pack_ballot(const int32_t* valid, int i, int NM, int K, int m, int lane, long& slot) {
  slot = ((long)i * NM + m) * K + lane;
  return __ballot(lane < K && valid[slot] != 0);
}

__global__ void __launch_bounds__(64 * PACK_WAVES) kpack_count_kernel(const int32_t* valid, int N, int NM, int K, int m, const int32_t* gt_off,
                                                                      int32_t* n_det, int64_t* n_pair) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * PACK_WAVES + (threadIdx.x >> 6);
  if (i >= N) return;
  long slot;
  const unsigned long long mask = pack_ballot(valid, i, NM, K, m, lane, slot);
  if (lane == 0) {
    const int n = __popcll(mask);
    n_det[i] = n;
    n_pair[i] = (int64_t)n * (gt_off[i + 1] - gt_off[i]);
  }
}

__global__ void __launch_bounds__(64 * PACK_WAVES) kpack_rows_kernel(const float* det, const int32_t* valid, int N, int NM, int K, int m,
                                                                     const int32_t* dt_off, double* dt) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * PACK_WAVES + (threadIdx.x >> 6);
  if (i >= N) return;
  long slot;
  const unsigned long long mask = pack_ballot(valid, i, NM, K, m, lane, slot);
  if (!((mask >> lane) & 1ull)) return;
  const int below = __popcll(mask & ((1ull << lane) - 1ull));
  kpack::pack_record(det + slot * kpack::ROW, dt + ((long)dt_off[i] + below) * kpack::REC);
}

static int check_pack(const void* valid, int N, int NM, int K, int m) {
  if (N <= 0 || NM <= 0 || K <= 0 || m < 0 || m >= NM) return mfx_fail(MFX_ERR_ARG, "kitti_eval_pack: bad sizes");
  if (K > MFX_EVAL_MAX_DET) return mfx_fail(MFX_ERR_ARG, "kitti_eval_pack: at most 64 detections per image");
  if (!valid) return mfx_fail(MFX_ERR_ARG, "kitti_eval_pack: null pointer");
  return MFX_OK;
}

}  // namespace mfx
using namespace mfx;

extern "C" int mfx_kitti_eval_pack_count(const int32_t* valid, int N, int NM, int K, int m, const int32_t* gt_off, int32_t* n_det,
                                         int64_t* n_pair, void* stream) {
  if (int rc = check_pack(valid, N, NM, K, m)) return rc;
  if (!gt_off || !n_det || !n_pair) return mfx_fail(MFX_ERR_ARG, "kitti_eval_pack: null pointer");
  hipLaunchKernelGGL(kpack_count_kernel, dim3((N + PACK_WAVES - 1) / PACK_WAVES), dim3(64 * PACK_WAVES), 0, (hipStream_t)stream, valid, N, NM, K, m,
                     gt_off, n_det, n_pair);
  MFX_HIP_CHECK(hipGetLastError());
  return MFX_OK;
}

extern "C" int mfx_kitti_eval_pack_rows(const float* det, const int32_t* valid, int N, int NM, int K, int m, const int32_t* dt_off,
                                        double* dt, void* stream) {
  if (int rc = check_pack(valid, N, NM, K, m)) return rc;
  if (!det || !dt_off || !dt) return mfx_fail(MFX_ERR_ARG, "kitti_eval_pack: null pointer");
  hipLaunchKernelGGL(kpack_rows_kernel, dim3((N + PACK_WAVES - 1) / PACK_WAVES), dim3(64 * PACK_WAVES), 0, (hipStream_t)stream, det, valid, N, NM, K, m,
                     dt_off, dt);
  MFX_HIP_CHECK(hipGetLastError());
  return MFX_OK;
}
