// KITTI input pipeline from a resident store (C ABI group 4): the kernels of kitti_encode.hip with a batch slot -> store row
// index in front.  The raw inputs of a whole split stay on the device (records, n_obj, P, img_wh, right: N rows; the uint8
// frames back to back with N offsets); a batch is B slots, slot b showing row index[b], flipped or not by flip[b].
// The arithmetic is kitti_encode_math.h, the mapping kitti_resident_map.h; this file maps threads onto them exactly as
// kitti_encode.hip does: one wave per image for the objects, one block per heat-map row, one thread per output pixel.
// A row outside [0, N) is not dereferenced: its slot gets status bit 4 and zero outputs (the block-uniform early branch).
#include <hip/hip_runtime.h>

#include "err.h"
#include "kitti_resident_map.h"

namespace mfx {

__global__ void __launch_bounds__(64) kitti_objects_indexed_kernel(mfx_kitti_desc d, const int32_t* index, int N, const int32_t* right,
                                                                   mfx_kitti_encode_cfg cfg) {
  const int b = blockIdx.x, row = index[b];          // uniform per block
  const int max_edge = 2 * (d.in_w / d.down + d.in_h / d.down);
  if (!kitti::row_ok(row, N)) {
    if (threadIdx.x == 0) kitti::bad_row_header(d, b);
    for (int i = threadIdx.x; i < d.max_objs; i += blockDim.x) kitti::bad_row_object(d, b, i);
    for (int k = threadIdx.x; k < max_edge; k += blockDim.x) kitti::bad_row_edge(d, b, k);
    return;
  }
  const mfx_kitti_desc s = kitti::slot_desc(d, b, row);
  const bool right_view = right && right[row] != 0;
  if (threadIdx.x == 0) kitti::image_header(s, b);
  __syncthreads();                                   // status[b] is initialised before any object ORs into it
  for (int i = threadIdx.x; i < d.max_objs; i += blockDim.x) kitti::encode_object(s, b, i, right_view, cfg);
  for (int k = threadIdx.x; k < max_edge; k += blockDim.x) kitti::edge_point(s, b, k);
}

__global__ void __launch_bounds__(256) kitti_heatmap_indexed_kernel(mfx_kitti_desc d, const int32_t* index, int N) {
  const int out_w = d.in_w / d.down, out_h = d.in_h / d.down;
  const int y = blockIdx.x % out_h, cls = (blockIdx.x / out_h) % d.num_classes, b = blockIdx.x / (out_h * d.num_classes);
  const int row = index[b];
  float* out = d.hm + (((long)b * d.num_classes + cls) * out_h + y) * out_w;
  if (!kitti::row_ok(row, N)) {
    for (int x = threadIdx.x; x < out_w; x += blockDim.x) out[x] = 0.f;
    return;
  }
  const mfx_kitti_desc s = kitti::slot_desc(d, b, row);
  for (int x = threadIdx.x; x < out_w; x += blockDim.x) out[x] = kitti::heat_pixel(s, b, cls, y, x);
}

struct Norm3 { float mean[3], stdv[3]; };

template <bool TO_BGR>
__global__ void __launch_bounds__(256) kitti_preprocess_indexed_kernel(const uint8_t* pixels, const int64_t* offsets, const int32_t* img_wh,
                                                                       const int32_t* index, int N, const int32_t* flip, float* out,
                                                                       int in_w, int in_h, Norm3 nm) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
  if (x < in_w) kitti::preprocess_pixel_row(pixels, offsets, img_wh, index[b], N, flip, out, b, y, x, in_w, in_h, nm.mean, nm.stdv, TO_BGR);
}

}  // namespace mfx

extern "C" int mfx_kitti_encode_targets_indexed(const mfx_kitti_desc* d, const int32_t* index, int32_t N, const int32_t* right,
                                                const mfx_kitti_encode_cfg* cfg, void* stream) {
  using namespace mfx;
  if (!d) return mfx_fail(MFX_ERR_ARG, "mfx_kitti_encode_targets_indexed: null descriptor");
  if (!index) return mfx_fail(MFX_ERR_ARG, "mfx_kitti_encode_targets_indexed: null index");
  if (N <= 0 || d->B <= 0 || d->max_objs <= 0 || d->num_classes <= 0 || d->down <= 0 || d->in_w % d->down || d->in_h % d->down)
    return mfx_fail(MFX_ERR_ARG, "mfx_kitti_encode_targets_indexed: bad sizes (N, B, max_objs, num_classes, down must be positive; input size divisible by down)");
  const void* ptrs[] = {d->records, d->n_obj, d->P, d->img_wh, d->flip, d->hm, d->cls_ids, d->target_centers, d->keypoints,
                        d->keypoints_depth_mask, d->dimensions, d->locations, d->reg_mask, d->reg_weight, d->offset_3D, d->bboxes,
                        d->gt_bboxes, d->rotys, d->trunc_mask, d->alphas, d->orientations, d->occlusions, d->truncations,
                        d->pad_size, d->edge_indices, d->edge_len, d->P_out, d->heat_radius, d->status};
  for (const void* p : ptrs)
    if (!p) return mfx_fail(MFX_ERR_ARG, "mfx_kitti_encode_targets_indexed: every input and output pointer of the descriptor must be set");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(kitti_objects_indexed_kernel, dim3(d->B), dim3(64), 0, st, *d, index, (int)N, right, cfg ? *cfg : kitti::yaml_cfg());
  const int out_h = d->in_h / d->down;
  hipLaunchKernelGGL(kitti_heatmap_indexed_kernel, dim3(d->B * d->num_classes * out_h), dim3(256), 0, st, *d, index, (int)N);
  MFX_HIP_CHECK(hipGetLastError());
  return MFX_OK;
}

extern "C" int mfx_kitti_preprocess_u8_indexed(const uint8_t* pixels, const int64_t* offsets, const int32_t* img_wh, const int32_t* index,
                                               const int32_t* flip, float* out, int B, int N, int in_w, int in_h, const float* mean3,
                                               const float* std3, int to_bgr, void* stream) {
  using namespace mfx;
  if (!pixels || !offsets || !img_wh || !index || !flip || !out || !mean3 || !std3)
    return mfx_fail(MFX_ERR_ARG, "mfx_kitti_preprocess_u8_indexed: null pointer");
  if (B <= 0 || N <= 0 || in_w <= 0 || in_h <= 0) return mfx_fail(MFX_ERR_ARG, "mfx_kitti_preprocess_u8_indexed: bad sizes");
  Norm3 nm;
  for (int c = 0; c < 3; ++c) { nm.mean[c] = mean3[c]; nm.stdv[c] = std3[c]; }
  hipLaunchKernelGGL(to_bgr ? kitti_preprocess_indexed_kernel<true> : kitti_preprocess_indexed_kernel<false>,
                     dim3((in_w + 255) / 256, in_h, B), dim3(256), 0, (hipStream_t)stream, pixels, offsets, img_wh, index, N, flip, out,
                     in_w, in_h, nm);
  MFX_HIP_CHECK(hipGetLastError());
  return MFX_OK;
}
