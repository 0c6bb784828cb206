// Batch slot -> store row mapping of the resident input path (mfx_kitti_encode_targets_indexed,
// mfx_kitti_preprocess_u8_indexed).
//
// A resident store keeps the raw inputs of N samples on the device (records, n_obj, P, img_wh, right, and the uint8 frames
// with their offsets); a batch is B slots, slot b showing store row index[b].  The arithmetic is kitti_encode_math.h,
// unchanged: every function there reads the inputs of "image b" and writes the outputs of "image b", so slot b is served by a
// copy of the descriptor whose store-sized input pointers are moved by (row - b) rows.  Input element b of the copy is then
// element `row` of the store, while `flip` and every output stay batch-sized and are addressed by b as before.
//
// A row outside [0, N) is never dereferenced: the slot gets status bit 4 (STATUS_BAD_ROW) and all-zero outputs.
// Plain C++ like kitti_encode_math.h, so tests/ compile the same mapping for the host.
#pragma once
#include "kitti_encode_math.h"

namespace mfx {
namespace kitti {

constexpr int STATUS_BAD_ROW = 16;

MFX_HD bool row_ok(int row, int N) { return row >= 0 && row < N; }

// The descriptor as slot b sees it when it shows store row `row` (row_ok holds).
MFX_HD mfx_kitti_desc slot_desc(const mfx_kitti_desc& d, int b, int row) {
  mfx_kitti_desc s = d;
  const long k = (long)row - b;
  s.records = d.records + k * d.max_objs * REC;
  s.n_obj = d.n_obj + k;
  s.P = d.P + k * 12;
  s.img_wh = d.img_wh + k * 2;
  return s;
}

// Slot b of a bad row: the per-image scalars, one object row, one edge slot.  Together with a zero heat map and a zero
// frame these are all the outputs of the slot.
MFX_HD void bad_row_header(const mfx_kitti_desc& d, int b) {
  d.pad_size[b * 2] = 0; d.pad_size[b * 2 + 1] = 0;
  for (int k = 0; k < 12; ++k) d.P_out[b * 12 + k] = 0.0;
  d.edge_len[b] = 0;
  d.status[b] = STATUS_BAD_ROW;
}

MFX_HD void bad_row_object(const mfx_kitti_desc& d, int b, int i) {
  const long row = (long)b * d.max_objs + i;
  d.cls_ids[row] = 0; d.reg_mask[row] = 0; d.trunc_mask[row] = 0; d.reg_weight[row] = 0.f;
  d.rotys[row] = 0.f; d.alphas[row] = 0.f; d.occlusions[row] = 0.0; d.truncations[row] = 0.0;
  d.target_centers[row * 2] = 0; d.target_centers[row * 2 + 1] = 0;
  d.offset_3D[row * 2] = 0.f; d.offset_3D[row * 2 + 1] = 0.f;
  for (int k = 0; k < 30; ++k) d.keypoints[row * 30 + k] = 0.f;
  for (int k = 0; k < 3; ++k) { d.keypoints_depth_mask[row * 3 + k] = 0.f; d.dimensions[row * 3 + k] = 0.f; d.locations[row * 3 + k] = 0.f; }
  for (int k = 0; k < 4; ++k) { d.bboxes[row * 4 + k] = 0.f; d.gt_bboxes[row * 4 + k] = 0.f; d.heat_radius[row * 4 + k] = 0; }
  for (int k = 0; k < 8; ++k) d.orientations[row * 8 + k] = 0.f;
}

MFX_HD void bad_row_edge(const mfx_kitti_desc& d, int b, int k) {
  const int max_edge = 2 * (d.in_w / d.down + d.in_h / d.down);
  int64_t* e = d.edge_indices + ((long)b * max_edge + k) * 2;
  e[0] = 0; e[1] = 0;
}

// Output pixel (b, y, x) of the network input from store row `row`: preprocess_pixel with the two store-sized arrays moved.
MFX_HD void preprocess_pixel_row(const uint8_t* pixels, const int64_t* offsets, const int32_t* img_wh, int row, int N,
                                 const int32_t* flip, float* out, int b, int y, int x, int in_w, int in_h, const float* mean,
                                 const float* stdv, bool to_bgr) {
  if (!row_ok(row, N)) {
    const long plane = (long)in_w * in_h;
    float* o = out + (long)b * 3 * plane + (long)y * in_w + x;
    for (int c = 0; c < 3; ++c) o[c * plane] = 0.f;
    return;
  }
  const long k = (long)row - b;
  preprocess_pixel(pixels, offsets + k, img_wh + k * 2, flip, out, b, y, x, in_w, in_h, mean, stdv, to_bgr);
}

}  // namespace kitti
}  // namespace mfx
