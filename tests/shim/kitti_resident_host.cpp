// TEST-ONLY host build of monoflex_amd/csrc/kitti_resident_map.h over kitti_encode_math.h: what kitti_objects_indexed_kernel /
// kitti_heatmap_indexed_kernel / kitti_preprocess_indexed_kernel map GPU threads onto, as plain loops.  The descriptor's inputs
// and `right` are store-sized (N rows), its outputs, `flip` and `index` batch-sized; cfg == NULL and right == NULL mean what they
// mean at mfx_kitti_encode_targets_indexed.  Nothing in the product loads this.
#include "../../monoflex_amd/csrc/kitti_resident_map.h"

extern "C" void shim_kitti_encode_indexed(const mfx_kitti_desc* dp, const int32_t* index, int32_t N, const int32_t* right,
                                          const mfx_kitti_encode_cfg* cfgp) {
  using namespace mfx::kitti;
  const mfx_kitti_desc& d = *dp;
  const mfx_kitti_encode_cfg cfg = cfgp ? *cfgp : yaml_cfg();
  const int out_w = d.in_w / d.down, out_h = d.in_h / d.down, max_edge = 2 * (out_w + out_h);
  for (int b = 0; b < d.B; ++b) {
    const int row = index[b];
    if (!row_ok(row, N)) {
      bad_row_header(d, b);
      for (int i = 0; i < d.max_objs; ++i) bad_row_object(d, b, i);
      for (int k = 0; k < max_edge; ++k) bad_row_edge(d, b, k);
      continue;
    }
    const mfx_kitti_desc s = slot_desc(d, b, row);
    image_header(s, b);
    for (int i = 0; i < d.max_objs; ++i) encode_object(s, b, i, right && right[row] != 0, cfg);
    for (int k = 0; k < max_edge; ++k) edge_point(s, b, k);
  }
  for (int b = 0; b < d.B; ++b) {
    const int row = index[b];
    for (int c = 0; c < d.num_classes; ++c)
      for (int y = 0; y < out_h; ++y)
        for (int x = 0; x < out_w; ++x)
          d.hm[(((long)b * d.num_classes + c) * out_h + y) * out_w + x] = row_ok(row, N) ? heat_pixel(slot_desc(d, b, row), b, c, y, x) : 0.f;
  }
}

extern "C" void shim_kitti_preprocess_indexed(const uint8_t* pixels, const int64_t* offsets, const int32_t* img_wh, const int32_t* index,
                                              const int32_t* flip, float* out, int B, int N, int in_w, int in_h, const float* mean3,
                                              const float* std3, int to_bgr) {
  for (int b = 0; b < B; ++b)
    for (int y = 0; y < in_h; ++y)
      for (int x = 0; x < in_w; ++x)
        mfx::kitti::preprocess_pixel_row(pixels, offsets, img_wh, index[b], N, flip, out, b, y, x, in_w, in_h, mean3, std3, to_bgr != 0);
}
