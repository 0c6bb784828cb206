// TEST-ONLY host build of monoflex_amd/csrc/kitti_encode_math.h with the dataset switches (mfx_kitti_encode_cfg) and the
// INPUT.TO_BGR frame conversion: what kitti_objects_kernel / kitti_heatmap_kernel / kitti_preprocess_kernel map GPU threads
// onto, as plain loops.  cfg == NULL and right == NULL mean what they mean at mfx_kitti_encode_targets_cfg.
// Nothing in the product loads this.
#include "../../monoflex_amd/csrc/kitti_encode_math.h"

extern "C" void shim_kitti_encode_cfg(const mfx_kitti_desc* dp, const int32_t* right, const mfx_kitti_encode_cfg* cfgp) {
  const mfx_kitti_desc& d = *dp;
  const mfx_kitti_encode_cfg cfg = cfgp ? *cfgp : mfx::kitti::yaml_cfg();
  const int out_w = d.in_w / d.down, out_h = d.in_h / d.down, max_edge = 2 * (out_w + out_h);
  for (int b = 0; b < d.B; ++b) {
    mfx::kitti::image_header(d, b);
    for (int i = 0; i < d.max_objs; ++i) mfx::kitti::encode_object(d, b, i, right && right[b] != 0, cfg);
    for (int k = 0; k < max_edge; ++k) mfx::kitti::edge_point(d, b, k);
  }
  for (int b = 0; b < d.B; ++b)
    for (int c = 0; c < d.num_classes; ++c)
      for (int y = 0; y < out_h; ++y)
        for (int x = 0; x < out_w; ++x)
          d.hm[(((long)b * d.num_classes + c) * out_h + y) * out_w + x] = mfx::kitti::heat_pixel(d, b, c, y, x);
}

extern "C" void shim_kitti_preprocess_bgr(const uint8_t* pixels, const int64_t* offsets, const int32_t* img_wh, const int32_t* flip,
                                          float* out, int B, int in_w, int in_h, const float* mean3, const float* std3, int to_bgr) {
  for (int b = 0; b < B; ++b)
    for (int y = 0; y < in_h; ++y)
      for (int x = 0; x < in_w; ++x)
        mfx::kitti::preprocess_pixel(pixels, offsets, img_wh, flip, out, b, y, x, in_w, in_h, mean3, std3, to_bgr != 0);
}

extern "C" int shim_sizeof_encode_cfg() { return (int)sizeof(mfx_kitti_encode_cfg); }

// writes 1..4 through the members in declaration order, for the ctypes layout check
extern "C" void shim_fill_encode_cfg(mfx_kitti_encode_cfg* c) {
  c->consider_outside_objs = 1; c->adjust_boundary_heatmap = 2; c->keypoint_visible_modify = 3; c->heatmap_center_2d = 4;
}
