// TEST-ONLY host build of monoflex_amd/csrc/kitti_encode_math.h with the per-sample view flag of
// mfx_kitti_encode_targets_views (right[b] = 1: right-camera sample, 2D boxes regenerated from the 3D corners).
// Same loop structure as kitti_encode_host.cpp; right == NULL is the left-view encoder.
#include "../../monoflex_amd/csrc/kitti_encode_math.h"

extern "C" void shim_kitti_encode_views(const mfx_kitti_desc* dp, const int32_t* right) {
  const mfx_kitti_desc& d = *dp;
  const int out_w = d.in_w / d.down, out_h = d.in_h / d.down, max_edge = 2 * (out_w + out_h);
  for (int b = 0; b < d.B; ++b) {
    mfx::kitti::image_header(d, b);
    const bool right_view = right && right[b] != 0;
    for (int i = 0; i < d.max_objs; ++i) mfx::kitti::encode_object(d, b, i, right_view);
    for (int k = 0; k < max_edge; ++k) mfx::kitti::edge_point(d, b, k);
  }
  for (int b = 0; b < d.B; ++b)
    for (int c = 0; c < d.num_classes; ++c)
      for (int y = 0; y < out_h; ++y)
        for (int x = 0; x < out_w; ++x)
          d.hm[(((long)b * d.num_classes + c) * out_h + y) * out_w + x] = mfx::kitti::heat_pixel(d, b, c, y, x);
}

// The regenerated right-view box of one object on its own (NaN and infinities included), for direct comparison.
extern "C" void shim_right_view_box(const double* P, double h, double w, double l, double ry, float t0, float t1, float t2,
                                    int img_w, int img_h, float* box) {
  mfx::kitti::right_view_box(P, h, w, l, ry, t0, t1, t2, img_w, img_h, box);
}
