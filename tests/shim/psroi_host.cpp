// Test-only host build of monoflex_amd/csrc/psroi_math.h: plain loops over (roi, class, bin, channel, sample) that call the SAME
// per-bin functions the gfx950 kernels of psroi_pool.hip call, in float.  tests/test_psroi_host_shim.py compiles this with g++ and
// compares it with tests/psroi_ref.py; it is never part of libmonoflex_hip.so.
#include "../../monoflex_amd/csrc/psroi_math.h"

#include <cstddef>

using namespace mfx::psroi;

namespace {

struct Dims {
  int B, C, H, W, N, num_classes, cpc, no_trans, P, part, S;
  float scale, trans_std;
};

// geometry of sample (ih, iw) of bin (ph, pw) of (roi n, class cls)
Sample<float> sample_of(const Dims& d, const Roi<float>& r, const float* trans, int n, int cls, int ph, int pw, int ih, int iw, size_t* cell) {
  const int part_h = part_index<float>(ph, d.P, d.part), part_w = part_index<float>(pw, d.P, d.part);
  *cell = ((((size_t)n * d.num_classes + cls) * 2) * d.part + part_h) * d.part + part_w;
  float tx = 0.f, ty = 0.f;
  if (!d.no_trans) {
    tx = trans[*cell] * d.trans_std;
    ty = trans[*cell + (size_t)d.part * d.part] * d.trans_std;
  }
  float wstart, hstart, w, h;
  bin_origin(r, ph, pw, tx, ty, wstart, hstart);
  sample_position(r, wstart, hstart, ih, iw, w, h);
  return sample_geometry(w, h, d.W, d.H);
}

Dims make_dims(int B, int C, int H, int W, int N, int trans_channels, int no_trans, float scale, int output_dim, int pooled, int part, int S, float trans_std) {
  Dims d;
  d.B = B; d.C = C; d.H = H; d.W = W; d.N = N; d.no_trans = no_trans; d.P = pooled; d.part = part; d.S = S; d.scale = scale; d.trans_std = trans_std;
  d.num_classes = no_trans ? 1 : trans_channels / 2;
  d.cpc = output_dim / d.num_classes;
  return d;
}

}  // namespace

extern "C" void shim_psroi_forward(const float* input, const float* rois, const float* trans, float* output, float* output_count,
                                   int B, int C, int H, int W, int N, int trans_channels, int no_trans, float scale, int output_dim,
                                   int pooled, int part, int S, float trans_std) {
  const Dims d = make_dims(B, C, H, W, N, trans_channels, no_trans, scale, output_dim, pooled, part, S, trans_std);
  for (int n = 0; n < N; ++n) {
    const Roi<float> r = roi_geometry(rois + (size_t)n * 5, scale, pooled, S);
    const bool image = r.batch >= 0 && r.batch < B;
    for (int ctop = 0; ctop < output_dim; ++ctop)
      for (int ph = 0; ph < pooled; ++ph)
        for (int pw = 0; pw < pooled; ++pw) {
          const size_t oi = (((size_t)n * output_dim + ctop) * pooled + ph) * pooled + pw;
          float sum = 0.f;
          int count = 0;
          if (image) {
            const float* plane = input + ((size_t)r.batch * C + ctop) * H * W;
            for (int ih = 0; ih < S; ++ih)
              for (int iw = 0; iw < S; ++iw) {
                size_t cell;
                const Sample<float> s = sample_of(d, r, trans, n, ctop / d.cpc, ph, pw, ih, iw, &cell);
                if (!s.valid) continue;
                sum += interpolate(plane[s.y0 * W + s.x0], plane[s.y1 * W + s.x0], plane[s.y0 * W + s.x1], plane[s.y1 * W + s.x1], s.dx, s.dy);
                ++count;
              }
          }
          output[oi] = count == 0 ? 0.f : sum / (float)count;
          output_count[oi] = (float)count;
        }
  }
}

// grad_input (B,C,H,W) and grad_trans (shape of trans; untouched when no_trans) must arrive zero-filled
extern "C" void shim_psroi_backward(const float* grad_out, const float* input, const float* rois, const float* trans, const float* top_count,
                                    float* grad_input, float* grad_trans, int B, int C, int H, int W, int N, int trans_channels, int no_trans,
                                    float scale, int output_dim, int pooled, int part, int S, float trans_std) {
  const Dims d = make_dims(B, C, H, W, N, trans_channels, no_trans, scale, output_dim, pooled, part, S, trans_std);
  for (int n = 0; n < N; ++n) {
    const Roi<float> r = roi_geometry(rois + (size_t)n * 5, scale, pooled, S);
    if (r.batch < 0 || r.batch >= B) continue;
    for (int ctop = 0; ctop < output_dim; ++ctop)
      for (int ph = 0; ph < pooled; ++ph)
        for (int pw = 0; pw < pooled; ++pw) {
          const size_t oi = (((size_t)n * output_dim + ctop) * pooled + ph) * pooled + pw;
          if (top_count[oi] <= 0.f) continue;
          const float diff_val = grad_out[oi] / top_count[oi];
          const float* plane = input + ((size_t)r.batch * C + ctop) * H * W;
          float* gplane = grad_input + ((size_t)r.batch * C + ctop) * H * W;
          for (int ih = 0; ih < S; ++ih)
            for (int iw = 0; iw < S; ++iw) {
              size_t cell;
              const Sample<float> s = sample_of(d, r, trans, n, ctop / d.cpc, ph, pw, ih, iw, &cell);
              if (!s.valid) continue;
              float q00, q01, q10, q11;
              corner_weights(s.dx, s.dy, q00, q01, q10, q11);
              gplane[s.y0 * W + s.x0] += q00 * diff_val;
              gplane[s.y1 * W + s.x0] += q01 * diff_val;
              gplane[s.y0 * W + s.x1] += q10 * diff_val;
              gplane[s.y1 * W + s.x1] += q11 * diff_val;
              if (no_trans) continue;
              const float u00 = plane[s.y0 * W + s.x0], u01 = plane[s.y1 * W + s.x0], u10 = plane[s.y0 * W + s.x1], u11 = plane[s.y1 * W + s.x1];
              grad_trans[cell] += offset_grad_x(u00, u01, u10, u11, s.dy, trans_std, diff_val, r.width);
              grad_trans[cell + (size_t)part * part] += offset_grad_y(u00, u01, u10, u11, s.dx, trans_std, diff_val, r.height);
            }
        }
  }
}
