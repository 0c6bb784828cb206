// Per-ROI / per-bin / per-sample arithmetic of deformable position-sensitive ROI pooling (mfx_dcn_v2_psroi_pooling_forward / _backward).
//
// Semantics: the reference's src/cuda/dcn_v2_psroi_pooling_cuda.cu:59-146 (forward) and :149-269 (backward), restated as small
// functions of one ROI, one bin or one sample, so that psroi_pool.hip only maps threads onto them.  They are plain C++ over
// <cmath>, templated on the arithmetic type: the shipped library instantiates them with float in device code, tests/ compile
// this header for the host (tests/shim/psroi_host.cpp) and run the same expressions on the CPU.
//
// The backward expressions are the reference's FORMULAS, not the derivative of the forward: where a sample was clamped to the
// map, the offset gradient ignores the clamp (:255-262).
#pragma once
#include <cmath>

#include "hd.h"

namespace mfx {
namespace psroi {

template <typename T>
struct Roi {
  int batch;                    // (int) roi[0]: truncation, :88
  T start_w, start_h;           // feature-map coordinates of the ROI's first sample column / row
  T width, height;              // floored at 0.1
  T bin_w, bin_h;               // width / pooled
  T sub_w, sub_h;               // bin / sample_per_part
};

// roi = (batch_index, x1, y1, x2, y2); `round` is C round (half away from zero), :88-103
template <typename T>
MFX_HD Roi<T> roi_geometry(const T* roi, T scale, int pooled, int sample_per_part) {
  Roi<T> r;
  r.batch = (int)roi[0];
  r.start_w = std::round(roi[1]) * scale - (T)0.5;
  r.start_h = std::round(roi[2]) * scale - (T)0.5;
  const T end_w = (std::round(roi[3]) + (T)1) * scale - (T)0.5;
  const T end_h = (std::round(roi[4]) + (T)1) * scale - (T)0.5;
  const T w = end_w - r.start_w, h = end_h - r.start_h;
  r.width = w > (T)0.1 ? w : (T)0.1;
  r.height = h > (T)0.1 ? h : (T)0.1;
  r.bin_w = r.width / (T)pooled;
  r.bin_h = r.height / (T)pooled;
  r.sub_w = r.bin_w / (T)sample_per_part;
  r.sub_h = r.bin_h / (T)sample_per_part;
  return r;
}

// which offset cell a pooled row / column reads, :105-106
template <typename T>
MFX_HD int part_index(int p, int pooled, int part_size) {
  return (int)std::floor((T)p / (T)pooled * (T)part_size);
}

// first sample of bin (ph, pw); trans_x / trans_y are the offsets already multiplied by trans_std, :111-114
template <typename T>
MFX_HD void bin_origin(const Roi<T>& r, int ph, int pw, T trans_x, T trans_y, T& wstart, T& hstart) {
  wstart = (T)pw * r.bin_w + r.start_w;
  wstart += trans_x * r.width;
  hstart = (T)ph * r.bin_h + r.start_h;
  hstart += trans_y * r.height;
}

// sample (ih, iw) of a bin, :128-129
template <typename T>
MFX_HD void sample_position(const Roi<T>& r, T wstart, T hstart, int ih, int iw, T& w, T& h) {
  w = wstart + (T)iw * r.sub_w;
  h = hstart + (T)ih * r.sub_h;
}

template <typename T>
struct Sample {
  int valid;                    // 0: dropped (outside [-0.5, W-0.5] x [-0.5, H-0.5])
  int x0, x1, y0, y1;           // floor / ceil corners of the clamped position (they coincide at an integer coordinate)
  T dx, dy;                     // distance to the floor corner
};

// :131-136 and :41-46 / :236-240
template <typename T>
MFX_HD Sample<T> sample_geometry(T w, T h, int W, int H) {
  Sample<T> s;
  s.valid = !(w < (T)-0.5 || w > (T)W - (T)0.5 || h < (T)-0.5 || h > (T)H - (T)0.5);
  s.x0 = s.x1 = s.y0 = s.y1 = 0;
  s.dx = s.dy = (T)0;
  if (!s.valid) return s;
  w = w > (T)0 ? w : (T)0;
  w = w < (T)(W - 1) ? w : (T)(W - 1);
  h = h > (T)0 ? h : (T)0;
  h = h < (T)(H - 1) ? h : (T)(H - 1);
  s.x0 = (int)std::floor(w);
  s.x1 = (int)std::ceil(w);
  s.y0 = (int)std::floor(h);
  s.y1 = (int)std::ceil(h);
  s.dx = w - (T)s.x0;
  s.dy = h - (T)s.y0;
  return s;
}

// bilinear weights of the corners (y0,x0), (y1,x0), (y0,x1), (y1,x1), :241-244
template <typename T>
MFX_HD void corner_weights(T dx, T dy, T& q00, T& q01, T& q10, T& q11) {
  q00 = ((T)1 - dx) * ((T)1 - dy);
  q01 = ((T)1 - dx) * dy;
  q10 = dx * ((T)1 - dy);
  q11 = dx * dy;
}

// u00 = data(y0,x0), u01 = data(y1,x0), u10 = data(y0,x1), u11 = data(y1,x1), :47-54
template <typename T>
MFX_HD T interpolate(T u00, T u01, T u10, T u11, T dx, T dy) {
  return ((T)1 - dx) * ((T)1 - dy) * u00 + ((T)1 - dx) * dy * u01 + dx * ((T)1 - dy) * u10 + dx * dy * u11;
}

// one sample's contribution to the gradient of its offset cell, :259-262 (diff_val = grad_out / count)
template <typename T>
MFX_HD T offset_grad_x(T u00, T u01, T u10, T u11, T dy, T trans_std, T diff_val, T roi_width) {
  T d = (u11 * dy + u10 * ((T)1 - dy) - u01 * dy - u00 * ((T)1 - dy)) * trans_std * diff_val;
  d *= roi_width;
  return d;
}

template <typename T>
MFX_HD T offset_grad_y(T u00, T u01, T u10, T u11, T dx, T trans_std, T diff_val, T roi_height) {
  T d = (u11 * dx + u01 * ((T)1 - dx) - u10 * dx - u00 * ((T)1 - dx)) * trans_std * diff_val;
  d *= roi_height;
  return d;
}

}  // namespace psroi
}  // namespace mfx
