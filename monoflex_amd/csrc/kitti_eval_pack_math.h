// Decode row -> evaluator record (mfx_kitti_eval_pack_*): the one statement of what the result-file round trip does to a value.
//
// The file path writes a detection with generate_kitti_3d_detection (evaluation.py; reference evaluate.py:34-52) and reads it
// back with parse_label_text (kitti_common.py:294-332).  Between the fp32 decode row
//   [cls, alpha, x1, y1, x2, y2, h, w, l, x, y, z, ry, score]
// and the fp64 record of mfx_kitti_eval_desc
//   [code, truncated, occluded, alpha, x1, y1, x2, y2, l, h, w, x, y, z, ry, score]
// lie `ndarray.round(4)` on a float32 array -- an fp32 multiply by 10000, rint (ties to even), a correctly rounded fp32
// DIVISION by 10000 (a multiply by 1e-4f differs on ~30 % of the values) -- then repr() and float(), which are exact for the
// widened value.  The class name maps back to the class id (ID_TYPE_CONVERSION 0/1/2 -> NAME_CODES car/pedestrian/cyclist),
// truncated and occluded are written as 0, and the dimensions change places: the file holds h, w, l, the record l, h, w.
// Plain C++ like kitti_eval_math.h, so tests/ compile the same rule for the host.  Build without fused multiply-add.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/monoflex_hip.h"

#include "hd.h"

namespace mfx {
namespace kpack {

constexpr int ROW = MFX_EVAL_DET_ROW, REC = MFX_EVAL_REC;

MFX_HD float round4(float v) {
  const float s = rintf(v * 10000.0f);
#ifdef __HIP_DEVICE_COMPILE__
  return __fdiv_rn(s, 10000.0f);
#else
  return s / 10000.0f;
#endif
}

MFX_HD void pack_record(const float* row, double* rec) {
  rec[0] = (double)(int)round4(row[0]);
  rec[1] = 0.0;
  rec[2] = 0.0;
  for (int k = 1; k <= 5; ++k) rec[2 + k] = (double)round4(row[k]);                 // alpha, x1, y1, x2, y2
  rec[8] = (double)round4(row[8]);                                                  // l
  rec[9] = (double)round4(row[6]);                                                  // h
  rec[10] = (double)round4(row[7]);                                                 // w
  for (int k = 9; k <= 13; ++k) rec[2 + k] = (double)round4(row[k]);                // x, y, z, ry, score
}

}  // namespace kpack
}  // namespace mfx
