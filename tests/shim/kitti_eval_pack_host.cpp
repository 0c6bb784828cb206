// TEST-ONLY host build of monoflex_amd/csrc/kitti_eval_pack_math.h: the record rule kpack_rows_kernel applies to each valid
// slot, as plain loops.  Nothing in the product loads this.
#include "../../monoflex_amd/csrc/kitti_eval_pack_math.h"

// n fp32 values -> the fp64 value the result-file round trip gives each.
extern "C" void shim_kitti_pack_round4(const float* in, long n, double* out) {
  for (long i = 0; i < n; ++i) out[i] = (double)mfx::kpack::round4(in[i]);
}

// n decode rows (n, 14) -> n evaluator records (n, 16).
extern "C" void shim_kitti_pack_records(const float* rows, long n, double* rec) {
  for (long i = 0; i < n; ++i) mfx::kpack::pack_record(rows + i * mfx::kpack::ROW, rec + i * mfx::kpack::REC);
}
