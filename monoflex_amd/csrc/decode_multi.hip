// Several depth modes of the box decode, and the reference's 'oracle', from one launch (C ABI mfx_decode_boxes_multi; `--eval_all_depths`,
// engine/inference.py:131-198, and `output_depth = 'oracle'`, detector_infer.py:199-202).  The depth mode enters a detection row through the
// location, roty, the uncertainty-scaled score and unc only: one workgroup per image ranks the ncls * K candidates as decode_boxes_kernel
// does, each of its first K lanes decodes what no mode changes ONCE (bdec::shared_part: 2D box, dimensions, alpha, the four estimates) and
// then finishes one row per requested mode (bdec::combine + bdec::finish_row, the expressions of bdec::decode_row).  Under the oracle bit the
// image's ground-truth rows are staged in LDS and every lane asks decode_oracle_math.h which single-estimate mode (or 'mean') its detection
// takes; that slice is then finished by the same code as the others, so an oracle row IS the row of its chosen mode.
// Latency-bound like decode_boxes_kernel (K * 50 values read, K * NM * 16 written per image); no atomics, no workspace, no synchronisation.
#include "../../include/monoflex_hip.h"
#include "common.h"
#include "box_decode_math.h"
#include "decode_oracle_math.h"
#include "err.h"

namespace mfx {

constexpr int kMultiThreads = 256;
constexpr uint32_t kOracleBit = 1u << MFX_DEPTH_ORACLE;

// (value desc, index asc) ordering; ties go to the lower position: select_topk stage 2, as decode.hip ranks
__device__ __forceinline__ bool ranks_first(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

__global__ __launch_bounds__(kMultiThreads) void decode_boxes_multi_kernel(const float* hmap, int ld, int reg_off, const float* scores, const int* index,
                                                                           int ncls, int H, int W, int K, const float* calib, const int* pad,
                                                                           const int* img_size, float threshold, mfx_decode_cfg dc, mfx_head_layout hl,
                                                                           uint32_t modes, int NM, const float* gt_rows, int M,
                                                                           float* det, float* topk, int* valid, float* unc, int* oracle_choice) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* cs = reinterpret_cast<float*>(smem_raw);          // [ncls*K]
    int* ci = reinterpret_cast<int*>(cs + ncls * K);         // [ncls*K]
    int* slot = ci + ncls * K;                               // [K] position (in the ncls*K list) of rank j
    __shared__ float gt[dorc::MAX_GT * dorc::GT_ROW];        // the image's ground-truth table (oracle bit only)
    const int b = blockIdx.x, tid = threadIdx.x, n = ncls * K;
    const bool oracle = (modes & kOracleBit) != 0;
    for (int t = tid; t < n; t += blockDim.x) { cs[t] = scores[(size_t)b * n + t]; ci[t] = index[(size_t)b * n + t]; }
    if (oracle)
        for (int t = tid; t < M * dorc::GT_ROW; t += blockDim.x) gt[t] = gt_rows[(size_t)b * M * dorc::GT_ROW + t];
    __syncthreads();
    // select_topk stage 2 (utils.py:88-91): top-K of the concatenated list, ties -> lower position
    for (int t = tid; t < n; t += blockDim.x) {
        const float v = cs[t];
        int rank = 0;
        for (int u = 0; u < n; ++u) rank += ranks_first(cs[u], u, v, t) ? 1 : 0;
        if (rank < K) slot[rank] = t;
    }
    __syncthreads();
    if (tid >= K) return;
    const int j = tid, pos = slot[j];
    const int cls = pos / K;                                  // utils.py:91 (integer floor division)
    const float score = cs[pos];
    const int idx = ci[pos];
    const int ys = idx / W, xs = idx - ys * W;                // utils.py:80-81
    const float* r = hmap + ((size_t)b * H * W + idx) * ld + reg_off;   // POI gather: one contiguous NHWC row
    const bdec::Camera cam = {calib[b * 6 + 0], calib[b * 6 + 1], calib[b * 6 + 2], calib[b * 6 + 3], calib[b * 6 + 4], calib[b * 6 + 5],
                              (float)pad[b * 2], (float)pad[b * 2 + 1]};
    const float px = (float)xs, py = (float)ys;
    // the 2D box clamp uses image 0's padded size
    bdec::Shared sh;
    bdec::shared_part(r, px, py, cls, cam, (float)(img_size[0] - 1), (float)(img_size[1] - 1), dc, hl, sh);
    const bool has_du = hl.ch[bdec::HK_DEPTH_UNC] >= 0, has_cu = hl.ch[bdec::HK_KPT] >= 0 && hl.ch[bdec::HK_KPT_UNC] >= 0;

    float* t = topk + ((size_t)b * K + j) * 5;
    t[0] = score; t[1] = (float)idx; t[2] = (float)cls; t[3] = py; t[4] = px;
    valid[b * K + j] = score >= threshold ? 1 : 0;

    // the oracle slice's mode: the chosen column's own decode mode, or 'mean'
    int oracle_mode = MFX_DEPTH_MEAN;
    if (oracle) {
        const int col = dorc::choose(sh.box, cls, score, threshold, sh.e.d, has_du, gt, M);
        if (col == 0) oracle_mode = MFX_DEPTH_DIRECT;
        else if (col > 0) oracle_mode = MFX_DEPTH_KEYPOINTS_CENTER + (col - 1);
        if (oracle_choice) oracle_choice[b * K + j] = col;
    }
    int s = 0;
#pragma nounroll
    for (int bit = 0; bit <= MFX_DEPTH_ORACLE; ++bit) {
        if (!((modes >> bit) & 1u)) continue;
        const int mode = bit == MFX_DEPTH_ORACLE ? oracle_mode : bit;
        const bdec::Combined z = bdec::combine(sh.e, mode, has_du, has_cu);
        const bdec::Row row = bdec::finish_row(sh, px, py, cls, score, cam, dc, z);
        const size_t o = (((size_t)b * NM + s) * K + j);
        for (int i = 0; i < 14; ++i) det[o * 14 + i] = row.det[i];
        if (unc) {                                            // [estimated_depth_error, uncertainty_conf]
            unc[o * 2 + 0] = row.as_conf ? row.sigma : 0.f;
            unc[o * 2 + 1] = row.as_conf ? row.conf : 0.f;
        }
        ++s;
    }
}

}  // namespace mfx
using namespace mfx;

extern "C" int mfx_decode_boxes_multi(const float* hmap, int ld, int reg_off, const float* scores, const int32_t* index,
                                      int ncls, int B, int H, int W, int K, const float* calib, const int32_t* pad,
                                      const int32_t* img_size, float threshold, const mfx_decode_cfg* cfg, const mfx_head_layout* heads,
                                      uint32_t modes, const float* gt_rows, int M, float* det, float* topk, int32_t* valid, float* unc,
                                      int32_t* oracle_choice, void* stream) {
    if (!cfg) return mfx_fail(MFX_ERR_ARG, "decode_boxes_multi: null cfg");
    if (!heads) return mfx_fail(MFX_ERR_ARG, "decode_boxes_multi: null heads");
    if (!hmap || !scores || !index || !calib || !pad || !img_size || !det || !topk || !valid)
        return mfx_fail(MFX_ERR_ARG, "decode_boxes_multi: null pointer");
    mfx_decode_cfg c = *cfg;
    c.output_depth = MFX_DEPTH_SOFT;                          // (not read: the modes come as bits)
    if (const char* e = bdec::decode_cfg_error(c)) return mfx_fail_in(MFX_ERR_ARG, "decode_boxes_multi", e);
    if (ncls < 1 || ncls > 3) return mfx_fail(MFX_ERR_ARG, "decode_boxes_multi: need 1 <= ncls <= 3 (rows of dim_mean / dim_std)");
    if (K < 1 || K > 256) return mfx_fail(MFX_ERR_ARG, "decode_boxes_multi: need 1 <= K <= 256");
    if (const char* e = bdec::head_layout_error(heads->ch, heads->reg_width)) return mfx_fail_in(MFX_ERR_ARG, "decode_boxes_multi", e);
    if (modes == 0) return mfx_fail(MFX_ERR_ARG, "decode_boxes_multi: modes is 0 (no depth mode requested)");
    if (modes >> (MFX_DEPTH_ORACLE + 1)) return mfx_fail(MFX_ERR_ARG, "decode_boxes_multi: modes has bits above 8 (bit m = MFX_DEPTH_* value m, bit 8 = oracle)");
    int NM = 0;
    for (int m = 0; m < MFX_DEPTH_ORACLE; ++m) {
        if (!((modes >> m) & 1u)) continue;
        ++NM;
        if (const char* e = bdec::output_depth_error(m, *heads)) return mfx_fail_in(MFX_ERR_ARG, "decode_boxes_multi", e);
    }
    if (modes & kOracleBit) {
        ++NM;
        if (heads->ch[bdec::HK_KPT] < 0 || heads->ch[bdec::HK_KPT_UNC] < 0)
            return mfx_fail(MFX_ERR_ARG, "decode_boxes_multi: output_depth oracle needs corner_offset and corner_uncertainty");
        if (!gt_rows) return mfx_fail(MFX_ERR_ARG, "decode_boxes_multi: the oracle bit needs gt_rows (the ground-truth table of every image)");
        if (M < 1 || M > dorc::MAX_GT) return mfx_fail(MFX_ERR_ARG, "decode_boxes_multi: the oracle bit needs 1 <= M <= 128 ground-truth slots per image (one table in LDS)");
    }
    const int R = heads->reg_width;
    if (B < 0 || H < 1 || W < 1 || ld < R || reg_off < 0 || reg_off + R > ld)
        return mfx_fail(MFX_ERR_ARG, "decode_boxes_multi: need B >= 0, H, W >= 1 and the regression channels inside a row (reg_off + reg_width <= ld)");
    if (B == 0) return MFX_OK;
    const size_t smem = (size_t)ncls * K * 8 + (size_t)K * 4;
    hipLaunchKernelGGL(decode_boxes_multi_kernel, dim3(B), dim3(kMultiThreads), smem, reinterpret_cast<hipStream_t>(stream),
                       hmap, ld, reg_off, scores, index, ncls, H, W, K, calib, pad, img_size, threshold, c, *heads, modes, NM,
                       (modes & kOracleBit) ? gt_rows : nullptr, M, det, topk, valid, unc, oracle_choice);
    MFX_HIP_CHECK(hipGetLastError());
    ++g_cnt_decode_multi;
    return MFX_OK;
}
