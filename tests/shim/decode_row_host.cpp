// TEST-ONLY host build of monoflex_amd/csrc/box_decode_math.h: decode.hip's decode_boxes_kernel as a plain loop over (image, rank) with the
// checks of mfx_decode_boxes_heads that need no device buffer, so the CPU suite can pin the float32 arithmetic without a GPU.
// Not loaded by the product.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>

#include "../../monoflex_amd/csrc/box_decode_math.h"

using namespace mfx::bdec;

// 0 on success, 1 when the arguments are refused; `why` (>= 160 bytes) receives the message.  unc may be null.
extern "C" int shim_decode_boxes(const float* hmap, int ld, int reg_off, const float* scores, const int32_t* index, int ncls, int B, int H, int W,
                                 int K, const float* calib, const int32_t* pad, const int32_t* img_size, float threshold,
                                 const mfx_decode_cfg* cfg, const mfx_head_layout* heads, float* det, float* topk, int32_t* valid, float* unc,
                                 char* why) {
    const char* e = !cfg ? "null cfg" : !heads ? "null heads" : decode_cfg_error(*cfg);
    if (!e && (ncls < 1 || ncls > 3)) e = "need 1 <= ncls <= 3 (rows of dim_mean / dim_std)";
    if (!e && (K < 1 || K > 256)) e = "need 1 <= K <= 256";
    if (!e) e = head_layout_error(heads->ch, heads->reg_width);
    if (!e) e = output_depth_error(cfg->output_depth, *heads);
    if (!e && (B < 0 || H < 1 || W < 1 || ld < heads->reg_width || reg_off < 0 || reg_off + heads->reg_width > ld))
        e = "need B >= 0, H, W >= 1 and the regression channels inside a row (reg_off + reg_width <= ld)";
    if (why) { why[0] = 0; if (e) std::strncpy(why, e, 159), why[159] = 0; }
    if (e) return 1;
    const int n = ncls * K;
    std::vector<int> order(n);
    for (int b = 0; b < B; ++b) {
        // select_topk stage 2: the K best of the concatenated list, value descending, ties to the lower position
        const float* cs = scores + (size_t)b * n;
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int p, int q) { return cs[p] > cs[q]; });
        const Camera cam = {calib[b * 6 + 0], calib[b * 6 + 1], calib[b * 6 + 2], calib[b * 6 + 3], calib[b * 6 + 4], calib[b * 6 + 5],
                            (float)pad[b * 2], (float)pad[b * 2 + 1]};
        for (int j = 0; j < K; ++j) {
            const int pos = order[j], cls = pos / K, idx = index[(size_t)b * n + pos];
            const int ys = idx / W, xs = idx - ys * W;
            const float score = cs[pos], px = (float)xs, py = (float)ys;
            const float* r = hmap + ((size_t)b * H * W + idx) * ld + reg_off;
            const Row row = decode_row(r, px, py, cls, score, cam, (float)(img_size[0] - 1), (float)(img_size[1] - 1), *cfg, *heads);
            const size_t o = (size_t)b * K + j;
            for (int i = 0; i < 14; ++i) det[o * 14 + i] = row.det[i];
            const float t[5] = {score, (float)idx, (float)cls, py, px};
            for (int i = 0; i < 5; ++i) topk[o * 5 + i] = t[i];
            valid[o] = score >= threshold ? 1 : 0;
            if (unc) { unc[o * 2] = row.as_conf ? row.sigma : 0.f; unc[o * 2 + 1] = row.as_conf ? row.conf : 0.f; }
        }
    }
    return 0;
}
