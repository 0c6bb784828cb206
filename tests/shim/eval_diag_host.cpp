// TEST-ONLY host build of monoflex_amd/csrc/eval_diag_math.h: the one-lane-per-object kernel of eval_diag.hip as a plain loop over the
// (image, slot) pairs with the entry point's configuration check, so the CPU suite can pin the float32 arithmetic without a GPU.
// Not loaded by the product.
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../monoflex_amd/csrc/eval_diag_math.h"

using namespace mfx::ediag;

// 0 on success, 1 when (cfg, heads, want) or the row geometry is refused; `why` (>= 160 bytes) receives the message
extern "C" int shim_eval_diagnostics(const float* hmap, int ld, int reg_off, const float* gt_rows, int B, int M, int H, int W,
                                     const float* calib, const int32_t* pad, const mfx_decode_cfg* cfg, const mfx_head_layout* heads,
                                     int want, float* depth_err, float* iou, float* boxes, char* why) {
    const char* e = config_error(*cfg, *heads, want);
    if (!e && (reg_off < 0 || reg_off + heads->reg_width > ld)) e = "eval_diagnostics: the regression channels reach outside a row";
    if (why) { why[0] = 0; if (e) std::strncpy(why, e, 159), why[159] = 0; }
    if (e) return 1;
    for (int n = 0; n < B * M; ++n) {
        const int b = n / M;
        eval_object(hmap + (size_t)b * H * W * ld + reg_off, ld, H, W, gt_rows + (size_t)n * GT_ROW, calib + b * 6, (float)pad[b * 2],
                    (float)pad[b * 2 + 1], *cfg, *heads, want, (want & 1) ? depth_err + (size_t)n * NDEPTH : nullptr,
                    (want & 2) ? iou + (size_t)n * NIOU : nullptr, boxes ? boxes + (size_t)n * NBOX * 7 : nullptr);
    }
    return 0;
}
