// TEST-ONLY host build of monoflex_amd/csrc/object_loss_math.h for the reduced head sets (cfg.ch[i] == -1, cfg.reg_width < 50): the
// wavefront-per-object kernel as plain loops (object, lane) over a row of `ld` floats of which only [ch_off, ch_off + reg_width) belong
// to the regression head, and the entry points' argument check (head_set_error).  Not loaded by the product.
#include <algorithm>
#include <cstddef>
#include <cstring>

#include "../../monoflex_amd/csrc/object_loss_math.h"

using namespace mfx::oloss;

namespace {
// every read of a regression channel goes through here: `touched` records which channels of the row the arithmetic looked at
struct TrackingReader {
    const float* p; int seed; unsigned char* touched;
    Dual operator()(int ch) const {
        if (ch < 0 || ch >= 64) { touched[64] = 1; return Dual{0.f, 0.f}; }       // a read outside the row: flagged, not performed
        touched[ch] = 1;
        return Dual{p[ch], ch == seed ? 1.f : 0.f};
    }
};
const float* object_pixel(const float* base, const float* t, int B, int H, int W, int ld, int ch_off) {
    const int b = std::min(std::max((int)t[R_B], 0), B - 1), cx = std::min(std::max((int)t[R_CX], 0), W - 1), cy = std::min(std::max((int)t[R_CY], 0), H - 1);
    return base + ((size_t)(b * H + cy) * W + cx) * ld + ch_off;
}
}  // namespace

// 0 when the cfg is one mfx_object_loss accepts, 1 otherwise; `why` (>= 160 bytes) receives the message
extern "C" int shim_head_set_error(const mfx_object_loss_cfg* cfg, char* why) {
    const char* e = head_set_error(*cfg);
    if (why) { why[0] = 0; if (e) std::strncpy(why, e, 159), why[159] = 0; }
    return e ? 1 : 0;
}

// touched[65]: OR over all objects and lanes of the channels (relative to ch_off) that object_terms read; [64]: a read outside 0..63
extern "C" int shim_object_loss_heads(const float* reg, int B, int H, int W, int ld, int ch_off, const float* rows, int N,
                                      const mfx_object_loss_cfg* cfg, float* vals, float* G, unsigned char* touched) {
    if (head_set_error(*cfg) || ch_off < 0 || ch_off + reg_width(*cfg) > ld) return 1;
    float cn[NNORM] = {0};
    for (int r = 0; r < N; ++r) {
        float q[NNORM];
        row_counts(rows + (size_t)r * ROW, q);
        for (int i = 0; i < NNORM; ++i) cn[i] += q[i];
    }
    for (int k = 0; k < NVAL; ++k) vals[k] = 0.f;
    for (int i = 0; i < 65; ++i) touched[i] = 0;
    for (int n = 0; n < N; ++n) {
        const float* t = rows + (size_t)n * ROW;
        for (int lane = 0; lane < 64; ++lane) {
            Dual out[NVAL];
            const TrackingReader X{object_pixel(reg, t, B, H, W, ld, ch_off), lane, touched};
            object_terms(X, t, *cfg, cn, out);
            for (int k = 0; k < NTERM; ++k) G[((size_t)n * NTERM + k) * 64 + lane] = out[k].d;
            if (lane == 0 && t[R_VALID] != 0.f)
                for (int k = 0; k < NVAL; ++k) vals[k] += out[k].v;
        }
    }
    return 0;
}
