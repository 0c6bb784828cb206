// Test-only host shim: everything monoflex_amd/csrc/dcn_sample_math.h returns for arrays of (output pixel, tap, offset pair), compiled by
// tests/test_dcn_sample_math_cpu.py with g++ -ffp-contract=off.
#include "../../monoflex_amd/csrc/dcn_sample_math.h"

using namespace mfx::dcns;

// geom = {H, W, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w}; form: 0 = tap3x3 + pos3x3 + sample<>, otherwise tap_of(tap, kw) + pos +
// the wide clamp.  Per sample: fl[10] = h, w, lh, lw, hh, hw, weight[4]; in[18] = th, tw, inside, h0, w0, valid[4],
// clamped (row, column) of the four corners, pre = 1 if sample_inside agrees with sample (evaluated only when inside); cw[8] = ch[4], cw[4].
extern "C" void shim_dcn_sample(const int* geom, int form, int n, const int* oh, const int* ow, const int* tap, const float* dh, const float* dw,
                                float* fl, int* in, float* cw) {
    const int H = geom[0], W = geom[1], kw = geom[2];
    for (int i = 0; i < n; ++i) {
        const Tap t = form == 0 ? tap3x3(tap[i]) : tap_of(tap[i], kw);
        const float h = form == 0 ? pos3x3(oh[i], t.th, dh[i]) : pos(oh[i], geom[3], geom[5], t.th, geom[7], dh[i]);
        const float w = form == 0 ? pos3x3(ow[i], t.tw, dw[i]) : pos(ow[i], geom[4], geom[6], t.tw, geom[8], dw[i]);
        const bool ins = inside(h, w, H, W);
        const Sample s = form == 0 ? sample(h, w) : sample<kClampLo, kClampHiWide>(h, w);
        float* f = fl + 10 * i;
        int* o = in + 18 * i;
        f[0] = h; f[1] = w; f[2] = s.lh; f[3] = s.lw; f[4] = s.hh; f[5] = s.hw;
        o[0] = t.th; o[1] = t.tw; o[2] = ins; o[3] = s.h0; o[4] = s.w0;
        for (int q = 0; q < 4; ++q) {
            f[6 + q] = corner_weight(s, q);
            o[5 + q] = corner_valid(s, ins, q, H, W);
            o[9 + 2 * q] = clamp_idx(corner_h(s, q), H);
            o[10 + 2 * q] = clamp_idx(corner_w(s, q), W);
        }
        o[17] = 1;
        if (ins) {
            const Sample u = sample_inside(h, w);
            o[17] = u.h0 == s.h0 && u.w0 == s.w0 && u.lh == s.lh && u.lw == s.lw && u.hh == s.hh && u.hw == s.hw;
            for (int q = 0; q < 4; ++q) o[17] &= in_map(corner_h(s, q), corner_w(s, q), H, W) == (o[5 + q] != 0);
        }
        const CoordWeights c = coord_weights(s);
        for (int q = 0; q < 4; ++q) { cw[8 * i + q] = c.ch[q]; cw[8 * i + 4 + q] = c.cw[q]; }
    }
}

extern "C" void shim_dcn_sample_consts(int* out) {
    out[0] = kRow; out[1] = kMaskBase; out[2] = off_h(5); out[3] = off_w(5); out[4] = mask_at(5); out[5] = kClampLo; out[6] = kClampHi; out[7] = kClampHiWide;
}
