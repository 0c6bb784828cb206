// Functions one translation unit of libmonoflex_hip.so defines for another: the one declaration of each, grouped by owning file.
// Both the owner and the callers include this header, so the compiler checks the definition against what the callers see.
// (wgrad.h declares wgrad_tr.hip's two entry points next to the geometry struct they take.)
#pragma once
#include "../../include/monoflex_hip.h"
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace mfx {

// conv_halo.hip, 3x3 LDS-staged halo kernels: 1 if handled, 0 to fall through to the implicit-GEMM kernel, < 0 on error;
// *stats_ran = 1 if the launch that ran accumulated d->stats
int try_conv_halo(const mfx_conv_desc* d, hipStream_t st, int* stats_ran);

// conv_cw.hip / conv_cws.hip (the latter: split precision), `v` = conv_halo.hip's variant number: 0 = ran, 1 = no instantiation, < 0 = error
int try_conv_cw(const mfx_conv_desc* d, int v, hipStream_t st);
int try_conv_cws(const mfx_conv_desc* d, int v, hipStream_t st);

// dcn_wave.hip: 1 if handled, 0 to fall back to the first-generation kernel, < 0 on error
int try_dcn_wave(const mfx_dcn_desc* d, hipStream_t st);

// dcn_patch.hip / dcn_lds.hip: 1 if handled, 0 to fall through to the older kernels, < 0 on error;
// *_fuses_offset_conv: the kernel would compute the offset/mask conv of this layer itself (the same test the launch makes)
int try_dcn_patch(const mfx_dcn_desc* d, hipStream_t st);
bool dcn_patch_fuses_offset_conv(const mfx_dcn_desc* d);
int try_dcn_lds(const mfx_dcn_desc* d, hipStream_t st);
bool dcn_lds_fuses_offset_conv(const mfx_dcn_desc* d);

// "would try_dcn_* take this layer?" without launching (the test each of them makes first; dcn_lds: the 16-bit modes only):
// mfx_dcn_module_group leaves such layers to mfx_dcn_nhwc
bool dcn_wave_takes(const mfx_dcn_desc* d);
bool dcn_patch_takes(const mfx_dcn_desc* d);
bool dcn_lds_takes_16bit(const mfx_dcn_desc* d);

// Grouped launches (mfx_dcn_module_group, conv_kernels.hip): n <= kGroupMax layers of identical geometry and dtype in one grid.
// conv_halo.hip: the grouped form of the fp32-out 3x3 kernel for the n offset/mask convs d[0..n), each with the variant try_conv_halo picks
// for it alone: 0 = ran, 1 = not applicable (nothing launched; the caller launches conv by conv), < 0 = error.  conv_cw.hip owns the kernel.
constexpr int kGroupMax = 4;
int try_conv_halo_group(const mfx_conv_desc* d, int n, hipStream_t st);
int try_conv_cw_group(const mfx_conv_desc* d, int n, int v, hipStream_t st);

}  // namespace mfx

// dcn_ext.hip: dst[b][cd0 + c][p] (+)= src[b][cs0 + c][p], c < Cg: a channel slice of an NCHW fp32 tensor (accumulate != 0: adds)
int mfx_internal_ext_slice(const float* src, float* dst, int B, int Cs, int cs0, int Cd, int cd0, int Cg, int HW, int accumulate, void* stream);

// dcn_bwd.hip: workspace of one deformable group of the `_ext` backward
extern "C" size_t mfx_dcn_v2_backward_workspace_bytes_(int B, int C, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw);

// dcn_bwd_tile.hip: the fp32 second-generation backward with d_raw's mask channels as the gradient of the MASK itself (the `_ext` boundary)
int mfx_internal_dcn_backward_v2_f32_rawmask(const float* x, const float* offmask, const float* weight_oihw, const float* dy, float* dx, float* d_raw,
                                             float* dweight, float* dbias, int B, int C, int H, int W, int Cout, void* workspace, size_t workspace_bytes, void* stream);

// train_kernels.hip: weight gradient with a dense [M][K] A operand (direct = 1), written as (Cout, Cin, kh, kw): the DCN weight gradient
// is a weight gradient over the dense columns matrix
int mfx_internal_conv_wgrad(const void* x, const void* dy, float* dw, int B, int H, int W, int x_pixstride, int Ck,
                            int kh, int kw, int stride, int pad_h, int pad_w, int Ho, int Wo, int Cout, int ldy,
                            int dtype, int oihw, int Cin_out, int Cout_out, void* stream, int dil_w,
                            void* workspace, size_t workspace_bytes, int direct);
// train_kernels.hip: sum `nslab` partial gradient blocks ws[slab][Cout][K] (k = tap*Ck + c) into dW (Cout, Ck, kh, kw)
int mfx_internal_wgrad_slab_sum(const float* ws, int nslab, int Cout, int Ck, int kh, int kw, float* dw_oihw, void* stream);
// train_kernels.hip: column sums ADDED into `out`, which an earlier kernel of the caller has zeroed
int mfx_internal_colsum_add(const void* x, float* out, long M, int C, int ld, int dtype, void* stream);

// split-precision range sentinel: the per-translation-unit flags of common.h's lds_operand<f32s_t> (MFX_RANGE_FLAG_ACCESSOR in each
// unit; capi.hip ORs them): the flag, or < 0 if reading it failed; reset != 0 clears it
int mfx_range_flag_conv_halo(int reset), mfx_range_flag_conv_kernels(int reset), mfx_range_flag_dcn_wave(int reset), mfx_range_flag_f1_fused(int reset),
    mfx_range_flag_heads(int reset), mfx_range_flag_stem(int reset), mfx_range_flag_dcn_lds(int reset), mfx_range_flag_conv_cws(int reset);
