// 3x3 / stride-1 / pad-1 convolution on 16-bit maps, second form of the LDS-halo kernel (conv_halo.hip): the SAME decomposition
// (8 x 16-pixel tile, halo patch staged once in LDS, wave-private output slices, fragment-major weights L2 -> registers, K-split
// waves, wave-private epilogue) with every piece of geometry a COMPILE-TIME constant and the K loop written as an explicit
// software pipeline.
//
// Why (round 5, ISA of conv3x3_wave_kernel<bf16, bf16, 2, 2, 1>, `hipcc --save-temps`): with the channel group, patch width and
// weight row length as run-time values, one K step of that kernel is 16 MFMAs inside ~60 other instructions -- per step three
// v_mul_lo_u32 and a dozen VALU to rebuild the lane's patch address from (tap, channel), two exec-masked branch diamonds around the
// weight fetch (null-pointer / K-padding tests), 64-bit VALU address arithmetic per weight load -- and two scheduling accidents
// that follow from the control flow: `s_waitcnt vmcnt(0)` at the top of EVERY step (the branches hide the load count from the
// waitcnt pass, so the five-deep weight ring drains to empty each step and every step exposes one full L2 round trip) and
// `s_waitcnt lgkmcnt(1)` in front of every MFMA pair (pixel fragments are read one pair = 34 cycles ahead of their use against an
// LDS round trip of 64-128).  The kernel was instruction-issue- and latency-bound by its own address code, not by a hardware unit
// (profiles/r03_conv_halo_probes.md: no unit above 25 % busy).
//
// Here <CG, CT, WN, FN, WK> are template parameters, so
//   * a pixel-fragment read is `ds_read_b128 v, v_lane offset:imm` -- the lane's patch base is computed once per workgroup;
//   * a weight-fragment fetch is `global_load_dwordx4 v, v_lane16, s[base] offset:imm` against a wave-uniform base advanced by SALU;
//   * the K loop is fully unrolled and branch-free (the waitcnt pass counts exactly: vmcnt(2 FN) / lgkmcnt(4) waits);
//   * pixel fragments are read HALF A STEP (8 FN MFMAs = 136+ cycles) ahead of their use into two 4-row register sets, weights two
//     steps ahead through a 3-deep ring; `sched_barrier`s pin that order;
//   * BN scale / shift are fetched before the K loop instead of at the head of the epilogue.
// Same K order, same accumulation order, same epilogue arithmetic as conv3x3_wave_kernel: outputs are bit-identical
// (tests/test_gpu_ops.py::test_conv_cw_kernel_is_bit_identical_to_the_halo_kernel).
//
// Reference layers: model/backbone/dla_dcn.py:84-98 (BasicBlock conv1 / conv2 of levels 2-5), 246-259 (Tree).
#include "../../include/monoflex_hip.h"
#include "err.h"
#include "internal.h"
#include "igemm.h"
#include <type_traits>

namespace mfx {

struct CwGeom { int B, H, W, Ho, Wo, tiles_x, tiles_y, tiles_n; };      // H x W: input map, Ho x Wo: output map (= H x W at stride 1)

constexpr int kCwRows = 8;

// patch of an 8 x 16 output tile at stride S: (7 S + 3) x (15 S + 3) input pixels (10 x 18, or 17 x 33 at stride 2)
template <int CG, int WN, int FN, int WK, int S = 1, int ROWS = kCwRows> struct CwSmem {
    static constexpr int PS = CG * 2 + 16;                                    // patch pixel stride: 16 consecutive pixels on 16 distinct 16-byte bank slots
    static constexpr int PH = (ROWS - 1) * S + 3, PW = 15 * S + 3;
    static constexpr int patch_bytes = PH * PW * PS;
    static constexpr int stage_ld = FN * 16 + 4;
    static constexpr int stage_bytes = 16 * stage_ld * 4;
    static constexpr int reduce_bytes = WN * (WK - 1) * ROWS * FN * 64 * 16;
    static constexpr int main_bytes = patch_bytes > reduce_bytes ? patch_bytes : reduce_bytes;
    static constexpr int total = main_bytes + WN * WK * stage_bytes;
};

// CG = channels per patch pass, CT = input channels of the layer (a multiple of CG), WN x FN x 16 = output channels per workgroup,
// WK = waves sharing an output slice (they take the K steps round-robin); OCC = waves per SIMD the register allocation must admit
// ROWS = output rows of a tile (8; 6 for maps whose height is a multiple of 6 but not of 8 -- the 12 x 40 level-5 maps: 2 x 3 tiles of 6 x 16 instead of
// 2 x 3 tiles of 8 x 16, a quarter less matrix work)
// ST: train-mode BN statistics of the stored values accumulated by the epilogue (mfx_conv_desc.stats; conv_halo.hip's arithmetic)
template <typename T, typename TO, int CG, int CT, int WN, int FN, int WK, int OCC, int S = 1, int ROWS = kCwRows, bool ST = false>
__global__ __launch_bounds__(WN * WK * 64, OCC) void conv3x3_cw_kernel(const T* __restrict__ x, const u32x4* __restrict__ wfm, CwGeom g, EpiArgs ep) {
#define CW_TILE_ID xcd_remap(blockIdx.x, gridDim.x)
#include "conv_cw_body.h"
#undef CW_TILE_ID
}

// Grouped form (mfx_dcn_module_group: the offset/mask convs of DCN modules that read different maps of one shape): workgroups [i * tiles_per,
// (i + 1) * tiles_per) are layer i's grid, in the order the one-layer launch gives them (xcd_remap inside the layer; where tiles_per is no
// multiple of 8 a layer's contiguous tile ranges no longer fall on one XCD each -- speed only).  The per-layer pointers come from the by-value
// table with a workgroup-uniform index (scalar loads from the kernel arguments); geometry and every other epilogue field are the group's.
struct CwGroupPtrs {
    const void* x[kGroupMax]; const u32x4* wfm[kGroupMax]; const float* scale[kGroupMax]; const float* shift[kGroupMax]; void* y[kGroupMax];
    int tiles_per;
};
template <typename T, typename TO, int CG, int CT, int WN, int FN, int WK, int OCC>
__global__ __launch_bounds__(WN * WK * 64, OCC) void conv3x3_cw_group_kernel(CwGroupPtrs gp, CwGeom g, EpiArgs ep) {
    constexpr int S = 1, ROWS = kCwRows;
    constexpr bool ST = false;
    const int layer = blockIdx.x / gp.tiles_per, local = blockIdx.x - layer * gp.tiles_per;
    const T* __restrict__ x = reinterpret_cast<const T*>(gp.x[layer]);
    const u32x4* __restrict__ wfm = gp.wfm[layer];
    ep.scale = gp.scale[layer]; ep.shift = gp.shift[layer]; ep.y = gp.y[layer];
#define CW_TILE_ID xcd_remap(local, gp.tiles_per)
#include "conv_cw_body.h"
#undef CW_TILE_ID
}

template <typename T, typename TO, int CG, int CT, int WN, int FN, int WK, int OCC, int S = 1, int ROWS = kCwRows, bool ST = false>
static int launch_cw(const mfx_conv_desc* d, hipStream_t st) {
    using SM = CwSmem<CG, WN, FN, WK, S, ROWS>;
    constexpr int BN = WN * FN * 16;
    CwGeom g;
    g.B = d->B; g.H = d->H; g.W = d->W; g.Ho = d->Ho; g.Wo = d->Wo;
    g.tiles_x = (d->Wo + 15) / 16; g.tiles_y = (d->Ho + ROWS - 1) / ROWS; g.tiles_n = d->Cout_pad / BN;
    EpiArgs ep;
    ep.scale = d->scale; ep.shift = d->shift; ep.res = d->res; ep.y = d->y; ep.ldy = d->ldy; ep.ldres = d->ldres;
    ep.Cout = d->Cout; ep.act = d->act; ep.K_pad = d->K_pad; ep.nk = 0; ep.tiles_n = g.tiles_n;
    ep.stats = ST ? d->stats : nullptr; ep.stats_ncopy = d->stats_ncopy > 0 ? d->stats_ncopy : 1;
    auto k = conv3x3_cw_kernel<T, TO, CG, CT, WN, FN, WK, OCC, S, ROWS, ST>;
    constexpr int smem = SM::total;
    static bool attr_done = false;
    if (!attr_done && smem > 64 * 1024) {
        MFX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, smem));
        attr_done = true;
    }
    const int tiles = g.tiles_n * g.tiles_x * g.tiles_y * d->B;
    hipLaunchKernelGGL(k, dim3(tiles), dim3(WN * WK * 64), smem, st, reinterpret_cast<const T*>(d->x), reinterpret_cast<const u32x4*>(d->w_frag), g, ep);
    MFX_HIP_CHECK(hipGetLastError());
    return MFX_OK;
}

static inline bool cw_rows6(const mfx_conv_desc* d) { return g_opt_cw_rows6 && d->Ho % 6 == 0 && d->Ho % 8 != 0 && d->Ho <= 48; }

template <typename T, int OCC> static int cw_shape(const mfx_conv_desc* d, int v, hipStream_t st) {
    const int C = d->Ck;
    if (d->stats) {                                           // training forward: statistics epilogue (outputs up to 128 channels wide)
        if (v == 6 && C == 64) return launch_cw<T, T, 64, 64, 2, 2, 1, OCC, 1, kCwRows, true>(d, st);
        if (v == 7 && C == 128) return launch_cw<T, T, 128, 128, 4, 2, 1, OCC, 1, kCwRows, true>(d, st);
        return 1;
    }
    // 32 input channels: the data gradients of the DCN modules' 27-channel offset / mask convs (training)
    if (v == 6 && C == 32) return launch_cw<T, T, 32, 32, 2, 2, 1, OCC>(d, st);
    if ((v == 7 || v == 11) && C == 32) return launch_cw<T, T, 32, 32, 4, 2, 1, OCC>(d, st);
    if (v == 12 && C == 128) return launch_cw<T, T, 128, 128, 2, 2, 2, OCC>(d, st);
    if (v == 13 && C == 256) return launch_cw<T, T, 256, 256, 2, 2, 4, OCC>(d, st);
    if (v == 5 && C == 64) return launch_cw<T, T, 64, 64, 4, 4, 1, OCC>(d, st);
    if (v == 6 && C == 64) return launch_cw<T, T, 64, 64, 2, 2, 1, OCC>(d, st);
    if (v == 7 && C == 128) return launch_cw<T, T, 128, 128, 4, 2, 1, OCC>(d, st);
    if (v == 7 && C == 64) return launch_cw<T, T, 64, 64, 4, 2, 1, OCC>(d, st);
    if (v == 11 && C == 256) return launch_cw<T, T, 256, 256, 4, 2, 2, OCC>(d, st);
    if (v == 11 && C == 512) return cw_rows6(d) ? launch_cw<T, T, 256, 512, 4, 2, 2, OCC, 1, 6>(d, st) : launch_cw<T, T, 256, 512, 4, 2, 2, OCC>(d, st);
    return 1;                                                 // no instantiation: the caller falls back
}

// the four stride-2 convs that open DLA levels 2-5 (dla_dcn.py:84-98 conv1 of the first BasicBlock): 17 x 33 patches; 32-channel groups keep a
// patch at 45 KB where no wave splits K, the K-split variant needs two steps per tap (64-channel groups, 81 KB: one workgroup per CU)
template <typename T> static int cw_shape_s2(const mfx_conv_desc* d, int v, hipStream_t st) {
    const int C = d->Ck;
    if (d->stats) {
        if (v == 6 && C == 32) return launch_cw<T, T, 32, 32, 2, 2, 1, 2, 2, kCwRows, true>(d, st);
        if (v == 7 && C == 64) return launch_cw<T, T, 32, 64, 4, 2, 1, 2, 2, kCwRows, true>(d, st);
        return 1;
    }
    if (v == 6 && C == 32) return launch_cw<T, T, 32, 32, 2, 2, 1, 2, 2>(d, st);
    if (v == 7 && C == 64) return launch_cw<T, T, 32, 64, 4, 2, 1, 2, 2>(d, st);
    if (v == 11 && C == 128) return launch_cw<T, T, 64, 128, 4, 2, 2, 2, 2>(d, st);
    if (v == 11 && C == 256) return cw_rows6(d) ? launch_cw<T, T, 64, 256, 4, 2, 2, 2, 2, 6>(d, st) : launch_cw<T, T, 64, 256, 4, 2, 2, 2, 2>(d, st);
    return 1;
}

// the 27-channel DCN offset / mask convs of the wide layers (fp32 out, sigmoid on the mask channels, N = 32): one output slice per workgroup,
// four waves share it and split K (conv_halo.hip's variants 8 = 32 channels per workgroup, 10 = 16)
template <typename T> static int cw_shape_f32out(const mfx_conv_desc* d, int v, hipStream_t st) {
    const int C = d->Ck;
    if (v == 8 && C == 128) return launch_cw<T, float, 128, 128, 1, 2, 4, 2>(d, st);
    if (v == 8 && C == 256) return launch_cw<T, float, 256, 256, 1, 2, 4, 2>(d, st);
    if (v == 8 && C == 512) return launch_cw<T, float, 256, 512, 1, 2, 4, 2>(d, st);      // (8 rows x 4-way K split: 6 rows do not divide)
    if (v == 10 && C == 128) return launch_cw<T, float, 128, 128, 1, 1, 4, 2>(d, st);
    if (v == 10 && C == 256) return launch_cw<T, float, 256, 256, 1, 1, 4, 2>(d, st);
    if (v == 10 && C == 512) return launch_cw<T, float, 256, 512, 1, 1, 4, 2>(d, st);
    return 1;
}

// returns MFX_OK (0) if this kernel ran, 1 if there is no instantiation for the shape / variant (caller runs conv3x3_wave_kernel), < 0 on error.
// `v` is conv_halo.hip's variant number (6: 2 waves x 32 channels, 7: 4 x 32, 11: 4 x 32 with a 2-way K split; 8 / 10: one slice, 4-way K split)
int try_conv_cw(const mfx_conv_desc* d, int v, hipStream_t st) {
    if (!g_opt_halo_cw || !d->w_frag || (d->stride != 1 && d->stride != 2)) return 1;
    if (d->stats && (d->out_dtype != d->dtype || d->Cout_pad > 128)) return 1;
    if (d->dtype != MFX_BF16 && d->dtype != MFX_F16) return 1;
    if (d->K_pad != (9 * d->Ck + 63) / 64 * 64) return 1;
    if ((long long)d->M * (d->ldy > d->ldres ? d->ldy : d->ldres) >= (1ll << 31) || (long long)d->H * d->W * d->Ck >= (1ll << 31)) return 1;      // 32-bit element offsets
    if (d->out_dtype == MFX_F32) {
        if (d->stride != 1 || d->res || d->Cout % 4 != 0 || d->Cout_pad != 32 || (v != 8 && v != 10)) return 1;
        return d->dtype == MFX_F16 ? cw_shape_f32out<half_t>(d, v, st) : cw_shape_f32out<bf16_t>(d, v, st);
    }
    if (d->out_dtype != d->dtype || d->Cout % 8 != 0 || d->act == MFX_ACT_DCN_OFFMASK) return 1;
    if ((v == 6 || v == 12 || v == 13) && d->Cout_pad % 64 != 0) return 1;
    if ((v == 7 || v == 11) && d->Cout_pad % 128 != 0) return 1;
    if (v == 5 && d->Cout_pad % 256 != 0) return 1;
    if (d->stride == 2) return d->dtype == MFX_F16 ? cw_shape_s2<half_t>(d, v, st) : cw_shape_s2<bf16_t>(d, v, st);
    if (d->dtype == MFX_F16) return cw_shape<half_t, 2>(d, v, st);
    return cw_shape<bf16_t, 2>(d, v, st);
}

template <typename T, int CG, int CT, int FN> static int launch_cw_group(const mfx_conv_desc* d, int n, hipStream_t st) {
    using SM = CwSmem<CG, 1, FN, 4>;
    const mfx_conv_desc& d0 = d[0];
    CwGeom g;
    g.B = d0.B; g.H = d0.H; g.W = d0.W; g.Ho = d0.Ho; g.Wo = d0.Wo;
    g.tiles_x = (d0.Wo + 15) / 16; g.tiles_y = (d0.Ho + kCwRows - 1) / kCwRows; g.tiles_n = d0.Cout_pad / (FN * 16);
    EpiArgs ep;
    ep.scale = nullptr; ep.shift = nullptr; ep.res = nullptr; ep.y = nullptr; ep.ldy = d0.ldy; ep.ldres = 0;
    ep.Cout = d0.Cout; ep.act = d0.act; ep.K_pad = d0.K_pad; ep.nk = 0; ep.tiles_n = g.tiles_n;
    ep.stats = nullptr; ep.stats_ncopy = 1;
    CwGroupPtrs gp;
    gp.tiles_per = g.tiles_n * g.tiles_x * g.tiles_y * d0.B;
    for (int i = 0; i < kGroupMax; ++i) {                     // unused slots repeat layer 0 (never indexed: the grid has n * tiles_per workgroups)
        const mfx_conv_desc& di = d[i < n ? i : 0];
        gp.x[i] = di.x; gp.wfm[i] = reinterpret_cast<const u32x4*>(di.w_frag); gp.scale[i] = di.scale; gp.shift[i] = di.shift; gp.y[i] = di.y;
    }
    auto k = conv3x3_cw_group_kernel<T, float, CG, CT, 1, FN, 4, 2>;
    constexpr int smem = SM::total;
    static bool attr_done = false;
    if (!attr_done && smem > 64 * 1024) {
        MFX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, smem));
        attr_done = true;
    }
    hipLaunchKernelGGL(k, dim3(gp.tiles_per * n), dim3(256), smem, st, gp, g, ep);
    MFX_HIP_CHECK(hipGetLastError());
    return MFX_OK;
}

// The grouped launch of n fp32-out offset/mask convs (cw_shape_f32out's 128- and 256-channel instantiations; `v` = the variant every one of them
// takes alone).  The layers differ in their pointers only: x, w_frag, scale, shift, y.  0 = ran, 1 = not applicable, < 0 = error.
int try_conv_cw_group(const mfx_conv_desc* d, int n, int v, hipStream_t st) {
    if (n < 1 || n > kGroupMax || (v != 8 && v != 10)) return 1;
    const mfx_conv_desc& d0 = d[0];
    for (int i = 0; i < n; ++i) {
        const mfx_conv_desc& e = d[i];
        if (!g_opt_halo_cw || !e.x || !e.y || !e.w_frag || e.stride != 1 || e.stats || e.res || e.rowmap) return 1;
        if ((e.dtype != MFX_BF16 && e.dtype != MFX_F16) || e.out_dtype != MFX_F32) return 1;
        if (e.K_pad != (9 * e.Ck + 63) / 64 * 64 || e.Cout % 4 != 0 || e.Cout_pad != 32) return 1;
        if ((long long)e.M * e.ldy >= (1ll << 31) || (long long)e.H * e.W * e.Ck >= (1ll << 31)) return 1;      // 32-bit element offsets
        if (e.dtype != d0.dtype || e.B != d0.B || e.H != d0.H || e.W != d0.W || e.Ho != d0.Ho || e.Wo != d0.Wo || e.Ck != d0.Ck || e.M != d0.M ||
            e.Cout != d0.Cout || e.K_pad != d0.K_pad || e.ldy != d0.ldy || e.act != d0.act) return 1;
    }
    if ((long long)n * d0.B * ((d0.Ho + kCwRows - 1) / kCwRows) * ((d0.Wo + 15) / 16) * 2 >= (1ll << 31)) return 1;
    const int C = d0.Ck;
    if (C != 128 && C != 256) return 1;                      // (512 -> 27 occurs once per network: nothing to group)
    if (d0.dtype == MFX_F16) {
        if (v == 8) return C == 128 ? launch_cw_group<half_t, 128, 128, 2>(d, n, st) : launch_cw_group<half_t, 256, 256, 2>(d, n, st);
        return C == 128 ? launch_cw_group<half_t, 128, 128, 1>(d, n, st) : launch_cw_group<half_t, 256, 256, 1>(d, n, st);
    }
    if (v == 8) return C == 128 ? launch_cw_group<bf16_t, 128, 128, 2>(d, n, st) : launch_cw_group<bf16_t, 256, 256, 2>(d, n, st);
    return C == 128 ? launch_cw_group<bf16_t, 128, 128, 1>(d, n, st) : launch_cw_group<bf16_t, 256, 256, 1>(d, n, st);
}

}  // namespace mfx
