// The conv chain of the edge fusion (detector_predictor.py:111-119,152-158) as ONE kernel: at the border points of the feature map, per fusion
// branch (class, 3d_offset)
//   trunk   3x3 64 -> 256 + folded ABN + LeakyReLU(0.01) (or BN + ReLU: mfx_edge_chain_act)                    (rounded to the activation type)
//   Conv1d  k = KS (1, 3, 5, 7; 3 in runs/monoflex.yaml) along the point sequence, replicate padded, 256 -> 256 + folded BN1d, or the bias alone
//           where EDGE_FUSION_NORM is not 'BN' (scale = 1, shift = bias) (+ ReLU)                 (rounded to the activation type)
//   1x1     256 -> c (<= 4) + bias                                                            (fp32)
// which mfx_conv2d_nhwc runs as five launches (row-map trunk for both branches, then two convs per branch) with the two intermediates in memory.
//
// A workgroup owns (a segment of SEG = 64 - 2 HALO consecutive sequence positions, HALO = KS / 2, a branch, an image): its 64 tile rows are the
// positions seg * SEG - HALO .. seg * SEG + SEG + HALO - 1, clamped to 0 .. L - 1 (the clamp IS the replicate padding; for L <= HALO several taps
// read the same position) -- the first and the last HALO are the Conv1d's halo, recomputed and never written (KS = 3: SEG = 62).  Four waves, each 64
// rows x 64 channels of the trunk and of the Conv1d (16 accumulator fragments), then one 16-row fragment of the 1x1.  The gathered 3x3 input (64 rows x 9 taps x
// 128 bytes) and the two intermediates live in LDS; the weights stream L2 -> registers through a ring of DEPTH k-steps, fragment-major
// (packing.fragment_major), so a fragment is one contiguous KiB and a lane's 16 bytes are its MFMA operand.
//
// Arithmetic is that of the five launches, operation for operation: the same v_mfma_f32_16x16x32 per 32 elements of K in ascending K, the same
// acc * scale + shift, activation and rounding at the same three places -- the results are bit-identical to them (tests/test_gpu_edge_chain.py).
#include "../../include/monoflex_hip.h"
#include "err.h"
#include "common.h"

namespace mfx {

namespace ec {
constexpr int ROWS = 64;                      // tile rows (the positions written + the halo rows)
constexpr int CIN = 64, HC = 256;             // feature channels, trunk / Conv1d channels
constexpr int NK1 = 9 * CIN / 32, NK3 = HC / 32;      // k-steps (32 elements of K) of the trunk and of the 1x1: 18, 8
constexpr int G_ROW = 9 * CIN * 2 + 16;       // bytes of a gathered row (+ one chunk: 16 rows on 16 distinct 16-byte bank slots; 73 slots per row)
constexpr int T_ROW = HC * 2 + 16;            // bytes of a trunk / Conv1d row (33 slots per row)
constexpr int G_BYTES = ROWS * G_ROW;         // 74752: the gathered input; the Conv1d output (ROWS * T_ROW) takes its place afterwards
constexpr int XY_BYTES = ROWS * 8;
constexpr int DEPTH = 6;                      // k-steps of weights in flight per wave (6 x 4 KiB)
static_assert(ROWS * T_ROW <= G_BYTES, "the Conv1d output reuses the gathered input's space");

// what follows from the Conv1d's window KS (1, 3, 5, 7)
template <int KS> struct Win {
    static_assert(KS == 1 || KS == 3 || KS == 5 || KS == 7, "odd windows up to 7");
    static constexpr int HALO = KS / 2;
    static constexpr int SEG = ROWS - 2 * HALO;            // positions written per workgroup: 64, 62, 60, 58
    static constexpr int NK2 = KS * HC / 32;               // k-steps of the Conv1d: 8, 24, 40, 56
    // trunk rows: KS - 1 more than the tile, never written (Conv1d tile rows SEG .. 63 read them, nothing keeps their sums): 34848 B at KS = 3
    static constexpr int T_BYTES = (ROWS + KS - 1) * T_ROW;
    static constexpr int SMEM = G_BYTES + T_BYTES + XY_BYTES;      // 109056, 110112, 111168, 112224
    static_assert((ROWS - 1) + (NK2 - 1) / 8 < T_BYTES / T_ROW, "the last Conv1d tile row's last k-step reads inside the trunk tile");
    static_assert(SEG + 2 * HALO == ROWS && SEG > 0, "a segment and its two halos fill the tile");
    static_assert(T_BYTES % 16 == 0 && SMEM <= 160 * 1024, "the LDS of one CU (one workgroup per CU, as at KS = 3)");
};
static_assert(Win<3>::SEG == 62 && Win<3>::NK2 == 24 && Win<3>::SMEM == 110112, "runs/monoflex.yaml's window: the kernel it has always been");
static_assert(Win<7>::SMEM == 74752 + 70 * 528 + 512, "the largest window");
}  // namespace ec

struct EdgeChainArgs {
    const void* x; const int* edge_xy;
    const void* w_trunk; const float* scale_trunk; const float* shift_trunk;
    const void* w_conv; const float* scale_conv; const float* shift_conv;
    const void* w_out; const float* bias_out;
    float* out;
    int B, H, W, L, relu;
};

// the wave's four weight fragments (output channels 16 (nf0 + j) ..) of k-step ks: `wl` points at this lane's chunk of fragment (nf0, 0)
template <int NK> __device__ __forceinline__ void ring_load(u32x4 (&slot)[4], const u32x4* wl, int ks) {
#pragma unroll
    for (int j = 0; j < 4; ++j) slot[j] = wl[(j * NK + ks) * 64];
}

template <int NK> __device__ __forceinline__ void ring_fill(u32x4 (&ring)[ec::DEPTH][4], const u32x4* wl) {
#pragma unroll
    for (int s = 0; s < ec::DEPTH; ++s)
        if (s < NK) ring_load<NK>(ring[s], wl, s);
}

// acc[i][j] += A (64 tile rows, from LDS: the lane's chunk of row fragment 0 at k-step ks is a_addr(ks), fragment i is 16 rows of ROWB bytes further)
//              x the ring's weights, K ascending; `ring` arrives filled with k-steps 0 .. DEPTH - 1
template <typename T, int NK, int ROWB, typename AF>
__device__ __forceinline__ void chain_gemm(f32x4 (&acc)[4][4], u32x4 (&ring)[ec::DEPTH][4], const u32x4* wl, AF a_addr) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
        u32x4 a[4], b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = ring[ks % ec::DEPTH][j];
        if (ks + ec::DEPTH < NK) ring_load<NK>(ring[ks % ec::DEPTH], wl, ks + ec::DEPTH);
        const char* ap = a_addr(ks);
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const u32x4*>(ap + i * 16 * ROWB);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) mma_chunk<T>(a[i], b[j], acc[i][j]);
    }
}

// act(acc * scale + shift), rounded to T, to rows of T_ROW bytes at `dst`: D layout col = lane & 15, row = (lane >> 4) * 4 + r
template <typename T, int ACT>
__device__ __forceinline__ void chain_epilogue(const f32x4 (&acc)[4][4], char* dst, const float* scale, const float* shift, int n0, int lane) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + j * 16 + (lane & 15);
        const float sc = scale[n], sh = shift[n];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = i * 16 + (lane >> 4) * 4;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = acc[i][j][r] * sc + sh;
                if (ACT == ACT_RELU) v = fmaxf(v, 0.f);
                if (ACT == ACT_LEAKY) v = v > 0.f ? v : 0.01f * v;
                // the fp32 value exists before it is rounded, as in the five launches (whose epilogue passes it through LDS): without this the compiler
                // folds the multiply-add and the conversion to half into v_fma_mixlo_f16, ONE rounding instead of two -- another result on ties
                asm volatile("" : "+v"(v));
                ElemTraits<T>::store(reinterpret_cast<T*>(dst + (m + r) * ec::T_ROW) + n, v);
            }
        }
    }
}

// TACT: the trunk's activation (ACT_LEAKY: InPlaceABN; ACT_RELU: BatchNorm2d + ReLU), the expressions of mfx_conv2d_nhwc's epilogue
template <typename T, int TACT, int KS>
__global__ __launch_bounds__(256) void edge_chain_kernel(EdgeChainArgs a) {
    using namespace ec;
    constexpr int HALO = Win<KS>::HALO, SEG = Win<KS>::SEG, NK2 = Win<KS>::NK2, T_BYTES = Win<KS>::T_BYTES;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Gs = smem;                          // gathered input, then the Conv1d output
    char* Ts = smem + G_BYTES;                // trunk
    int* xy = reinterpret_cast<int*>(smem + G_BYTES + T_BYTES);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int seg = blockIdx.x, br = blockIdx.y, b = blockIdx.z;
    const int p0 = seg * SEG;                 // first position written; tile row r is position p0 - HALO + r

    // weights of the trunk first: they are in flight while the rows are gathered
    u32x4 ring[DEPTH][4];
    const u32x4* w1 = reinterpret_cast<const u32x4*>(a.w_trunk) + (size_t)(br * 16 + wave * 4) * NK1 * 64 + lane;
    ring_fill<NK1>(ring, w1);

    if (tid < ROWS) {
        const int p = min(max(p0 - HALO + tid, 0), a.L - 1);
        const int* e = a.edge_xy + ((size_t)b * a.L + p) * 2;
        xy[2 * tid] = min(max(e[0], 0), a.W - 1);
        xy[2 * tid + 1] = min(max(e[1], 0), a.H - 1);
    }
    __syncthreads();
    {
        // 64 rows x 9 taps x 8 chunks of 16 bytes, 18 per thread, all in flight together; taps outside the image are zeros
        const char* xb = reinterpret_cast<const char*>(a.x) + (size_t)b * a.H * a.W * (CIN * 2);
        constexpr int PER = ROWS * 72 / 256;
        u32x4 g[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int idx = tid + 256 * i, row = idx / 72, rem = idx - row * 72, tap = rem >> 3, c = rem & 7;
            const int th = tap / 3, tw = tap - th * 3;
            const int ih = xy[2 * row + 1] + th - 1, iw = xy[2 * row] + tw - 1;
            const bool ok = ih >= 0 && ih < a.H && iw >= 0 && iw < a.W;
            const int ihc = min(max(ih, 0), a.H - 1), iwc = min(max(iw, 0), a.W - 1);
            const u32x4 z = *reinterpret_cast<const u32x4*>(xb + ((size_t)ihc * a.W + iwc) * (CIN * 2) + c * 16);
            g[i] = ok ? z : u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int idx = tid + 256 * i, row = idx / 72, rem = idx - row * 72;
            *reinterpret_cast<u32x4*>(Gs + row * G_ROW + rem * 16) = g[i];
        }
    }
    __syncthreads();

    const int frag = (lane & 15), kq16 = (lane >> 4) * 16;
    f32x4 acc[4][4];
    // ---- trunk: [64 rows][576] x [256][576]^T
    chain_gemm<T, NK1, G_ROW>(acc, ring, w1, [&](int ks) { return Gs + frag * G_ROW + ks * 64 + kq16; });
    const u32x4* w2 = reinterpret_cast<const u32x4*>(a.w_conv) + (size_t)(br * 16 + wave * 4) * NK2 * 64 + lane;
    ring_fill<NK2>(ring, w2);                 // (the Conv1d's first weights travel under the epilogue)
    chain_epilogue<T, TACT>(acc, Ts, a.scale_trunk + br * HC, a.shift_trunk + br * HC, wave * 64, lane);
    __syncthreads();                          // trunk complete; every wave is done with the gathered input

    // ---- Conv1d: tile row i = position p0 + i, taps = trunk rows i .. i + KS - 1; K = (tap, channel)
    chain_gemm<T, NK2, T_ROW>(acc, ring, w2, [&](int ks) { return Ts + (frag + (ks >> 3)) * T_ROW + (ks & 7) * 64 + kq16; });
    if (a.relu) chain_epilogue<T, ACT_RELU>(acc, Gs, a.scale_conv + br * HC, a.shift_conv + br * HC, wave * 64, lane);
    else chain_epilogue<T, ACT_NONE>(acc, Gs, a.scale_conv + br * HC, a.shift_conv + br * HC, wave * 64, lane);
    __syncthreads();

    // ---- 1x1: wave w = rows 16 w .. 16 w + 15, one fragment of 16 output channels (4 real)
    const u32x4* w3 = reinterpret_cast<const u32x4*>(a.w_out) + (size_t)br * NK3 * 64 + lane;
    u32x4 b3[NK3];
#pragma unroll
    for (int ks = 0; ks < NK3; ++ks) b3[ks] = w3[ks * 64];
    f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < NK3; ++ks)
        mma_chunk<T>(*reinterpret_cast<const u32x4*>(Gs + (wave * 16 + frag) * T_ROW + ks * 64 + kq16), b3[ks], o);
    const int n = lane & 15;
    if (n < 4) {
        const float bias = a.bias_out[br * 16 + n];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = wave * 16 + (lane >> 4) * 4 + r, p = p0 + i;
            if (i < SEG && p < a.L) a.out[(((size_t)br * a.B + b) * a.L + p) * 4 + n] = o[r] + bias;
        }
    }
}

static bool edge_chain_supported(const mfx_edge_chain_desc* d) {
    return (d->dtype == MFX_BF16 || d->dtype == MFX_F16) && d->C == ec::CIN && d->head_conv == ec::HC && d->ksize == 3;
}

static bool edge_chain_window_served(int ksize) { return ksize == 1 || ksize == 3 || ksize == 5 || ksize == 7; }

template <typename T, int TACT, int KS = 3> static int launch_edge_chain(const EdgeChainArgs& a, hipStream_t st) {
    using W = ec::Win<KS>;
    auto k = edge_chain_kernel<T, TACT, KS>;
    static bool attr_set = false;
    if (!attr_set) {
        MFX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, W::SMEM));
        attr_set = true;
    }
    const int nseg = (a.L + W::SEG - 1) / W::SEG;
    hipLaunchKernelGGL(k, dim3(nseg, 2, a.B), dim3(256), W::SMEM, st, a);
    MFX_HIP_CHECK(hipGetLastError());
    return MFX_OK;
}

}  // namespace mfx
using namespace mfx;

extern "C" int mfx_edge_chain_applies(const mfx_edge_chain_desc* d) { return (d && g_opt_edge_chain != 0 && edge_chain_supported(d)) ? 1 : 0; }

extern "C" int mfx_edge_chain(const mfx_edge_chain_desc* d, void* stream) { return mfx_edge_chain_act(d, MFX_ACT_LEAKY, stream); }

// the argument checks every entry makes before any device work, then the descriptor as kernel arguments; `window_ok`: the entry's own rule for ksize
static int edge_chain_check(const mfx_edge_chain_desc* d, int act, bool window_ok, const char* window_msg, EdgeChainArgs& a) {
    if (!d || !d->x || !d->edge_xy || !d->w_trunk || !d->scale_trunk || !d->shift_trunk || !d->w_conv || !d->scale_conv || !d->shift_conv ||
        !d->w_out || !d->bias_out || !d->out)
        return mfx_fail(MFX_ERR_ARG, "edge_chain: null pointer");
    if (d->dtype != MFX_BF16 && d->dtype != MFX_F16) return mfx_fail(MFX_ERR_UNSUPPORTED, "edge_chain: bf16 or fp16 activations only");
    if (!window_ok || d->C != ec::CIN || d->head_conv != ec::HC) return mfx_fail(MFX_ERR_UNSUPPORTED, window_msg);
    if (act != MFX_ACT_LEAKY && act != MFX_ACT_RELU) return mfx_fail(MFX_ERR_UNSUPPORTED, "edge_chain: the trunk activation is MFX_ACT_LEAKY or MFX_ACT_RELU");
    if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->L < 0) return mfx_fail(MFX_ERR_ARG, "edge_chain: bad B / H / W / L");
    if (d->B > 65535) return mfx_fail(MFX_ERR_UNSUPPORTED, "edge_chain: more than 65535 images");
    a.x = d->x; a.edge_xy = d->edge_xy;
    a.w_trunk = d->w_trunk; a.scale_trunk = d->scale_trunk; a.shift_trunk = d->shift_trunk;
    a.w_conv = d->w_conv; a.scale_conv = d->scale_conv; a.shift_conv = d->shift_conv;
    a.w_out = d->w_out; a.bias_out = d->bias_out; a.out = d->out;
    a.B = d->B; a.H = d->H; a.W = d->W; a.L = d->L; a.relu = d->relu ? 1 : 0;
    return MFX_OK;
}

template <int KS> static int launch_edge_chain_ks(const EdgeChainArgs& a, int dtype, int act, hipStream_t st) {
    if (act == MFX_ACT_RELU) return dtype == MFX_BF16 ? launch_edge_chain<bf16_t, ACT_RELU, KS>(a, st) : launch_edge_chain<half_t, ACT_RELU, KS>(a, st);
    return dtype == MFX_BF16 ? launch_edge_chain<bf16_t, ACT_LEAKY, KS>(a, st) : launch_edge_chain<half_t, ACT_LEAKY, KS>(a, st);
}

extern "C" int mfx_edge_chain_act(const mfx_edge_chain_desc* d, int act, void* stream) {
    EdgeChainArgs a;
    const int rc = edge_chain_check(d, act, d && d->ksize == 3, "edge_chain: built for 64 feature channels, 256 head channels and a k = 3 Conv1d", a);
    if (rc != MFX_OK || d->L == 0) return rc;
    ++g_cnt_edge_chain;
    return launch_edge_chain_ks<3>(a, d->dtype, act, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int mfx_edge_chain_ks_applies(const mfx_edge_chain_desc* d) {
    return (d && g_opt_edge_chain != 0 && (d->dtype == MFX_BF16 || d->dtype == MFX_F16) && d->C == ec::CIN && d->head_conv == ec::HC &&
            edge_chain_window_served(d->ksize)) ? 1 : 0;
}

extern "C" int mfx_edge_chain_ks(const mfx_edge_chain_desc* d, int act, void* stream) {
    EdgeChainArgs a;
    const int rc = edge_chain_check(d, act, d && edge_chain_window_served(d->ksize),
                                    "edge_chain_ks: built for 64 feature channels, 256 head channels and a Conv1d of k = 1, 3, 5 or 7 (odd, at most 7)", a);
    if (rc != MFX_OK || d->L == 0) return rc;
    ++g_cnt_edge_chain;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    switch (d->ksize) {
        case 1: return launch_edge_chain_ks<1>(a, d->dtype, act, st);
        case 3: return launch_edge_chain_ks<3>(a, d->dtype, act, st);      // the instantiation mfx_edge_chain_act launches
        case 5: return launch_edge_chain_ks<5>(a, d->dtype, act, st);
        default: return launch_edge_chain_ks<7>(a, d->dtype, act, st);
    }
}
