// Deformable position-sensitive ROI pooling: the other half of the reference's `_ext` boundary
// (src/dcn_v2.h:94-190, kernels src/cuda/dcn_v2_psroi_pooling_cuda.cu:59-146 / :149-269), NCHW fp32.
//
// One workgroup owns one (roi, class).  The sample geometry of a bin -- S*S positions, their corner index, corner steps and
// bilinear distances, validity -- is the same for every channel of the class, so the workgroup computes it ONCE into LDS
// (psroi_math.h, one sample per thread) and then runs the channels over it:
//   forward   one thread per (channel, bin), bins on neighbouring lanes: reads of one channel plane, coalesced stores;
//   backward  G lanes per bin (G = power of two <= 64 covering the class's channels), each lane walks its channels and the bin's
//             samples: grad_input is scattered with float atomics (runs of samples that share their four corners are summed in
//             registers first), the two offset-gradient sums are reduced over the G lanes by wave shuffles, then over the bins of
//             each offset cell in bin order by ONE thread that owns the cell: no atomic touches grad_offset, so it is
//             run-to-run bitwise repeatable.  grad_input is order-dependent in its last bits.
// Bins are taken in chunks of at most MAX_SAMPLES / (S*S), so any pooled size fits; S*S itself must fit (S <= 32).
#include "../../include/monoflex_hip.h"
#include "err.h"
#include "fill.h"
#include "psroi_math.h"
#include <cstdio>

namespace mfx {
namespace psroi {

constexpr int THREADS = 256;
constexpr int MAX_SAMPLES = 1024;          // samples of one chunk of bins held in LDS (12 KiB)

struct PoolDims {
    int B, C, H, W, N, P, part, S, num_classes, cpc, no_trans, bins_per_chunk;
    float scale, trans_std;
};

// key of a kept sample: ((y0 * W + x0) << 2) | (x1 - x0) << 1 | (y1 - y0); -1 = dropped.  Samples with equal keys share all four corners.
// LDS layout [sample][bin of the chunk]: neighbouring bins on neighbouring banks.
__device__ __forceinline__ void fill_geometry(const PoolDims& d, const Roi<float>& r, const float* __restrict__ trans, int n, int cls, int bin0, int nb,
                                              int* s_key, float* s_dx, float* s_dy) {
    const int S2 = d.S * d.S;
    for (int i = threadIdx.x; i < nb * S2; i += THREADS) {
        const int bl = i % nb, s = i / nb;
        const int b = bin0 + bl, ph = b / d.P, pw = b % d.P;
        float tx = 0.f, ty = 0.f;
        if (!d.no_trans) {
            const int part_h = part_index<float>(ph, d.P, d.part), part_w = part_index<float>(pw, d.P, d.part);
            const size_t cell = ((((size_t)n * d.num_classes + cls) * 2) * d.part + part_h) * d.part + part_w;
            tx = trans[cell] * d.trans_std;
            ty = trans[cell + (size_t)d.part * d.part] * d.trans_std;
        }
        float wstart, hstart, w, h;
        bin_origin(r, ph, pw, tx, ty, wstart, hstart);
        sample_position(r, wstart, hstart, s / d.S, s % d.S, w, h);
        const Sample<float> g = sample_geometry(w, h, d.W, d.H);
        s_key[i] = g.valid ? (((g.y0 * d.W + g.x0) << 2) | ((g.x1 - g.x0) << 1) | (g.y1 - g.y0)) : -1;
        s_dx[i] = g.dx;
        s_dy[i] = g.dy;
    }
}

__global__ __launch_bounds__(THREADS) void psroi_forward_kernel(const float* __restrict__ input, const float* __restrict__ rois, const float* __restrict__ trans,
                                                                float* __restrict__ output, float* __restrict__ output_count, PoolDims d) {
    __shared__ int s_key[MAX_SAMPLES];
    __shared__ float s_dx[MAX_SAMPLES], s_dy[MAX_SAMPLES];
    const int n = blockIdx.x / d.num_classes, cls = blockIdx.x % d.num_classes;
    const int PP = d.P * d.P, S2 = d.S * d.S;
    const Roi<float> r = roi_geometry(rois + (size_t)n * 5, d.scale, d.P, d.S);
    float* out = output + ((size_t)n * d.C + (size_t)cls * d.cpc) * PP;
    float* cnt = output_count + ((size_t)n * d.C + (size_t)cls * d.cpc) * PP;
    if (r.batch < 0 || r.batch >= d.B) {                       // the reference reads out of bounds here; this build: output 0, count 0
        for (int i = threadIdx.x; i < d.cpc * PP; i += THREADS) { out[i] = 0.f; cnt[i] = 0.f; }
        return;
    }
    const float* planes = input + ((size_t)r.batch * d.C + (size_t)cls * d.cpc) * d.H * d.W;
    for (int bin0 = 0; bin0 < PP; bin0 += d.bins_per_chunk) {
        const int nb = min(d.bins_per_chunk, PP - bin0);
        __syncthreads();
        fill_geometry(d, r, trans, n, cls, bin0, nb, s_key, s_dx, s_dy);
        __syncthreads();
        for (int item = threadIdx.x; item < nb * d.cpc; item += THREADS) {
            const int bl = item % nb, c = item / nb;
            const float* plane = planes + (size_t)c * d.H * d.W;
            float sum = 0.f;
            int count = 0;
            for (int s = 0; s < S2; ++s) {                      // sample order (ih, iw), as the reference sums
                const int key = s_key[s * nb + bl];
                if (key < 0) continue;
                const int o = key >> 2, sx = (key >> 1) & 1, sy = (key & 1) * d.W;
                sum += interpolate(plane[o], plane[o + sy], plane[o + sx], plane[o + sy + sx], s_dx[s * nb + bl], s_dy[s * nb + bl]);
                ++count;
            }
            out[(size_t)c * PP + bin0 + bl] = count == 0 ? 0.f : sum / (float)count;
            cnt[(size_t)c * PP + bin0 + bl] = (float)count;
        }
    }
}

__global__ __launch_bounds__(THREADS) void psroi_backward_kernel(const float* __restrict__ grad_out, const float* __restrict__ input, const float* __restrict__ rois,
                                                                 const float* __restrict__ trans, const float* __restrict__ top_count,
                                                                 float* __restrict__ grad_input, float* __restrict__ grad_trans, PoolDims d, int G) {
    __shared__ int s_key[MAX_SAMPLES];
    __shared__ float s_dx[MAX_SAMPLES], s_dy[MAX_SAMPLES];
    __shared__ float s_bin[2 * MAX_SAMPLES];                   // per bin of the chunk: its offset-gradient sums over the class's channels (x, y)
    const int n = blockIdx.x / d.num_classes, cls = blockIdx.x % d.num_classes;
    const int PP = d.P * d.P, S2 = d.S * d.S;
    const Roi<float> r = roi_geometry(rois + (size_t)n * 5, d.scale, d.P, d.S);
    if (r.batch < 0 || r.batch >= d.B) return;                 // no gradient from a ROI of no image
    const size_t class_base = ((size_t)n * d.C + (size_t)cls * d.cpc) * PP;
    const size_t plane_base = ((size_t)r.batch * d.C + (size_t)cls * d.cpc) * d.H * d.W;
    for (int bin0 = 0; bin0 < PP; bin0 += d.bins_per_chunk) {
        const int nb = min(d.bins_per_chunk, PP - bin0);
        __syncthreads();
        fill_geometry(d, r, trans, n, cls, bin0, nb, s_key, s_dx, s_dy);
        __syncthreads();
        const int nitems = nb * G;
        for (int base = 0; base < nitems; base += THREADS) {   // uniform trip count: every lane of a wave reaches the shuffles
            const int item = base + threadIdx.x;
            const bool active = item < nitems;
            const int bl = item / G, g = item % G;
            float off_x = 0.f, off_y = 0.f;
            if (active) {
                for (int c = g; c < d.cpc; c += G) {
                    const size_t oi = class_base + (size_t)c * PP + bin0 + bl;
                    const float count = top_count[oi];
                    if (count <= 0.f) continue;
                    const float diff_val = grad_out[oi] / count;
                    const float* plane = input + plane_base + (size_t)c * d.H * d.W;
                    float* gplane = grad_input + plane_base + (size_t)c * d.H * d.W;
                    int cur = -1;
                    float a00 = 0.f, a01 = 0.f, a10 = 0.f, a11 = 0.f;
                    for (int s = 0; s <= S2; ++s) {
                        const int key = s < S2 ? s_key[s * nb + bl] : -1;
                        if (key < 0 && s < S2) continue;
                        if (key != cur) {                       // flush the run of samples that shared their four corners
                            if (cur >= 0) {
                                const int o = cur >> 2, sx = (cur >> 1) & 1, sy = (cur & 1) * d.W;
                                atomicAdd(gplane + o, a00);
                                atomicAdd(gplane + o + sy, a01);
                                atomicAdd(gplane + o + sx, a10);
                                atomicAdd(gplane + o + sy + sx, a11);
                            }
                            cur = key;
                            a00 = a01 = a10 = a11 = 0.f;
                        }
                        if (s == S2) break;
                        const float dx = s_dx[s * nb + bl], dy = s_dy[s * nb + bl];
                        float q00, q01, q10, q11;
                        corner_weights(dx, dy, q00, q01, q10, q11);
                        a00 += q00 * diff_val;
                        a01 += q01 * diff_val;
                        a10 += q10 * diff_val;
                        a11 += q11 * diff_val;
                        if (!d.no_trans) {
                            const int o = key >> 2, sx = (key >> 1) & 1, sy = (key & 1) * d.W;
                            const float u00 = plane[o], u01 = plane[o + sy], u10 = plane[o + sx], u11 = plane[o + sy + sx];
                            off_x += offset_grad_x(u00, u01, u10, u11, dy, d.trans_std, diff_val, r.width);
                            off_y += offset_grad_y(u00, u01, u10, u11, dx, d.trans_std, diff_val, r.height);
                        }
                    }
                }
            }
            if (!d.no_trans) {
                for (int m = G >> 1; m > 0; m >>= 1) {          // fixed-order sum over the G lanes of the bin
                    off_x += __shfl_xor(off_x, m, 64);
                    off_y += __shfl_xor(off_y, m, 64);
                }
                if (active && g == 0) { s_bin[2 * bl] = off_x; s_bin[2 * bl + 1] = off_y; }
            }
        }
        if (!d.no_trans) {
            __syncthreads();
            float* gt = grad_trans + (((size_t)n * d.num_classes + cls) * 2) * d.part * d.part;
            for (int cell = threadIdx.x; cell < d.part * d.part; cell += THREADS) {      // one owner per cell, bins in order
                const int cell_h = cell / d.part, cell_w = cell % d.part;
                float ax = 0.f, ay = 0.f;
                bool any = false;
                for (int bl = 0; bl < nb; ++bl) {
                    const int b = bin0 + bl;
                    if (part_index<float>(b / d.P, d.P, d.part) != cell_h || part_index<float>(b % d.P, d.P, d.part) != cell_w) continue;
                    ax += s_bin[2 * bl];
                    ay += s_bin[2 * bl + 1];
                    any = true;
                }
                if (any) {                                     // (zero-filled before the launch; later chunks add to what this thread wrote)
                    gt[cell] += ax;
                    gt[cell + d.part * d.part] += ay;
                }
            }
        }
    }
}

static int check_dims(const char* who, int B, int C, int H, int W, int N, int trans_channels, int no_trans, int output_dim, int group_size, int pooled_size,
                      int part_size, int sample_per_part, PoolDims* d) {
    static thread_local char msg[256];
    if (B < 0 || C < 0 || H < 0 || W < 0 || N < 0) { snprintf(msg, sizeof msg, "%s: negative size", who); return mfx_fail(MFX_ERR_ARG, msg); }
    if (C != output_dim) {                                     // :295 / :371
        snprintf(msg, sizeof msg, "%s: input channels and output channels must equal (got %d and output_dim %d)", who, C, output_dim);
        return mfx_fail(MFX_ERR_ARG, msg);
    }
    if (group_size != 1) {
        snprintf(msg, sizeof msg, "%s: group_size must be 1 (got %d): the reference requires channels == output_dim, so its channel index "
                 "(ctop * group_size + gh) * group_size + gw runs past the input for any other value", who, group_size);
        return mfx_fail(MFX_ERR_UNSUPPORTED, msg);
    }
    if (pooled_size < 1 || part_size < 1 || sample_per_part < 1) { snprintf(msg, sizeof msg, "%s: pooled_size, part_size and sample_per_part must be positive", who); return mfx_fail(MFX_ERR_ARG, msg); }
    if (sample_per_part * sample_per_part > MAX_SAMPLES) { snprintf(msg, sizeof msg, "%s: sample_per_part must be at most 32 (a bin's samples are held on chip)", who); return mfx_fail(MFX_ERR_UNSUPPORTED, msg); }
    if (pooled_size > 1024 || part_size > 1024) { snprintf(msg, sizeof msg, "%s: pooled_size and part_size must be at most 1024", who); return mfx_fail(MFX_ERR_UNSUPPORTED, msg); }
    if ((long)H * W >= (1L << 29)) { snprintf(msg, sizeof msg, "%s: maps of 2^29 pixels or more are not supported", who); return mfx_fail(MFX_ERR_UNSUPPORTED, msg); }
    const int num_classes = no_trans ? 1 : trans_channels / 2;     // :303-304
    if (!no_trans && (trans_channels < 2 || trans_channels % 2 != 0 || output_dim % num_classes != 0)) {
        snprintf(msg, sizeof msg, "%s: offset channels must be 2 * num_classes with num_classes dividing output_dim (got %d channels, output_dim %d)", who, trans_channels, output_dim);
        return mfx_fail(MFX_ERR_ARG, msg);
    }
    d->B = B; d->C = C; d->H = H; d->W = W; d->N = N; d->P = pooled_size; d->part = part_size; d->S = sample_per_part;
    d->num_classes = num_classes; d->cpc = output_dim / num_classes; d->no_trans = no_trans ? 1 : 0;
    d->bins_per_chunk = MAX_SAMPLES / (sample_per_part * sample_per_part);
    if (d->bins_per_chunk > pooled_size * pooled_size) d->bins_per_chunk = pooled_size * pooled_size;
    if ((long)N * num_classes > 0x7fffffffL) { snprintf(msg, sizeof msg, "%s: too many ROIs", who); return mfx_fail(MFX_ERR_UNSUPPORTED, msg); }
    return MFX_OK;
}

}  // namespace psroi
}  // namespace mfx
using namespace mfx::psroi;

extern "C" int mfx_dcn_v2_psroi_pooling_forward(const float* input, const float* bbox, const float* trans, float* output, float* output_count,
                                                int B, int C, int H, int W, int N, int trans_rois, int trans_channels,
                                                int no_trans, float spatial_scale, int output_dim, int group_size, int pooled_size, int part_size,
                                                int sample_per_part, float trans_std, void* stream) {
    PoolDims d;
    int rc = check_dims("dcn_v2_psroi_pooling_forward", B, C, H, W, N, trans_channels, no_trans, output_dim, group_size, pooled_size, part_size, sample_per_part, &d);
    if (rc) return rc;
    if (!no_trans && trans_rois < N) return mfx_fail(MFX_ERR_ARG, "dcn_v2_psroi_pooling_forward: fewer offset rows than ROIs");
    if (N == 0 || output_dim == 0) return MFX_OK;              // empty output: nothing to launch (:308-312)
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t out_bytes = (size_t)N * output_dim * pooled_size * pooled_size * sizeof(float);
    if (!output || !output_count) return mfx_fail(MFX_ERR_ARG, "dcn_v2_psroi_pooling_forward: null output");
    if (B == 0 || H == 0 || W == 0) {                          // no image to read: every ROI's batch index is out of range
        MFX_HIP_CHECK(mfx::zero_async(output, out_bytes, st));
        MFX_HIP_CHECK(mfx::zero_async(output_count, out_bytes, st));
        return MFX_OK;
    }
    if (!input || !bbox || (!no_trans && !trans)) return mfx_fail(MFX_ERR_ARG, "dcn_v2_psroi_pooling_forward: null pointer");
    d.scale = spatial_scale; d.trans_std = trans_std;
    hipLaunchKernelGGL(psroi_forward_kernel, dim3((unsigned)(N * d.num_classes)), dim3(THREADS), 0, st, input, bbox, trans, output, output_count, d);
    MFX_HIP_CHECK(hipGetLastError());
    return MFX_OK;
}

extern "C" int mfx_dcn_v2_psroi_pooling_backward(const float* out_grad, const float* input, const float* bbox, const float* trans, const float* top_count,
                                                 float* grad_input, float* grad_trans,
                                                 int B, int C, int H, int W, int N, int trans_rois, int trans_channels,
                                                 int no_trans, float spatial_scale, int output_dim, int group_size, int pooled_size, int part_size,
                                                 int sample_per_part, float trans_std, void* stream) {
    PoolDims d;
    int rc = check_dims("dcn_v2_psroi_pooling_backward", B, C, H, W, N, trans_channels, no_trans, output_dim, group_size, pooled_size, part_size, sample_per_part, &d);
    if (rc) return rc;
    if (!no_trans && trans_rois < N) return mfx_fail(MFX_ERR_ARG, "dcn_v2_psroi_pooling_backward: fewer offset rows than ROIs");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t in_bytes = (size_t)B * C * H * W * sizeof(float);
    const size_t trans_bytes = no_trans ? 0 : (size_t)trans_rois * trans_channels * part_size * part_size * sizeof(float);
    if ((in_bytes && !grad_input) || (trans_bytes && !grad_trans)) return mfx_fail(MFX_ERR_ARG, "dcn_v2_psroi_pooling_backward: null gradient buffer");
    // both gradients are sums: zero fill first, as a kernel on the same stream (fill.h: a memset NODE of a captured graph is not reliably ordered here)
    MFX_HIP_CHECK(mfx::zero_async(grad_input, in_bytes, st));
    MFX_HIP_CHECK(mfx::zero_async(grad_trans, trans_bytes, st));
    if (N == 0 || in_bytes == 0) return MFX_OK;                // :381-385
    if (!out_grad || !input || !bbox || !top_count || (!no_trans && !trans)) return mfx_fail(MFX_ERR_ARG, "dcn_v2_psroi_pooling_backward: null pointer");
    d.scale = spatial_scale; d.trans_std = trans_std;
    int G = 1;
    while (G < d.cpc && G < 64) G <<= 1;
    hipLaunchKernelGGL(psroi_backward_kernel, dim3((unsigned)(N * d.num_classes)), dim3(THREADS), 0, st, out_grad, input, bbox, trans, top_count, grad_input,
                       grad_trans, d, G);
    MFX_HIP_CHECK(hipGetLastError());
    return MFX_OK;
}
