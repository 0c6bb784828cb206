// AdamW over ALL parameter tensors of the model in one launch (r06).  The reference's optimizer is torch.optim.AdamW with one group per parameter
// (solver/__init__.py:10-60: 280 groups); this build's host side merges them into two groups (weights / biases, monoflex_amd/solver.py) and ran torch's
// fused multi-tensor kernel: 25 launches and 345 us of a 18 ms training step for 560 MB of traffic (20 M parameters x (read p, g, m, v + write p, m, v)).
// Here every workgroup owns one 4096-element chunk of one tensor (a pointer table on the device says which: the chunk -> tensor search is one ballot per
// 256 table entries, as in pack_conv_weight_batched_kernel), streams it with 16-byte accesses and applies
//     p -= lr wd p;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// (decoupled weight decay, bias correction in double: the arithmetic of torch's `_fused_adamw_`, capturable form: t and lr are read from the device).
// The per-tensor step counters (torch keeps one per parameter) are advanced by a one-workgroup launch in front, so every chunk reads a settled value.
// `found_inf` (the fp16 loss scaler's flag): when set, nothing moves -- parameters, moments and counters stay as they are.
//
// Training recipes (mfx_optim_multi, mfx_grad_norm_multi): the same launch serves the reference's other optimizer and its gradient clipping.
//   RULE      MFX_OPTIM_ADAMW as above; MFX_OPTIM_ADAM_L2 = torch.optim.Adam(weight_decay) (reference solver/__init__.py:33-34; torch's capturable
//             `_fused_adam_`): g' = g + wd p, both moments on g', then the same bias-corrected step.
//   COEF      every gradient element is multiplied by the device scalar *grad_coef in fp32 before anything else -- the rounding of
//             clip_grad_norm_'s in-place `g.mul_(coef)` followed by the optimizer's read.  The gradient is NOT written back: after a clipped
//             step p.grad keeps the UNCLIPPED values (nothing downstream of the optimizer step reads them; zero_grad drops them).
//   norm      coef = min(1, max_norm / (total_norm + 1e-6)) comes from two launches over the same tables: grad_sq_partials_kernel (one workgroup
//             per chunk: 16 squares per thread added in series in fp32, then a fixed shuffle + LDS tree, one partial per chunk stored by one
//             lane) and grad_norm_finish_kernel (one workgroup: partials added in a fixed order in double).  No atomics anywhere, so the norm
//             is the same bits in every run, eager or replayed, and on every rank holding the same (all-reduced) gradients.
// Both are template parameters: <MFX_OPTIM_ADAMW, false> compiles to the expressions that were here before them (mfx_adamw_multi: same launches, same bits).
//
// One-cycle recipe (mfx_optim_multi_sched: SOLVER.OPTIMIZER 'adam_onecycle', the reference's fastai OptimWrapper over optim.Adam, solver/fastai_optim.py):
//   RULE      MFX_OPTIM_ADAM_TRUE_WD: p *= shrink with shrink = (float)(1 - wd lr) taken in double -- the rounding of the wrapper's `p.data.mul_(1 - wd * lr)`,
//             a product, not p - decay p -- then Adam's moments on the unmodified gradient and the bias-corrected step.
//   DEVB1     beta1 is read from the device like lr (a table of one pointer per group): the one-cycle schedule moves it every iteration, and a host
//             float would be baked into a captured launch.  1 - b1 and b1^t come from (double)*beta1.  A template parameter as COEF is: the
//             instantiations without it read the group record's host float as before.
//   rows      group < 0 marks a NORM-ONLY row (a gradient the clip's norm covers although the optimizer does not hold its parameter: the update
//             returns for its chunks, p / m / v / step may be null).  g == null marks a DECAY-ONLY row of the true-weight-decay rule (a held parameter
//             without a gradient: the wrapper shrinks it all the same and Adam skips it; m / v / step may be null, the norm counts it as zero).
//             The drivers of the two older rules mark no row.
#include "../../include/monoflex_hip.h"
#include "err.h"
#include "common.h"

namespace mfx {

constexpr int AW_CHUNK = 4096;

__global__ __launch_bounds__(256) void adamw_bump_steps_kernel(const mfx_adamw_desc* __restrict__ descs, int n, const float* __restrict__ found_inf) {
    if (found_inf && *found_inf != 0.f) return;
    for (int i = threadIdx.x; i < n; i += blockDim.x)
        if (descs[i].step) *descs[i].step += 1.f;                              // (norm-only and decay-only rows have no counter)
}

// the tensor that owns chunk `chunk`: the last i with prefix[i] <= chunk (one ballot per 256 table entries; all 256 threads call this)
__device__ __forceinline__ int chunk_owner(const long long* __restrict__ prefix, int n, long chunk, int* below) {
    int cnt = 0;
    for (int base = 0; base < n; base += 256) {
        const int idx = base + (int)threadIdx.x;
        cnt += __popcll(__ballot(idx < n && (long)prefix[idx] <= chunk));
    }
    if ((threadIdx.x & 63) == 0) below[threadIdx.x >> 6] = cnt;
    __syncthreads();
    return below[0] + below[1] + below[2] + below[3] - 1;
}

template <int RULE, bool COEF, bool DEVB1>
__global__ __launch_bounds__(256) void adamw_multi_kernel(const mfx_adamw_desc* __restrict__ descs, const long long* __restrict__ prefix, int n,
                                                         const mfx_adamw_group* __restrict__ groups, const float* __restrict__ found_inf,
                                                         const float* __restrict__ grad_coef, const float* const* __restrict__ beta1_tab) {
    if (found_inf && *found_inf != 0.f) return;
    __shared__ int below[4];
    const long chunk = blockIdx.x;
    const int ti = chunk_owner(prefix, n, chunk, below);
    const mfx_adamw_desc d = descs[ti];
    if (d.group < 0) return;                                                  // a norm-only row (uniform per workgroup)
    const mfx_adamw_group gr = groups[d.group];
    const long j0 = (chunk - (long)prefix[ti]) * AW_CHUNK;
    const long j1 = j0 + AW_CHUNK < d.numel ? j0 + AW_CHUNK : d.numel;
    float* p = reinterpret_cast<float*>(d.p);
    const float* g = reinterpret_cast<const float*>(d.g);
    // scalars of the step (uniform per tensor)
    const float fb1 = DEVB1 ? *beta1_tab[d.group] : gr.beta1;
    const double lr = (double)*gr.lr, b1 = (double)fb1, b2 = (double)gr.beta2;
    const float shrink = (float)(1.0 - (double)gr.weight_decay * lr);         // (MFX_OPTIM_ADAM_TRUE_WD only)
    if (RULE == MFX_OPTIM_ADAM_TRUE_WD && g == nullptr) {                     // a decay-only row: the same elements in the same order, one product each
        for (long j = j0 + (long)threadIdx.x * 4; j < j1; j += 1024)
            for (long e = j; e < j + 4 && e < j1; ++e) p[e] *= shrink;
        return;
    }
    const double t = (double)*d.step;                                         // already advanced (adamw_bump_steps_kernel)
    const float decay = (float)(lr * (double)gr.weight_decay);
    const float step_size = (float)(lr / (1.0 - pow(b1, t)));
    const float bc2_sqrt = (float)sqrt(1.0 - pow(b2, t));
    const float w1 = (float)(1.0 - b1), fb2 = gr.beta2, w2 = (float)(1.0 - b2), eps = gr.eps;
    const float wd = gr.weight_decay, coef = COEF ? *grad_coef : 1.f;
    float* m = reinterpret_cast<float*>(d.m);
    float* v = reinterpret_cast<float*>(d.v);
    auto upd = [&](float& pp, float gg, float& mm, float& vv) {
        if (COEF) {
            gg *= coef;
            asm volatile("" : "+v"(gg));              // the scaled gradient is a finished fp32 value, as if read back from memory: what follows is the
        }                                             // expression the unscaled kernel evaluates (coef == 1 gives the unclipped step's bits)
        if (RULE == MFX_OPTIM_ADAM_L2) gg += wd * pp;
        else if (RULE == MFX_OPTIM_ADAM_TRUE_WD) {
            pp *= shrink;
            asm volatile("" : "+v"(pp));              // a finished fp32 product (`mul_`), not to be contracted into the step's subtraction
        } else pp -= decay * pp;
        mm = fb1 * mm + w1 * gg;
        vv = fb2 * vv + w2 * gg * gg;
        pp -= step_size * mm / (sqrtf(vv) / bc2_sqrt + eps);
    };
    const bool vec = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) & 15) == 0;
    long j = j0 + (long)threadIdx.x * 4;
    if (vec) {
        for (; j + 4 <= j1; j += 1024) {
            f32x4 pv = *reinterpret_cast<const f32x4*>(p + j), mv = *reinterpret_cast<const f32x4*>(m + j), vv = *reinterpret_cast<const f32x4*>(v + j);
            const f32x4 gv = *reinterpret_cast<const f32x4*>(g + j);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float pe = pv[e], me = mv[e], ve = vv[e];
                upd(pe, gv[e], me, ve);
                pv[e] = pe; mv[e] = me; vv[e] = ve;
            }
            *reinterpret_cast<f32x4*>(p + j) = pv; *reinterpret_cast<f32x4*>(m + j) = mv; *reinterpret_cast<f32x4*>(v + j) = vv;
        }
    }
    // the chunk's ragged end (and every element of a tensor whose storage is not 16-byte aligned)
    for (; j < j1; j += 1024)
        for (long e = j; e < j + 4 && e < j1; ++e) upd(p[e], g[e], m[e], v[e]);
}

// ---- gradient norm over the same tables ------------------------------------------------------------------------------------------
// partial[chunk] = sum of g^2 over the chunk: thread t adds its 16 elements (4 consecutive ones at j0 + 4t + 1024k, k = 0..3) in that order,
// then xor-shuffle levels 32..1 inside each wave and waves 0..3 in order -- at most 16 serial additions and 8 tree levels in fp32.
__global__ __launch_bounds__(256) void grad_sq_partials_kernel(const mfx_adamw_desc* __restrict__ descs, const long long* __restrict__ prefix, int n,
                                                              float* __restrict__ partial) {
    __shared__ int below[4];
    __shared__ float wsum[4];
    const long chunk = blockIdx.x;
    const int ti = chunk_owner(prefix, n, chunk, below);
    const mfx_adamw_desc d = descs[ti];
    const long j0 = (chunk - (long)prefix[ti]) * AW_CHUNK;
    const long j1 = j0 + AW_CHUNK < d.numel ? j0 + AW_CHUNK : d.numel;
    const float* g = reinterpret_cast<const float*>(d.g);
    const bool vec = (reinterpret_cast<uintptr_t>(g) & 15) == 0;
    float s = 0.f;
    long j = g ? j0 + (long)threadIdx.x * 4 : j1;                              // (a decay-only row has no gradient: its partial is 0)
    if (vec) {
        for (; j + 4 <= j1; j += 1024) {
            const f32x4 gv = *reinterpret_cast<const f32x4*>(g + j);
#pragma unroll
            for (int e = 0; e < 4; ++e) s += gv[e] * gv[e];
        }
    }
    for (; j < j1; j += 1024)                                                  // ragged end / unaligned storage: the same elements in the same order
        for (long e = j; e < j + 4 && e < j1; ++e) s += g[e] * g[e];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[chunk] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// out2 = [total_norm, coef]: thread t adds partials t, t + 256, ... in double, then a fixed LDS tree; torch's clip_grad_norm_ rule in fp32 on the
// rounded norm (a NaN norm gives a NaN coef, as torch's clamp does).  found_inf set: the norm is still written, coef stays 1.
__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const float* __restrict__ partial, long nchunk, float max_norm, float* __restrict__ out2,
                                                              const float* __restrict__ found_inf) {
    __shared__ double acc[256];
    double s = 0.0;
    for (long i = threadIdx.x; i < nchunk; i += 256) s += (double)partial[i];
    acc[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) acc[threadIdx.x] += acc[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float total = (float)sqrt(acc[0]);
        float c = max_norm / (total + 1e-6f);
        if (c > 1.f) c = 1.f;
        if (found_inf && *found_inf != 0.f) c = 1.f;
        out2[0] = total;
        out2[1] = c;
    }
}

}  // namespace mfx
using namespace mfx;

extern "C" int mfx_adamw_chunk_elems(void) { return AW_CHUNK; }

extern "C" int mfx_adamw_multi(const mfx_adamw_desc* descs_dev, const long long* prefix_dev, int n, long long total_chunks,
                               const mfx_adamw_group* groups_dev, const float* found_inf, void* stream) {
    if (n <= 0 || total_chunks <= 0) return MFX_OK;
    if (!descs_dev || !prefix_dev || !groups_dev) return mfx_fail(MFX_ERR_ARG, "adamw_multi: null pointer");
    if (total_chunks >= (1LL << 31)) return mfx_fail(MFX_ERR_ARG, "adamw_multi: too many chunks");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(adamw_bump_steps_kernel, dim3(1), dim3(256), 0, st, descs_dev, n, found_inf);
    hipLaunchKernelGGL((adamw_multi_kernel<MFX_OPTIM_ADAMW, false, false>), dim3((unsigned)total_chunks), dim3(256), 0, st, descs_dev, prefix_dev, n, groups_dev,
                       found_inf, (const float*)nullptr, (const float* const*)nullptr);
    ++g_cnt_adamw_multi;
    MFX_HIP_CHECK(hipGetLastError());
    return MFX_OK;
}

extern "C" int mfx_optim_multi(const mfx_adamw_desc* descs_dev, const long long* prefix_dev, int n, long long total_chunks,
                               const mfx_adamw_group* groups_dev, int rule, const float* grad_coef, const float* found_inf, void* stream) {
    if (rule != MFX_OPTIM_ADAMW && rule != MFX_OPTIM_ADAM_L2) return mfx_fail(MFX_ERR_ARG, "optim_multi: rule must be 0 (AdamW) or 1 (Adam with L2 decay)");
    if (n <= 0 || total_chunks <= 0) return MFX_OK;
    if (!descs_dev || !prefix_dev || !groups_dev) return mfx_fail(MFX_ERR_ARG, "optim_multi: null pointer");
    if (total_chunks >= (1LL << 31)) return mfx_fail(MFX_ERR_ARG, "optim_multi: too many chunks");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(adamw_bump_steps_kernel, dim3(1), dim3(256), 0, st, descs_dev, n, found_inf);
#define MFX_OPTIM_LAUNCH(R_, C_) \
    hipLaunchKernelGGL((adamw_multi_kernel<R_, C_, false>), dim3((unsigned)total_chunks), dim3(256), 0, st, descs_dev, prefix_dev, n, groups_dev, found_inf, grad_coef, \
                       (const float* const*)nullptr)
    if (rule == MFX_OPTIM_ADAMW) { if (grad_coef) MFX_OPTIM_LAUNCH(MFX_OPTIM_ADAMW, true); else MFX_OPTIM_LAUNCH(MFX_OPTIM_ADAMW, false); }
    else { if (grad_coef) MFX_OPTIM_LAUNCH(MFX_OPTIM_ADAM_L2, true); else MFX_OPTIM_LAUNCH(MFX_OPTIM_ADAM_L2, false); }
#undef MFX_OPTIM_LAUNCH
    ++g_cnt_optim_multi;
    MFX_HIP_CHECK(hipGetLastError());
    return MFX_OK;
}

extern "C" int mfx_optim_multi_sched(const mfx_adamw_desc* descs_dev, const long long* prefix_dev, int n, long long total_chunks,
                                     const mfx_adamw_group* groups_dev, const float* const* beta1_dev, int rule, const float* grad_coef, const float* found_inf,
                                     void* stream) {
    if (rule != MFX_OPTIM_ADAMW && rule != MFX_OPTIM_ADAM_L2 && rule != MFX_OPTIM_ADAM_TRUE_WD)
        return mfx_fail(MFX_ERR_ARG, "optim_multi_sched: rule must be 0 (AdamW), 1 (Adam with L2 decay) or 2 (Adam with true weight decay)");
    if (n <= 0 || total_chunks <= 0) return MFX_OK;
    if (!descs_dev || !prefix_dev || !groups_dev || !beta1_dev) return mfx_fail(MFX_ERR_ARG, "optim_multi_sched: null pointer");
    if (total_chunks >= (1LL << 31)) return mfx_fail(MFX_ERR_ARG, "optim_multi_sched: too many chunks");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(adamw_bump_steps_kernel, dim3(1), dim3(256), 0, st, descs_dev, n, found_inf);
#define MFX_OPTIM_LAUNCH(R_, C_) \
    hipLaunchKernelGGL((adamw_multi_kernel<R_, C_, true>), dim3((unsigned)total_chunks), dim3(256), 0, st, descs_dev, prefix_dev, n, groups_dev, found_inf, grad_coef, \
                       beta1_dev)
    if (rule == MFX_OPTIM_ADAMW) { if (grad_coef) MFX_OPTIM_LAUNCH(MFX_OPTIM_ADAMW, true); else MFX_OPTIM_LAUNCH(MFX_OPTIM_ADAMW, false); }
    else if (rule == MFX_OPTIM_ADAM_L2) { if (grad_coef) MFX_OPTIM_LAUNCH(MFX_OPTIM_ADAM_L2, true); else MFX_OPTIM_LAUNCH(MFX_OPTIM_ADAM_L2, false); }
    else { if (grad_coef) MFX_OPTIM_LAUNCH(MFX_OPTIM_ADAM_TRUE_WD, true); else MFX_OPTIM_LAUNCH(MFX_OPTIM_ADAM_TRUE_WD, false); }
#undef MFX_OPTIM_LAUNCH
    ++g_cnt_optim_multi_sched;
    MFX_HIP_CHECK(hipGetLastError());
    return MFX_OK;
}

extern "C" size_t mfx_grad_norm_workspace_bytes(long long total_chunks) { return sizeof(float) * (size_t)(total_chunks > 0 ? total_chunks : 1); }

extern "C" int mfx_grad_norm_multi(const mfx_adamw_desc* descs_dev, const long long* prefix_dev, int n, long long total_chunks, float max_norm,
                                   void* workspace, size_t workspace_bytes, float* out2, const float* found_inf, void* stream) {
    if (n < 0 || total_chunks < 0 || !(max_norm > 0.f)) return mfx_fail(MFX_ERR_ARG, "grad_norm_multi: bad sizes or max_norm <= 0");
    if (!out2 || ((n > 0 && total_chunks > 0) && (!descs_dev || !prefix_dev || !workspace))) return mfx_fail(MFX_ERR_ARG, "grad_norm_multi: null pointer");
    if (total_chunks >= (1LL << 31)) return mfx_fail(MFX_ERR_ARG, "grad_norm_multi: too many chunks");
    if (workspace_bytes < mfx_grad_norm_workspace_bytes(total_chunks)) return mfx_fail(MFX_ERR_ARG, "grad_norm_multi: workspace too small (mfx_grad_norm_workspace_bytes)");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long long nchunk = n > 0 ? total_chunks : 0;
    if (nchunk > 0)
        hipLaunchKernelGGL(grad_sq_partials_kernel, dim3((unsigned)nchunk), dim3(256), 0, st, descs_dev, prefix_dev, n, reinterpret_cast<float*>(workspace));
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, st, reinterpret_cast<const float*>(workspace), (long)nchunk, max_norm, out2, found_inf);
    ++g_cnt_grad_norm_multi;
    MFX_HIP_CHECK(hipGetLastError());
    return MFX_OK;
}
