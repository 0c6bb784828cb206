// Detection decode on device (reference model/layers/utils.py:39-145, model/head/detector_infer.py:77-237,
// model/anno_encoder.py:69-295): sigmoid/clamp -> 3x3 max NMS -> per-class top-K -> merge to K ->
// POI gather (free in NHWC) -> 2D box / dimensions / 4 depths / soft fusion / location / orientation.
// Latency-bound (reads 3*H*W + K*50 values per image); two launches, no host sync.
#include "../../include/monoflex_hip.h"
#include "common.h"
#include "box_decode_math.h"
#include "err.h"
#include <cmath>

namespace mfx {

constexpr int kTopkThreads = 1024;

__device__ __forceinline__ float sigmoid_clamp(float x) {          // layers/utils.py:39-43
    const float s = 1.f / (1.f + expf(-x));
    return fminf(fmaxf(s, 1e-4f), 1.f - 1e-4f);
}

// (value desc, index asc) ordering; ties go to the lower flat index
__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// Exact k-th-largest selection by radix histograms over LDS-resident keys.
// Among the elements p in [0,n) with `pred(p)`, returns the key of rank `need` (1 = largest) and writes how many
// of the elements EQUAL to that key belong to the top `need` into *take_eq.  keys are < 2^32, examined in
// three digit levels (12 + 10 + 10 bits).  One workgroup; hist has 4096 ints; sh[0..1] is scratch.
// NLEV = 3: digits of 12 + 10 + 10 bits (few passes over many keys); NLEV = 4: four 8-bit digits (small key sets: the
// per-level cost is then the 256-bin scan, not the 4096-bin one).
template <int NLEV = 3, class KeyF, class PredF>
__device__ uint32_t select_kth(KeyF key, PredF pred, int n, int need, int* hist, int* sh, int* take_eq) {
    const int tid = threadIdx.x, lane = tid & 63, nthreads = blockDim.x;
    const int shifts[4] = {NLEV == 3 ? 20 : 24, NLEV == 3 ? 10 : 16, NLEV == 3 ? 0 : 8, 0};
    const int nbits[4] = {NLEV == 3 ? 12 : 8, NLEV == 3 ? 10 : 8, NLEV == 3 ? 10 : 8, 8};
    uint32_t prefix = 0;
    for (int lev = 0; lev < NLEV; ++lev) {
        const int nb = 1 << nbits[lev], sft = shifts[lev];
        for (int i = tid; i < nb; i += nthreads) hist[i] = 0;
        __syncthreads();
        for (int p = tid; p < n; p += nthreads) {
            if (!pred(p)) continue;
            const uint32_t k = key(p);
            const bool match = lev == 0 || (k >> (sft + nbits[lev])) == prefix;
            if (match) atomicAdd(&hist[(k >> sft) & (nb - 1)], 1);
        }
        __syncthreads();
        if (tid < 64) {                                   // one wave walks the bins from the top
            const int per = nb / 64;
            int local = 0;
            for (int j = 0; j < per; ++j) local += hist[lane * per + j];
            int incl = local;                             // inclusive suffix sum over lanes (lane 63 = highest bins)
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int v = __shfl_down(incl, off);
                if (lane + off < 64) incl += v;
            }
            const int excl = incl - local;
            if (incl >= need && excl < need) {            // exactly one lane owns the bin
                int c = excl, bsel = lane * per;
                for (int j = per - 1; j >= 0; --j) {
                    const int h = hist[lane * per + j];
                    if (c + h >= need) { bsel = lane * per + j; break; }
                    c += h;
                }
                sh[0] = bsel; sh[1] = need - c;           // remaining rank inside the chosen bin
            }
        }
        __syncthreads();
        prefix = (prefix << nbits[lev]) | (uint32_t)sh[0];
        need = sh[1];
        __syncthreads();
    }
    *take_eq = need;
    return prefix;
}

// One workgroup per (class, image): sigmoid/clamp + 3x3 NMS into LDS, exact top-K by radix selection
// (ties toward the lower flat index), rank-sort of the K winners.
__global__ __launch_bounds__(kTopkThreads) void decode_topk_kernel(const float* hmap, long b_stride, long c_stride, long p_stride,
                                                                    int H, int W, int K, float* scores, int* index) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* nm = reinterpret_cast<float*>(smem_raw);                // [H*W]: logits, then heat after NMS
    __shared__ int hist[4096];
    __shared__ int sh[2];
    __shared__ int cnt;
    __shared__ float cand_v[256];
    __shared__ int cand_i[256];
    const int cls = blockIdx.x, b = blockIdx.y, ncls = gridDim.x, HW = H * W;
    const int tid = threadIdx.x;
    const float* src = hmap + (size_t)b * b_stride + (size_t)cls * c_stride;
    // stage the class logits in LDS: one global read per pixel (contiguous when the map is planar)
    for (int p = tid; p < HW; p += kTopkThreads) nm[p] = src[(size_t)p * p_stride];
    __syncthreads();
    // nms_hm (layers/utils.py:45-58): keep where the 3x3 max-pool equals the value (plateaus survive).
    // sigmoid/clamp is monotone: compare logits, evaluate the heat only to decide ties after rounding/clamping.
    unsigned long long keepmask = 0ull;                           // this thread's pixels p = tid + i*1024, i < 64
    int i = 0;
    for (int p = tid; p < HW; p += kTopkThreads, ++i) {
        const int y = p / W, x = p - y * W;
        const float xv = nm[p];
        float xm = -3.0e38f;
        for (int dy = -1; dy <= 1; ++dy) {
            const int yy = y + dy;
            if (yy < 0 || yy >= H) continue;
            for (int dx = -1; dx <= 1; ++dx) {
                const int xx = x + dx;
                if (xx < 0 || xx >= W || (dx == 0 && dy == 0)) continue;
                xm = fmaxf(xm, nm[yy * W + xx]);
            }
        }
        const bool keep = xv >= xm || sigmoid_clamp(xv) == sigmoid_clamp(xm);
        keepmask |= (unsigned long long)(keep ? 1 : 0) << i;
    }
    __syncthreads();
    i = 0;
    for (int p = tid; p < HW; p += kTopkThreads, ++i) nm[p] = ((keepmask >> i) & 1ull) ? sigmoid_clamp(nm[p]) : 0.f;
    if (tid == 0) { cnt = 0; sh[0] = 0; }
    __syncthreads();
    // ~90 % of the map is exactly 0 after the NMS: histogramming those would serialise ~27 k LDS atomics on one bin per
    // radix level (that was 80 % of this kernel's time).  Count the survivors; when at least K exist the zeros cannot be
    // among the top K and are left out of the selection.
    {
        int nz = 0;
        for (int p = tid; p < HW; p += kTopkThreads) nz += nm[p] != 0.f ? 1 : 0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) nz += __shfl_xor(nz, off);
        if ((tid & 63) == 0 && nz) atomicAdd(&sh[0], nz);
    }
    __syncthreads();
    const bool skip_zero = sh[0] >= K;
    __syncthreads();
    // K-th largest heat T; take_eq = how many of the elements equal to T are in the top K
    int take_eq = 0;
    const uint32_t T = select_kth([&](int p) { return __float_as_uint(nm[p]); }, [&](int p) { return !skip_zero || nm[p] != 0.f; },
                                  HW, K, hist, sh, &take_eq);
    // among the elements equal to T keep the take_eq lowest flat indices: k-th largest of (HW-1-p)
    int dummy = 0;
    const uint32_t I = select_kth([&](int p) { return (uint32_t)(HW - 1 - p); },
                                  [&](int p) { return __float_as_uint(nm[p]) == T; }, HW, take_eq, hist, sh, &dummy);
    for (int p = tid; p < HW; p += kTopkThreads) {
        const uint32_t kb = __float_as_uint(nm[p]);
        if (kb > T || (kb == T && (uint32_t)(HW - 1 - p) >= I)) {
            const int slot = atomicAdd(&cnt, 1);
            if (slot < 256) { cand_v[slot] = nm[p]; cand_i[slot] = p; }
        }
    }
    __syncthreads();
    const int n = cnt < K ? cnt : K;                      // == K by construction
    if (tid < n) {
        const float v = cand_v[tid]; const int i = cand_i[tid];
        int rank = 0;
        for (int u = 0; u < n; ++u) rank += better(cand_v[u], cand_i[u], v, i) ? 1 : 0;
        scores[((size_t)b * ncls + cls) * K + rank] = v;
        index[((size_t)b * ncls + cls) * K + rank] = i;
    }
}

// ---- strip-parallel form of stage 1 ---------------------------------------------------------------------------------
// The single-workgroup kernel above keeps one (class, image) map in one CU's LDS: 24 workgroups for B=8, i.e. a 256-CU
// device runs a chain of serial radix passes on 9 % of its CUs (79 us).  Here each map is cut into row strips; every strip
// (its rows + one halo row each side for the NMS) is reduced to its own exact top-K by one small workgroup, and a second
// tiny kernel merges the S*K candidates.  Any element of the global top-K is in the top-K of its strip under the same total
// order (value desc, flat index asc), so the result is identical.
#ifndef MFX_STRIP_THREADS
#define MFX_STRIP_THREADS 1024
#endif
constexpr int kStripThreads = MFX_STRIP_THREADS;

__global__ __launch_bounds__(kStripThreads) void decode_topk_strip_kernel(const float* hmap, long b_stride, long c_stride, long p_stride,
                                                                          int H, int W, int K, int rows_per, float* cand_v, int* cand_i) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int strip = blockIdx.x, S = gridDim.x, cls = blockIdx.y, ncls = gridDim.y, b = blockIdx.z;
    const int r0 = strip * rows_per, r1 = min(H, r0 + rows_per);
    const int ylo = max(r0 - 1, 0), yhi = min(r1 + 1, H);
    const int nloc = (r1 - r0) * W, nstage = (yhi - ylo) * W;
    float* lg = reinterpret_cast<float*>(smem_raw);                 // [(rows_per+2)*W] logits of rows ylo..yhi
    float* nm = lg + (rows_per + 2) * W;                            // [rows_per*W] heat after NMS
    __shared__ int hist[256];
    __shared__ int sh[2];
    __shared__ int cnt;
    __shared__ float cv[256];
    __shared__ int ci[256];
    const int tid = threadIdx.x;
    const float* src = hmap + (size_t)b * b_stride + (size_t)cls * c_stride;
    for (int q = tid; q < nstage; q += kStripThreads) lg[q] = src[(size_t)(ylo * W + q) * p_stride];
    if (tid == 0) { cnt = 0; sh[0] = 0; }
    __syncthreads();
    int nz = 0;
    for (int q = tid; q < nloc; q += kStripThreads) {               // nms_hm (layers/utils.py:45-58), same tie rule as above
        const int y = r0 + q / W, x = q % W;
        const float xv = lg[(y - ylo) * W + x];
        float xm = -3.0e38f;
        for (int dy = -1; dy <= 1; ++dy) {
            const int yy = y + dy;
            if (yy < 0 || yy >= H) continue;
            for (int dx = -1; dx <= 1; ++dx) {
                const int xx = x + dx;
                if (xx < 0 || xx >= W || (dx == 0 && dy == 0)) continue;
                xm = fmaxf(xm, lg[(yy - ylo) * W + xx]);
            }
        }
        const bool keep = xv >= xm || sigmoid_clamp(xv) == sigmoid_clamp(xm);
        const float h = keep ? sigmoid_clamp(xv) : 0.f;
        nm[q] = h;
        nz += h != 0.f ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nz += __shfl_xor(nz, off);
    if ((tid & 63) == 0 && nz) atomicAdd(&sh[0], nz);
    __syncthreads();
    const int need = K < nloc ? K : nloc;
    const bool skip_zero = sh[0] >= need;
    float* ov = cand_v + (((size_t)b * ncls + cls) * S + strip) * K;
    int* oi = cand_i + (((size_t)b * ncls + cls) * S + strip) * K;
    // Fast path (the usual case: the 3x3 NMS leaves ~1 pixel in 9, a few hundred per strip): when the survivors alone fill the strip's top-K and fit
    // the list below, they are compacted and every survivor COUNTS the survivors ahead of it under the same total order (value desc, flat index
    // asc: one 64-bit key, heat bits high -- heat > 0, so bit order is value order -- and ~index low).  Its count is its rank: ranks < need are the
    // strip's top-K, already sorted.  Same set as the radix selection below (which stays for dense maps and for strips that must take zeros).
    constexpr int kSurvCap = 512;
    __shared__ unsigned long long surv[kSurvCap];
    const int ns = sh[0];
    if (ns >= need && ns <= kSurvCap && need > 0) {
        for (int q = tid; q < nloc; q += kStripThreads) {
            const float h = nm[q];
            if (h != 0.f) surv[atomicAdd(&cnt, 1)] = ((unsigned long long)__float_as_uint(h) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)q);
        }
        __syncthreads();
        for (int c = tid; c < ns; c += kStripThreads) {
            const unsigned long long mine = surv[c];
            int rank = 0;
#pragma unroll 8
            for (int u = 0; u < ns; ++u) rank += surv[u] > mine ? 1 : 0;            // (every lane reads the same entry: one broadcast LDS read)
            if (rank < need) { ov[rank] = __uint_as_float((uint32_t)(mine >> 32)); oi[rank] = r0 * W + (int)(0xffffffffu - (uint32_t)mine); }
        }
        for (int t = need + tid; t < K; t += kStripThreads) { ov[t] = -1.f; oi[t] = 0x7fffffff; }
        return;
    }
    __syncthreads();
    int take_eq = 0, dummy = 0;
    const uint32_t T = select_kth<4>([&](int q) { return __float_as_uint(nm[q]); }, [&](int q) { return !skip_zero || nm[q] != 0.f; },
                                     nloc, need, hist, sh, &take_eq);
    const uint32_t I = select_kth<4>([&](int q) { return (uint32_t)(nloc - 1 - q); },
                                  [&](int q) { return __float_as_uint(nm[q]) == T; }, nloc, take_eq, hist, sh, &dummy);
    for (int q = tid; q < nloc; q += kStripThreads) {
        const uint32_t kb = __float_as_uint(nm[q]);
        if (kb > T || (kb == T && (uint32_t)(nloc - 1 - q) >= I)) {
            const int slot = atomicAdd(&cnt, 1);
            if (slot < 256) { cv[slot] = nm[q]; ci[slot] = r0 * W + q; }
        }
    }
    __syncthreads();
    const int n = cnt < need ? cnt : need;                          // == need by construction
    for (int t = tid; t < K; t += kStripThreads) {
        if (t < n) { ov[t] = cv[t]; oi[t] = ci[t]; }
        else { ov[t] = -1.f; oi[t] = 0x7fffffff; }                   // padding: below every heat value (heat >= 0)
    }
}

// Rank of every candidate among the S*K candidates of its map.  One wave per candidate: the lanes split the comparison
// range (independent LDS reads, a few per lane) and add their counts; a thread-per-candidate loop over all n candidates is a
// chain of ~2n dependent LDS round trips and took longer than the whole single-workgroup selection.
__global__ __launch_bounds__(512) void decode_topk_merge_kernel(const float* cand_v, const int* cand_i, int n, int K, float* scores, int* index) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* v = reinterpret_cast<float*>(smem_raw);
    int* ix = reinterpret_cast<int*>(v + n);
    const size_t map = (size_t)blockIdx.y * gridDim.x + blockIdx.x;   // (image, class)
    for (int t = threadIdx.x; t < n; t += blockDim.x) { v[t] = cand_v[map * n + t]; ix[t] = cand_i[map * n + t]; }
    __syncthreads();
    const int lane = threadIdx.x & 63, nwaves = (blockDim.x >> 6) * gridDim.z, wave = blockIdx.z * (blockDim.x >> 6) + (threadIdx.x >> 6);
    for (int c = wave; c < n; c += nwaves) {                        // the candidates are dealt to the waves of gridDim.z workgroups
        const float mv = v[c]; const int mi = ix[c];
        int rank = 0;
#pragma unroll 4
        for (int u = lane; u < n; u += 64) rank += better(v[u], ix[u], mv, mi) ? 1 : 0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) rank += __shfl_xor(rank, off);
        if (lane == 0 && rank < K) { scores[map * K + rank] = mv; index[map * K + rank] = mi; }
    }
}

__global__ __launch_bounds__(256) void decode_boxes_kernel(const float* hmap, int ld, int reg_off, const float* scores, const int* index,
                                                           int ncls, int H, int W, int K, const float* calib, const int* pad,
                                                           const int* img_size, float threshold, mfx_decode_cfg dc, mfx_head_layout hl,
                                                           float* det, float* topk, int* valid, float* unc) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* cs = reinterpret_cast<float*>(smem_raw);          // [ncls*K]
    int* ci = reinterpret_cast<int*>(cs + ncls * K);         // [ncls*K]
    int* slot = ci + ncls * K;                               // [K] position (in the ncls*K list) of rank j
    const int b = blockIdx.x, tid = threadIdx.x, n = ncls * K;
    for (int t = tid; t < n; t += blockDim.x) { cs[t] = scores[(size_t)b * n + t]; ci[t] = index[(size_t)b * n + t]; }
    __syncthreads();
    // select_topk stage 2 (utils.py:88-91): top-K of the concatenated list, ties -> lower position
    for (int t = tid; t < n; t += blockDim.x) {
        const float v = cs[t];
        int rank = 0;
        for (int u = 0; u < n; ++u) rank += better(cs[u], u, v, t) ? 1 : 0;
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
    const bdec::Row row = bdec::decode_row(r, px, py, cls, score, cam, (float)(img_size[0] - 1), (float)(img_size[1] - 1), dc, hl);

    float* o = det + ((size_t)b * K + j) * 14;
    for (int i = 0; i < 14; ++i) o[i] = row.det[i];
    float* t = topk + ((size_t)b * K + j) * 5;
    t[0] = score; t[1] = (float)idx; t[2] = (float)cls; t[3] = py; t[4] = px;
    valid[b * K + j] = score >= threshold ? 1 : 0;
    if (unc) {                                                // [estimated_depth_error, uncertainty_conf]
        unc[((size_t)b * K + j) * 2 + 0] = row.as_conf ? row.sigma : 0.f;
        unc[((size_t)b * K + j) * 2 + 1] = row.as_conf ? row.conf : 0.f;
    }
}

}  // namespace mfx
using namespace mfx;


extern "C" size_t mfx_decode_topk_workspace_bytes(int ncls, int B, int K) {
    return (size_t)B * ncls * 16 * K * 8;                           // up to 16 strips of K (value, index) pairs
}

extern "C" int mfx_decode_topk(const float* hmap, long b_stride, long c_stride, long p_stride, int ncls, int B, int H, int W, int K,
                               float* scores, int32_t* index, void* workspace, size_t workspace_bytes, void* stream) {
    if (!hmap || !scores || !index) return mfx_fail(MFX_ERR_ARG, "decode_topk: null pointer");
    if (K < 1 || K > H * W || K > 256) return mfx_fail(MFX_ERR_ARG, "decode_topk: need 1 <= K <= min(H*W, 256)");
    if (B * ncls == 0) return MFX_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int S = g_opt_topk_strips < 1 ? 1 : (g_opt_topk_strips > 16 ? 16 : g_opt_topk_strips);
    while (S > 1 && ((H + S - 1) / S) * W < K) --S;                 // every strip must be able to hold K candidates ...
    while (S > 1 && (S - 1) * ((H + S - 1) / S) >= H) --S;          // ... and no strip may be empty
    if (workspace && S > 1 && workspace_bytes >= (size_t)B * ncls * S * K * 8) {
        const int rows_per = (H + S - 1) / S;
        float* cand_v = reinterpret_cast<float*>(workspace);
        int* cand_i = reinterpret_cast<int*>(cand_v + (size_t)B * ncls * S * K);
        const size_t smem = (size_t)(2 * rows_per + 2) * W * sizeof(float);
        if (smem <= 48 * 1024) {
            hipLaunchKernelGGL(decode_topk_strip_kernel, dim3(S, ncls, B), dim3(kStripThreads), smem, st,
                               hmap, b_stride, c_stride, p_stride, H, W, K, rows_per, cand_v, cand_i);
            hipLaunchKernelGGL(decode_topk_merge_kernel, dim3(ncls, B, g_opt_topk_merge_z < 1 ? 1 : g_opt_topk_merge_z), dim3(g_opt_topk_merge_threads), (size_t)S * K * 8, st, cand_v, cand_i, S * K, K, scores, index);
            MFX_HIP_CHECK(hipGetLastError());
            return MFX_OK;
        }
    }
    const size_t smem = (size_t)H * W * sizeof(float);
    if (smem > 136 * 1024) return mfx_fail(MFX_ERR_UNSUPPORTED, "decode_topk: heat map larger than LDS (H*W <= 34816)");
    auto k = decode_topk_kernel;
    static size_t attr_smem = 0;
    if (smem > attr_smem) { MFX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem)); attr_smem = smem; }
    hipLaunchKernelGGL(k, dim3(ncls, B), dim3(kTopkThreads), smem, st, hmap, b_stride, c_stride, p_stride, H, W, K, scores, index);
    MFX_HIP_CHECK(hipGetLastError());
    return MFX_OK;
}

extern "C" int mfx_decode_boxes(const float* hmap, int ld, int reg_off, const float* scores, const int32_t* index,
                                int ncls, int B, int H, int W, int K, const float* calib, const int32_t* pad,
                                const int32_t* img_size, float threshold, float* det, float* topk, int32_t* valid,
                                void* stream) {
    return mfx_decode_boxes_mode(hmap, ld, reg_off, scores, index, ncls, B, H, W, K, calib, pad, img_size, threshold, MFX_DEPTH_SOFT, det, topk, valid, stream);
}

extern "C" int mfx_decode_boxes_mode(const float* hmap, int ld, int reg_off, const float* scores, const int32_t* index,
                                     int ncls, int B, int H, int W, int K, const float* calib, const int32_t* pad,
                                     const int32_t* img_size, float threshold, int depth_mode, float* det, float* topk, int32_t* valid,
                                     void* stream) {
    if (depth_mode < MFX_DEPTH_SOFT || depth_mode > MFX_DEPTH_KEYPOINTS_13) return mfx_fail(MFX_ERR_ARG, "decode_boxes: depth_mode must be one of MFX_DEPTH_*");
    if (!hmap || !scores || !index || !calib || !pad || !img_size || !det || !topk || !valid)
        return mfx_fail(MFX_ERR_ARG, "decode_boxes: null pointer");
    if (K > 256 || ncls != 3) return mfx_fail(MFX_ERR_UNSUPPORTED, "decode_boxes: K <= 256, 3 classes (dimension means)");
    // the runs/monoflex.yaml decode: KITTI DIMENSION_MEAN (config/defaults.py:206-208), exp dimensions without std, inv_sigmoid depth in [0.1, 100],
    // uncertainty-scaled score
    const mfx_decode_cfg cfg = {{3.8840f, 1.5261f, 1.6286f, 0.8423f, 1.7607f, 0.6602f, 1.7635f, 1.7372f, 0.5968f},
                                {0.4259f, 0.1367f, 0.1022f, 0.2349f, 0.1133f, 0.1427f, 0.1766f, 0.0948f, 0.1242f},
                                {26.494627f, 16.05988f}, {0.1f, 100.f}, 4.f, 1e-3f, 2, 1, 0, 1, depth_mode};
    return mfx_decode_boxes_cfg(hmap, ld, reg_off, scores, index, ncls, B, H, W, K, calib, pad, img_size, threshold, &cfg, det, topk, valid, nullptr, stream);
}

extern "C" int mfx_decode_boxes_cfg(const float* hmap, int ld, int reg_off, const float* scores, const int32_t* index,
                                    int ncls, int B, int H, int W, int K, const float* calib, const int32_t* pad,
                                    const int32_t* img_size, float threshold, const mfx_decode_cfg* cfg, float* det, float* topk, int32_t* valid,
                                    float* unc, void* stream) {
    using namespace bdec;
    const mfx_head_layout full = {{R_2D, R_OFF3D, R_KPT, R_KPT_UNC, R_DIM3D, R_ORI_CLS, R_ORI_OFF, R_DEPTH, R_DEPTH_UNC}, R_TOTAL};
    return mfx_decode_boxes_heads(hmap, ld, reg_off, scores, index, ncls, B, H, W, K, calib, pad, img_size, threshold, cfg, &full, det, topk, valid, unc, stream);
}

extern "C" int mfx_decode_boxes_heads(const float* hmap, int ld, int reg_off, const float* scores, const int32_t* index,
                                      int ncls, int B, int H, int W, int K, const float* calib, const int32_t* pad,
                                      const int32_t* img_size, float threshold, const mfx_decode_cfg* cfg, const mfx_head_layout* heads,
                                      float* det, float* topk, int32_t* valid, float* unc, void* stream) {
    if (!cfg) return mfx_fail(MFX_ERR_ARG, "decode_boxes_heads: null cfg");
    if (!heads) return mfx_fail(MFX_ERR_ARG, "decode_boxes_heads: null heads");
    if (!hmap || !scores || !index || !calib || !pad || !img_size || !det || !topk || !valid)
        return mfx_fail(MFX_ERR_ARG, "decode_boxes_heads: null pointer");
    if (const char* e = bdec::decode_cfg_error(*cfg)) return mfx_fail_in(MFX_ERR_ARG, "decode_boxes_heads", e);
    if (ncls < 1 || ncls > 3) return mfx_fail(MFX_ERR_ARG, "decode_boxes_heads: need 1 <= ncls <= 3 (rows of dim_mean / dim_std)");
    if (K < 1 || K > 256) return mfx_fail(MFX_ERR_ARG, "decode_boxes_heads: need 1 <= K <= 256");
    const char* e = bdec::head_layout_error(heads->ch, heads->reg_width);
    if (!e) e = bdec::output_depth_error(cfg->output_depth, *heads);
    if (e) return mfx_fail_in(MFX_ERR_ARG, "decode_boxes_heads", e);
    const int R = heads->reg_width;
    if (B < 0 || H < 1 || W < 1 || ld < R || reg_off < 0 || reg_off + R > ld)
        return mfx_fail(MFX_ERR_ARG, "decode_boxes_heads: need B >= 0, H, W >= 1 and the regression channels inside a row (reg_off + reg_width <= ld)");
    if (B == 0) return MFX_OK;
    const size_t smem = (size_t)ncls * K * 8 + (size_t)K * 4;
    hipLaunchKernelGGL(decode_boxes_kernel, dim3(B), dim3(256), smem, reinterpret_cast<hipStream_t>(stream),
                       hmap, ld, reg_off, scores, index, ncls, H, W, K, calib, pad, img_size, threshold, *cfg, *heads, det, topk, valid, unc);
    MFX_HIP_CHECK(hipGetLastError());
    return MFX_OK;
}
