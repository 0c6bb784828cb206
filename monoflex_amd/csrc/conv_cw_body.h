// The workgroup body of conv_cw.hip's 3x3 kernel, as TEXT: conv3x3_cw_kernel and conv3x3_cw_group_kernel both include it inside their function
// bodies.  (As text and not as a function on purpose: the one-layer kernel's token stream is what it was before the grouped kernel existed, so every
// existing instantiation compiles to the same code; routed through an inlined function the trunk's instantiations changed register counts.)
// The including function provides: template parameters / constants T, TO, CG, CT, WN, FN, WK, S, ROWS, ST; `x`, `wfm` (this layer's map and
// fragment-major weights), `g` (CwGeom), `ep` (EpiArgs); and the macro CW_TILE_ID = this workgroup's tile id inside its layer.
// No include guard: included once per kernel.
    static_assert(sizeof(T) == 2, "16-bit maps");
    static_assert(ROWS % 2 == 0, "the K loop reads the pixel fragments in two half-tiles");
    using SM = CwSmem<CG, WN, FN, WK, S, ROWS>;
    constexpr int NT = WN * WK * 64, FM = ROWS, HR = ROWS / 2, PW = SM::PW, PH = SM::PH;
    constexpr int PS = SM::PS, CPP = CG / 8;
    constexpr int KS = CG / 32;                       // 64-byte K steps per tap and channel group
    constexpr int NG = CT / CG, FSTEPS = (9 * CT + 63) / 64 * 2;   // channel groups; steps per fragment row of the fragment-major weights (K padded to 128 bytes)
    constexpr int SPG = 9 * KS, NL = SPG / WK;        // steps per group; steps per wave and group
    static_assert(KS % WK == 0 && CT % CG == 0 && FM % WK == 0, "K split must divide the steps of a tap and the rows");
    constexpr int BN = WN * FN * 16;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave % WN, wk = wave / WN;
    const int xl = lane & 15, kq = lane >> 4;

    int tile = CW_TILE_ID;
    const int tn = tile % g.tiles_n; tile /= g.tiles_n;
    const int tx = tile % g.tiles_x; tile /= g.tiles_x;
    const int ty = tile % g.tiles_y; const int b = tile / g.tiles_y;
    const int x0 = tx * 16, y0 = ty * ROWS, n0 = tn * BN + wn * (FN * 16);

    char* patch = smem;
    float* stage = reinterpret_cast<float*>(smem + SM::main_bytes + wave * SM::stage_bytes);

    f32x4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // BN scale / shift of this lane's output columns: in flight during the whole K loop
    float sc[FN], sh[FN];
#pragma unroll
    for (int j = 0; j < FN; ++j) {
        sc[j] = ep.scale ? ep.scale[n0 + j * 16 + xl] : 1.f;
        sh[j] = ep.shift ? ep.shift[n0 + j * 16 + xl] : 0.f;
    }

    // lane's patch base: pixel column xl, K chunk kq of the wave's first step (wave wk starts at step wk of every tap)
    const char* abase = patch + xl * S * PS + kq * 16 + wk * 64;
    const uint32_t loff = (uint32_t)lane * 16u;
    const T* xb = x + (size_t)b * g.H * g.W * CT;

    for (int grp = 0; grp < NG; ++grp) {
        if (grp > 0) __syncthreads();                         // every wave is done reading the previous patch
        // ---- halo patch: 10 x 18 input pixels x CG channels, zero outside the image.  Branch-free: every lane loads from a CLAMPED (always
        // valid) address and the out-of-image chunks are zeroed by a select, so all of a lane's loads are in flight together (as exec-masked
        // branch diamonds the compiler serialised some of them behind `s_waitcnt vmcnt(0)`); 32-bit element offsets against the image base
        {
            constexpr int nchunks = PH * PW * CPP;
            constexpr int PU = (nchunks + NT - 1) / NT < 12 ? (nchunks + NT - 1) / NT : 12;
            const T* xg = xb + grp * CG;
#pragma unroll
            for (int base = 0; base < nchunks; base += NT * PU) {
                u32x4 pr[PU];
#pragma unroll
                for (int u = 0; u < PU; ++u) {
                    int idx = base + u * NT + tid;
                    if (base + u * NT + NT > nchunks) idx = idx < nchunks ? idx : nchunks - 1;
                    const int pix = idx / CPP, ch = idx % CPP;
                    const int py = pix / PW, px = pix - py * PW;
                    const int iy = y0 * S - 1 + py, ix = x0 * S - 1 + px;
                    const bool in = iy >= 0 && iy < g.H && ix >= 0 && ix < g.W;
                    const int cy = min(max(iy, 0), g.H - 1), cx = min(max(ix, 0), g.W - 1);
                    const u32x4 z = *reinterpret_cast<const u32x4*>(xg + (uint32_t)((cy * g.W + cx) * CT + ch * 8));
                    pr[u] = in ? z : u32x4{0u, 0u, 0u, 0u};
                }
#pragma unroll
                for (int u = 0; u < PU; ++u) {
                    const int idx = base + u * NT + tid;
                    if (base + u * NT + NT <= nchunks || idx < nchunks) *reinterpret_cast<u32x4*>(patch + (idx / CPP) * PS + (idx % CPP) * 16) = pr[u];
                }
            }
        }

        // wave-uniform base of this wave's weight fragments: fragment row n0/16, step (grp * KS + wk) of tap 0
        const char* wbase = reinterpret_cast<const char*>(wfm) + ((size_t)(n0 >> 4) * FSTEPS + grp * KS + wk) * 1024;
        // step m of this wave: q = m * WK (+ wk, folded into the bases) -> tap q / KS, K step q % KS inside the tap
        auto bload = [&](int m, u32x4 (&bf)[FN]) {
            const int q = m * WK, tap = q / KS, ks = q % KS;
            const int st = tap * (CT / 32) + ks;
#pragma unroll
            for (int j = 0; j < FN; ++j) bf[j] = *reinterpret_cast<const u32x4*>(wbase + ((size_t)j * FSTEPS + st) * 1024 + loff);
        };
        auto aread = [&](int m, int i) -> u32x4 {
            const int q = m * WK, tap = q / KS, ks = q % KS;
            const int th = tap / 3, tw = tap - th * 3;
            return *reinterpret_cast<const u32x4*>(abase + ((th + i * S) * PW + tw) * PS + ks * 64);
        };

        constexpr int RING = 3;
        u32x4 wb[RING][FN];
        bload(0, wb[0]);
        if (NL > 1) bload(1, wb[1]);
        __syncthreads();                                      // patch visible to all waves

        u32x4 a0[HR], a1[HR];
#pragma unroll
        for (int i = 0; i < HR; ++i) a0[i] = aread(0, i);
#pragma unroll
        for (int m = 0; m < NL; ++m) {
            if (m + 2 < NL) bload(m + 2, wb[(m + 2) % RING]);
#pragma unroll
            for (int i = 0; i < HR; ++i) a1[i] = aread(m, HR + i);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < HR; ++i)
#pragma unroll
                for (int j = 0; j < FN; ++j) mma_chunk<T>(a0[i], wb[m % RING][j], acc[i][j]);
            __builtin_amdgcn_sched_barrier(0);
            if (m + 1 < NL) {
#pragma unroll
                for (int i = 0; i < HR; ++i) a0[i] = aread(m + 1, i);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < HR; ++i)
#pragma unroll
                for (int j = 0; j < FN; ++j) mma_chunk<T>(a1[i], wb[m % RING][j], acc[HR + i][j]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    // ---- K-split: partial accumulators -> LDS (the patch is dead), wave wk sums and finishes rows wk*RW .. +RW
    constexpr int RW = FM / WK;
    if constexpr (WK > 1) {
        __syncthreads();
        f32x4* red = reinterpret_cast<f32x4*>(smem);
#pragma unroll
        for (int dst = 0; dst < WK; ++dst) {
            if (dst == wk) continue;
            const int slot = wk < dst ? wk : wk - 1;
#pragma unroll
            for (int r = 0; r < RW; ++r)
#pragma unroll
                for (int j = 0; j < FN; ++j)
                    red[((((wn * WK + dst) * (WK - 1) + slot) * RW + r) * FN + j) * 64 + lane] = acc[dst * RW + r][j];
        }
        __syncthreads();
        f32x4 own[RW][FN];
#pragma unroll
        for (int r = 0; r < RW; ++r)
#pragma unroll
            for (int j = 0; j < FN; ++j) {
                f32x4 t = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int q = 0; q < WK; ++q) if (q == wk) t = acc[q * RW + r][j];
#pragma unroll
                for (int slot = 0; slot < WK - 1; ++slot) t += red[((((wn * WK + wk) * (WK - 1) + slot) * RW + r) * FN + j) * 64 + lane];
                own[r][j] = t;
            }
#pragma unroll
        for (int r = 0; r < RW; ++r)
#pragma unroll
            for (int j = 0; j < FN; ++j) acc[r][j] = own[r][j];
    }

    // ---- epilogue, wave-private: accumulator row-fragment -> stage -> 16-byte stores (conv_halo.hip's arithmetic, bit for bit).
    // The residual chunks of ALL the wave's rows are fetched up front (the K loop's fragment registers are dead by now, so they cost no
    // occupancy): one exposed memory round trip per tile instead of one per output row; 32-bit element offsets.
    constexpr int LDS_ = SM::stage_ld;
    constexpr int OE = ElemTraits<TO>::ELEMS;                 // output elements per 16-byte store: 8 (16-bit maps) / 4 (fp32: the DCN offset / mask conv)
    constexpr int GPR = FN * 16 / OE;
    constexpr int RITEMS = (16 * GPR + 63) / 64;
    constexpr bool kRes = std::is_same<T, TO>::value;         // residual operand: same type as the output (the launcher rejects the other case)
    const T* res = kRes ? reinterpret_cast<const T*>(ep.res) : nullptr;
    TO* y = reinterpret_cast<TO*>(ep.y);
    const uint32_t pix0 = (uint32_t)((b * g.Ho + y0) * g.Wo + x0);            // first pixel of the tile (32-bit: M * ld < 2^31 checked by the launcher)
    f32x2 st_s[FN], st_q[FN];
#pragma unroll
    for (int j = 0; j < FN; ++j) { st_s[j] = f32x2{0.f, 0.f}; st_q[j] = f32x2{0.f, 0.f}; }
    u32x4 rres[RW][RITEMS];
    if (res) {
#pragma unroll
        for (int ii = 0; ii < RW; ++ii) {
            const int i = WK > 1 ? wk * RW + ii : ii;
#pragma unroll
            for (int q = 0; q < RITEMS; ++q) {
                const int it = q * 64 + lane;
                const int px = it / GPR, ng = it - px * GPR;
                const bool ok = (16 * GPR % 64 == 0 || it < 16 * GPR) && y0 + i < g.Ho && x0 + px < g.Wo && n0 + ng * OE < ep.Cout;
                u32x4 z = {0u, 0u, 0u, 0u};
                if (ok) z = *reinterpret_cast<const u32x4*>(res + (pix0 + (uint32_t)(i * g.Wo + px)) * (uint32_t)ep.ldres + (uint32_t)(n0 + ng * OE));
                rres[ii][q] = z;
            }
        }
    }
#pragma unroll
    for (int ii = 0; ii < RW; ++ii) {
        const int i = WK > 1 ? wk * RW + ii : ii;
#pragma unroll
        for (int j = 0; j < FN; ++j) {
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = acc[ii][j][r] * sc[j] + sh[j];
                stage[((lane >> 4) * 4 + r) * LDS_ + j * 16 + xl] = v[r];
            }
            if constexpr (ST) {
                if (y0 + i < g.Ho) {                          // every lane sums its column over its pixels, of the values AS STORED
                    const int px = x0 + (lane >> 4) * 4;
#pragma unroll
                    for (int r = 0; r < 4; r += 2) {
                        f32x2 vr = {ElemTraits<TO>::round(v[r]), ElemTraits<TO>::round(v[r + 1])};
                        if (px + r + 1 >= g.Wo) { if (px + r >= g.Wo) vr[0] = 0.f; vr[1] = 0.f; }      // ragged right edge only
                        st_s[j] += vr; st_q[j] += vr * vr;
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int q = 0; q < RITEMS; ++q) {
            const int it = q * 64 + lane;
            const int px = it / GPR, ng = it - px * GPR;
            const int gn = n0 + ng * OE;
            const bool ok = (16 * GPR % 64 == 0 || it < 16 * GPR) && y0 + i < g.Ho && x0 + px < g.Wo && gn < ep.Cout;
            if (ok) {
                float v[OE];
#pragma unroll
                for (int e = 0; e < OE; e += 4) {
                    const f32x4 t = *reinterpret_cast<const f32x4*>(stage + px * LDS_ + ng * OE + e);
                    v[e] = t[0]; v[e + 1] = t[1]; v[e + 2] = t[2]; v[e + 3] = t[3];
                }
                if constexpr (kRes) {
                    if (res) {
                        float rv[OE];
                        ElemTraits<T>::unpack(rres[ii][q], rv);
#pragma unroll
                        for (int e = 0; e < OE; ++e) v[e] += rv[e];
                    }
                }
                apply_act_chunk<OE>(v, ep.act, gn);
                *reinterpret_cast<u32x4*>(y + (pix0 + (uint32_t)(i * g.Wo + px)) * (uint32_t)ep.ldy + (uint32_t)gn) = ElemTraits<TO>::pack(v);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    if constexpr (ST) {                                       // the four pixel groups of the wave meet by shuffles, lanes 0..15 add into the layer's scratch
        float* sp = ep.stats + (size_t)(blockIdx.x % ep.stats_ncopy) * 2 * ep.Cout;
#pragma unroll
        for (int j = 0; j < FN; ++j) {
            float a = st_s[j][0] + st_s[j][1], q = st_q[j][0] + st_q[j][1];
            a += __shfl_xor(a, 16); q += __shfl_xor(q, 16);
            a += __shfl_xor(a, 32); q += __shfl_xor(q, 32);
            const int n = n0 + j * 16 + xl;
            if (lane < 16 && n < ep.Cout) { unsafeAtomicAdd(sp + n, a); unsafeAtomicAdd(sp + ep.Cout + n, q); }
        }
    }
