// The body of the two F(4x4, 2x2) kernels, conv_wino42p_kernel (conv_wino42p.inc) and conv_wino42s_kernel (conv_wino42s.inc):
// included inside the kernel behind `typedef W42Kind<KIND> K;` (text, not a function: a wrapper changed the register allocation
// of conv_wino42p_kernel).  Mapping, wave placement (W42_ROLE_SIMD), staging scheme and epilogue are described in conv_wino42p.inc;
// the next-tile touch behind the K loop (K::PREFETCH, off in both kernels) below.
    constexpr int STEP_FLOATS = K::NSETS * W42_WAVE_FLOATS;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                       // [2][W42_CHUNK]; the epilogue's exchange buffers afterwards

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#if W42_ROLE_SIMD
    // waves land on SIMD wave % 4: SIMDs 0 / 1 carry the full-row wave, the column wave and row wave 0 of half 0 / 1 (13 MFMAs per K
    // step, two staging waves), SIMDs 2 / 3 the row waves 1 - 3 of half 0 / 1 (12 MFMAs, three staging waves)
    const int nbh = wave & 1;                               // column half
    const int wr = (wave & 2) ? (wave >> 2) + 1 : (wave < 4 ? 4 : (wave < 8 ? 5 : 0));     // role: 0..3 row wave xi = r + 1, 4 full-row wave xi = 0, 5 column wave
#else
    const int nbh = wave / 6, wr = wave - 6 * nbh;          // column half, role: 0..3 row wave xi = r + 1, 4 full-row wave xi = 0, 5 column wave
#endif
    const bool colw = wr == 5;
    const int xi = wr < 4 ? wr + 1 : (colw ? 1 : 0);         // plane row (the column wave: its first)
    const int fid = colw ? 5 : xi;                          // place in the epilogue's exchange: plane row, or 5
    const int l31 = lane & 31, h = lane >> 5;
    const ConvTileId T = conv_tile<W42_PW, W42_PH, K::PARITY_IN_Z>(P);         // KIND 2: z = output parity class (the kernels have no split-K form)
    const int nt_ = T.nt, py = T.py, px = T.px;
    const int n0 = nt_ * W42_BN + 32 * nbh;                 // first output column of this wave
    const int n = T.n, y0 = T.y0, x0 = T.x0;

    // staging item of this thread: (tile row sty, staged column shx, channel quad q); the row waves' threads take them in order
#if W42_ROLE_SIMD
    const int sidx = (wave - (wave > 5 ? 2 : 0)) * 64 + lane;      // the column waves are waves 4 and 5
#else
    const int sidx = (wave - (wave > 5 ? 1 : 0)) * 64 + lane;
#endif
    const int q = sidx & 3;
    const bool stager = !colw && sidx < W42_ITEMS;
    const int sit = stager ? sidx >> 2 : 0;
    const int sty = sit / W42_COLS, shx = sit - sty * W42_COLS;
    // source pixels of the item's five input rows: one base pixel + flags (W42Kind)
    unsigned spix1, sdst;
    {
        unsigned flags;
        K::item(P, T, sty, shx, spix1, flags);
        sdst = (unsigned)((4 * q) * W42_PLANE + sty * W42_ROWP + shx) | flags;      // + xi * 4 * W42_ROWP per result, + k * W42_PLANE per channel
    }

    const int nchunks = P.chunks_per_tap;
    const int nkb = nchunks * K::NPH;       // K blocks: (chunk, input parity phase)
    // the source of a chunk; inside the K loop scale / shift come from the LDS table (bn) and sc / sh are not loaded
    struct ChunkSrc : HaloSrc { const float2* bn; };
    float2* s_bn = reinterpret_cast<float2*>(As + 2 * W42_CHUNK + W4Stats::BYTES / sizeof(float));    // [padded input channel] (scale, shift), behind the float64 statistics scratch
    auto chunk_src = [&](int kb, bool in_loop) { return ChunkSrc{halo_src<K::NPH>(P, n, q, kb, !in_loop), s_bn + (kb / K::NPH) * BK + 4 * q}; };
    auto load_a = [&](const ChunkSrc& cs, int r) { return halo_load(cs, K::pixel(P, cs, spix1, sdst, r), q); };
    // BatchNorm + activation, the zero mask and the vertical transform of channel k of the quad, 5 LDS stores (one channel per K step)
    auto store_t1 = [&](const ChunkSrc& cs, const float4 (&v)[5], float* buf, auto KC, bool in_loop = false) {
        constexpr int k = decltype(KC)::value;
        float sc = k == 0 ? cs.sc.x : k == 1 ? cs.sc.y : k == 2 ? cs.sc.z : cs.sc.w;
        float sh = k == 0 ? cs.sh.x : k == 1 ? cs.sh.y : k == 2 ? cs.sh.z : cs.sh.w;
        if (in_loop) { const float2 t = cs.bn[k]; sc = t.x; sh = t.y; }
        const float mx = (sdst & (1u << 16)) ? 1.f : 0.f;
        const float m0 = (sdst & (1u << 14)) ? 0.f : mx, m4 = (sdst & (1u << 15)) ? 0.f : mx;
        float d[5], o[5];
#pragma unroll
        for (int r = 0; r < 5; r++) {
            const float x = k == 0 ? v[r].x : k == 1 ? v[r].y : k == 2 ? v[r].z : v[r].w;
            d[r] = normalize1(x, sc, sh, cs.act);
            if (K::ZERO_OUTSIDE) d[r] *= (r == 0 ? m0 : (r == 4 ? m4 : mx));
        }
        w42_bt(d, o);
        float* a = buf + (sdst & 0x3fffu) + k * W42_PLANE;
#pragma unroll
        for (int j = 0; j < 5; j++) a[j * 4 * W42_ROWP] = o[j];
    };

    // transformed weights of this column tile, class and half; the image carries W42_BDIST K steps of padding behind the last one,
    // so the look-ahead needs no clamp
    const __amdgpu_buffer_rsrc_t wrsrc = buffer_rsrc(P.weight_wino);
    const unsigned bvoff = (unsigned)(h * 32 + l31) * 16u;
    const unsigned bvoff_hi = 1024u + (unsigned)(h * 32 + l31) * 4u;
    unsigned bsoff = ((unsigned)nt_ * (unsigned)(nkb * 8 + W42_BDIST) * (unsigned)STEP_FLOATS +
                      (unsigned)(T.par * 2 + nbh) * (unsigned)W42_WAVE_FLOATS + (unsigned)(colw ? 1344 : wr * 256)) * 4u;
    struct BRegs { floatx4 lo; float hi; };

    const int ty = l31 >> 3, tx = l31 & 7;
    // T row of this lane's tile: channel 2 s + h, row (xi, ty), columns 4 tx .. 4 tx + 4 (the column wave: xi = 1, + 4 rows per plane row)
    const float* rcur = As + h * W42_PLANE + (xi * 4 + ty) * W42_ROWP + 4 * tx;
    const float* rnxt = rcur + W42_CHUNK;

    floatx16 acc[5];            // plane-row waves: [plane nu] (row waves: 0..3 in the K loop, 4 from the column wave afterwards); column wave: [plane row xi - 1]
#pragma unroll
    for (int p = 0; p < 5; p++)
#pragma unroll
        for (int g = 0; g < 16; g++) acc[p][g] = 0.0f;

    float* buf_cur = As;
    float* buf_nxt = As + W42_CHUNK;
    {
        const ChunkSrc cs = chunk_src(0, false);
        if (stager) {
            float4 v[5];
#pragma unroll
            for (int r = 0; r < 5; r++) v[r] = load_a(cs, r);
            store_t1(cs, v, buf_cur, std::integral_constant<int, 0>{});
            store_t1(cs, v, buf_cur, std::integral_constant<int, 1>{});
            store_t1(cs, v, buf_cur, std::integral_constant<int, 2>{});
            store_t1(cs, v, buf_cur, std::integral_constant<int, 3>{});
        }
    }
    {                       // the BatchNorm table of this view: every padded input channel of both sources
        const int ctot = nchunks * BK;
        for (int ch = tid; ch < ctot; ch += W42_THREADS) {
            const int sidx2 = ch < P.chunks0 * BK ? 0 : 1;
            const int cl = ch - (sidx2 ? P.chunks0 * BK : 0);
            float2 t = make_float2(1.f, 0.f);
            if (P.src_scale[sidx2]) t.x = P.src_scale[sidx2][(size_t)n * P.src_c[sidx2] + cl];
            if (P.src_shift[sidx2]) t.y = P.src_shift[sidx2][(size_t)n * P.src_c[sidx2] + cl];
            s_bn[ch] = t;
        }
    }

    // the K loop, instantiated per role
    auto k_loop = [&](auto ROLE) {
        constexpr int RL = decltype(ROLE)::value;   // 0 row wave, 1 full-row wave, 2 column wave
        constexpr bool CW = RL == 2;
        constexpr int NR = CW ? 4 : 1;              // row segments read per K step
        constexpr int NM = RL == 1 ? 5 : 4;         // MFMAs per K step
        auto load_b = [&](BRegs& dst) {             // the block of the K step W42_BDIST ahead
            dst.lo = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, (int)bvoff, (int)bsoff, 0));
            if (RL == 1) dst.hi = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(wrsrc, (int)bvoff_hi, (int)bsoff, 0));
            bsoff += (unsigned)(STEP_FLOATS * 4);
        };
        auto read_rows = [&](float (&d)[NR][5], const float* row, int s) {
#pragma unroll
            for (int j = 0; j < NR; j++) {
                const float* p = row + 2 * s * W42_PLANE + j * 4 * W42_ROWP;
                const float4 a = *reinterpret_cast<const float4*>(__builtin_assume_aligned(p, 16));
                d[j][0] = a.x; d[j][1] = a.y; d[j][2] = a.z; d[j][3] = a.w; d[j][4] = p[4];
            }
        };
        BRegs breg[4];
#pragma unroll
        for (int k = 0; k < W42_BDIST; k++) load_b(breg[k]);
        __syncthreads();                    // chunk 0 and the BatchNorm table are staged
        float raw[NR][5], V[5];
        read_rows(raw, rcur, 0);

        auto chunk_body = [&](auto NEXT, int c) {
            constexpr bool next_chunk = decltype(NEXT)::value;
            const ChunkSrc csn = chunk_src(next_chunk ? c + 1 : c, true);
            float4 avr[5];
#pragma unroll
            for (int s = 0; s < 8; s++) {
                // the next chunk's image is complete and nobody reads the buffer before the current one any more
                if (next_chunk && s == 7) __syncthreads();
                load_b(breg[(s + W42_BDIST) & 3]);
                // the horizontal half of the input transform
                if (CW) {
#pragma unroll
                    for (int j = 0; j < NR; j++) V[j] = w42_bt_row4(raw[j]);
                } else if (RL == 1) {
                    w42_bt(raw[0], V);
                } else {
                    w42_bt_rows03(raw[0], V);
                }
                if (s < 7) read_rows(raw, rcur, s + 1);
                else if (next_chunk) read_rows(raw, rnxt, 0);
                // the next chunk's input rows: requested in K steps 0 - 2, transformed and stored one channel of the quad per K step
                // in steps 3 - 6 (conv_wino4_kernel)
                if (!CW && next_chunk && stager) {
                    if (s == 0) { avr[0] = load_a(csn, 0); avr[1] = load_a(csn, 1); }
                    if (s == 1) { avr[2] = load_a(csn, 2); avr[3] = load_a(csn, 3); }
                    if (s == 2) avr[4] = load_a(csn, 4);
                }
#pragma unroll
                for (int p = 0; p < NM; p++) {
                    const float b = p < 4 ? breg[s & 3].lo[p] : breg[s & 3].hi;
                    acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(V[p], b, acc[p], 0, 0, 0);
                }
                if (!CW && next_chunk && stager) {
                    if (s == 3) store_t1(csn, avr, buf_nxt, std::integral_constant<int, 0>{}, true);
                    if (s == 4) store_t1(csn, avr, buf_nxt, std::integral_constant<int, 1>{}, true);
                    if (s == 5) store_t1(csn, avr, buf_nxt, std::integral_constant<int, 2>{}, true);
                    if (s == 6) store_t1(csn, avr, buf_nxt, std::integral_constant<int, 3>{}, true);
                }
#if W42_SGB > 0
                // one MFMA, then its share of the step's other work
#pragma unroll
                for (int p = 0; p < NM; p++) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // MFMA
                    if (CW) {
                        if (p < 1) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);      // VMEM read: the weight block
                        __builtin_amdgcn_sched_group_barrier(0x002, W42_SGB, 0);           // VALU
                        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                 // DS read: a row segment
                    } else {
                        const bool st_step = next_chunk && s >= 3 && s < 7;
                        if (p < (RL == 1 ? 2 : 1)) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);      // VMEM read: the weight block
                        if (next_chunk && s < 3 && p >= 2 && p < 4) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);     // ... and the input rows
                        if (st_step) __builtin_amdgcn_sched_group_barrier(0x002, W42_SGB_ST, 0);           // VALU, staging steps
                        else __builtin_amdgcn_sched_group_barrier(0x002, W42_SGB, 0);      // VALU
                        if (p >= 2) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);     // DS read
                        if (st_step) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);    // DS write (the staging stores)
                        if (st_step && p == 0) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
                    }
                }
#endif
            }
            const float* t = rcur; rcur = rnxt; rnxt = t;
            float* u = buf_cur; buf_cur = buf_nxt; buf_nxt = u;
        };
        for (int c = 0; c + 1 < nkb; c++) chunk_body(std::true_type{}, c);
        chunk_body(std::false_type{}, nkb - 1);
    };
    if (colw) k_loop(std::integral_constant<int, 2>{});
    else if (wr == 4) k_loop(std::integral_constant<int, 1>{});
    else k_loop(std::integral_constant<int, 0>{});

    // Next-tile touch (r10, conv_wino4_kernel's of r05).  One workgroup per CU: the first staged image of a tile is a cold read that
    // every CU asks for at the same moment, right behind the previous round's output stores.  The workgroup that holds the CU before
    // — block b - K::PREFETCH: blocks are handed out in order and block_coords gives an XCD consecutive ids, so it ran on the same XCD
    // = the same L2 — touches that image here, directly behind its K loop, so that the epilogue's LDS rounds cover the returns: one
    // pixel per thread (17 x 33 of the 768), W42_PF_TOUCH dwords of source 0's first chunk(s) each.  The successor's tile, view, class
    // and origin come from the decode it will run itself (conv_tile_of_block), par_inner order included.  The values are never used;
    // the registers stay pinned until the kernel ends so that a late return cannot land in a register given to something else.
    unsigned pf[W42_PF_TOUCH] = {};
    if constexpr (K::PREFETCH > 0) {
        const int b2 = (int)blockIdx.x + K::PREFETCH;
        const ConvParams Q = touch_params();
        if (b2 < Q.mtiles * Q.ntiles * Q.zdim && tid < W42_PF_ROWS * W42_COLS) {
            const ConvTileId T2 = conv_tile_of_block<W42_PW, W42_PH, K::PARITY_IN_Z>(Q, b2);
            const int hy = tid / W42_COLS, hx = tid - hy * W42_COLS;
            touch_pixel(Q, T2.n, K::first_image_pixel(Q, T2, hy, hx), pf);
        }
    }

    // ---- epilogue: Y = A^T M A per (tile, column), statistics, BatchNorm arrival, stores ----
    // C layout of a 32 x 32 block: column = lane % 32, row (= tile) = (g & 3) + 8 (g >> 2) + 4 h: tile row g >> 2, tile column
    // (g & 3) + 4 h.  The column wave hands plane (xi, 4) to row wave xi = 1..4
    __syncthreads();            // every wave is done with the T images
    if (colw) {
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int g = 0; g < 16; g++) As[((nbh * 4 + j) * 16 + g) * 64 + lane] = acc[j][g];
    }
    __syncthreads();
    // rr[g][b] = sum_nu A^T[b][nu] M[xi][nu]: the column combinations of a row wave's plane row
    float rr[16][4];
#pragma unroll
    for (int g = 0; g < 16; g++) {
        const float m4 = wr < 4 ? As[((nbh * 4 + xi - 1) * 16 + g) * 64 + lane] : acc[4][g];
        const float m[5] = {acc[0][g], acc[1][g], acc[2][g], acc[3][g], m4};
        w42_at(m, rr[g]);
    }
    // wave `fid` of a half finishes register rows [G0, G1): Y[a][b] = sum_xi A^T[a][xi] rr_xi[g][b] over the five plane rows
    constexpr int G0[6] = {0, 3, 6, 9, 12, 14}, G1[6] = {3, 6, 9, 12, 14, 16};
    float yv[3][4][4];                      // [row][a][b]; waves 4, 5 use two rows
    float2* xb = reinterpret_cast<float2*>(As);             // [row wave][<= 14 rows it does not finish][lane]
    const int wbase = nbh * 5;
    auto finish = [&](auto F) {
        constexpr int f = decltype(F)::value;
#pragma unroll
        for (int bp = 0; bp < 2; bp++) {    // output columns b = 2 bp, 2 bp + 1
            __syncthreads();        // round 0: every row wave has read its plane (xi, 4); round 1: the previous exchange is read
            if (f < 5) {
                int k = 0;
#pragma unroll
                for (int g = 0; g < 16; g++) {
                    if (g >= G0[f] && g < G1[f]) continue;
                    xb[((wbase + f) * 14 + k) * 64 + lane] = make_float2(rr[g][2 * bp], rr[g][2 * bp + 1]);
                    k++;
                }
            }
            __syncthreads();
#pragma unroll
            for (int g = G0[f]; g < G1[f]; g++) {
                float m0[5], m1[5];
#pragma unroll
                for (int o = 0; o < 5; o++) {
                    if (o == f) { m0[o] = rr[g][2 * bp]; m1[o] = rr[g][2 * bp + 1]; continue; }
                    // position of row g among the rows wave o does not finish
                    const int ko = g < G0[o] ? g : g - (G1[o] - G0[o]);
                    const float2 v = xb[((wbase + o) * 14 + ko) * 64 + lane];
                    m0[o] = v.x; m1[o] = v.y;
                }
                float c0[4], c1[4];
                w42_at(m0, c0); w42_at(m1, c1);
#pragma unroll
                for (int a = 0; a < 4; a++) { yv[g - G0[f]][a][2 * bp] = c0[a]; yv[g - G0[f]][a][2 * bp + 1] = c1[a]; }
            }
        }
    };
    if (fid == 0) finish(std::integral_constant<int, 0>{});
    else if (fid == 1) finish(std::integral_constant<int, 1>{});
    else if (fid == 2) finish(std::integral_constant<int, 2>{});
    else if (fid == 3) finish(std::integral_constant<int, 3>{});
    else if (fid == 4) finish(std::integral_constant<int, 4>{});
    else finish(std::integral_constant<int, 5>{});
    const int g0 = fid < 4 ? 3 * fid : 12 + 2 * (fid - 4), ng = fid < 4 ? 3 : 2;

    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++)
        if (k < ng)
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int b = 0; b < 4; b++) { const double v = yv[k][a][b]; s1 += v; s2 += v * v; }
    static_assert(W42_CHUNK % 2 == 0, "float64 scratch alignment");
    double* red = W4Stats::red(As + 2 * W42_CHUNK);         // behind the image / exchange buffers
    const bool with_stats = P.stats != nullptr;
    if (with_stats) {
        s1 += __shfl_xor(s1, 32, 64);
        s2 += __shfl_xor(s2, 32, 64);
        if (h == 0) {
            red[((6 * nbh + wr) * 32 + l31) * 2 + 0] = s1;      // slot: half, role (the sums' order does not depend on the placement)
            red[((6 * nbh + wr) * 32 + l31) * 2 + 1] = s2;
        }
        // the six waves of column half tid >> 5
        W4Stats::publish<W42_BN>(P, red, n, nt_ * W42_BN, tid, [tid](int j) { return (tid >> 5) * 6 + j; });
    }
    BnArrival arr = {nullptr, 0u};
    const bool bn = with_stats && P.arrive;
    if (bn) arr = bn_arrive(P, n, tid);
    {
        // register row g = tile row g >> 2, tile column (g & 3) + 4 h; outputs (4 ty + a, 4 tx + b) of the tile -> output pixels
        // (PIX (y0 + 4 ty + a) + py, PIX (x0 + 4 tx + b) + px): KIND 2 every other pixel of every other row, KIND 1 contiguous
        float* base = P.out + (((size_t)n * P.OH + K::PIX * y0 + py) * P.OW + K::PIX * x0 + px) * P.c_out_pad + n0;
        const ColumnStore<1, WINO_OUT_AUX> cst(P, base, n0, 0, l31, K::PIX * 16 * h);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            if (k >= ng) continue;
            const int g = g0 + k;
            const int tyr = g >> 2, txr = g & 3;
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int b = 0; b < 4; b++) cst.store(yv[k][a][b], 0, (unsigned)(K::PIX * ((4 * tyr + a) * P.OW + 4 * txr + b)));
        }
    }
    if (bn) bn_complete(P, arr, n, tid, W4Stats::flag(red));
    if constexpr (K::PREFETCH > 0) {
#pragma unroll
        for (int j = 0; j < W42_PF_TOUCH; j++) asm volatile("" :: "v"(pf[j]));
    }
