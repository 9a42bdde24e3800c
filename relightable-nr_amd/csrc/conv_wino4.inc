// Winograd F(4x4, 3x3) for the 3x3 convolutions of the U-Net (descriptor flag RNR_CONV_WINOGRAD4: the default of UNetPlan / RNRPipeline since r04, conv_algo = 'winograd4'), exact-fp32 operands on
// v_mfma_f32_32x32x2_f32.  Included by conv.hip behind conv_wino2.inc (same helpers, same epilogue building blocks).
//
//   Y = A^T [ sum_c (G g_c G^T) .* (B^T d_c B) ] A      with the 6 interpolation points (0, 3/4, -3/4, 3/2, -3/2, inf)
//
// A 4 x 4 output tile costs 36 multiplications per (input channel, output channel) instead of 144: 2.25 per output against
// 4 for F(2x2, 3x3) and 9 for the direct form.  The point set is the one a float32 study of the U-Net's layer shapes
// favours (scripts/experiments/winograd_accuracy_study.py: rms error 4.5 x the direct form's against 9 x for Lavin & Gray's
// (0, +-1, +-2), 3.5 x the shipped F(2x2, 3x3)); it is symmetric, so the 1-D transforms keep the 12-operation form:
//   B^T d:  p = d4 - b2 d2, q = d3 - b2 d1, r = d4 - a2 d2, s = d3 - a2 d1        (a = 3/4, b = 3/2, a2 = a^2, b2 = b^2)
//           o0 = a2 b2 d0 - (a2 + b2) d2 + d4,  o1 = p + a q,  o2 = p - a q,  o3 = r + b s,  o4 = r - b s,
//           o5 = a2 b2 d1 - (a2 + b2) d3 + d5
//   A^T m:  y0 = m0 + (m1 + m2) + (m3 + m4),  y1 = a (m1 - m2) + b (m3 - m4),  y2 = a2 (m1 + m2) + b2 (m3 + m4),
//           y3 = a^3 (m1 - m2) + b^3 (m3 - m4) + m5
// All constants are multiples of 2^-6.  G carries the Lagrange denominators (pack_weight_wino4_kernel, float64, rounded once).
//
// Mapping.  A workgroup is 12 waves (three per SIMD, one workgroup per CU) = 2 column halves x 6 plane rows xi.  It owns
// 32 x 16 output pixels = 32 tiles (8 x 4) x 64 output columns; wave (xi, nb) owns the six planes (xi, nu = 0..5) of all 32
// tiles for the 32 columns of half nb: six 32 x 32 accumulator blocks (96 registers).
//   * THE VERTICAL HALF OF THE INPUT TRANSFORM IS DONE AT STAGING TIME.  The staging threads do not copy the halo: an item
//     (tile row ty, halo column, channel quad) loads the six halo rows 4 ty .. 4 ty + 5 of its column (BatchNorm + activation
//     applied on the way, as in every kernel here), runs the 12-operation network down the column and stores the six results
//     T[xi] = sum_r B^T[xi][r] d[r] to LDS: image [16 channels][xi][ty][36] (34 columns used).  Per K step wave xi then reads
//     ONE row segment of 6 floats (ds_read_b128 + ds_read_b64), runs the horizontal network (12 VALU) and has the operands of
//     its six planes: 12 VALU + 2 LDS reads per 6 MFMAs, the same for every xi (combining the 3 - 4 halo rows per wave and K
//     step would cost 30 VALU + 8 LDS reads).  Price: the halo rows shared by vertically adjacent tiles are fetched 1.5 times
//     and an item carries 24 registers of loads in flight (requested in K steps 0 - 2 of the chunk before; the arithmetic and
//     the stores take one channel of the quad per K step in steps 3 - 6: done in a single step, the stager waves of a SIMD
//     are all on the vector ALU at once and its matrix pipe waits, 3 - 4 % of the kernel);
//   * weights: one buffer_load_dwordx4 + one dwordx2 per K step (6 planes x 2 channels of a column = 24 bytes per lane) from
//     the pre-transformed image [64-column tile][K step][xi][half][384 floats: lanes x planes 0..3, then lanes x planes 4, 5], two K steps ahead (r05; one in r04:
//     the third live block took the registers that the BatchNorm scale / shift quads and five of the six halo-row pixel
//     registers held — the former now come from an LDS table of the view, the latter are one base pixel + two flags);
//   * epilogue: A^T . A per wave over its planes' columns (r[b] = sum_nu A^T[b][nu] M[xi][nu]), the six plane rows of a
//     half meet through LDS in two rounds (two output columns b each), wave xi finishes the register rows {0-2, 3-5, 6-8,
//     9-11, 12-13, 14-15}[xi] (= tiles), statistics / BatchNorm arrival / stores as in conv_wino2_kernel.

constexpr int W4_THREADS = 768;
constexpr int W4_PW = 32, W4_PH = 16;               // output pixels per workgroup tile (8 x 4 tiles of 4 x 4)
constexpr int W4_HW = W4_PW + 2;                    // halo columns
constexpr int W4_ROWP = 36;                         // floats per T row (34 used; 16-byte aligned rows)
constexpr int W4_PLANE = 24 * W4_ROWP + 4;          // floats per channel plane: [xi][ty] rows (+ 4: 4 planes = 16 banks apart for the staging stores)
constexpr int W4_CHUNK = BK * W4_PLANE;             // floats per staged K block
constexpr int W4_ITEMS = 4 * W4_HW * 4;             // staging items per chunk: (tile row, halo column, channel quad) = 544
constexpr int W4_BN = 64;
#ifndef W4_SGB
#define W4_SGB 4                    // VALU instructions placed behind each MFMA by the scheduling pipeline of a K step (0 = the compiler's own order; r04: 3)
#endif
#ifndef W4_SGB_ST
#define W4_SGB_ST 8                 // ... in the K steps that also stage one channel of the next chunk (r04 A/B: 5 / 8 / 12 / 16 / 24 -> 12, profiles/archive/r04_wino_epilogue_ab.txt (8);
                                    // r05, with the weights two K steps ahead: 6 / 8 / 10 / 12 / 16 -> 8 with W4_SGB 4, -0.7 %, profiles/r05_wino4_ab.txt (4))
#endif
#ifndef W4_BDIST_K
#define W4_BDIST_K 2                // r05: 1 -> 2 (12 MFMAs of look-ahead) once the K loop had the registers for a third live block: L1 -1.8 %, L4 -1.2 %,
                                    // L6 / L8 -1.9 % (profiles/r05_wino4_ab.txt (4)); 3 spills 9 registers and loses 6 %
#endif
constexpr int W4_BDIST = W4_BDIST_K;                // K steps between the request of a weight block and its MFMAs (ring of 2 for 1, of 4 above)
constexpr int W4_BRING = W4_BDIST == 1 ? 2 : 4;
#ifndef W4_PREFETCH
#define W4_PREFETCH 256             // > 0: the epilogue touches the first halo image of block + W4_PREFETCH's tile (behind the K loop); 0: off
#endif
#ifndef W4_PF_TOUCH
#define W4_PF_TOUCH 2               // dwords touched per halo pixel, 128 bytes apart (profiles/r05_tile_prefetch_ab.txt: 1 / 2 / 4)
#endif
// (r05) the staging steps of the K loop read BatchNorm scale / shift of their channel from an LDS table (one ds_read_b64 per
// channel) instead of holding two float4 per thread across the chunk: 8 registers for the weight ring
constexpr int W4_BN_MAXC = 1024;                    // channels the table holds (both sources)
constexpr int W4_STEP_FLOATS = 6 * 2 * 2 * 32 * 6;  // weight image per (column tile, K step): [xi][half][h][32][6]
constexpr int W4_XCHG = 12 * 14 * 64 * 2;           // floats of one exchange round: [wave][<= 14 register rows it does not finish][lane][2]
static_assert(W4_ITEMS <= W4_THREADS, "one staging item per thread");
static_assert(2 * W4_CHUNK >= W4_XCHG, "the exchange buffer of the epilogue lives in the halo buffers");
constexpr float W4_A = 0.75f, W4_B = 1.5f, W4_A2 = 0.5625f, W4_B2 = 2.25f, W4_A3 = 0.421875f, W4_B3 = 3.375f;
constexpr float W4_A2B2 = 1.265625f, W4_A2PB2 = 2.8125f;

typedef StatScratch<12, 32> W4Stats;                // the statistics scratch: one slot per wave, 32 columns each

__host__ __device__ constexpr size_t wino4_lds_bytes() {
    return (size_t)(2 * W4_CHUNK + 2 * W4_BN_MAXC) * sizeof(float) + W4Stats::BYTES;
}

// B^T applied to six values (both directions of the input transform)
__device__ __forceinline__ void w4_bt(const float (&d)[6], float (&o)[6]) {
    const float p = __builtin_fmaf(-W4_B2, d[2], d[4]), q = __builtin_fmaf(-W4_B2, d[1], d[3]);
    const float r = __builtin_fmaf(-W4_A2, d[2], d[4]), s = __builtin_fmaf(-W4_A2, d[1], d[3]);
    o[0] = __builtin_fmaf(W4_A2B2, d[0], __builtin_fmaf(-W4_A2PB2, d[2], d[4]));
    o[1] = __builtin_fmaf(W4_A, q, p);
    o[2] = __builtin_fmaf(-W4_A, q, p);
    o[3] = __builtin_fmaf(W4_B, s, r);
    o[4] = __builtin_fmaf(-W4_B, s, r);
    o[5] = __builtin_fmaf(W4_A2B2, d[1], __builtin_fmaf(-W4_A2PB2, d[3], d[5]));
}
// A^T applied to six values
__device__ __forceinline__ void w4_at(const float (&m)[6], float (&y)[4]) {
    const float s1 = m[1] + m[2], d1 = m[1] - m[2], s2 = m[3] + m[4], d2 = m[3] - m[4];
    y[0] = m[0] + (s1 + s2);
    y[1] = __builtin_fmaf(W4_A, d1, W4_B * d2);
    y[2] = __builtin_fmaf(W4_A2, s1, W4_B2 * s2);
    y[3] = __builtin_fmaf(W4_A3, d1, __builtin_fmaf(W4_B3, d2, m[5]));
}

__global__ void __launch_bounds__(W4_THREADS)
conv_wino4_kernel(const ConvParams P) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                       // [2][W4_CHUNK]; the epilogue's exchange buffer afterwards

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nbh = wave / 6, xi = wave - 6 * nbh;          // column half, plane row
    const int l31 = lane & 31, h = lane >> 5;
    const ConvTileId T = conv_tile<W4_PW, W4_PH, false>(P);
    const int nt_ = T.nt, z_ = T.z;
    const int n0 = nt_ * W4_BN + 32 * nbh;                  // first output column of this wave
    const int n = T.n, y0 = T.y0, x0 = T.x0;

    // staging item of this thread: (tile row sty, halo column shx, channel quad q); threads past the items stage nothing
    const int q = tid & 3;
    const bool stager = tid < W4_ITEMS;
    const int sit = stager ? tid >> 2 : 0;
    const int sty = sit / W4_HW, shx = sit - sty * W4_HW;
    // source pixels of the six halo rows 4 sty - 1 + r of column x0 - 1 + shx, as one base pixel + two reflection flags (r05; six
    // halo-row pixel registers before).  Rows 1 .. 4 of an item are never reflected (4 sty .. 4 sty + 3 lie inside the map), so they
    // are spix1 + (r - 1) W; row 0 reflects to spix1 + W at the top border, row 5 to spix1 + 2 W at the bottom
    unsigned spix1, sflags;
    {
        const int ix = reflect1(x0 - 1 + shx, P.W);
        const int ya = y0 + 4 * sty;
        spix1 = (unsigned)(ya * P.W + ix);
        sflags = (ya == 0 ? 1u << 14 : 0u) | (ya + 4 >= P.H ? 1u << 15 : 0u);       // kept in the spare bits of sdst
    }
    auto spix_of = [&](int r, unsigned packed) {
        if (r == 0) return (packed & (1u << 14)) ? spix1 + (unsigned)P.W : spix1 - (unsigned)P.W;
        if (r == 5) return (packed & (1u << 15)) ? spix1 + 2u * (unsigned)P.W : spix1 + 4u * (unsigned)P.W;
        return spix1 + (unsigned)((r - 1) * P.W);
    };
    const unsigned sdst = (unsigned)((4 * q) * W4_PLANE + sty * W4_ROWP + shx) | sflags;      // + xi * 4 * W4_ROWP per result, + k * W4_PLANE per channel

    // split-K (small grids, e.g. the 128^2 / 64^2 layers at one view per call): slice z_ of P.splitk takes the chunks
    // [c_begin, c_end) and writes its partial outputs — the output transform is linear — to its own slab; splitk_reduce_kernel
    // adds the slabs and takes the statistics
    const int nchunks = P.chunks_per_tap;
    const int c_begin = T.c_begin, c_end = T.c_end;
    // the source of a chunk; inside the K loop scale / shift come from the LDS table (bn) and sc / sh are not loaded
    struct ChunkSrc : HaloSrc { const float2* bn; };
    float2* s_bn = reinterpret_cast<float2*>(As + 2 * W4_CHUNK + W4Stats::BYTES / sizeof(float));    // [padded input channel] (scale, shift), behind the float64 statistics scratch
    auto chunk_src = [&](int c, bool in_loop) { return ChunkSrc{halo_src<1>(P, n, q, c, !in_loop), s_bn + c * BK + 4 * q}; };
    auto load_a = [&](const ChunkSrc& cs, int r) {
        return halo_load(cs, spix_of(r, sdst), q);
    };
    // BatchNorm + activation and the vertical transform of channel k of the quad, 6 LDS stores (one channel per K step)
    auto store_t1 = [&](const ChunkSrc& cs, const float4 (&v)[6], float* buf, auto KC, bool in_loop = false) {
        constexpr int k = decltype(KC)::value;
        float sc = k == 0 ? cs.sc.x : k == 1 ? cs.sc.y : k == 2 ? cs.sc.z : cs.sc.w;
        float sh = k == 0 ? cs.sh.x : k == 1 ? cs.sh.y : k == 2 ? cs.sh.z : cs.sh.w;
        if (in_loop) { const float2 t = cs.bn[k]; sc = t.x; sh = t.y; }
        float d[6], o[6];
#pragma unroll
        for (int r = 0; r < 6; r++) {
            const float x = k == 0 ? v[r].x : k == 1 ? v[r].y : k == 2 ? v[r].z : v[r].w;
            d[r] = normalize1(x, sc, sh, cs.act);
        }
        w4_bt(d, o);
        float* a = buf + (sdst & 0x3fffu) + k * W4_PLANE;
#pragma unroll
        for (int j = 0; j < 6; j++) a[j * 4 * W4_ROWP] = o[j];
    };

    // transformed weights of this column tile: [K step][xi][half] blocks of 384 floats ([lane = h * 32 + column][planes 0..3], then [lane][planes 4, 5]); the image carries W4_BDIST K
    // steps of padding behind the last one, so the look-ahead needs no clamp
    const __amdgpu_buffer_rsrc_t wrsrc = buffer_rsrc(P.weight_wino);
    // the 1536-byte block of a wave and K step is [64 lanes][planes 0..3] then [64 lanes][planes 4, 5]: both loads of a K step read
    // consecutive lanes' consecutive bytes (8 + 4 cache lines instead of 12 + 12 at a lane stride of 24 bytes)
    const unsigned bvoff = (unsigned)(h * 32 + l31) * 16u;
    const unsigned bvoff_hi = 1024u + (unsigned)(h * 32 + l31) * 8u;
    unsigned bsoff = ((unsigned)nt_ * (unsigned)(nchunks * 8 + W4_BDIST) + (unsigned)(c_begin * 8)) * (unsigned)(W4_STEP_FLOATS * 4) +
                     (unsigned)((xi * 2 + nbh) * 2) * 768u;
    typedef float floatx2 __attribute__((ext_vector_type(2)));
    struct BRegs { floatx4 lo; floatx2 hi; };
    auto load_b = [&](BRegs& dst) {      // the next K step's block
        dst.lo = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, (int)bvoff, (int)bsoff, 0));
        dst.hi = __builtin_bit_cast(floatx2, __builtin_amdgcn_raw_buffer_load_b64(wrsrc, (int)bvoff_hi, (int)bsoff, 0));
        bsoff += (unsigned)(W4_STEP_FLOATS * 4);
    };

    // T row of this lane's tile: channel 2 s + h, row (xi, ty), columns 4 tx .. 4 tx + 5
    const int ty = l31 >> 3, tx = l31 & 7;
    const float* rcur = As + h * W4_PLANE + (xi * 4 + ty) * W4_ROWP + 4 * tx;
    const float* rnxt = rcur + W4_CHUNK;
    auto read_row = [&](float (&d)[6], const float* row, int s) {
        const float* p = row + 2 * s * W4_PLANE;
        const float4 a = *reinterpret_cast<const float4*>(__builtin_assume_aligned(p, 16));
        const float2 b = *reinterpret_cast<const float2*>(p + 4);
        d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w; d[4] = b.x; d[5] = b.y;
    };

    floatx16 acc[6];            // [plane nu]
#pragma unroll
    for (int p = 0; p < 6; p++)
#pragma unroll
        for (int g = 0; g < 16; g++) acc[p][g] = 0.0f;

    float* buf_cur = As;
    float* buf_nxt = As + W4_CHUNK;
    {
        const ChunkSrc cs = chunk_src(c_begin, false);
        if (stager) {
            float4 v[6];
#pragma unroll
            for (int r = 0; r < 6; r++) v[r] = load_a(cs, r);
            store_t1(cs, v, buf_cur, std::integral_constant<int, 0>{});
            store_t1(cs, v, buf_cur, std::integral_constant<int, 1>{});
            store_t1(cs, v, buf_cur, std::integral_constant<int, 2>{});
            store_t1(cs, v, buf_cur, std::integral_constant<int, 3>{});
        }
    }
    BRegs breg[W4_BRING];
#pragma unroll
    for (int k = 0; k < W4_BDIST; k++) load_b(breg[k]);
    {                       // the BatchNorm table of this view: every padded input channel of both sources
        const int ctot = nchunks * BK;
        for (int ch = tid; ch < ctot; ch += W4_THREADS) {
            const int sidx = ch < P.chunks0 * BK ? 0 : 1;
            const int cl = ch - (sidx ? P.chunks0 * BK : 0);
            float2 t = make_float2(1.f, 0.f);
            if (P.src_scale[sidx]) t.x = P.src_scale[sidx][(size_t)n * P.src_c[sidx] + cl];
            if (P.src_shift[sidx]) t.y = P.src_shift[sidx][(size_t)n * P.src_c[sidx] + cl];
            s_bn[ch] = t;
        }
    }
    __syncthreads();
    float raw[6], V[6];
    read_row(raw, rcur, 0);

    auto chunk_body = [&](auto NEXT, int c) {
        constexpr bool next_chunk = decltype(NEXT)::value;
        const ChunkSrc csn = chunk_src(next_chunk ? c + 1 : c, true);
        float4 avr[6];
#pragma unroll
        for (int s = 0; s < 8; s++) {
            // the next chunk's image is complete and nobody reads the buffer before the current one any more
            if (next_chunk && s == 7) __syncthreads();
            load_b(breg[(s + W4_BDIST) & (W4_BRING - 1)]);
            w4_bt(raw, V);                                   // the horizontal half of the input transform
            if (s < 7) read_row(raw, rcur, s + 1);
            else if (next_chunk) read_row(raw, rnxt, 0);
            // the next chunk's halo rows: requested in K steps 0 - 2, transformed and stored one channel of the quad per K step
            // in steps 3 - 6 (all of it in one step leaves the matrix pipe of a SIMD idle while its stager waves do it together)
            if (next_chunk && stager && s < 3) { avr[2 * s] = load_a(csn, 2 * s); avr[2 * s + 1] = load_a(csn, 2 * s + 1); }
#pragma unroll
            for (int p = 0; p < 6; p++) {
                const float b = p < 4 ? breg[s & (W4_BRING - 1)].lo[p] : breg[s & (W4_BRING - 1)].hi[p - 4];
                acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(V[p], b, acc[p], 0, 0, 0);
            }
            if (next_chunk && stager) {
                if (s == 3) store_t1(csn, avr, buf_nxt, std::integral_constant<int, 0>{}, true);
                if (s == 4) store_t1(csn, avr, buf_nxt, std::integral_constant<int, 1>{}, true);
                if (s == 5) store_t1(csn, avr, buf_nxt, std::integral_constant<int, 2>{}, true);
                if (s == 6) store_t1(csn, avr, buf_nxt, std::integral_constant<int, 3>{}, true);
            }
#if W4_SGB > 0
            // one MFMA, then its share of the step's other work, six times
#pragma unroll
            for (int p = 0; p < 6; p++) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // MFMA
                if (p < 3) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);      // VMEM read
                if (next_chunk && s >= 3 && s < 7) __builtin_amdgcn_sched_group_barrier(0x002, W4_SGB_ST, 0);       // VALU, staging steps
                else __builtin_amdgcn_sched_group_barrier(0x002, W4_SGB, 0);            // VALU
                if (p >= 4) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);     // DS read
                if (next_chunk && s >= 3 && s < 7) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);   // DS write (the staging stores)
            }
#endif
        }
        const float* t = rcur; rcur = rnxt; rnxt = t;
        float* u = buf_cur; buf_cur = buf_nxt; buf_nxt = u;
    };
    for (int c = c_begin; c + 1 < c_end; c++) chunk_body(std::true_type{}, c);
    chunk_body(std::false_type{}, c_end - 1);

#if W4_PREFETCH
    // Next-tile prefetch (r05).  One workgroup per CU: a workgroup's first halo image is a cold read that every CU of the chip asks for at the same
    // moment, right behind the previous round's output stores (2.3 - 2.7 us until it is back, profiles/r05_wino4_tile_timeline.txt).  The
    // workgroup that holds the CU before — block b - 256: the dispatcher hands blocks out in order and tile_coords gives an XCD consecutive
    // ids, so that block ran on the same XCD = the same L2 — touches that image while its own epilogue works on LDS and the vector ALU: one
    // dword per 128 bytes of a halo pixel's first chunk(s) pulls the lines into L2 / MALL.  The values are never used; the registers stay
    // pinned until the kernel ends so that a late return cannot land in a register the compiler has given to something else.
    unsigned pf[W4_PF_TOUCH] = {};
    {
        const int total = P.mtiles * P.ntiles * P.zdim;
        const int b2 = (int)blockIdx.x + W4_PREFETCH;
        if (b2 < total && tid < W4_HW * (W4_PH + 2)) {
            const int q8 = total >> 3, r8 = total & 7;      // tile_coords of block b2
            const int xcd = b2 & 7, idx = b2 >> 3;
            const int id = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
            const int t2 = id / P.ntiles;
            const int mt2 = t2 % P.mtiles, z2 = t2 / P.mtiles;
            int n2, y2, x2;
            tile_origin<W4_PW, W4_PH>(P, mt2, n2, y2, x2);
            const int hy = tid / W4_HW, hx = tid - hy * W4_HW;
            const int iy = min(max(y2 - 1 + hy, 0), P.H - 1), ix = min(max(x2 - 1 + hx, 0), P.W - 1);
            const int c2 = split_range(P, z2).begin;
            const int s2 = c2 < P.chunks0 ? 0 : 1;
            const unsigned C2 = (unsigned)P.src_c[s2];
            const __amdgpu_buffer_rsrc_t r2 = buffer_rsrc(P.src_data[s2] + (size_t)n2 * P.H * P.W * C2);
            const unsigned pix = (unsigned)(iy * P.W + ix) * C2 * 4u, cb = (unsigned)((c2 - (s2 ? P.chunks0 : 0)) * BK) * 4u;
#pragma unroll
            for (int j = 0; j < W4_PF_TOUCH; j++)
                pf[j] = __builtin_amdgcn_raw_buffer_load_b32(r2, (int)(pix + min(cb + 128u * j, C2 * 4u - 4u)), 0, 0);
        }
    }
#endif
    // ---- epilogue: Y = A^T M A per (tile, column), statistics, BatchNorm arrival, stores ----
    // C layout of a 32 x 32 block: column = lane % 32, row (= tile) = (g & 3) + 8 (g >> 2) + 4 h: tile row g >> 2, tile column
    // (g & 3) + 4 h.  rr[g][b] = sum_nu A^T[b][nu] M[xi][nu]: the column combinations of this wave's plane row
    float rr[16][4];
#pragma unroll
    for (int g = 0; g < 16; g++) {
        const float m[6] = {acc[0][g], acc[1][g], acc[2][g], acc[3][g], acc[4][g], acc[5][g]};
        w4_at(m, rr[g]);
    }
    // wave xi finishes register rows [G0, G1): Y[a][b] = sum_xi' A^T[a][xi'] rr_xi'[g][b] over the plane rows of its half
    constexpr int G0[6] = {0, 3, 6, 9, 12, 14}, G1[6] = {3, 6, 9, 12, 14, 16};
    float yv[3][4][4];                      // [row][a][b]; waves 4, 5 use two rows
    float2* xb = reinterpret_cast<float2*>(As);             // [wave][<= 14 rows it does not finish][lane]
    const int wbase = nbh * 6;
    auto finish = [&](auto F) {
        constexpr int f = decltype(F)::value;
#pragma unroll
        for (int bp = 0; bp < 2; bp++) {    // output columns b = 2 bp, 2 bp + 1
            __syncthreads();        // round 0: every wave is done with the T images; round 1: with the previous exchange
            int k = 0;
#pragma unroll
            for (int g = 0; g < 16; g++) {
                if (g >= G0[f] && g < G1[f]) continue;
                xb[((wbase + f) * 14 + k) * 64 + lane] = make_float2(rr[g][2 * bp], rr[g][2 * bp + 1]);
                k++;
            }
            __syncthreads();
#pragma unroll
            for (int g = G0[f]; g < G1[f]; g++) {
                float m0[6], m1[6];
#pragma unroll
                for (int o = 0; o < 6; o++) {
                    if (o == f) { m0[o] = rr[g][2 * bp]; m1[o] = rr[g][2 * bp + 1]; continue; }
                    // position of row g among the rows wave o does not finish
                    const int ko = g < G0[o] ? g : g - (G1[o] - G0[o]);
                    const float2 v = xb[((wbase + o) * 14 + ko) * 64 + lane];
                    m0[o] = v.x; m1[o] = v.y;
                }
                float c0[4], c1[4];
                w4_at(m0, c0); w4_at(m1, c1);
#pragma unroll
                for (int a = 0; a < 4; a++) { yv[g - G0[f]][a][2 * bp] = c0[a]; yv[g - G0[f]][a][2 * bp + 1] = c1[a]; }
            }
        }
    };
    if (xi == 0) finish(std::integral_constant<int, 0>{});
    else if (xi == 1) finish(std::integral_constant<int, 1>{});
    else if (xi == 2) finish(std::integral_constant<int, 2>{});
    else if (xi == 3) finish(std::integral_constant<int, 3>{});
    else if (xi == 4) finish(std::integral_constant<int, 4>{});
    else finish(std::integral_constant<int, 5>{});
    const int g0 = xi < 4 ? 3 * xi : 12 + 2 * (xi - 4), ng = xi < 4 ? 3 : 2;

    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++)
        if (k < ng)
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int b = 0; b < 4; b++) { const double v = yv[k][a][b]; s1 += v; s2 += v * v; }
    static_assert(W4_CHUNK % 2 == 0, "float64 scratch alignment");
    double* red = W4Stats::red(As + 2 * W4_CHUNK);         // behind the image / exchange buffers
    const bool with_stats = P.stats != nullptr && P.splitk == 1;
    if (with_stats) {
        s1 += __shfl_xor(s1, 32, 64);
        s2 += __shfl_xor(s2, 32, 64);
        if (h == 0) {
            red[(wave * 32 + l31) * 2 + 0] = s1;
            red[(wave * 32 + l31) * 2 + 1] = s2;
        }
        // the six plane-row waves of column half tid >> 5
        W4Stats::publish<W4_BN>(P, red, n, nt_ * W4_BN, tid, [tid](int j) { return (tid >> 5) * 6 + j; });
    }
    BnArrival arr = {nullptr, 0u};
    const bool bn = with_stats && P.arrive;
    if (bn) arr = bn_arrive(P, n, tid);
    {
        // register row g = tile row g >> 2, tile column (g & 3) + 4 h; outputs (4 ty + a, 4 tx + b) of the tile
        float* base = P.out + (size_t)z_ * P.slab_stride + (((size_t)n * P.OH + y0) * P.OW + x0) * P.c_out_pad + n0;
        const ColumnStore<1, WINO_OUT_AUX> cst(P, base, n0, 0, l31, 16 * h);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            if (k >= ng) continue;
            const int g = g0 + k;
            const int tyr = g >> 2, txr = g & 3;
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int b = 0; b < 4; b++) cst.store(yv[k][a][b], 0, (unsigned)((4 * tyr + a) * P.OW + 4 * txr + b));
        }
    }
    if (bn) bn_complete(P, arr, n, tid, W4Stats::flag(red));
#if W4_PREFETCH
#pragma unroll
    for (int j = 0; j < W4_PF_TOUCH; j++) asm volatile("" :: "v"(pf[j]));
#endif
}

// element (xi, nu) of U = G g G^T for input channel c (padded index) and output column co: float64, rounded once
__device__ __forceinline__ float w4_weight_u(const rnr_conv_desc& d, const float* __restrict__ w, int c, int co, int xi, int nu) {
    const double pts[5] = {0.0, 0.75, -0.75, 1.5, -1.5};
    double G[6][3];
#pragma unroll
    for (int j = 0; j < 5; j++) {
        double den = 1.0;
#pragma unroll
        for (int k = 0; k < 5; k++)
            if (k != j) den *= pts[j] - pts[k];
        G[j][0] = 1.0 / den; G[j][1] = pts[j] / den; G[j][2] = pts[j] * pts[j] / den;
    }
    G[5][0] = 0.0; G[5][1] = 0.0; G[5][2] = 1.0;
    double g[3][3];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) g[a][b] = (double)gemm_weight(d, w, 0, a * 3 + b, c, co);
    // row xi of G g, then column nu of (.) G^T
    double u = 0.0;
#pragma unroll
    for (int b = 0; b < 3; b++) {
        double row = 0.0;
#pragma unroll
        for (int a = 0; a < 3; a++) row += G[xi][a] * g[a][b];
        u += row * G[nu][b];
    }
    return (float)u;
}

// Transformed weights U = G g G^T for the points (0, a, -a, b, -b, inf): G[j] = (1, p_j, p_j^2) / prod_{k != j} (p_j - p_k),
// G[inf] = (0, 0, 1); computed in float64 and rounded once.  i enumerates
// [64-column tile][K step][xi][column half][h][32 columns][6 planes nu]; K step = chunk * 8 + s holds the padded input channels
// chunk * 16 + 2 s + h; the W4_BDIST K steps behind the last one are zeros.
__global__ void __launch_bounds__(256)
pack_weight_wino4_kernel(rnr_conv_desc d, const float* __restrict__ w, float* __restrict__ image, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int nsteps = (d.c_in0_pad + d.c_in1_pad) / 2;
    // block of a (K step, xi, column half): 384 floats
    const int wb = (int)(i % 384);
    long r = i / 384;
    // [64 lanes][planes 0..3], then [64 lanes][planes 4, 5]; lane = h * 32 + column
    const int ln = wb < 256 ? wb >> 2 : (wb - 256) >> 1;
    const int nu = wb < 256 ? wb & 3 : 4 + ((wb - 256) & 1);
    const int col = ln & 31, hh = ln >> 5;
    const int nb = (int)(r & 1); r >>= 1;
    const int xi = (int)(r % 6); r /= 6;
    const int step = (int)(r % (nsteps + W4_BDIST));
    const int nt = (int)(r / (nsteps + W4_BDIST));
    if (step >= nsteps) { image[i] = 0.0f; return; }
    const int c = (step >> 3) * 16 + 2 * (step & 7) + hh;
    const int co = nt * W4_BN + nb * 32 + col;
    image[i] = w4_weight_u(d, w, c, co, xi, nu);
}

static void launch_wino4(const dim3 grid, const ConvParams& P, hipStream_t st) {
    static bool attr_set = false;
    if (!attr_set) {         // > 64 KiB of dynamic LDS needs the opt-in
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_wino4_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)wino4_lds_bytes());
        attr_set = true;
    }
    hipLaunchKernelGGL(conv_wino4_kernel, grid, dim3(W4_THREADS), wino4_lds_bytes(), st, P);
}
