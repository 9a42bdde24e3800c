// Winograd F(4x4, 2x2) for the transposed 4x4 stride-2 convolution of the U-Net (KIND 2; descriptor flag RNR_CONV_WINOGRAD42),
// exact-fp32 operands on v_mfma_f32_32x32x2_f32.  Included by conv.hip behind conv_wino4.inc (its staging scheme, its BatchNorm
// table and statistics scratch; tile decode, halo source and column stores from conv_stage.inc).
//
// ConvTranspose2d 4x4 s2 p1 = four output parity classes (py, px), each a 2x2-tap correlation of the input (conv_wino2.inc):
//   out[2y + py][2x + px] = sum_{a,b in {0,1}} in[y + py - 1 + a][x + px - 1 + b] g_class[a][b]        (zero outside the map).
// The minimal algorithm F(4, 2) takes 5 multiplications for 4 outputs of a 2-tap filter; nested, 25 per 4 x 4 outputs of a class:
// 1.5625 per output against 2.25 for F(2x2, 2x2) and 4 for the direct form.  Interpolation points (0, 3/4, -3/4, 2, inf):
//   B^T d:  o0 = a2b d0 - a2 d1 - b d2 + d3,  o1 = d3 + (a - b) d2 - ab d1,  o2 = d3 - (a + b) d2 + ab d1,  o3 = d3 - a2 d1,
//           o4 = a2b d1 - a2 d2 - b d3 + d4                                                   (a = 3/4, b = 2, a2 = a^2)
//   A^T m:  y0 = m0 + m1 + m2 + m3,  y1 = a (m1 - m2) + b m3,  y2 = a2 (m1 + m2) + b^2 m3,  y3 = a^3 (m1 - m2) + b^3 m3 + m4
// (the record of the first, slower form of this kernel: profiles/archive/r04_wino42_transposed_ab.txt).
//
// Mapping.  A workgroup is 12 waves, three per SIMD, one workgroup per CU, and ALL TWELVE ISSUE MFMAs.  It owns 32 x 16
// positions of ONE parity class (= input pixels) = 32 tiles (8 x 4) of 4 x 4 outputs x 64 output columns: 25 planes (xi, nu) x 2
// column halves = 50 accumulator blocks of 32 x 32.  Wave w = 6 half + r:
//   r = 0..3  "row wave" xi = r + 1:  planes (xi, nu = 0..3) of its half — 4 blocks, 64 accumulator registers;
//   r = 4     "full-row wave" xi = 0: planes (0, nu = 0..4)            — 5 blocks, 80 accumulator registers;
//   r = 5     "column wave":          planes (xi = 1..4, nu = 4)       — 4 blocks, 64 accumulator registers.
// Ten waves x 4 + two waves x 5 = 50.  A wave whose planes share xi needs ONE row segment per K step and the column wave four,
// so the plane row that keeps its fifth plane is the price of one light wave more, and the column wave holds four blocks, not
// five.  Waves go to SIMD w % 4: each SIMD carries two row waves and one of the four special waves — 13 / 12 / 13 / 12 MFMAs
// per K step, the 13 on the SIMDs of the (light) full-row waves, the 12 on those of the (heavy) column waves (the first form
// of the kernel: 15 / 15 / 10 / 10).
//   * staging (no dedicated waves): as in conv_wino4_kernel the VERTICAL half of the input transform happens on the way into
//     LDS.  An item (tile row, column, channel quad) loads the five input rows 4 ty + py - 1 .. + 3 of its column (zero outside
//     the map, the producer's BatchNorm + activation applied), runs B^T down the column and stores T[xi]: image
//     [16 channels][xi][tile row][36], columns already shifted by px so that a tile's row segment is 16-byte aligned.  The 528
//     items of a chunk are spread over the threads of the row and full-row waves (the column waves, whose K step is the heaviest,
//     stage nothing): five loads requested in K steps 0 - 2 of the chunk before, one channel of the quad transformed and stored per K
//     step in steps 3 - 6;
//   * row wave, per K step: ONE row segment of 5 floats (ds_read_b128 + ds_read_b32), rows 0..3 of the horizontal B^T (8 VALU),
//     one buffer_load_dwordx4 of weights, 4 MFMAs; the full-row wave: all five rows of B^T (11 VALU), dwordx4 + dword, 5 MFMAs;
//   * column wave, per K step: the four row segments (xi = 1..4) of its tiles, row 4 of the horizontal B^T of each (12 VALU),
//     one buffer_load_dwordx4 of weights, 4 MFMAs;
//   * weights two K steps ahead in a ring of four blocks; image [column tile][K step][class][half][1600 floats: row wave r at
//     256 r as [lane][nu 0..3], the full-row wave at 1024 as [lane][nu 0..3] and at 1280 as [lane][nu = 4], the column wave at
//     1344 as [lane][xi 1..4]];
//   * epilogue: the column wave hands M[xi][4] to row wave xi through LDS; every plane-row wave then holds its whole plane row
//     and runs A^T over it (rr[g][b] = sum_nu A^T[b][nu] M[xi][nu]); the five plane rows of a half meet through LDS in two rounds
//     (two output columns b each) and ALL SIX waves of the half finish register rows (= tiles): plane-row wave xi rows
//     {0-2, 3-5, 6-8, 9-11, 12-13}[xi], the column wave, which reads all five plane rows, 14-15; class-strided stores (every other
//     pixel), statistics, BatchNorm arrival.
//
// Why one class per workgroup.  A class costs 50 blocks = 800 accumulator registers per lane over the workgroup; twelve waves at
// three per SIMD have 168 registers each (512 / 3), of which the K loop needs ~50 for operands, the weight ring and the staged
// loads: two classes (100 blocks, 133 - 144 registers per wave) or four (267) do not fit, and a 16-wave workgroup drops to two
// waves per SIMD.  Looping over the classes inside a K chunk would need all their accumulators at once.  So the four classes of
// a pixel tile stay four workgroups.  Where the input of a view is at least as large as the packed weights (conv_params'
// par_inner rule, written for the direct kernels' 16-tap image: L18 and L20 of the benchmark network) tile_coords makes them
// neighbours and the input comes from HBM once and from L2 three times; on L14 and L16 (4 / 16 MB of input per view against 33 /
// 17 MB of weights) the class is the slowest tile index: the workgroups in flight share one class's weights and the small input
// is re-read from L2 / MALL per class.  (The rule was left as it is: both orders were inside the layers' measured gain.)  The vertical transform of classes (py, 0) and (py, 1) is the same up to the one-column shift, but sharing it
// needs both classes' accumulators in one workgroup, which the register file rules out; halving the columns instead (2 classes
// x 32 columns) leaves the number of staged images per MFMA unchanged.  LDS: 2 x 16 x 724 floats of T images (92.7 KB) + the
// statistics scratch (6 KB) + the BatchNorm table (8 KB) = 107 KB of 160.

constexpr int W42_THREADS = 768;
constexpr int W42_PW = 32, W42_PH = 16;             // class positions (= input pixels) per workgroup tile
constexpr int W42_COLS = W42_PW + 1;                // staged columns (33)
constexpr int W42_ROWP = 36;                        // floats per T row
constexpr int W42_PLANE = 20 * W42_ROWP + 4;        // floats per channel plane: [xi (5)][ty (4)] rows (+ 4: bank spread of the staging stores)
constexpr int W42_CHUNK = BK * W42_PLANE;           // floats per staged K block
constexpr int W42_ITEMS = 4 * W42_COLS * 4;         // staging items per chunk: (tile row, column, channel quad) = 528
constexpr int W42_BN = 64;
#ifndef W42_BDIST_K
#define W42_BDIST_K 2
#endif
constexpr int W42_BDIST = W42_BDIST_K;              // K steps between the request of a weight block and its MFMAs (ring of 4: at most 3)
constexpr int W42_WAVE_FLOATS = 5 * 256 + 320;      // weight floats of the six waves of a (class, half) per K step
constexpr int W42_STEP_FLOATS = 4 * 2 * W42_WAVE_FLOATS;    // weight image per (column tile, K step): [class][half][1600]
constexpr int W42_XM4 = 8 * 16 * 64;                // floats of the nu = 4 hand-off: [half][xi - 1][register row][lane]
constexpr int W42_XCHG = 10 * 14 * 64 * 2;          // floats of one exchange round: [row wave][<= 14 register rows it does not finish][lane][2]
#ifndef W42_SGB
#define W42_SGB 6                   // VALU instructions behind each MFMA in the scheduling pipeline of a K step (0 / 3 / 4 / 6 / 8 / 12: within 1 %, profiles/r07_wino42p_ab.txt)
#endif
#ifndef W42_SGB_ST
#define W42_SGB_ST 14               // ... in the K steps that also stage one channel of the next chunk
#endif
static_assert(W42_ITEMS <= 10 * 64, "one staging item per thread of the row waves");
static_assert(2 * W42_CHUNK >= W42_XCHG && 2 * W42_CHUNK >= W42_XM4, "the exchange buffers of the epilogue live in the T buffers");
static_assert(W42_CHUNK < (1 << 14), "the staging destination is packed into 14 bits");
constexpr float W42_A = 0.75f, W42_B = 2.0f, W42_A2 = 0.5625f, W42_A3 = 0.421875f, W42_AB = 1.5f, W42_A2B = 1.125f;

__host__ __device__ constexpr size_t wino42p_lds_bytes() {
    return (size_t)(2 * W42_CHUNK + 2 * W4_BN_MAXC) * sizeof(float) + W4Stats::BYTES;
}

// B^T applied to five values: all five rows (the vertical half, at staging time), rows 0..3 (row waves), row 4 (column waves)
__device__ __forceinline__ void w42_bt(const float (&d)[5], float (&o)[5]) {
    o[0] = __builtin_fmaf(W42_A2B, d[0], __builtin_fmaf(-W42_A2, d[1], __builtin_fmaf(-W42_B, d[2], d[3])));
    o[1] = __builtin_fmaf(W42_A - W42_B, d[2], __builtin_fmaf(-W42_AB, d[1], d[3]));
    o[2] = __builtin_fmaf(-(W42_A + W42_B), d[2], __builtin_fmaf(W42_AB, d[1], d[3]));
    o[3] = __builtin_fmaf(-W42_A2, d[1], d[3]);
    o[4] = __builtin_fmaf(W42_A2B, d[1], __builtin_fmaf(-W42_A2, d[2], __builtin_fmaf(-W42_B, d[3], d[4])));
}
__device__ __forceinline__ void w42_bt_rows03(const float (&d)[5], float (&o)[5]) {
    o[0] = __builtin_fmaf(W42_A2B, d[0], __builtin_fmaf(-W42_A2, d[1], __builtin_fmaf(-W42_B, d[2], d[3])));
    o[1] = __builtin_fmaf(W42_A - W42_B, d[2], __builtin_fmaf(-W42_AB, d[1], d[3]));
    o[2] = __builtin_fmaf(-(W42_A + W42_B), d[2], __builtin_fmaf(W42_AB, d[1], d[3]));
    o[3] = __builtin_fmaf(-W42_A2, d[1], d[3]);
}
__device__ __forceinline__ float w42_bt_row4(const float (&d)[5]) {
    return __builtin_fmaf(W42_A2B, d[1], __builtin_fmaf(-W42_A2, d[2], __builtin_fmaf(-W42_B, d[3], d[4])));
}
// A^T applied to five values
__device__ __forceinline__ void w42_at(const float (&m)[5], float (&y)[4]) {
    const float s = m[1] + m[2], t = m[1] - m[2];
    y[0] = (m[0] + s) + m[3];
    y[1] = __builtin_fmaf(W42_A, t, W42_B * m[3]);
    y[2] = __builtin_fmaf(W42_A2, s, (W42_B * W42_B) * m[3]);
    y[3] = __builtin_fmaf(W42_A3, t, __builtin_fmaf(W42_B * W42_B * W42_B, m[3], m[4]));
}

__global__ void __launch_bounds__(W42_THREADS)
conv_wino42p_kernel(const ConvParams P) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                       // [2][W42_CHUNK]; the epilogue's exchange buffers afterwards

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nbh = wave / 6, wr = wave - 6 * nbh;          // column half, role: 0..3 row wave xi = r + 1, 4 full-row wave xi = 0, 5 column wave
    const bool colw = wr == 5;
    const int xi = wr < 4 ? wr + 1 : (colw ? 1 : 0);         // plane row (the column wave: its first)
    const int fid = colw ? 5 : xi;                          // place in the epilogue's exchange: plane row, or 5
    const int l31 = lane & 31, h = lane >> 5;
    const ConvTileId T = conv_tile<W42_PW, W42_PH, true>(P);           // z = output parity class (the kernel has no split-K form)
    const int nt_ = T.nt, py = T.py, px = T.px;
    const int n0 = nt_ * W42_BN + 32 * nbh;                 // first output column of this wave
    const int n = T.n, y0 = T.y0, x0 = T.x0;

    // staging item of this thread: (tile row sty, staged column shx, channel quad q); the row waves' threads take them in order
    const int sidx = (wave - (wave > 5 ? 1 : 0)) * 64 + lane;
    const int q = sidx & 3;
    const bool stager = !colw && sidx < W42_ITEMS;
    const int sit = stager ? sidx >> 2 : 0;
    const int sty = sit / W42_COLS, shx = sit - sty * W42_COLS;
    // source pixels of the five input rows ya - 1 .. ya + 3 of column x0 + px - 1 + shx, as one base pixel + flags.  Rows 1 .. 3 of
    // an item (ya .. ya + 2) always lie inside the map; row 0 falls off the top for the first tile row of class py = 0, row 4 off
    // the bottom for the last of py = 1, the column off either side at the map's edge: the clamped pixel is fetched and the
    // value replaced by exactly 0 (mask), not act(shift)
    unsigned spix1, sdst;
    {
        const int ix = x0 + px - 1 + shx;
        const int ya = y0 + 4 * sty + py;
        spix1 = (unsigned)(ya * P.W + min(max(ix, 0), P.W - 1));
        const unsigned flags = (ya - 1 < 0 ? 1u << 14 : 0u) | (ya + 3 >= P.H ? 1u << 15 : 0u) | (ix >= 0 && ix < P.W ? 1u << 16 : 0u);
        sdst = (unsigned)((4 * q) * W42_PLANE + sty * W42_ROWP + shx) | flags;      // + xi * 4 * W42_ROWP per result, + k * W42_PLANE per channel
    }
    auto spix_of = [&](int r) {
        if (r == 0) return (sdst & (1u << 14)) ? spix1 : spix1 - (unsigned)P.W;
        if (r == 4) return (sdst & (1u << 15)) ? spix1 + 2u * (unsigned)P.W : spix1 + 3u * (unsigned)P.W;
        return spix1 + (unsigned)((r - 1) * P.W);
    };

    const int nchunks = P.chunks_per_tap;
    // the source of a chunk; inside the K loop scale / shift come from the LDS table (bn) and sc / sh are not loaded
    struct ChunkSrc : HaloSrc { const float2* bn; };
    float2* s_bn = reinterpret_cast<float2*>(As + 2 * W42_CHUNK + W4Stats::BYTES / sizeof(float));    // [padded input channel] (scale, shift), behind the float64 statistics scratch
    auto chunk_src = [&](int c, bool in_loop) { return ChunkSrc{halo_src<1>(P, n, q, c, !in_loop), s_bn + c * BK + 4 * q}; };
    auto load_a = [&](const ChunkSrc& cs, int r) { return halo_load(cs, spix_of(r), q); };
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
            d[r] = normalize1(x, sc, sh, cs.act) * (r == 0 ? m0 : (r == 4 ? m4 : mx));
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
    unsigned bsoff = ((unsigned)nt_ * (unsigned)(nchunks * 8 + W42_BDIST) * (unsigned)W42_STEP_FLOATS +
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
            bsoff += (unsigned)(W42_STEP_FLOATS * 4);
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
        for (int c = 0; c + 1 < nchunks; c++) chunk_body(std::true_type{}, c);
        chunk_body(std::false_type{}, nchunks - 1);
    };
    if (colw) k_loop(std::integral_constant<int, 2>{});
    else if (wr == 4) k_loop(std::integral_constant<int, 1>{});
    else k_loop(std::integral_constant<int, 0>{});

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
            red[(wave * 32 + l31) * 2 + 0] = s1;
            red[(wave * 32 + l31) * 2 + 1] = s2;
        }
        // the six waves of column half tid >> 5
        W4Stats::publish<W42_BN>(P, red, n, nt_ * W42_BN, tid, [tid](int j) { return (tid >> 5) * 6 + j; });
    }
    BnArrival arr = {nullptr, 0u};
    const bool bn = with_stats && P.arrive;
    if (bn) arr = bn_arrive(P, n, tid);
    {
        // register row g = tile row g >> 2, tile column (g & 3) + 4 h; class outputs (4 ty + a, 4 tx + b) of the tile -> output
        // pixels (2 (y0 + 4 ty + a) + py, 2 (x0 + 4 tx + b) + px): every other pixel of every other row
        float* base = P.out + (((size_t)n * P.OH + 2 * y0 + py) * P.OW + 2 * x0 + px) * P.c_out_pad + n0;
        const ColumnStore<1, WINO_OUT_AUX> cst(P, base, n0, 0, l31, 2 * 16 * h);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            if (k >= ng) continue;
            const int g = g0 + k;
            const int tyr = g >> 2, txr = g & 3;
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int b = 0; b < 4; b++) cst.store(yv[k][a][b], 0, (unsigned)(2 * ((4 * tyr + a) * P.OW + 4 * txr + b)));
        }
    }
    if (bn) bn_complete(P, arr, n, tid, W4Stats::flag(red));
}

// Transformed weights U = G g G^T of the 2x2-tap correlation g of a parity class (taps in increasing input row / column, as
// w2_weight) for the points (0, a, -a, b, inf): G[j] = (1, p_j) / prod_{k != j} (p_j - p_k), G[inf] = (0, 1); float64, rounded
// once.  i enumerates [64-column tile][K step][class][half][1600]: [row wave xi = 1..4][lane = h * 32 + column][nu 0..3], the
// full-row wave's (xi = 0) [lane][nu 0..3] and [lane][nu = 4], then the column wave's [lane][xi 1..4] of plane column nu = 4.  K step = chunk * 8 + s holds the padded input channels
// chunk * 16 + 2 s + h; the W42_BDIST K steps behind the last one are zeros.
__global__ void __launch_bounds__(256)
pack_weight_wino42p_kernel(rnr_conv_desc d, const float* __restrict__ w, float* __restrict__ image, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int nsteps = (d.c_in0_pad + d.c_in1_pad) / 2;
    const int wb = (int)(i % W42_WAVE_FLOATS);
    long r = i / W42_WAVE_FLOATS;
    int ln, xi, nu;
    if (wb < 1024) { xi = (wb >> 8) + 1; ln = (wb & 255) >> 2; nu = wb & 3; }
    else if (wb < 1280) { xi = 0; ln = (wb - 1024) >> 2; nu = wb & 3; }
    else if (wb < 1344) { xi = 0; ln = wb - 1280; nu = 4; }
    else { ln = (wb - 1344) >> 2; xi = ((wb - 1344) & 3) + 1; nu = 4; }
    const int col = ln & 31, hh = ln >> 5;
    const int nb = (int)(r & 1); r >>= 1;
    const int cls = (int)(r & 3); r >>= 2;
    const int step = (int)(r % (nsteps + W42_BDIST));
    const int nt = (int)(r / (nsteps + W42_BDIST));
    if (step >= nsteps) { image[i] = 0.0f; return; }
    const int c = (step >> 3) * 16 + 2 * (step & 7) + hh;
    const int co = nt * W42_BN + nb * 32 + col;
    const double pts[4] = {0.0, 0.75, -0.75, 2.0};
    double G[5][2];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        double den = 1.0;
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k != j) den *= pts[j] - pts[k];
        G[j][0] = 1.0 / den; G[j][1] = pts[j] / den;
    }
    G[4][0] = 0.0; G[4][1] = 1.0;
    double g[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) g[a][b] = (double)gemm_weight(d, w, cls, (1 - a) * 2 + (1 - b), c, co);
    double u = 0.0;
#pragma unroll
    for (int b = 0; b < 2; b++) u += (G[xi][0] * g[0][b] + G[xi][1] * g[1][b]) * G[nu][b];
    image[i] = (float)u;
}

static void launch_wino42p(const dim3 grid, const ConvParams& P, hipStream_t st) {
    static bool attr_set = false;
    if (!attr_set) {         // > 64 KiB of dynamic LDS needs the opt-in
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_wino42p_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)wino42p_lds_bytes());
        attr_set = true;
    }
    hipLaunchKernelGGL(conv_wino42p_kernel, grid, dim3(W42_THREADS), wino42p_lds_bytes(), st, P);
}
