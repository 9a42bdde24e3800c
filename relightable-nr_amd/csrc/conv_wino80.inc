// Winograd F(2x2, 3x3) for the 3x3 OUT LAYER of the U-Net (78 output channels in 80 columns), exact-fp32 operands on
// v_mfma_f32_16x16x4_f32.  Included by conv.hip behind conv_wino.inc (same algorithm, helpers and software pipeline).
//
// 80 columns are 2.5 of the 32-column blocks conv_wino_kernel multiplies; on the 16 x 16 x 4 instruction (same FLOP rate,
// four input channels per MFMA) they are exactly five blocks.  A workgroup (4 waves, two to three workgroups per CU) owns
// 16 x 4 output pixels = 16 Winograd tiles (8 x 2) x 80 columns; wave xi owns plane row xi: 4 planes x 5 column blocks =
// twenty 16 x 16 accumulator blocks (80 registers).  Per K step of four input channels a wave issues 20 MFMAs (640
// matrix-pipe cycles) and
//   * A operands: an MFMA lane is (tile m = lane % 16, channel k = lane / 16) — one (tile, channel) pair: 4 ds_read_b64
//     (the two patch rows plane row xi combines) + 8 VALU give the four A operands, each used by five MFMAs;
//   * B operands: five lane-linear buffer_load_dwordx4 from the pre-transformed weight image
//     (pack_weight_wino80_kernel: [K step][xi][column block][k][16 columns][4 planes]), two K steps ahead;
//   * the halo of the chunk after next (18 x 6 pixels x 16 channels, two float4 per thread): global loads in the last two K
//     steps of a chunk, BatchNorm + activation + LDS stores in the first two of the next.
// Epilogue: as conv_wino_kernel — column combinations per wave, the four plane rows meet through LDS, wave f finishes
// accumulator register f of every block (4 tiles x 80 columns per wave).  Pixel tiles whose tile_mask is 0 are skipped
// (rnr_conv2d_masked: the ray renderer never reads background pixels).
//
// LDS halo image of a chunk: channel p at p * 160 + (p / 4) * 8 floats, [6 rows][24]: the 32 lanes of a ds_read_b64 group
// are 2 channels x 2 tile rows x 8 tile columns = four disjoint 16-word runs of the 64 banks.

constexpr int W80_PW = 16, W80_PH = 4;              // output pixels per workgroup tile
constexpr int W80_HW = W80_PW + 2, W80_HH = W80_PH + 2;
constexpr int W80_PLANE = 160;                      // floats per channel plane (6 x 24 = 144, padded to 32 mod 64)
constexpr int W80_CHUNK = 16 * W80_PLANE + 32;      // floats per chunk image (with the (p / 4) * 8 skew)
constexpr int W80_SLOTS = W80_HW * W80_HH * 4;      // 432 float4 slots
constexpr int W80_APT = (W80_SLOTS + CTHREADS - 1) / CTHREADS;      // 2
#ifndef W80_SGB
#define W80_SGB 2                   // VALU instructions behind each MFMA in the scheduling pipeline of a K step (0 = compiler's order: +14 %)
#endif
#ifndef W80_BDIST_K
#define W80_BDIST_K 3               // 2 -> 3 (r05, the whole ring of four in use): 3221 - 3238 -> 3190 us on the out layer at 16 views
#endif
constexpr int W80_BDIST = W80_BDIST_K;                        // K steps between the request of a weight block and its MFMAs
constexpr int W80_STEP_FLOATS = 4 * 5 * 4 * 16 * 4; // weight image per K step: [xi][block][k][16][4]
constexpr int W80_XCHG = 4 * 3 * 5 * 64 * 2;        // floats of the epilogue exchange: [finishing wave][source][block][lane][2]

__host__ __device__ constexpr int w80_plane_off(int p) { return p * W80_PLANE + (p >> 2) * 8; }
typedef StatScratch<4, 80> W80Stats;                // the statistics scratch: one slot per wave
__host__ __device__ constexpr size_t wino80_lds_bytes() {
    return (size_t)(2 * W80_CHUNK > W80_XCHG ? 2 * W80_CHUNK : W80_XCHG) * sizeof(float) + W80Stats::BYTES;
}

__global__ void __launch_bounds__(CTHREADS, 2)
conv_wino80_kernel(const ConvParams P) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                       // [2][W80_CHUNK]; the epilogue's exchange buffer afterwards

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int xi = __builtin_amdgcn_readfirstlane(tid >> 6);        // the wave's plane row
    const int l15 = lane & 15, kq = lane >> 4;
    const ConvTileId T = conv_tile<W80_PW, W80_PH, false>(P);   // one column tile, no split-K: mt alone counts
    const int n = T.n, y0 = T.y0, x0 = T.x0;
    if (P.tile_mask && P.tile_mask[T.mt] == 0) return;      // workgroup-uniform, before any barrier

    // halo slots of this thread (wrapped slots are staged twice: no predicate)
    const int q = tid & 3;
    unsigned spix[W80_APT];
    float* sd_cur[W80_APT];
    float* sd_nxt[W80_APT];
#pragma unroll
    for (int j = 0; j < W80_APT; j++) {
        int hy, hx;
        float m;
        halo_slot<W80_HW, W80_SLOTS, CTHREADS>(tid, j, hy, hx);
        spix[j] = halo_pixel<0>(P, y0, x0, hy, hx, m);
        sd_cur[j] = As + (4 * q) * W80_PLANE + q * 8 + hy * WINO_ROWP + hx;      // plane 4 q: w80_plane_off
        sd_nxt[j] = sd_cur[j] + W80_CHUNK;
    }

    const int nchunks = P.chunks_per_tap;
    auto chunk_src = [&](int c) { return halo_src<1>(P, n, q, c); };
    auto load_a = [&](const HaloSrc& cs, int j) { return halo_load(cs, spix[j], q); };
    auto store_a = [&](const HaloSrc& cs, float4 v, float* a) {
        const float4 u = normalize4<false>(cs, v);
        a[0] = u.x; a[W80_PLANE] = u.y; a[2 * W80_PLANE] = u.z; a[3 * W80_PLANE] = u.w;
    };

    // transformed weights: [K step][xi][column block][k][16 columns][4 planes]: lane-linear 1 KB per (xi, block)
    const __amdgpu_buffer_rsrc_t wrsrc = buffer_rsrc(P.weight_wino);
    const unsigned bvoff = (unsigned)lane * 16u;
    unsigned bsoff = (unsigned)xi * 5u * 1024u;
    struct BRegs { floatx4 b[5]; };
    auto load_b = [&](BRegs& dst) {      // the next K step's block
#pragma unroll
        for (int nbk = 0; nbk < 5; nbk++)
            dst.b[nbk] = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, (int)(bvoff + 1024u * nbk), (int)bsoff, 0));
        bsoff += (unsigned)(W80_STEP_FLOATS * 4);
    };

    // the two patch rows plane row xi combines, t = Ra + sigma Rc:  xi 0: d0 - d2, 1: d1 + d2, 2: d2 - d1, 3: d1 - d3
    const int ty = l15 >> 3, tx = l15 & 7;
    const int row_a = xi == 0 ? 0 : (xi == 2 ? 2 : 1), row_c = xi == 3 ? 3 : (xi == 2 ? 1 : 2);
    const float sigma = xi == 1 ? 1.0f : -1.0f;
    struct Rows { const float* a; const float* c; };
    Rows rcur, rnxt;
    rcur.a = As + kq * W80_PLANE + (2 * ty + row_a) * WINO_ROWP + 2 * tx;      // channel 4 s + kq: + s * (4 * W80_PLANE + 8)
    rcur.c = As + kq * W80_PLANE + (2 * ty + row_c) * WINO_ROWP + 2 * tx;
    rnxt.a = rcur.a + W80_CHUNK;
    rnxt.c = rcur.c + W80_CHUNK;
    auto read_patch = [&](float (&d)[8], const Rows& rows, int s) {
        const int xo = s * (4 * W80_PLANE + 8);
        const float2 a0 = *reinterpret_cast<const float2*>(rows.a + xo), a1 = *reinterpret_cast<const float2*>(rows.a + xo + 2);
        const float2 c0 = *reinterpret_cast<const float2*>(rows.c + xo), c1 = *reinterpret_cast<const float2*>(rows.c + xo + 2);
        d[0] = a0.x; d[1] = a0.y; d[2] = a1.x; d[3] = a1.y;
        d[4] = c0.x; d[5] = c0.y; d[6] = c1.x; d[7] = c1.y;
    };
    auto transform = [&](const float (&d)[8], float (&v)[4]) {
        float t[4];
#pragma unroll
        for (int j = 0; j < 4; j++) t[j] = __builtin_fmaf(sigma, d[4 + j], d[j]);
        v[0] = t[0] - t[2]; v[1] = t[1] + t[2]; v[2] = t[2] - t[1]; v[3] = t[1] - t[3];
    };

    floatx4 acc[4][5];          // [plane nu][column block]
#pragma unroll
    for (int p = 0; p < 4; p++)
#pragma unroll
        for (int b = 0; b < 5; b++) acc[p][b] = floatx4{0.f, 0.f, 0.f, 0.f};

    {
        const HaloSrc cs = chunk_src(0);
#pragma unroll
        for (int j = 0; j < W80_APT; j++) store_a(cs, load_a(cs, j), sd_cur[j]);
    }
    // the halo of chunk c + 1 is fetched during chunk c - 1 (its last two K steps) and stored during chunk c (its first two)
    HaloSrc cs_in = chunk_src(nchunks > 1 ? 1 : 0);
    float4 avr[W80_APT];
#pragma unroll
    for (int j = 0; j < W80_APT; j++) avr[j] = load_a(cs_in, j);
    BRegs breg[4];
#pragma unroll
    for (int k = 0; k < W80_BDIST; k++) load_b(breg[k]);
    __syncthreads();
    // software pipeline of a K step t: patch rows are read during step t - 2, transformed during step t - 1, multiplied in t
    float raw[2][8], V[2][4];
    read_patch(raw[0], rcur, 0);
    transform(raw[0], V[0]);
    read_patch(raw[1], rcur, 1);

    auto chunk_body = [&](auto NEXT, int c) {
        constexpr bool next_chunk = decltype(NEXT)::value;
        const HaloSrc cs_st = cs_in;                       // chunk c + 1: in flight since the previous chunk
        if (next_chunk) cs_in = chunk_src(c + 2 < nchunks ? c + 2 : c + 1);
#pragma unroll
        for (int s = 0; s < 4; s++) {
            // the next chunk's halo is complete and nobody reads the buffer before the current one any more
            if (next_chunk && s == 2) __syncthreads();
            load_b(breg[(s + W80_BDIST) & 3]);
            if (s < 2) read_patch(raw[s & 1], rcur, s + 2);
            else if (next_chunk) read_patch(raw[s & 1], rnxt, s - 2);
            if (next_chunk && s < W80_APT) store_a(cs_st, avr[s], sd_nxt[s]);
#pragma unroll
            for (int p = 0; p < 4; p++)
#pragma unroll
                for (int b = 0; b < 5; b++)
                    acc[p][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(V[s & 1][p], breg[s & 3].b[b][p], acc[p][b], 0, 0, 0);
            if (s < 3 || next_chunk) transform(raw[(s + 1) & 1], V[(s + 1) & 1]);
            if (next_chunk && s >= 2) avr[s - 2] = load_a(cs_in, s - 2);      // (past the last chunk: a harmless re-read)
#if W80_SGB > 0
            // one MFMA, then its share of the step's other work, twenty times
#pragma unroll
            for (int p = 0; p < 20; p++) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // MFMA
                if (p < 4) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);       // DS read
                if (p < 6) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);       // VMEM read
                __builtin_amdgcn_sched_group_barrier(0x002, W80_SGB, 0);            // VALU
                if (p >= 8 && p < 12) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);   // DS write
            }
#endif
        }
        const Rows t = rcur; rcur = rnxt; rnxt = t;
#pragma unroll
        for (int j = 0; j < W80_APT; j++) { float* u = sd_cur[j]; sd_cur[j] = sd_nxt[j]; sd_nxt[j] = u; }
    };
    for (int c = 0; c + 1 < nchunks; c++) chunk_body(std::true_type{}, c);
    chunk_body(std::false_type{}, nchunks - 1);

    // ---- epilogue: Y = A^T M A per (tile, column), statistics, BatchNorm arrival, stores ----
    // C layout of a 16 x 16 block: column = lane % 16, row (= tile) = 4 (lane / 16) + register.
    // rr[block][register] = the column combinations (r[b = 0], r[b = 1]) of this wave's plane row
    float2 rr[5][4];
#pragma unroll
    for (int b = 0; b < 5; b++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            rr[b][r].x = acc[0][b][r] + acc[1][b][r] + acc[2][b][r];
            rr[b][r].y = acc[1][b][r] - acc[2][b][r] - acc[3][b][r];
        }
    __syncthreads();            // every wave is done with the halo: LDS becomes the exchange buffer
    float2* xb = reinterpret_cast<float2*>(As);             // [finishing wave f][source slot][block][lane]
    // wave f finishes accumulator register f of every block: tile 4 (lane / 16) + f; the other three hand it their plane rows
    float2 y0v[5], y1v[5];
    auto exchange = [&](auto F) {
        constexpr int f = decltype(F)::value;
#pragma unroll
        for (int o = 0; o < 4; o++) {
            if (o == f) continue;
            const int slot = f < o ? f : f - 1;         // this wave's position among the sources of wave o
#pragma unroll
            for (int b = 0; b < 5; b++) xb[((o * 3 + slot) * 5 + b) * 64 + lane] = rr[b][o];
        }
        __syncthreads();
#pragma unroll
        for (int b = 0; b < 5; b++) {
            float2 R[4];
#pragma unroll
            for (int o = 0; o < 4; o++) {
                if (o == f) R[o] = rr[b][f];
                else R[o] = xb[((f * 3 + (o < f ? o : o - 1)) * 5 + b) * 64 + lane];
            }
            y0v[b] = make_float2(R[0].x + R[1].x + R[2].x, R[0].y + R[1].y + R[2].y);
            y1v[b] = make_float2(R[1].x - R[2].x - R[3].x, R[1].y - R[2].y - R[3].y);
        }
    };
    if (xi == 0) exchange(std::integral_constant<int, 0>{});
    else if (xi == 1) exchange(std::integral_constant<int, 1>{});
    else if (xi == 2) exchange(std::integral_constant<int, 2>{});
    else exchange(std::integral_constant<int, 3>{});

    static_assert((2 * W80_CHUNK > W80_XCHG ? 2 * W80_CHUNK : W80_XCHG) % 2 == 0, "float64 scratch alignment");
    double* red = W80Stats::red(As + (2 * W80_CHUNK > W80_XCHG ? 2 * W80_CHUNK : W80_XCHG));
    const bool with_stats = P.stats != nullptr;
    if (with_stats) {
#pragma unroll
        for (int b = 0; b < 5; b++) {
            const double p = y0v[b].x, q = y0v[b].y, r = y1v[b].x, t = y1v[b].y;
            double s1 = (p + q) + (r + t);
            double s2 = (p * p + q * q) + (r * r + t * t);
            s1 += __shfl_xor(s1, 16, 64); s2 += __shfl_xor(s2, 16, 64);
            s1 += __shfl_xor(s1, 32, 64); s2 += __shfl_xor(s2, 32, 64);
            if (kq == 0) {
                red[(xi * 80 + 16 * b + l15) * 2 + 0] = s1;
                red[(xi * 80 + 16 * b + l15) * 2 + 1] = s2;
            }
        }
        W80Stats::publish(P, red, n, 0, tid);
    }
    BnArrival arr = {nullptr, 0u};
    const bool bn = with_stats && P.arrive;
    if (bn) arr = bn_arrive(P, n, tid);
    {
        // this lane's tile for register xi: 4 kq + xi -> tile row kq >> 1, tile column 4 (kq & 1) + xi
        float* base = P.out + (((size_t)n * P.OH + y0) * P.OW + x0) * P.c_out_pad;
        // (not a ColumnStore: all 80 columns exist, there is no padding column to drop, and a column block is a byte offset)
        const __amdgpu_buffer_rsrc_t rsrc = buffer_rsrc(base);
        const unsigned cp4 = (unsigned)P.c_out_pad * 4u;
        const unsigned voff = (unsigned)(2 * (kq >> 1) * P.OW + 8 * (kq & 1)) * cp4 + (unsigned)l15 * 4u;
#pragma unroll
        for (int b = 0; b < 5; b++)
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int e = 0; e < 2; e++) {
                    const unsigned soff = (unsigned)(a * P.OW + 2 * xi + e) * cp4 + (unsigned)(64 * b);
                    const float2 yy = a ? y1v[b] : y0v[b];
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(e ? yy.y : yy.x), rsrc, (int)voff, (int)soff, WINO_OUT_AUX);
                }
    }
    if (bn) bn_complete(P, arr, n, tid, W80Stats::flag(red));
}

// Transformed weights U = G g G^T (as pack_weight_wino_kernel) in the layout of conv_wino80_kernel:
// i enumerates [K step][xi][column block][k][16 columns][4 planes nu]; K step s4 holds the padded input channels 4 s4 + k;
// the W80_BDIST K steps behind the last one are zeros.
__global__ void __launch_bounds__(256)
pack_weight_wino80_kernel(rnr_conv_desc d, const float* __restrict__ w, float* __restrict__ image, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int nsteps = (d.c_in0_pad + d.c_in1_pad) / 4;
    const int nu = (int)(i & 3);
    long r = i >> 2;
    const int col = (int)(r & 15); r >>= 4;
    const int k = (int)(r & 3); r >>= 2;
    const int nbk = (int)(r % 5); r /= 5;
    const int xi = (int)(r & 3); r >>= 2;
    const int step = (int)r;
    if (step >= nsteps) { image[i] = 0.0f; return; }
    const int c = step * 4 + k;
    const int co = nbk * 16 + col;
    double g[3][3];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) g[a][b] = (double)gemm_weight(d, w, 0, a * 3 + b, c, co);
    double row[3];
#pragma unroll
    for (int b = 0; b < 3; b++)
        row[b] = xi == 0 ? g[0][b] : (xi == 3 ? g[2][b] : 0.5 * (g[0][b] + (xi == 1 ? g[1][b] : -g[1][b]) + g[2][b]));
    const double u = nu == 0 ? row[0] : (nu == 3 ? row[2] : 0.5 * (row[0] + (nu == 1 ? row[1] : -row[1]) + row[2]));
    image[i] = (float)u;
}

static void launch_wino80(const dim3 grid, const ConvParams& P, hipStream_t st) {
    hipLaunchKernelGGL(conv_wino80_kernel, grid, dim3(CTHREADS), wino80_lds_bytes(), st, P);
}
