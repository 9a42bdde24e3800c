// Winograd F(2x2, 3x3) for the 3x3 convolutions of the U-Net (KIND 0), exact-fp32 operands on v_mfma_f32_32x32x2_f32.
// Included by conv.hip (shares ConvParams, the tile order and the BatchNorm / statistics epilogue helpers).
//
//   Y = A^T [ sum_c (G g_c G^T) .* (B^T d_c B) ] A        (Lavin & Gray 2016, the minimal F(2x2, 3x3) algorithm)
//
// A 2 x 2 output tile costs 16 multiplications per (input channel, output channel) instead of 36, i.e. the MFMA work
// of a 3x3 layer drops 2.25 x; the transforms only add and halve, so everything stays fp32 (the result differs from
// the direct convolution by rounding of the same order as a different summation order, tests/test_gpu_unet.py).
//
// Mapping.  A workgroup (4 waves, two workgroups per CU = two waves per SIMD) owns 16 x 8 output pixels = 32 Winograd
// tiles (8 x 4) x 64 output channels; wave xi owns plane row xi — the four Winograd planes (xi, nu = 0..3) — of all 32
// tiles and both 32-column halves: eight 32 x 32 accumulator blocks (128 registers).  Per K step of two input channels
// a wave issues 8 MFMAs (512 matrix-pipe cycles); the matrix pipe of a SIMD is shared with the wave of the other
// workgroup and an f32 MFMA leaves ~16 issue slots per 64 cycles, so what counts is instructions per MFMA:
//   * A operands: an MFMA lane is (tile m = lane % 32, channel parity h = lane / 32) — exactly one (tile, channel) pair,
//     so the lane reads the two rows of its own 4 x 4 input patch that plane row xi combines (4 ds_read_b64) and computes
//     row xi of B^T d B in registers (8 VALU): xi = 0: d0 - d2, 1: d1 + d2, 2: d2 - d1, 3: d1 - d3 (one wave-uniform
//     sign), then the column combinations.  The four results ARE the A operands of the wave's four planes, each used by
//     two MFMAs (the two column halves).  No transformed activations in LDS or HBM;
//   * B operands: two coalesced buffer_load_dwordx4 per K step from the pre-transformed weight image
//     (pack_weight_wino_kernel: [64-column tile][K step][xi][column half][h][32 columns][4 planes]; a workgroup streams
//     8 KB per K step, each byte once), requested five K steps ahead into a ring of eight register blocks;
//   * the halo of the next 16-channel chunk (18 x 10 pixels, prologue BatchNorm + activation applied on the way, as in
//     conv_halo_kernel): global -> registers -> LDS, one barrier per chunk.
// Patch rows are read two K steps ahead and transformed one step ahead; a K step has no branch.
// Epilogue: every wave combines its planes' columns (A^T . A needs r = M0 + M1 + M2 and M1 - M2 - M3 per plane row), the
// four plane rows meet through LDS — wave f finishes tile row f: Y0 = r0 + r1 + r2, Y1 = r1 - r2 - r3 — and each wave
// runs the statistics / BatchNorm / store path of the direct kernels for its 8 tiles x 64 columns.
//
// LDS halo image of a chunk: [16 channels][10 rows][24], 242 floats per channel plane.  Lane (ty, tx) reads columns
// 2 tx .. 2 tx + 3 of rows 2 ty + a: 8-byte reads whose 32 lanes cover 16 consecutive words per tile row, tile rows 48
// words apart: conflict-free ds_read_b64 (64 banks).

constexpr int WINO_PW = 16, WINO_PH = 8;            // output pixels per workgroup tile
constexpr int WINO_HW = WINO_PW + 2, WINO_HH = WINO_PH + 2;     // halo
constexpr int WINO_ROWP = 24;                       // floats per halo row
constexpr int WINO_PLANE = WINO_HH * WINO_ROWP + 2; // floats per channel plane (+ 2: the staging stores of the four channel quads spread over the banks)
constexpr int WINO_CHUNK = BK * WINO_PLANE;         // floats per chunk image
constexpr int WINO_SLOTS = WINO_HW * WINO_HH * 4;   // float4 slots of one halo chunk
constexpr int WINO_APT = (WINO_SLOTS + CTHREADS - 1) / CTHREADS;    // 3
constexpr int WINO_BN = 64;
#ifndef WINO_BDIST_K
#define WINO_BDIST_K 5              // 3 -> 5: -2 % on the 512-channel layers (their 16 MB of weights come from beyond the L2)
#endif
#ifndef WINO_SGB
#define WINO_SGB 5                  // VALU instructions placed behind each MFMA by the scheduling pipeline below (2: +2 %, 0 = the compiler's own order: +8 %)
#endif
constexpr int WINO_BDIST = WINO_BDIST_K;            // K steps between the request of a weight block and its MFMAs
constexpr int WINO_BRING = WINO_BDIST < 4 ? 4 : 8;  // weight blocks in registers (a power of two that divides the 8 steps of a chunk)
constexpr int WINO_STEP_FLOATS = 4 * 2 * 2 * 32 * 4;        // weight image per (column tile, K step): [xi][half][h][32][4]
constexpr int WINO_XCHG = 4 * 3 * 4 * 64 * 4;       // floats of the epilogue exchange: [finishing wave][source][4 register rows][lane][4]

typedef StatScratch<4, WINO_BN> WinoStats;          // the statistics scratch: one slot per wave, behind the exchange buffer
__host__ __device__ constexpr size_t wino_lds_bytes() {
    return (size_t)(2 * WINO_CHUNK > WINO_XCHG ? 2 * WINO_CHUNK : WINO_XCHG) * sizeof(float) + WinoStats::BYTES;
}

__global__ void __launch_bounds__(CTHREADS, 2)
conv_wino_kernel(const ConvParams P) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                       // [2][WINO_CHUNK]; the epilogue's exchange buffer afterwards

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int xi = __builtin_amdgcn_readfirstlane(tid >> 6);        // the wave's plane row
    const int l31 = lane & 31, h = lane >> 5;
    const ConvTileId T = conv_tile<WINO_PW, WINO_PH, false>(P);
    const int nt_ = T.nt, z_ = T.z;
    const int n0 = nt_ * WINO_BN;
    const int n = T.n, y0 = T.y0, x0 = T.x0;

    // halo slots of this thread (fixed source pixels for the whole K loop); wrapped slots are staged twice: loads and stores
    // need no predicate
    const int q = tid & 3;
    unsigned spix[WINO_APT];
    float* sd_cur[WINO_APT];        // staging destinations in the buffer being read / being filled
    float* sd_nxt[WINO_APT];
#pragma unroll
    for (int j = 0; j < WINO_APT; j++) {
        int hy, hx;
        float m;
        halo_slot<WINO_HW, WINO_SLOTS, CTHREADS>(tid, j, hy, hx);
        spix[j] = halo_pixel<0>(P, y0, x0, hy, hx, m);
        sd_cur[j] = As + (4 * q) * WINO_PLANE + hy * WINO_ROWP + hx;
        sd_nxt[j] = sd_cur[j] + WINO_CHUNK;
    }

    // split-K (small grids): slice z_ of P.splitk takes the chunks [c_begin, c_end) and writes its partial outputs — the output
    // transform is linear — to its own slab; splitk_reduce_kernel adds the slabs (and takes the statistics)
    const int nchunks = P.chunks_per_tap;
    const int c_begin = T.c_begin, c_end = T.c_end;
    auto chunk_src = [&](int c) { return halo_src<1>(P, n, q, c); };
    auto load_a = [&](const HaloSrc& cs, int j) { return halo_load(cs, spix[j], q); };
    auto store_a = [&](const HaloSrc& cs, float4 v, float* a) {
        const float4 u = normalize4<false>(cs, v);
        a[0] = u.x; a[WINO_PLANE] = u.y; a[2 * WINO_PLANE] = u.z; a[3 * WINO_PLANE] = u.w;
    };

    // transformed weights of this column tile: [K step][xi][column half][h][32 columns][4 planes]; the image carries
    // WINO_BDIST K steps of padding behind the last one, so the look-ahead needs no clamp
    const __amdgpu_buffer_rsrc_t wrsrc = buffer_rsrc(P.weight_wino);
    const unsigned bvoff = (unsigned)(h * 32 + l31) * 16u;
    unsigned bsoff = ((unsigned)nt_ * (unsigned)(nchunks * 8 + WINO_BDIST) + (unsigned)(c_begin * 8)) * (unsigned)(WINO_STEP_FLOATS * 4) +
                     (unsigned)xi * 2048u;
    struct BRegs { floatx4 b[2]; };
    auto load_b = [&](BRegs& dst) {      // the next K step's block
        dst.b[0] = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, (int)bvoff, (int)bsoff, 0));
        dst.b[1] = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, (int)(bvoff + 1024u), (int)bsoff, 0));
        bsoff += (unsigned)(WINO_STEP_FLOATS * 4);
    };

    // the two patch rows plane row xi combines, t = Ra + sigma Rc:  xi 0: d0 - d2, 1: d1 + d2, 2: d2 - d1, 3: d1 - d3.
    // One base register per (row, buffer): every read is base + immediate.
    const int ty = l31 >> 3, tx = l31 & 7;
    const int row_a = xi == 0 ? 0 : (xi == 2 ? 2 : 1), row_c = xi == 3 ? 3 : (xi == 2 ? 1 : 2);
    const float sigma = xi == 1 ? 1.0f : -1.0f;
    struct Rows { const float* a; const float* c; };
    Rows rcur, rnxt;
    rcur.a = As + h * WINO_PLANE + (2 * ty + row_a) * WINO_ROWP + 2 * tx;
    rcur.c = As + h * WINO_PLANE + (2 * ty + row_c) * WINO_ROWP + 2 * tx;
    rnxt.a = rcur.a + WINO_CHUNK;
    rnxt.c = rcur.c + WINO_CHUNK;
    auto read_patch = [&](float (&d)[8], const Rows& rows, int s) {
        const int xo = 2 * s * WINO_PLANE;
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

    floatx16 acc[8];            // [plane nu][column half]
#pragma unroll
    for (int p = 0; p < 8; p++)
#pragma unroll
        for (int g = 0; g < 16; g++) acc[p][g] = 0.0f;

    if (c_begin < c_end) {
        const HaloSrc cs = chunk_src(c_begin);
#pragma unroll
        for (int j = 0; j < WINO_APT; j++) store_a(cs, load_a(cs, j), sd_cur[j]);
    }
    BRegs breg[WINO_BRING];
#pragma unroll
    for (int k = 0; k < WINO_BDIST; k++) load_b(breg[k]);
    __syncthreads();
    // software pipeline of a K step t: patch rows are read during step t - 2, transformed during step t - 1, multiplied in t
    float raw[2][8], V[2][4];
    read_patch(raw[0], rcur, 0);
    transform(raw[0], V[0]);
    read_patch(raw[1], rcur, 1);

    auto chunk_body = [&](auto NEXT, int c) {
        constexpr bool next_chunk = decltype(NEXT)::value;
        const HaloSrc csn = chunk_src(next_chunk ? c + 1 : c);
        float4 avr[WINO_APT];
#pragma unroll
        for (int s = 0; s < 8; s++) {
            // the next chunk's halo is complete and nobody reads the buffer before the current one any more
            if (next_chunk && s == 6) __syncthreads();
            load_b(breg[(s + WINO_BDIST) & (WINO_BRING - 1)]);
            if (s < 6) read_patch(raw[s & 1], rcur, s + 2);
            else if (next_chunk) read_patch(raw[s & 1], rnxt, s - 6);
            if (next_chunk && s < WINO_APT) avr[s] = load_a(csn, s);
#pragma unroll
            for (int p = 0; p < 8; p++)
                acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(V[s & 1][p >> 1], breg[s & (WINO_BRING - 1)].b[p & 1][p >> 1], acc[p], 0, 0, 0);
            if (s < 7 || next_chunk) transform(raw[(s + 1) & 1], V[(s + 1) & 1]);
            if (next_chunk && s >= 3 && s < 3 + WINO_APT) store_a(csn, avr[s - 3], sd_nxt[s - 3]);
#if WINO_SGB > 0
            // one MFMA, then its share of the step's other work, eight times
#pragma unroll
            for (int p = 0; p < 8; p++) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // MFMA
                // (weight loads first, patch reads in the second half, staging stores in the first: 1.2 % faster than reads first;
                // without the memory groups, i.e. MFMA + VALU pacing only, 10 % slower)
                if (p < 3) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);  // VMEM read
                __builtin_amdgcn_sched_group_barrier(0x002, WINO_SGB, 0);      // VALU
                if (p >= 4) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); // DS read
                if (p < 4) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);  // DS write
            }
#endif
        }
        // swap the roles of the two LDS buffers
        const Rows t = rcur; rcur = rnxt; rnxt = t;
#pragma unroll
        for (int j = 0; j < WINO_APT; j++) { float* u = sd_cur[j]; sd_cur[j] = sd_nxt[j]; sd_nxt[j] = u; }
    };
    for (int c = c_begin; c + 1 < c_end; c++) chunk_body(std::true_type{}, c);
    if (c_begin < c_end) chunk_body(std::false_type{}, c_end - 1);

    // ---- epilogue: Y = A^T M A per (tile, column), statistics, BatchNorm arrival, stores ----
    // C layout of a 32 x 32 block: column = lane % 32, row (= tile) = (g & 3) + 8 (g >> 2) + 4 h, i.e. tile row g >> 2, tile
    // column (g & 3) + 4 h.  rr[g] = the column combinations of this wave's plane row for both column halves:
    // (r[b = 0], r[b = 1]) of half 0, then of half 1.
    floatx4 rr[16];
#pragma unroll
    for (int g = 0; g < 16; g++) {
        rr[g][0] = acc[0][g] + acc[2][g] + acc[4][g];
        rr[g][1] = acc[2][g] - acc[4][g] - acc[6][g];
        rr[g][2] = acc[1][g] + acc[3][g] + acc[5][g];
        rr[g][3] = acc[3][g] - acc[5][g] - acc[7][g];
    }
    __syncthreads();            // every wave is done with the halo: LDS becomes the exchange buffer
    floatx4* xb = reinterpret_cast<floatx4*>(As);           // [finishing wave f][source slot][g & 3][lane]
    // wave f finishes tile row f (register rows 4 f .. 4 f + 3); the other three hand it their plane rows
    floatx4 y0v[4], y1v[4];
    auto exchange = [&](auto F) {
        constexpr int f = decltype(F)::value;
#pragma unroll
        for (int o = 0; o < 4; o++) {
            if (o == f) continue;
            const int slot = f < o ? f : f - 1;         // this wave's position among the sources of wave o
#pragma unroll
            for (int gq = 0; gq < 4; gq++) xb[((o * 3 + slot) * 4 + gq) * 64 + lane] = rr[4 * o + gq];
        }
        __syncthreads();
#pragma unroll
        for (int gq = 0; gq < 4; gq++) {
            floatx4 R[4];
#pragma unroll
            for (int o = 0; o < 4; o++) {
                if (o == f) R[o] = rr[4 * f + gq];
                else R[o] = xb[((f * 3 + (o < f ? o : o - 1)) * 4 + gq) * 64 + lane];
            }
            y0v[gq] = R[0] + R[1] + R[2];
            y1v[gq] = R[1] - R[2] - R[3];
        }
    };
    if (xi == 0) exchange(std::integral_constant<int, 0>{});
    else if (xi == 1) exchange(std::integral_constant<int, 1>{});
    else if (xi == 2) exchange(std::integral_constant<int, 2>{});
    else exchange(std::integral_constant<int, 3>{});

    double s1[2] = {0.0, 0.0}, s2[2] = {0.0, 0.0};
#pragma unroll
    for (int gq = 0; gq < 4; gq++)
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const double a = y0v[gq][e], b = y1v[gq][e];
            s1[e >> 1] += a + b;
            s2[e >> 1] += a * a + b * b;
        }
    static_assert(WINO_XCHG % 2 == 0, "float64 scratch alignment");
    double* red = WinoStats::red(As + WINO_XCHG);
    const bool with_stats = P.stats != nullptr && P.splitk == 1;
    if (with_stats) {
#pragma unroll
        for (int nb = 0; nb < 2; nb++) {
            s1[nb] += __shfl_xor(s1[nb], 32, 64);
            s2[nb] += __shfl_xor(s2[nb], 32, 64);
            if (h == 0) {
                red[(xi * WINO_BN + 32 * nb + l31) * 2 + 0] = s1[nb];
                red[(xi * WINO_BN + 32 * nb + l31) * 2 + 1] = s2[nb];
            }
        }
        WinoStats::publish(P, red, n, n0, tid);
    }
    BnArrival arr = {nullptr, 0u};
    const bool bn = with_stats && P.arrive;
    if (bn) arr = bn_arrive(P, n, tid);
    {
        // this wave finishes tile row xi: output rows 2 xi, 2 xi + 1 of the tile
        float* base = P.out + (size_t)z_ * P.slab_stride + (((size_t)n * P.OH + y0 + 2 * xi) * P.OW + x0) * P.c_out_pad + n0;
        const ColumnStore<2, WINO_OUT_AUX> cst(P, base, n0, 0, l31, 8 * h);
#pragma unroll
        for (int gq = 0; gq < 4; gq++)
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int e = 0; e < 4; e++)
                    cst.store(a ? y1v[gq][e] : y0v[gq][e], e >> 1, (unsigned)(a * P.OW + 2 * gq + (e & 1)));
    }
    if (bn) bn_complete(P, arr, n, tid, WinoStats::flag(red));
}

// Transformed weights U = G g G^T, G = [[1, 0, 0], [1/2, 1/2, 1/2], [1/2, -1/2, 1/2], [0, 0, 1]], computed in float64 and
// rounded once.  i enumerates [64-column tile][K step][xi][column half][h][32 columns][4 planes nu]; K step = chunk * 8 + s
// holds the padded input channels chunk * 16 + 2 s + h; the WINO_BDIST K steps behind the last one are zeros.
__global__ void __launch_bounds__(256)
pack_weight_wino_kernel(rnr_conv_desc d, const float* __restrict__ w, float* __restrict__ image, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int nsteps = (d.c_in0_pad + d.c_in1_pad) / 2;
    const int nu = (int)(i & 3);
    long r = i >> 2;
    const int col = (int)(r & 31); r >>= 5;
    const int hh = (int)(r & 1); r >>= 1;
    const int nb = (int)(r & 1); r >>= 1;
    const int xi = (int)(r & 3); r >>= 2;
    const int step = (int)(r % (nsteps + WINO_BDIST));
    const int nt = (int)(r / (nsteps + WINO_BDIST));
    if (step >= nsteps) { image[i] = 0.0f; return; }
    const int c = (step >> 3) * 16 + 2 * (step & 7) + hh;
    const int co = nt * WINO_BN + nb * 32 + col;
    double g[3][3];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) g[a][b] = (double)gemm_weight(d, w, 0, a * 3 + b, c, co);
    // row xi of G g, then column nu of (.) G^T
    double row[3];
#pragma unroll
    for (int b = 0; b < 3; b++)
        row[b] = xi == 0 ? g[0][b] : (xi == 3 ? g[2][b] : 0.5 * (g[0][b] + (xi == 1 ? g[1][b] : -g[1][b]) + g[2][b]));
    const double u = nu == 0 ? row[0] : (nu == 3 ? row[2] : 0.5 * (row[0] + (nu == 1 ? row[1] : -row[1]) + row[2]));
    image[i] = (float)u;
}

static void launch_wino(const dim3 grid, const ConvParams& P, hipStream_t st) {
    const size_t lds = wino_lds_bytes();
    hipLaunchKernelGGL(conv_wino_kernel, grid, dim3(CTHREADS), lds, st, P);
}
