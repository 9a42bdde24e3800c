// Winograd F(2x2, 2x2) for the two 4x4 stride-2 convolutions of the U-Net, exact-fp32 operands on v_mfma_f32_32x32x2_f32.
// Included by conv.hip behind conv_wino.inc (the staging helpers of conv_stage.inc, same LDS halo layout, same software pipeline).
//
// Both decompose into 2x2-tap stride-1 correlations (conv_halo_kernel does the same):
//   KIND 2  ConvTranspose2d 4x4 s2 p1: output parity class (py, px) is a 2x2-tap correlation of the input,
//           out[2y + py][2x + px] = sum_{a,b in {0,1}} in[y + py - 1 + a][x + px - 1 + b] g_class[a][b]    (zero outside);
//   KIND 1  ReflectionPad2d(1) + Conv2d 4x4 s2: the sum over the four input parity phases (py, px) of a 2x2-tap correlation
//           of the phase image, out[y][x] = sum_phase sum_{a,b} in[2 (y - py + a) + py][2 (x - px + b) + px] g_phase[a][b].
// The minimal 1-D algorithm F(2, 2) takes 3 multiplications for 2 outputs of a 2-tap filter:
//   m1 = (d0 - d1) g0,  m2 = d1 (g0 + g1),  m3 = (d1 - d2) g1;   y0 = m1 + m2,  y1 = m2 - m3
// i.e. B^T = [[1,-1,0],[0,1,0],[0,1,-1]], G = [[1,0],[1,1],[0,1]], A^T = [[1,1,0],[0,1,-1]]: 9 multiplications per 2 x 2
// outputs instead of 16, all coefficients 0 / +-1 (the weight transform adds up to four weights, in float64, rounded once).
//
// Mapping.  A workgroup is 12 waves (three per SIMD, one workgroup per CU) = 4 groups x 3 plane rows xi.  Wave (group, xi)
// owns the three planes (xi, nu) of 8 x 4 Winograd tiles (16 x 8 outputs of a class / of the convolution) and two 32-column
// halves: six 32 x 32 accumulator blocks (96 registers).
//   KIND 2: group = parity class (py, px): all four classes of 16 x 8 input pixels share ONE staged input halo (18 x 10
//           pixels: they read it one row / column apart) and the workgroup's 64 output columns — 32 x 16 output pixels;
//   KIND 1: group = (tile-row half mb, 64-column half): 16 x 16 output pixels x 128 columns; the K loop runs over
//           (chunk, phase) and stages the 18 x 17 pixels of one phase image per K block.
// Epilogue: column combinations per wave, the three plane rows of a group meet through LDS in two rounds (one per column
// half), wave xi finishes register rows {0-5, 6-10, 11-15}[xi]; statistics / BatchNorm / stores as in the direct kernels.
//
// Two kernels, one per kind, share everything but their K loop and weight-image layout (the w2_* functions below):
//   conv_wino2_kernel<1>  (this file): per K step of two input channels a wave issues 6 MFMAs, 4 LDS reads (two patch rows),
//                         5 VALU (row xi of B^T d B, then the column combinations) and two buffer_load_dwordx3 from the
//                         pre-transformed weight image (pack_weight_wino2_kernel: [column tile][K step][column half][xi][half][h]
//                         [32 columns][3 planes]; the two tile-row halves read the same block); two staged float4 per thread
//                         per K block;
//   conv_wino2p_kernel<2> (conv_wino2p.inc): K-step pairs (r05), one staged float4 per thread per K block.

constexpr int W2_THREADS = 768;
constexpr int W2_HW = 18;                           // staged halo columns (17 used by KIND 1)
constexpr int W2_XCHG = 12 * 11 * 64 * 2;           // floats of one exchange round: [wave][<= 11 register rows][lane][2]
template <int KIND> struct W2Kind {
    static_assert(KIND == 1 || KIND == 2, "4x4 stride-2 convolutions");
    static constexpr int NPH = KIND == 1 ? 4 : 1;               // K blocks per 16-channel chunk (input parity phases)
    static constexpr int BNW = KIND == 1 ? 128 : 64;            // output columns per workgroup
    static constexpr int TPH = KIND == 1 ? 16 : WINO_PH;        // rows of the GEMM row space per workgroup tile
    static constexpr int HH = KIND == 1 ? 17 : 10;              // staged rows
    static constexpr int SLOTS = W2_HW * HH * 4;                // float4 slots: 1224 / 720
    static constexpr int APT = (SLOTS + W2_THREADS - 1) / W2_THREADS;       // 2 / 1
};

// ---- shared by conv_wino2_kernel<1> and conv_wino2p_kernel<2> ----

// this thread's wave, group and plane row; the workgroup's tile
struct W2Tile {
    int tid, lane, wave, wgrp, xi, grp, l31, h;
    int nt, z;          // column tile, split-K slice
    int py, mb;         // KIND 2: row parity of the output class (column parity px = grp); KIND 1: tile rows 4 mb .. 4 mb + 3 of 8
    int n0;             // first output column of this wave
    int n, y0, x0;      // view, first row / column of the tile in the GEMM row space (output pixels, KIND 1, or input pixels, KIND 2)
    int c_begin, c_end; // 16-channel chunks of the split-K slice
};
template <int KIND>
__device__ __forceinline__ W2Tile w2_tile(const ConvParams& P) {
    W2Tile T;
    T.tid = threadIdx.x;
    T.lane = T.tid & 63;
    T.wave = __builtin_amdgcn_readfirstlane(T.tid >> 6);
    T.wgrp = T.wave / 3; T.xi = T.wave - 3 * T.wgrp;       // group of three plane-row waves
    const int sub = T.wgrp >> 1;                            // KIND 2: (py, px); KIND 1: (tile-row half, column half)
    T.grp = T.wgrp & 1;
    T.l31 = T.lane & 31; T.h = T.lane >> 5;
    // all four parity classes of the transposed conv live in one workgroup: z is the split-K slice alone for both kinds
    const ConvTileId C = conv_tile<WINO_PW, W2Kind<KIND>::TPH, false>(P);
    T.nt = C.nt; T.z = C.z;
    T.py = KIND == 2 ? sub : 0;
    T.mb = KIND == 1 ? sub : 0;
    T.n0 = T.nt * W2Kind<KIND>::BNW + (KIND == 1 ? 64 * T.grp : 0);
    T.n = C.n; T.y0 = C.y0; T.x0 = C.x0;
    T.c_begin = C.c_begin; T.c_end = C.c_end;
    return T;
}

// Halo slot j of a thread: a float4 of channel quad q = tid & 3.  Staged row hy / column hx is
//   KIND 2: input pixel (y0 - 1 + hy, x0 - 1 + hx), zero outside the map (mask; py / px shift the READ by one row / column);
//   KIND 1, phase (phy, phx): input pixel (reflect1(2 (y0 + hy) - phy), reflect1(2 (x0 + hx) - phx)).  Reflection only ever
//           moves row 2 (y0 + hy) = H to H - 2 (phy = 0) and row -1 to 1 (phy = 1), so the four pixels of a slot are
//           spix + phy * (+-W) + phx * (+-1): one register per slot and two sign bits, instead of two reflections per
//           staging load (r05; ~14 VALU each, - 1 % on the five stride-2 layers).
struct W2Slot {
    int hy, hx;
    unsigned spix;
    unsigned sign;      // KIND 1: bit 1: the phase-1 row lies BELOW the phase-0 row (+W), bit 0: the phase-1 column lies RIGHT of it (+1)
    float mask;         // KIND 2: 1 inside the map, 0 outside
};
template <int KIND>
__device__ __forceinline__ W2Slot w2_slot(const ConvParams& P, const W2Tile& T, int j) {
    W2Slot S;
    halo_slot<W2_HW, W2Kind<KIND>::SLOTS, W2_THREADS>(T.tid, j, S.hy, S.hx);
    S.sign = 0; S.mask = 1.f;
    if (KIND == 2) {
        S.spix = halo_pixel<2>(P, T.y0, T.x0, S.hy, S.hx, S.mask);
    } else {
        const int ry = 2 * (T.y0 + S.hy), cx = 2 * (T.x0 + S.hx);
        const int r0 = reflect1(ry, P.H), r1 = reflect1(ry - 1, P.H), c0 = reflect1(cx, P.W), c1 = reflect1(cx - 1, P.W);
        S.spix = (unsigned)(r0 * P.W + c0);
        S.sign = (unsigned)((r1 > r0 ? 2 : 0) | (c1 > c0 ? 1 : 0));
    }
    return S;
}

// the raw float4 of a slot in K block kb = (chunk, input parity phase): spix, and for KIND 1 the slot's sign bits at bit
// `sbit` + 1 / `sbit` of `signs`
template <int KIND>
__device__ __forceinline__ float4 w2_load_halo(const ConvParams& P, const HaloSrc& cs, unsigned pixel, unsigned signs, int sbit, int q) {
    if (KIND == 1) {
        if (cs.phy) pixel += (signs >> (sbit + 1)) & 1u ? (unsigned)P.W : 0u - (unsigned)P.W;
        if (cs.phx) pixel += (signs >> sbit) & 1u ? 1u : ~0u;
    }
    return halo_load(cs, pixel, q);
}

// Transformed weight U[xi][nu] = (G g G^T)[xi][nu], G = [[1, 0], [1, 1], [0, 1]], of the 2x2-tap correlation g of parity class
// grp (KIND 2) or phase (KIND 1) for input channel c, output column co: taps in increasing input index, float64, rounded once.
template <int KIND>
__device__ __forceinline__ float w2_weight(const rnr_conv_desc& d, const float* __restrict__ w, int grp, int phase, int xi, int nu,
                                           int c, int co) {
    double g[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) {
            if (KIND == 2) {
                // class grp = 2 py + px: conv_halo_kernel's tap (ty, tx) reads input row y + py - ty, column x + px - tx
                g[a][b] = (double)gemm_weight(d, w, grp, (1 - a) * 2 + (1 - b), c, co);
            } else {
                // phase (phy, phx): tap a is kernel row ky = phy ? 2 a : 1 + 2 a (conv_halo_kernel, KIND 1), same for columns
                const int phy = phase >> 1, phx = phase & 1;
                const int ky = phy ? 2 * a : 1 + 2 * a, kx = phx ? 2 * b : 1 + 2 * b;
                g[a][b] = (double)gemm_weight(d, w, 0, ky * 4 + kx, c, co);
            }
        }
    double row[2];
#pragma unroll
    for (int b = 0; b < 2; b++) row[b] = xi == 0 ? g[0][b] : (xi == 2 ? g[1][b] : g[0][b] + g[1][b]);
    return (float)(nu == 0 ? row[0] : (nu == 2 ? row[1] : row[0] + row[1]));
}

// ---- conv_wino2_kernel<1>: the stride-2 convolution, one K step per 6 MFMAs ----

struct W2Geo {
    static constexpr int PLANE = W2Kind<1>::HH * WINO_ROWP + 2;    // floats per channel plane
    static constexpr int CHUNK = BK * PLANE;                        // floats per staged K block
};
#ifndef W2_SGB
#define W2_SGB 3                    // VALU instructions behind each MFMA in the scheduling pipeline of a K step (1 - 2: +3 ... +5 %,
                                    // 0 = compiler's order: up to +7 %)
#endif
#ifndef W2_BDIST_K
#define W2_BDIST_K 3
#endif
constexpr int W2_BDIST = W2_BDIST_K;                         // K steps between the request of a weight block and its MFMAs
constexpr int W2_STEP_FLOATS = 2 * 3 * 2 * 2 * 32 * 3;       // weight image per K step: [column half][xi][half][h][32][3]

typedef StatScratch<12, 64> W2Stats;                // the statistics scratch of conv_wino2_epilogue.inc: one slot per wave
__host__ __device__ constexpr size_t wino2_lds_bytes() {
    return (size_t)(2 * W2Geo::CHUNK > W2_XCHG ? 2 * W2Geo::CHUNK : W2_XCHG) * sizeof(float) + W2Stats::BYTES;
}

template <int KIND>
__global__ void __launch_bounds__(W2_THREADS, 3)
conv_wino2_kernel(const ConvParams P) {
    static_assert(KIND == 1, "the stride-2 convolution (the transposed one runs conv_wino2p_kernel)");
    constexpr int NPH = W2Kind<KIND>::NPH, APT = W2Kind<KIND>::APT;
    constexpr int PLANE = W2Geo::PLANE, CHUNK = W2Geo::CHUNK;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                       // [2][CHUNK]; the epilogue's exchange buffer afterwards

    const W2Tile T = w2_tile<KIND>(P);
    const int xi = T.xi, l31 = T.l31, h = T.h;
    const int q = T.tid & 3;
    unsigned spix[APT];
    unsigned ssign = 0;     // the sign bits of slot j at bits 2 j + 1, 2 j
    float* sd_cur[APT];
    float* sd_nxt[APT];
#pragma unroll
    for (int j = 0; j < APT; j++) {
        const W2Slot S = w2_slot<KIND>(P, T, j);
        spix[j] = S.spix;
        ssign |= S.sign << (2 * j);
        sd_cur[j] = As + (4 * q) * PLANE + S.hy * WINO_ROWP + S.hx;
        sd_nxt[j] = sd_cur[j] + CHUNK;
    }

    // split-K (small grids): slice z of P.splitk takes the chunks [c_begin, c_end) and writes partial outputs to its own slab
    const int nchunks = P.chunks_per_tap;
    const int kb_begin = T.c_begin * NPH, kb_end = T.c_end * NPH;   // K blocks: (chunk, phase)
    auto block_src = [&](int kb) { return halo_src<NPH>(P, T.n, q, kb); };
    auto load_a = [&](const HaloSrc& cs, int j) { return w2_load_halo<KIND>(P, cs, spix[j], ssign, 2 * j, q); };
    auto store_a = [&](const HaloSrc& cs, float4 v, int j, float* a) {
        const float4 u = normalize4<false>(cs, v);
        a[0] = u.x; a[PLANE] = u.y; a[2 * PLANE] = u.z; a[3 * PLANE] = u.w;
    };

    // transformed weights of this column tile: [K step][column half][xi][half][h][32 columns][3 planes]
    const int nsteps = nchunks * NPH * 8;
    const __amdgpu_buffer_rsrc_t wrsrc = buffer_rsrc(P.weight_wino);
    const unsigned bvoff = (unsigned)(h * 32 + l31) * 12u;
    unsigned bsoff = ((unsigned)T.nt * (unsigned)(nsteps + W2_BDIST) + (unsigned)(kb_begin * 8)) * (unsigned)(W2_STEP_FLOATS * 4) +
                     (unsigned)((T.grp * 3 + xi) * 2) * 768u;
    typedef float floatx3 __attribute__((ext_vector_type(3)));
    struct BRegs { floatx3 b[2]; };
    auto load_b = [&](BRegs& dst) {      // the next K step's block
        dst.b[0] = __builtin_bit_cast(floatx3, __builtin_amdgcn_raw_buffer_load_b96(wrsrc, (int)bvoff, (int)bsoff, 0));
        dst.b[1] = __builtin_bit_cast(floatx3, __builtin_amdgcn_raw_buffer_load_b96(wrsrc, (int)(bvoff + 768u), (int)bsoff, 0));
        bsoff += (unsigned)(W2_STEP_FLOATS * 4);
    };

    // the two patch rows plane row xi combines, t = Ra + sigma Rc:  xi 0: d0 - d1, 1: d1, 2: d1 - d2
    const int ty = l31 >> 3, tx = l31 & 7;
    const int row_a = xi == 0 ? 0 : 1, row_c = xi == 2 ? 2 : 1;
    const float sigma = xi == 1 ? 0.0f : -1.0f;
    struct Rows { const float* a; const float* c; };
    Rows rcur, rnxt;
    const int row0 = 2 * (4 * T.mb + ty);       // first patch row of this lane's tile in the staged image
    rcur.a = As + h * PLANE + (row0 + row_a) * WINO_ROWP + 2 * tx;
    rcur.c = As + h * PLANE + (row0 + row_c) * WINO_ROWP + 2 * tx;
    rnxt.a = rcur.a + CHUNK;
    rnxt.c = rcur.c + CHUNK;
    auto read_patch = [&](float (&d)[8], const Rows& rows, int s) {
        const int xo = 2 * s * PLANE;
        const float2 a0 = *reinterpret_cast<const float2*>(rows.a + xo), a1 = *reinterpret_cast<const float2*>(rows.a + xo + 2);
        const float2 c0 = *reinterpret_cast<const float2*>(rows.c + xo), c1 = *reinterpret_cast<const float2*>(rows.c + xo + 2);
        d[0] = a0.x; d[1] = a0.y; d[2] = a1.x; d[3] = a1.y;
        d[4] = c0.x; d[5] = c0.y; d[6] = c1.x; d[7] = c1.y;
    };

    floatx16 acc[6];            // [plane nu][column half]
#pragma unroll
    for (int p = 0; p < 6; p++)
#pragma unroll
        for (int g = 0; g < 16; g++) acc[p][g] = 0.0f;

    if (kb_begin < kb_end) {
        const HaloSrc cs = block_src(kb_begin);
#pragma unroll
        for (int j = 0; j < APT; j++) store_a(cs, load_a(cs, j), j, sd_cur[j]);
    }
    BRegs breg[4];
#pragma unroll
    for (int k = 0; k < W2_BDIST; k++) load_b(breg[k]);
    __syncthreads();

    // the K loop (a lambda, like conv_wino2p_kernel's: written straight into the kernel it spills two registers)
    auto k_loop = [&]() {
        auto transform = [&](const float (&d)[8], float (&v)[3]) {
            float t[3];
#pragma unroll
            for (int j = 0; j < 3; j++) t[j] = __builtin_fmaf(sigma, d[4 + j], d[j]);
            v[0] = t[0] - t[1]; v[1] = t[1]; v[2] = t[1] - t[2];
        };
        float raw[2][8], V[2][3];
        read_patch(raw[0], rcur, 0);
        transform(raw[0], V[0]);
        read_patch(raw[1], rcur, 1);
        auto block_body = [&](auto NEXT, int kb) {
            constexpr bool next_block = decltype(NEXT)::value;
            const HaloSrc csn = block_src(next_block ? kb + 1 : kb);
            float4 avr[APT];
#pragma unroll
            for (int s = 0; s < 8; s++) {
                if (next_block && s == 6) __syncthreads();
                load_b(breg[(s + W2_BDIST) & 3]);
                if (s < 6) read_patch(raw[s & 1], rcur, s + 2);
                else if (next_block) read_patch(raw[s & 1], rnxt, s - 6);
                if (next_block && s < APT) avr[s] = load_a(csn, s);
#pragma unroll
                for (int p = 0; p < 6; p++)
                    acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(V[s & 1][p >> 1], breg[s & 3].b[p & 1][p >> 1], acc[p], 0, 0, 0);
                if (s < 7 || next_block) transform(raw[(s + 1) & 1], V[(s + 1) & 1]);
                if (next_block && s >= 3 && s < 3 + APT) store_a(csn, avr[s - 3], s - 3, sd_nxt[s - 3]);
#pragma unroll
                for (int p = 0; p < (W2_SGB > 0 ? 6 : 0); p++) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // MFMA
                    if (p < 4) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);      // DS read
                    __builtin_amdgcn_sched_group_barrier(0x002, W2_SGB, 0);      // VALU
                    if (p < 3) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);  // VMEM read
                    if (p >= 2) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0); // DS write
                }
            }
            const Rows t = rcur; rcur = rnxt; rnxt = t;
#pragma unroll
            for (int j = 0; j < APT; j++) { float* u = sd_cur[j]; sd_cur[j] = sd_nxt[j]; sd_nxt[j] = u; }
        };
        for (int kb = kb_begin; kb + 1 < kb_end; kb++) block_body(std::true_type{}, kb);
        if (kb_begin < kb_end) block_body(std::false_type{}, kb_end - 1);

    };
    k_loop();

#include "conv_wino2_epilogue.inc"
}

// conv_wino2_kernel's weight image: i enumerates [column tile][K step][column half grp][xi][half][h][32 columns][3 planes nu];
// a K step is ((chunk * 4 + phase) * 8 + s) and holds the padded input channels chunk * 16 + 2 s + h; the W2_BDIST K steps
// behind the last one are zeros.
__global__ void __launch_bounds__(256)
pack_weight_wino2_kernel(rnr_conv_desc d, const float* __restrict__ w, float* __restrict__ image, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int nsteps = (d.c_in0_pad + d.c_in1_pad) / 2 * 4;
    const int nu = (int)(i % 3);
    long r = i / 3;
    const int col = (int)(r & 31); r >>= 5;
    const int hh = (int)(r & 1); r >>= 1;
    const int nb = (int)(r & 1); r >>= 1;
    const int xi = (int)(r % 3); r /= 3;
    const int grp = (int)(r % 2); r /= 2;
    const int step = (int)(r % (nsteps + W2_BDIST));
    const int nt = (int)(r / (nsteps + W2_BDIST));
    if (step >= nsteps) { image[i] = 0.0f; return; }
    const int kb = step >> 3, s = step & 7;
    const int c = (kb / 4) * 16 + 2 * s + hh;
    image[i] = w2_weight<1>(d, w, 0, kb % 4, xi, nu, c, nt * 128 + grp * 64 + nb * 32 + col);
}

static void launch_wino2(const dim3 grid, const ConvParams& P, hipStream_t st) {
    static bool attr_set = false;
    if (!attr_set) {         // > 64 KiB of dynamic LDS needs the opt-in
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_wino2_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)wino2_lds_bytes());
        attr_set = true;
    }
    hipLaunchKernelGGL((conv_wino2_kernel<1>), grid, dim3(W2_THREADS), wino2_lds_bytes(), st, P);
}
