// Winograd F(2x2, 2x2) for the transposed 4x4 stride-2 convolution (KIND 2), second generation (r05): the algorithm, the
// workgroup mapping and the epilogue of conv_wino2.inc (read its header first; tiles, halo staging, split-K, the exchange of the
// plane rows, statistics, BatchNorm arrival and stores are its w2_* functions) with a K loop that issues fewer instructions
// per MFMA.
//
// What bounded the first-generation K loop (r04 PMC + ISA: per 48 MFMAs of a wave 34 - 40 LDS instructions, 16 buffer_load_dwordx3,
// 85 - 103 VALU, a dwordx3 spill reload in the K loop of the transposed kernel; every one of them costs matrix-pipe time beside
// an f32 MFMA, DESIGN 3.3a):  a K step (two input channels: lane half h takes channel 2 s + h) read two patch rows of 3 floats
// as ds_read_b64 + ds_read_b32 each and its six weights as two dwordx3.
//
// Here a wave works on K-step PAIRS (12 MFMAs):
//   * LDS image: the two channels a lane half needs in a pair (4 P + h and 4 P + 2 + h) are INTERLEAVED per pixel —
//     image [pair P][h][row][pixel][2] — so a patch row of a pair is 6 consecutive floats: ds_read_b128 + ds_read_b64 per row
//     and pair (4 LDS reads per 12 MFMAs instead of 8 - 10), staged by two ds_write_b64 per float4 of the halo instead of
//     four ds_write_b32;
//   * weights: the 12 floats of a lane for a pair (2 steps x 2 column halves x 3 planes) are contiguous in the image
//     [column tile][pair][class][xi][h][32 columns][12]: three buffer_load_dwordx4 per 12 MFMAs instead of four dwordx3, one
//     pair ahead in a ring of two pair blocks (24 registers, what the ring of four step blocks took);
//   * the K loop is instantiated per plane row xi and per column parity px of the class: the patch-row offsets are
//     immediates (one address register instead of four), the middle plane row (xi = 1: t = d1) reads ONE patch row and runs
//     no row combination, and nothing is kept in scratch.
// -4.3 ... -4.7 % on the transposed layers against conv_wino2_kernel's K loop.  The stride-2 convolutions were measured on this
// K loop too and lost (+8 ... +23 %: the kernel needs scratch there and its 12-MFMA weight look-ahead stalls behind the two HBM
// halo loads of every phase block; profiles/r05_wino2_pairs_ab.txt), so they stay on conv_wino2_kernel<1>.

#ifndef W2P_ROWQ_K
#define W2P_ROWQ_K 40
#endif
constexpr int W2P_ROWQ = W2P_ROWQ_K;                        // floats per image row: 18 pixels x 2 channels = 36 used; rows stay 16-byte aligned
#ifndef W2P_AHEAD
#define W2P_AHEAD 3                // weight quads (16 bytes per lane = 4 MFMAs) requested ahead of the one being consumed
#endif
#ifndef W2P_RING
#define W2P_RING (W2P_AHEAD < 4 ? 4 : 6)            // quad registers of the weight ring: > W2P_AHEAD and a divisor of the 12 quads of a K block
#endif
static_assert(W2P_RING > W2P_AHEAD && 12 % W2P_RING == 0, "weight ring");
constexpr int W2P_PAD_PAIRS = (W2P_AHEAD + 2) / 3;  // zero pair-steps behind the last one of a column tile (the weight look-ahead)
struct W2PGeo {
    static constexpr int PLANE = W2Kind<2>::HH * W2P_ROWQ + 4;  // floats per (pair, h) plane: 16-byte aligned, 2 * PLANE = 24 mod 32 spreads the four channel quads of a staging store over the banks
    static constexpr int CHUNK = 8 * PLANE;                     // floats per staged K block (16 channels)
};
#ifndef W2P_SGB
#define W2P_SGB 5                   // VALU instructions behind each MFMA in the scheduling pipeline of a pair (r05 A/B: 0: +5 %, 3 / 5: equal)
#endif
constexpr int W2P_PAIR_FLOATS = 4 * 3 * 2 * 32 * 12;       // weight image per pair-step: [class][xi][h][32][12]

__host__ __device__ constexpr size_t wino2p_lds_bytes() {
    return (size_t)(2 * W2PGeo::CHUNK > W2_XCHG ? 2 * W2PGeo::CHUNK : W2_XCHG) * sizeof(float) + W2Stats::BYTES;
}

template <int KIND>
__global__ void __launch_bounds__(W2_THREADS, 3)
conv_wino2p_kernel(const ConvParams P) {
    static_assert(KIND == 2, "the transposed convolution (the stride-2 one runs conv_wino2_kernel)");
    constexpr int APT = W2Kind<KIND>::APT;
    constexpr int PLANE = W2PGeo::PLANE, CHUNK = W2PGeo::CHUNK;
    constexpr int PAIR_BYTES = W2P_PAIR_FLOATS * 4;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                       // [2][CHUNK]; the epilogue's exchange buffer afterwards

    const W2Tile T = w2_tile<KIND>(P);
    const int xi = T.xi, l31 = T.l31, h = T.h;
    const int q = T.tid & 3;
    unsigned spix[APT];
    float smask[APT];
    // sdpack: the LDS float index of slot j in image 0 in bits 16 j .. 16 j + 13 (< 2 * CHUNK < 2^14)
    unsigned sdpack = 0;
    static_assert(2 * CHUNK < (1 << 14) && APT <= 2, "slot indices are packed into 14 bits each");
#pragma unroll
    for (int j = 0; j < APT; j++) {
        const W2Slot S = w2_slot<KIND>(P, T, j);
        spix[j] = S.spix;
        smask[j] = S.mask;
        // channel quad q = pair q of the block: plane (q, h = 0) takes channels (4 q, 4 q + 2), plane (q, 1) takes (4 q + 1, 4 q + 3)
        sdpack |= (unsigned)((2 * q) * PLANE + S.hy * W2P_ROWQ + 2 * S.hx) << (16 * j);
    }

    const int nchunks = P.chunks_per_tap;
    const int kb_begin = T.c_begin, kb_end = T.c_end;           // K blocks: one per chunk
    auto block_src = [&](int kb) { return halo_src<1>(P, T.n, q, kb); };
    auto load_a = [&](const HaloSrc& cs, int j) { return w2_load_halo<KIND>(P, cs, spix[j], 0u, 0, q); };
    auto store_a = [&](const HaloSrc& cs, float4 v, int j, float* a) {
        const float4 u = normalize4<true>(cs, v, smask[j]);
        *reinterpret_cast<float2*>(a) = make_float2(u.x, u.z);              // lane half 0: channels 4 q, 4 q + 2 (steps 2 q, 2 q + 1)
        *reinterpret_cast<float2*>(a + PLANE) = make_float2(u.y, u.w);      // lane half 1: channels 4 q + 1, 4 q + 3
    };

    // transformed weights of this column tile: [pair][class][xi][h][32 columns][12 = step in pair, column half, plane]
    const int npairs = nchunks * 4;
    const __amdgpu_buffer_rsrc_t wrsrc = buffer_rsrc(P.weight_wino);
    const unsigned bvoff = (unsigned)(h * 32 + l31) * 48u;
    unsigned bsoff = ((unsigned)T.nt * (unsigned)(npairs + W2P_PAD_PAIRS) + (unsigned)(kb_begin * 4)) * (unsigned)PAIR_BYTES +
                     (unsigned)(T.wgrp * 3 + xi) * 3072u;
    // the 48 bytes of a pair are three quads; quad Q of a K block (12 per block) is requested while quad Q - W2P_AHEAD is being
    // consumed — a look-ahead of 4 W2P_AHEAD MFMAs — into a ring of W2P_RING quad registers (4: 16 VGPRs).  12 quads are a whole
    // number of turns of the ring: every block starts at ring position 0.
    floatx4 wq[W2P_RING];
    auto load_quad = [&](int qi) {      // qi = quad of the pair (0..2), compile-time after unrolling; the next pair begins behind quad 2
        const floatx4 v = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, (int)(bvoff + 16u * qi), (int)bsoff, 0));
        if (qi == 2) bsoff += (unsigned)PAIR_BYTES;
        return v;
    };

    const int ty = l31 >> 3, tx = l31 & 7;
    const int row0 = 2 * ty + T.py;                                     // first patch row of this lane's tile in the staged image
    const float* rbase = As + h * PLANE + row0 * W2P_ROWQ + 4 * tx;     // + 2 px (floats), + row * ROWQ, + 2 P * PLANE: immediates

    floatx16 acc[6];            // [plane nu][column half]
#pragma unroll
    for (int p = 0; p < 6; p++)
#pragma unroll
        for (int g = 0; g < 16; g++) acc[p][g] = 0.0f;

    if (kb_begin < kb_end) {
        const HaloSrc cs = block_src(kb_begin);
#pragma unroll
        for (int j = 0; j < APT; j++) store_a(cs, load_a(cs, j), j, As + ((sdpack >> (16 * j)) & 0x3fffu));
    }
#pragma unroll
    for (int k = 0; k < W2P_AHEAD; k++) wq[k] = load_quad(k % 3);
    __syncthreads();

    // the K loop, instantiated per column parity of the class (px) and per plane row xi
    auto k_loop = [&](auto PXC, auto XIC) {
        constexpr int px = decltype(PXC)::value, XI = decltype(XIC)::value;
        constexpr int ROW_A = (XI == 0 ? 0 : 1) * W2P_ROWQ + 2 * px, ROW_C = (XI == 2 ? 2 : 1) * W2P_ROWQ + 2 * px;
        constexpr int NROW = XI == 1 ? 1 : 2;
        struct Raw { float a[6], c[6]; };
        // the six floats (3 pixels x 2 steps) of a patch row of pair pp: 16-byte + 8-byte reads, the aligned one first or last
        auto read_row = [&](float (&d)[6], const float* p) {
            if (px == 0) {
                const float4 u = *reinterpret_cast<const float4*>(__builtin_assume_aligned(p, 16));
                const float2 v = *reinterpret_cast<const float2*>(p + 4);
                d[0] = u.x; d[1] = u.y; d[2] = u.z; d[3] = u.w; d[4] = v.x; d[5] = v.y;
            } else {
                const float2 v = *reinterpret_cast<const float2*>(p);
                const float4 u = *reinterpret_cast<const float4*>(__builtin_assume_aligned(p + 2, 16));
                d[0] = v.x; d[1] = v.y; d[2] = u.x; d[3] = u.y; d[4] = u.z; d[5] = u.w;
            }
        };
        auto read_pair = [&](Raw& r, const float* buf_base, int pp) {
            read_row(r.a, buf_base + 2 * pp * PLANE + ROW_A);
            if (NROW == 2) read_row(r.c, buf_base + 2 * pp * PLANE + ROW_C);
        };
        // row xi of B^T d, then the column combinations, for both steps of the pair: d[2 j + e] = pixel j, step e
        auto transform = [&](const Raw& r, float (&v)[2][3]) {
#pragma unroll
            for (int e = 0; e < 2; e++) {
                float t[3];
#pragma unroll
                for (int j = 0; j < 3; j++) t[j] = NROW == 2 ? r.a[2 * j + e] - r.c[2 * j + e] : r.a[2 * j + e];
                v[e][0] = t[0] - t[1]; v[e][1] = t[1]; v[e][2] = t[1] - t[2];
            }
        };
        Raw raw;
        float V[2][2][3];
        read_pair(raw, rbase, 0);
        transform(raw, V[0]);
        const float* rcur = rbase;              // this lane's patch origin in the image being read
        int nxt_off = CHUNK;                    // offset of the image being staged (wave-uniform): the other image
        auto block_body = [&](auto NEXT, int kb) {
            constexpr bool next_block = decltype(NEXT)::value;
            const HaloSrc csn = block_src(next_block ? kb + 1 : kb);
            float4 avr[APT];
#pragma unroll
            for (int pp = 0; pp < 4; pp++) {
                // pair 3 reads pair 0 of the next block: its image is complete, and nobody reads this block's image any more
                if (next_block && pp == 3) __syncthreads();
                if (pp < 3) read_pair(raw, rcur, pp + 1);
                else if (next_block) read_pair(raw, rcur + (2 * nxt_off - CHUNK), 0);
#ifndef W2P_STORE_PAIR
#define W2P_STORE_PAIR 2           // the halo float4s of the next block are requested in pair 0 and stored in this pair (2: 24 MFMAs
                                   // later; with 1 the layers whose input comes from HBM stall on it: L3 + 8 %, r05 A/B)
#endif
                if (next_block && pp == 0) {
#pragma unroll
                    for (int j = 0; j < APT; j++) avr[j] = load_a(csn, j);
                }
#pragma unroll
                for (int m = 0; m < 12; m++) {          // m = step e * 6 + column half * 3 + plane nu: the order of the weight image
                    const int Q = 3 * pp + (m >> 2);    // quad of the block this MFMA reads
                    if ((m & 3) == 0) wq[(Q + W2P_AHEAD) % W2P_RING] = load_quad((Q + W2P_AHEAD) % 3);      // the quads are consecutive in the image
                    const int e = m / 6, nb = (m % 6) / 3, nu = m % 3;
                    acc[2 * nu + nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(V[pp & 1][e][nu], wq[Q % W2P_RING][m & 3], acc[2 * nu + nb], 0, 0, 0);
                }
                if (pp < 3 || next_block) transform(raw, V[(pp + 1) & 1]);
                if (next_block && pp == W2P_STORE_PAIR) {
#pragma unroll
                    for (int j = 0; j < APT; j++) store_a(csn, avr[j], j, As + nxt_off + ((sdpack >> (16 * j)) & 0x3fffu));
                }
#if W2P_SGB > 0
#pragma unroll
                for (int p = 0; p < 12; p++) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // MFMA
                    if (p < 2 * NROW) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);        // DS read
                    __builtin_amdgcn_sched_group_barrier(0x002, W2P_SGB, 0);        // VALU
                    if ((p & 3) == 1) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);        // VMEM read: a weight quad per four MFMAs
                    if (p >= 6 && p < 6 + APT && next_block && pp == 0) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);    // ... and the halo loads
                    if (p >= 8 && p < 8 + 2 * APT && next_block && pp == W2P_STORE_PAIR) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);    // DS write
                }
#endif
            }
            rcur += 2 * nxt_off - CHUNK;
            nxt_off = CHUNK - nxt_off;
        };
        for (int kb = kb_begin; kb + 1 < kb_end; kb++) block_body(std::true_type{}, kb);
        if (kb_begin < kb_end) block_body(std::false_type{}, kb_end - 1);
    };
    auto k_loop_xi = [&](auto PXC) {
        if (xi == 0) k_loop(PXC, std::integral_constant<int, 0>{});
        else if (xi == 1) k_loop(PXC, std::integral_constant<int, 1>{});
        else k_loop(PXC, std::integral_constant<int, 2>{});
    };
    if (T.grp == 1) k_loop_xi(std::integral_constant<int, 1>{});
    else k_loop_xi(std::integral_constant<int, 0>{});

#include "conv_wino2_epilogue.inc"
}

// conv_wino2p_kernel's weight image: i enumerates [column tile][pair-step][class grp][xi][h][32 columns][12 = e (step of the pair),
// nb (column half), nu (plane)]; K step 2 pair + e = 8 chunk + s holds the padded input channels chunk * 16 + 2 s + h; the
// W2P_PAD_PAIRS pair-steps behind the last one are zeros.
__global__ void __launch_bounds__(256)
pack_weight_wino2p_kernel(rnr_conv_desc d, const float* __restrict__ w, float* __restrict__ image, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int npairs = (d.c_in0_pad + d.c_in1_pad) / 4;
    const int w12 = (int)(i % 12);
    const int nu = w12 % 3, nb = (w12 / 3) & 1, e = w12 / 6;
    long r = i / 12;
    const int col = (int)(r & 31); r >>= 5;
    const int hh = (int)(r & 1); r >>= 1;
    const int xi = (int)(r % 3); r /= 3;
    const int grp = (int)(r % 4); r /= 4;
    const int pstep = (int)(r % (npairs + W2P_PAD_PAIRS));
    const int nt = (int)(r / (npairs + W2P_PAD_PAIRS));
    if (pstep >= npairs) { image[i] = 0.0f; return; }
    const int step = 2 * pstep + e;
    const int c = (step >> 3) * 16 + 2 * (step & 7) + hh;
    image[i] = w2_weight<2>(d, w, grp, 0, xi, nu, c, nt * 64 + nb * 32 + col);
}

static void launch_wino2p(const dim3 grid, const ConvParams& P, hipStream_t st) {
    static bool attr_set = false;
    if (!attr_set) {         // > 64 KiB of dynamic LDS needs the opt-in
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_wino2p_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)wino2p_lds_bytes());
        attr_set = true;
    }
    hipLaunchKernelGGL((conv_wino2p_kernel<2>), grid, dim3(W2_THREADS), wino2p_lds_bytes(), st, P);
}
