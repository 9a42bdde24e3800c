// Winograd F(4x4, 3x3) for the 3x3 OUT LAYER of the U-Net (78 output channels in 80 columns; descriptor flag
// RNR_CONV_WINOGRAD4_OUT), exact-fp32 operands on v_mfma_f32_16x16x4_f32.  Included by conv.hip behind conv_wino80.inc (whose
// F(2x2, 3x3) kernel stays the fall-back) and conv_wino4.inc (the algorithm: its points (0, +-3/4, +-3/2, inf), w4_bt, w4_at,
// w4_weight_u; its staging scheme and BatchNorm table).
//
// 80 columns are five 16-column blocks of the 16 x 16 x 4 instruction: 36 multiplications per 4 x 4 outputs and no padding
// column — 0.5625 x the MFMAs of conv_wino80_kernel (16 per 2 x 2), where conv_wino4_kernel's 64-column tiles would run 128.
//
// Mapping.  A workgroup is 12 waves (three per SIMD, one workgroup per CU).  It owns 16 x 16 output pixels = 16 tiles (4 x 4)
// of 4 x 4 outputs x all 80 columns: 36 planes x 5 column blocks = 180 accumulator blocks of 16 x 16.  Wave w = 6 nh + xi owns the
// planes (xi, nu = 3 nh .. 3 nh + 2) x 5 blocks = 15 blocks (60 registers).  An MFMA lane is (tile m = lane % 16 = 4 ty + tx,
// channel kq = lane / 16); a K step is four input channels, a chunk of 16 channels four K steps.  Per K step a wave
//   * reads ONE row segment of 6 floats of the staged image (ds_read_b128 + ds_read_b64) and runs its half of the horizontal
//     B^T: with the symmetric points {o0, o1, o2} need p, q and {o3, o4, o5} need r, s of w4_bt (7 VALU each; the K loop is
//     instantiated per half, the other half of w4_bt is dead code), three A operands, each used by five MFMAs;
//   * loads 15 dwords of weights per lane straight into B operand registers (three lane-linear buffer_load_dwordx4 + one
//     dwordx3 from pack_weight_wino80f4_kernel's image [K step][wave][3 x [lane][4] + [lane][3]], dword e = 5 nu' + block),
//     W8F_BDIST K steps ahead;
//   * issues 15 MFMAs (480 matrix-pipe cycles; 1440 per SIMD and K step).
// Staging (conv_wino4_kernel's scheme): the VERTICAL half of the input transform happens on the way into LDS.  An item (tile
// row sty, halo column shx of 18, channel PAIR cp of 8) = 576 per chunk = the threads of waves 0 - 8 (wave-uniform: the K loop
// is instantiated with and without staging, so a K step is one basic block) loads the six halo rows 4 sty - 1 .. 4 sty + 4 of
// its column as six dwordx2 (one base pixel + two reflection flags), applies the producer's BatchNorm + activation from the LDS
// table of the view, runs w4_bt down the column and stores T[xi] with six dword stores per channel (the compiler pairs them: three ds_write2st64_b32).  Pairs, not quads as in
// conv_wino4_kernel: a chunk has four K steps here and the image must be complete before the fourth, so channel 0 is
// stored in K step 0, channel 1 in step 1, and the loads of the chunk after next are requested in step 2 — two K steps and a
// barrier before their first use, in 12 registers.
// LDS image of a chunk: channel 4 s + kq at s * PB + kq * PA, [xi][ty] rows of 32 floats (18 used):
//   PA = 24 * 32 + 16 = 784, PB = 4 * PA + 8 = 3144, chunk 12 576 floats (50.3 KB), double-buffered.
// Bank arithmetic (MI355X LDS: ds_read_b128 in four 16-lane groups {0-3, 12-15, 20-27}, ... on 64 banks; ds_read_b64 and
// ds_write_b32 in 32-lane halves, the stores on 32 banks):
//   * ds_read_b128: a group holds tile rows {0, 3} of channel kq and {1, 2} of kq + 1 (or the reverse).  16-byte slot of a lane
//     = (kq * 196 + 8 (4 xi + ty) + tx) mod 16 = 4 kq + 8 (ty & 1) + tx: {0-3, 8-11} from one channel, {4-7, 12-15} from the
//     other: CONFLICT-FREE (degree 1);
//   * ds_read_b64 (floats 4 tx + 4, 4 tx + 5): tile rows ty and ty + 2 of a channel fall on the same banks: degree 2 (two extra
//     LDS cycles per wave and K step, 24 of the 1440 cycles of a K step per CU);
//   * staging ds_write_b32: a 32-lane half is 8 pairs x 4 consecutive items; bank = 8 (cp >> 1) + shx (mod 32), the two pairs
//     of a K step share it: degree 2, which a ds_write_b32 hides behind its own data transfer (a row wrap inside the four
//     items keeps it at 2).
// Epilogue.  C layout of a 16 x 16 block: column = lane % 16, row (= tile) = 4 (lane / 16) + register.  (1) the two nu-halves of
// a plane row swap half of their accumulators through the idle image buffers: wave (xi, nh) keeps registers 2 nh, 2 nh + 1
// (tiles (ty = lane / 16, tx = 2 nh + r')) of all six planes nu and runs w4_at over them (rr = the column combinations).  (2) the six
// plane rows of a half meet through LDS in two rounds (two output columns each) as in conv_wino4_kernel: of the ten (block,
// r') items wave xi finishes {0-1, 2-3, 4-5, 6-7, 8, 9}[xi] — one column block per wave (block min(xi, 4)).  Statistics go
// through a StatScratch<4, 80>: waves xi < 4 fill slots nh and (zeros) nh + 2 of their 16 columns, waves xi = 4, 5 the four
// slots of columns 64 - 79; BatchNorm arrival / finalise as everywhere.  Columns >= c_out are zero because their weights are.
// Pixel tiles whose tile_mask is 0 are skipped (rnr_conv2d_masked).
// LDS: 2 x 50.3 KB of T images + 8 KB BatchNorm table + 5 KB statistics scratch = 114 KB of 160.
// Next-tile touch (r10, W8F_PREFETCH / W8F_PF_TOUCH; conv_wino4_kernel's of r05).  With 42 us per tile and one workgroup per CU the
// cold first halo image is a large part of what a tile cannot hide.  Directly behind its K loop — the weight ring and the staging
// registers are dead, the epilogue's LDS rounds cover the returns — workgroup b touches the 18 x 18 halo pixels of block b + 256's
// tile, one pixel per thread, two dwords 128 bytes apart of source 0; block_coords gives that block's tile as it will decode it
// itself (same XCD, same L2, very likely this CU).  What the touch reads of the parameter block it fetches again from the kernel
// arguments (touch_params, conv_stage.inc): held in SGPRs across the K loop the fields cost 116 bytes of scratch at this kernel's
// 168 VGPRs; re-read, the kernel keeps 168 VGPRs, 87 SGPRs, no scratch, and its MFMA / LDS counts, with two more VMEM instructions.
// L22 -2.5 ... -2.8 % at 16 views, -1 % at one; one dword per pixel -2.3 ... -2.5 % (profiles/r10_tile_touch_ab.txt (2) - (4)).

constexpr int W8F_THREADS = 768;
constexpr int W8F_PW = 16, W8F_PH = 16;             // output pixels per workgroup tile (4 x 4 tiles of 4 x 4)
constexpr int W8F_HW = W8F_PW + 2;                  // halo columns
constexpr int W8F_ROWP = 32;                        // floats per T row (18 used)
constexpr int W8F_PA = 24 * W8F_ROWP + 16;          // floats between the four channels of a K step: [xi][ty] rows (+ 16: see the bank arithmetic)
constexpr int W8F_PB = 4 * W8F_PA + 8;              // floats between the K steps of a chunk (+ 8: bank spread of the staging stores)
constexpr int W8F_CHUNK = 4 * W8F_PB;               // floats per staged K block
constexpr int W8F_ITEMS = 4 * W8F_HW * 8;           // staging items per chunk: (tile row, halo column, channel pair) = 576
constexpr int W8F_STAGE_WAVES = W8F_ITEMS / 64;     // 9
#ifndef W8F_BDIST_K
#define W8F_BDIST_K 1               // K steps between the request of a weight block and its MFMAs (1: ring of 2 = 30 registers; 2, 3: ring of 4)
#endif
constexpr int W8F_BDIST = W8F_BDIST_K;
constexpr int W8F_BRING = W8F_BDIST == 1 ? 2 : 4;
#ifndef W8F_SGB
#define W8F_SGB 1                   // VALU instructions placed behind each MFMA by the scheduling pipeline of a K step (0 = the compiler's own order; 2 / 4 spill 8 registers)
#endif
#ifndef W8F_SGB_ST
#define W8F_SGB_ST 3                // ... in the K steps that also stage one channel of the next chunk
#endif
#ifndef W8F_PREFETCH
#define W8F_PREFETCH 256            // > 0: behind the K loop a workgroup touches the halo of block + W8F_PREFETCH's tile (W4_PREFETCH); 0: off
#endif
#ifndef W8F_PF_TOUCH
#define W8F_PF_TOUCH 2              // dwords touched per halo pixel, 128 bytes apart (profiles/r10_tile_touch_ab.txt)
#endif
static_assert(W8F_HW * W8F_HW <= W8F_THREADS, "one touched pixel per thread");
constexpr int W8F_WAVE_FLOATS = 64 * 15;           // weight floats of a wave per K step
constexpr int W8F_STEP_FLOATS = 12 * W8F_WAVE_FLOATS;       // weight image per K step: 36 planes x 4 channels x 80 columns
constexpr int W8F_XHALF = 12 * 15 * 64 * 2;         // floats of the nu-half swap: [wave][nu'][block][lane][2 registers]
constexpr int W8F_XCHG = 12 * 9 * 64 * 2;           // floats of one exchange round: [wave][<= 9 items it does not finish][lane][2]
static_assert(W8F_ITEMS % 64 == 0 && W8F_STAGE_WAVES <= 12, "whole waves stage");
static_assert(2 * W8F_CHUNK >= W8F_XHALF && 2 * W8F_CHUNK >= W8F_XCHG, "the exchange buffers of the epilogue live in the T buffers");
static_assert(W8F_CHUNK < (1 << 14), "the staging destination is packed into 14 bits");
static_assert(W8F_PA % 4 == 0 && W8F_PB % 4 == 0 && W8F_ROWP % 4 == 0, "16-byte aligned row segments");

typedef StatScratch<4, 80> W8FStats;
__host__ __device__ constexpr size_t wino80f4_lds_bytes() {
    return (size_t)(2 * W8F_CHUNK + 2 * W4_BN_MAXC) * sizeof(float) + W8FStats::BYTES;
}

__global__ void __launch_bounds__(W8F_THREADS)
conv_wino80f4_kernel(const ConvParams P) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                       // [2][W8F_CHUNK]; the epilogue's exchange buffers afterwards

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nh = wave / 6, xi = wave - 6 * nh;            // plane-column half, plane row
    const int l15 = lane & 15, kq = lane >> 4;
    const ConvTileId T = conv_tile<W8F_PW, W8F_PH, false>(P);   // one column tile, no split-K: mt alone counts
    const int n = T.n, y0 = T.y0, x0 = T.x0;
    if (P.tile_mask && P.tile_mask[T.mt] == 0) return;      // workgroup-uniform, before any barrier

    // staging item of this thread: (tile row sty, halo column shx, channel pair cp); waves past the items stage nothing
    const int cp = tid & 7;
    const bool stager = wave < W8F_STAGE_WAVES;
    const int sit = stager ? tid >> 3 : 0;
    const int sty = sit / W8F_HW, shx = sit - sty * W8F_HW;
    // source pixels of the six halo rows 4 sty - 1 + r of column x0 - 1 + shx, as one base pixel + two reflection flags
    // (conv_wino4_kernel): rows 1 .. 4 lie inside the map, row 0 reflects at the top border, row 5 at the bottom
    unsigned spix1, sdst;
    {
        const int ix = reflect1(x0 - 1 + shx, P.W);
        const int ya = y0 + 4 * sty;
        spix1 = (unsigned)(ya * P.W + ix);
        const unsigned sflags = (ya == 0 ? 1u << 14 : 0u) | (ya + 4 >= P.H ? 1u << 15 : 0u);
        // channel 2 cp + k = K step cp >> 1, channel 2 (cp & 1) + k of it; + xi * 4 * W8F_ROWP per result, + k * W8F_PA per channel
        sdst = (unsigned)((cp >> 1) * W8F_PB + 2 * (cp & 1) * W8F_PA + sty * W8F_ROWP + shx) | sflags;
    }
    auto spix_of = [&](int r) {
        if (r == 0) return (sdst & (1u << 14)) ? spix1 + (unsigned)P.W : spix1 - (unsigned)P.W;
        if (r == 5) return (sdst & (1u << 15)) ? spix1 + 2u * (unsigned)P.W : spix1 + 4u * (unsigned)P.W;
        return spix1 + (unsigned)((r - 1) * P.W);
    };

    const int nchunks = P.chunks_per_tap;
    // the source of a chunk; scale / shift come from the LDS table (bn)
    struct ChunkSrc : HaloSrc { const float2* bn; };
    float2* s_bn = reinterpret_cast<float2*>(As + 2 * W8F_CHUNK + W8FStats::BYTES / sizeof(float));     // [padded input channel] (scale, shift), behind the float64 statistics scratch
    auto chunk_src = [&](int c) { return ChunkSrc{halo_src<1>(P, n, 0, c, false), s_bn + c * BK + 2 * cp}; };
    typedef float floatx2 __attribute__((ext_vector_type(2)));
    typedef float floatx3 __attribute__((ext_vector_type(3)));
    auto load_a = [&](const ChunkSrc& cs, int r) {
        const unsigned voff = (spix_of(r) * cs.C + 2u * (unsigned)cp) * 4u;
        return __builtin_bit_cast(floatx2, __builtin_amdgcn_raw_buffer_load_b64(cs.rsrc, (int)voff, (int)cs.soff, 0));
    };
    // BatchNorm + activation and the vertical transform of channel k of the pair, 6 LDS stores (one channel per K step)
    auto store_t1 = [&](const ChunkSrc& cs, const floatx2 (&v)[6], float* buf, auto KC) {
        constexpr int k = decltype(KC)::value;
        const float2 t = cs.bn[k];
        float d[6], o[6];
#pragma unroll
        for (int r = 0; r < 6; r++) d[r] = normalize1(k == 0 ? v[r].x : v[r].y, t.x, t.y, cs.act);
        w4_bt(d, o);
        float* a = buf + (sdst & 0x3fffu) + k * W8F_PA;
#pragma unroll
        for (int j = 0; j < 6; j++) a[j * 4 * W8F_ROWP] = o[j];
    };

    // transformed weights: [K step][wave] blocks of 960 floats, three [lane][4] and one [lane][3]; the image carries W8F_BDIST K
    // steps of padding behind the last one, so the look-ahead needs no clamp
    const __amdgpu_buffer_rsrc_t wrsrc = buffer_rsrc(P.weight_wino);
    const unsigned bvoff = (unsigned)lane * 16u;
    const unsigned bvoff3 = 3072u + (unsigned)lane * 12u;
    unsigned bsoff = (unsigned)wave * (unsigned)(W8F_WAVE_FLOATS * 4);
    struct BRegs { floatx4 q[3]; floatx3 t; };
    auto load_b = [&](BRegs& dst) {      // the next K step's block
#pragma unroll
        for (int j = 0; j < 3; j++)
            dst.q[j] = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, (int)(bvoff + 1024u * j), (int)bsoff, 0));
        dst.t = __builtin_bit_cast(floatx3, __builtin_amdgcn_raw_buffer_load_b96(wrsrc, (int)bvoff3, (int)bsoff, 0));
        bsoff += (unsigned)(W8F_STEP_FLOATS * 4);
    };

    // T row of this lane's tile: channel 4 s + kq, row (xi, ty), columns 4 tx .. 4 tx + 5
    const int ty = l15 >> 2, tx = l15 & 3;
    const float* rcur = As + kq * W8F_PA + (xi * 4 + ty) * W8F_ROWP + 4 * tx;
    const float* rnxt = rcur + W8F_CHUNK;
    auto read_row = [&](float (&d)[6], const float* row, int s) {
        const float* p = row + s * W8F_PB;
        const float4 a = *reinterpret_cast<const float4*>(__builtin_assume_aligned(p, 16));
        const float2 b = *reinterpret_cast<const float2*>(p + 4);
        d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w; d[4] = b.x; d[5] = b.y;
    };

    floatx4 acc[3][5];          // [plane nu - 3 nh][column block]
#pragma unroll
    for (int p = 0; p < 3; p++)
#pragma unroll
        for (int b = 0; b < 5; b++) acc[p][b] = floatx4{0.f, 0.f, 0.f, 0.f};

    float* buf_cur = As;
    float* buf_nxt = As + W8F_CHUNK;
    floatx2 avr[6];             // the halo rows of the chunk after the current one, in flight since the chunk before
    {
        const ChunkSrc cs0 = chunk_src(0);
        if (stager) {
#pragma unroll
            for (int r = 0; r < 6; r++) avr[r] = load_a(cs0, r);
        }
        {                       // the BatchNorm table of this view: every padded input channel of both sources
            const int ctot = nchunks * BK;
            for (int ch = tid; ch < ctot; ch += W8F_THREADS) {
                const int sidx = ch < P.chunks0 * BK ? 0 : 1;
                const int cl = ch - (sidx ? P.chunks0 * BK : 0);
                float2 t = make_float2(1.f, 0.f);
                if (P.src_scale[sidx]) t.x = P.src_scale[sidx][(size_t)n * P.src_c[sidx] + cl];
                if (P.src_shift[sidx]) t.y = P.src_shift[sidx][(size_t)n * P.src_c[sidx] + cl];
                s_bn[ch] = t;
            }
        }
        __syncthreads();
        if (stager) {
            store_t1(cs0, avr, buf_cur, std::integral_constant<int, 0>{});
            store_t1(cs0, avr, buf_cur, std::integral_constant<int, 1>{});
            const ChunkSrc cs1 = chunk_src(nchunks > 1 ? 1 : 0);
#pragma unroll
            for (int r = 0; r < 6; r++) avr[r] = load_a(cs1, r);
        }
    }

    // the K loop, instantiated per (staging wave or not, plane-column half)
    auto k_loop = [&](auto STG_, auto NH_) {
        constexpr bool STG = decltype(STG_)::value;
        constexpr int NH = decltype(NH_)::value;
        BRegs breg[W8F_BRING];
#pragma unroll
        for (int k = 0; k < W8F_BDIST; k++) load_b(breg[k]);
        __syncthreads();                    // chunk 0 is staged
        float raw[6], V[6];
        read_row(raw, rcur, 0);

        auto chunk_body = [&](auto NEXT, int c) {
            constexpr bool next_chunk = decltype(NEXT)::value;
            const ChunkSrc cst = chunk_src(next_chunk ? c + 1 : c);                 // stored in this chunk
            const ChunkSrc cld = chunk_src(c + 2 < nchunks ? c + 2 : nchunks - 1);  // requested in this chunk (past the last chunk: a harmless re-read)
#pragma unroll
            for (int s = 0; s < 4; s++) {
                // the next chunk's image is complete and nobody reads the buffer before the current one any more
                if (next_chunk && s == 3) __syncthreads();
                load_b(breg[(s + W8F_BDIST) & (W8F_BRING - 1)]);
                w4_bt(raw, V);                                   // the horizontal half of the input transform (this half's three rows survive)
                if (s < 3) read_row(raw, rcur, s + 1);
                else if (next_chunk) read_row(raw, rnxt, 0);
#pragma unroll
                for (int p = 0; p < 3; p++)
#pragma unroll
                    for (int b = 0; b < 5; b++) {
                        const int e = p * 5 + b;
                        const BRegs& br = breg[s & (W8F_BRING - 1)];
                        const float wv = e < 12 ? br.q[e >> 2][e & 3] : br.t[e - 12];
                        acc[p][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(V[3 * NH + p], wv, acc[p][b], 0, 0, 0);
                    }
                if (STG && next_chunk) {
                    if (s == 0) store_t1(cst, avr, buf_nxt, std::integral_constant<int, 0>{});
                    if (s == 1) store_t1(cst, avr, buf_nxt, std::integral_constant<int, 1>{});
                    if (s == 2) {
#pragma unroll
                        for (int r = 0; r < 6; r++) avr[r] = load_a(cld, r);
                    }
                }
#if W8F_SGB > 0
                // one MFMA, then its share of the step's other work, fifteen times
#pragma unroll
                for (int p = 0; p < 15; p++) {
                    const bool st_step = STG && next_chunk && s < 2;
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // MFMA
                    if (p < 4) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);      // VMEM read: the weight block
                    if (STG && next_chunk && s == 2 && p >= 4 && p < 10) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);    // ... and the halo rows
                    if (st_step && p == 0) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);       // DS read: scale / shift
                    if (st_step) __builtin_amdgcn_sched_group_barrier(0x002, W8F_SGB_ST, 0);        // VALU, staging steps
                    else __builtin_amdgcn_sched_group_barrier(0x002, W8F_SGB, 0);                   // VALU
                    if (p >= 4 && p < 6) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);         // DS read: the row segment
                    if (st_step && p >= 8 && p < 14) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);     // DS write (the staging stores)
                }
#endif
            }
            const float* t = rcur; rcur = rnxt; rnxt = t;
            float* u = buf_cur; buf_cur = buf_nxt; buf_nxt = u;
        };
        for (int c = 0; c + 1 < nchunks; c++) chunk_body(std::true_type{}, c);
        chunk_body(std::false_type{}, nchunks - 1);
    };
    if (nh == 0) k_loop(std::true_type{}, std::integral_constant<int, 0>{});
    else if (stager) k_loop(std::true_type{}, std::integral_constant<int, 1>{});
    else k_loop(std::false_type{}, std::integral_constant<int, 1>{});

#if W8F_PREFETCH
    // Next-tile touch (r10; conv_wino4_kernel's of r05, the reasoning in conv_wino4.inc): behind its K loop a workgroup touches the 18 x 18
    // halo pixels of block + W8F_PREFETCH's tile — the workgroup that gets this CU next, on the same XCD's L2 — one pixel per thread,
    // W8F_PF_TOUCH dwords of source 0's first chunk(s) each, reflected as the staging reflects.  A masked-out successor wastes a touch.
    // The values are never used; the registers stay pinned until the kernel ends.
    unsigned pf[W8F_PF_TOUCH] = {};
    {
        const int b2 = (int)blockIdx.x + W8F_PREFETCH;
        const ConvParams Q = touch_params();
        if (b2 < Q.mtiles * Q.ntiles * Q.zdim && tid < W8F_HW * W8F_HW) {
            const ConvTileId T2 = conv_tile_of_block<W8F_PW, W8F_PH, false>(Q, b2);
            const int hy = tid / W8F_HW, hx = tid - hy * W8F_HW;
            touch_pixel(Q, T2.n, (unsigned)(reflect1(T2.y0 - 1 + hy, Q.H) * Q.W + reflect1(T2.x0 - 1 + hx, Q.W)), pf);
        }
    }
#endif

    // ---- epilogue: Y = A^T M A per (tile, column), statistics, BatchNorm arrival, stores ----
    // (1) the nu-halves of a plane row swap registers: this wave keeps registers 2 nh, 2 nh + 1 of every block and hands the
    // other two of its three planes to its partner (xi, 1 - nh)
    __syncthreads();            // every wave is done with the T images
    float2* xa = reinterpret_cast<float2*>(As);             // [wave][nu'][block][lane]
#pragma unroll
    for (int p = 0; p < 3; p++)
#pragma unroll
        for (int b = 0; b < 5; b++) {
            const float lo = nh ? acc[p][b][0] : acc[p][b][2], hi = nh ? acc[p][b][1] : acc[p][b][3];
            xa[(wave * 15 + p * 5 + b) * 64 + lane] = make_float2(lo, hi);
        }
    __syncthreads();
    // rr[item g = 2 block + r'][bc] = sum_nu A^T[bc][nu] M[xi][nu]: the column combinations of this wave's plane row
    float rr[10][4];
    {
        const int pw = (1 - nh) * 6 + xi;
#pragma unroll
        for (int b = 0; b < 5; b++) {
            float own[3][2], oth[3][2];
#pragma unroll
            for (int p = 0; p < 3; p++) {
                own[p][0] = nh ? acc[p][b][2] : acc[p][b][0];
                own[p][1] = nh ? acc[p][b][3] : acc[p][b][1];
                const float2 v = xa[(pw * 15 + p * 5 + b) * 64 + lane];
                oth[p][0] = v.x; oth[p][1] = v.y;
            }
#pragma unroll
            for (int r = 0; r < 2; r++) {
                float m[6];
#pragma unroll
                for (int p = 0; p < 3; p++) {
                    m[p] = nh ? oth[p][r] : own[p][r];
                    m[3 + p] = nh ? own[p][r] : oth[p][r];
                }
                w4_at(m, rr[2 * b + r]);
            }
        }
    }
    // (2) wave xi of a half finishes items [G0, G1): Y[a][bc] = sum_xi' A^T[a][xi'] rr_xi'[g][bc] over the plane rows of its half
    constexpr int G0[6] = {0, 2, 4, 6, 8, 9}, G1[6] = {2, 4, 6, 8, 9, 10};
    float yv[2][4][4];                      // [item][a][bc]; waves 4, 5 use one item
    float2* xb = reinterpret_cast<float2*>(As);             // [wave][<= 9 items it does not finish][lane]
    const int wbase = nh * 6;
    auto finish = [&](auto F) {
        constexpr int f = decltype(F)::value;
#pragma unroll
        for (int bp = 0; bp < 2; bp++) {    // output columns bc = 2 bp, 2 bp + 1
            __syncthreads();        // round 0: the half swap is read; round 1: the previous exchange
            int k = 0;
#pragma unroll
            for (int g = 0; g < 10; g++) {
                if (g >= G0[f] && g < G1[f]) continue;
                xb[((wbase + f) * 9 + k) * 64 + lane] = make_float2(rr[g][2 * bp], rr[g][2 * bp + 1]);
                k++;
            }
            __syncthreads();
#pragma unroll
            for (int g = G0[f]; g < G1[f]; g++) {
                float m0[6], m1[6];
#pragma unroll
                for (int o = 0; o < 6; o++) {
                    if (o == f) { m0[o] = rr[g][2 * bp]; m1[o] = rr[g][2 * bp + 1]; continue; }
                    // position of item g among the items wave o does not finish
                    const int ko = g < G0[o] ? g : g - (G1[o] - G0[o]);
                    const float2 v = xb[((wbase + o) * 9 + ko) * 64 + lane];
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
    const int g0 = xi < 4 ? 2 * xi : 4 + xi, ng = xi < 4 ? 2 : 1;
    const int blk = g0 >> 1;                // the column block of this wave's items

    static_assert(W8F_CHUNK % 2 == 0, "float64 scratch alignment");
    double* red = W8FStats::red(As + 2 * W8F_CHUNK);        // behind the image / exchange buffers
    const bool with_stats = P.stats != nullptr;
    if (with_stats) {
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int k = 0; k < 2; k++)
            if (k < ng)
#pragma unroll
                for (int a = 0; a < 4; a++)
#pragma unroll
                    for (int b = 0; b < 4; b++) { const double v = yv[k][a][b]; s1 += v; s2 += v * v; }
        s1 += __shfl_xor(s1, 16, 64); s2 += __shfl_xor(s2, 16, 64);
        s1 += __shfl_xor(s1, 32, 64); s2 += __shfl_xor(s2, 32, 64);
        if (kq == 0) {
            // columns 0 - 63: two waves per block (slots nh; nh + 2 hold zeros); columns 64 - 79: four waves
            const int slot = xi < 4 ? nh : (xi - 4) * 2 + nh;
            red[(slot * 80 + 16 * blk + l15) * 2 + 0] = s1;
            red[(slot * 80 + 16 * blk + l15) * 2 + 1] = s2;
            if (xi < 4) {
                red[((slot + 2) * 80 + 16 * blk + l15) * 2 + 0] = 0.0;
                red[((slot + 2) * 80 + 16 * blk + l15) * 2 + 1] = 0.0;
            }
        }
        W8FStats::publish(P, red, n, 0, tid);
    }
    BnArrival arr = {nullptr, 0u};
    const bool bn = with_stats && P.arrive;
    if (bn) arr = bn_arrive(P, n, tid);
    {
        // item g = (block g >> 1, r' = g & 1): tile row kq, tile column 2 nh + r'; outputs (4 kq + a, 4 (2 nh + r') + bc) of the workgroup tile
        float* base = P.out + (((size_t)n * P.OH + y0) * P.OW + x0) * P.c_out_pad;
        const ColumnStore<1, WINO_OUT_AUX, 16> cst(P, base, 0, 16 * blk, l15, 4 * kq * P.OW);
#pragma unroll
        for (int k = 0; k < 2; k++) {
            if (k >= ng) continue;
            const int txr = 2 * nh + ((g0 + k) & 1);
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int b = 0; b < 4; b++) cst.store(yv[k][a][b], 0, (unsigned)(a * P.OW + 4 * txr + b));
        }
    }
    if (bn) bn_complete(P, arr, n, tid, W8FStats::flag(red));
#if W8F_PREFETCH
#pragma unroll
    for (int j = 0; j < W8F_PF_TOUCH; j++) asm volatile("" :: "v"(pf[j]));
#endif
}

// Transformed weights U = G g G^T (w4_weight_u, as pack_weight_wino4_kernel) in the layout of conv_wino80f4_kernel: i enumerates
// [K step][wave = 6 nh + xi][960]: three blocks [lane][4] and one [lane][3], a lane's dword e = 5 (nu - 3 nh) + column block;
// lane = 16 kq + column; K step s4 holds the padded input channels 4 s4 + kq; the W8F_BDIST K steps behind the last one are zeros.
__global__ void __launch_bounds__(256)
pack_weight_wino80f4_kernel(rnr_conv_desc d, const float* __restrict__ w, float* __restrict__ image, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int nsteps = (d.c_in0_pad + d.c_in1_pad) / 4;
    const int wb = (int)(i % W8F_WAVE_FLOATS);
    long r = i / W8F_WAVE_FLOATS;
    const int ln = wb < 768 ? (wb & 255) >> 2 : (wb - 768) / 3;
    const int e = wb < 768 ? (wb >> 8) * 4 + (wb & 3) : 12 + (wb - 768) % 3;
    const int wv = (int)(r % 12);
    const int step = (int)(r / 12);
    if (step >= nsteps) { image[i] = 0.0f; return; }
    const int nu = 3 * (wv / 6) + e / 5, xi = wv % 6;
    const int c = step * 4 + (ln >> 4);
    const int co = (e % 5) * 16 + (ln & 15);
    image[i] = w4_weight_u(d, w, c, co, xi, nu);
}

static void launch_wino80f4(const dim3 grid, const ConvParams& P, hipStream_t st) {
    static bool attr_set = false;
    if (!attr_set) {         // > 64 KiB of dynamic LDS needs the opt-in
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_wino80f4_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)wino80f4_lds_bytes());
        attr_set = true;
    }
    hipLaunchKernelGGL(conv_wino80f4_kernel, grid, dim3(W8F_THREADS), wino80f4_lds_bytes(), st, P);
}
