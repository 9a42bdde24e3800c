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
// column halves = 50 accumulator blocks of 32 x 32.  The six roles r of a half:
//   r = 0..3  "row wave" xi = r + 1:  planes (xi, nu = 0..3) of its half — 4 blocks, 64 accumulator registers;
//   r = 4     "full-row wave" xi = 0: planes (0, nu = 0..4)            — 5 blocks, 80 accumulator registers;
//   r = 5     "column wave":          planes (xi = 1..4, nu = 4)       — 4 blocks, 64 accumulator registers.
// Ten waves x 4 + two waves x 5 = 50.  A wave whose planes share xi needs ONE row segment per K step and the column wave four,
// so the plane row that keeps its fifth plane is the price of one light wave more, and the column wave holds four blocks, not
// five.  Which wave takes which role (W42_ROLE_SIMD, r10; the roles, their accumulators, weight offsets and epilogue places do
// not depend on it, so the output is bit-identical).  Waves go to SIMD w % 4.  Until r09, w = 6 half + r: each SIMD carried two
// row waves and one special wave — 13 / 12 / 13 / 12 MFMAs per K step, but THREE staging waves beside every full-row wave and two
// beside every column wave, and the barrier at the end of a chunk paces all four SIMDs by the slowest.  Now half = w & 1 and SIMD
// 0 / 1 carry the full-row wave (w = 0 / 1), the column wave (4 / 5) and row wave 0 (8 / 9) of half 0 / 1 — 13 MFMAs and TWO
// staging waves — and SIMD 2 / 3 the row waves 1 - 3 (w = 2, 6, 10 / 3, 7, 11) — 12 MFMAs and three staging waves: -1.7 ... -3.1 %
// on every layer of both kernels (profiles/r10_tile_touch_ab.txt (3); the first form of the kernel: 15 / 15 / 10 / 10 MFMAs).
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
constexpr int W42S_STEP_FLOATS = 2 * W42_WAVE_FLOATS;       // ... of conv_wino42s_kernel: [half][1600]
constexpr int W42_XM4 = 8 * 16 * 64;                // floats of the nu = 4 hand-off: [half][xi - 1][register row][lane]
constexpr int W42_XCHG = 10 * 14 * 64 * 2;          // floats of one exchange round: [row wave][<= 14 register rows it does not finish][lane][2]
#ifndef W42_SGB
#define W42_SGB 6                   // VALU instructions behind each MFMA in the scheduling pipeline of a K step (0 / 3 / 4 / 6 / 8 / 12: within 1 %, profiles/r07_wino42p_ab.txt)
#endif
#ifndef W42_SGB_ST
#define W42_SGB_ST 14               // ... in the K steps that also stage one channel of the next chunk
#endif
// Next-tile touch (r10; conv_wino4_kernel's W4_PREFETCH / W4_PF_TOUCH, described in conv_wino42_body.inc).  > 0: behind the K loop
// a workgroup touches the first staged image of block + PREFETCH's tile; 0: off, and the kernel is the one without the code.
// One macro per kernel, because each kernel's default is what its own check decided (profiles/r10_tile_touch_ab.txt (1), (2)); both
// are OFF:
//   conv_wino42p_kernel keeps its registers with the touch (145 VGPRs, 96 SGPRs, no scratch) and misses its layer gate: the four
//     layers -0.03 % in sum with L14 / L16 not faster under the old wave placement, +0.1 ... +8 % under W42_ROLE_SIMD 1 (the
//     classes of a pixel tile already share their input through L2, DESIGN 3.3);
//   conv_wino42s_kernel fails the register check: 143 -> 147 VGPRs in its K loop and its 99 SGPRs at the cap of 100 in every form
//     tried (parameters held or re-read, 1 or 2 dwords, lane index recomputed, block id carried through LDS), and that build
//     measured 0 ... +1.7 % on L3 - L9.
#ifndef W42_PREFETCH
#define W42_PREFETCH 0              // both kernels' at once (an A/B build: -DW42_PREFETCH=256)
#endif
#ifndef W42P_PREFETCH
#define W42P_PREFETCH W42_PREFETCH
#endif
#ifndef W42S_PREFETCH
#define W42S_PREFETCH W42_PREFETCH
#endif
#ifndef W42_PF_TOUCH
#define W42_PF_TOUCH 2              // dwords touched per pixel, 128 bytes apart
#endif
#ifndef W42_ROLE_SIMD
#define W42_ROLE_SIMD 1             // 1: a half's full-row and column wave share a SIMD (r10: -1.7 ... -3.1 % on every layer of both kernels,
                                    // profiles/r10_tile_touch_ab.txt (3)); 0: wave = 6 half + role, the placement of r07 - r09
#endif
constexpr int W42_PF_ROWS = W42_PH + 1;             // rows of a staged image: 17 x W42_COLS pixels, one per thread
static_assert(W42_PF_ROWS * W42_COLS <= W42_THREADS, "one touched pixel per thread");
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

// What differs between the two F(4x4, 2x2) kernels, conv_wino42p_kernel (KIND 2, this file) and conv_wino42s_kernel (KIND 1,
// conv_wino42s.inc); everything else — the transform rows, the K-step roles, the weight ring, the exchange rounds, statistics
// and BatchNorm arrival — is conv_wino42_body.inc, written once and included by both kernels.
//   NPH          K blocks per 16-channel chunk (the stride-2 convolution stages one input parity phase per K block);
//   NSETS        (class, half) weight sets per K step of a column tile;
//   PIX          output pixels between neighbouring positions of the workgroup's tile;
//   item()       base pixel and border flags (bits 14 - 16 of the staging destination) of a staging item;
//   pixel()      source pixel of input row r = 0..4 of an item in the K block `cs` feeds;
//   ZERO_OUTSIDE whether flagged rows / columns are replaced by exactly 0 (the transposed convolution's border).
template <int KIND> struct W42Kind;
template <> struct W42Kind<2> {
    static constexpr int NPH = 1, NSETS = 8, PIX = 2;
    static constexpr bool PARITY_IN_Z = true, ZERO_OUTSIDE = true;
    // source pixels of the five input rows ya - 1 .. ya + 3 of column x0 + px - 1 + shx, as one base pixel + flags.  Rows 1 .. 3 of
    // an item (ya .. ya + 2) always lie inside the map; row 0 falls off the top for the first tile row of class py = 0, row 4 off
    // the bottom for the last of py = 1, the column off either side at the map's edge: the clamped pixel is fetched and the
    // value replaced by exactly 0 (mask), not act(shift)
    static __device__ __forceinline__ void item(const ConvParams& P, const ConvTileId& T, int sty, int shx, unsigned& spix1, unsigned& flags) {
        const int ix = T.x0 + T.px - 1 + shx;
        const int ya = T.y0 + 4 * sty + T.py;
        spix1 = (unsigned)(ya * P.W + min(max(ix, 0), P.W - 1));
        flags = (ya - 1 < 0 ? 1u << 14 : 0u) | (ya + 3 >= P.H ? 1u << 15 : 0u) | (ix >= 0 && ix < P.W ? 1u << 16 : 0u);
    }
    static __device__ __forceinline__ unsigned pixel(const ConvParams& P, const HaloSrc&, unsigned spix1, unsigned flags, int r) {
        if (r == 0) return (flags & (1u << 14)) ? spix1 : spix1 - (unsigned)P.W;
        if (r == 4) return (flags & (1u << 15)) ? spix1 + 2u * (unsigned)P.W : spix1 + 3u * (unsigned)P.W;
        return spix1 + (unsigned)((r - 1) * P.W);
    }
    // pixel (hy < 17, hx < 33) of the input pixels tile T stages per chunk, clamped to the map as item() / pixel() clamp them
    static __device__ __forceinline__ unsigned first_image_pixel(const ConvParams& P, const ConvTileId& T, int hy, int hx) {
        const int iy = min(max(T.y0 + T.py - 1 + hy, 0), P.H - 1), ix = min(max(T.x0 + T.px - 1 + hx, 0), P.W - 1);
        return (unsigned)(iy * P.W + ix);
    }
    static constexpr int PREFETCH = W42P_PREFETCH;
};

__global__ void __launch_bounds__(W42_THREADS)
conv_wino42p_kernel(const ConvParams P) {
    typedef W42Kind<2> K;
#include "conv_wino42_body.inc"
}

// Transformed weights U = G g G^T of the 2x2-tap correlation g of a parity class (taps in increasing input row / column, as
// w2_weight) for the points (0, a, -a, b, inf): G[j] = (1, p_j) / prod_{k != j} (p_j - p_k), G[inf] = (0, 1); float64, rounded
// once.  i enumerates [64-column tile][K step][class][half][1600]: [row wave xi = 1..4][lane = h * 32 + column][nu 0..3], the
// full-row wave's (xi = 0) [lane][nu 0..3] and [lane][nu = 4], then the column wave's [lane][xi 1..4] of plane column nu = 4.  K step = chunk * 8 + s holds the padded input channels
// chunk * 16 + 2 s + h; the W42_BDIST K steps behind the last one are zeros.
// place wb of the 1600 floats of a (class, half): lane, plane row xi, plane column nu
__device__ __forceinline__ void w42_wave_slot(int wb, int& ln, int& xi, int& nu) {
    if (wb < 1024) { xi = (wb >> 8) + 1; ln = (wb & 255) >> 2; nu = wb & 3; }
    else if (wb < 1280) { xi = 0; ln = (wb - 1024) >> 2; nu = wb & 3; }
    else if (wb < 1344) { xi = 0; ln = wb - 1280; nu = 4; }
    else { ln = (wb - 1344) >> 2; xi = ((wb - 1344) & 3) + 1; nu = 4; }
}
// (G g G^T)[xi][nu] of the 2x2-tap correlation g
__device__ __forceinline__ double w42_weight_u(const double (&g)[2][2], int xi, int nu) {
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
    double u = 0.0;
#pragma unroll
    for (int b = 0; b < 2; b++) u += (G[xi][0] * g[0][b] + G[xi][1] * g[1][b]) * G[nu][b];
    return u;
}
__global__ void __launch_bounds__(256)
pack_weight_wino42p_kernel(rnr_conv_desc d, const float* __restrict__ w, float* __restrict__ image, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int nsteps = (d.c_in0_pad + d.c_in1_pad) / 2;
    const int wb = (int)(i % W42_WAVE_FLOATS);
    long r = i / W42_WAVE_FLOATS;
    int ln, xi, nu;
    w42_wave_slot(wb, ln, xi, nu);
    const int col = ln & 31, hh = ln >> 5;
    const int nb = (int)(r & 1); r >>= 1;
    const int cls = (int)(r & 3); r >>= 2;
    const int step = (int)(r % (nsteps + W42_BDIST));
    const int nt = (int)(r / (nsteps + W42_BDIST));
    if (step >= nsteps) { image[i] = 0.0f; return; }
    const int c = (step >> 3) * 16 + 2 * (step & 7) + hh;
    const int co = nt * W42_BN + nb * 32 + col;
    double g[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) g[a][b] = (double)gemm_weight(d, w, cls, (1 - a) * 2 + (1 - b), c, co);
    image[i] = (float)w42_weight_u(g, xi, nu);
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
