// Winograd F(4x4, 2x2) for the 4x4 stride-2 convolution of the U-Net (KIND 1; descriptor flag RNR_CONV_WINOGRAD42S), exact-fp32
// operands on v_mfma_f32_32x32x2_f32.  Included by conv.hip behind conv_wino42p.inc, whose kernel body (conv_wino42_body.inc) it shares:
// the transform rows (w42_bt / w42_at, points (0, +-3/4, 2, inf)), the wave roles, the weight ring, the exchange rounds, the
// statistics and the BatchNorm arrival are written there, once.  This file holds what the stride-2 convolution does differently:
// where a staging item reads (W42Kind<1>), the weight image and the launch.
//
// ReflectionPad2d(1) + Conv2d 4x4 s2 = the sum over the four input parity phases p = (phy, phx) of a 2x2-tap correlation of the
// phase image D_p (conv_wino2.inc):
//   out[y][x] = sum_p sum_{a,b in {0,1}} D_p[y + a][x + b] g_p[a][b],   D_p[r][c] = in[reflect1(2 r - phy)][reflect1(2 c - phx)].
// F(4, 2) tile t (outputs 4 t .. 4 t + 3) reads D_p[4 t .. 4 t + 4]; nested, 25 multiplications per 4 x 4 outputs and phase where
// F(2x2, 2x2) takes 36: 30.6 % fewer MFMAs than conv_wino2_kernel<1>.  All four phases accumulate into ONE set of accumulators
// (K = 4 c_in, K order (chunk, phase) as in conv_wino2_kernel<1>), every input pixel is staged once per workgroup and the stores
// go to contiguous pixels.
//
// Mapping: conv_wino42p_kernel's.  A 12-wave workgroup owns 32 x 16 OUTPUT pixels x 64 columns = 25 planes x 2 column halves =
// 50 accumulator blocks; row waves, full-row wave and column wave as there.  A K block stages the 17 x 33 pixels of one phase
// image of one 16-channel chunk: item (tile row, column, channel quad) loads rows 4 sty .. 4 sty + 4 of D_p in its column and
// stores B^T of them.  Source pixels are addressed as w2_slot does: reflection only ever moves row 2 Ho = H to H - 2 (phy = 0,
// the last row of the last tile row), row -1 to 1 (phy = 1, the first row of the first tile row) and the same for columns, so an
// item keeps the pixel of (row 2 ya, phase-0 column) and three flag bits, and the phase of the K block (wave-uniform) picks the
// offsets.  Row segments start at column 4 tx whatever the phase.
//
// LDS row stride: W42_ROWP = 36 floats, conv_wino42p_kernel's image, kept on purpose.  By the bank rule of conv_wino80f4.inc
// (ds_read_b128 served in 16-lane groups {0-3, 12-15, 20-27} / {4-11, 16-19, 28-31} over 64 banks; conflict-free when the
// sixteen 16-byte slots (ROWP / 4 * ty + tx) mod 16 of a group differ) a group holds tile rows ty = 0, 3 at tx 0-3 and ty = 1, 2
// at tx 4-7, which is conflict-free only for ROWP = 32 (mod 64) — 33 staged columns rule 32 out and 96 does not fit LDS twice.
// Of the strides that do fit (36, 40, 44, 48: 16-byte aligned segments need a multiple of 4) 36 gives degree 2 (slots {0-3},
// {13-0}, {6-9}, {11-14}), 40 and 44 degree 3, 48 degree 2 with 12 KB more per buffer.  The fifth float of a segment is a
// ds_read_b32 at a stride of four floats between neighbouring tiles: 16 of the 64 banks whatever the row stride — the conflicts
// conv_wino42p_kernel measured (5.9 cycles per LDS instruction) and this kernel inherits; moving that column out of the row is
// recorded as the next step in DESIGN section 8, not taken here, because it changes the K loop both kernels share.

template <> struct W42Kind<1> {
    static constexpr int NPH = 4, NSETS = 2, PIX = 1;
    static constexpr bool PARITY_IN_Z = false, ZERO_OUTSIDE = false;
    // item (sty, shx): rows ya .. ya + 4 (ya = y0 + 4 sty), column xa = x0 + shx of the phase images.  spix1 = the pixel of
    // (row 2 ya, phase-0 column); bit 14: ya = 0 (phase-1 row -1 reflects to 1), bit 15: ya + 4 = Ho (phase-0 row H reflects to
    // H - 2), bit 16: the phase-1 column lies RIGHT of the phase-0 column (xa = 0: -1 -> 1; xa = Wo: phase 0 reads W - 2)
    static __device__ __forceinline__ void item(const ConvParams& P, const ConvTileId& T, int sty, int shx, unsigned& spix1, unsigned& flags) {
        const int ya = T.y0 + 4 * sty, xa = T.x0 + shx;
        const int c0 = xa == P.Wo ? P.W - 2 : 2 * xa;
        spix1 = (unsigned)(2 * ya * P.W + c0);
        flags = (ya == 0 ? 1u << 14 : 0u) | (ya + 4 == P.Ho ? 1u << 15 : 0u) | (xa == 0 || xa == P.Wo ? 1u << 16 : 0u);
    }
    // row r of the item in phase (cs.phy, cs.phx): input row 2 (ya + r) - phy, reflected
    static __device__ __forceinline__ unsigned pixel(const ConvParams& P, const HaloSrc& cs, unsigned spix1, unsigned flags, int r) {
        unsigned p = spix1;
        if (cs.phx) p += (flags & (1u << 16)) ? 1u : ~0u;
        const unsigned W = (unsigned)P.W;
        if (cs.phy) return r == 0 ? ((flags & (1u << 14)) ? p + W : p - W) : p + (unsigned)(2 * r - 1) * W;
        return r == 4 ? ((flags & (1u << 15)) ? p + 6u * W : p + 8u * W) : p + (unsigned)(2 * r) * W;
    }
    // pixel (hy < 17, hx < 33) of phase image 0 of tile T, the first image it stages: D_0[y0 + hy][x0 + hx]
    static __device__ __forceinline__ unsigned first_image_pixel(const ConvParams& P, const ConvTileId& T, int hy, int hx) {
        return (unsigned)(reflect1(2 * (T.y0 + hy), P.H) * P.W + reflect1(2 * (T.x0 + hx), P.W));
    }
    static constexpr int PREFETCH = W42S_PREFETCH;
};

__global__ void __launch_bounds__(W42_THREADS)
conv_wino42s_kernel(const ConvParams P) {
    typedef W42Kind<1> K;
#include "conv_wino42_body.inc"
}

// Transformed weights U = G g_phase G^T (G as in pack_weight_wino42p_kernel; the taps of a phase as in w2_weight<1>), float64,
// rounded once.  i enumerates [64-column tile][K step][half][1600] with conv_wino42p_kernel's 1600-float wave layout; K step =
// ((chunk * 4 + phase) * 8 + s) holds the padded input channels chunk * 16 + 2 s + h; the W42_BDIST K steps behind the last one
// are zeros.
__global__ void __launch_bounds__(256)
pack_weight_wino42s_kernel(rnr_conv_desc d, const float* __restrict__ w, float* __restrict__ image, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int nsteps = (d.c_in0_pad + d.c_in1_pad) / 2 * 4;
    int ln, xi, nu;
    w42_wave_slot((int)(i % W42_WAVE_FLOATS), ln, xi, nu);
    long r = i / W42_WAVE_FLOATS;
    const int col = ln & 31, hh = ln >> 5;
    const int nb = (int)(r & 1); r >>= 1;
    const int step = (int)(r % (nsteps + W42_BDIST));
    const int nt = (int)(r / (nsteps + W42_BDIST));
    if (step >= nsteps) { image[i] = 0.0f; return; }
    const int kb = step >> 3, phase = kb & 3;
    const int c = (kb >> 2) * 16 + 2 * (step & 7) + hh;
    const int co = nt * W42_BN + nb * 32 + col;
    const int phy = phase >> 1, phx = phase & 1;
    double g[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) g[a][b] = (double)gemm_weight(d, w, 0, (phy ? 2 * a : 1 + 2 * a) * 4 + (phx ? 2 * b : 1 + 2 * b), c, co);
    image[i] = (float)w42_weight_u(g, xi, nu);
}

static void launch_wino42s(const dim3 grid, const ConvParams& P, hipStream_t st) {
    static bool attr_set = false;
    if (!attr_set) {         // > 64 KiB of dynamic LDS needs the opt-in
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_wino42s_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)wino42p_lds_bytes());
        attr_set = true;
    }
    hipLaunchKernelGGL(conv_wino42s_kernel, grid, dim3(W42_THREADS), wino42p_lds_bytes(), st, P);
}
