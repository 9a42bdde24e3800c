// Backward of the U-Net convolution stack (include/rnr_hip.h, "U-Net backward"), exact fp32 only.
//   * rnr_conv_out_backward[_dropout]  activation + BatchNorm (or bias) backward of one layer: reduce, then apply; with the
//                                      Dropout2d multipliers of a dropped layer
//   * rnr_conv2d_weight_backward       the weight gradient as an implicit GEMM on v_mfma_f32_32x32x2_f32, split over pixels
//   * rnr_conv2d_input_backward_ring   the border pixels of the data gradient, where the forward kernels run on the upstream
//                                      gradient do not give the adjoint of ReflectionPad2d / zero padding
//   * rnr_conv_backward_desc           descriptor of that gradient convolution
//   * rnr_unet_out_backward            tanh backward + NCHW -> padded channel-last
// The data gradients themselves are launches of rnr_conv2d, and the statistics the BatchNorm backward reads are kept by the
// forward's finalise (conv.hip, rnr_bn_finalize_saved).  What has to equal the forward bit for bit — reflection, the
// consumer-side value, descriptor checks, map sizes — is conv_common.h's.  No atomics, no scratch memory; every sum has a
// fixed order.
#include "conv_common.h"

#include <algorithm>

using namespace rnr;

namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------------------------------------
// rnr_conv_out_backward[_dropout]: g_v = mult * (g_z0 + g_z1) * act'(v), mult the Dropout2d multiplier of (view, channel) or 1;
// without mult the slope is taken in float32 (the bits of before), with mult the factor mult * act'(v) is formed and applied in
// float64 (the zeros of a dropped view leave S1 and D of a whole-batch group to the other views' terms alone, where a float32
// rounding per term is no longer small against the result);  reduce S1 = sum g_v, S2 = sum g_v * y per (group, channel) in
// float64 (per-workgroup partials, added in workgroup order), then apply.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int OB_THREADS = 256;
constexpr int OB_MAX_PARTS = 256;     // partial sums per group
constexpr int OB_MAX_CPAD = 1024;    // channel quads of a pixel fit one workgroup

struct OutBwdParams {
    const float* y; const float* scale; const float* shift; const float* mult; const float* gz0; const float* gz1;
    const float* gamma; const double* saved;
    float* gy; float* g_gamma; float* g_beta;
    double* partial;        // [groups][parts][c_pad][2]
    int mode, act, N, channels, c_pad;
    long hw;                // pixels per view
    int groups, parts;
    long group_pixels;      // pixels per group
    long part_pixels;       // pixels per partial sum
    int apply_blocks;       // workgroups per view of the apply launch
};

static int ob_parts(int groups, long group_pixels) {
    long p = std::max(1L, 1024L / groups);
    p = std::min<long>(p, OB_MAX_PARTS);
    p = std::min<long>(p, (group_pixels + 63) / 64);
    return (int)std::max(1L, p);
}

// -> g with g_v = g * f: without dropout g = (g_z0 + g_z1) * act'(v) in float32 and f = 1; with it g = g_z0 + g_z1 and
// f = mult * act'(v) (exact in float64: a product of two float32)
__device__ __forceinline__ float4 ob_grad_v(const OutBwdParams& P, size_t off, int n, int c4, float slope, float4* y_out,
                                            double f[4]) {
    const float4 y = *reinterpret_cast<const float4*>(P.y + off);
    float4 g = *reinterpret_cast<const float4*>(P.gz0 + off);
    if (P.gz1) {
        const float4 g1 = *reinterpret_cast<const float4*>(P.gz1 + off);
        g.x += g1.x; g.y += g1.y; g.z += g1.z; g.w += g1.w;
    }
    float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
    if (P.scale) sc = *reinterpret_cast<const float4*>(P.scale + (size_t)n * P.c_pad + c4);
    if (P.shift) sh = *reinterpret_cast<const float4*>(P.shift + (size_t)n * P.c_pad + c4);
    // torch's convention at v == 0: the derivative is the negative side's slope
    const float d[4] = {(y.x * sc.x + sh.x > 0.f) ? 1.f : slope, (y.y * sc.y + sh.y > 0.f) ? 1.f : slope,
                        (y.z * sc.z + sh.z > 0.f) ? 1.f : slope, (y.w * sc.w + sh.w > 0.f) ? 1.f : slope};
    *y_out = y;
    if (P.mult) {
        const float4 m = *reinterpret_cast<const float4*>(P.mult + (size_t)n * P.c_pad + c4);
        f[0] = (double)m.x * (double)d[0]; f[1] = (double)m.y * (double)d[1];
        f[2] = (double)m.z * (double)d[2]; f[3] = (double)m.w * (double)d[3];
    } else {
        g.x *= d[0]; g.y *= d[1]; g.z *= d[2]; g.w *= d[3];
        f[0] = f[1] = f[2] = f[3] = 1.0;
    }
    return g;
}

__global__ void __launch_bounds__(OB_THREADS)
out_bwd_reduce_kernel(const OutBwdParams P) {
    __shared__ double red[OB_THREADS * 8];
    const int tid = threadIdx.x;
    const int CQ = P.c_pad >> 2;                    // channel quads, <= 256
    const int PL = OB_THREADS / CQ;                 // pixel lanes
    const int q = tid % CQ, pl = tid / CQ;
    const int part = blockIdx.x, group = blockIdx.y;
    const float slope = act_slope(P.act);
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    if (pl < PL) {
        const long p0 = (long)part * P.part_pixels;
        const long p1 = p0 + P.part_pixels < P.group_pixels ? p0 + P.part_pixels : P.group_pixels;
        for (long p = p0 + pl; p < p1; p += PL) {
            const long gp = (long)group * P.group_pixels + p;       // pixel index over the call
            const int n = (int)(gp / P.hw);
            float4 y;
            double f[4];
            const float4 g = ob_grad_v(P, (size_t)gp * P.c_pad + 4 * q, n, 4 * q, slope, &y, f);
            const double gv[4] = {(double)g.x * f[0], (double)g.y * f[1], (double)g.z * f[2], (double)g.w * f[3]};
            s1[0] += gv[0]; s2[0] += gv[0] * (double)y.x;
            s1[1] += gv[1]; s2[1] += gv[1] * (double)y.y;
            s1[2] += gv[2]; s2[2] += gv[2] * (double)y.z;
            s1[3] += gv[3]; s2[3] += gv[3] * (double)y.w;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; e++) {
        red[(tid * 4 + e) * 2 + 0] = s1[e];
        red[(tid * 4 + e) * 2 + 1] = s2[e];
    }
    __syncthreads();
    // pixel lanes are added in lane order by one thread per channel
    for (int c = tid; c < P.c_pad; c += OB_THREADS) {
        double a = 0.0, b = 0.0;
        for (int l = 0; l < PL; l++) {
            const int t = l * CQ + (c >> 2);
            a += red[(t * 4 + (c & 3)) * 2 + 0];
            b += red[(t * 4 + (c & 3)) * 2 + 1];
        }
        double* dst = P.partial + (((size_t)group * P.parts + part) * P.c_pad + c) * 2;
        dst[0] = a;
        dst[1] = b;
    }
}

// S1, S2 of (group, channel): the partials in workgroup order
__device__ __forceinline__ void ob_group_sums(const OutBwdParams& P, int group, int c, double* s1, double* s2) {
    double a = 0.0, b = 0.0;
    const double* src = P.partial + ((size_t)group * P.parts * P.c_pad + c) * 2;
    for (int p = 0; p < P.parts; p++) {
        a += src[(size_t)p * P.c_pad * 2 + 0];
        b += src[(size_t)p * P.c_pad * 2 + 1];
    }
    *s1 = a;
    *s2 = b;
}

__global__ void __launch_bounds__(OB_THREADS)
out_bwd_apply_kernel(const OutBwdParams P) {
    // per channel: mean, gamma * r, S1 / m, r * D / m  (train-mode BatchNorm; eval mode under dropout: gamma * r only)
    __shared__ double coef[OB_MAX_CPAD * 4];
    const int tid = threadIdx.x;
    const int n = blockIdx.y;
    const bool bn_train = P.gamma && P.mode != 2;
    const bool bn_eval_dropped = P.gamma && P.mode == 2 && P.mult;      // scale holds mult: gamma * r from `saved`
    const int group = (P.gamma && P.mode == 0) ? n : 0;
    // ---- parameter gradients: the first workgroups of view 0, one lane per channel, groups in order ----
    if (n == 0) {
        const int c = blockIdx.x * OB_THREADS + tid;
        if (c < P.channels && blockIdx.x * OB_THREADS < P.channels) {
            double gb = 0.0, gg = 0.0;
            for (int g = 0; g < P.groups; g++) {
                double s1, s2;
                ob_group_sums(P, g, c, &s1, &s2);
                gb += s1;
                if (P.gamma) {
                    const double mu = P.saved[((size_t)g * P.c_pad + c) * 2 + 0];
                    const double r = P.saved[((size_t)g * P.c_pad + c) * 2 + 1];
                    gg += r * (s2 - mu * s1);
                }
            }
            if (P.g_beta) P.g_beta[c] = (float)gb;
            if (P.gamma && P.g_gamma) P.g_gamma[c] = (float)gg;
        }
    }
    if (bn_train) {
        const double m = (double)P.group_pixels;
        for (int c = tid; c < P.c_pad; c += OB_THREADS) {
            double mu = 0.0, a = 0.0, cm = 0.0, cd = 0.0;
            if (c < P.channels) {
                double s1, s2;
                ob_group_sums(P, group, c, &s1, &s2);
                mu = P.saved[((size_t)group * P.c_pad + c) * 2 + 0];
                const double r = P.saved[((size_t)group * P.c_pad + c) * 2 + 1];
                a = (double)P.gamma[c] * r;
                cm = s1 / m;
                cd = r * (r * (s2 - mu * s1)) / m;
            }
            coef[c * 4 + 0] = mu; coef[c * 4 + 1] = a; coef[c * 4 + 2] = cm; coef[c * 4 + 3] = cd;
        }
        __syncthreads();
    } else if (bn_eval_dropped) {
        for (int c = tid; c < P.c_pad; c += OB_THREADS)
            coef[c * 4 + 1] = c < P.channels ? (double)P.gamma[c] * P.saved[(size_t)c * 2 + 1] : 0.0;
        __syncthreads();
    }
    const int CQ = P.c_pad >> 2;
    const long total = P.hw * CQ;                               // float4s of this view
    const long per = (total + P.apply_blocks - 1) / P.apply_blocks;
    const long i0 = (long)blockIdx.x * per, i1 = i0 + per < total ? i0 + per : total;
    const float slope = act_slope(P.act);
    for (long i = i0 + tid; i < i1; i += OB_THREADS) {
        const int q = (int)(i % CQ);
        const size_t off = ((size_t)n * P.hw) * P.c_pad + (size_t)i * 4;
        float4 y;
        double mm[4];
        const float4 g = ob_grad_v(P, off, n, 4 * q, slope, &y, mm);
        float r[4] = {g.x, g.y, g.z, g.w};
        const float yy[4] = {y.x, y.y, y.z, y.w};
        if (bn_train) {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const double* k = &coef[(4 * q + e) * 4];
                r[e] = (float)(k[1] * ((double)r[e] * mm[e] - k[2] - ((double)yy[e] - k[0]) * k[3]));
            }
        } else if (bn_eval_dropped) {
#pragma unroll
            for (int e = 0; e < 4; e++) r[e] = (float)(coef[(4 * q + e) * 4 + 1] * ((double)r[e] * mm[e]));
        } else if (P.mult) {            // no BatchNorm: g_y = (float)g_v
#pragma unroll
            for (int e = 0; e < 4; e++) r[e] = (float)((double)r[e] * mm[e]);
        } else if (P.gamma) {        // eval-mode BatchNorm: g_y = a * g_v
            const float4 sc = *reinterpret_cast<const float4*>(P.scale + (size_t)n * P.c_pad + 4 * q);
            r[0] *= sc.x; r[1] *= sc.y; r[2] *= sc.z; r[3] *= sc.w;
        }
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (4 * q + e >= P.channels) r[e] = 0.f;            // padding channels: exactly 0
        *reinterpret_cast<float4*>(P.gy + off) = make_float4(r[0], r[1], r[2], r[3]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// rnr_conv2d_weight_backward.  For one tap:  g_W[co, ci] = sum over anchor pixels p of  g_y[a(p)][co] * X[b(p)][ci]
//   kind 0 / 1: p walks the OUTPUT map, a(p) = p, b(p) = the reflection-padded input pixel of the tap;
//   kind 2    : p walks the INPUT map,  b(p) = p, a(p) = 2 p - 1 + tap (zero outside the output map).
// An MFMA 32x32x2 takes A[i = lane & 31][k = lane >> 5] and B[k][j = lane & 31]: with M = c_out, N = c_in and K = pixels both
// operands of a lane are ONE float of a channel-contiguous row, so LDS holds plain [pixel][channel] rows and a wave reads
// 32 consecutive floats per half.  Workgroup: 4 waves as 2 x 2, each wave (32 WM) x (32 WN) outputs; chunks of WG_KC pixels are
// fetched into registers (affine + activation of X applied there) while the previous chunk is multiplied.
// Grid: (tile, tap) x pixel slice; every slice writes its slab, wg_reduce_kernel adds the slabs in slice order and writes
// torch's layout.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int WG_THREADS = 256;
constexpr int WG_KC = 32;

struct WgParams {
    const float* gy;
    const float* src_data[2]; const float* src_scale[2]; const float* src_shift[2];
    int src_c[2]; int src_act[2];
    float* slabs;           // [slices][taps][c_out_pad][cin_pad]
    int kind, N, H, W, OH, OW, AH, AW;
    int c_out_pad, cin_pad, c_in0_pad;
    int taps, mtiles, ntiles;
    long P;                 // anchor pixels of the call
    long slice;             // anchor pixels per slice (multiple of WG_KC)
};

template <int WM, int WN>
__global__ void __launch_bounds__(WG_THREADS)
wg_kernel(const WgParams P) {
    constexpr int BM = 64 * WM, BN = 64 * WN;
    constexpr int AQ = BM / 4, BQ = BN / 4;                 // float4s per pixel row
    constexpr int AR = WG_KC * AQ / WG_THREADS, BR = WG_KC * BQ / WG_THREADS;
    __shared__ float As[WG_KC * BM];
    __shared__ float Bs[WG_KC * BN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int wm0 = (wave & 1) * 32 * WM, wn0 = (wave >> 1) * 32 * WN;
    int t = blockIdx.x;
    const int tap = t % P.taps; t /= P.taps;
    const int mt = t % P.mtiles, nt = t / P.mtiles;
    const int m0 = mt * BM, n0 = nt * BN;
    const int split = blockIdx.y;
    const long p_begin = (long)split * P.slice;
    const long p_end = p_begin + P.slice < P.P ? p_begin + P.slice : P.P;
    const int KW = P.kind == 0 ? 3 : 4;
    const int ky = tap / KW, kx = tap - ky * KW;
    const long amap = (long)P.AH * P.AW;

    float4 areg[AR], breg[BR];

    auto load_regs = [&](long p0) {
#pragma unroll
        for (int r = 0; r < AR; r++) {
            const int e = tid + WG_THREADS * r;
            const int k = e / AQ, q = e - k * AQ;
            const long gp = p0 + k;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            const int col = m0 + 4 * q;
            if (gp < p_end && col < P.c_out_pad) {
                const int n = (int)(gp / amap);
                const int rem = (int)(gp - (long)n * amap);
                const int ay = rem / P.AW, ax = rem - ay * P.AW;
                int oy = ay, ox = ax;
                bool ok = true;
                if (P.kind == 2) {
                    oy = 2 * ay - 1 + ky; ox = 2 * ax - 1 + kx;
                    ok = oy >= 0 && oy < P.OH && ox >= 0 && ox < P.OW;
                }
                if (ok) v = *reinterpret_cast<const float4*>(P.gy + (((size_t)n * P.OH + oy) * P.OW + ox) * P.c_out_pad + col);
            }
            areg[r] = v;
        }
#pragma unroll
        for (int r = 0; r < BR; r++) {
            const int e = tid + WG_THREADS * r;
            const int k = e / BQ, q = e - k * BQ;
            const long gp = p0 + k;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            const int col = n0 + 4 * q;
            if (gp < p_end && col < P.cin_pad) {
                const int n = (int)(gp / amap);
                const int rem = (int)(gp - (long)n * amap);
                const int ay = rem / P.AW, ax = rem - ay * P.AW;
                int iy = ay, ix = ax;
                if (P.kind == 0) { iy = reflect1(ay + ky - 1, P.H); ix = reflect1(ax + kx - 1, P.W); }
                else if (P.kind == 1) { iy = reflect1(2 * ay + ky - 1, P.H); ix = reflect1(2 * ax + kx - 1, P.W); }
                const int s = col >= P.c_in0_pad ? 1 : 0;
                const int cc = col - (s ? P.c_in0_pad : 0);
                const int C = P.src_c[s];
                v = *reinterpret_cast<const float4*>(P.src_data[s] + (((size_t)n * P.H + iy) * P.W + ix) * C + cc);
                float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
                if (P.src_scale[s]) sc = *reinterpret_cast<const float4*>(P.src_scale[s] + (size_t)n * C + cc);
                if (P.src_shift[s]) sh = *reinterpret_cast<const float4*>(P.src_shift[s] + (size_t)n * C + cc);
                const float slope = act_slope(P.src_act[s]);
                v = make_float4(normalize1_slope(v.x, sc.x, sh.x, slope), normalize1_slope(v.y, sc.y, sh.y, slope),
                                normalize1_slope(v.z, sc.z, sh.z, slope), normalize1_slope(v.w, sc.w, sh.w, slope));
                // transposed kind: a tap that falls outside the output map has no term.  X becomes 0 like g_y above, or a
                // non-finite X would surface as 0 * X in a tap that never reads it
                if (P.kind == 2) {
                    const unsigned oy = 2 * ay - 1 + ky, ox = 2 * ax - 1 + kx;
                    if (oy >= (unsigned)P.OH || ox >= (unsigned)P.OW) v = make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
            breg[r] = v;
        }
    };
    auto store_lds = [&]() {
#pragma unroll
        for (int r = 0; r < AR; r++) *reinterpret_cast<float4*>(&As[(tid + WG_THREADS * r) * 4]) = areg[r];
#pragma unroll
        for (int r = 0; r < BR; r++) *reinterpret_cast<float4*>(&Bs[(tid + WG_THREADS * r) * 4]) = breg[r];
    };

    floatx16 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; i++)
#pragma unroll
        for (int j = 0; j < WN; j++)
#pragma unroll
            for (int g = 0; g < 16; g++) acc[i][j][g] = 0.0f;

    if (p_begin < p_end) load_regs(p_begin);
    for (long p0 = p_begin; p0 < p_end; p0 += WG_KC) {
        store_lds();
        __syncthreads();
        if (p0 + WG_KC < p_end) load_regs(p0 + WG_KC);
#pragma unroll 4
        for (int s = 0; s < WG_KC / 2; s++) {
            const int k = 2 * s + h;
            float a[WM], b[WN];
#pragma unroll
            for (int i = 0; i < WM; i++) a[i] = As[k * BM + wm0 + 32 * i + l31];
#pragma unroll
            for (int j = 0; j < WN; j++) b[j] = Bs[k * BN + wn0 + 32 * j + l31];
#pragma unroll
            for (int i = 0; i < WM; i++)
#pragma unroll
                for (int j = 0; j < WN; j++)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }

    float* slab = P.slabs + ((size_t)split * P.taps + tap) * P.c_out_pad * (size_t)P.cin_pad;
#pragma unroll
    for (int i = 0; i < WM; i++)
#pragma unroll
        for (int g = 0; g < 16; g++) {
            const int row = m0 + wm0 + 32 * i + (g & 3) + 8 * (g >> 2) + 4 * h;
            if (row < P.c_out_pad) {
#pragma unroll
                for (int j = 0; j < WN; j++) {
                    const int col = n0 + wn0 + 32 * j + l31;
                    if (col < P.cin_pad) slab[(size_t)row * P.cin_pad + col] = acc[i][j][g];
                }
            }
        }
}

// slabs in slice order -> torch's layout ([c_out, c_in, k, k]; transposed kind [c_in, c_out, 4, 4]), live channels only
__global__ void __launch_bounds__(256)
wg_reduce_kernel(const float* __restrict__ slabs, float* __restrict__ grad_weight, int kind, int slices, int taps, int c_out,
                 int c_out_pad, int cin_pad, int c_in0, int c_in0_pad, int c_in1, long total) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int col = (int)(idx % cin_pad);
    const int co = (int)((idx / cin_pad) % c_out_pad);
    const int tap = (int)(idx / ((long)cin_pad * c_out_pad));
    const int ci = live_channel(col, c_in0, c_in0_pad, c_in1);
    if (ci < 0 || co >= c_out) return;
    float s = 0.f;
    for (int k = 0; k < slices; k++) s += slabs[(size_t)k * total + idx];
    const int cin = c_in0 + c_in1;
    const size_t o = kind == 2 ? ((size_t)ci * c_out + co) * taps + tap : ((size_t)co * cin + ci) * taps + tap;
    grad_weight[o] = s;
}

struct WgPlan { int wm, wn, mtiles, ntiles, taps, slices; long P, slice; int AH, AW, OH, OW, cin_pad; };

static WgPlan wg_plan(const rnr_conv_desc* d, int num_views, int in_h, int in_w) {
    WgPlan p = {};
    p.taps = d->kind == RNR_CONV3x3_REFLECT ? 9 : 16;
    p.cin_pad = d->c_in0_pad + d->c_in1_pad;
    p.wm = d->c_out_pad > 64 ? 2 : 1;
    p.wn = p.cin_pad > 64 ? 2 : 1;
    p.mtiles = (d->c_out_pad + 64 * p.wm - 1) / (64 * p.wm);
    p.ntiles = (p.cin_pad + 64 * p.wn - 1) / (64 * p.wn);
    p.OH = conv_out_size(d->kind, in_h); p.OW = conv_out_size(d->kind, in_w);
    // anchor pixels: the output map, for the transposed kind the input map
    p.AH = d->kind == RNR_CONVT4x4S2 ? in_h : p.OH; p.AW = d->kind == RNR_CONVT4x4S2 ? in_w : p.OW;
    p.P = (long)num_views * p.AH * p.AW;
    // split the pixels until the grid holds ~4 workgroups per CU (256 CUs); a slice is a whole number of chunks
    const long tiles = (long)p.mtiles * p.ntiles * p.taps;
    const long chunks = (p.P + WG_KC - 1) / WG_KC;
    long want = std::max(1L, std::min<long>(512, (1024 + tiles - 1) / tiles));
    want = std::min(want, chunks);
    p.slice = (chunks + want - 1) / want * WG_KC;
    p.slices = (int)((p.P + p.slice - 1) / p.slice);
    return p;
}

// ---------------------------------------------------------------------------------------------------------------------
// rnr_conv2d_input_backward_ring: the defining sum of the adjoint on the border pixels.  One lane per (ring pixel, input
// channel); the (output pixel, tap) pairs that read the pixel through the padding are enumerated per axis.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool ring_has(int kind, int i, int n) {
    if (kind == 0) return i < 2 || i >= n - 2;
    if (kind == 1) return i == 1 || i == n - 2;
    return i == 0 || i == n - 1;
}
__host__ __device__ __forceinline__ int ring_count(int kind, int n) {
    if (kind == 0) return n < 4 ? n : 4;
    if (kind == 1) return 2;                 // rows 1 and n - 2 (n even: distinct, also for n = 2)
    return n < 2 ? n : 2;
}
__device__ __forceinline__ int ring_coord(int kind, int k, int n) {
    if (kind == 0) return k < 2 ? k : n - ring_count(0, n) + k;
    if (kind == 1) return k == 0 ? 1 : n - 2;
    return k == 0 ? 0 : n - 1;
}
// does output coordinate o with tap k read input coordinate i (of n)?
__device__ __forceinline__ bool ring_reads(int kind, int o, int k, int i, int n) {
    if (kind == 0) return reflect1(o + k - 1, n) == i;
    if (kind == 1) return reflect1(2 * o + k - 1, n) == i;
    return o == 2 * i - 1 + k;
}

struct RingParams {
    const float* gy; const float* weight; float* grad_in;
    int kind, N, H, W, OH, OW, c_out, c_out_pad, cs, cs_pad, ci_off, cin;
    int nrows, ncols;
    long per_view;      // enumerated pixels per view: nrows * W + H * ncols
};

__global__ void __launch_bounds__(256)
ring_kernel(const RingParams P) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)P.N * P.per_view * P.cs_pad) return;
    const int c = (int)(idx % P.cs_pad);
    long rp = idx / P.cs_pad;
    const int n = (int)(rp / P.per_view);
    rp -= (long)n * P.per_view;
    int iy, ix;
    if (rp < (long)P.nrows * P.W) {                         // the ring rows, whole
        iy = ring_coord(P.kind, (int)(rp / P.W), P.H);
        ix = (int)(rp % P.W);
    } else {                                                // the ring columns of the other rows
        rp -= (long)P.nrows * P.W;
        iy = (int)(rp / P.ncols);
        ix = ring_coord(P.kind, (int)(rp % P.ncols), P.W);
        if (ring_has(P.kind, iy, P.H)) return;
    }
    float* dst = P.grad_in + (((size_t)n * P.H + iy) * P.W + ix) * P.cs_pad + c;
    if (c >= P.cs) { *dst = 0.f; return; }
    const int KW = P.kind == 0 ? 3 : 4;
    // candidate output coordinates per axis
    int oy0, oy1, ox0, ox1;
    if (P.kind == 0) { oy0 = iy - 2; oy1 = iy + 2; ox0 = ix - 2; ox1 = ix + 2; }
    else if (P.kind == 1) { oy0 = iy / 2 - 2; oy1 = iy / 2 + 2; ox0 = ix / 2 - 2; ox1 = ix / 2 + 2; }
    else { oy0 = 2 * iy - 1; oy1 = 2 * iy + 2; ox0 = 2 * ix - 1; ox1 = 2 * ix + 2; }
    oy0 = oy0 < 0 ? 0 : oy0; ox0 = ox0 < 0 ? 0 : ox0;
    oy1 = oy1 > P.OH - 1 ? P.OH - 1 : oy1; ox1 = ox1 > P.OW - 1 ? P.OW - 1 : ox1;
    // which (candidate output coordinate, tap) pairs read this pixel: one bit each, at most 5 x 4 per axis
    unsigned my = 0, mx = 0;
    for (int oy = oy0; oy <= oy1; oy++)
        for (int ky = 0; ky < KW; ky++)
            if (ring_reads(P.kind, oy, ky, iy, P.H)) my |= 1u << ((oy - oy0) * KW + ky);
    for (int ox = ox0; ox <= ox1; ox++)
        for (int kx = 0; kx < KW; kx++)
            if (ring_reads(P.kind, ox, kx, ix, P.W)) mx |= 1u << ((ox - ox0) * KW + kx);
    const int ci = P.ci_off + c;
    const int taps = KW * KW;
    // co outermost: the taps of one (co, ci) share a cache line, and the lanes of a wave (consecutive ci) read g_y[co] together
    const float* wbase = P.kind == 2 ? P.weight + (size_t)ci * P.c_out * taps : P.weight + (size_t)ci * taps;
    const size_t wstep = P.kind == 2 ? (size_t)taps : (size_t)P.cin * taps;
    const float* gview = P.gy + (size_t)n * P.OH * P.OW * P.c_out_pad;
    float s = 0.f;
    for (int co = 0; co < P.c_out; co++) {
        const float* w = wbase + (size_t)co * wstep;
        for (unsigned by = my; by; by &= by - 1) {
            const int b = __builtin_ctz(by);
            const int oy = oy0 + b / KW, ky = b - (b / KW) * KW;
            for (unsigned bx = mx; bx; bx &= bx - 1) {
                const int a = __builtin_ctz(bx);
                const int ox = ox0 + a / KW, kx = a - (a / KW) * KW;
                s = fmaf(gview[((size_t)oy * P.OW + ox) * P.c_out_pad + co], w[ky * KW + kx], s);
            }
        }
    }
    *dst = s;
}

__global__ void __launch_bounds__(256)
unet_out_backward_kernel(const float* __restrict__ g_out, const float* __restrict__ out, int apply_tanh,
                         float* __restrict__ g_raw, int n, int c, int h, int w, int c_pad) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long hw = (long)h * w;
    if (idx >= (long)n * hw * c_pad) return;
    const int ch = (int)(idx % c_pad);
    const long pix = idx / c_pad;
    float v = 0.f;
    if (ch < c) {
        const long nn = pix / hw, p = pix - nn * hw;
        const size_t src = ((size_t)nn * c + ch) * hw + p;
        v = g_out[src];
        if (apply_tanh) { const float o = out[src]; v *= 1.0f - o * o; }
    }
    g_raw[idx] = v;
}

static int check_bwd_desc(const rnr_conv_desc* d, const char* who) {
    if (int e = check_desc(d, who)) return e;
    RNR_REQUIRE(!(d->flags & CONV_16BIT_FLAGS), "%s: the backward is exact fp32 only (emulation flags 0x%x)", who,
                d->flags & CONV_16BIT_FLAGS);
    return 0;
}
static int check_bwd_size(const rnr_conv_desc* d, int num_views, int in_h, int in_w, const char* who) {
    if (int e = check_size(d, num_views, in_h, in_w, who)) return e;
    RNR_REQUIRE((long)in_h * in_w * 4 < (1L << 31) && (long)num_views * in_h * in_w * 4 < (1L << 40), "%s: too large", who);
    return 0;
}

}  // namespace

extern "C" size_t rnr_conv_out_backward_workspace_bytes(int num_views, int h, int w, int c_pad) {
    if (num_views <= 0 || h <= 0 || w <= 0 || c_pad <= 0) return 0;
    const long hw = (long)h * w;
    const size_t per_view = (size_t)num_views * ob_parts(num_views, hw);
    const size_t whole = (size_t)ob_parts(1, hw * num_views);
    return std::max(per_view, whole) * c_pad * 2 * sizeof(double) + 256;
}

extern "C" int rnr_conv_out_backward(const float* y, const float* scale, const float* shift, int act, const float* g_z0,
                                     const float* g_z1, const float* gamma, const double* saved, int mode, float* g_y,
                                     float* g_gamma, float* g_beta, int num_views, int h, int w, int channels, int c_pad,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    return rnr_conv_out_backward_dropout(y, scale, shift, nullptr, act, g_z0, g_z1, gamma, saved, mode, g_y, g_gamma, g_beta,
                                         num_views, h, w, channels, c_pad, workspace, workspace_bytes, stream);
}

// (the messages keep rnr_conv_out_backward's name: callers and tests match on it whichever entry point they came through)
extern "C" int rnr_conv_out_backward_dropout(const float* y, const float* scale, const float* shift, const float* mult, int act,
                                             const float* g_z0, const float* g_z1, const float* gamma, const double* saved,
                                             int mode, float* g_y, float* g_gamma, float* g_beta, int num_views, int h, int w,
                                             int channels, int c_pad, void* workspace, size_t workspace_bytes, void* stream) {
    RNR_REQUIRE(y && g_z0 && g_y && workspace, "rnr_conv_out_backward: null pointer argument");
    RNR_REQUIRE(num_views > 0 && h > 0 && w > 0 && channels > 0 && c_pad >= channels && c_pad % 16 == 0 && c_pad <= OB_MAX_CPAD,
                "rnr_conv_out_backward: bad sizes N=%d h=%d w=%d channels=%d c_pad=%d (c_pad: a multiple of 16, at most %d)",
                num_views, h, w, channels, c_pad, OB_MAX_CPAD);
    RNR_REQUIRE(act >= 0 && act <= 2, "rnr_conv_out_backward: unknown activation %d", act);
    RNR_REQUIRE(mode >= 0 && mode <= 2, "rnr_conv_out_backward: unknown mode %d", mode);
    RNR_REQUIRE(!gamma || (saved && scale && shift), "rnr_conv_out_backward: BatchNorm needs saved, scale and shift");
    RNR_REQUIRE(((uintptr_t)workspace & 7) == 0, "rnr_conv_out_backward: workspace must be 8-byte aligned");
    OutBwdParams P = {};
    P.y = y; P.scale = scale; P.shift = shift; P.mult = mult; P.gz0 = g_z0; P.gz1 = g_z1; P.gamma = gamma; P.saved = saved;
    P.gy = g_y; P.g_gamma = g_gamma; P.g_beta = g_beta; P.partial = reinterpret_cast<double*>(workspace);
    P.mode = mode; P.act = act; P.N = num_views; P.channels = channels; P.c_pad = c_pad;
    P.hw = (long)h * w;
    P.groups = (gamma && mode == RNR_BN_BWD_BATCH) ? num_views : 1;
    P.group_pixels = P.groups == 1 ? P.hw * num_views : P.hw;
    P.parts = ob_parts(P.groups, P.group_pixels);
    P.part_pixels = (P.group_pixels + P.parts - 1) / P.parts;
    RNR_REQUIRE((size_t)P.groups * P.parts * c_pad * 2 * sizeof(double) <= workspace_bytes,
                "rnr_conv_out_backward: workspace of %zu bytes is too small", workspace_bytes);
    const long quads = P.hw * (c_pad / 4);
    P.apply_blocks = (int)std::max(1L, std::min(256L, quads / (4 * OB_THREADS)));
    P.apply_blocks = std::max(P.apply_blocks, (channels + OB_THREADS - 1) / OB_THREADS);   // the parameter-gradient lanes
    hipLaunchKernelGGL(out_bwd_reduce_kernel, dim3((unsigned)P.parts, (unsigned)P.groups), dim3(OB_THREADS), 0, as_stream(stream), P);
    if (int e = check_launch("out_bwd_reduce_kernel")) return e;
    hipLaunchKernelGGL(out_bwd_apply_kernel, dim3((unsigned)P.apply_blocks, (unsigned)num_views), dim3(OB_THREADS), 0,
                       as_stream(stream), P);
    return check_launch("out_bwd_apply_kernel");
}

extern "C" size_t rnr_conv2d_weight_backward_workspace_bytes(const rnr_conv_desc* d, int num_views, int in_h, int in_w) {
    if (!d || num_views <= 0 || in_h <= 0 || in_w <= 0 || d->kind < 0 || d->kind > 2) return 0;
    const WgPlan p = wg_plan(d, num_views, in_h, in_w);
    return (size_t)p.slices * p.taps * d->c_out_pad * p.cin_pad * sizeof(float) + 256;
}

extern "C" int rnr_conv2d_weight_backward(const rnr_conv_desc* d, const rnr_conv_src* src0, const rnr_conv_src* src1,
                                          const float* g_y, float* grad_weight, int num_views, int in_h, int in_w,
                                          void* workspace, size_t workspace_bytes, void* stream) {
    if (int e = check_bwd_desc(d, "rnr_conv2d_weight_backward")) return e;
    if (int e = check_bwd_size(d, num_views, in_h, in_w, "rnr_conv2d_weight_backward")) return e;
    RNR_REQUIRE(src0 && src0->data && g_y && grad_weight && workspace, "rnr_conv2d_weight_backward: null pointer argument");
    RNR_REQUIRE(src0->channels == d->c_in0_pad, "rnr_conv2d_weight_backward: src0 has %d channels, descriptor says %d",
                src0->channels, d->c_in0_pad);
    RNR_REQUIRE(d->c_in1_pad == 0 || (src1 && src1->data && src1->channels == d->c_in1_pad),
                "rnr_conv2d_weight_backward: second source missing or channel mismatch");
    RNR_REQUIRE(((uintptr_t)workspace & 15) == 0, "rnr_conv2d_weight_backward: workspace must be 16-byte aligned");
    const WgPlan pl = wg_plan(d, num_views, in_h, in_w);
    const size_t slab = (size_t)pl.taps * d->c_out_pad * pl.cin_pad;
    RNR_REQUIRE(slab * pl.slices * sizeof(float) <= workspace_bytes, "rnr_conv2d_weight_backward: workspace of %zu bytes is too small",
                workspace_bytes);
    RNR_REQUIRE((long)pl.mtiles * pl.ntiles * pl.taps < (1L << 31) && slab < (1UL << 40), "rnr_conv2d_weight_backward: too large");
    WgParams P = {};
    P.gy = g_y;
    P.src_data[0] = src0->data; P.src_scale[0] = src0->scale; P.src_shift[0] = src0->shift;
    P.src_c[0] = src0->channels; P.src_act[0] = src0->act;
    if (d->c_in1_pad) {
        P.src_data[1] = src1->data; P.src_scale[1] = src1->scale; P.src_shift[1] = src1->shift;
        P.src_c[1] = src1->channels; P.src_act[1] = src1->act;
    }
    P.slabs = reinterpret_cast<float*>(workspace);
    P.kind = d->kind; P.N = num_views; P.H = in_h; P.W = in_w; P.OH = pl.OH; P.OW = pl.OW; P.AH = pl.AH; P.AW = pl.AW;
    P.c_out_pad = d->c_out_pad; P.cin_pad = pl.cin_pad; P.c_in0_pad = d->c_in0_pad;
    P.taps = pl.taps; P.mtiles = pl.mtiles; P.ntiles = pl.ntiles; P.P = pl.P; P.slice = pl.slice;
    const dim3 grid((unsigned)(pl.mtiles * pl.ntiles * pl.taps), (unsigned)pl.slices);
    if (pl.wm == 1 && pl.wn == 1) hipLaunchKernelGGL((wg_kernel<1, 1>), grid, dim3(WG_THREADS), 0, as_stream(stream), P);
    else if (pl.wm == 1) hipLaunchKernelGGL((wg_kernel<1, 2>), grid, dim3(WG_THREADS), 0, as_stream(stream), P);
    else if (pl.wn == 1) hipLaunchKernelGGL((wg_kernel<2, 1>), grid, dim3(WG_THREADS), 0, as_stream(stream), P);
    else hipLaunchKernelGGL((wg_kernel<2, 2>), grid, dim3(WG_THREADS), 0, as_stream(stream), P);
    if (int e = check_launch("wg_kernel")) return e;
    const long total = (long)slab;
    hipLaunchKernelGGL(wg_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), P.slabs, grad_weight,
                       d->kind, pl.slices, pl.taps, d->c_out, d->c_out_pad, pl.cin_pad, d->c_in0, d->c_in0_pad, d->c_in1, total);
    return check_launch("wg_reduce_kernel");
}

extern "C" int rnr_conv_backward_desc(const rnr_conv_desc* d, int source, rnr_conv_desc* out) {
    if (int e = check_bwd_desc(d, "rnr_conv_backward_desc")) return e;
    RNR_REQUIRE(out, "rnr_conv_backward_desc: null output");
    RNR_REQUIRE(source == 0 || (source == 1 && d->c_in1_pad > 0), "rnr_conv_backward_desc: no source %d", source);
    rnr_conv_desc b = {};
    b.kind = d->kind == RNR_CONV3x3_REFLECT ? RNR_CONV3x3_REFLECT
             : (d->kind == RNR_CONV4x4S2_REFLECT ? RNR_CONVT4x4S2 : RNR_CONV4x4S2_REFLECT);
    b.c_in0 = d->c_out; b.c_in0_pad = d->c_out_pad;
    b.c_out = source ? d->c_in1 : d->c_in0;
    b.c_out_pad = source ? d->c_in1_pad : d->c_in0_pad;
    // the forward's algorithm choice carries over: Winograd if it has it, the F(4x4, .) form of the gradient's own kind if the
    // forward has any, under the column rules of each flag (include/rnr_hip.h)
    if (d->flags & RNR_CONV_WINOGRAD) {
        b.flags |= RNR_CONV_WINOGRAD;
        if (d->flags & (RNR_CONV_WINOGRAD4 | RNR_CONV_WINOGRAD42 | RNR_CONV_WINOGRAD4_OUT | RNR_CONV_WINOGRAD42S)) {
            if (b.kind == RNR_CONV3x3_REFLECT && b.c_out_pad % 64 == 0) b.flags |= RNR_CONV_WINOGRAD4;
            if (b.kind == RNR_CONV3x3_REFLECT && b.c_out_pad == 80) b.flags |= RNR_CONV_WINOGRAD4_OUT;
            if (b.kind == RNR_CONVT4x4S2 && b.c_out_pad % 64 == 0) b.flags |= RNR_CONV_WINOGRAD42;
            if (b.kind == RNR_CONV4x4S2_REFLECT && b.c_out_pad % 64 == 0) b.flags |= RNR_CONV_WINOGRAD42S;
        }
    }
    *out = b;
    return 0;
}

extern "C" int rnr_conv2d_input_backward_ring(const rnr_conv_desc* d, int source, const float* g_y, const float* weight,
                                              float* grad_in, int num_views, int in_h, int in_w, void* stream) {
    if (int e = check_bwd_desc(d, "rnr_conv2d_input_backward_ring")) return e;
    if (int e = check_bwd_size(d, num_views, in_h, in_w, "rnr_conv2d_input_backward_ring")) return e;
    RNR_REQUIRE(g_y && weight && grad_in, "rnr_conv2d_input_backward_ring: null pointer argument");
    RNR_REQUIRE(source == 0 || (source == 1 && d->c_in1_pad > 0), "rnr_conv2d_input_backward_ring: no source %d", source);
    RingParams P = {};
    P.gy = g_y; P.weight = weight; P.grad_in = grad_in;
    P.kind = d->kind; P.N = num_views; P.H = in_h; P.W = in_w;
    P.OH = conv_out_size(d->kind, in_h); P.OW = conv_out_size(d->kind, in_w);
    P.c_out = d->c_out; P.c_out_pad = d->c_out_pad;
    P.cs = source ? d->c_in1 : d->c_in0;
    P.cs_pad = source ? d->c_in1_pad : d->c_in0_pad;
    P.ci_off = source ? d->c_in0 : 0;
    P.cin = d->c_in0 + d->c_in1;
    P.nrows = ring_count(d->kind, in_h);
    P.ncols = ring_count(d->kind, in_w);
    P.per_view = (long)P.nrows * in_w + (long)in_h * P.ncols;
    const long total = (long)num_views * P.per_view * P.cs_pad;
    RNR_REQUIRE(total < (1L << 39), "rnr_conv2d_input_backward_ring: too large");
    hipLaunchKernelGGL(ring_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), P);
    return check_launch("ring_kernel");
}

extern "C" int rnr_unet_out_backward(const float* g_out, const float* out, int apply_tanh, float* g_raw, int n, int c, int h,
                                     int w, int c_pad, void* stream) {
    RNR_REQUIRE(g_out && g_raw && (out || !apply_tanh), "rnr_unet_out_backward: null pointer argument");
    RNR_REQUIRE(n > 0 && c > 0 && h > 0 && w > 0 && c_pad >= c, "rnr_unet_out_backward: bad sizes");
    const long total = (long)n * h * w * c_pad;
    RNR_REQUIRE(total < (1L << 39), "rnr_unet_out_backward: too large");
    hipLaunchKernelGGL(unet_out_backward_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), g_out, out,
                       apply_tanh, g_raw, n, c, h, w, c_pad);
    return check_launch("unet_out_backward_kernel");
}
