// Dropout2d in train mode (include/rnr_hip.h, "Dropout2d in train mode"):
//   * rnr_dropout_draw     the multipliers of every dropped layer of a plan, one launch, Philox4x32-10
//   * rnr_dropout_affine   the (scale, shift) a dropped layer's consumers apply
// rnr_conv_out_backward_dropout, the one kernel whose arithmetic dropout changes, is unet_bwd.hip's.  Compiled without FMA
// contraction like the other bit-exact units; nothing here has a sum.
#include "rnr_internal.h"

using namespace rnr;

namespace {

constexpr int DR_THREADS = 256;

struct DrawLayer { float* mult; int channels, c_pad, cbase; float p, keep_scale; };
struct DrawParams {
    DrawLayer layer[RNR_DROPOUT_MAX_LAYERS];
    int num_layers, num_views, c_total;
    unsigned long long seed, offset;
};

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned out[4]) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// one lane per Philox block: four consecutive channels of one (view, layer), one 16-byte store
__global__ void __launch_bounds__(DR_THREADS)
dropout_draw_kernel(const DrawParams P) {
    const int quads = P.c_total >> 2;
    const long t = (long)blockIdx.x * DR_THREADS + threadIdx.x;
    if (t >= (long)P.num_views * quads) return;
    const int n = (int)(t / quads);
    const int col = (int)(t - (long)n * quads) * 4;         // column of the view's row of C_total
    int l = 0;
    while (l + 1 < P.num_layers && col >= P.layer[l + 1].cbase) l++;
    const DrawLayer& Ly = P.layer[l];
    const int c = col - Ly.cbase;
    const unsigned long long b = P.offset + (unsigned long long)t;      // t = i >> 2
    unsigned w[4];
    philox4x32_10((unsigned)b, (unsigned)(b >> 32), 0u, 0x524E5244u, (unsigned)P.seed, (unsigned)(P.seed >> 32), w);
    float m[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const float u = (float)(w[e] >> 8) * 5.9604644775390625e-08f;   // 2^-24: exact
        m[e] = (c + e < Ly.channels && u >= Ly.p) ? Ly.keep_scale : 0.f;
    }
    *reinterpret_cast<float4*>(Ly.mult + (size_t)n * Ly.c_pad + c) = make_float4(m[0], m[1], m[2], m[3]);
}

__global__ void __launch_bounds__(DR_THREADS)
dropout_affine_kernel(const float* scale, const float* shift, const float* mult, float* scale_out, float* shift_out, long quads) {
    const long t = (long)blockIdx.x * DR_THREADS + threadIdx.x;
    if (t >= quads) return;
    const float4 m = reinterpret_cast<const float4*>(mult)[t];
    float4 a = m, b = make_float4(0.f, 0.f, 0.f, 0.f);
    if (scale) {
        const float4 s = reinterpret_cast<const float4*>(scale)[t];
        a = make_float4(m.x * s.x, m.y * s.y, m.z * s.z, m.w * s.w);
    }
    if (shift) {
        const float4 s = reinterpret_cast<const float4*>(shift)[t];
        b = make_float4(m.x * s.x, m.y * s.y, m.z * s.z, m.w * s.w);
    }
    reinterpret_cast<float4*>(scale_out)[t] = a;
    reinterpret_cast<float4*>(shift_out)[t] = b;
}

}  // namespace

extern "C" int rnr_dropout_draw(const rnr_dropout_layer* layers, int num_layers, int num_views, int64_t seed, int64_t offset,
                                void* stream) {
    RNR_REQUIRE(layers && num_layers > 0 && num_views > 0, "rnr_dropout_draw: null layers, or num_layers = %d / num_views = %d not positive",
                num_layers, num_views);
    RNR_REQUIRE(num_layers <= RNR_DROPOUT_MAX_LAYERS, "rnr_dropout_draw: %d layers, at most %d", num_layers, RNR_DROPOUT_MAX_LAYERS);
    DrawParams P = {};
    long c_total = 0;
    for (int l = 0; l < num_layers; l++) {
        const rnr_dropout_layer& s = layers[l];
        RNR_REQUIRE(s.mult && aligned_to(16, {s.mult}), "rnr_dropout_draw: layer %d: mult is null or not 16-byte aligned", l);
        RNR_REQUIRE(s.channels > 0 && s.c_pad >= s.channels && s.c_pad % 16 == 0,
                    "rnr_dropout_draw: layer %d: channels=%d c_pad=%d (c_pad: a multiple of 16, at least channels)", l, s.channels, s.c_pad);
        RNR_REQUIRE(s.p >= 0.f && s.p <= 1.f, "rnr_dropout_draw: layer %d: p = %g outside [0, 1]", l, (double)s.p);
        DrawLayer& d = P.layer[l];
        d.mult = s.mult; d.channels = s.channels; d.c_pad = s.c_pad; d.cbase = (int)c_total; d.p = s.p;
        d.keep_scale = s.p < 1.f ? 1.0f / (1.0f - s.p) : 0.f;
        c_total += s.c_pad;
        RNR_REQUIRE(c_total < (1L << 30), "rnr_dropout_draw: too many channels");
    }
    P.num_layers = num_layers; P.num_views = num_views; P.c_total = (int)c_total;
    P.seed = (unsigned long long)seed; P.offset = (unsigned long long)offset;
    const long lanes = (long)num_views * (c_total / 4);
    RNR_REQUIRE(lanes < (1L << 39), "rnr_dropout_draw: too large");
    hipLaunchKernelGGL(dropout_draw_kernel, dim3((unsigned)((lanes + DR_THREADS - 1) / DR_THREADS)), dim3(DR_THREADS), 0,
                       as_stream(stream), P);
    return check_launch("dropout_draw_kernel");
}

extern "C" int rnr_dropout_affine(const float* scale, const float* shift, const float* mult, float* scale_out, float* shift_out,
                                  int num_views, int c_pad, void* stream) {
    RNR_REQUIRE(mult && scale_out && shift_out, "rnr_dropout_affine: null pointer argument");
    RNR_REQUIRE(num_views > 0 && c_pad > 0 && c_pad % 4 == 0, "rnr_dropout_affine: bad sizes N=%d c_pad=%d (c_pad: a multiple of 4)",
                num_views, c_pad);
    RNR_REQUIRE(aligned_to(16, {scale, shift, mult, scale_out, shift_out}), "rnr_dropout_affine: the tables must be 16-byte aligned");
    const long quads = (long)num_views * (c_pad / 4);
    hipLaunchKernelGGL(dropout_affine_kernel, dim3((unsigned)((quads + DR_THREADS - 1) / DR_THREADS)), dim3(DR_THREADS), 0,
                       as_stream(stream), scale, shift, mult, scale_out, shift_out, quads);
    return check_launch("dropout_affine_kernel");
}
