// What the convolution kernels (conv.hip and its .inc files) and their backward (unet_bwd.hip) must state identically: the
// backward recomputes the forward's consumer-side values and BatchNorm affine and has to get the same bits, so each formula
// lives here once.  Both files are compiled with the same flags (Makefile, CONVFLAGS).
#pragma once
#include "rnr_internal.h"

namespace rnr {

constexpr int BK = 16;      // channels per K chunk of the implicit GEMM: every channel count is padded to a multiple

__device__ __forceinline__ int reflect1(int i, int n) {   // ReflectionPad2d(1)
    i = i < 0 ? -i : i;
    return i >= n ? 2 * n - 2 - i : i;
}

// act(v) = max(v, slope * v) with slope = 1 (none), 0.2 (LeakyReLU 0.2), 0 (ReLU): branch-free, wave-uniform slope
__device__ __forceinline__ float act_slope(int act) {
    return act == RNR_ACT_LRELU02 ? 0.2f : (act == RNR_ACT_RELU ? 0.0f : 1.0f);
}
__device__ __forceinline__ float act_value(float v, float slope) { return fmaxf(v, slope * v); }
__device__ __forceinline__ float apply_act(float v, int act) { return act_value(v, act_slope(act)); }
// the value a consumer reads: the producer's BatchNorm (+ bias) and activation on its raw output; normalize1_slope for the
// callers that hold act_slope(act) already
__device__ __forceinline__ float normalize1_slope(float x, float sc, float sh, float slope) { return act_value(x * sc + sh, slope); }
__device__ __forceinline__ float normalize1(float x, float sc, float sh, int act) { return normalize1_slope(x, sc, sh, act_slope(act)); }

// BatchNorm's affine from a channel's statistics: biased variance clamped at 0, float64, one rounding to float32
struct BnAffine { double mean, var; float scale, shift; };
__device__ __forceinline__ BnAffine bn_affine(double s1, double s2, double count, float gamma, float beta, float eps) {
    const double mean = s1 / count;
    double var = s2 / count - mean * mean;
    var = var < 0.0 ? 0.0 : var;
    const double g = (double)gamma / sqrt(var + (double)eps);
    return {mean, var, (float)g, (float)((double)beta - mean * g)};
}
// torch.nn.BatchNorm2d in train mode also moves its running statistics: momentum, UNBIASED variance
__device__ __forceinline__ void bn_update_running(const BnAffine& a, double count, float momentum, float* running_mean,
                                                  float* running_var, int c) {
    if (running_mean) running_mean[c] = (float)((1.0 - (double)momentum) * (double)running_mean[c] + (double)momentum * a.mean);
    if (running_var) {
        const double unb = count > 1.0 ? a.var * count / (count - 1.0) : a.var;
        running_var[c] = (float)((1.0 - (double)momentum) * (double)running_var[c] + (double)momentum * unb);
    }
}

// output map size, per axis, of a convolution of `kind` on an input of `in` pixels
__host__ __device__ __forceinline__ int conv_out_size(int kind, int in) {
    return kind == RNR_CONV3x3_REFLECT ? in : (kind == RNR_CONV4x4S2_REFLECT ? in / 2 : 2 * in);
}

// live input channel (index into torch's weight, the two sources concatenated) of padded column c, -1 for a padding column
__host__ __device__ __forceinline__ int live_channel(int c, int c_in0, int c_in0_pad, int c_in1) {
    int ci = -1;
    if (c < c_in0_pad) { if (c < c_in0) ci = c; }
    else if (c - c_in0_pad < c_in1) ci = c_in0 + c - c_in0_pad;
    return ci;
}

// the flags whose convolutions run conv_halo_emu_kernel on the 16-bit matrix cores: the two fp32 emulations and plain fp16
constexpr int CONV_16BIT_FLAGS = RNR_CONV_F32_EMU_ANY | RNR_CONV_F16;

// the refusals every entry point that takes a descriptor shares
inline int check_desc(const rnr_conv_desc* d, const char* who) {
    RNR_REQUIRE(d, "%s: null descriptor", who);
    RNR_REQUIRE(d->kind >= 0 && d->kind <= 2, "%s: unknown kind %d", who, d->kind);
    RNR_REQUIRE(d->c_in0 > 0 && d->c_in0_pad >= d->c_in0 && d->c_in0_pad % BK == 0,
                "%s: c_in0 %d / pad %d (pad must be a multiple of %d)", who, d->c_in0, d->c_in0_pad, BK);
    RNR_REQUIRE(d->c_in1 >= 0 && d->c_in1_pad >= d->c_in1 && d->c_in1_pad % BK == 0,
                "%s: c_in1 %d / pad %d", who, d->c_in1, d->c_in1_pad);
    RNR_REQUIRE(d->c_out > 0 && d->c_out_pad >= d->c_out && d->c_out_pad % BK == 0,
                "%s: c_out %d / pad %d", who, d->c_out, d->c_out_pad);
    RNR_REQUIRE((d->flags & ~(RNR_CONV_STATS_PREZEROED | CONV_16BIT_FLAGS | RNR_CONV_WINOGRAD | RNR_CONV_WINOGRAD4 |
                              RNR_CONV_WINOGRAD42 | RNR_CONV_WINOGRAD4_OUT | RNR_CONV_WINOGRAD42S)) == 0,
                "%s: unknown flags 0x%x", who, d->flags);
    RNR_REQUIRE(!(d->flags & RNR_CONV_WINOGRAD4) || (d->flags & RNR_CONV_WINOGRAD),
                "%s: RNR_CONV_WINOGRAD4 goes with RNR_CONV_WINOGRAD (its fallback for the shapes it does not cover)", who);
    RNR_REQUIRE(!(d->flags & RNR_CONV_WINOGRAD42) || (d->flags & RNR_CONV_WINOGRAD),
                "%s: RNR_CONV_WINOGRAD42 goes with RNR_CONV_WINOGRAD (its fallback for the shapes it does not cover)", who);
    RNR_REQUIRE(!(d->flags & RNR_CONV_WINOGRAD42S) || (d->flags & RNR_CONV_WINOGRAD),
                "%s: RNR_CONV_WINOGRAD42S goes with RNR_CONV_WINOGRAD (its fallback for the shapes it does not cover)", who);
    RNR_REQUIRE(!(d->flags & RNR_CONV_WINOGRAD4_OUT) || (d->flags & RNR_CONV_WINOGRAD),
                "%s: RNR_CONV_WINOGRAD4_OUT goes with RNR_CONV_WINOGRAD (its fallback for the shapes it does not cover)", who);
    RNR_REQUIRE((d->flags & RNR_CONV_F32_EMU_ANY) != RNR_CONV_F32_EMU_ANY, "%s: choose ONE emulation format", who);
    RNR_REQUIRE(!(d->flags & RNR_CONV_F16) || !(d->flags & RNR_CONV_F32_EMU_ANY),
                "%s: RNR_CONV_F16 is a precision of its own, not combined with the emulation formats (flags 0x%x)", who,
                d->flags & CONV_16BIT_FLAGS);
    RNR_REQUIRE(!(d->flags & RNR_CONV_WINOGRAD) || !(d->flags & CONV_16BIT_FLAGS),
                "%s: RNR_CONV_WINOGRAD is an exact-fp32 algorithm, not combined with the emulation formats or RNR_CONV_F16", who);
    return 0;
}
// The upper size limits of a convolution call (include/rnr_hip.h, "Size limits"): what the kernels and the planner hold in an
// int or in a 32-bit buffer offset.  Null when the sizes fit, else the limit they break — for check_size's message and for the
// host queries, which return their error value instead of planning with a wrapped int.
//   pixels per view            H * W < 2^31                    the pixel index inside a view (halo_pixel, the gather kernel's rows)
//   GEMM rows, output pixels   N * H * W, N * OH * OW < 2^31   ConvPlan::M, mtiles, the tile decode, the split-K reduce's rows per view
//   one band of output rows    64 * OW * c_out_pad * 4 < 2^31  ColumnStore's offsets behind a tile's first pixel (a tile spans at most
//                                                              33 output rows), which must stay below the offset the stores drop
//   statistics                 N * c_out_pad < 2^24            bn_finalize_views' byte offsets into the eight statistics shards
// (conv.hip adds what needs the plan or the packed layout: the workgroup count, the packed weight below 2^31 bytes, a source view
// of 2^31 bytes or more)
constexpr long CONV_INT_MAX = 0x7fffffffL;
inline const char* conv_size_limit(const rnr_conv_desc* d, int num_views, int in_h, int in_w) {
    // (the output size in long: conv_out_size doubles the transposed kind's map in an int)
    const long N = num_views, hw = (long)in_h * in_w, up = d->kind == RNR_CONVT4x4S2 ? 2 : 1;
    const long oh = d->kind == RNR_CONV4x4S2_REFLECT ? in_h / 2 : up * in_h, ow = d->kind == RNR_CONV4x4S2_REFLECT ? in_w / 2 : up * in_w;
    if (hw > CONV_INT_MAX) return "H * W pixels per view do not fit the 32-bit pixel index";
    const long ohw = oh * ow;                       // <= 4 H W: no long overflows below
    if (N * hw > CONV_INT_MAX || N * ohw > CONV_INT_MAX) return "N * H * W or N * OH * OW does not fit an int";
    if (ow * d->c_out_pad > CONV_INT_MAX / 256)     // 64 rows x 4 bytes
        return "64 output rows of OW * c_out_pad floats do not fit a 32-bit byte offset";
    if (N * d->c_out_pad >= (1L << 24)) return "N * c_out_pad statistics do not fit a 32-bit byte offset";
    return nullptr;
}
inline int check_size(const rnr_conv_desc* d, int num_views, int in_h, int in_w, const char* who) {
    const int min_hw = d->kind == RNR_CONVT4x4S2 ? 1 : 2;   // ReflectionPad2d(1) needs >= 2 pixels
    RNR_REQUIRE(num_views > 0 && in_h >= min_hw && in_w >= min_hw, "%s: bad sizes N=%d H=%d W=%d", who, num_views, in_h, in_w);
    RNR_REQUIRE(d->kind != RNR_CONV4x4S2_REFLECT || (in_h % 2 == 0 && in_w % 2 == 0), "%s: stride-2 conv needs even input size",
                who);
    const char* limit = conv_size_limit(d, num_views, in_h, in_w);
    RNR_REQUIRE(!limit, "%s: too large (N=%d H=%d W=%d, c_out_pad %d): %s", who, num_views, in_h, in_w, d->c_out_pad, limit);
    return 0;
}

}  // namespace rnr
