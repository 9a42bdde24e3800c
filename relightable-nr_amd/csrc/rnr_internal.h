// Internal helpers shared by the HIP translation units of librnr_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <initializer_list>

#include "../../include/rnr_hip.h"

namespace rnr {

// thread-local last-error text (rnr_last_error)
char* err_buf();
int fail(const char* fmt, ...);

inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail("%s: %s", what, hipGetErrorString(e));
    return 0;
}

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// raster.hip: the regions of an rnr_rasterize_gbuffer workspace that are cleared per call (for rnr_frame_prepare)
void gbuffer_clear_regions(void* workspace, int num_views, int num_faces, int image_size, uint4** counters, long* counter_vec,
                           uint4** keys, long* key_vec);

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// every pointer of the list (NULL: an optional operand left out) is a multiple of `bytes`: the alignment contract of rnr_hip.h,
// checked by the entry points before any launch
inline bool aligned_to(size_t bytes, std::initializer_list<const void*> ptrs) {
    uintptr_t bits = 0;
    for (const void* p : ptrs) bits |= (uintptr_t)p;
    return bits % bytes == 0;
}

#define RNR_REQUIRE(cond, ...)                     \
    do {                                           \
        if (!(cond)) return rnr::fail(__VA_ARGS__); \
    } while (0)

#define RNR_HIP(call)                                                                  \
    do {                                                                               \
        hipError_t e__ = (call);                                                       \
        if (e__ != hipSuccess) return rnr::fail("%s: %s", #call, hipGetErrorString(e__)); \
    } while (0)

#if defined(__HIPCC__)
// Sum of v over a workgroup of WAVES full waves in a fixed order (shuffle tree per wave, then the waves in order); the result is
// valid in thread 0.  `sh` holds WAVES doubles; the leading barrier lets consecutive calls share it.  (metric.hip, loss.hip)
template <int WAVES>
__device__ __forceinline__ double block_sum(double v, double* sh) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < WAVES; i++) t += sh[i];
    return t;
}

// tanh(x) + 1 = 2 - 2 / (e^{2x} + 1) on v_exp_f32 / v_rcp_f32 (the light transport factor of the ray renderer): absolute
// error ~1e-7, exact limits at +-inf; ocml's tanhf costs ~25 instructions and this kernel is VALU-bound.
__device__ __forceinline__ float fast_tanh_plus1f(float x) {
    const float e = __builtin_amdgcn_exp2f(x * 2.8853900817779268f);
    return __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(e + 1.0f), 2.0f);
}

// One axis of the INTER_AREA box filter (OpenCV's computeResizeAreaTab, restated in shade.hip above resize_area_kernel): output
// cell d covers [d*scale, (d+1)*scale) of a source axis of ssize pixels; pixel s1 - 1 weighs a_first, s1 .. s2 - 1 a_mid, s2 a_last.
__device__ __forceinline__ void area_cell(int d, double scale, int ssize, int& s1, int& s2, float& a_first, float& a_mid,
                                          float& a_last) {
    const double f1 = d * scale, f2 = f1 + scale;
    const double cell = fmin(scale, (double)ssize - f1);
    s1 = (int)ceil(f1);
    s2 = (int)floor(f2);
    s2 = min(s2, ssize - 1);
    s1 = min(s1, s2);
    a_first = (s1 - f1 > 1e-3) ? (float)((s1 - f1) / cell) : 0.0f;          // weight of pixel s1 - 1
    a_mid = (float)(1.0 / cell);                                            // pixels s1 .. s2 - 1
    a_last = (f2 - s2 > 1e-3) ? (float)(fmin(fmin(f2 - s2, 1.0), cell) / cell) : 0.0f;   // weight of pixel s2
}

// Output pixel (dy, dx) of the area-average resize of an sh x sw image to dh x dw, for NCH channels at once (the weights do not
// depend on the channel): acc[k] = the resized value of fetch(y, x, k), 0 <= y < sh, 0 <= x < sw.  Float32 throughout, row sums
// in x order, then * wy in y order; the area-mode bilinear when an axis enlarges.  The ONE statement of this arithmetic:
// resize_area_kernel (shade.hip) and photo_prepare_kernel (photo.hip) call it, both compiled with -ffp-contract=off, so that
// equal source values give equal bits.
template <int NCH, class Fetch>
__device__ __forceinline__ void resize_area_pixel(int dy, int dx, int sh, int sw, int dh, int dw, Fetch fetch, float (&acc)[NCH]) {
    const double scx = (double)sw / dw, scy = (double)sh / dh;
    for (int k = 0; k < NCH; k++) acc[k] = 0.0f;
    if (scx >= 1.0 && scy >= 1.0) {
        int x1, x2, y1, y2;
        float xa, xm, xl, ya, ym, yl;
        area_cell(dx, scx, sw, x1, x2, xa, xm, xl);
        area_cell(dy, scy, sh, y1, y2, ya, ym, yl);
        for (int y = y1 - 1; y <= y2; y++) {
            const float wy = y < y1 ? ya : (y < y2 ? ym : yl);
            if (wy == 0.0f || y < 0) continue;
            float row[NCH];
            for (int k = 0; k < NCH; k++) row[k] = 0.0f;
            for (int x = x1 - 1; x <= x2; x++) {
                const float wx = x < x1 ? xa : (x < x2 ? xm : xl);
                if (wx == 0.0f || x < 0) continue;
                for (int k = 0; k < NCH; k++) row[k] += fetch(y, x, k) * wx;
            }
            for (int k = 0; k < NCH; k++) acc[k] += row[k] * wy;
        }
    } else {
        int sx = (int)floor(dx * scx), sy = (int)floor(dy * scy);
        float fx = (float)((dx + 1) - (sx + 1) / scx), fy = (float)((dy + 1) - (sy + 1) / scy);
        fx = fx <= 0.0f ? 0.0f : fx - floorf(fx);
        fy = fy <= 0.0f ? 0.0f : fy - floorf(fy);
        sx = min(sx, sw - 1); sy = min(sy, sh - 1);
        const int sx1 = min(sx + 1, sw - 1), sy1 = min(sy + 1, sh - 1);
        for (int k = 0; k < NCH; k++) {
            const float v00 = fetch(sy, sx, k), v01 = fetch(sy, sx1, k);
            const float v10 = fetch(sy1, sx, k), v11 = fetch(sy1, sx1, k);
            acc[k] = (v00 * (1.0f - fx) + v01 * fx) * (1.0f - fy) + (v10 * (1.0f - fx) + v11 * fx) * fy;
        }
    }
}
#endif

}  // namespace rnr
