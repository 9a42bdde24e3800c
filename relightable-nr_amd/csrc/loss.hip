// The two per-pixel terms of train_rnr.py's objective (formulas and edge cases: include/rnr_hip.h):
//   rnr_rays_chrom_loss      network.RaysLTChromLoss (network.py:391-411) on rays_lt [N,R,3,H,W]
//   rnr_masked_l1_loss       the alpha-weighted L1 on the central crop (train_rnr.py:564-569, 581-585)
// and their adjoints.
//
//   forward   launch 1  one thread per pixel: the pixel's term and its alpha, summed over the workgroup -> one partial record
//             launch 2  one workgroup: the records summed in a fixed order -> loss_out
//   backward  one launch, one thread per pixel; the scale g / (sum alpha R) or g / count comes from device memory
//
// A thread reads plane after plane of its pixel and neighbouring lanes read neighbouring pixels, so every load of a wave is
// one contiguous 256-byte run.  Inputs are float32; the per-pixel arithmetic and all sums are float64, a gradient is rounded to
// float32 once.  No atomics: every record is written by one thread and every sum has a fixed order, so two calls on the same
// inputs give the same bits.  Every workspace word that is read was written earlier in the same call.
#include "rnr_internal.h"
#include <math.h>

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr double EPS = 1.0e-12;          // F.normalize's default
constexpr int R_KEPT = 26;               // the ray count of the reference's configs: 78 floats stay in registers in the backward

struct ChromPartial {
    double pix, alpha;
};

struct Vec3 {
    double x, y, z;
};
__device__ __forceinline__ double dot(Vec3 a, Vec3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// c = x / max(|x|, eps) as x * inv, inv = 1 / max(|x|, eps): what the adjoint divides by as well; *n = |x|
__device__ __forceinline__ Vec3 unit(float x0, float x1, float x2, double* n, double* inv) {
    const Vec3 x = {(double)x0, (double)x1, (double)x2};
    *n = sqrt(dot(x, x));
    *inv = 1.0 / (*n < EPS ? EPS : *n);                  // a NaN norm stays NaN, as torch's clamp_min keeps it
    return Vec3{x.x * *inv, x.y * *inv, x.z * *inv};
}

// mh = m / max(|m|, eps) with m = S / R; *M = |m|
__device__ __forceinline__ Vec3 mean_dir(Vec3 S, int R, double* M) {
    const Vec3 m = {S.x / (double)R, S.y / (double)R, S.z / (double)R};
    *M = sqrt(dot(m, m));
    const double d = *M < EPS ? EPS : *M;
    return Vec3{m.x / d, m.y / d, m.z / d};
}

// alpha * w of pixel q of view n, w = min(20 |img|, 1) (a NaN stays a NaN) or 1 without img
__device__ __forceinline__ double pixel_weight(float a, const float* __restrict__ img, long n, long q, long HW) {
    double w = 1.0;
    if (img) {
        const float* p = img + n * 3 * HW + q;
        const Vec3 v = {(double)p[0], (double)p[HW], (double)p[2 * HW]};
        const double s = 20.0 * sqrt(dot(v, v));
        w = s > 1.0 ? 1.0 : s;
    }
    return (double)a * w;
}

// ------------------------------------------------------------------------------------------------------------------------
// chromaticity loss
// ------------------------------------------------------------------------------------------------------------------------
// MAPS: one of the three map outputs is wanted; then every pixel is computed and a second sweep over the rays forms chrom_diff.
template <bool MAPS>
__global__ void __launch_bounds__(THREADS) chrom_forward_kernel(const float* __restrict__ rays, const float* __restrict__ alpha,
                                                                const float* __restrict__ img, float* __restrict__ chrom,
                                                                float* __restrict__ chrom_mean, float* __restrict__ chrom_diff,
                                                                ChromPartial* __restrict__ partials, int R, long HW, long pixels) {
    __shared__ double sh[WAVES];
    const long p = (long)blockIdx.x * THREADS + threadIdx.x;
    double pix = 0.0, a = 0.0;
    if (p < pixels) {
        const long n = p / HW, q = p % HW;
        a = (double)alpha[p];
        const double aw = pixel_weight(alpha[p], img, n, q, HW);
        const bool on = aw != 0.0;                       // a NaN weight counts as on and propagates
        if (on || MAPS) {
            const long base = n * R * 3 * HW + q;
            const float* x = rays + base;
            Vec3 S = {0.0, 0.0, 0.0};
            for (int r = 0; r < R; r++) {
                double nr, inv;
                const Vec3 c = unit(x[(3 * r) * HW], x[(3 * r + 1) * HW], x[(3 * r + 2) * HW], &nr, &inv);
                S.x += c.x;
                S.y += c.y;
                S.z += c.z;
                if (MAPS && chrom) {
                    float* o = chrom + base + (long)(3 * r) * HW;
                    o[0] = (float)c.x;
                    o[HW] = (float)c.y;
                    o[2 * HW] = (float)c.z;
                }
            }
            double M;
            const Vec3 mh = mean_dir(S, R, &M);
            pix = on ? aw * ((double)R - dot(S, mh)) : 0.0;
            if (MAPS && chrom_mean) {
                float* o = chrom_mean + n * 3 * HW + q;
                o[0] = (float)mh.x;
                o[HW] = (float)mh.y;
                o[2 * HW] = (float)mh.z;
            }
            if (MAPS && chrom_diff)
                for (int r = 0; r < R; r++) {
                    double nr, inv;
                    const Vec3 c = unit(x[(3 * r) * HW], x[(3 * r + 1) * HW], x[(3 * r + 2) * HW], &nr, &inv);
                    chrom_diff[(n * R + r) * HW + q] = on ? (float)((1.0 - dot(c, mh)) * aw) : 0.0f;
                }
        }
    }
    pix = rnr::block_sum<WAVES>(pix, sh);
    a = rnr::block_sum<WAVES>(a, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = ChromPartial{pix, a};
}

__global__ void __launch_bounds__(THREADS) chrom_finalise_kernel(const ChromPartial* __restrict__ partials, int num,
                                                                 double* __restrict__ out, int R) {
    __shared__ double sh[WAVES];
    double pix = 0.0, a = 0.0;
    for (int i = threadIdx.x; i < num; i += THREADS) {
        pix += partials[i].pix;
        a += partials[i].alpha;
    }
    pix = rnr::block_sum<WAVES>(pix, sh);
    a = rnr::block_sum<WAVES>(a, sh);
    if (threadIdx.x == 0) {
        out[0] = pix / a / (double)R;          // 0 / 0 = NaN when no pixel is covered, as in the reference
        out[1] = a;
    }
}

// RT > 0: the ray count is RT and the pixel's 3 RT values stay in registers between the two sweeps; RT == 0: any ray count,
// the second sweep reads them again.  Four waves per SIMD asked for (at most 128 VGPRs): left alone the compiler takes 256 for
// <26> and runs one.  Resource report: <26> 116 VGPRs, <0> 38, no scratch.
template <int RT>
__global__ void __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(4)))
chrom_backward_kernel(const float* __restrict__ rays, const float* __restrict__ alpha, const float* __restrict__ img,
                      const double* __restrict__ loss_out, const float* __restrict__ g_loss, float* __restrict__ grad, int R_any, long HW,
                      long pixels) {
    const int R = RT > 0 ? RT : R_any;
    constexpr int UNROLL = RT > 0 ? RT : 1;
    const long p = (long)blockIdx.x * THREADS + threadIdx.x;
    if (p >= pixels) return;
    const long n = p / HW, q = p % HW;
    const long base = n * R * 3 * HW + q;
    const float* x = rays + base;
    float* gx = grad + base;
    const double aw = pixel_weight(alpha[p], img, n, q, HW);
    if (!(aw != 0.0)) {
        for (int i = 0; i < 3 * R; i++) gx[i * HW] = 0.0f;
        return;
    }
    const double k = (double)*g_loss * aw / (loss_out[1] * (double)R);
    float kept[RT > 0 ? 3 * RT : 1];
    Vec3 S = {0.0, 0.0, 0.0};
#pragma unroll UNROLL
    for (int r = 0; r < R; r++) {
        const float x0 = x[(3 * r) * HW], x1 = x[(3 * r + 1) * HW], x2 = x[(3 * r + 2) * HW];
        if (RT > 0) {
            kept[3 * r] = x0;
            kept[3 * r + 1] = x1;
            kept[3 * r + 2] = x2;
        }
        double nr, inv;
        const Vec3 c = unit(x0, x1, x2, &nr, &inv);
        S.x += c.x;
        S.y += c.y;
        S.z += c.z;
    }
    double M;
    const Vec3 mh = mean_dir(S, R, &M);
    const double sm = dot(S, mh);
    const bool live = M >= EPS;
    const double td = (live ? M : EPS) * (double)R;
    const Vec3 t = {(live ? S.x - sm * mh.x : S.x) / td, (live ? S.y - sm * mh.y : S.y) / td, (live ? S.z - sm * mh.z : S.z) / td};
    const Vec3 gc = {-k * (mh.x + t.x), -k * (mh.y + t.y), -k * (mh.z + t.z)};
#pragma unroll UNROLL
    for (int r = 0; r < R; r++) {
        float x0 = RT > 0 ? kept[3 * r] : x[(3 * r) * HW];
        float x1 = RT > 0 ? kept[3 * r + 1] : x[(3 * r + 1) * HW];
        float x2 = RT > 0 ? kept[3 * r + 2] : x[(3 * r + 2) * HW];
        // opaque to the optimiser: otherwise it keeps the first sweep's float64 c_r and 1 / n_r of all rays (130 doubles) and spills
        if (RT > 0) asm volatile("" : "+v"(x0), "+v"(x1), "+v"(x2));
        double nr, inv;
        const Vec3 c = unit(x0, x1, x2, &nr, &inv);
        const double gcc = nr >= EPS ? dot(gc, c) : 0.0;                 // |x| >= eps: project; below: gc / eps
        gx[(3 * r) * HW] = (float)((gc.x - gcc * c.x) * inv);
        gx[(3 * r + 1) * HW] = (float)((gc.y - gcc * c.y) * inv);
        gx[(3 * r + 2) * HW] = (float)((gc.z - gcc * c.z) * inv);
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// cropped L1
// ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool in_crop(long q, int W, int H, int b) {
    const int y = (int)(q / W), xx = (int)(q % W);
    return y >= b && y < H - b && xx >= b && xx < W - b;
}

__global__ void __launch_bounds__(THREADS) l1_forward_kernel(const float* __restrict__ est, const float* __restrict__ gt,
                                                             const float* __restrict__ alpha, int border,
                                                             double* __restrict__ partials, int C, int H, int W, long pixels) {
    __shared__ double sh[WAVES];
    const long HW = (long)H * W;
    const long p = (long)blockIdx.x * THREADS + threadIdx.x;
    double s = 0.0;
    if (p < pixels) {
        const long n = p / HW, q = p % HW;
        if (in_crop(q, W, H, border)) {
            const float a = alpha[p];
            for (int c = 0; c < C; c++) {
                const long i = (n * C + c) * HW + q;
                const float e = est[i] * a, g = gt[i] * a;             // rounded to float32 as the reference rounds them
                s += fabs((double)e - (double)g);
            }
        }
    }
    s = rnr::block_sum<WAVES>(s, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ void __launch_bounds__(THREADS) l1_finalise_kernel(const double* __restrict__ partials, int num,
                                                              double* __restrict__ out, double count) {
    __shared__ double sh[WAVES];
    double s = 0.0;
    for (int i = threadIdx.x; i < num; i += THREADS) s += partials[i];
    s = rnr::block_sum<WAVES>(s, sh);
    if (threadIdx.x == 0) out[0] = s / count;
}

__global__ void __launch_bounds__(THREADS) l1_backward_kernel(const float* __restrict__ est, const float* __restrict__ gt,
                                                              const float* __restrict__ alpha, int border,
                                                              const float* __restrict__ g_loss, float* __restrict__ grad, int C,
                                                              int H, int W, long pixels, double count) {
    const long HW = (long)H * W;
    const long p = (long)blockIdx.x * THREADS + threadIdx.x;
    if (p >= pixels) return;
    const long n = p / HW, q = p % HW;
    const bool inside = in_crop(q, W, H, border);
    const float a = alpha[p];
    const double scale = (double)*g_loss * (double)a / count;
    for (int c = 0; c < C; c++) {
        const long i = (n * C + c) * HW + q;
        float g = 0.0f;
        if (inside) {
            const float e = est[i] * a, t = gt[i] * a;
            g = e > t ? (float)scale : e < t ? (float)-scale : 0.0f;     // sign(0) = 0; a NaN difference gives 0
        }
        grad[i] = g;
    }
}

unsigned blocks_for(long pixels) { return (unsigned)((pixels + THREADS - 1) / THREADS); }

int check_chrom(const char* who, int N, int R, int H, int W) {
    RNR_REQUIRE(N > 0 && H > 0 && W > 0, "%s: sizes must be positive (got %d views of %d x %d)", who, N, H, W);
    RNR_REQUIRE(R >= 1, "%s: the ray count must be at least 1 (got %d)", who, R);
    RNR_REQUIRE((double)N * (double)R * 3.0 * (double)H * (double)W < 2147483648.0, "%s: %d x %d x 3 x %d x %d elements: 2^31 or more",
                who, N, R, H, W);
    return 0;
}

int check_l1(const char* who, int border, int N, int C, int H, int W) {
    RNR_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, "%s: sizes must be positive (got %d x %d x %d x %d)", who, N, C, H, W);
    RNR_REQUIRE((double)N * (double)C * (double)H * (double)W < 2147483648.0, "%s: %d x %d x %d x %d elements: 2^31 or more", who, N, C,
                H, W);
    RNR_REQUIRE(border >= 0, "%s: border must not be negative (got %d)", who, border);
    RNR_REQUIRE(H > 2 * (long)border && W > 2 * (long)border, "%s: a border of %d leaves nothing of %d x %d", who, border, H, W);
    return 0;
}

}  // namespace

extern "C" size_t rnr_rays_chrom_loss_workspace_bytes(int num_views, int num_rays, int height, int width) {
    if (num_views <= 0 || num_rays <= 0 || height <= 0 || width <= 0) return 0;
    return (size_t)blocks_for((long)num_views * height * width) * sizeof(ChromPartial);
}

extern "C" int rnr_rays_chrom_loss(const float* rays_lt, const float* alpha, const float* img, double* loss_out, float* chrom,
                                   float* chrom_mean, float* chrom_diff, void* workspace, int num_views, int num_rays, int height,
                                   int width, void* stream) {
    RNR_REQUIRE(rays_lt && alpha && loss_out && workspace, "rnr_rays_chrom_loss: rays_lt, alpha, loss_out and workspace must not be NULL");
    if (int rc = check_chrom("rnr_rays_chrom_loss", num_views, num_rays, height, width)) return rc;
    RNR_REQUIRE(((uintptr_t)workspace | (uintptr_t)loss_out) % 8 == 0, "rnr_rays_chrom_loss: workspace and loss_out must be 8-byte aligned");
    const long HW = (long)height * width, pixels = (long)num_views * HW;
    const unsigned blocks = blocks_for(pixels);
    ChromPartial* partials = reinterpret_cast<ChromPartial*>(workspace);
    hipStream_t st = rnr::as_stream(stream);
    if (chrom || chrom_mean || chrom_diff)
        hipLaunchKernelGGL(chrom_forward_kernel<true>, dim3(blocks), dim3(THREADS), 0, st, rays_lt, alpha, img, chrom, chrom_mean,
                           chrom_diff, partials, num_rays, HW, pixels);
    else
        hipLaunchKernelGGL(chrom_forward_kernel<false>, dim3(blocks), dim3(THREADS), 0, st, rays_lt, alpha, img, chrom, chrom_mean,
                           chrom_diff, partials, num_rays, HW, pixels);
    if (int rc = rnr::check_launch("rays chrom loss: chrom_forward_kernel")) return rc;
    hipLaunchKernelGGL(chrom_finalise_kernel, dim3(1), dim3(THREADS), 0, st, (const ChromPartial*)partials, (int)blocks, loss_out, num_rays);
    return rnr::check_launch("rays chrom loss: chrom_finalise_kernel");
}

extern "C" int rnr_rays_chrom_loss_backward(const float* rays_lt, const float* alpha, const float* img, const double* loss_out,
                                            const float* g_loss, float* grad_rays_lt, int num_views, int num_rays, int height,
                                            int width, void* stream) {
    RNR_REQUIRE(rays_lt && alpha && loss_out && g_loss && grad_rays_lt,
                "rnr_rays_chrom_loss_backward: rays_lt, alpha, loss_out, g_loss and grad_rays_lt must not be NULL");
    if (int rc = check_chrom("rnr_rays_chrom_loss_backward", num_views, num_rays, height, width)) return rc;
    RNR_REQUIRE((uintptr_t)loss_out % 8 == 0, "rnr_rays_chrom_loss_backward: loss_out must be 8-byte aligned");
    const long HW = (long)height * width, pixels = (long)num_views * HW;
    hipStream_t st = rnr::as_stream(stream);
    if (num_rays == R_KEPT)
        hipLaunchKernelGGL(chrom_backward_kernel<R_KEPT>, dim3(blocks_for(pixels)), dim3(THREADS), 0, st, rays_lt, alpha, img, loss_out,
                           g_loss, grad_rays_lt, num_rays, HW, pixels);
    else
        hipLaunchKernelGGL(chrom_backward_kernel<0>, dim3(blocks_for(pixels)), dim3(THREADS), 0, st, rays_lt, alpha, img, loss_out,
                           g_loss, grad_rays_lt, num_rays, HW, pixels);
    return rnr::check_launch("rays chrom loss: chrom_backward_kernel");
}

extern "C" size_t rnr_masked_l1_loss_workspace_bytes(int num_views, int height, int width) {
    if (num_views <= 0 || height <= 0 || width <= 0) return 0;
    return (size_t)blocks_for((long)num_views * height * width) * sizeof(double);
}

extern "C" int rnr_masked_l1_loss(const float* est, const float* gt, const float* alpha, int border, double* loss_out, void* workspace,
                                  int num_views, int channels, int height, int width, void* stream) {
    RNR_REQUIRE(est && gt && alpha && loss_out && workspace, "rnr_masked_l1_loss: est, gt, alpha, loss_out and workspace must not be NULL");
    if (int rc = check_l1("rnr_masked_l1_loss", border, num_views, channels, height, width)) return rc;
    RNR_REQUIRE(((uintptr_t)workspace | (uintptr_t)loss_out) % 8 == 0, "rnr_masked_l1_loss: workspace and loss_out must be 8-byte aligned");
    const long pixels = (long)num_views * height * width;
    const unsigned blocks = blocks_for(pixels);
    const double count = (double)num_views * channels * (double)(height - 2 * border) * (double)(width - 2 * border);
    double* partials = reinterpret_cast<double*>(workspace);
    hipStream_t st = rnr::as_stream(stream);
    hipLaunchKernelGGL(l1_forward_kernel, dim3(blocks), dim3(THREADS), 0, st, est, gt, alpha, border, partials, channels, height, width,
                       pixels);
    if (int rc = rnr::check_launch("masked l1 loss: l1_forward_kernel")) return rc;
    hipLaunchKernelGGL(l1_finalise_kernel, dim3(1), dim3(THREADS), 0, st, (const double*)partials, (int)blocks, loss_out, count);
    return rnr::check_launch("masked l1 loss: l1_finalise_kernel");
}

extern "C" int rnr_masked_l1_loss_backward(const float* est, const float* gt, const float* alpha, int border, const float* g_loss,
                                           float* grad_est, int num_views, int channels, int height, int width, void* stream) {
    RNR_REQUIRE(est && gt && alpha && g_loss && grad_est,
                "rnr_masked_l1_loss_backward: est, gt, alpha, g_loss and grad_est must not be NULL");
    if (int rc = check_l1("rnr_masked_l1_loss_backward", border, num_views, channels, height, width)) return rc;
    const long pixels = (long)num_views * height * width;
    const double count = (double)num_views * channels * (double)(height - 2 * border) * (double)(width - 2 * border);
    hipLaunchKernelGGL(l1_backward_kernel, dim3(blocks_for(pixels)), dim3(THREADS), 0, rnr::as_stream(stream), est, gt, alpha, border,
                       g_loss, grad_est, channels, height, width, pixels, count);
    return rnr::check_launch("masked l1 loss: l1_backward_kernel");
}
