// The stitched light probe of stitch_lp.py on the device (formulas, layouts and limits: include/rnr_hip.h):
//   rnr_background_mask     the pixels farther than `radius` from every covered pixel          stitch_lp.py:135-140
//   rnr_stitch_accumulate   background pixels of N views scattered into an equirect probe       stitch_lp.py:142-150
//   rnr_stitch_finalize     sum / count -> probe and mask                                       stitch_lp.py:152-153
//   rnr_probe_prepare       NaN -> 0, gamma, uncovered texels <- mean of the covered ones       train_rnr.py:288-295
//
// The scatter is numpy's fancy-index `+=`: within a view a texel takes the value of the LAST pixel (row-major) that maps to it
// and its count rises by one; views add up in view order in float64.  Two launches, no float atomics:
//   pass 1  one thread per pixel: direction, texel, atomicMax(winner[view][texel], pixel index + 1)        (integer maximum:
//           the result does not depend on the order of arrival)
//   pass 2  one thread per texel, neighbouring lanes on neighbouring texels: the call's views in order; a non-zero winner's
//           three floats are added to the texel's float64 sum, its count rises by one and the winner is cleared again.
// Every sum has a fixed order, so two runs give the same bits, and so does any split of the views over successive calls.
// Bytes of one call (T = lp_h lp_w texels, P = N H W pixels, B background pixels): pass 1 reads P mask bytes and issues B
// 4-byte atomics; pass 2 reads 4 N T winner bytes, clears the non-zero ones, fetches 12 bytes per winner and reads and writes
// 28 bytes of state per texel that a view of the call saw.
#include "rnr_internal.h"
#include <math.h>

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int TILE = 32;                        // background_mask_kernel: output pixels per workgroup side
constexpr int SPAN = TILE + 2 * RNR_BACKGROUND_MASK_MAX_RADIUS;
constexpr double PI = 3.141592653589793;        // np.pi

// ------------------------------------------------------------------------------------------------------------------------
// background mask: 1 - dilation of (alpha > 0) by a (2r+1) x (2r+1) window clipped to the image
// ------------------------------------------------------------------------------------------------------------------------
// One workgroup per 32 x 32 tile: coverage of the tile and its halo in LDS, the row maximum over 2r+1 columns, then the column
// maximum over 2r+1 rows.  Floor: 4 bytes read and 1 written per pixel, 5 N H W (the halo is read again from L2).
__global__ void __launch_bounds__(THREADS) background_mask_kernel(const float* __restrict__ alpha, uint8_t* __restrict__ background,
                                                                  int H, int W, int r, int tiles_x, int tiles_y) {
    __shared__ uint8_t cov[SPAN * SPAN];
    __shared__ uint8_t rowm[SPAN * TILE];
    const int tx = (int)(blockIdx.x % (unsigned)tiles_x), ty = (int)((blockIdx.x / (unsigned)tiles_x) % (unsigned)tiles_y);
    const long n = (long)(blockIdx.x / ((unsigned)tiles_x * (unsigned)tiles_y));
    const long base = n * (long)H * W;
    const int span = TILE + 2 * r, x0 = tx * TILE - r, y0 = ty * TILE - r;
    for (int i = threadIdx.x; i < span * span; i += THREADS) {
        const int yy = i / span, xx = i % span, gy = y0 + yy, gx = x0 + xx;
        uint8_t c = 0;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) c = alpha[base + (long)gy * W + gx] > 0.0f ? 1 : 0;      // NaN: not covered
        cov[yy * span + xx] = c;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < span * TILE; i += THREADS) {
        const int yy = i / TILE, c = i % TILE;
        uint8_t m = 0;
        for (int k = 0; k <= 2 * r; k++) m |= cov[yy * span + c + k];
        rowm[yy * TILE + c] = m;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < TILE * TILE; i += THREADS) {
        const int yy = i / TILE, c = i % TILE, gy = ty * TILE + yy, gx = tx * TILE + c;
        if (gy < H && gx < W) {
            uint8_t m = 0;
            for (int k = 0; k <= 2 * r; k++) m |= rowm[(yy + k) * TILE + c];
            background[base + (long)gy * W + gx] = m ? 0 : 1;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// stitch
// ------------------------------------------------------------------------------------------------------------------------
// texel of pixel (row, col) of view n, all in float64 (stitch_lp.py:26-33, 21-23, 145-147); false when the direction is not
// finite (a singular matrix), which the reference answers with an index error
__device__ __forceinline__ bool pixel_texel(const double* __restrict__ proj_inv, const double* __restrict__ R_inv, long n, int row,
                                            int col, int lp_h, int lp_w, long* texel) {
    const double* Pi = proj_inv + n * 9;
    const double* Ri = R_inv + n * 9;
    const double px = (double)col + 0.5, py = (double)row + 0.5;
    const double cx = Pi[0] * px + Pi[1] * py + Pi[2], cy = Pi[3] * px + Pi[4] * py + Pi[5], cz = Pi[6] * px + Pi[7] * py + Pi[8];
    double wx = Ri[0] * cx + Ri[1] * cy + Ri[2] * cz, wy = Ri[3] * cx + Ri[4] * cy + Ri[5] * cz,
           wz = Ri[6] * cx + Ri[7] * cy + Ri[8] * cz;
    const double len = sqrt(wx * wx + wy * wy + wz * wz);
    wx /= len;
    wy /= len;
    wz /= len;
    const double u = atan2(wz, wx) * 0.5 / PI + 0.5, v = acos(wy) * 1.0 / PI;
    double fu = u * (double)lp_w, fv = v * (double)lp_h;
    fu = fu > (double)lp_w - 1.0 ? (double)lp_w - 1.0 : fu;
    fv = fv > (double)lp_h - 1.0 ? (double)lp_h - 1.0 : fv;
    if (!(fu >= 0.0 && fv >= 0.0)) return false;                   // NaN
    *texel = (long)rint(fv) * lp_w + (long)rint(fu);              // np.round: half to even
    return true;
}

__global__ void __launch_bounds__(THREADS) stitch_winner_kernel(const uint8_t* __restrict__ background,
                                                                const double* __restrict__ proj_inv,
                                                                const double* __restrict__ R_inv, unsigned* __restrict__ winner,
                                                                int H, int W, int lp_h, int lp_w, long pixels) {
    const long p = (long)blockIdx.x * THREADS + threadIdx.x;
    if (p >= pixels || !background[p]) return;
    const long HW = (long)H * W, n = p / HW, q = p % HW;
    long texel;
    if (!pixel_texel(proj_inv, R_inv, n, (int)(q / W), (int)(q % W), lp_h, lp_w, &texel)) return;
    atomicMax(winner + n * ((long)lp_h * lp_w) + texel, (unsigned)(q + 1));
}

template <bool CHANNELS_LAST>
__global__ void __launch_bounds__(THREADS) stitch_sum_kernel(const float* __restrict__ images, unsigned* __restrict__ winner,
                                                             double* __restrict__ sum, int* __restrict__ count, int N, long HW,
                                                             long texels) {
    const long t = (long)blockIdx.x * THREADS + threadIdx.x;
    if (t >= texels) return;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    int seen = 0;
    for (int n0 = 0; n0 < N; n0 += 4) {                   // four views' winners in flight before the first dependent fetch
        unsigned win[4];
        for (int j = 0; j < 4; j++) win[j] = n0 + j < N ? winner[(long)(n0 + j) * texels + t] : 0u;
        for (int j = 0; j < 4; j++) {
            if (win[j] == 0) continue;
            const long n = n0 + j, q = (long)win[j] - 1;
            float a, b, c;
            if (CHANNELS_LAST) {
                const float* px = images + (n * HW + q) * 3;
                a = px[0], b = px[1], c = px[2];
            } else {
                const float* px = images + n * 3 * HW + q;
                a = px[0], b = px[HW], c = px[2 * HW];
            }
            if (seen == 0) s0 = sum[3 * t], s1 = sum[3 * t + 1], s2 = sum[3 * t + 2];
            s0 += (double)a;
            s1 += (double)b;
            s2 += (double)c;
            seen++;
            winner[n * texels + t] = 0;
        }
    }
    if (seen) {
        sum[3 * t] = s0;
        sum[3 * t + 1] = s1;
        sum[3 * t + 2] = s2;
        count[t] += seen;
    }
}

__global__ void __launch_bounds__(THREADS) stitch_finalize_kernel(const double* __restrict__ sum, const int* __restrict__ count,
                                                                  float* __restrict__ lp, uint8_t* __restrict__ mask, long texels) {
    const long t = (long)blockIdx.x * THREADS + threadIdx.x;
    if (t >= texels) return;
    const int k = count[t];
    const bool on = k > 0;
    for (int c = 0; c < 3; c++) lp[3 * t + c] = on ? (float)(sum[3 * t + c] / (double)k) : 0.0f;
    mask[t] = on ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------------------
// probe prepare
// ------------------------------------------------------------------------------------------------------------------------
struct FillPartial {
    double s[3], n;
};

// (lp and out may be one buffer: a thread reads its texel before it writes it)
__global__ void __launch_bounds__(THREADS) prepare_gamma_kernel(const float* lp, const uint8_t* __restrict__ mask, double gamma,
                                                                float* out,
                                                                FillPartial* __restrict__ partials, long texels) {
    __shared__ double sh[WAVES];
    const long t = (long)blockIdx.x * THREADS + threadIdx.x;
    double s[3] = {0.0, 0.0, 0.0}, n = 0.0;
    if (t < texels) {
        const bool on = mask[t] != 0;
        for (int c = 0; c < 3; c++) {
            float v = lp[3 * t + c];
            if (v != v) v = 0.0f;
            if (gamma != 1.0) v = (float)pow((double)v, gamma);
            out[3 * t + c] = v;
            if (on) s[c] = (double)v;
        }
        n = on ? 1.0 : 0.0;
    }
    FillPartial r;
    for (int c = 0; c < 3; c++) r.s[c] = rnr::block_sum<WAVES>(s[c], sh);
    r.n = rnr::block_sum<WAVES>(n, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = r;
}

// mean[c] = sum / count over the covered texels (0 / 0 = NaN for an empty mask, as numpy's mean of nothing)
__global__ void __launch_bounds__(THREADS) prepare_mean_kernel(const FillPartial* __restrict__ partials, int num,
                                                               double* __restrict__ mean) {
    __shared__ double sh[WAVES];
    double s[3] = {0.0, 0.0, 0.0}, n = 0.0;
    for (int i = threadIdx.x; i < num; i += THREADS) {
        for (int c = 0; c < 3; c++) s[c] += partials[i].s[c];
        n += partials[i].n;
    }
    for (int c = 0; c < 3; c++) s[c] = rnr::block_sum<WAVES>(s[c], sh);
    n = rnr::block_sum<WAVES>(n, sh);
    if (threadIdx.x == 0)
        for (int c = 0; c < 3; c++) mean[c] = s[c] / n;
}

__global__ void __launch_bounds__(THREADS) prepare_fill_kernel(const uint8_t* __restrict__ mask, const double* __restrict__ mean,
                                                               float* __restrict__ out, long texels) {
    const long t = (long)blockIdx.x * THREADS + threadIdx.x;
    if (t >= texels || mask[t] != 0) return;
    for (int c = 0; c < 3; c++) out[3 * t + c] = (float)mean[c];
}

long blocks_for(long items) { return (items + THREADS - 1) / THREADS; }

int check_probe(const char* who, int lp_h, int lp_w) {
    RNR_REQUIRE(lp_h > 0 && lp_w > 0, "%s: the probe's sizes must be positive (got %d x %d)", who, lp_h, lp_w);
    RNR_REQUIRE((double)lp_h * (double)lp_w < 2147483648.0 / 3.0, "%s: a probe of %d x %d texels: 2^31 / 3 or more", who, lp_h, lp_w);
    return 0;
}

}  // namespace

extern "C" int rnr_background_mask(const float* alpha, int radius, uint8_t* background, int num_views, int height, int width,
                                   void* stream) {
    RNR_REQUIRE(alpha && background, "rnr_background_mask: alpha and background must not be NULL");
    RNR_REQUIRE(num_views > 0 && height > 0 && width > 0, "rnr_background_mask: sizes must be positive (got %d views of %d x %d)",
                num_views, height, width);
    RNR_REQUIRE(radius >= 0 && radius <= RNR_BACKGROUND_MASK_MAX_RADIUS, "rnr_background_mask: radius must be in 0..%d (got %d)",
                RNR_BACKGROUND_MASK_MAX_RADIUS, radius);
    const int tiles_x = (width + TILE - 1) / TILE, tiles_y = (height + TILE - 1) / TILE;
    const double blocks = (double)tiles_x * (double)tiles_y * (double)num_views;
    RNR_REQUIRE(blocks < 2147483648.0, "rnr_background_mask: %d views of %d x %d: 2^31 tiles or more", num_views, height, width);
    hipLaunchKernelGGL(background_mask_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, rnr::as_stream(stream), alpha, background,
                       height, width, radius, tiles_x, tiles_y);
    return rnr::check_launch("background mask: background_mask_kernel");
}

extern "C" size_t rnr_stitch_workspace_bytes(int num_views, int lp_h, int lp_w) {
    if (num_views <= 0 || lp_h <= 0 || lp_w <= 0) return 0;
    return (size_t)num_views * (size_t)lp_h * (size_t)lp_w * sizeof(unsigned);
}

extern "C" int rnr_stitch_accumulate(const float* images, int channels_last, const uint8_t* background, const double* proj_inv,
                                     const double* R_inv, double* sum, int32_t* count, void* workspace, size_t workspace_bytes,
                                     int num_views, int height, int width, int lp_h, int lp_w, void* stream) {
    RNR_REQUIRE(images && background && proj_inv && R_inv && sum && count && workspace,
                "rnr_stitch_accumulate: images, background, proj_inv, R_inv, sum, count and workspace must not be NULL");
    RNR_REQUIRE(num_views > 0 && height > 0 && width > 0, "rnr_stitch_accumulate: sizes must be positive (got %d views of %d x %d)",
                num_views, height, width);
    if (int rc = check_probe("rnr_stitch_accumulate", lp_h, lp_w)) return rc;
    RNR_REQUIRE((double)height * (double)width < 4294967295.0, "rnr_stitch_accumulate: a view of %d x %d pixels: 2^32 - 1 or more",
                height, width);
    const long HW = (long)height * width, pixels = (long)num_views * HW, texels = (long)lp_h * lp_w;
    RNR_REQUIRE(blocks_for(pixels) < 2147483648L, "rnr_stitch_accumulate: %d views of %d x %d: 2^39 pixels or more", num_views, height,
                width);
    RNR_REQUIRE(workspace_bytes >= rnr_stitch_workspace_bytes(num_views, lp_h, lp_w),
                "rnr_stitch_accumulate: workspace of %zu bytes, %zu needed (rnr_stitch_workspace_bytes)", workspace_bytes,
                rnr_stitch_workspace_bytes(num_views, lp_h, lp_w));
    RNR_REQUIRE(((uintptr_t)proj_inv | (uintptr_t)R_inv | (uintptr_t)sum) % 8 == 0 && ((uintptr_t)workspace | (uintptr_t)count) % 4 == 0,
                "rnr_stitch_accumulate: proj_inv, R_inv and sum must be 8-byte aligned, count and workspace 4-byte aligned");
    unsigned* winner = reinterpret_cast<unsigned*>(workspace);
    hipStream_t st = rnr::as_stream(stream);
    hipLaunchKernelGGL(stitch_winner_kernel, dim3((unsigned)blocks_for(pixels)), dim3(THREADS), 0, st, background, proj_inv, R_inv,
                       winner, height, width, lp_h, lp_w, pixels);
    if (int rc = rnr::check_launch("stitch accumulate: stitch_winner_kernel")) return rc;
    if (channels_last)
        hipLaunchKernelGGL(stitch_sum_kernel<true>, dim3((unsigned)blocks_for(texels)), dim3(THREADS), 0, st, images, winner, sum,
                           (int*)count, num_views, HW, texels);
    else
        hipLaunchKernelGGL(stitch_sum_kernel<false>, dim3((unsigned)blocks_for(texels)), dim3(THREADS), 0, st, images, winner, sum,
                           (int*)count, num_views, HW, texels);
    return rnr::check_launch("stitch accumulate: stitch_sum_kernel");
}

extern "C" int rnr_stitch_finalize(const double* sum, const int32_t* count, float* lp, uint8_t* mask, int lp_h, int lp_w,
                                   void* stream) {
    RNR_REQUIRE(sum && count && lp && mask, "rnr_stitch_finalize: sum, count, lp and mask must not be NULL");
    if (int rc = check_probe("rnr_stitch_finalize", lp_h, lp_w)) return rc;
    RNR_REQUIRE((uintptr_t)sum % 8 == 0 && ((uintptr_t)count | (uintptr_t)lp) % 4 == 0,
                "rnr_stitch_finalize: sum must be 8-byte aligned, count and lp 4-byte aligned");
    const long texels = (long)lp_h * lp_w;
    hipLaunchKernelGGL(stitch_finalize_kernel, dim3((unsigned)blocks_for(texels)), dim3(THREADS), 0, rnr::as_stream(stream), sum,
                       (const int*)count, lp, mask, texels);
    return rnr::check_launch("stitch finalize: stitch_finalize_kernel");
}

extern "C" size_t rnr_probe_prepare_workspace_bytes(int lp_h, int lp_w) {
    if (lp_h <= 0 || lp_w <= 0) return 0;
    return (size_t)blocks_for((long)lp_h * lp_w) * sizeof(FillPartial) + 4 * sizeof(double);
}

extern "C" int rnr_probe_prepare(const float* lp, const uint8_t* mask, double gamma, float* out, void* workspace, int lp_h, int lp_w,
                                 void* stream) {
    RNR_REQUIRE(lp && mask && out && workspace, "rnr_probe_prepare: lp, mask, out and workspace must not be NULL");
    if (int rc = check_probe("rnr_probe_prepare", lp_h, lp_w)) return rc;
    RNR_REQUIRE((uintptr_t)workspace % 8 == 0 && ((uintptr_t)lp | (uintptr_t)out) % 4 == 0,
                "rnr_probe_prepare: workspace must be 8-byte aligned, lp and out 4-byte aligned");
    const long texels = (long)lp_h * lp_w;
    const unsigned blocks = (unsigned)blocks_for(texels);
    double* mean = reinterpret_cast<double*>(workspace);                       // 4 doubles, then the partial records
    FillPartial* partials = reinterpret_cast<FillPartial*>(mean + 4);
    hipStream_t st = rnr::as_stream(stream);
    hipLaunchKernelGGL(prepare_gamma_kernel, dim3(blocks), dim3(THREADS), 0, st, lp, mask, gamma, out, partials, texels);
    if (int rc = rnr::check_launch("probe prepare: prepare_gamma_kernel")) return rc;
    hipLaunchKernelGGL(prepare_mean_kernel, dim3(1), dim3(THREADS), 0, st, (const FillPartial*)partials, (int)blocks, mean);
    if (int rc = rnr::check_launch("probe prepare: prepare_mean_kernel")) return rc;
    hipLaunchKernelGGL(prepare_fill_kernel, dim3(blocks), dim3(THREADS), 0, st, mask, (const double*)mean, out, texels);
    return rnr::check_launch("probe prepare: prepare_fill_kernel");
}
