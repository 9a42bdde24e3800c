// rnr_image_metrics: the twelve per-view error metrics of metric.compute_err_metrics (metric.py:19-84) in three launches:
// MAE / MSE / PSNR over the image, the mask's bounding box and the mask, and SSIM over the image and the box.
//
//   launch 1  sums_kernel      one workgroup per (band of rows, view): S1 = sum |d|, S2 = sum d^2 over the three channels, the
//                              number of mask pixels and the min / max of their x and y -> one Band record
//   launch 2  ssim_kernel      one workgroup per (tile of TILE x TILE windows, view): the 11-tap Gaussian moments of the
//                              masked images, horizontal then vertical pass through LDS, the SSIM map value of every window,
//                              summed over all windows of the image and over the windows inside the box -> one Tile record
//   launch 3  finalise_kernel  one workgroup per view: the records summed in a fixed order, the twelve outputs and the box
//
// Every value is x = float32(v * scale) where mask == 1 and 0 elsewhere (a select: what lies outside the mask is never used in
// arithmetic), widened to double; all moment arithmetic and every sum is float64 (E[x^2] - mu^2 cancels near 65025 on bright
// flat regions: float32 moments are off by 2.4e-4 per window there).  No atomics: every record is written by one thread and
// every sum has a fixed order, so two calls on the same inputs give the same bits.  Every workspace word that is read was
// written earlier in the same call.
#include "rnr_internal.h"
#include <math.h>

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int TAPS = 11;
constexpr int HALO = TAPS - 1;
constexpr int TILE = 32;                       // windows per tile side
constexpr int STAGE = TILE + HALO;             // 42 staged pixels per tile side
constexpr int STAGE_LD = STAGE + 1;            // 43 floats: rows 0..3 of a half wave start on banks 0, 11, 22, 1 (no conflict)
constexpr int H_LD = TILE + 1;                 // 33 doubles per row of a horizontal-pass plane
constexpr int STAGE_ITEMS = STAGE * STAGE;     // 1764 pixels
constexpr int STAGE_ROUNDS = (STAGE_ITEMS + THREADS - 1) / THREADS;     // 7
constexpr int COLS_PER_ITEM = 4;               // horizontal pass: outputs per (row, column group) item
constexpr int ROWS_PER_THREAD = TILE / (THREADS / TILE);                // vertical pass: 4 windows per thread
constexpr int BAND_ROWS = 8;

struct Band {              // launch 1 -> launches 2, 3
    double s1, s2;
    int count, xmin, xmax, ymin, ymax, pad;      // xmax, ymax inclusive; xmin > xmax when the band has no mask pixel
};
struct Tile {              // launch 2 -> launch 3
    double all, box;
};
struct Weights {
    double w[TAPS];
};
struct Box {
    int xmin, xmax, ymin, ymax;
};

__device__ __forceinline__ long pixel_index(int layout, int n, int c, int y, int x, int H, int W) {
    return layout == RNR_METRIC_PLANAR ? (((long)n * 3 + c) * H + y) * W + x : (((long)n * H + y) * W + x) * 3 + c;
}

__device__ __forceinline__ double block_sum(double v, double* sh) { return rnr::block_sum<WAVES>(v, sh); }

__device__ __forceinline__ int block_sum_int(int v, int* sh) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    int t = 0;
    if (threadIdx.x == 0)
        for (int i = 0; i < WAVES; i++) t += sh[i];
    return t;
}

// Box of per-thread boxes over the workgroup, valid in every thread.  `sh` holds WAVES + 1 boxes.
__device__ __forceinline__ Box block_box(Box b, Box* sh) {
    for (int o = 32; o > 0; o >>= 1) {
        b.xmin = min(b.xmin, __shfl_down(b.xmin, o));
        b.xmax = max(b.xmax, __shfl_down(b.xmax, o));
        b.ymin = min(b.ymin, __shfl_down(b.ymin, o));
        b.ymax = max(b.ymax, __shfl_down(b.ymax, o));
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        Box t = sh[0];
        for (int i = 1; i < WAVES; i++) {
            t.xmin = min(t.xmin, sh[i].xmin);
            t.xmax = max(t.xmax, sh[i].xmax);
            t.ymin = min(t.ymin, sh[i].ymin);
            t.ymax = max(t.ymax, sh[i].ymax);
        }
        sh[WAVES] = t;
    }
    __syncthreads();
    return sh[WAVES];
}

__device__ __forceinline__ Box empty_box() { return Box{INT32_MAX, -1, INT32_MAX, -1}; }

// The box of a view's mask from its Band records (integer min / max: any order gives the same result).
__device__ __forceinline__ Box view_box(const Band* __restrict__ bands, int num_bands, Box* sh) {
    Box b = empty_box();
    for (int i = threadIdx.x; i < num_bands; i += THREADS) {
        const Band r = bands[i];
        b.xmin = min(b.xmin, r.xmin);
        b.xmax = max(b.xmax, r.xmax);
        b.ymin = min(b.ymin, r.ymin);
        b.ymax = max(b.ymax, r.ymax);
    }
    return block_box(b, sh);
}

// ------------------------------------------------------------------------------------------------------------------------
// launch 1
// ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(THREADS) sums_kernel(const float* __restrict__ est, const float* __restrict__ gt,
                                                       const float* __restrict__ mask, int layout, float scale,
                                                       Band* __restrict__ bands, int num_bands, int band_rows, int H, int W) {
    __shared__ double sh_d[WAVES];
    __shared__ int sh_i[WAVES];
    __shared__ Box sh_b[WAVES + 1];
    const int n = blockIdx.x / num_bands, band = blockIdx.x % num_bands;
    const int y0 = band * band_rows, y1 = min(y0 + band_rows, H);
    double s1 = 0.0, s2 = 0.0;
    int count = 0;
    Box b = empty_box();
    for (int y = y0; y < y1; y++)
        for (int x = threadIdx.x; x < W; x += THREADS) {
            const bool valid = mask == nullptr || mask[((long)n * H + y) * W + x] == 1.0f;
            if (!valid) continue;
            count++;
            b.xmin = min(b.xmin, x);
            b.xmax = max(b.xmax, x);
            b.ymin = min(b.ymin, y);
            b.ymax = max(b.ymax, y);
            for (int c = 0; c < 3; c++) {
                const long i = pixel_index(layout, n, c, y, x, H, W);
                const float a = est[i] * scale, g = gt[i] * scale;
                const double d = fabs((double)a - (double)g);
                s1 += d;
                s2 += d * d;
            }
        }
    s1 = block_sum(s1, sh_d);
    s2 = block_sum(s2, sh_d);
    count = block_sum_int(count, sh_i);
    b = block_box(b, sh_b);
    if (threadIdx.x == 0) {
        Band r;
        r.s1 = s1;
        r.s2 = s2;
        r.count = count;
        r.xmin = b.xmin;
        r.xmax = b.xmax;
        r.ymin = b.ymin;
        r.ymax = b.ymax;
        r.pad = 0;
        bands[blockIdx.x] = r;
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// launch 2
// ------------------------------------------------------------------------------------------------------------------------
// LDS: two staged images 2 x 42 x 43 floats (14448 B) + five horizontal-pass planes 5 x 42 x 33 doubles (55440 B) + the
// reduction scratch: 69.9 KB, two workgroups per CU.
__global__ void __launch_bounds__(THREADS) ssim_kernel(const float* __restrict__ est, const float* __restrict__ gt,
                                                       const float* __restrict__ mask, int layout, float scale,
                                                       const Band* __restrict__ bands, int num_bands, Tile* __restrict__ tiles,
                                                       int tiles_x, int tiles_y, int H, int W, Weights wt) {
    __shared__ float sx[STAGE * STAGE_LD], sy[STAGE * STAGE_LD];
    __shared__ double hp[5][STAGE * H_LD];
    __shared__ double sh_d[WAVES];
    __shared__ Box sh_b[WAVES + 1];
    const int tid = threadIdx.x;
    const int per_view = tiles_x * tiles_y;
    const int n = blockIdx.x / per_view, t = blockIdx.x % per_view;
    const int oy = (t / tiles_x) * TILE, ox = (t % tiles_x) * TILE;
    const Box box = view_box(bands + (long)n * num_bands, num_bands, sh_b);

    // which of this thread's staged pixels are inside the image and the mask (the same for the three channels)
    unsigned valid = 0;
#pragma unroll
    for (int r = 0; r < STAGE_ROUNDS; r++) {
        const int i = tid + r * THREADS;
        const int y = oy + i / STAGE, x = ox + i % STAGE;
        if (i < STAGE_ITEMS && y < H && x < W && (mask == nullptr || mask[((long)n * H + y) * W + x] == 1.0f)) valid |= 1u << r;
    }

    const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
    const int wx = tid % TILE, wy0 = (tid / TILE) * ROWS_PER_THREAD;        // this thread's windows: column wx, rows wy0..wy0+3
    double sum_all = 0.0, sum_box = 0.0;
    for (int c = 0; c < 3; c++) {
#pragma unroll
        for (int r = 0; r < STAGE_ROUNDS; r++) {
            const int i = tid + r * THREADS;
            if (i < STAGE_ITEMS) {
                const int ly = i / STAGE, lx = i % STAGE;
                float a = 0.f, g = 0.f;
                if (valid >> r & 1) {
                    const long p = pixel_index(layout, n, c, oy + ly, ox + lx, H, W);
                    a = est[p] * scale;
                    g = gt[p] * scale;
                }
                sx[ly * STAGE_LD + lx] = a;
                sy[ly * STAGE_LD + lx] = g;
            }
        }
        __syncthreads();

        // horizontal pass: item = (staged row, group of 4 window columns); 14 pixels in, 4 x 5 moments out
        for (int item = tid; item < STAGE * (TILE / COLS_PER_ITEM); item += THREADS) {
            const int row = item / (TILE / COLS_PER_ITEM), col0 = (item % (TILE / COLS_PER_ITEM)) * COLS_PER_ITEM;
            double acc[COLS_PER_ITEM][5];
#pragma unroll
            for (int o = 0; o < COLS_PER_ITEM; o++)
#pragma unroll
                for (int m = 0; m < 5; m++) acc[o][m] = 0.0;
#pragma unroll
            for (int k = 0; k < COLS_PER_ITEM + HALO; k++) {
                const double a = (double)sx[row * STAGE_LD + col0 + k], g = (double)sy[row * STAGE_LD + col0 + k];
                const double v[5] = {a, g, a * a, g * g, a * g};
#pragma unroll
                for (int o = 0; o < COLS_PER_ITEM; o++)
                    if (k - o >= 0 && k - o < TAPS) {
#pragma unroll
                        for (int m = 0; m < 5; m++) acc[o][m] = __builtin_fma(wt.w[k - o], v[m], acc[o][m]);
                    }
            }
#pragma unroll
            for (int m = 0; m < 5; m++)
#pragma unroll
                for (int o = 0; o < COLS_PER_ITEM; o++) hp[m][row * H_LD + col0 + o] = acc[o][m];
        }
        __syncthreads();

        // vertical pass: 14 rows of the planes in, the moments of 4 windows out
        double acc[ROWS_PER_THREAD][5];
#pragma unroll
        for (int o = 0; o < ROWS_PER_THREAD; o++)
#pragma unroll
            for (int m = 0; m < 5; m++) acc[o][m] = 0.0;
#pragma unroll
        for (int k = 0; k < ROWS_PER_THREAD + HALO; k++) {
            double v[5];
#pragma unroll
            for (int m = 0; m < 5; m++) v[m] = hp[m][(wy0 + k) * H_LD + wx];
#pragma unroll
            for (int o = 0; o < ROWS_PER_THREAD; o++)
                if (k - o >= 0 && k - o < TAPS) {
#pragma unroll
                    for (int m = 0; m < 5; m++) acc[o][m] = __builtin_fma(wt.w[k - o], v[m], acc[o][m]);
                }
        }
#pragma unroll
        for (int o = 0; o < ROWS_PER_THREAD; o++) {
            const int y = oy + wy0 + o, x = ox + wx;                  // top-left pixel of the window
            const double mu1 = acc[o][0], mu2 = acc[o][1];
            const double s11 = acc[o][2] - mu1 * mu1, s22 = acc[o][3] - mu2 * mu2, s12 = acc[o][4] - mu1 * mu2;
            const double num = (2.0 * mu1 * mu2 + C1) * (2.0 * s12 + C2);
            const double den = (mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2);
            const double v = num / den;
            const bool in_image = y < H - HALO && x < W - HALO;
            const bool in_box = in_image && y >= box.ymin && y <= box.ymax - HALO && x >= box.xmin && x <= box.xmax - HALO;
            sum_all += in_image ? v : 0.0;
            sum_box += in_box ? v : 0.0;
        }
        // the next channel's staging writes sx / sy only (last read before the barrier above); its horizontal pass writes hp
        // behind the barrier that follows the staging, which every thread reaches after this vertical pass
    }
    sum_all = block_sum(sum_all, sh_d);
    sum_box = block_sum(sum_box, sh_d);
    if (tid == 0) tiles[blockIdx.x] = Tile{sum_all, sum_box};
}

// ------------------------------------------------------------------------------------------------------------------------
// launch 3
// ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double psnr_of(double mse) {
    const double m = mse / (255.0 * 255.0);
    return m < 1.0e-10 ? 100.0 : -10.0 * log10(m);
}

__global__ void __launch_bounds__(THREADS) finalise_kernel(const Band* __restrict__ bands, int num_bands,
                                                           const Tile* __restrict__ tiles, int num_tiles, double* __restrict__ out,
                                                           int32_t* __restrict__ box_out, int H, int W) {
    __shared__ double sh_d[WAVES];
    __shared__ int sh_i[WAVES];
    __shared__ Box sh_b[WAVES + 1];
    const int n = blockIdx.x;
    bands += (long)n * num_bands;
    tiles += (long)n * num_tiles;
    double s1 = 0.0, s2 = 0.0, all = 0.0, inbox = 0.0;
    int count = 0;
    for (int i = threadIdx.x; i < num_bands; i += THREADS) {
        s1 += bands[i].s1;
        s2 += bands[i].s2;
        count += bands[i].count;
    }
    for (int i = threadIdx.x; i < num_tiles; i += THREADS) {
        all += tiles[i].all;
        inbox += tiles[i].box;
    }
    const Box b = view_box(bands, num_bands, sh_b);
    s1 = block_sum(s1, sh_d);
    s2 = block_sum(s2, sh_d);
    all = block_sum(all, sh_d);
    inbox = block_sum(inbox, sh_d);
    count = block_sum_int(count, sh_i);
    if (threadIdx.x != 0) return;

    const double nan = __builtin_nan("");
    const bool empty = count == 0;
    const int bw = empty ? 0 : b.xmax + 1 - b.xmin, bh = empty ? 0 : b.ymax + 1 - b.ymin;
    const double n_img = 3.0 * (double)H * (double)W, n_box = 3.0 * (double)bw * (double)bh, n_valid = 3.0 * (double)count;
    double* o = out + (long)n * 12;
    o[RNR_METRIC_MAE] = s1 / n_img;
    o[RNR_METRIC_MAE_BB] = empty ? nan : s1 / n_box;
    o[RNR_METRIC_MAE_VALID] = empty ? nan : s1 / n_valid;
    o[RNR_METRIC_MSE] = s2 / n_img;
    o[RNR_METRIC_MSE_BB] = empty ? nan : s2 / n_box;
    o[RNR_METRIC_MSE_VALID] = empty ? nan : s2 / n_valid;
    o[RNR_METRIC_PSNR] = psnr_of(s2 / n_img);
    o[RNR_METRIC_PSNR_BB] = empty ? nan : psnr_of(s2 / n_box);
    o[RNR_METRIC_PSNR_VALID] = empty ? nan : psnr_of(s2 / n_valid);
    const bool have_ssim = num_tiles > 0;                              // compute_ssim and H, W >= 11
    const bool have_box_ssim = have_ssim && bw >= TAPS && bh >= TAPS;
    const double ssim_bb = have_box_ssim ? inbox / (3.0 * (double)(bw - HALO) * (double)(bh - HALO)) : nan;
    o[RNR_METRIC_SSIM] = have_ssim ? all / (3.0 * (double)(H - HALO) * (double)(W - HALO)) : nan;
    o[RNR_METRIC_SSIM_BB] = ssim_bb;
    o[RNR_METRIC_SSIM_VALID] = ssim_bb;       // metric.py:79-82 copies ground truth over pixels both images already have as 0
    if (box_out) {
        int32_t* q = box_out + (long)n * 5;
        q[0] = empty ? 0 : b.xmin;
        q[1] = empty ? 0 : b.xmax + 1;
        q[2] = empty ? 0 : b.ymin;
        q[3] = empty ? 0 : b.ymax + 1;
        q[4] = count;
    }
}

struct Plan {
    int band_rows, num_bands, tiles_x, tiles_y;
    size_t tiles_offset, bytes;
};

// Bands of 8 rows, or of as many as it takes to stay at 256 bands per view (what one pass of view_box reads).
Plan make_plan(int N, int H, int W) {
    Plan p;
    p.band_rows = BAND_ROWS > (H + 255) / 256 ? BAND_ROWS : (H + 255) / 256;
    p.num_bands = (H + p.band_rows - 1) / p.band_rows;
    const bool ssim = H >= TAPS && W >= TAPS;
    p.tiles_x = ssim ? (W - HALO + TILE - 1) / TILE : 0;
    p.tiles_y = ssim ? (H - HALO + TILE - 1) / TILE : 0;
    p.tiles_offset = (size_t)N * p.num_bands * sizeof(Band);
    p.bytes = p.tiles_offset + (size_t)N * p.tiles_x * p.tiles_y * sizeof(Tile);
    return p;
}

}  // namespace

extern "C" size_t rnr_image_metrics_workspace_bytes(int num_views, int height, int width) {
    if (num_views <= 0 || height <= 0 || width <= 0) return 0;
    return make_plan(num_views, height, width).bytes;
}

extern "C" int rnr_image_metrics(const float* est, const float* gt, const float* mask, int layout, float scale, int compute_ssim,
                                 double* out, int32_t* box, void* workspace, int num_views, int height, int width, void* stream) {
    RNR_REQUIRE(est && gt && out && workspace, "rnr_image_metrics: est, gt, out and workspace must not be NULL");
    RNR_REQUIRE(num_views > 0 && height > 0 && width > 0, "rnr_image_metrics: sizes must be positive (got %d views of %d x %d)",
                num_views, height, width);
    RNR_REQUIRE((double)num_views * 3.0 * (double)height * (double)width < 2147483648.0,
                "rnr_image_metrics: %d x 3 x %d x %d elements: 2^31 or more", num_views, height, width);
    RNR_REQUIRE(layout == RNR_METRIC_PLANAR || layout == RNR_METRIC_CHANNELS_LAST, "rnr_image_metrics: unknown layout %d", layout);
    RNR_REQUIRE(((uintptr_t)workspace | (uintptr_t)out) % 8 == 0, "rnr_image_metrics: workspace and out must be 8-byte aligned");
    const Plan p = make_plan(num_views, height, width);
    Band* bands = reinterpret_cast<Band*>(workspace);
    Tile* tiles = reinterpret_cast<Tile*>(reinterpret_cast<char*>(workspace) + p.tiles_offset);
    const int num_tiles = compute_ssim ? p.tiles_x * p.tiles_y : 0;
    hipStream_t st = rnr::as_stream(stream);

    hipLaunchKernelGGL(sums_kernel, dim3((unsigned)(num_views * p.num_bands)), dim3(THREADS), 0, st, est, gt, mask, layout, scale, bands,
                       p.num_bands, p.band_rows, height, width);
    if (int rc = rnr::check_launch("image metrics: sums_kernel")) return rc;
    if (num_tiles > 0) {
        Weights wt;                           // exp(-k^2 / (2 sigma^2)) / sum, sigma = 1.5, in double
        double sum = 0.0;
        for (int k = 0; k < TAPS; k++) {
            const double d = (double)(k - TAPS / 2);
            wt.w[k] = exp(-d * d / 4.5);
            sum += wt.w[k];
        }
        for (int k = 0; k < TAPS; k++) wt.w[k] /= sum;
        hipLaunchKernelGGL(ssim_kernel, dim3((unsigned)(num_views * num_tiles)), dim3(THREADS), 0, st, est, gt, mask, layout, scale,
                           (const Band*)bands, p.num_bands, tiles, p.tiles_x, p.tiles_y, height, width, wt);
        if (int rc = rnr::check_launch("image metrics: ssim_kernel")) return rc;
    }
    hipLaunchKernelGGL(finalise_kernel, dim3((unsigned)num_views), dim3(THREADS), 0, st, (const Band*)bands, p.num_bands,
                       (const Tile*)tiles, num_tiles, out, box, height, width);
    return rnr::check_launch("image metrics: finalise_kernel");
}
