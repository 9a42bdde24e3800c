// Photographs in: an 8-bit interleaved image on the device -> the [3, S, S] float32 ground truth of a training view, one launch.
//
// What data_util.load_img(square_crop=True, downsampling_order=1) + [:, :, :3] + transpose(2, 0, 1) + ** img_gamma do on the host
// (data_util.py:21-54, dataio.py:171-174):
//   v   = (float)byte / 255.0f                              IEEE division: the 256 values are numpy's float32 quotients
//   r   = INTER_AREA of v over the crop window to dst_h x dst_w: rnr_internal.h's resize_area_pixel, the arithmetic of
//         rnr_resize_area (this file is compiled with -ffp-contract=off like shade.hip, so equal values give equal bits)
//   out = gamma == 1 ? r : (float)pow((double)r, gamma)     the float32 nearest to the float64 power
// One lane per output pixel carries the three channels: the weights are shared, the three bytes of a pixel are adjacent, and
// neighbouring lanes read neighbouring cells of a source row.  A load-time operator: once per photograph, not per training step.
#include "rnr_internal.h"

#include <math.h>

using namespace rnr;

__global__ void __launch_bounds__(256)
photo_prepare_kernel(const uint8_t* __restrict__ src, int src_w, int src_ch, int crop_y0, int crop_x0, int crop_h, int crop_w,
                     double gamma, float* __restrict__ dst, int dh, int dw) {
    const long npix = (long)dh * dw;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const int dx = (int)(i % dw), dy = (int)(i / dw);
    // (y, x) below are window coordinates, 0 <= y < crop_h and 0 <= x < crop_w: inside the image by the entry point's checks
    const uint8_t* win = src + ((size_t)crop_y0 * src_w + crop_x0) * src_ch;
    float acc[3];
    resize_area_pixel<3>(dy, dx, crop_h, crop_w, dh, dw,
                         [&](int y, int x, int k) { return (float)win[((size_t)y * src_w + x) * src_ch + k] / 255.0f; }, acc);
    for (int k = 0; k < 3; k++) dst[k * npix + i] = gamma == 1.0 ? acc[k] : (float)pow((double)acc[k], gamma);
}

extern "C" int rnr_photo_prepare(const uint8_t* src, int src_h, int src_w, int src_channels, int crop_y0, int crop_x0, int crop_h,
                                 int crop_w, double gamma, float* dst, int dst_h, int dst_w, void* stream) {
    RNR_REQUIRE(src && dst, "rnr_photo_prepare: src and dst must not be NULL");
    RNR_REQUIRE(src_h > 0 && src_w > 0 && crop_h > 0 && crop_w > 0 && dst_h > 0 && dst_w > 0,
                "rnr_photo_prepare: sizes must be positive (src %d x %d, crop %d x %d, dst %d x %d)", src_h, src_w, crop_h, crop_w,
                dst_h, dst_w);
    RNR_REQUIRE(src_channels == 3 || src_channels == 4, "rnr_photo_prepare: src_channels must be 3 or 4, got %d", src_channels);
    RNR_REQUIRE(crop_y0 >= 0 && crop_x0 >= 0 && (long)crop_y0 + crop_h <= src_h && (long)crop_x0 + crop_w <= src_w,
                "rnr_photo_prepare: crop window [%d, %ld) x [%d, %ld) is not inside the %d x %d image", crop_y0,
                (long)crop_y0 + crop_h, crop_x0, (long)crop_x0 + crop_w, src_h, src_w);
    RNR_REQUIRE(isfinite(gamma) && gamma > 0.0, "rnr_photo_prepare: gamma must be finite and > 0, got %g", gamma);
    RNR_REQUIRE(aligned_to(4, {dst}), "rnr_photo_prepare: dst must be 4-byte aligned");
    const long npix = (long)dst_h * dst_w;
    hipLaunchKernelGGL(photo_prepare_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, as_stream(stream), src, src_w,
                       src_channels, crop_y0, crop_x0, crop_h, crop_w, gamma, dst, dst_h, dst_w);
    return check_launch("photo_prepare_kernel");
}
