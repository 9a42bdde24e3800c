// OpenEXR photographs and probes in: the per-byte and per-pixel halves of reading a scanline file, after rnr_amd/exr.py has parsed,
// validated and inflated it on the host.
//
// exr_unpack_kernel: chunk payloads -> the raw scanline buffer.  A ZIP / ZIPS chunk of n bytes t[0..n) is reconstructed by
//   predictor   t'[i] = (t'[i-1] + t[i] - 128) mod 256, i >= 1       a prefix sum mod 256
//   interleave  raw[2k] = t'[k], raw[2k+1] = t'[half + k], half = (n + 1) / 2
// so raw byte pairs need the prefix at k AND at half + k.  One workgroup of 256 lanes owns a chunk:
//   1. it sums the lower half (coalesced byte loads, a shuffle tree and four LDS words): t'[half - 1], where the upper half starts;
//   2. it walks both halves together in passes of 256 x 16 positions (RNR_EXR_PASS_BYTES = 2 x 4096 bytes of the chunk): a lane
//      sums its 16 + 16 bytes, the two sums packed into one word (bits 0-7 and 16-23, masked after every add) go through ONE
//      wave scan and a four-word LDS exchange, and the lane then writes its 32 output bytes, adjacent in raw.  The running sums
//      of both halves are carried in registers from pass to pass, so a chunk of any length is many passes of one workgroup.
// Integer arithmetic mod 256 is associative: the bytes do not depend on the order of the scan.  Byte loads and byte stores
// throughout: the source, the half point and the destination have no alignment.
//
// photo_prepare_hdr_kernel: photo.hip's kernel with a HALF / FLOAT source addressed per channel and no / 255.
#include "rnr_internal.h"

#include <math.h>

using namespace rnr;

namespace {

constexpr int UNPACK_LANES = 256;
constexpr int UNPACK_PER_LANE = 16;                                      // positions of EACH half per lane and pass
constexpr int UNPACK_PASS = UNPACK_LANES * UNPACK_PER_LANE;              // positions of each half per pass
static_assert(2 * UNPACK_PASS == RNR_EXR_PASS_BYTES, "rnr_hip.h states the span of one pass");

constexpr uint32_t PAIR_MASK = 0x00ff00ffu;                              // low half's sum in bits 0-7, upper half's in 16-23

}  // namespace

__global__ void __launch_bounds__(UNPACK_LANES)
exr_unpack_kernel(const uint8_t* __restrict__ payload, const int64_t* __restrict__ table, uint8_t* __restrict__ raw) {
    __shared__ uint32_t wave_sum[UNPACK_LANES / 64];
    const int64_t* row = table + 4 * (int64_t)blockIdx.x;
    const uint8_t* t = payload + row[0];
    uint8_t* out = raw + row[1];
    const int64_t n = row[2];
    const int lane = threadIdx.x, wave = lane >> 6;
    if (row[3] == 0) {
        for (int64_t i = lane; i < n; i += UNPACK_LANES) out[i] = t[i];
        return;
    }
    const int64_t half = (n + 1) / 2;
    // 1. t'[half - 1] = 128 + sum_{j < half} (t[j] - 128): the -128 of every step but the first
    uint32_t s = 0;
    for (int64_t i = lane; i < half; i += UNPACK_LANES) s += t[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
    if ((lane & 63) == 0) wave_sum[wave] = s;
    __syncthreads();
    uint32_t low_total = 0;
    for (int w = 0; w < UNPACK_LANES / 64; w++) low_total += wave_sum[w];
    // running sums in front of position k of each half, packed; 128 * half mod 256 is 128 for an odd half
    uint32_t carry = 128u | (((low_total + 128u + (uint32_t)((half & 1) << 7)) & 0xffu) << 16);
    // 2.
    for (int64_t k0 = 0; k0 < half; k0 += UNPACK_PASS) {
        const int64_t k = k0 + (int64_t)lane * UNPACK_PER_LANE;
        uint32_t lo[UNPACK_PER_LANE], hi[UNPACK_PER_LANE];
        uint32_t mine = 0;
        for (int j = 0; j < UNPACK_PER_LANE; j++) {
            // the step of an absent position is 0: t = 128
            lo[j] = k + j < half ? t[k + j] : 128u;
            hi[j] = half + k + j < n ? t[half + k + j] : 128u;
            mine = (mine + ((lo[j] | (hi[j] << 16)) ^ 0x00800080u)) & PAIR_MASK;      // t - 128 = t ^ 128 mod 256
        }
        uint32_t incl = mine;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(incl, o);
            if ((lane & 63) >= o) incl = (incl + up) & PAIR_MASK;
        }
        __syncthreads();                                    // the previous round's readers are done with wave_sum
        if ((lane & 63) == 63) wave_sum[wave] = incl;
        __syncthreads();
        uint32_t before = carry, total = carry;
        for (int w = 0; w < UNPACK_LANES / 64; w++) {
            const uint32_t ws = wave_sum[w];
            if (w < wave) before = (before + ws) & PAIR_MASK;
            total = (total + ws) & PAIR_MASK;
        }
        carry = total;
        uint32_t run = (before + incl + (PAIR_MASK + 0x00010001u - mine)) & PAIR_MASK;      // exclusive: + incl - mine
        for (int j = 0; j < UNPACK_PER_LANE; j++) {
            run = (run + ((lo[j] | (hi[j] << 16)) ^ 0x00800080u)) & PAIR_MASK;
            if (k + j < half) out[2 * (k + j)] = (uint8_t)run;
            if (half + k + j < n) out[2 * (k + j) + 1] = (uint8_t)(run >> 16);
        }
    }
}

extern "C" int rnr_exr_unpack(const uint8_t* payload, const int64_t* table, int num_chunks, uint8_t* raw, void* stream) {
    RNR_REQUIRE(payload && table && raw, "rnr_exr_unpack: payload, table and raw must not be NULL");
    RNR_REQUIRE(num_chunks > 0, "rnr_exr_unpack: num_chunks must be positive, got %d", num_chunks);
    RNR_REQUIRE(aligned_to(8, {table}), "rnr_exr_unpack: table must be 8-byte aligned");
    hipLaunchKernelGGL(exr_unpack_kernel, dim3((unsigned)num_chunks), dim3(UNPACK_LANES), 0, as_stream(stream), payload, table, raw);
    return check_launch("exr_unpack_kernel");
}

namespace {

struct HdrChannel {
    int64_t offset;
    int stride, type;
};

// IEEE binary16 bits -> the float32 of the same value, in integer arithmetic: exact for every pattern whatever the wave's
// denormal mode, and a NaN keeps its payload (numpy's npy_halfbits_to_floatbits does the same)
__device__ __forceinline__ float half_bits_to_float(uint32_t h) {
    const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
    if (e == 0) return __uint_as_float(sign | __float_as_uint((float)m * 5.9604644775390625e-08f));      // m * 2^-24, exact
    if (e == 31) return __uint_as_float(sign | 0x7f800000u | (m << 13));
    return __uint_as_float(sign | ((e + 112u) << 23) | (m << 13));
}

// little-endian loads at any address, from the widest loads that are legal there
__device__ __forceinline__ uint32_t load_u16(const uint8_t* p) {
    if (((uintptr_t)p & 1) == 0) return *reinterpret_cast<const uint16_t*>(p);
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8);
}

__device__ __forceinline__ uint32_t load_u32(const uint8_t* p) {
    if (((uintptr_t)p & 3) == 0) return *reinterpret_cast<const uint32_t*>(p);
    if (((uintptr_t)p & 1) == 0)
        return (uint32_t) * reinterpret_cast<const uint16_t*>(p) | ((uint32_t) * reinterpret_cast<const uint16_t*>(p + 2) << 16);
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

}  // namespace

__global__ void __launch_bounds__(256)
photo_prepare_hdr_kernel(const uint8_t* __restrict__ src, int64_t row_bytes, HdrChannel c0, HdrChannel c1, HdrChannel c2, int crop_y0,
                         int crop_x0, int crop_h, int crop_w, double gamma, float* __restrict__ dst, int dh, int dw) {
    const long npix = (long)dh * dw;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const int dx = (int)(i % dw), dy = (int)(i / dw);
    // (y, x) below are window coordinates, 0 <= y < crop_h and 0 <= x < crop_w: inside the image by the entry point's checks
    float acc[3];
    resize_area_pixel<3>(dy, dx, crop_h, crop_w, dh, dw,
                         [&](int y, int x, int k) {
                             const HdrChannel& c = k == 0 ? c0 : (k == 1 ? c1 : c2);
                             const uint8_t* p = src + (int64_t)(crop_y0 + y) * row_bytes + c.offset + (int64_t)(crop_x0 + x) * c.stride;
                             return c.type == RNR_EXR_HALF ? half_bits_to_float(load_u16(p)) : __uint_as_float(load_u32(p));
                         },
                         acc);
    for (int k = 0; k < 3; k++) dst[k * npix + i] = gamma == 1.0 ? acc[k] : (float)pow((double)acc[k], gamma);
}

extern "C" int rnr_photo_prepare_hdr(const uint8_t* src, int src_h, int src_w, int64_t row_bytes, int64_t r_offset, int r_stride,
                                     int r_type, int64_t g_offset, int g_stride, int g_type, int64_t b_offset, int b_stride,
                                     int b_type, int crop_y0, int crop_x0, int crop_h, int crop_w, double gamma, float* dst,
                                     int dst_h, int dst_w, void* stream) {
    RNR_REQUIRE(src && dst, "rnr_photo_prepare_hdr: src and dst must not be NULL");
    RNR_REQUIRE(src_h > 0 && src_w > 0 && crop_h > 0 && crop_w > 0 && dst_h > 0 && dst_w > 0,
                "rnr_photo_prepare_hdr: sizes must be positive (src %d x %d, crop %d x %d, dst %d x %d)", src_h, src_w, crop_h, crop_w,
                dst_h, dst_w);
    RNR_REQUIRE(row_bytes > 0, "rnr_photo_prepare_hdr: row_bytes must be positive, got %ld", (long)row_bytes);
    const HdrChannel ch[3] = {{r_offset, r_stride, r_type}, {g_offset, g_stride, g_type}, {b_offset, b_stride, b_type}};
    for (int k = 0; k < 3; k++) {
        const HdrChannel& c = ch[k];
        RNR_REQUIRE(c.type == RNR_EXR_HALF || c.type == RNR_EXR_FLOAT,
                    "rnr_photo_prepare_hdr: channel %c has unknown type %d (RNR_EXR_HALF = %d, RNR_EXR_FLOAT = %d)", "RGB"[k], c.type,
                    RNR_EXR_HALF, RNR_EXR_FLOAT);
        const int size = c.type == RNR_EXR_HALF ? 2 : 4;
        RNR_REQUIRE(c.offset >= 0 && c.stride >= size && c.offset + (int64_t)(src_w - 1) * c.stride + size <= row_bytes,
                    "rnr_photo_prepare_hdr: channel %c (offset %ld, stride %d, %d-byte values, %d columns) does not fit inside "
                    "row_bytes = %ld", "RGB"[k], (long)c.offset, c.stride, size, src_w, (long)row_bytes);
    }
    RNR_REQUIRE(crop_y0 >= 0 && crop_x0 >= 0 && (long)crop_y0 + crop_h <= src_h && (long)crop_x0 + crop_w <= src_w,
                "rnr_photo_prepare_hdr: crop window [%d, %ld) x [%d, %ld) is not inside the %d x %d image", crop_y0,
                (long)crop_y0 + crop_h, crop_x0, (long)crop_x0 + crop_w, src_h, src_w);
    RNR_REQUIRE(isfinite(gamma) && gamma > 0.0, "rnr_photo_prepare_hdr: gamma must be finite and > 0, got %g", gamma);
    RNR_REQUIRE(aligned_to(4, {dst}), "rnr_photo_prepare_hdr: dst must be 4-byte aligned");
    const long npix = (long)dst_h * dst_w;
    hipLaunchKernelGGL(photo_prepare_hdr_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, as_stream(stream), src, row_bytes,
                       ch[0], ch[1], ch[2], crop_y0, crop_x0, crop_h, crop_w, gamma, dst, dst_h, dst_w);
    return check_launch("photo_prepare_hdr_kernel");
}
