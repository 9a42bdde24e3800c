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
//
// OpenEXR out.  exr_pack_kernel: float32 RGB images -> the bytes handed to deflate (or stored as they are).  Coding has no scan:
// with u[k] the k-th 16-bit unit of a chunk (a half value, or one half of a float's bits), lo / hi its bytes and m = n / 2 units,
//   coded[k] = lo(k) - lo(k-1) + 128,  coded[m + k] = hi(k) - hi(k-1) + 128  (mod 256),  coded[0] = lo(0),  coded[m] = hi(0) - lo(m-1) + 128
// so the grid is (image, chunk, segment of the chunk) and every lane makes 16 consecutive bytes of EACH half from 16 units it loads
// itself plus ONE more value: its predecessor u[k-1], or for the chunk's first lane the chunk's last unit (the junction).  A lane
// stores its 16 bytes as dwords between the single bytes that bring the address to a multiple of 4 (the half point m and a chunk's
// start have no alignment).  No LDS, no barrier, no lane exchange.
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

namespace {

constexpr int PACK_LANES = 256;
constexpr int PACK_UNITS = 16;                                           // 16-bit units of the chunk per lane: bytes of each half
static_assert(PACK_LANES * PACK_UNITS == RNR_EXR_PACK_SEGMENT, "rnr_hip.h states the units of one workgroup");

struct PackArgs {
    const uint32_t* src;                                                 // the floats' bit patterns
    int64_t image_stride, row_stride, x_stride;
    int64_t offset[3];                                                   // of B, G, R: the order of the runs in a scanline
    int height, width, lines;
    uint32_t chunks, segments;
    uint8_t* dst;
};

// float32 bits -> IEEE binary16 bits, as include/rnr_hip.h states it at rnr_exr_pack.  Integer arithmetic only.
__device__ __forceinline__ uint32_t float_bits_to_half(uint32_t f) {
    const uint32_t sign = (f >> 16) & 0x8000u, a = f & 0x7fffffffu;
    if (a > 0x7f800000u) {
        const uint32_t m = (a & 0x007fffffu) >> 13;
        return sign | 0x7c00u | m | (uint32_t)(m == 0);
    }
    if (a >= 0x477ff000u) return sign | 0x7c00u;                         // 65520, the tie between 65504 and 2^16, and all above: inf
    uint32_t h, rest, mid;
    if (a >= 0x38800000u) {                                              // >= 2^-14: a half normal
        const uint32_t r = a - 0x38000000u;                              // exponent rebiased by 112
        h = r >> 13, rest = r & 0x1fffu, mid = 0x1000u;                  // a carry out of the mantissa is the next exponent
    } else {
        const uint32_t e = a >> 23;
        if (e < 102u) return sign;                                       // < 2^-25: below half of the smallest subnormal
        const uint32_t m = (a & 0x007fffffu) | 0x00800000u, s = 126u - e;      // value = m * 2^(e - 150) = (m >> s) * 2^-24, s in 14..24
        h = m >> s, rest = m & ((1u << s) - 1u), mid = 1u << (s - 1u);
    }
    h += (uint32_t)(rest > mid || (rest == mid && (h & 1u)));
    return sign | h;
}

// bytes [0, count) of the little-endian words w to p, p at any address.  A full lane (count = 4 NW): single bytes up to the next
// multiple of 4, whole dwords, single bytes behind the last; a ragged lane (the end of a chunk's half): single bytes.
template <int NW>
__device__ __forceinline__ void store_bytes(uint8_t* p, const uint32_t (&w)[NW], int count) {
    if (count < 4 * NW) {
#pragma unroll
        for (int j = 0; j < 4 * NW; j++)
            if (j < count) p[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
        return;
    }
    const int head = (int)(-(uintptr_t)p & 3);
    if (head == 0) {
#pragma unroll
        for (int i = 0; i < NW; i++) reinterpret_cast<uint32_t*>(p)[i] = w[i];
        return;
    }
    const int sh = 8 * head;                                             // 8, 16 or 24
#pragma unroll
    for (int j = 0; j < 3; j++)
        if (j < head) p[j] = (uint8_t)(w[0] >> (8 * j));
    uint32_t* q = reinterpret_cast<uint32_t*>(p + head);
#pragma unroll
    for (int i = 0; i + 1 < NW; i++) q[i] = (w[i] >> sh) | (w[i + 1] << (32 - sh));
    const uint32_t last = w[NW - 1] >> sh;
    uint8_t* t = p + head + 4 * (NW - 1);
#pragma unroll
    for (int j = 0; j < 3; j++)
        if (j < 4 - head) t[j] = (uint8_t)(last >> (8 * j));
}

}  // namespace

template <int TYPE, int CODED>
__global__ void __launch_bounds__(PACK_LANES) exr_pack_kernel(PackArgs a) {
    constexpr uint32_t UPV = TYPE == RNR_EXR_HALF ? 1 : 2;               // units per value
    constexpr int NV = PACK_UNITS / UPV;                                 // values per lane
    const uint32_t seg = blockIdx.x % a.segments, rest = blockIdx.x / a.segments;
    const uint32_t chunk = rest % a.chunks, image = rest / a.chunks;
    const int y0 = (int)chunk * a.lines;
    const uint32_t nl = (uint32_t)min(a.lines, a.height - y0);
    const uint32_t W = (uint32_t)a.width, row_values = 3u * W;
    const uint32_t units = nl * row_values * UPV;                        // n / 2 <= 2^30: the entry point bounds height * row_bytes
    const uint32_t k0 = (seg * PACK_LANES + threadIdx.x) * PACK_UNITS;
    if (k0 >= units) return;
    const int cnt = (int)min((uint32_t)PACK_UNITS, units - k0);          // a multiple of UPV, as units and k0 are
    const uint32_t* img = a.src + (int64_t)image * a.image_stride + (int64_t)y0 * a.row_stride;
    auto load = [&](uint32_t line, uint32_t ch, uint32_t x) {
        return img[(int64_t)line * a.row_stride + (int64_t)x * a.x_stride + (ch == 0 ? a.offset[0] : (ch == 1 ? a.offset[1] : a.offset[2]))];
    };
    const uint32_t v0 = k0 / UPV;
    uint32_t line = v0 / row_values, ch = (v0 - line * row_values) / W, x = v0 - line * row_values - ch * W;
    uint32_t prev = 0;                                                   // lo in bits 0-7, hi in bits 16-23, of the unit in front
    if (CODED) {
        if (k0 == 0) {                                                   // coded[0] = lo(0); coded[m] = hi(0) - lo(m - 1) + 128
            const uint32_t bits = load(nl - 1, 2, W - 1);
            const uint32_t last = TYPE == RNR_EXR_HALF ? float_bits_to_half(bits) : bits >> 16;
            prev = 128u | ((last & 0xffu) << 16);
        } else {
            uint32_t pl = line, pc = ch, px = x;
            if (px == 0) {
                px = W;
                if (pc == 0) pc = 3, pl--;
                pc--;
            }
            px--;
            const uint32_t bits = load(pl, pc, px);
            const uint32_t u = TYPE == RNR_EXR_HALF ? float_bits_to_half(bits) : bits >> 16;
            prev = (u & 0xffu) | ((u >> 8) << 16);
        }
    }
    uint32_t unit[PACK_UNITS];
#pragma unroll
    for (int j = 0; j < NV; j++) {
        uint32_t bits = 0;
        if (j * (int)UPV < cnt) {
            bits = load(line, ch, x);
            if (++x == W) {
                x = 0;
                if (++ch == 3) ch = 0, line++;
            }
        }
        if constexpr (TYPE == RNR_EXR_HALF) {
            unit[j] = float_bits_to_half(bits);
        } else {
            unit[2 * j] = bits & 0xffffu;
            unit[2 * j + 1] = bits >> 16;
        }
    }
    uint8_t* out = a.dst + (int64_t)image * ((int64_t)a.height * row_values * (2 * UPV)) + (int64_t)y0 * row_values * (2 * UPV);
    if (!CODED) {
        uint32_t w[PACK_UNITS / 2];
#pragma unroll
        for (int i = 0; i < PACK_UNITS / 2; i++) w[i] = unit[2 * i] | (unit[2 * i + 1] << 16);
        store_bytes(out + 2 * (int64_t)k0, w, 2 * cnt);
        return;
    }
    uint32_t lo[PACK_UNITS / 4] = {}, hi[PACK_UNITS / 4] = {};
#pragma unroll
    for (int j = 0; j < PACK_UNITS; j++) {
        const uint32_t pair = (unit[j] & 0xffu) | ((unit[j] >> 8) << 16);
        // both differences + 128 at once: bit 8 and bit 24 lend what a field borrows, the mask drops them
        const uint32_t d = ((pair | 0x01000100u) - prev + 0x00800080u) & 0x00ff00ffu;
        prev = pair;
        lo[j >> 2] |= (d & 0xffu) << (8 * (j & 3));
        hi[j >> 2] |= (d >> 16) << (8 * (j & 3));
    }
    store_bytes(out + k0, lo, cnt);
    store_bytes(out + (int64_t)units + k0, hi, cnt);
}

extern "C" int rnr_exr_pack(const float* src, int num_images, int height, int width, int64_t image_stride, int64_t row_stride,
                            int64_t x_stride, int64_t r_offset, int64_t g_offset, int64_t b_offset, int pixel_type,
                            int lines_per_chunk, int coded, uint8_t* dst, void* stream) {
    RNR_REQUIRE(src && dst, "rnr_exr_pack: src and dst must not be NULL");
    RNR_REQUIRE(num_images > 0 && height > 0 && width > 0, "rnr_exr_pack: sizes must be positive (%d images of %d x %d)", num_images,
                height, width);
    RNR_REQUIRE(image_stride >= 0 && row_stride >= 0 && x_stride >= 0 && r_offset >= 0 && g_offset >= 0 && b_offset >= 0,
                "rnr_exr_pack: strides and offsets must not be negative (image %ld, row %ld, x %ld; r %ld, g %ld, b %ld)",
                (long)image_stride, (long)row_stride, (long)x_stride, (long)r_offset, (long)g_offset, (long)b_offset);
    RNR_REQUIRE(pixel_type == RNR_EXR_HALF || pixel_type == RNR_EXR_FLOAT,
                "rnr_exr_pack: unknown pixel_type %d (RNR_EXR_HALF = %d, RNR_EXR_FLOAT = %d)", pixel_type, RNR_EXR_HALF, RNR_EXR_FLOAT);
    RNR_REQUIRE(coded == 0 || coded == 1, "rnr_exr_pack: coded must be 0 or 1, got %d", coded);
    RNR_REQUIRE(lines_per_chunk > 0, "rnr_exr_pack: lines_per_chunk must be positive, got %d", lines_per_chunk);
    RNR_REQUIRE(aligned_to(4, {src}), "rnr_exr_pack: src must be 4-byte aligned");
    const int64_t row_bytes = 3 * (int64_t)width * (pixel_type == RNR_EXR_HALF ? 2 : 4);
    RNR_REQUIRE(row_bytes * height <= (int64_t)RNR_EXR_MAX_RAW_BYTES,
                "rnr_exr_pack: %d x %d pixels of %d bytes exceed RNR_EXR_MAX_RAW_BYTES = %ld", width, height, (int)(row_bytes / width),
                (long)RNR_EXR_MAX_RAW_BYTES);
    const int lines = lines_per_chunk < height ? lines_per_chunk : height;
    const int64_t chunks = ((int64_t)height + lines - 1) / lines;
    const int64_t segments = (lines * row_bytes / 2 + RNR_EXR_PACK_SEGMENT - 1) / RNR_EXR_PACK_SEGMENT;
    const int64_t groups = (int64_t)num_images * chunks * segments;
    RNR_REQUIRE(groups <= 0x7fffffffLL, "rnr_exr_pack: %d images of %ld chunks of %ld segments are more than 2^31 - 1 workgroups",
                num_images, (long)chunks, (long)segments);
    const PackArgs a = {reinterpret_cast<const uint32_t*>(src), image_stride, row_stride, x_stride, {b_offset, g_offset, r_offset},
                        height, width, lines, (uint32_t)chunks, (uint32_t)segments, dst};
    const dim3 grid((unsigned)groups), block(PACK_LANES);
    if (pixel_type == RNR_EXR_HALF) {
        if (coded) hipLaunchKernelGGL((exr_pack_kernel<RNR_EXR_HALF, 1>), grid, block, 0, as_stream(stream), a);
        else hipLaunchKernelGGL((exr_pack_kernel<RNR_EXR_HALF, 0>), grid, block, 0, as_stream(stream), a);
    } else {
        if (coded) hipLaunchKernelGGL((exr_pack_kernel<RNR_EXR_FLOAT, 1>), grid, block, 0, as_stream(stream), a);
        else hipLaunchKernelGGL((exr_pack_kernel<RNR_EXR_FLOAT, 0>), grid, block, 0, as_stream(stream), a);
    }
    return check_launch("exr_pack_kernel");
}
