// Tiled, order-preserving z-resolve rasterizer for gfx950 + fused G-buffer attribute interpolation.
//
// Replaces (does not translate) the reference's brute-force forward kernels
//   forward_face_index_map_cuda_kernel_1/2  rasterize_cuda_kernel.cu:24-169   (O(pixels x faces))
//   forward_texture_sampling_cuda_kernel    rasterize_cuda_kernel.cu:171-242
// and, in the fused entry point, the torch glue of network.Rasterizer.forward (network.py:156-214).
//
// Design:
//   1. face_setup (one lane per (view, face)): back-face predicate, the 3x3 barycentric inverse (same IEEE
//      binary32 operation sequence as the reference, this file is built with -ffp-contract=off), and a
//      conservative pixel bounding box.  Faces whose box cannot be trusted (degenerate / sliver / non-finite)
//      are flagged and decided by the exact tile test (may_touch_tile).
//   2. What becomes of a face, in the same lane.  near >= 0, the product path: setup_splat_faces_kernel goes on
//      from the setup's registers — a face whose trusted box covers <= 256 pixels walks them itself
//      (splat_pixels) and folds (depth bits, face index) into a per-pixel 64-bit key with one atomicMin; every
//      other face takes bin_or_list_face: a trusted box over at most 64 tiles is binned into the 16x16-pixel
//      tiles it touches (exact, rounding-monotone tile test), untrusted boxes and huge faces go to a per-view
//      wide list, which every tile of raster_tile_kernel tests against itself (records of six coordinates +
//      index, 1024 per round trip).  With at most two views in the launch four lanes share a face (box rows
//      modulo 4).  near < 0, where the key order does not hold: face_setup_kernel, then bin_faces_kernel puts
//      every face through bin_or_list_face.
//   3. raster_tile_kernel, one 256-thread workgroup per tile: evaluates the reference's per-candidate
//      arithmetic for its binned candidates on LDS-broadcast face records — unordered lists, so the
//      reference's "ascending faces, strict <" rule is applied in its order-free form (smallest zp, ties ->
//      smallest face index) —, walks the zero-area wide faces (two coincident vertices: the pole faces of a UV sphere)
//      along their line — only the two pixels next to the line's crossing of a row / column can pass the reference's
//      inside test, see walk_lines —, merges the winner with the pixel's key, and writes either the extension's maps
//      (drop-in mode) or the perspective-corrected attribute interpolation of network.py:176-214, already
//      vertically flipped.  A tile whose list overflowed rescans every face box itself (the in-order ballot
//      scan of round 1, kept as the fallback: capacity never changes results).
//   face_index_map, weight_map and depth_map are bit-identical to the reference evaluated without FMA
//   contraction (tests/test_gpu_raster.py, tests/golden/raster_*.npz).
#include "rnr_internal.h"

namespace rnr {

constexpr int TILE = 16;
constexpr int RTHREADS = 256;
constexpr int SCAN_ITEMS = 4;
constexpr int SCAN_CHUNK = RTHREADS * SCAN_ITEMS;
constexpr int FLUSH_EVERY = 4;                          // scan steps between queue-level checks (one barrier each)
constexpr int QCAP = (FLUSH_EVERY + 2) * SCAN_CHUNK;    // a flush is forced once more than 2 chunks are queued
constexpr int STAGE = 128;                             // candidates staged in LDS per evaluation batch
constexpr int STAGE_FLOATS = 24;

struct __attribute__((aligned(8))) FaceBox {
    short xlo, xhi, ylo, yhi;  // inclusive pixel-index bounds, rows in the kernel's native (unflipped) order
};
// xlo == BOX_EXACT : bounding box not trustworthy, the exact tile test decides
// empty_box()     : never a candidate (back face, or entirely off-screen)
constexpr short BOX_EXACT = -2;
// a box that overlaps no tile under the interval test `lo <= t_hi && hi >= t_lo` (lo > every tile index, hi < 0)
__host__ __device__ __forceinline__ FaceBox empty_box() {
    FaceBox b;
    b.xlo = 32767; b.xhi = -1; b.ylo = 32767; b.yhi = -1;
    return b;
}

__device__ __forceinline__ bool backface(const float* f) {
    // rasterize_cuda_kernel.cu:40 / :111
    return (f[7] - f[1]) * (f[3] - f[0]) < (f[4] - f[1]) * (f[6] - f[0]);
}

__device__ __forceinline__ float pix_center(int i, int is) {
    // rasterize_cuda_kernel.cu:93-94: (2*i + 1 - is) / is  (exact small integer, one correctly rounded divide)
    return (float)(2 * i + 1 - is) / (float)is;
}
// pix_center for the loops that take many centres: where `is` is a power of two, (2i + 1 - is) / is == (2i + 1 - is) * (1 / is)
// exactly (both are exact), without the division sequence per pixel.  pow2 may be a compile-time constant (splat_pixels).
struct PixCenter {
    int is;
    float inv_is;
    bool pow2;
    __device__ __forceinline__ PixCenter(int is_, bool pow2_) : is(is_), inv_is(1.0f / (float)is_), pow2(pow2_) {}
    __device__ __forceinline__ float operator()(int i) const { return pow2 ? (float)(2 * i + 1 - is) * inv_is : pix_center(i, is); }
};
__host__ __device__ __forceinline__ bool is_pow2(int is) { return (is & (is - 1)) == 0; }

// ------------------------------------------------------------------------------------------------
// 1. per-face setup
// ------------------------------------------------------------------------------------------------
// Setup of face i: writes faces_out (GATHER) / faces_inv / boxes and leaves the same values in f / inv / box for a caller
// that goes on with them (setup_splat_faces_kernel).  False = back face (inv undefined).
template <bool GATHER>
__device__ __forceinline__ bool face_setup(long i, const float* __restrict__ faces_in, const float* __restrict__ v_uvz,
                                           const int32_t* __restrict__ fidx, float* __restrict__ faces_out,
                                           float* __restrict__ faces_inv, FaceBox* __restrict__ boxes, int nf, int nv, int is,
                                           float (&f)[9], float (&inv)[9], FaceBox& box, bool write = true) {
    if (GATHER) {  // vertices_to_faces.py:4-25 fused in
        const int bn = (int)(i / nf), fn = (int)(i % nf);
#pragma unroll
        for (int v = 0; v < 3; v++) {
            const int vi = fidx[3 * fn + v];
            const float* p = v_uvz + ((long)bn * nv + vi) * 3;
            f[3 * v + 0] = p[0];
            f[3 * v + 1] = p[1];
            f[3 * v + 2] = p[2];
        }
#pragma unroll
        for (int k = 0; k < 9; k++) if (write) faces_out[i * 9 + k] = f[k];
    } else {
#pragma unroll
        for (int k = 0; k < 9; k++) f[k] = faces_in[i * 9 + k];
    }
    if (backface(f)) {  // reference returns before writing: caller's zero fill stays (rasterize.py:163)
        box = empty_box();
        if (write) boxes[i] = box;
        if (GATHER && write) {
#pragma unroll
            for (int k = 0; k < 9; k++) faces_inv[i * 9 + k] = 0.0f;
        }
        return false;
    }
    // ---- barycentric inverse, rasterize_cuda_kernel.cu:44-66 (operation order preserved) ----
    const float s = (float)is;
    float px[3], py[3];
#pragma unroll
    for (int v = 0; v < 3; v++) {
        px[v] = 0.5f * (f[3 * v + 0] * s + s - 1.0f);
        py[v] = 0.5f * (f[3 * v + 1] * s + s - 1.0f);
    }
    float m[9];
    m[0] = py[1] - py[2]; m[1] = px[2] - px[1]; m[2] = px[1] * py[2] - px[2] * py[1];
    m[3] = py[2] - py[0]; m[4] = px[0] - px[2]; m[5] = px[2] * py[0] - px[0] * py[2];
    m[6] = py[0] - py[1]; m[7] = px[1] - px[0]; m[8] = px[0] * py[1] - px[1] * py[0];
    const float den = px[2] * (py[0] - py[1]) + px[0] * (py[1] - py[2]) + px[1] * (py[2] - py[0]);
#pragma unroll
    for (int k = 0; k < 9; k++) { inv[k] = m[k] / den; if (write) faces_inv[i * 9 + k] = inv[k]; }

    // ---- conservative pixel bounding box (double; DESIGN.md §Rasterizer gives the bound) ----
    const double x0 = f[0], y0 = f[1], x1 = f[3], y1 = f[4], x2 = f[6], y2 = f[7];
    const double minx = fmin(x0, fmin(x1, x2)), maxx = fmax(x0, fmax(x1, x2));
    const double miny = fmin(y0, fmin(y1, y2)), maxy = fmax(y0, fmax(y1, y2));
    const double maxabs = fmax(fmax(fabs(minx), fabs(maxx)), fmax(fabs(miny), fabs(maxy)));
    const double ax = x1 - x0, ay = y1 - y0, bx = x2 - x0, by = y2 - y0, cx = x2 - x1, cy = y2 - y1;
    const double area2 = fabs(ax * by - bx * ay);
    const double l2 = fmax(ax * ax + ay * ay, fmax(bx * bx + by * by, cx * cx + cy * cy));
    const double sin_min = area2 / l2;                         // <= sin(smallest interior angle)
    const double u = 5.9604644775390625e-08;                   // 2^-24
    const double pad_ndc = 4.0 * (32.0 * u * (1.0 + maxabs) / sin_min);
    const double pad_px = pad_ndc * is * 0.5 + 1.0;
    const bool finite = isfinite(maxabs);
    if (!finite || !(sin_min > 0.0) || !(pad_px <= 16.0)) {
        box.xlo = BOX_EXACT; box.xhi = (short)(is - 1); box.ylo = 0; box.yhi = (short)(is - 1);
    } else {
        // pixel i has its centre at NDC (2i + 1 - is) / is, i.e. NDC x is the pixel coordinate (x * is + is - 1) / 2: the pixels
        // whose centre lies within pad_ndc (>= 10 x the proven distance bound) of the face's extent are exactly
        // [ceil(lo), floor(hi)].  (Until r06 the box carried up to four further pixels per side — the +1 of pad_px, which
        // belongs to the trust criterion above, a -1 / +1 here, and floor / ceil the other way round — and a pixel-sized face
        // of the 65 536-face sphere walked 80 pixels instead of 30.)
        double lx = ceil(((minx - pad_ndc) * is + is - 1) * 0.5);
        double hx = floor(((maxx + pad_ndc) * is + is - 1) * 0.5);
        double ly = ceil(((miny - pad_ndc) * is + is - 1) * 0.5);
        double hy = floor(((maxy + pad_ndc) * is + is - 1) * 0.5);
        lx = fmax(lx, 0.0); ly = fmax(ly, 0.0);
        hx = fmin(hx, (double)(is - 1)); hy = fmin(hy, (double)(is - 1));
        if (lx > hx || ly > hy) {
            box = empty_box();
        } else {
            box.xlo = (short)lx; box.xhi = (short)hx; box.ylo = (short)ly; box.yhi = (short)hy;
        }
    }
    if (write) boxes[i] = box;
    return true;
}

struct FaceSetupArgs {
    const float* faces_in; const float* v_uvz; const int32_t* fidx; int nv;     // GATHER: v_uvz / fidx / nv, else faces_in
    float* faces_out; float* faces_inv; FaceBox* boxes;                          // faces_out: GATHER only
};

template <bool GATHER>
__global__ void __launch_bounds__(256)
face_setup_kernel(const float* __restrict__ faces_in, const float* __restrict__ v_uvz,
                  const int32_t* __restrict__ fidx, float* __restrict__ faces_out,
                  float* __restrict__ faces_inv, FaceBox* __restrict__ boxes, int batch, int nf, int nv,
                  int is) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)batch * nf) return;
    float f[9], inv[9];
    FaceBox box;
    face_setup<GATHER>(i, faces_in, v_uvz, fidx, faces_out, faces_inv, boxes, nf, nv, is, f, inv, box);
}

// Exact conservative tile test.  The reference rejects pixel p for edge a->b iff
//     fl(fl(yp - ya) * fl(xb - xa)) < fl(fl(xp - xa) * fl(yb - ya))          (rasterize_cuda_kernel.cu:115-117)
// Rounding is monotone, so over a tile the left product lies between its values at the tile's first/last
// row and the right product between its values at the first/last column.  If all four corner comparisons
// say "reject", every pixel of the tile rejects.  Any NaN makes a comparison false => tile kept.
__device__ __forceinline__ bool edge_rejects_tile(float xa, float ya, float xb, float yb, float xlo,
                                                  float xhi, float ylo, float yhi) {
    const float dx = xb - xa, dy = yb - ya;
    const float p0 = (ylo - ya) * dx, p1 = (yhi - ya) * dx;
    const float q0 = (xlo - xa) * dy, q1 = (xhi - xa) * dy;
    return (p0 < q0) && (p0 < q1) && (p1 < q0) && (p1 < q1);
}
// the centres of a tile's first / last column and row: what the test above needs of tile (tx, ty)
struct TileBounds { float xlo, xhi, ylo, yhi; };
__device__ __forceinline__ TileBounds tile_bounds(int tx, int ty, int is) {
    const int tx0 = tx * TILE, ty0 = ty * TILE;
    const int tx1 = min(tx0 + TILE - 1, is - 1), ty1 = min(ty0 + TILE - 1, is - 1);
    return {pix_center(tx0, is), pix_center(tx1, is), pix_center(ty0, is), pix_center(ty1, is)};
}
__device__ __forceinline__ bool may_touch_tile(float x0, float y0, float x1, float y1, float x2, float y2, const TileBounds t) {
    return !(edge_rejects_tile(x0, y0, x1, y1, t.xlo, t.xhi, t.ylo, t.yhi) || edge_rejects_tile(x1, y1, x2, y2, t.xlo, t.xhi, t.ylo, t.yhi) ||
             edge_rejects_tile(x2, y2, x0, y0, t.xlo, t.xhi, t.ylo, t.yhi));
}

// ------------------------------------------------------------------------------------------------
// 1b. face-parallel binning: O(faces x tiles-per-face) instead of every tile scanning every face.
//     Each kept face is appended (LDS-free, one global atomic per (face, tile)) to the candidate list of every tile
//     whose exact tile test it survives.  Lists are unordered; the z-resolve is order-free.  Faces whose box is not
//     trustworthy (BOX_EXACT) or spans many tiles go to a per-view "wide" list, which every tile of raster_tile_kernel
//     tests against itself (a launch of its own until r04: 10 - 26 us for a list that is empty on the bench scene).  A tile
//     whose list overflows BIN_CAP falls back to scanning all boxes itself, so capacity never affects results.
// ------------------------------------------------------------------------------------------------
constexpr int BIN_CAP = 2048;
constexpr int WIDE_TILES = 64;
// A face on the wide list leaves the record every tile tests: (x0, y0, x1, y1) (x2, y2, face index, -) — two 16-byte loads
// at consecutive addresses per lane, where the tile kernel used to chase index -> box -> nine floats at a stride of 36 bytes
// through three dependent round trips per 256 wide faces (the 65 536-face sphere has 520 of them, its zero-area pole faces:
// 42 of the tile kernel's 52 us at one view per call, r06).
constexpr int WIDE_REC_FLOATS = 8;

// what the binning writes: per view, candidate lists of the tiles and the wide list
struct BinLists {
    int* tile_count;    // [B,ntiles]  candidates binned per tile (may exceed BIN_CAP: then the tile rescans)
    int* tile_list;     // [B,ntiles,BIN_CAP]
    int* wide_count;    // [B]
    float* wide_rec;    // [B,nf,WIDE_REC_FLOATS]
};

__device__ __forceinline__ bool box_is_empty(const FaceBox b) { return b.xlo != BOX_EXACT && b.xlo > b.xhi; }  // empty_box()
// a box that is not empty as pixel ranges inside the image (all of it for an untrusted box, `exact`)
struct PixBox {
    int xa, xb, ya, yb;
    bool exact;
    __device__ __forceinline__ int pixels() const { return (xb - xa + 1) * (yb - ya + 1); }
};
__device__ __forceinline__ PixBox pix_box(const FaceBox b) {
    return {max((int)b.xlo, 0), b.xhi, max((int)b.ylo, 0), b.yhi, b.xlo == BOX_EXACT};
}

// Face fn of view bn (box p, coordinates in f[0..8]) is not resolved by its own lane: it is appended to the list of every tile
// it may touch, or — untrusted box, or more than WIDE_TILES tiles — to the view's wide list.
__device__ __forceinline__ void bin_or_list_face(const BinLists L, const PixBox p, const float* f, int bn, int fn, int nf, int is) {
    const int tiles_x = (is + TILE - 1) / TILE;
    const int txa = p.xa / TILE, txb = p.xb / TILE, tya = p.ya / TILE, tyb = p.yb / TILE;
    if (p.exact || (txb - txa + 1) * (tyb - tya + 1) > WIDE_TILES) {
        const int pos = atomicAdd(L.wide_count + bn, 1);
        float4* r = reinterpret_cast<float4*>(L.wide_rec + ((size_t)bn * nf + pos) * WIDE_REC_FLOATS);
        r[0] = make_float4(f[0], f[1], f[3], f[4]);
        r[1] = make_float4(f[6], f[7], __builtin_bit_cast(float, fn), 0.0f);
        return;
    }
    int* tc = L.tile_count + (size_t)bn * tiles_x * tiles_x;
    int* tl = L.tile_list + (size_t)bn * tiles_x * tiles_x * BIN_CAP;
    for (int ty = tya; ty <= tyb; ty++)
        for (int tx = txa; tx <= txb; tx++) {
            if (!may_touch_tile(f[0], f[1], f[3], f[4], f[6], f[7], tile_bounds(tx, ty, is))) continue;
            const int tile = ty * tiles_x + tx;
            const int slot = atomicAdd(tc + tile, 1);
            if (slot < BIN_CAP) tl[(size_t)tile * BIN_CAP + slot] = fn;
        }
}

__global__ void __launch_bounds__(256)
bin_faces_kernel(const float* __restrict__ faces, const FaceBox* __restrict__ boxes, int* __restrict__ tile_count,
                 int* __restrict__ tile_list, int* __restrict__ wide_count, float* __restrict__ wide_rec, int batch, int nf, int is) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)batch * nf) return;
    const FaceBox b = boxes[i];
    if (box_is_empty(b)) return;
    bin_or_list_face({tile_count, tile_list, wide_count, wide_rec}, pix_box(b), faces + i * 9, (int)(i / nf), (int)(i % nf), nf, is);
}

// The reference's per-(face, pixel) candidate arithmetic (rasterize_cuda_kernel.cu:115-139) on a 24-float face record
//   r0 = (x0, y0, x1, y1)  r1 = (x2, y2, x1-x0, y1-y0)  r2 = (x2-x1, y2-y1, x0-x2, y0-y2)                 the edge half
//   r3 = (inv0..3)  r4 = (inv4..7)  r5 = (inv8, z0, z1, z2)                                                the depth half
// One record, one builder per half and one definition of the arithmetic for the pixel walk (splat_pixels), the tile queue
// (LDS-broadcast records) and the line walk: the same (face, pixel) gives the same bits on every path.
struct FaceEdges { float4 r0, r1, r2; };
struct FaceDepth { float4 r3, r4, r5; };
struct FaceRec { FaceEdges e; FaceDepth d; };
static_assert(sizeof(FaceRec) == STAGE_FLOATS * sizeof(float), "the LDS image of a record");

__device__ __forceinline__ FaceEdges face_edges(float x0, float y0, float x1, float y1, float x2, float y2) {
    return {make_float4(x0, y0, x1, y1), make_float4(x2, y2, x1 - x0, y1 - y0), make_float4(x2 - x1, y2 - y1, x0 - x2, y0 - y2)};
}
// f / fi: the face's 9 + 9 floats (global memory or the registers of the setup that has just produced them)
__device__ __forceinline__ FaceDepth face_depth(const float* f, const float* fi) {
    return {make_float4(fi[0], fi[1], fi[2], fi[3]), make_float4(fi[4], fi[5], fi[6], fi[7]), make_float4(fi[8], f[2], f[5], f[8])};
}
__device__ __forceinline__ FaceRec face_rec(const float* f, const float* fi) {
    return {face_edges(f[0], f[1], f[3], f[4], f[6], f[7]), face_depth(f, fi)};
}

__device__ __forceinline__ bool cand_inside(const FaceEdges e, float xp, float yp) {
    // inside test (rasterize_cuda_kernel.cu:115-118)
    if ((yp - e.r0.y) * e.r1.z < (xp - e.r0.x) * e.r1.w) return false;
    if ((yp - e.r0.w) * e.r2.x < (xp - e.r0.z) * e.r2.y) return false;
    if ((yp - e.r1.y) * e.r2.z < (xp - e.r1.x) * e.r2.w) return false;
    return true;
}
__device__ __forceinline__ bool cand_depth(const FaceDepth d, float fxi, float fyi, float near_, float far_, float& zp, float& w0,
                                           float& w1, float& w2) {
    // w = face_inv * (xi, yi, 1), clamp, renormalise (cu:121-134)
    w0 = d.r3.x * fxi + d.r3.y * fyi + d.r3.z;
    w1 = d.r3.w * fxi + d.r4.x * fyi + d.r4.y;
    w2 = d.r4.z * fxi + d.r4.w * fyi + d.r5.x;
    w0 = fminf(fmaxf(w0, 0.0f), 1.0f);
    w1 = fminf(fmaxf(w1, 0.0f), 1.0f);
    w2 = fminf(fmaxf(w2, 0.0f), 1.0f);
    float wsum = 0.0f;
    wsum += w0; wsum += w1; wsum += w2;
    w0 /= wsum; w1 /= wsum; w2 /= wsum;
    zp = 1.0f / (w0 / d.r5.y + w1 / d.r5.z + w2 / d.r5.w);   // cu:136
    return !(zp <= near_ || far_ <= zp);                      // cu:137-139 (a NaN zp is rejected by neither test: kept, never wins)
}
// The reference's winner rule — ascending faces, strict `<` (cu:142-153) — in its order-free form: smallest zp, equal zp ->
// smallest face index; a NaN zp never wins either way.  (best < 0: nothing yet, best_z = far.)
__device__ __forceinline__ bool beats(float zp, int fn, float best_z, int best) {
    return zp < best_z || (zp == best_z && best >= 0 && fn < best);
}

// ------------------------------------------------------------------------------------------------
// 1c. face-parallel z-resolve for small faces ("splat"): one lane per (view, face) walks the few pixels of the face's
//     trusted bounding box, runs the reference's candidate arithmetic on each and folds the result into a per-pixel
//     64-bit key with ONE atomic:  key = (bits of zp) << 32 | face index,  atomicMin.
//     For zp > 0 the bit pattern of a float orders like the float, so the minimum key is "smallest zp, ties -> smallest
//     face index" — exactly beats().  The path is only taken when near >= 0.
//     Work: faces x box pixels (a pixel-sized face of the bench mesh: ~16-36 tests) instead of tiles x candidates x 256.
//     Every other face goes to the tile lists or the wide list and to the tile kernel (bin_or_list_face); the tile kernel
//     merges both results per pixel.
// ------------------------------------------------------------------------------------------------
constexpr int SPLAT_MAX_PIX = 256;
constexpr unsigned long long KEY_EMPTY = ~0ull;

// Only a zp > 0 has a key.  zp > near >= 0 is what cand_depth's near test leaves — except a NaN, which no reject test
// catches (it never wins in beats() either) and whose bits the key order cannot rank: every path that makes keys filters
// with this first.
__device__ __forceinline__ bool has_key(float zp) { return zp > 0.0f; }
__device__ __forceinline__ unsigned long long make_key(float zp, int fn) {
    return ((unsigned long long)__builtin_bit_cast(unsigned, zp) << 32) | (unsigned)fn;
}
__device__ __forceinline__ float key_depth(unsigned long long key) { return __builtin_bit_cast(float, (unsigned)(key >> 32)); }
__device__ __forceinline__ int key_face(unsigned long long key) { return (int)(unsigned)(key & 0xffffffffull); }

// The pixel walk of one face.  A row is scanned in 32-column pieces: first the cheap inside tests of the piece (a bit per
// pixel), then the depth arithmetic — seven correctly rounded divisions — for the set bits only: a wave then runs it as
// often as its busiest lane has inside pixels, not once per column in which ANY lane is inside.
__device__ __forceinline__ void splat_pixels(const FaceRec r, const PixCenter center, int xa, int xb, int ya, int yb, int ystep, int fn,
                                             unsigned long long* __restrict__ kv, int is, float near_, float far_) {
    for (int yi = ya; yi <= yb; yi += ystep) {
        const float yp = center(yi);
        for (int xc = xa; xc <= xb; xc += 32) {
            const int xe = min(xb, xc + 31);
            unsigned m = 0u;
            for (int xi = xc; xi <= xe; xi++)
                if (cand_inside(r.e, center(xi), yp)) m |= 1u << (xi - xc);
            while (m) {
                const int xi = xc + __builtin_ctz(m);
                m &= m - 1u;
                float zp, w0, w1, w2;
                if (!cand_depth(r.d, (float)xi, (float)yi, near_, far_, zp, w0, w1, w2)) continue;
                if (!has_key(zp)) continue;
                atomicMin(kv + (size_t)yi * is + xi, make_key(zp, fn));
            }
        }
    }
}

// face_setup + the splat in one launch (r04): both are one lane per (view, face) and the splat needs nothing but its own
// face's record, which it takes from the registers of the setup — the same values the setup writes for the tile kernel.
// LPF lanes per face (r06): with a single view in the launch two thirds of the waves hold back faces only and leave at once,
// the others walk ~30 pixels per lane at one wave per SIMD; four lanes per face (each repeats the setup — same instructions,
// lane 0 stores — and walks every fourth box row) spread the live faces over four times the waves: 23.8 -> 15.7 us per 512^2 view.
// Batches that fill the chip anyway keep one lane per face.
template <bool GATHER, int LPF>
__global__ void __launch_bounds__(256)
setup_splat_faces_kernel(const float* __restrict__ faces_in, const float* __restrict__ v_uvz, const int32_t* __restrict__ fidx,
                         float* __restrict__ faces_out, float* __restrict__ faces_inv, FaceBox* __restrict__ boxes,
                         unsigned long long* __restrict__ keys, int* __restrict__ tile_count, int* __restrict__ tile_list,
                         int* __restrict__ wide_count, float* __restrict__ wide_rec, int batch, int nf, int nv, int is,
                         float near_, float far_) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long i = t / LPF;
    const int sub = (int)(t % LPF);     // this lane walks the box rows sub, sub + LPF, ...; lane 0 alone stores, bins and lists
    if (i >= (long)batch * nf) return;
    float f[9], inv[9];
    FaceBox b;
    if (!face_setup<GATHER>(i, faces_in, v_uvz, fidx, faces_out, faces_inv, boxes, nf, nv, is, f, inv, b, sub == 0)) return;
    const int bn = (int)(i / nf), fn = (int)(i % nf);
    if (box_is_empty(b)) return;
    const PixBox p = pix_box(b);
    if (p.exact || p.pixels() > SPLAT_MAX_PIX) {        // not to be walked pixel by pixel
        if (sub == 0) bin_or_list_face({tile_count, tile_list, wide_count, wide_rec}, p, f, bn, fn, nf, is);
        return;
    }
    const FaceRec r = face_rec(f, inv);
    unsigned long long* kv = keys + (size_t)bn * is * is;
    if (is_pow2(is)) splat_pixels(r, PixCenter(is, true), p.xa, p.xb, p.ya + sub, p.yb, LPF, fn, kv, is, near_, far_);
    else splat_pixels(r, PixCenter(is, false), p.xa, p.xb, p.ya + sub, p.yb, LPF, fn, kv, is, near_, far_);
}

// ------------------------------------------------------------------------------------------------
// 2. tile kernel
// ------------------------------------------------------------------------------------------------
struct RasterParams {
    const float* faces;      // [B,nf,9]
    const float* faces_inv;  // [B,nf,9]
    const FaceBox* boxes;    // [B,nf]
    const int* tile_count;   // [B,ntiles]  candidates binned per tile (may exceed BIN_CAP: then the tile rescans)
    const int* tile_list;    // [B,ntiles,BIN_CAP]
    const unsigned long long* keys;   // [B,is,is] winners of the face-parallel path (KEY_EMPTY = none) or NULL
    const int* wide_count;   // [B] faces on the wide list: untrusted or huge boxes, tested by every tile itself
    const float* wide_rec;   // [B,nf,WIDE_REC_FLOATS] what the tiles test of a wide face (bin_or_list_face)
    int nf, is;
    float near_, far_;
    int flip;                // 1: write row (is-1-yi)
    // drop-in outputs (MODE 0)
    int32_t* face_index_map;
    float* weight_map;
    float* depth_map;
    float* face_inv_map;     // may be NULL
    // fused outputs (MODE 1)
    rnr_mesh mesh;
    rnr_gbuffer gb;
    const float* pose;       // [B,4,4] or NULL
};

// Wave-ballot compaction into an LDS queue: the lanes of a wave whose pred holds take consecutive slots from *counter, one
// LDS atomic per wave.  Returns the lane's slot (meaningless where pred is false).
__device__ __forceinline__ int queue_slot(bool pred, int* counter, int lane) {
    const unsigned long long bal = __ballot(pred);
    if (!bal) return 0;                                 // wave-uniform: most calls add nothing
    int base = 0;
    if (lane == 0) base = atomicAdd(counter, __popcll(bal));
    base = __shfl(base, 0, 64);
    return base + __popcll(bal & ((1ull << lane) - 1ull));
}

// Epilogue, drop-in mode: the extension's maps.  Uncovered pixels keep the caller's pre-fill (cu:156-168).
__device__ __forceinline__ void write_dropin_maps(const RasterParams& P, const float* faces_inv, size_t pix, int best, float best_z,
                                                  float bw0, float bw1, float bw2) {
    if (best < 0) return;
    P.depth_map[pix] = best_z;
    P.face_index_map[pix] = best;
    P.weight_map[3 * pix + 0] = bw0;
    P.weight_map[3 * pix + 1] = bw1;
    P.weight_map[3 * pix + 2] = bw2;
    if (P.face_inv_map) {
        const float* fi = faces_inv + (size_t)best * 9;
#pragma unroll
        for (int k = 0; k < 9; k++) P.face_inv_map[9 * pix + k] = fi[k];
    }
}

// out = the rows idx[0..2] of attr [.,N], blended with the perspective-corrected weights
template <int N>
__device__ __forceinline__ void blend_rows(const float* attr, const int32_t* idx, float wp0, float wp1, float wp2, float (&out)[N]) {
    const float* a = attr + (size_t)idx[0] * N;
    const float* b = attr + (size_t)idx[1] * N;
    const float* c = attr + (size_t)idx[2] * N;
#pragma unroll
    for (int k = 0; k < N; k++) out[k] = a[k] * wp0 + b[k] * wp1 + c[k] * wp2;
}

// Epilogue, fused mode: network.Rasterizer.forward's attribute interpolation (network.py:176-214)
__device__ __forceinline__ void write_gbuffer(const RasterParams& P, const float* faces, int bn, size_t pix, int best, float best_z,
                                              float bw0, float bw1, float bw2) {
    const rnr_gbuffer& G = P.gb;
    const int fa = best >= 0 ? best : P.nf - 1;  // torch indexing wraps -1 to the last face (weights are 0 there)
    const float* f = faces + (size_t)fa * 9;
    const float depth = best_z;                 // far on background (rasterize.py:52)
    const float wp0 = ((1.0f / f[2]) * bw0) * depth;
    const float wp1 = ((1.0f / f[5]) * bw1) * depth;
    const float wp2 = ((1.0f / f[8]) * bw2) * depth;
    if (G.face_index_map) G.face_index_map[pix] = best;
    if (G.alpha) G.alpha[pix] = best >= 0 ? 1.0f : 0.0f;
    if (G.depth) G.depth[pix] = depth;
    if (G.raw_weight_map) {
        G.raw_weight_map[3 * pix + 0] = bw0; G.raw_weight_map[3 * pix + 1] = bw1; G.raw_weight_map[3 * pix + 2] = bw2;
    }
    if (G.weight_map) {
        G.weight_map[3 * pix + 0] = wp0; G.weight_map[3 * pix + 1] = wp1; G.weight_map[3 * pix + 2] = wp2;
    }
    if (G.uv_map) {
        float uv[2];
        blend_rows<2>(P.mesh.vt, P.mesh.f_vt_idx + (size_t)fa * 3, wp0, wp1, wp2, uv);
        G.uv_map[2 * pix + 0] = uv[0] - floorf(uv[0]);
        G.uv_map[2 * pix + 1] = uv[1] - floorf(uv[1]);
    }
    float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, T[3] = {0, 0, 0};
    if (P.pose) {
        const float* ps = P.pose + (size_t)bn * 16;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            R[3 * r + 0] = ps[4 * r + 0]; R[3 * r + 1] = ps[4 * r + 1]; R[3 * r + 2] = ps[4 * r + 2];
            T[r] = ps[4 * r + 3];
        }
    }
    if (G.normal_map || G.normal_map_cam) {
        float n[3];
        blend_rows<3>(P.mesh.vn, P.mesh.f_vn_idx + (size_t)fa * 3, wp0, wp1, wp2, n);
        float n0 = n[0], n1 = n[1], n2 = n[2];
        float inv = 1.0f / fmaxf(sqrtf(n0 * n0 + n1 * n1 + n2 * n2), 1e-12f);  // F.normalize
        n0 *= inv; n1 *= inv; n2 *= inv;
        if (G.normal_map) {
            G.normal_map[3 * pix + 0] = n0; G.normal_map[3 * pix + 1] = n1; G.normal_map[3 * pix + 2] = n2;
        }
        if (G.normal_map_cam) {
            float c0 = R[0] * n0 + R[1] * n1 + R[2] * n2;
            float c1 = R[3] * n0 + R[4] * n1 + R[5] * n2;
            float c2 = R[6] * n0 + R[7] * n1 + R[8] * n2;
            float ic = 1.0f / fmaxf(sqrtf(c0 * c0 + c1 * c1 + c2 * c2), 1e-12f);
            G.normal_map_cam[3 * pix + 0] = c0 * ic;
            G.normal_map_cam[3 * pix + 1] = c1 * ic;
            G.normal_map_cam[3 * pix + 2] = c2 * ic;
        }
    }
    if (G.position_map || G.position_map_cam) {
        float p[3];
        blend_rows<3>(P.mesh.v, P.mesh.f_v_idx + (size_t)fa * 3, wp0, wp1, wp2, p);
        const float p0 = p[0], p1 = p[1], p2 = p[2];
        if (G.position_map) {
            G.position_map[3 * pix + 0] = p0; G.position_map[3 * pix + 1] = p1; G.position_map[3 * pix + 2] = p2;
        }
        if (G.position_map_cam) {
            G.position_map_cam[3 * pix + 0] = R[0] * p0 + R[1] * p1 + R[2] * p2 + T[0];
            G.position_map_cam[3 * pix + 1] = R[3] * p0 + R[4] * p1 + R[5] * p2 + T[1];
            G.position_map_cam[3 * pix + 2] = R[6] * p0 + R[7] * p1 + R[8] * p2 + T[2];
        }
    }
}

template <int MODE>
__global__ void __launch_bounds__(RTHREADS)
raster_tile_kernel(const RasterParams P) {
    __shared__ int s_queue[QCAP];
    __shared__ __attribute__((aligned(16))) float s_stage[STAGE * STAGE_FLOATS];
    __shared__ int s_qn;
    __shared__ int s_dn;                                // zero-area wide faces queued from the END of s_queue (walk_lines)
    __shared__ unsigned long long s_key[RTHREADS];      // their per-pixel winners: the same (depth bits, face) key as P.keys

    const int is = P.is, nf = P.nf;
    const int tiles_x = (is + TILE - 1) / TILE;
    const int tile = blockIdx.x;
    const int bn = blockIdx.y;
    const int tx0 = (tile % tiles_x) * TILE, ty0 = (tile / tiles_x) * TILE;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int xi = tx0 + (tid & (TILE - 1)), yi = ty0 + (tid >> 4);
    const bool in_img = (xi < is) && (yi < is);
    const int tx1 = min(tx0 + TILE - 1, is - 1), ty1 = min(ty0 + TILE - 1, is - 1);
    const float xp = pix_center(xi, is), yp = pix_center(yi, is);
    const float fxi = (float)xi, fyi = (float)yi;
    const TileBounds tb = tile_bounds(tile % tiles_x, tile / tiles_x, is);

    const float* faces = P.faces + (size_t)bn * nf * 9;
    const float* faces_inv = P.faces_inv + (size_t)bn * nf * 9;
    const FaceBox* boxes = P.boxes + (size_t)bn * nf;

    float best_z = P.far_;
    int best = -1;
    float bw0 = 0.f, bw1 = 0.f, bw2 = 0.f;

    // the face-parallel path's winner of this pixel, requested up front: independent of everything the lists below need
    unsigned long long key = KEY_EMPTY;
    if (P.keys && in_img) key = P.keys[((size_t)bn * is + yi) * is + xi];

    if (tid == 0) { s_qn = 0; s_dn = 0; }
    s_key[tid] = KEY_EMPTY;
    __syncthreads();

    // Evaluate the queued candidates.  The queue is NOT in face order (waves append independently): beats() is order-free.
    auto process_queue = [&](const int* ids, int qn) {
        FaceRec* stage = reinterpret_cast<FaceRec*>(s_stage);
        for (int s0 = 0; s0 < qn; s0 += STAGE) {
            const int n = min(STAGE, qn - s0);
            if (tid < n) {
                const int fn = ids[s0 + tid];
                stage[tid] = face_rec(faces + (size_t)fn * 9, faces_inv + (size_t)fn * 9);
            }
            __syncthreads();
            if (in_img) {
                for (int c = 0; c < n; c++) {
                    if (!cand_inside(stage[c].e, xp, yp)) continue;
                    float zp, w0, w1, w2;
                    if (!cand_depth(stage[c].d, fxi, fyi, P.near_, P.far_, zp, w0, w1, w2)) continue;
                    const int fn = ids[s0 + c];
                    if (beats(zp, fn, best_z, best)) {
                        best_z = zp;
                        best = fn;
                        bw0 = w0; bw1 = w1; bw2 = w2;
                    }
                }
            }
            __syncthreads();
        }
    };

    // fast path: the candidate list built by the binning kernels; a list that overflowed is ignored and the
    // tile scans every box itself (slow, same result)
    const int ntiles_all = tiles_x * tiles_x;
    const int binned = P.tile_count ? P.tile_count[(size_t)bn * ntiles_all + tile] : BIN_CAP + 1;
    const int nsteps = binned <= BIN_CAP ? 0 : (nf + SCAN_CHUNK - 1) / SCAN_CHUNK;
    if (binned <= BIN_CAP) process_queue(P.tile_list + ((size_t)bn * ntiles_all + tile) * BIN_CAP, binned);
    // the wide list (untrusted boxes, faces over more than WIDE_TILES tiles): every tile tests it against itself — usually
    // empty, and then this costs one scalar load where bin_wide_kernel cost a launch (r04).  A tile that rescans every face
    // anyway (overflowed list) meets the wide faces there.
    // Zero-area wide faces (two coincident vertices: the pole faces of a UV sphere, 520 of the 65 536-face bench mesh).  Their
    // pass region is a line: with the distinct vertices a, b the reference's three edge tests reduce to  P1 >= Q1  and
    // P2 <= Q2, rounded evaluations of the same edge function E(p) = (yp - ya) dx - (xp - xa) dy  (dx = fl(xb - xa), dy alike;
    // the opposite edge has exactly the negated differences), so a pixel can only pass with |E(p)| <= 2.01 u (|yp - ya| |dx| +
    // |xp - xa| |dy|) + 2 u |dx dy|.  With every coordinate in [-4, 4] that puts the pixel centre within 36 u = 2.2e-6 NDC of
    // the line along the axis the line is steeper in — 0.018 pixels at the largest image the library accepts (16384).  So of
    // each pixel row (column, for a shallow line) of the tile only the two pixels next to the crossing can pass; they get the
    // reference's candidate arithmetic (cand_inside / cand_depth: the same bits as everywhere else), 32 tests per (tile, face)
    // instead of 256, sixteen faces at a time, and the result is folded into a per-pixel key like the splat path's.  A tile at
    // a pole of the sphere holds ~260 such candidates: 36 us as ordinary queue entries at one view per call, r06.
    // Faces outside the conditions (three coincident vertices, |coordinate| > 4, |b - a| < 1e-6, near < 0) stay ordinary.
    // what the walk needs of a zero-area face, 12 floats: (x0, y0, x1, y1) (x2, y2, face, steep) and, as doubles, (c0, c1): the
    // crossing of row / column i with the line, in pixel coordinates, is c0 + c1 * pix_center(i)
    constexpr int LINE_FLOATS = 12;
    static_assert(RTHREADS * LINE_FLOATS <= STAGE * STAGE_FLOATS, "a batch of line records fits the staging array");
    auto stage_line = [&](int slot, const float4 ra, const float4 rb) {
        const float x0 = ra.x, y0 = ra.y, x1 = ra.z, y1 = ra.w, x2 = rb.x, y2 = rb.y;
        // the two distinct points: v0 and v1, or v0 and v2 when v0 == v1
        const bool e01 = x0 == x1 && y0 == y1;
        const float xa = x0, ya = y0, xb = e01 ? x2 : x1, yb = e01 ? y2 : y1;
        const float dx = xb - xa, dy = yb - ya;
        const bool steep = fabsf(dy) >= fabsf(dx);
        // steep: x(yp) = xa + (yp - ya) dx / dy, else y(xp) = ya + (xp - xa) dy / dx; NDC t -> pixel coordinate (t * is + is - 1) / 2
        const double sl = steep ? (double)dx / (double)dy : (double)dy / (double)dx;
        const double t0 = steep ? (double)xa - (double)ya * sl : (double)ya - (double)xa * sl;
        const double c0 = (t0 * is + is - 1) * 0.5, c1 = sl * is * 0.5;
        float4* dst = reinterpret_cast<float4*>(s_stage + slot * LINE_FLOATS);
        dst[0] = ra;
        dst[1] = make_float4(x2, y2, rb.z, steep ? 1.0f : 0.0f);
        reinterpret_cast<double2*>(dst)[2] = make_double2(c0, c1);
    };
    const PixCenter center(is, is_pow2(is));
    // The first RTHREADS records were staged by the lanes that queued them (registers -> LDS, no second fetch); later batches
    // are fetched again by their slot number.
    auto walk_lines = [&](int dn) {
        for (int d0 = 0; d0 < dn; d0 += RTHREADS) {
            const int n = min(RTHREADS, dn - d0);
            if (d0 > 0) {
                if (tid < n) {
                    const int w = s_queue[QCAP - 1 - (d0 + tid)];
                    const float4* r = reinterpret_cast<const float4*>(P.wide_rec + ((size_t)bn * nf + w) * WIDE_REC_FLOATS);
                    stage_line(tid, r[0], r[1]);
                }
                __syncthreads();
            }
            const int sub = tid & 15;
            for (int c = tid >> 4; c < n; c += RTHREADS / 16) {
                const float4* rec = reinterpret_cast<const float4*>(s_stage + c * LINE_FLOATS);
                const float4 ra = rec[0], rb = rec[1];
                const double2 cc = reinterpret_cast<const double2*>(rec)[2];
                const int fn = __builtin_bit_cast(int, rb.z);
                const bool steep = rb.w != 0.0f;
                // the crossing of this lane's row (steep) or column with the line, in pixel coordinates
                const int fixed = (steep ? ty0 : tx0) + sub;
                const float cf = center(fixed);
                const double tp = cc.x + cc.y * (double)cf;
                if (!(tp > -2.0 && tp < (double)is + 1.0)) continue;
                const int lo = (int)floor(tp);
                const FaceEdges e = face_edges(ra.x, ra.y, ra.z, ra.w, rb.x, rb.y);
#pragma unroll
                for (int side = 0; side < 2; side++) {
                    const int pxi = steep ? lo + side : fixed, pyi = steep ? fixed : lo + side;
                    if (pxi < tx0 || pxi > tx1 || pyi < ty0 || pyi > ty1) continue;
                    if (!cand_inside(e, steep ? center(pxi) : cf, steep ? cf : center(pyi))) continue;
                    float zp, w0, w1, w2;
                    if (!cand_depth(face_depth(faces + (size_t)fn * 9, faces_inv + (size_t)fn * 9), (float)pxi, (float)pyi, P.near_,
                                    P.far_, zp, w0, w1, w2))
                        continue;
                    if (!has_key(zp)) continue;         // (near >= 0 here)
                    atomicMin(&s_key[(pyi - ty0) * TILE + (pxi - tx0)], make_key(zp, fn));
                }
            }
            __syncthreads();
        }
    };
    if (P.wide_count && binned <= BIN_CAP) {
        const int wn = P.wide_count[bn];
        const float4* wr = reinterpret_cast<const float4*>(P.wide_rec + (size_t)bn * nf * WIDE_REC_FLOATS);
        // WIDE_ITEMS records per lane and round, all of a round's loads in flight together: one round trip and one barrier
        // pair per 1024 wide faces
        constexpr int WIDE_ITEMS = 4;
        for (int w0 = 0; w0 < wn; w0 += RTHREADS * WIDE_ITEMS) {
            float4 ra[WIDE_ITEMS], rb[WIDE_ITEMS];
#pragma unroll
            for (int j = 0; j < WIDE_ITEMS; j++) {
                const int w = w0 + j * RTHREADS + tid;
                if (w < wn) { ra[j] = wr[2 * w]; rb[j] = wr[2 * w + 1]; }
            }
#pragma unroll
            for (int j = 0; j < WIDE_ITEMS; j++) {
                const int w = w0 + j * RTHREADS + tid;
                if (w0 + j * RTHREADS >= wn) break;                     // block-uniform
                const float x0 = ra[j].x, y0 = ra[j].y, x1 = ra[j].z, y1 = ra[j].w, x2 = rb[j].x, y2 = rb[j].y;
                const bool k = w < wn && may_touch_tile(x0, y0, x1, y1, x2, y2, tb);
                bool line = false;
                if (k && P.keys) {      // (P.keys: near >= 0)
                    const int ne = (x0 == x1 && y0 == y1 ? 1 : 0) + (x1 == x2 && y1 == y2 ? 1 : 0) + (x2 == x0 && y2 == y0 ? 1 : 0);
                    const float amax = fmaxf(fmaxf(fmaxf(fabsf(x0), fabsf(y0)), fmaxf(fabsf(x1), fabsf(y1))), fmaxf(fabsf(x2), fabsf(y2)));
                    const float ex = (x0 == x1 && y0 == y1) ? x2 - x0 : x1 - x0, ey = (x0 == x1 && y0 == y1) ? y2 - y0 : y1 - y0;
                    line = ne == 1 && amax <= 4.0f && fmaxf(fabsf(ex), fabsf(ey)) >= 1e-6f;
                }
                const int qs = queue_slot(k && !line, &s_qn, lane);
                if (k && !line) s_queue[qs] = __builtin_bit_cast(int, rb[j].z);
                const int slot = queue_slot(line, &s_dn, lane);
                if (line) {             // the record's slot number, from the end of the queue
                    s_queue[QCAP - 1 - slot] = w;
                    if (slot < RTHREADS) stage_line(slot, ra[j], rb[j]);
                }
            }
            __syncthreads();
            const int qn = s_qn, dn = s_dn;
            __syncthreads();        // every wave has read the counts before any wave's next append: the flush decision IS block-uniform
            if (qn + dn > QCAP - RTHREADS * WIDE_ITEMS || w0 + RTHREADS * WIDE_ITEMS >= wn) {
                walk_lines(dn);                                    // first: it reads the staging array this round filled; ends with a barrier
                process_queue(s_queue, qn);                        // ends with a barrier
                if (tid == 0) { s_qn = 0; s_dn = 0; }
                __syncthreads();
            }
        }
    }
    FaceBox bx[SCAN_ITEMS];
    auto fetch_boxes = [&](int step) {
#pragma unroll
        for (int j = 0; j < SCAN_ITEMS; j++) {
            const int fn = step * SCAN_CHUNK + j * RTHREADS + tid;
            FaceBox b = empty_box();
            if (fn < nf) b = boxes[fn];
            bx[j] = b;
        }
    };
    if (nsteps > 0) fetch_boxes(0);
    for (int step = 0; step < nsteps; step++) {
        FaceBox cur[SCAN_ITEMS];
#pragma unroll
        for (int j = 0; j < SCAN_ITEMS; j++) cur[j] = bx[j];
        if (step + 1 < nsteps) fetch_boxes(step + 1);          // next step's boxes are in flight during this step
#pragma unroll
        for (int j = 0; j < SCAN_ITEMS; j++) {
            const int fn = step * SCAN_CHUNK + j * RTHREADS + tid;
            const FaceBox b = cur[j];
            bool k = false;
            const bool exact_only = (b.xlo == BOX_EXACT);
            if (fn < nf && (exact_only || (b.xlo <= tx1 && b.xhi >= tx0 && b.ylo <= ty1 && b.yhi >= ty0))) {
                const float* f = faces + (size_t)fn * 9;
                k = may_touch_tile(f[0], f[1], f[3], f[4], f[6], f[7], tb);
            }
            const int qs = queue_slot(k, &s_qn, lane);
            if (k) s_queue[qs] = fn;
        }
        if ((step % FLUSH_EVERY) == FLUSH_EVERY - 1 || step == nsteps - 1) {
            __syncthreads();
            const int qn = s_qn;
            __syncthreads();        // as above: no wave appends (next step) before all have read the count
            if (qn > 2 * SCAN_CHUNK || step == nsteps - 1) {
                process_queue(s_queue, qn);                    // ends with a barrier
                if (tid == 0) s_qn = 0;
                __syncthreads();
            }
        }
    }

    if (!in_img) return;
    // winner of the face-parallel paths for this pixel (walk_lines ended with a barrier); the key order is beats()
    key = min(key, s_key[tid]);
    if (key != KEY_EMPTY && beats(key_depth(key), key_face(key), best_z, best)) {
        // recompute this face's weights at this pixel: the same arithmetic on the same inputs, hence the same bits
        best = key_face(key);
        cand_depth(face_depth(faces + (size_t)best * 9, faces_inv + (size_t)best * 9), fxi, fyi, P.near_, P.far_, best_z, bw0, bw1, bw2);
    }
    const int yo = P.flip ? (is - 1 - yi) : yi;
    const size_t pix = ((size_t)bn * is + yo) * is + xi;
    if (MODE == 0) write_dropin_maps(P, faces_inv, pix, best, best_z, bw0, bw1, bw2);
    else write_gbuffer(P, faces, bn, pix, best, best_z, bw0, bw1, bw2);
}

// ------------------------------------------------------------------------------------------------
// per-face texture cube sampling (API completeness; the hot path passes an all-zero texture)
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
texture_sampling_kernel(const float* __restrict__ faces, const float* __restrict__ textures,
                        const int32_t* __restrict__ face_index_map, const float* __restrict__ weight_map,
                        const float* __restrict__ depth_map, float* __restrict__ rgb_map,
                        int32_t* __restrict__ sampling_index_map, float* __restrict__ sampling_weight_map,
                        long npix, int nf, int is, int ts, float eps) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const int fidx = face_index_map[i];
    if (fidx < 0) return;
    const int bn = (int)(i / ((long)is * is));
    const float* f = faces + ((size_t)bn * nf + fidx) * 9;
    const float* tex = textures + ((size_t)bn * nf + fidx) * ts * ts * ts * 3;
    const float depth = depth_map[i];
    float t[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {  // cu:208-213
        float v = weight_map[3 * i + k] * (float)(ts - 1) * (depth / f[3 * k + 2]);
        v = fmaxf(v, 0.0f);
        v = fminf(v, (float)(ts - 1) - eps);
        t[k] = v;
    }
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f;
#pragma unroll
    for (int corner = 0; corner < 8; corner++) {  // cu:217-236
        float w = 1.0f;
        int ti[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int b = (int)t[k];
            const float frac = t[k] - (float)b;
            if (((corner >> k) & 1) == 0) { w *= 1.0f - frac; ti[k] = b; }
            else                          { w *= frac;        ti[k] = b + 1; }
        }
        const int isc = ti[0] * ts * ts + ti[1] * ts + ti[2];
        acc0 += w * tex[isc * 3 + 0];
        acc1 += w * tex[isc * 3 + 1];
        acc2 += w * tex[isc * 3 + 2];
        sampling_index_map[8 * i + corner] = isc;
        sampling_weight_map[8 * i + corner] = w;
    }
    rgb_map[3 * i + 0] = acc0; rgb_map[3 * i + 1] = acc1; rgb_map[3 * i + 2] = acc2;
}

// ------------------------------------------------------------------------------------------------
// workspace
// ------------------------------------------------------------------------------------------------
static int num_tiles(int is) { const int t = (is + TILE - 1) / TILE; return t * t; }

// The layout of a rasterizer workspace, stated once:
//   boxes | faces | faces_inv (the fused entry point only: the drop-in one has the caller's arrays) |
//   tile_count, wide_count | tile_list | keys | wide_rec
// Every region is 256-byte aligned and padded, so the two that are cleared before every call — the counters to 0, the keys
// to ~0 — are whole uint4 vectors.  ws == NULL: sizes only.
struct RasterWorkspace {
    FaceBox* boxes;             // [B,nf]
    float* faces;               // [B,nf,9]
    float* faces_inv;           // [B,nf,9]
    int* tile_count;            // [B,ntiles], followed by
    int* wide_count;            // [B]
    int* tile_list;             // [B,ntiles,BIN_CAP]
    unsigned long long* keys;   // [B,is,is]
    float* wide_rec;            // [B,nf,WIDE_REC_FLOATS]
    long counter_vec, key_vec;  // uint4 vectors from tile_count / keys to the end of their region

    RasterWorkspace(void* ws, int batch, int nf, int is, bool with_face_arrays) {
        const size_t faces_n = with_face_arrays ? (size_t)batch * nf * 9 : 0;
        boxes = take<FaceBox>(ws, (size_t)batch * nf);
        faces = take<float>(ws, faces_n);
        faces_inv = take<float>(ws, faces_n);
        tile_count = take<int>(ws, (size_t)batch * (num_tiles(is) + 1));
        wide_count = tile_count + (size_t)batch * num_tiles(is);
        counter_vec = vectors_to_end(tile_count, ws);
        tile_list = take<int>(ws, (size_t)batch * num_tiles(is) * BIN_CAP);
        keys = take<unsigned long long>(ws, (size_t)batch * is * is);
        key_vec = vectors_to_end(keys, ws);
        wide_rec = take<float>(ws, (size_t)batch * nf * WIDE_REC_FLOATS);
    }
    size_t bytes() const { return end; }
    uint4* counter_region() const { return reinterpret_cast<uint4*>(tile_count); }
    uint4* key_region() const { return reinterpret_cast<uint4*>(keys); }

private:
    size_t end = 0;
    template <typename T> T* take(void* ws, size_t n) {
        T* p = reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(ws) + end);
        end += align_up(n * sizeof(T), 256);
        return p;
    }
    template <typename T> long vectors_to_end(const T* region, void* ws) const {
        return (long)((reinterpret_cast<uintptr_t>(ws) + end - reinterpret_cast<uintptr_t>(region)) / sizeof(uint4));
    }
};

// Clears the bin counters (zeros) and the per-pixel depth keys (all ones) in one launch.  Not hipMemsetAsync: memset
// nodes of a captured HIP graph went stale on replay once any other copy / fill had run in between (GPU write fault,
// scripts/exp_graph2.py raster), kernels replay correctly.
__global__ void __launch_bounds__(256)
raster_clear_kernel(uint4* __restrict__ counters, long counter_vec, uint4* __restrict__ keys, long key_vec) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < counter_vec) counters[i] = make_uint4(0u, 0u, 0u, 0u);
    else if (i - counter_vec < key_vec) keys[i - counter_vec] = make_uint4(~0u, ~0u, ~0u, ~0u);
}

// Everything in front of the tile kernel: runs the per-face setup S and fills W's lists and keys (P's pointers to them).
// near >= 0: small trusted faces are resolved face-parallel into the keys by the setup's own launch, the others binned by it;
// near < 0: the setup, then bin_faces_kernel for every face.  precleared: the caller has cleared W's two regions already.
static int run_binning(const RasterWorkspace& W, const FaceSetupArgs& S, int batch, int nf, int is, RasterParams* P,
                       hipStream_t st, bool precleared) {
    const long total = (long)batch * nf;
    const bool gather = S.v_uvz != nullptr;
    const bool splat = P->near_ >= 0.0f;            // the key order needs zp > 0, which the near test then guarantees (has_key)
    if (!precleared) {
        const long kvec = splat ? W.key_vec : 0;
        hipLaunchKernelGGL(raster_clear_kernel, dim3((unsigned)((W.counter_vec + kvec + 255) / 256)), dim3(256), 0, st,
                           W.counter_region(), W.counter_vec, W.key_region(), kvec);
        if (int e = check_launch("raster_clear_kernel")) return e;
    }
    const dim3 fgrid((unsigned)((total + 255) / 256));
    if (!splat) {
        auto setup = [&](auto kernel) { hipLaunchKernelGGL(kernel, fgrid, dim3(256), 0, st, S.faces_in, S.v_uvz, S.fidx, S.faces_out, S.faces_inv, S.boxes, batch, nf, S.nv, is);
        };
        if (gather) setup(face_setup_kernel<true>); else setup(face_setup_kernel<false>);
        if (int e = check_launch("face_setup_kernel")) return e;
        hipLaunchKernelGGL(bin_faces_kernel, fgrid, dim3(256), 0, st, P->faces, W.boxes, W.tile_count, W.tile_list, W.wide_count, W.wide_rec,
                           batch, nf, is);
        if (int e = check_launch("bin_faces_kernel")) return e;
    } else {
        // lanes per face: four while the launch would otherwise leave most SIMDs with one wave or none (RNR_SPLAT_LPF overrides)
        static const int forced = [] { const char* e = getenv("RNR_SPLAT_LPF"); return e ? atoi(e) : 0; }();
        const int lpf = forced == 1 || forced == 4 ? forced : (total <= 2 * 65536 ? 4 : 1);
        const dim3 sgrid((unsigned)((total * lpf + 255) / 256));
        auto setup_splat = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, sgrid, dim3(256), 0, st, S.faces_in, S.v_uvz, S.fidx, S.faces_out, S.faces_inv, S.boxes, W.keys,
                               W.tile_count, W.tile_list, W.wide_count, W.wide_rec, batch, nf, S.nv, is, P->near_, P->far_);
        };
        if (gather) { if (lpf == 4) setup_splat(setup_splat_faces_kernel<true, 4>); else setup_splat(setup_splat_faces_kernel<true, 1>); }
        else { if (lpf == 4) setup_splat(setup_splat_faces_kernel<false, 4>); else setup_splat(setup_splat_faces_kernel<false, 1>); }
        if (int e = check_launch("setup_splat_faces_kernel")) return e;
        P->keys = W.keys;
    }
    P->boxes = W.boxes;
    P->wide_count = W.wide_count;    // tested by the tile kernel (bin_wide_kernel's work, without its launch)
    P->wide_rec = W.wide_rec;
    P->tile_count = W.tile_count;
    P->tile_list = W.tile_list;
    return 0;
}

}  // namespace rnr

using namespace rnr;

extern "C" size_t rnr_raster_workspace_bytes(int batch_size, int num_faces, int image_size) {
    return RasterWorkspace(nullptr, batch_size, num_faces, image_size, false).bytes();
}

extern "C" int rnr_forward_face_index_map(const float* faces, int32_t* face_index_map, float* weight_map,
                                          float* depth_map, float* face_inv_map, float* faces_inv,
                                          int batch_size, int num_faces, int image_size, float near_,
                                          float far_, int return_rgb, int return_alpha, int return_depth,
                                          void* workspace, void* stream) {
    (void)return_rgb; (void)return_alpha;
    RNR_REQUIRE(faces && face_index_map && weight_map && depth_map && faces_inv && workspace,
                "rnr_forward_face_index_map: null pointer argument");
    RNR_REQUIRE(batch_size > 0 && num_faces > 0 && image_size > 0 && image_size <= 16384,
                "rnr_forward_face_index_map: bad sizes B=%d nf=%d is=%d", batch_size, num_faces, image_size);
    RNR_REQUIRE(!return_depth || face_inv_map, "rnr_forward_face_index_map: return_depth needs face_inv_map");
    hipStream_t st = as_stream(stream);
    const RasterWorkspace W(workspace, batch_size, num_faces, image_size, false);
    const FaceSetupArgs setup = {faces, nullptr, nullptr, 0, nullptr, faces_inv, W.boxes};
    RasterParams P = {};
    P.faces = faces; P.faces_inv = faces_inv; P.nf = num_faces; P.is = image_size;
    P.near_ = near_; P.far_ = far_; P.flip = 0;
    P.face_index_map = face_index_map; P.weight_map = weight_map; P.depth_map = depth_map;
    P.face_inv_map = return_depth ? face_inv_map : nullptr;
    if (int e = run_binning(W, setup, batch_size, num_faces, image_size, &P, st, false)) return e;
    const int tiles = (image_size + TILE - 1) / TILE;
    hipLaunchKernelGGL(raster_tile_kernel<0>, dim3(tiles * tiles, batch_size), dim3(RTHREADS), 0, st, P);
    return check_launch("raster_tile_kernel<0>");
}

extern "C" int rnr_forward_texture_sampling(const float* faces, const float* textures,
                                            const int32_t* face_index_map, const float* weight_map,
                                            const float* depth_map, float* rgb_map,
                                            int32_t* sampling_index_map, float* sampling_weight_map,
                                            int batch_size, int num_faces, int image_size, int texture_size,
                                            float eps, void* stream) {
    RNR_REQUIRE(faces && textures && face_index_map && weight_map && depth_map && rgb_map &&
                    sampling_index_map && sampling_weight_map,
                "rnr_forward_texture_sampling: null pointer argument");
    RNR_REQUIRE(batch_size > 0 && num_faces > 0 && image_size > 0 && texture_size > 1,
                "rnr_forward_texture_sampling: bad sizes");
    const long npix = (long)batch_size * image_size * image_size;
    hipLaunchKernelGGL(texture_sampling_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0,
                       as_stream(stream), faces, textures, face_index_map, weight_map, depth_map, rgb_map,
                       sampling_index_map, sampling_weight_map, npix, num_faces, image_size, texture_size, eps);
    return check_launch("texture_sampling_kernel");
}

extern "C" size_t rnr_gbuffer_workspace_bytes(int num_views, int num_faces, int image_size) {
    return RasterWorkspace(nullptr, num_views, num_faces, image_size, true).bytes();
}

// the two regions of an rnr_rasterize_gbuffer workspace that must be cleared before every call (tile / wide-list counters to
// 0, depth keys to ~0), as whole uint4 vectors: for rnr_frame_prepare (shade.hip), which clears them in its own launch
void rnr::gbuffer_clear_regions(void* workspace, int num_views, int num_faces, int image_size, uint4** counters, long* counter_vec,
                                uint4** keys, long* key_vec) {
    const RasterWorkspace W(workspace, num_views, num_faces, image_size, true);
    *counters = W.counter_region();
    *counter_vec = W.counter_vec;
    *keys = W.key_region();
    *key_vec = W.key_vec;
}

static int rasterize_gbuffer_impl(const rnr_mesh* mesh, const float* v_uvz, const float* pose, int num_views, int image_size,
                                  float near_, float far_, const rnr_gbuffer* out, void* workspace, void* stream, bool precleared) {
    RNR_REQUIRE(mesh && v_uvz && out && workspace, "rnr_rasterize_gbuffer: null pointer argument");
    RNR_REQUIRE(mesh->v && mesh->f_v_idx && mesh->num_faces > 0 && mesh->num_vertices > 0,
                "rnr_rasterize_gbuffer: incomplete mesh");
    RNR_REQUIRE(!(out->uv_map) || (mesh->vt && mesh->f_vt_idx), "rnr_rasterize_gbuffer: uv_map needs vt");
    RNR_REQUIRE(!(out->normal_map || out->normal_map_cam) || (mesh->vn && mesh->f_vn_idx),
                "rnr_rasterize_gbuffer: normal maps need vn");
    RNR_REQUIRE(!(out->normal_map_cam || out->position_map_cam) || pose,
                "rnr_rasterize_gbuffer: camera-space maps need pose");
    RNR_REQUIRE(num_views > 0 && image_size > 0 && image_size <= 16384, "rnr_rasterize_gbuffer: bad sizes");
    // the clear and the wide-face records move uint4 / float4, the keys are 64-bit: every region starts a multiple of 256 bytes in
    RNR_REQUIRE(aligned_to(16, {workspace}), "rnr_rasterize_gbuffer: workspace must be 16-byte aligned");
    RNR_REQUIRE(aligned_to(4, {mesh->v, mesh->vt, mesh->vn, mesh->f_v_idx, mesh->f_vt_idx, mesh->f_vn_idx, v_uvz, pose}),
                "rnr_rasterize_gbuffer: the mesh arrays, v_uvz and pose must be 4-byte aligned");
    RNR_REQUIRE(aligned_to(4, {out->face_index_map, out->alpha, out->depth, out->weight_map, out->raw_weight_map, out->uv_map,
                               out->normal_map, out->normal_map_cam, out->position_map, out->position_map_cam}),
                "rnr_rasterize_gbuffer: every map of out must be 4-byte aligned");
    hipStream_t st = as_stream(stream);
    const int nf = mesh->num_faces;
    const RasterWorkspace W(workspace, num_views, nf, image_size, true);
    const FaceSetupArgs setup = {nullptr, v_uvz, mesh->f_v_idx, mesh->num_vertices, W.faces, W.faces_inv, W.boxes};
    RasterParams P = {};
    P.faces = W.faces; P.faces_inv = W.faces_inv; P.nf = nf; P.is = image_size;
    P.near_ = near_; P.far_ = far_; P.flip = 1;
    P.mesh = *mesh; P.gb = *out; P.pose = pose;
    if (int e = run_binning(W, setup, num_views, nf, image_size, &P, st, precleared)) return e;
    const int tiles = (image_size + TILE - 1) / TILE;
    hipLaunchKernelGGL(raster_tile_kernel<1>, dim3(tiles * tiles, num_views), dim3(RTHREADS), 0, st, P);
    return check_launch("raster_tile_kernel<1>");
}

extern "C" int rnr_rasterize_gbuffer(const rnr_mesh* mesh, const float* v_uvz, const float* pose,
                                     int num_views, int image_size, float near_, float far_,
                                     const rnr_gbuffer* out, void* workspace, void* stream) {
    return rasterize_gbuffer_impl(mesh, v_uvz, pose, num_views, image_size, near_, far_, out, workspace, stream, false);
}

extern "C" int rnr_rasterize_gbuffer_prepared(const rnr_mesh* mesh, const float* v_uvz, const float* pose,
                                              int num_views, int image_size, float near_, float far_,
                                              const rnr_gbuffer* out, void* workspace, void* stream) {
    return rasterize_gbuffer_impl(mesh, v_uvz, pose, num_views, image_size, near_, far_, out, workspace, stream, true);
}
