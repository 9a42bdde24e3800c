// Shading-side kernels of the hot path (everything between the rasterizer and the U-Net, and after it).
//
//   project_vertices_kernel   nr.projection                      projection.py:6-53
//   face_tangents_kernel      per-face tangent of get_TBN_map    render.py:135-150
//   shade_inputs_kernel       TBN + view dir + SH(lmax 2) + 4-level neural texture + 26 rays + channel
//                             assembly -> channel-last network input, written once, coalesced
//                             (render.py:152-166, camera.py:5-45, test_rnr.py:303-356, network.py:67-91,
//                              network.py:445-472, misc.py:5-42, sph_harm.py:41-71)
//   ray_render_kernel         out-layer bias + tanh + RayRenderer (network.py:253, 481-527; test_rnr.py:357-359)
//   present_u8_kernel         the frame as cv2.imwrite gets it: 8-bit, channel-last, over the light-probe background
//                             (test_rnr.py:377, 386-393)
//   sh_basis / sh_reconstruct / sh_fit / interpolate_bilinear / layout helpers
//
// Built with -ffp-contract=off: the integer tap indices of the bilinear sampler (misc.py:16-25) must be the
// bits the reference's float32 expressions produce (u*(S-1), (S-1) - v*(S-1), floor), so no FMA contraction.
//
// Every per-pixel formula of the reference is stated ONCE, as a force-inlined device function that the fused kernels and
// the stand-alone operators of the drop-in API both call.  Without contraction and without fast-math the same operations
// on the same operands in the same order give the same bits wherever they are inlined.
//
//   NormExact / NormFast              normalize3 (sqrt + divisions) | normalize3_fast (v_rsq): the Norm argument below
//   TrigOcml / TrigPoly               equirect u, v from ocml's atan2f / acosf | the polynomial pair: the Trig argument
//   pixel_coords, view_dir<Norm>      view / row / column of a pixel; its camera / world view direction   camera.py:19-30
//   wrap_face_index, tbn_frame<Norm>  negative face-index wrap; N, B = N x T, T = B x N        render.py:152-161
//   reflect_ray<Norm>, tbn_ray<Norm>  reflected ray in tangent space; normalise(TBN . lt)      camera.py:43, network.py:455-465
//   ray_uv<Trig>                      rays_uv from a direction, alpha, the background -1       render.py:96-102, network.py:469-470
//   Taps::blend / Taps::blend_fma     four-tap blend, plain | explicit-FMA chain               misc.py:42
//   Taps::x / y / w / texel<I>, texel_offset<I>   tap j of the four; texel offsets in the calling kernel's index width
//   level_taps                        taps at the texture-level coordinates u (S-1), (S-1) - v (S-1)   network.py:71-85
//   envmap_taps, envmap_texels        env-map taps min(u W, W-1); the four texel pointers      network.py:497, misc.py:5-42
//   background_colour<Norm,Trig,FMA>  the light probe seen along -view_dir of a pixel           test_rnr.py:386-391
//   quantise_u8                       saturate_u8(round_half_even(v * 255)): the float -> 8-bit conversion of cv2.imwrite
//   element_coords                    (n, c, p, pix) of element i of an [N,C,hw] map: the drop-in operators' one lane per element
//   sh_scaled, texbwd_idle, texbwd_scatter_tap   TextureMapper's SH factor; its adjoint's skip rule and tap scatter, both forms
//   probe_colour<I>, ray_n_spec .. ray_group_albedo   RayRenderer and its adjoint: a ray's colour; the group rule   network.py:497-527
//   RA_PIX, RA_QTR, RA_CH, RayTile    the tiled form of both: prologue (uv staging), epilogue (partial sums in LDS), launch_ray_api
//   RayLanes                          32-lanes-per-pixel layout, net_in row staging, alpha of ray_render / ray_weights
//   view_offset                       view index and in-view offset from the workgroup quotient
// Host side: grid256 / ray_grid, transpose_pivots, fill_texture_levels, ray_launch_checks (ni_need and the shared checks),
// texture_mapper_operands / ray_renderer_operands (checks and parameter block of a forward and its adjoint), launch_ray_api.
// One exception: ray_render_kernel keeps the text of envmap_texels and Taps::blend_fma in its own body (sharing them changed
// its register allocation); the comment there names what it mirrors.
#include "rnr_internal.h"

namespace rnr {

#define RNR_PI_F 3.14159265358979323846f

__device__ __forceinline__ float3 f3(float x, float y, float z) { return make_float3(x, y, z); }
__device__ __forceinline__ float dot3(float3 a, float3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ float3 cross3(float3 a, float3 b) {
    return f3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
// torch.nn.functional.normalize: x / max(||x||_2, 1e-12)
__device__ __forceinline__ float3 normalize3(float3 a) {
    const float n = fmaxf(sqrtf(a.x * a.x + a.y * a.y + a.z * a.z), 1e-12f);
    return f3(a.x / n, a.y / n, a.z / n);
}

// same with the hardware reciprocal square root (v_rsq_f32, 1 ulp) instead of a correctly rounded sqrt and three
// correctly rounded divisions (~45 VALU instructions): for the fused shading kernel, whose unit vectors only feed
// float-tolerance quantities (ray directions, SH basis), never an integer index
__device__ __forceinline__ float3 normalize3_fast(float3 a) {
    const float inv = fminf(__builtin_amdgcn_rsqf(a.x * a.x + a.y * a.y + a.z * a.z), 1e12f);
    return f3(a.x * inv, a.y * inv, a.z * inv);
}
struct NormExact { static __device__ __forceinline__ float3 of(float3 a) { return normalize3(a); } };
struct NormFast { static __device__ __forceinline__ float3 of(float3 a) { return normalize3_fast(a); } };

// Polynomial atan2 / acos for the fused ray renderer (max abs error 3e-8 / 8e-8 rad, i.e. float rounding level; the
// uv they feed is only used to pick env-map taps).  ocml's atan2f/acosf cost ~100 instructions each and made this
// kernel transcendental-bound (26 rays per pixel).  The stand-alone ray-sampler operator keeps the ocml versions.
__device__ __forceinline__ float fast_atan2f(float y, float x) {
    const float ax = fabsf(x), ay = fabsf(y);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    const float a = mx > 0.0f ? mn * __builtin_amdgcn_rcpf(mx) : 0.0f;      // 1 ulp reciprocal: the result only picks env-map taps
    const float s = a * a;
    // explicit FMAs: this file is compiled with -ffp-contract=off (bit-exact tap indices elsewhere), which would turn
    // every Horner step into a multiply and an add — the kernel is VALU-bound
    float p = 0.002899040700867772f;
    p = __builtin_fmaf(p, s, -0.01637016236782074f);
    p = __builtin_fmaf(p, s, 0.04338274151086807f);
    p = __builtin_fmaf(p, s, -0.07582952827215195f);
    p = __builtin_fmaf(p, s, 0.10688958317041397f);
    p = __builtin_fmaf(p, s, -0.14219146966934204f);
    p = __builtin_fmaf(p, s, 0.19995006918907166f);
    p = __builtin_fmaf(p, s, -0.3333321213722229f);
    p = __builtin_fmaf(p, s, 1.0f);
    float r = p * a;
    if (ay > ax) r = 1.57079632679489662f - r;
    // quadrant from the sign BITS, as IEEE atan2 (ocml, torch.atan2) does: atan2(-0, x < 0) = -pi and atan2(+-0, -0) = +-pi.
    // A test of y < 0 gave +pi for y = -0 — u = 1 instead of 0, the env-map tap of column W-1 instead of column 0 — on the
    // seam direction an axis-aligned -x normal produces with the diffuse pivot (0, 0, 1)
    if (__builtin_signbit(x)) r = 3.14159265358979324f - r;
    return __builtin_copysignf(r, y);
}
__device__ __forceinline__ float fast_acosf(float x) {
    const float ax = fminf(fabsf(x), 1.0f);
    float p = -0.001102376147173345f;
    p = __builtin_fmaf(p, ax, 0.006096228025853634f);
    p = __builtin_fmaf(p, ax, -0.01627347804605961f);
    p = __builtin_fmaf(p, ax, 0.03031114861369133f);
    p = __builtin_fmaf(p, ax, -0.049957286566495895f);
    p = __builtin_fmaf(p, ax, 0.08893882483243942f);
    p = __builtin_fmaf(p, ax, -0.2145957499742508f);
    p = __builtin_fmaf(p, ax, 1.570796251296997f);
    const float r = __builtin_amdgcn_sqrtf(1.0f - ax) * p;
    return x < 0.0f ? 3.14159265358979324f - r : r;
}
// equirect u, v of a unit direction before the alpha mask (render.py:96-102): ocml's functions with the reference's
// operation order, or the polynomial pair with the scaling folded into one FMA / one multiplication
struct TrigOcml {
    static __device__ __forceinline__ float u(float z, float x) { return atan2f(z, x) * 0.5f / RNR_PI_F + 0.5f; }
    static __device__ __forceinline__ float v(float y) { return acosf(y) * 1.0f / RNR_PI_F; }
};
struct TrigPoly {
    static __device__ __forceinline__ float u(float z, float x) { return __builtin_fmaf(fast_atan2f(z, x), 0.5f / RNR_PI_F, 0.5f); }
    static __device__ __forceinline__ float v(float y) { return fast_acosf(y) * (1.0f / RNR_PI_F); }
};

// ---- the per-pixel formulas, each stated once -------------------------------------------------------
// view n, row and column of pixel pix of an [N,H,W] batch
__device__ __forceinline__ void pixel_coords(long pix, int H, int W, int& n, int& row, int& col) {
    const int hw = H * W;
    n = (int)(pix / hw);
    const int rem = (int)(pix % hw);
    row = rem / W; col = rem % W;
}
// view direction of pixel (row, col) of view n in camera (dc) and world (vd) coordinates (camera.py:19-30)
template <class Norm>
__device__ __forceinline__ void view_dir(const float* proj_inv, const float* R_inv, int n, int row, int col, float3& dc, float3& vd) {
    const float* Pi = proj_inv + n * 9;
    const float* Ri = R_inv + n * 9;
    const float pu = (float)col + 0.5f, pv = (float)row + 0.5f;    // camera.py:19-20
    float3 c = f3(-(Pi[0] * pu + Pi[1] * pv + Pi[2]), -(Pi[3] * pu + Pi[4] * pv + Pi[5]), -(Pi[6] * pu + Pi[7] * pv + Pi[8]));
    c = Norm::of(c);
    float3 w = f3(Ri[0] * c.x + Ri[1] * c.y + Ri[2] * c.z, Ri[3] * c.x + Ri[4] * c.y + Ri[5] * c.z,
                  Ri[6] * c.x + Ri[7] * c.y + Ri[8] * c.z);
    w = Norm::of(w);
    dc = c; vd = w;     // (locals, not the references, feed the second product: the callers' machine code stays what it was)
}

// row of the per-face tangent table a pixel's face index selects: torch's negative index wrap (render.py:152)
__device__ __forceinline__ int wrap_face_index(int fi, int num_faces) { return fi < 0 ? fi + num_faces : fi; }
// the orthonormal frame of get_TBN_map from the interpolated normal and the face tangent
template <class Norm>
__device__ __forceinline__ void tbn_frame(const float3& normal_in, const float3& tangent, float3& tt, float3& bt, float3& nm) {
    nm = Norm::of(normal_in);                   // render.py:155
    bt = Norm::of(cross3(nm, tangent));         // render.py:156-157
    tt = Norm::of(cross3(bt, nm));              // render.py:160-161
}

// tangent-space view direction v reflected about the pivot pv, scaled by alpha (camera.py:43, network.py:455-459)
template <class Norm>
__device__ __forceinline__ float3 reflect_ray(const float3& pv, const float3& v, float a) {
    const float s = dot3(pv, v) * 2.0f;                         // camera.py:43
    const float3 lt = Norm::of(f3(s * pv.x - v.x, s * pv.y - v.y, s * pv.z - v.z));
    return f3(lt.x * a, lt.y * a, lt.z * a);
}
// world direction of the tangent-space ray lt: normalise(TBN . lt), columns T, B, N (network.py:461-465).  The sums run
// T, B, N in this order whether the caller holds the columns (fused kernel) or the stored row-major 3x3 (ray sampler)
template <class Norm>
__device__ __forceinline__ float3 tbn_ray(const float3& tt, const float3& bt, const float3& nm, const float3& lt) {
    float3 d = f3(tt.x * lt.x + bt.x * lt.y + nm.x * lt.z, tt.y * lt.x + bt.y * lt.y + nm.y * lt.z,
                  tt.z * lt.x + bt.z * lt.y + nm.z * lt.z);
    d = Norm::of(d);
    return d;
}
// rays_uv of the unit direction d at a pixel of coverage a; background pixels get -1 (render.py:96-102, network.py:469-470)
template <class Trig>
__device__ __forceinline__ void ray_uv(const float3& d, float a, float& u, float& v) {
    u = Trig::u(d.z, d.x);
    v = Trig::v(d.y);
    const float bg = (a == 0.0f) ? 1.0f : 0.0f;
    u = u * a - bg;
    v = v * a - bg;
}

// ------------------------------------------------------------------------------------------------
// nr.projection for vertex i of the view batch (projection.py:6-53).  POSE: R and t are read straight from the [N,4,4] pose
// matrices (R = pose[:, :3, :3], t = pose[:, :3, 3]) — the same operands, the same arithmetic, the same bits as with the
// separate [N,3,3] / [N,3] tensors the reference builds (test_rnr.py:283-284).
template <bool POSE>
__device__ __forceinline__ void project_vertex(long i, const float* __restrict__ vertices, const float* __restrict__ K,
                                               const float* __restrict__ R, const float* __restrict__ t,
                                               const float* __restrict__ dist, const float* __restrict__ offset,
                                               const float* __restrict__ scale, float* __restrict__ out, int nviews, int nv,
                                               float orig_size, float eps) {
    if (i >= (long)nviews * nv) return;
    const int n = (int)(i / nv), vi = (int)(i % nv);
    const float* p = vertices + (size_t)vi * 3;
    constexpr int RS = POSE ? 4 : 3;            // row stride of R
    const float* Rn = R + n * (POSE ? 16 : 9);
    const float* Kn = K + n * 9;
    const float t0 = POSE ? Rn[3] : t[n * 3 + 0], t1 = POSE ? Rn[7] : t[n * 3 + 1], t2 = POSE ? Rn[11] : t[n * 3 + 2];
    const float vx = p[0], vy = p[1], vz = p[2];
    // vertices . R^T + t   (projection.py:22)
    const float x = vx * Rn[0] + vy * Rn[1] + vz * Rn[2] + t0;
    const float y = vx * Rn[RS + 0] + vy * Rn[RS + 1] + vz * Rn[RS + 2] + t1;
    const float z = vx * Rn[2 * RS + 0] + vy * Rn[2 * RS + 1] + vz * Rn[2 * RS + 2] + t2;
    const float xn = x / (z + eps), yn = y / (z + eps);
    float k1 = 0.f, k2 = 0.f, p1 = 0.f, p2 = 0.f, k3 = 0.f;
    if (dist) { k1 = dist[n * 5 + 0]; k2 = dist[n * 5 + 1]; p1 = dist[n * 5 + 2]; p2 = dist[n * 5 + 3]; k3 = dist[n * 5 + 4]; }
    const float r = sqrtf(xn * xn + yn * yn);
    const float r2 = r * r, r4 = r2 * r2, r6 = r4 * r2;
    const float radial = 1.0f + k1 * r2 + k2 * r4 + k3 * r6;
    const float xd = xn * radial + 2.0f * p1 * xn * yn + p2 * (r2 + 2.0f * xn * xn);
    const float yd = yn * radial + p1 * (r2 + 2.0f * yn * yn) + 2.0f * p2 * xn * yn;
    float u = xd * Kn[0] + yd * Kn[1] + Kn[2];
    float v = xd * Kn[3] + yd * Kn[4] + Kn[5];
    if (offset && scale) {  // projection.py:42-46 (note the swapped component order)
        u = (u + offset[n * 2 + 1]) * scale[n * 2 + 1];
        v = (v + offset[n * 2 + 0]) * scale[n * 2 + 0];
    }
    v = orig_size - v;
    u = 2.0f * (u - orig_size / 2.0f) / orig_size;
    v = 2.0f * (v - orig_size / 2.0f) / orig_size;
    out[i * 3 + 0] = u;
    out[i * 3 + 1] = v;
    out[i * 3 + 2] = z;
}

__global__ void __launch_bounds__(256)
project_vertices_kernel(const float* __restrict__ vertices, const float* __restrict__ K,
                        const float* __restrict__ R, const float* __restrict__ t,
                        const float* __restrict__ dist, const float* __restrict__ offset,
                        const float* __restrict__ scale, float* __restrict__ out, int nviews, int nv,
                        float orig_size, float eps) {
    project_vertex<false>((long)blockIdx.x * blockDim.x + threadIdx.x, vertices, K, R, t, dist, offset, scale, out, nviews, nv,
                          orig_size, eps);
}

// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void face_tangent(int i, const rnr_mesh& mesh, float* __restrict__ out) {
    if (i >= mesh.num_faces) return;
    const int32_t* vi = mesh.f_v_idx + (size_t)i * 3;
    const int32_t* ti = mesh.f_vt_idx + (size_t)i * 3;
    const float* a = mesh.v + (size_t)vi[0] * 3;
    const float* b = mesh.v + (size_t)vi[1] * 3;
    const float* c = mesh.v + (size_t)vi[2] * 3;
    const float* ta = mesh.vt + (size_t)ti[0] * 2;
    const float* tb = mesh.vt + (size_t)ti[1] * 2;
    const float* tc = mesh.vt + (size_t)ti[2] * 2;
    const float3 e1 = f3(b[0] - a[0], b[1] - a[1], b[2] - a[2]);
    const float3 e2 = f3(c[0] - a[0], c[1] - a[1], c[2] - a[2]);
    const float d1x = tb[0] - ta[0], d1y = tb[1] - ta[1];
    const float d2x = tc[0] - ta[0], d2y = tc[1] - ta[1];
    const float f = 1.0f / fmaxf(d1x * d2y - d2x * d1y, 1e-8f);   // clamp(min=1e-8), render.py:143
    const float3 tn = normalize3(f3(f * (d2y * e1.x - d1y * e2.x), f * (d2y * e1.y - d1y * e2.y),
                                    f * (d2y * e1.z - d1y * e2.z)));
    out[i * 3 + 0] = tn.x; out[i * 3 + 1] = tn.y; out[i * 3 + 2] = tn.z;
}

__global__ void __launch_bounds__(256)
face_tangents_kernel(rnr_mesh mesh, float* __restrict__ out) {
    face_tangent(blockIdx.x * blockDim.x + threadIdx.x, mesh, out);
}

// ------------------------------------------------------------------------------------------------
// offset of texel (x, y) of a channel-last [rows, width, C] map, in the index type I of the calling kernel
template <class I> __device__ __forceinline__ I texel_offset(int x, int y, int width, int C) { return ((I)y * width + x) * C; }
// bilinear taps of misc.interpolate_bilinear (misc.py:14-40)
struct Taps {
    int x0, y0, x1, y1;
    float w00, w10, w01, w11;
    // I00*w00 + I10*w10 + I01*w01 + I11*w11 (misc.py:42), every product rounded as the reference's torch ops round it
    __device__ __forceinline__ float blend(float i00, float i10, float i01, float i11) const {
        return i00 * w00 + i10 * w10 + i01 * w01 + i11 * w11;
    }
    // the same sum as an explicit FMA chain for the VALU-bound ray kernels (see fast_atan2f; <= 1 ulp from blend)
    __device__ __forceinline__ float blend_fma(float i00, float i10, float i01, float i11) const {
        return __builtin_fmaf(i11, w11, __builtin_fmaf(i01, w01, __builtin_fmaf(i10, w10, i00 * w00)));
    }
    // tap j of (w00, w10, w01, w11): its column, row, weight and the offset of its texel in a [rows, width, C] map
    __device__ __forceinline__ int x(int j) const { return j < 2 ? x0 : x1; }
    __device__ __forceinline__ int y(int j) const { return (j & 1) ? y1 : y0; }
    __device__ __forceinline__ float w(int j) const { return j == 0 ? w00 : j == 1 ? w10 : j == 2 ? w01 : w11; }
    template <class I> __device__ __forceinline__ I texel(int j, int width, int C) const { return texel_offset<I>(x(j), y(j), width, C); }
};
__device__ __forceinline__ Taps bilinear_taps(float x, float y, int W, int H) {
    Taps t;
    const float valid = (x >= 0.0f && x <= (float)(W - 1) && y >= 0.0f && y <= (float)(H - 1)) ? 1.0f : 0.0f;
    // floor -> int64 in the reference; clamp in float first so NaN / huge coordinates stay defined
    const float fx = floorf(x), fy = floorf(y);
    int x0 = (int)fminf(fmaxf(fx, -2.0f), (float)W + 1.0f);
    int y0 = (int)fminf(fmaxf(fy, -2.0f), (float)H + 1.0f);
    int x1 = x0 + 1, y1 = y0 + 1;
    x0 = min(max(x0, 0), W - 1); x1 = min(max(x1, 0), W - 1);
    y0 = min(max(y0, 0), H - 1); y1 = min(max(y1, 0), H - 1);
    t.x0 = x0; t.y0 = y0; t.x1 = x1; t.y1 = y1;
    const float x0w = (float)(x0 - (x0 == x1 ? 1 : 0)), y0w = (float)(y0 - (y0 == y1 ? 1 : 0));
    const float x1f = (float)x1, y1f = (float)y1;
    t.w00 = (x1f - x) * (y1f - y) * valid;
    t.w10 = (x1f - x) * (y - y0w) * valid;
    t.w01 = (x - x0w) * (y1f - y) * valid;
    t.w11 = (x - x0w) * (y - y0w) * valid;
    return t;
}
// colour of the probe channel lp [Hl, Wl, C] points at under t: the four texels times lp_scale, then the blend (network.py:497-503)
template <class I> __device__ __forceinline__ float probe_colour(const Taps& t, const float* lp, int lp_w, int C, float lp_scale) {
    return t.blend(lp[t.texel<I>(0, lp_w, C)] * lp_scale, lp[t.texel<I>(1, lp_w, C)] * lp_scale, lp[t.texel<I>(2, lp_w, C)] * lp_scale,
                   lp[t.texel<I>(3, lp_w, C)] * lp_scale);
}
// element i of an [N, C, hw] map: view n, channel c, pixel p of the view, pixel pix of the batch
__device__ __forceinline__ void element_coords(long i, int C, int hw, long& n, int& c, long& p, long& pix) {
    const long rem = i % ((long)C * hw);
    n = i / ((long)C * hw); c = (int)(rem / hw); p = rem % hw; pix = n * hw + p;
}
// taps of a square texture level of size s at uv (TextureMapper.forward, network.py:71-85): x = u (s-1), y = (s-1) - v (s-1)
__device__ __forceinline__ Taps level_taps(float u, float v, int s) {
    const float sm1 = (float)(s - 1);
    const float x = u * sm1;
    const float y = sm1 - v * sm1;
    return bilinear_taps(x, y, s, s);
}
// env-map taps of a ray (network.py:497; misc.py:5-42): clamp(max=) only, then the validity mask zeroes uv = -1.  The minimum
// is the NaN-propagating one, as torch.clamp is: fminf gave a NaN coordinate the last column / row, a valid
// tap, and the NaN never reached the colour (tests/test_gpu_shade_guard.py plants one); now the weights are NaN, as level_taps' are
__device__ __forceinline__ Taps envmap_taps(float u, float v, int lp_w, int lp_h) {
    const float x = __builtin_elementwise_minimum(u * (float)lp_w, (float)(lp_w - 1));
    const float y = __builtin_elementwise_minimum(v * (float)lp_h, (float)(lp_h - 1));
    return bilinear_taps(x, y, lp_w, lp_h);
}
// the four texels of a three-channel env map (lp_w3 = 3 lp_w) under the taps t.  Texel offsets with 24-bit multiplies (full
// rate; v_mul_lo_u32 runs at a quarter of it): the probe has far fewer than 2^24 floats
__device__ __forceinline__ void envmap_texels(const float* lp, int lp_w3, const Taps& t, const float*& l00,
                                              const float*& l10, const float*& l01, const float*& l11) {
    const unsigned r0 = __umul24((unsigned)t.y0, (unsigned)lp_w3), r1 = __umul24((unsigned)t.y1, (unsigned)lp_w3);
    const unsigned q0 = __umul24((unsigned)t.x0, 3u), q1 = __umul24((unsigned)t.x1, 3u);
    l00 = lp + (r0 + q0);
    l10 = lp + (r1 + q0);
    l01 = lp + (r0 + q1);
    l11 = lp + (r1 + q1);
}

// colour of the light probe lp [lp_h, lp_w, 3] behind pixel (row, col) of view n (test_rnr.py:386-391): the env-map taps of
// (u, v) = spherical_mapping(-view_dir_world).  The negation flips the sign BIT (fneg, not 0 - x): -(+0) = -0 has to reach atan2,
// which decides the seam by it (see fast_atan2f).  FMA selects Taps::blend_fma
template <class Norm, class Trig, bool FMA>
__device__ __forceinline__ void background_colour(const float* proj_inv, const float* R_inv, const float* lp, int lp_h, int lp_w,
                                                  int n, int row, int col, float& c0, float& c1, float& c2) {
    float3 dc, vd;
    view_dir<Norm>(proj_inv, R_inv, n, row, col, dc, vd);
    const float3 d = f3(-vd.x, -vd.y, -vd.z);
    const Taps t = envmap_taps(Trig::u(d.z, d.x), Trig::v(d.y), lp_w, lp_h);
    const float *l00, *l10, *l01, *l11;
    envmap_texels(lp, lp_w * 3, t, l00, l10, l01, l11);
    if (FMA) {
        c0 = t.blend_fma(l00[0], l10[0], l01[0], l11[0]);
        c1 = t.blend_fma(l00[1], l10[1], l01[1], l11[1]);
        c2 = t.blend_fma(l00[2], l10[2], l01[2], l11[2]);
    } else {
        c0 = t.blend(l00[0], l10[0], l01[0], l11[0]);
        c1 = t.blend(l00[1], l10[1], l01[1], l11[1]);
        c2 = t.blend(l00[2], l10[2], l01[2], l11[2]);
    }
}

// q(v) = saturate_u8(round_half_even(v * 255)): one float32 product, v_rndne_f32, then the clamp as two selects whose
// comparisons are false for a NaN: NaN -> 0, +inf -> 255, -inf -> 0 (what cv::Mat::convertTo(CV_8U) does to the float array
// test_rnr.py:377 hands to cv2.imwrite)
__device__ __forceinline__ unsigned quantise_u8(float v) {
    float t = __builtin_rintf(v * 255.0f);
    t = t > 0.0f ? t : 0.0f;
    t = t < 255.0f ? t : 255.0f;
    return (unsigned)t;
}

constexpr int SH_PIX = 32;        // pixels per workgroup (32 beat 16 / 64 / 128 on the GPU: 17 KB of LDS, 9 workgroups per CU)
constexpr int SH_THREADS = 256;
constexpr int MAX_LEVELS = 8;
constexpr int MAX_RAYS = 32;

struct ShadeParams {
    const int32_t* face_index_map;
    const float* alpha;
    const float* uv_map;
    const float* normal_map;
    const float* tangents;
    int num_faces;
    const float* proj_inv;
    const float* R_inv;
    const float* tex[MAX_LEVELS];
    int tex_size[MAX_LEVELS];
    int num_levels, C, sh_start;
    float piv_spec[MAX_RAYS * 3];   // [r][xyz]
    float piv_diff[MAX_RAYS * 3];
    int n_spec, n_diff;
    float* net_in;
    int c_pad;
    float* rays_uv;
    float* neural_img;
    float* sh_basis_map;
    long npix;                      // N*H*W
    int H, W;
};

// sum over the levels of the bilinear fetch of channel quad q at (u, v)  (TextureMapper.forward, network.py:71-85; the
// integer taps follow misc.py:16-35 exactly: this file is built without FMA contraction)
__device__ __forceinline__ float4 texture_quad(const ShadeParams& P, float u, float v, int q, int quads) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int l = 0; l < P.num_levels; l++) {
        const int s = P.tex_size[l];
        const Taps t = level_taps(u, v, s);
        // r04: a workgroup-uniform buffer resource per level and one 32-bit lane offset per tap (a level of <= 2 GiB): the flat
        // form spent ~6 VALU instructions of 64-bit address arithmetic on each of the 16 gathers of an item
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(P.tex[l]), 0, 0x7fffffff, 0x27000);
        const unsigned texel = (unsigned)quads * 16u, rowb = (unsigned)s * texel;
        const unsigned r0 = (unsigned)t.y0 * rowb + (unsigned)q * 16u, r1 = (unsigned)t.y1 * rowb + (unsigned)q * 16u;
        const unsigned c0 = (unsigned)t.x0 * texel, c1 = (unsigned)t.x1 * texel;
        auto tap = [&](unsigned off) { return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)off, 0, 0)); };
        const float4 i00 = tap(r0 + c0);
        const float4 i10 = tap(r1 + c0);
        const float4 i01 = tap(r0 + c1);
        const float4 i11 = tap(r1 + c1);
        const float4 lv = make_float4(t.blend(i00.x, i10.x, i01.x, i11.x), t.blend(i00.y, i10.y, i01.y, i11.y),
                                      t.blend(i00.z, i10.z, i01.z, i11.z), t.blend(i00.w, i10.w, i01.w, i11.w));
        if (l == 0) acc = lv;
        else { acc.x += lv.x; acc.y += lv.y; acc.z += lv.z; acc.w += lv.w; }
    }
    return acc;
}

// geometry record per pixel in LDS: T(3) B(3) N(3) vtan(3) uv(2) alpha(1) sh(9) = 24 floats
constexpr int GEO = 24;

__global__ void __launch_bounds__(SH_THREADS)
shade_inputs_kernel(const ShadeParams P) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* tile = smem;                               // [SH_PIX][c_pad]
    float* geo = smem + SH_PIX * P.c_pad;             // [SH_PIX][GEO]
    const int tid = threadIdx.x;
    const long pix0 = (long)blockIdx.x * SH_PIX;
    const int cp = P.c_pad;
    const int n_rays = P.n_spec + P.n_diff;
    const int c_geo = 3 * n_rays;                     // first channel of normal

    // zero the padding channels once
    const int c_in = c_geo + 6 + P.C;
    for (int i = tid; i < SH_PIX * (cp - c_in); i += SH_THREADS) {
        const int p = i / (cp - c_in), c = c_in + i % (cp - c_in);
        tile[p * cp + c] = 0.0f;
    }

    // ---- phase 2a (waves 1..3): the texture gathers, issued FIRST ----
    // Phase 0 is a chain of dependent loads on 32 lanes of wave 0 (face index -> tangent -> frame); the 16 bilinear gathers
    // of a (pixel, channel quad) item depend on the uv map only.  With C = 24 the 32 x 6 items are exactly the 192 threads of
    // waves 1..3, which fetch and blend them while wave 0 walks its chain: the two latency chains of a workgroup overlap
    // instead of following each other (the kernel is latency-bound).  The SH factor (phase 0's result) is
    // applied after the barrier; more than 192 items fall back to the loop behind phase 1.
    const int quads = P.C / 4;
    const bool tex_early = SH_PIX * quads <= SH_THREADS - 64;
    float4 tex_acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int tex_p = -1, tex_q = 0;
    if (tex_early && tid >= 64 && tid - 64 < SH_PIX * quads) {
        const int i = tid - 64;
        tex_p = i / quads; tex_q = i - tex_p * quads;
        const long pix = pix0 + tex_p;
        float u = 0.f, v = 0.f;
        if (pix < P.npix) { u = P.uv_map[pix * 2 + 0]; v = P.uv_map[pix * 2 + 1]; }
        tex_acc = texture_quad(P, u, v, tex_q, quads);
    }

    // ---- phase 0: one lane per pixel: TBN, view direction, SH basis ----
    if (tid < SH_PIX) {
        const long pix = pix0 + tid;
        float* g = geo + tid * GEO;
        if (pix < P.npix) {
            int n, row, col;
            pixel_coords(pix, P.H, P.W, n, row, col);
            const int fi = wrap_face_index(P.face_index_map[pix], P.num_faces);
            const float a = P.alpha[pix];
            const float3 tg = f3(P.tangents[fi * 3 + 0], P.tangents[fi * 3 + 1], P.tangents[fi * 3 + 2]);
            const float3 nm_in = f3(P.normal_map[pix * 3 + 0], P.normal_map[pix * 3 + 1], P.normal_map[pix * 3 + 2]);
            float3 tt, bt, nm, dc, vd;
            tbn_frame<NormFast>(nm_in, tg, tt, bt, nm);
            view_dir<NormFast>(P.proj_inv, P.R_inv, n, row, col, dc, vd);
            // tangent-space view direction = normalize(TBN^T v) (test_rnr.py:314-315)
            const float3 vt = normalize3_fast(f3(dot3(tt, vd), dot3(bt, vd), dot3(nm, vd)));
            g[0] = tt.x; g[1] = tt.y; g[2] = tt.z;
            g[3] = bt.x; g[4] = bt.y; g[5] = bt.z;
            g[6] = nm.x; g[7] = nm.y; g[8] = nm.z;
            g[9] = vt.x; g[10] = vt.y; g[11] = vt.z;
            g[12] = P.uv_map[pix * 2 + 0]; g[13] = P.uv_map[pix * 2 + 1];
            g[14] = a;
            // real SH, lmax = 2, orthonormal, no Condon-Shortley phase, colatitude from +z
            const float3 d = normalize3_fast(vd);
            float* sh = g + 15;
            sh[0] = 0.28209479177387814f;
            sh[1] = 0.4886025119029199f * d.y;
            sh[2] = 0.4886025119029199f * d.z;
            sh[3] = 0.4886025119029199f * d.x;
            sh[4] = 1.0925484305920792f * d.x * d.y;
            sh[5] = 1.0925484305920792f * d.y * d.z;
            sh[6] = 0.31539156525252005f * (3.0f * d.z * d.z - 1.0f);
            sh[7] = 1.0925484305920792f * d.x * d.z;
            sh[8] = 0.5462742152960396f * (d.x * d.x - d.y * d.y);
            if (P.sh_basis_map) {
#pragma unroll
                for (int k = 0; k < 9; k++) P.sh_basis_map[pix * 9 + k] = sh[k];
            }
            float* tp = tile + tid * cp + c_geo;      // channels: normal (3), view_dir (3) (test_rnr.py:351-352)
            tp[0] = nm_in.x; tp[1] = nm_in.y; tp[2] = nm_in.z;
            tp[3] = vd.x; tp[4] = vd.y; tp[5] = vd.z;
        } else {
            for (int k = 0; k < GEO; k++) g[k] = 0.0f;
        }
    }
    __syncthreads();

    // ---- phase 1: (pixel, ray) items: reflect / diffuse directions (network.py:455-465) ----
    // lanes run over the rays of a pixel first: a wave stores 3-float records at a stride of 3 floats (3 is coprime with
    // the 32 banks: conflict-free), and reads the geometry record of only ~3 pixels (LDS broadcast).  With the pixel
    // fastest every lane of a wave hit one of two banks (row stride 112 floats = 16 mod 32): 16-way conflicts,
    // 72 M conflict cycles per dispatch in the round-1 profile.
    const float inv_rays = 1.0f / (float)n_rays;
    for (int i = tid; i < SH_PIX * n_rays; i += SH_THREADS) {
        const int p = (int)(((float)i + 0.5f) * inv_rays), r = i - p * n_rays;      // exact i / n_rays for i < 2^20

        const float* g = geo + p * GEO;
        const float3 tt = f3(g[0], g[1], g[2]), bt = f3(g[3], g[4], g[5]), nm = f3(g[6], g[7], g[8]);
        const float a = g[14];
        float3 lt;   // direction in tangent space
        if (r < P.n_spec) {
            const float3 pv = f3(P.piv_spec[r * 3 + 0], P.piv_spec[r * 3 + 1], P.piv_spec[r * 3 + 2]);
            lt = reflect_ray<NormFast>(pv, f3(g[9], g[10], g[11]), a);
        } else {
            const int rd = r - P.n_spec;
            lt = f3(P.piv_diff[rd * 3 + 0], P.piv_diff[rd * 3 + 1], P.piv_diff[rd * 3 + 2]);
        }
        const float3 d = tbn_ray<NormFast>(tt, bt, nm, lt);
        float* tp = tile + p * cp + 3 * r;                              // ray-major, xyz inner (test_rnr.py:350)
        tp[0] = d.x; tp[1] = d.y; tp[2] = d.z;
        if (P.rays_uv) {
            const long pix = pix0 + p;
            if (pix < P.npix) {
                float u, v;
                ray_uv<TrigOcml>(d, a, u, v);
                P.rays_uv[(pix * 2 + 0) * n_rays + r] = u;
                P.rays_uv[(pix * 2 + 1) * n_rays + r] = v;
            }
        }
    }

    // ---- phase 2: (pixel, channel-quad) items: sum over levels of bilinear fetches (network.py:71-85) ----
    const float inv_quads = 1.0f / (float)quads;
    auto finish_quad = [&](float4 acc, int p, int q) {
        const float* g = geo + p * GEO;
        if (P.sh_start >= 0) {  // output[:, s:s+9] *= sh_basis (network.py:88-89)
            const float* sh = g + 15;
            const int c0 = 4 * q - P.sh_start;
            if (c0 + 0 >= 0 && c0 + 0 < 9) acc.x *= sh[c0 + 0];
            if (c0 + 1 >= 0 && c0 + 1 < 9) acc.y *= sh[c0 + 1];
            if (c0 + 2 >= 0 && c0 + 2 < 9) acc.z *= sh[c0 + 2];
            if (c0 + 3 >= 0 && c0 + 3 < 9) acc.w *= sh[c0 + 3];
        }
        float* tp = tile + p * cp + c_geo + 6 + 4 * q;
        if (((c_geo + 6) & 3) == 0) *reinterpret_cast<float4*>(tp) = acc;     // one ds_write_b128 (rows are 16-byte aligned)
        else { tp[0] = acc.x; tp[1] = acc.y; tp[2] = acc.z; tp[3] = acc.w; }
    };
    if (tex_early) {
        if (tex_p >= 0) finish_quad(tex_acc, tex_p, tex_q);
    } else {
        for (int i = tid; i < SH_PIX * quads; i += SH_THREADS) {
            const int p = (int)(((float)i + 0.5f) * inv_quads), q = i - p * quads;
            const float* g = geo + p * GEO;
            finish_quad(texture_quad(P, g[12], g[13], q, quads), p, q);
        }
    }
    __syncthreads();

    // ---- phase 3: one coalesced sweep of the tile to HBM ----
    const long valid_pix = min((long)SH_PIX, P.npix - pix0);
    const int n4 = (int)(valid_pix * cp / 4);
    float4* dst = reinterpret_cast<float4*>(P.net_in + pix0 * cp);
    const float4* src = reinterpret_cast<const float4*>(tile);
    for (int i = tid; i < n4; i += SH_THREADS) dst[i] = src[i];
    if (P.neural_img) {  // [N, C, H, W] copy for the API (TextureMapper.forward's return value)
        const int hw = P.H * P.W;
        // i runs over a grid of SH_PIX pixels per channel, so the bound is SH_PIX * C even in a ragged last workgroup
        // (valid_pix * C would stop before the last channels); the pixels past the end are masked below
        for (int i = tid; i < SH_PIX * P.C; i += SH_THREADS) {
            const int p = i % SH_PIX, c = i / SH_PIX;
            if (p < valid_pix) {
                const long pix = pix0 + p;
                const long n = pix / hw, rem = pix % hw;
                P.neural_img[(n * P.C + c) * hw + rem] = tile[p * cp + c_geo + 6 + c];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Ray renderer: 32 lanes per pixel (one ray each), 16-lane segmented shuffle reductions.
// lane layout inside a 32-lane half: lanes 0..15 -> specular rays 0..15, lanes 16..31 -> diffuse rays 0..15
// ------------------------------------------------------------------------------------------------

struct RayParams {
    const float* unet_raw; int c_out_pad;
    const float* bias;
    const float* net_in; int c_pad;
    const float* alpha;
    const float* lp; int lp_h, lp_w;
    int n_spec, n_diff, alb_diff_ch, alb_spec_ch;
    float* image;
    long npix; int hw;
    int ni_need;        // floats of a net_in row the kernel reads (directions, normal / view, albedo), multiple of 4
};

// sum over each aligned group of 16 lanes, result in every lane of the group: four DPP adds on the VALU (quad_perm
// swaps 1 and 2 apart, row_half_mirror and row_mirror fold 8 and 16 lanes) instead of four ds_bpermute round trips
__device__ __forceinline__ float dpp_add(float v, const int ctrl_sel) {
    const int x = __builtin_bit_cast(int, v);
    int y;
    if (ctrl_sel == 0) y = __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, false);        // quad_perm [1,0,3,2]
    else if (ctrl_sel == 1) y = __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, false);   // quad_perm [2,3,0,1]
    else if (ctrl_sel == 2) y = __builtin_amdgcn_update_dpp(0, x, 0x141, 0xF, 0xF, false);  // row_half_mirror
    else y = __builtin_amdgcn_update_dpp(0, x, 0x140, 0xF, 0xF, false);                     // row_mirror
    return v + __builtin_bit_cast(float, y);
}
__device__ __forceinline__ float seg16_sum(float v) {
    v = dpp_add(v, 0);
    v = dpp_add(v, 1);
    v = dpp_add(v, 2);
    v = dpp_add(v, 3);
    return v;
}

#ifndef RNR_RR_PIX
#define RNR_RR_PIX 4
#endif
constexpr int RR_PIX = RNR_RR_PIX;     // pixels per lane: independent load chains in flight (the kernel is latency-bound)
// a 32-lane half-wave owns RR_PIX consecutive pixels; a workgroup owns 8 * RR_PIX consecutive pixels, so every
// global address is a workgroup-uniform base (SGPR pair) plus a small 32-bit lane offset: no 64-bit VALU math
constexpr int RR_WG_PIX = 8 * RR_PIX;

// What ray_render_kernel and ray_weights_kernel share: the lane layout above, the coverage of a lane's pixels and the staging
// of the workgroup's net_in rows
struct RayLanes {
    int sub, lp0;           // lane inside the 32-lane half; first pixel of this half-wave inside the workgroup
    bool is_diff, ray_live; // diffuse group; the lane holds a ray
    int r;                  // its index among the n_spec + n_diff rays
    int wg_valid;           // pixels of the workgroup inside the batch
    __device__ __forceinline__ RayLanes(int n_spec, int n_diff, long npix, long wg_pix0) {
        sub = (int)(threadIdx.x & 31);
        lp0 = (int)(threadIdx.x >> 5) * RR_PIX;
        is_diff = sub >= 16;
        const int rr = sub & 15;
        ray_live = is_diff ? rr < n_diff : rr < n_spec;
        r = is_diff ? n_spec + rr : rr;
        wg_valid = (int)min((long)RR_WG_PIX, npix - wg_pix0);
    }
    __device__ __forceinline__ void load_alpha(const float* wg_alpha, float (&al)[RR_PIX]) const {
#pragma unroll
        for (int k = 0; k < RR_PIX; k++) al[k] = (lp0 + k < wg_valid) ? wg_alpha[lp0 + k] : 0.0f;
    }
    // Stage the workgroup's rows in LDS with coalesced float4 loads: the vector memory path retires one wave instruction
    // per ~16 cycles whatever its width, and 3-float-per-lane reads of the rows cost 7 instructions per (pixel, lane
    // group) — 112 per 32 pixels against 22 for the float4 sweep.  ni_need = ray directions + normal / view + the albedo
    // channels, rounded up to whole float4s (multiple of 4, <= c_pad): s_ni is [RR_WG_PIX][ni_need]
    __device__ __forceinline__ void stage_net_in(float* s_ni, const float* wg_net_in, int c_pad, int ni_need) const {
        const int q_ni = ni_need >> 2;
        const float inv_q = 1.0f / (float)q_ni;
        for (int i = threadIdx.x; i < wg_valid * q_ni; i += 256) {
            const int p = (int)(((float)i + 0.5f) * inv_q), q4 = i - __mul24(p, q_ni);
            reinterpret_cast<float4*>(s_ni)[i] = *reinterpret_cast<const float4*>(wg_net_in + (unsigned)(__mul24(p, c_pad) + 4 * q4));
        }
    }
};
// view and in-view offset of the pixel at offset rem0 >= 0 from the start of view n0, walked from the workgroup's (scalar)
// quotient: no per-lane 64-bit division
__device__ __forceinline__ void view_offset(long n0, int rem0, int hw, long& n, int& rem) {
    rem = rem0;
    n = n0;
    while (rem >= hw) { rem -= hw; n += 1; }      // at most once unless a view has fewer pixels than a workgroup
}

__global__ void __launch_bounds__(256)
ray_render_kernel(const RayParams P) {
    constexpr int PIX_PER_WG = RR_WG_PIX;
    const long wg_pix0 = (long)blockIdx.x * PIX_PER_WG;
    const RayLanes L(P.n_spec, P.n_diff, P.npix, wg_pix0);
    const int sub = L.sub, lp0 = L.lp0, r = L.r, wg_valid = L.wg_valid;
    const bool ray_live = L.ray_live;
    const long pix0 = wg_pix0 + lp0;
    const long wg_n0 = wg_pix0 / P.hw;                       // workgroup-uniform (SALU)
    const int wg_rem0 = (int)(wg_pix0 - wg_n0 * P.hw);
    const float* wg_net_in = P.net_in + wg_pix0 * P.c_pad;
    const float* wg_raw = P.unet_raw + wg_pix0 * P.c_out_pad;
    const float* wg_alpha = P.alpha + wg_pix0;
    // unet_raw and net_in rows go through LDS (RayLanes::stage_net_in)
    extern __shared__ __attribute__((aligned(16))) float rr_smem[];
    const int ni_need = P.ni_need;                          // multiple of 4, <= c_pad
    float* s_raw = rr_smem;                                 // [PIX_PER_WG][c_out_pad]
    float* s_ni = rr_smem + PIX_PER_WG * P.c_out_pad;       // [PIX_PER_WG][ni_need]
    float al[RR_PIX];
    L.load_alpha(wg_alpha, al);
    {
        // r04: a workgroup whose 32 pixels are all background writes its zeros and is done — the frame is exactly 0 there
        // whatever the network produced (rays_uv = -1 masks every env-map tap, network.py:469-470, 497), so neither the 320 +
        // 368 bytes per pixel of unet_raw / net_in nor the 26 rays are touched (bit-identical frames; about half of the bench
        // scene's pixels)
        int fg = 0;
#pragma unroll
        for (int k = 0; k < RR_PIX; k++) fg |= al[k] != 0.0f ? 1 : 0;
        if (!__syncthreads_or(fg)) {
            if (sub == 0) {
#pragma unroll
                for (int k = 0; k < RR_PIX; k++) {
                    if (lp0 + k >= wg_valid) continue;
                    int rem;
                    long n;
                    view_offset(wg_n0, wg_rem0 + lp0 + k, P.hw, n, rem);
#pragma unroll
                    for (int c = 0; c < 3; c++) P.image[(n * 3 + c) * P.hw + rem] = 0.0f;
                }
            }
            return;
        }
    }
    {
        const int q_raw = P.c_out_pad >> 2;
        const float4* g_raw = reinterpret_cast<const float4*>(wg_raw);
        for (int i = threadIdx.x; i < wg_valid * q_raw; i += 256) reinterpret_cast<float4*>(s_raw)[i] = g_raw[i];
        L.stage_net_in(s_ni, wg_net_in, P.c_pad, ni_need);
    }
    __syncthreads();
    float dx[RR_PIX], dy[RR_PIX], dz[RR_PIX], y0[RR_PIX], y1[RR_PIX], y2[RR_PIX];
    bool live[RR_PIX];
#pragma unroll
    for (int k = 0; k < RR_PIX; k++) {
        live[k] = ray_live && (lp0 + k < wg_valid);
        dx[k] = dy[k] = dz[k] = y0[k] = y1[k] = y2[k] = 0.f;
        if (live[k]) {      // lanes of a half-wave read 3-float records at a stride of 3 floats: conflict-free
            const float* d = s_ni + __mul24(lp0 + k, ni_need) + 3 * r;
            const float* yr = s_raw + __mul24(lp0 + k, P.c_out_pad) + 3 * r;
            dx[k] = d[0]; dy[k] = d[1]; dz[k] = d[2];
            y0[k] = yr[0]; y1[k] = yr[1]; y2[k] = yr[2];
        }
    }
    float b0 = 0.f, b1 = 0.f, b2 = 0.f;
    if (ray_live) { b0 = P.bias[3 * r + 0]; b1 = P.bias[3 * r + 1]; b2 = P.bias[3 * r + 2]; }
    Taps tp[RR_PIX];
#pragma unroll
    for (int k = 0; k < RR_PIX; k++) {
        float u, v;
        ray_uv<TrigPoly>(f3(dx[k], dy[k], dz[k]), al[k], u, v);
        tp[k] = envmap_taps(u, v, P.lp_w, P.lp_h);
    }
    // mean over the rays of a group as a multiplication by the reciprocal (one division per thread instead of six
    // correctly rounded ones per pixel; <= 1 ulp from network.py:505-513's `.sum(1) / num_ray`)
    const int lp_w3 = P.lp_w * 3;
    const float inv_spec = 1.0f / (float)P.n_spec;
    const float inv_diff = P.n_diff > 0 ? 1.0f / (float)P.n_diff : 0.0f;
    float c0[RR_PIX], c1[RR_PIX], c2[RR_PIX];
#pragma unroll
    for (int k = 0; k < RR_PIX; k++) {
        c0[k] = c1[k] = c2[k] = 0.f;
        if (live[k]) {
            const Taps& t = tp[k];
            // (mirrors envmap_texels and Taps::blend_fma: sharing them changed this kernel's register allocation)
            const unsigned r0 = __umul24((unsigned)t.y0, (unsigned)lp_w3), r1 = __umul24((unsigned)t.y1, (unsigned)lp_w3);
            const unsigned q0 = __umul24((unsigned)t.x0, 3u), q1 = __umul24((unsigned)t.x1, 3u);
            const float* l00 = P.lp + (r0 + q0);
            const float* l10 = P.lp + (r1 + q0);
            const float* l01 = P.lp + (r0 + q1);
            const float* l11 = P.lp + (r1 + q1);
            const float col0 = __builtin_fmaf(l11[0], t.w11, __builtin_fmaf(l01[0], t.w01, __builtin_fmaf(l10[0], t.w10, l00[0] * t.w00)));
            const float col1 = __builtin_fmaf(l11[1], t.w11, __builtin_fmaf(l01[1], t.w01, __builtin_fmaf(l10[1], t.w10, l00[1] * t.w00)));
            const float col2 = __builtin_fmaf(l11[2], t.w11, __builtin_fmaf(l01[2], t.w01, __builtin_fmaf(l10[2], t.w10, l00[2] * t.w00)));
            // network.py:253 tanh; test_rnr.py:359 (y*0.5+0.5)*2 = y + 1 (the two scalings by 2 are exact)
            c0[k] = fast_tanh_plus1f(y0[k] + b0) * col0;
            c1[k] = fast_tanh_plus1f(y1[k] + b1) * col1;
            c2[k] = fast_tanh_plus1f(y2[k] + b2) * col2;
            // background pixels contribute exactly 0 whatever the network produced there (col = 0 by the uv = -1
            // mask); select rather than multiply: the out layer may have skipped the tile (rnr_conv2d_masked) and
            // left non-finite garbage.  Done here, after every load has landed, so the loads stay independent.
            if (al[k] == 0.0f) { c0[k] = 0.f; c1[k] = 0.f; c2[k] = 0.f; }
        }
    }
#pragma unroll
    for (int k = 0; k < RR_PIX; k++) {
        const float s0 = seg16_sum(c0[k]), s1 = seg16_sum(c1[k]), s2 = seg16_sum(c2[k]);
        // lane 0 of each 16-lane segment holds its segment's sum; bring the diffuse sum to the group's first lane
        const float d0 = __shfl_down(s0, 16, 64), d1 = __shfl_down(s1, 16, 64), d2 = __shfl_down(s2, 16, 64);
        const long pix = pix0 + k;
        if (sub == 0 && pix < P.npix) {
            const float* ni = s_ni + __mul24(lp0 + k, ni_need) + 3 * (P.n_spec + P.n_diff) + 6;
            int rem;
            long n;
            view_offset(wg_n0, wg_rem0 + lp0 + k, P.hw, n, rem);
            const float o[3] = {s0, s1, s2}, dd[3] = {d0, d1, d2};
#pragma unroll
            for (int c = 0; c < 3; c++) {
                float out = ni[P.alb_spec_ch + c] * (o[c] * inv_spec);
                if (P.n_diff > 0) out = out + ni[P.alb_diff_ch + c] * (dd[c] * inv_diff);
                P.image[(n * 3 + c) * P.hw + rem] = out;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Ray weights: the part of the ray renderer that does not depend on the U-Net (rnr_ray_weights; the rest runs in the
// out-layer convolution's epilogue, rnr_conv2d_ray).  For pixel p, ray r, colour channel c
//     W[p][3 r + c] = albedo_group(r)[p][c] * env-map colour(direction of ray r)[c] / rays in the group
// so that the frame is  image[p][c] = sum_r (tanh(y[p][3 r + c] + b[3 r + c]) + 1) * W[p][3 r + c]  (network.py:253, 481-527,
// test_rnr.py:357-359).  Same lane layout, uv arithmetic and taps as ray_render_kernel; background pixels get W = 0.
// ------------------------------------------------------------------------------------------------
struct RayWeightParams {
    const float* net_in; int c_pad;
    const float* alpha;
    const float* lp; int lp_h, lp_w;
    int n_spec, n_diff, alb_diff_ch, alb_spec_ch;
    float* ray_w; int c_w;          // [npix][c_w], c_w >= 3 * rays (padding columns are written as zeros)
    long npix;
    int ni_need;
};

__global__ void __launch_bounds__(256)
ray_weights_kernel(const RayWeightParams P) {
    constexpr int PIX_PER_WG = RR_WG_PIX;
    const long wg_pix0 = (long)blockIdx.x * PIX_PER_WG;
    const RayLanes L(P.n_spec, P.n_diff, P.npix, wg_pix0);
    const int sub = L.sub, lp0 = L.lp0, r = L.r, wg_valid = L.wg_valid;
    const bool is_diff = L.is_diff, ray_live = L.ray_live;
    const float* wg_net_in = P.net_in + wg_pix0 * P.c_pad;
    const float* wg_alpha = P.alpha + wg_pix0;
    extern __shared__ __attribute__((aligned(16))) float rw_smem[];
    const int ni_need = P.ni_need;
    float* s_ni = rw_smem;                                  // [PIX_PER_WG][ni_need]
    float* s_w = rw_smem + PIX_PER_WG * ni_need;            // [PIX_PER_WG][c_w]: the weights leave as coalesced float4 rows
    L.stage_net_in(s_ni, wg_net_in, P.c_pad, ni_need);
    float al[RR_PIX];
    L.load_alpha(wg_alpha, al);
    __syncthreads();
    const int lp_w3 = P.lp_w * 3;
    const float inv_n = is_diff ? (P.n_diff > 0 ? 1.0f / (float)P.n_diff : 0.0f) : 1.0f / (float)P.n_spec;
    const int alb_ch = 3 * (P.n_spec + P.n_diff) + 6 + (is_diff ? P.alb_diff_ch : P.alb_spec_ch);
    const int n_cols = 3 * (P.n_spec + P.n_diff);
#pragma unroll
    for (int k = 0; k < RR_PIX; k++) {
        if (lp0 + k >= wg_valid) continue;
        float* out = s_w + __mul24(lp0 + k, P.c_w);
        if (sub == 31) for (int c = n_cols; c < P.c_w; c++) out[c] = 0.0f;        // padding columns (lane 31 never holds a ray)
        if (!ray_live) continue;
        const float* d = s_ni + __mul24(lp0 + k, ni_need) + 3 * r;
        float u, v;
        ray_uv<TrigPoly>(f3(d[0], d[1], d[2]), al[k], u, v);
        const Taps t = envmap_taps(u, v, P.lp_w, P.lp_h);
        const float *l00, *l10, *l01, *l11;
        envmap_texels(P.lp, lp_w3, t, l00, l10, l01, l11);
        const float* alb = s_ni + __mul24(lp0 + k, ni_need) + alb_ch;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float col = t.blend_fma(l00[c], l10[c], l01[c], l11[c]);
            out[3 * r + c] = (al[k] == 0.0f) ? 0.0f : alb[c] * (col * inv_n);
        }
    }
    __syncthreads();
    {
        const int n4 = wg_valid * P.c_w / 4;               // c_w is a multiple of 4 (the out layer's channel stride)
        float4* dst = reinterpret_cast<float4*>(P.ray_w + wg_pix0 * P.c_w);
        for (int i = threadIdx.x; i < n4; i += 256) dst[i] = reinterpret_cast<const float4*>(s_w)[i];
    }
}

// ------------------------------------------------------------------------------------------------
// Ray transport (rnr_ray_transport): the lighting-independent state of ray_render_kernel unpacked into the tensors
// RayRenderer.forward takes, so that the frame under ANY probe is rnr_ray_renderer of them (and its adjoint
// rnr_ray_renderer_backward).  Same lane layout, staging and uv arithmetic as ray_render_kernel: the taps of the unpacked
// uv are that kernel's taps.  Background pixels get uv = -1 and rays_lt = 0 by select (the out layer may have skipped their
// tile and left non-finite values).  The outputs leave through LDS: uv rows are contiguous per pixel, rays_lt and the
// albedos are written along the pixels of a plane.
// ------------------------------------------------------------------------------------------------
struct RayTransportParams {
    const float* unet_raw; int c_out_pad;
    const float* bias;
    const float* net_in; int c_pad;
    const float* alpha;
    int n_spec, n_diff, alb_diff_ch, alb_spec_ch;
    float* rays_uv;     // [N,H,W,2,R]
    float* rays_lt;     // [N,R,3,H,W]
    float* alb_spec;    // [N,3,H,W]
    float* alb_diff;    // [N,3,H,W]
    long npix; int hw;
    int ni_need;
};

__global__ void __launch_bounds__(256)
ray_transport_kernel(const RayTransportParams P) {
    constexpr int PIX_PER_WG = RR_WG_PIX, LT_ROW = RR_WG_PIX + 1;
    static_assert((PIX_PER_WG & (PIX_PER_WG - 1)) == 0, "the plane sweep splits its item index with a mask");
    const long wg_pix0 = (long)blockIdx.x * PIX_PER_WG;
    const RayLanes L(P.n_spec, P.n_diff, P.npix, wg_pix0);
    const int lp0 = L.lp0, r = L.r, wg_valid = L.wg_valid;
    const int R = P.n_spec + P.n_diff;
    const long wg_n0 = wg_pix0 / P.hw;
    const int wg_rem0 = (int)(wg_pix0 - wg_n0 * P.hw);
    extern __shared__ __attribute__((aligned(16))) float rt_smem[];
    const int ni_need = P.ni_need;
    float* s_raw = rt_smem;                                 // [PIX_PER_WG][c_out_pad]
    float* s_ni = s_raw + PIX_PER_WG * P.c_out_pad;         // [PIX_PER_WG][ni_need]
    float* s_uv = s_ni + PIX_PER_WG * ni_need;              // [PIX_PER_WG][2 R]
    float* s_lt = s_uv + PIX_PER_WG * 2 * R;                // [3 R][LT_ROW]
    float al[RR_PIX];
    L.load_alpha(P.alpha + wg_pix0, al);
    {
        const int q_raw = P.c_out_pad >> 2;
        const float4* g_raw = reinterpret_cast<const float4*>(P.unet_raw + wg_pix0 * P.c_out_pad);
        for (int i = threadIdx.x; i < wg_valid * q_raw; i += 256) reinterpret_cast<float4*>(s_raw)[i] = g_raw[i];
        L.stage_net_in(s_ni, P.net_in + wg_pix0 * P.c_pad, P.c_pad, ni_need);
    }
    __syncthreads();
    float b[3] = {0.f, 0.f, 0.f};
    if (L.ray_live) { b[0] = P.bias[3 * r + 0]; b[1] = P.bias[3 * r + 1]; b[2] = P.bias[3 * r + 2]; }
#pragma unroll
    for (int k = 0; k < RR_PIX; k++) {
        if (lp0 + k >= wg_valid || !L.ray_live) continue;
        const float* d = s_ni + __mul24(lp0 + k, ni_need) + 3 * r;
        const float* yr = s_raw + __mul24(lp0 + k, P.c_out_pad) + 3 * r;
        float u, v;
        ray_uv<TrigPoly>(f3(d[0], d[1], d[2]), al[k], u, v);
        const bool bg = al[k] == 0.0f;
        float* uv = s_uv + __mul24(lp0 + k, 2 * R);
        uv[r] = bg ? -1.0f : u;
        uv[R + r] = bg ? -1.0f : v;
#pragma unroll
        for (int c = 0; c < 3; c++) s_lt[(3 * r + c) * LT_ROW + lp0 + k] = bg ? 0.0f : fast_tanh_plus1f(yr[c] + b[c]);
    }
    __syncthreads();
    {
        float* dst = P.rays_uv + wg_pix0 * 2 * R;
        for (int i = threadIdx.x; i < wg_valid * 2 * R; i += 256) dst[i] = s_uv[i];
    }
    // planes: item (row j, pixel px); rows 0 .. 3R-1 are rays_lt's (ray, channel) planes, then the two albedos' channels
    for (int i = threadIdx.x; i < (3 * R + 6) * PIX_PER_WG; i += 256) {
        const int px = i & (PIX_PER_WG - 1), j = i / PIX_PER_WG;
        if (px >= wg_valid) continue;
        int rem;
        long n;
        view_offset(wg_n0, wg_rem0 + px, P.hw, n, rem);
        if (j < 3 * R) {
            P.rays_lt[(n * 3 * R + j) * P.hw + rem] = s_lt[j * LT_ROW + px];
        } else {
            const int a = j - 3 * R, c = a % 3;
            const float* ni = s_ni + __mul24(px, ni_need) + 3 * R + 6;
            if (a < 3) P.alb_spec[(n * 3 + c) * P.hw + rem] = ni[P.alb_spec_ch + c];
            else P.alb_diff[(n * 3 + c) * P.hw + rem] = ni[P.alb_diff_ch + c];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Presenter: the float frame [N,3,H,W] as the 8-bit channel-last image cv2.imwrite makes of it (test_rnr.py:377), composited
// over the light-probe background of test_rnr.py:386-391 where the mesh is not.  One launch behind the ray stage instead of
// get_view_dir_map, spherical_mapping_batch, the Interpolater, a where, x255, round, clamp, cast and a channel flip.
// PIX = 4: a thread owns four consecutive pixels of the flat [N H W] index (H W a multiple of 4, so they share a view, but
// they may straddle a row: row and column are walked per pixel), reads its planes as three float4 and writes 12 bytes as
// three dwords.  PIX = 1: one pixel, three byte stores (any H W, any alignment of out).  Memory-bound on foreground pixels
// (12 + 4 bytes in, 3 out), transcendental-bound on background pixels, whose colour is computed only where it is shown:
// polynomial atan2 / acos, v_rsq normalisation and the FMA blend, as ray_render_kernel uses for its taps.
// ------------------------------------------------------------------------------------------------
struct PresentParams {
    const float* image; const float* alpha;
    const float* proj_inv; const float* R_inv;
    const float* lp; int lp_h, lp_w;
    int mode, rgb;
    uint8_t* out;
    long npix; int H, W;
};

template <int PIX>      // 4 or 1
__global__ void __launch_bounds__(256)
present_u8_kernel(const PresentParams P) {
    const long pix0 = ((long)blockIdx.x * 256 + threadIdx.x) * PIX;
    if (pix0 >= P.npix) return;
    const int hw = P.H * P.W;
    const int n = (int)(pix0 / hw);
    const int rem0 = (int)(pix0 - (long)n * hw);
    float c[3][PIX];
    bool bg[PIX];
#pragma unroll
    for (int k = 0; k < PIX; k++) bg[k] = P.mode == RNR_PRESENT_BACKGROUND;
    if (P.mode != RNR_PRESENT_BACKGROUND) {
        const float* plane = P.image + (long)n * 3 * hw + rem0;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            if constexpr (PIX == 4) {
                const float4 v = *reinterpret_cast<const float4*>(plane + (long)ch * hw);
                c[ch][0] = v.x; c[ch][1] = v.y; c[ch][2] = v.z; c[ch][3] = v.w;
            } else {
                c[ch][0] = plane[(long)ch * hw];
            }
        }
        if (P.mode == RNR_PRESENT_COMPOSITE) {
            float a[PIX];
            if constexpr (PIX == 4) {
                const float4 v = *reinterpret_cast<const float4*>(P.alpha + pix0);
                a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
            } else {
                a[0] = P.alpha[pix0];
            }
#pragma unroll
            for (int k = 0; k < PIX; k++) bg[k] = !(a[k] > 0.0f);
        }
    }
    int row = rem0 / P.W, col = rem0 - row * P.W;
#pragma unroll
    for (int k = 0; k < PIX; k++) {
        if (bg[k]) background_colour<NormFast, TrigPoly, true>(P.proj_inv, P.R_inv, P.lp, P.lp_h, P.lp_w, n, row, col, c[0][k], c[1][k], c[2][k]);
        if (++col == P.W) { col = 0; row++; }
    }
    // byte j of a pixel is channel 2 - j (cv2's B, G, R) or channel j (RNR_PRESENT_RGB)
    unsigned b[3 * PIX];
#pragma unroll
    for (int k = 0; k < PIX; k++) {
        const unsigned q0 = quantise_u8(c[0][k]), q1 = quantise_u8(c[1][k]), q2 = quantise_u8(c[2][k]);
        b[3 * k + 0] = P.rgb ? q0 : q2;
        b[3 * k + 1] = q1;
        b[3 * k + 2] = P.rgb ? q2 : q0;
    }
    uint8_t* o = P.out + pix0 * 3;
    if constexpr (PIX == 4) {
        unsigned* o4 = reinterpret_cast<unsigned*>(o);      // 12 bytes per thread, 4-byte aligned (rnr_present_u8 checks out)
#pragma unroll
        for (int w = 0; w < 3; w++) o4[w] = b[4 * w] | (b[4 * w + 1] << 8) | (b[4 * w + 2] << 16) | (b[4 * w + 3] << 24);
    } else {
        o[0] = (uint8_t)b[0]; o[1] = (uint8_t)b[1]; o[2] = (uint8_t)b[2];
    }
}

// ------------------------------------------------------------------------------------------------
// spherical harmonics, float64 internally like the reference's numpy/pyshtools path
// ------------------------------------------------------------------------------------------------
constexpr int SH_LMAX_MAX = 16;

__global__ void __launch_bounds__(128)
sh_basis_kernel(const float* __restrict__ dirs, float* __restrict__ out, int n, int lmax) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = dirs[i * 3 + 0], y = dirs[i * 3 + 1], z = dirs[i * 3 + 2];
    // sph_harm.py:14-15, 54-57: azimuth = atan2(y,x); colatitude = pi/2 - atan2(z, sqrt(x^2+y^2))
    const double rho = sqrt(x * x + y * y);
    const double phi = atan2(y, x);
    const double rr = sqrt(rho * rho + z * z);
    const double ct = rr > 0.0 ? z / rr : 1.0, st = rr > 0.0 ? rho / rr : 0.0;
    const int nb = (lmax + 1) * (lmax + 1);
    float* o = out + (size_t)i * nb;
    const double fourpi = 12.566370614359172;
    // P_m^m upward in m; for each m run the l-recurrence and emit columns (l, +m) and (l, -m)
    double pmm = 1.0;
    for (int m = 0; m <= lmax; m++) {
        if (m > 0) pmm *= (2 * m - 1) * st;      // no Condon-Shortley phase
        const double cm = cos(m * phi), sm = sin(m * phi);
        double p_lm2 = 0.0, p_lm1 = 0.0;
        for (int l = m; l <= lmax; l++) {
            double p;
            if (l == m) p = pmm;
            else if (l == m + 1) p = ct * (2 * m + 1) * pmm;
            else p = ((2 * l - 1) * ct * p_lm1 - (l + m - 1) * p_lm2) / (l - m);
            p_lm2 = p_lm1; p_lm1 = p;
            // (l-m)!/(l+m)!
            double ratio = 1.0;
            for (int k = l - m + 1; k <= l + m; k++) ratio /= (double)k;
            const double norm = sqrt((m == 0 ? 1.0 : 2.0) * (2 * l + 1) / fourpi * ratio);
            const int base = l * l + l;          // column of (l, 0)
            o[base + m] = (float)(norm * p * cm);
            if (m > 0) o[base - m] = (float)(norm * p * sm);
        }
    }
}

// out[s,c] = sum_b basis[s,b] * coeff[b,c].  64 samples per workgroup: their basis rows are one contiguous block of
// 64*nb floats, staged through LDS with coalesced loads (a lane-per-output version reads rows nb floats apart).
constexpr int SHR_ROWS = 64;
__device__ __forceinline__ void sh_reconstruct_block(int block, float* sh_lds, const float* __restrict__ basis,
                                                     const float* __restrict__ coeff, float* __restrict__ out, int ns, int nb, int nc) {
    float* bl = sh_lds;                             // [SHR_ROWS*nb] basis rows, then [nb*nc] coefficients
    float* cl = sh_lds + SHR_ROWS * nb;
    const int s0 = block * SHR_ROWS;
    const int rows = min(SHR_ROWS, ns - s0);
    for (int i = threadIdx.x; i < rows * nb; i += blockDim.x) bl[i] = basis[(size_t)s0 * nb + i];
    for (int i = threadIdx.x; i < nb * nc; i += blockDim.x) cl[i] = coeff[i];
    __syncthreads();
    for (int o = threadIdx.x; o < rows * nc; o += blockDim.x) {
        const int s = o / nc, c = o - s * nc;
        float acc = 0.f;
        for (int b = 0; b < nb; b++) acc += bl[s * nb + b] * cl[b * nc + c];
        out[(size_t)(s0 + s) * nc + c] = acc;
    }
}

__global__ void __launch_bounds__(256)
sh_reconstruct_kernel(const float* __restrict__ basis, const float* __restrict__ coeff, float* __restrict__ out,
                      int ns, int nb, int nc) {
    extern __shared__ float sh_lds[];
    sh_reconstruct_block(blockIdx.x, sh_lds, basis, coeff, out, ns, nb, nc);
}

// ------------------------------------------------------------------------------------------------
// rnr_frame_prepare: the per-call preliminaries of a frame batch in ONE launch (r04; at one view per call they were six
// launches of ~5 us each in front of a 2.5 ms frame): block ranges of one grid run
//   [0, b_proj)            vertex projection straight from the [N,4,4] poses (no R / t copies);
//   [b_proj, b_tan)        per-face tangents, recomputed per call as render.get_TBN_map does (render.py:135-150);
//   [b_tan, b_lp)          the light probe reconstructed from SH coefficients (LightingSH.reconstruct_lp, network.py:622-627);
//   [b_lp, b_clear)        the per-call clearing of the rasterizer workspace (tile counters 0, depth keys ~0).
// The parts are independent of each other; each runs the code of its stand-alone kernel (same bits).
struct FramePrepParams {
    rnr_mesh mesh;
    const float* K; const float* pose; float* v_uvz; int nviews; float orig_size, eps;
    float* tangents;
    const float* lp_basis; const float* lp_coeff; float* lp_out; int lp_ns, lp_nb, lp_nc;
    uint4* counters; long counter_vec; uint4* keys; long key_vec;
    int b_proj, b_tan, b_lp, b_clear;
};
__global__ void __launch_bounds__(256)
frame_prepare_kernel(const FramePrepParams P) {
    extern __shared__ float sh_lds[];
    const int b = blockIdx.x;
    if (b < P.b_proj) {
        project_vertex<true>((long)b * 256 + threadIdx.x, P.mesh.v, P.K, P.pose, nullptr, nullptr, nullptr, nullptr, P.v_uvz,
                             P.nviews, P.mesh.num_vertices, P.orig_size, P.eps);
    } else if (b < P.b_tan) {
        face_tangent((b - P.b_proj) * 256 + threadIdx.x, P.mesh, P.tangents);
    } else if (b < P.b_lp) {
        sh_reconstruct_block(b - P.b_tan, sh_lds, P.lp_basis, P.lp_coeff, P.lp_out, P.lp_ns, P.lp_nb, P.lp_nc);
    } else {
        const long i = (long)(b - P.b_lp) * 256 + threadIdx.x;
        if (i < P.counter_vec) P.counters[i] = make_uint4(0u, 0u, 0u, 0u);
        else if (i - P.counter_vec < P.key_vec) P.keys[i - P.counter_vec] = make_uint4(~0u, ~0u, ~0u, ~0u);
    }
}

// FIT: the uniform-quadrature projection of sph_harm.fit_sh_coeff (factor 4 pi / ns).  !FIT: the bare sum, which is the
// adjoint of sh_reconstruct_kernel in the coefficients (rnr_sh_reconstruct_backward: samples = the upstream gradient)
template <bool FIT>
__global__ void __launch_bounds__(256)
sh_fit_kernel(const float* __restrict__ samples, const float* __restrict__ basis, float* __restrict__ out,
              int ns, int nb, int nc) {
    __shared__ float red[256];
    const int o = blockIdx.x;            // output (b, c)
    const int b = o / nc, c = o % nc;
    float acc = 0.f;
    for (int s = threadIdx.x; s < ns; s += blockDim.x) acc += samples[(size_t)s * nc + c] * basis[(size_t)s * nb + b];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[o] = FIT ? red[0] * (4.0f * RNR_PI_F / (float)ns) : red[0];
}

__global__ void __launch_bounds__(256)
interpolate_bilinear_kernel(const float* __restrict__ data, int h, int w, int c, const float* __restrict__ x,
                            const float* __restrict__ y, float* __restrict__ out, int32_t* __restrict__ taps, int n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)n * c) return;
    const int s = (int)(i / c), ch = (int)(i % c);
    const Taps t = bilinear_taps(x[s], y[s], w, h);
    out[i] = t.blend(data[((size_t)t.y0 * w + t.x0) * c + ch], data[((size_t)t.y1 * w + t.x0) * c + ch],
                     data[((size_t)t.y0 * w + t.x1) * c + ch], data[((size_t)t.y1 * w + t.x1) * c + ch]);
    if (taps && ch == 0) {
        taps[s * 4 + 0] = t.x0; taps[s * 4 + 1] = t.y0; taps[s * 4 + 2] = t.x1; taps[s * 4 + 3] = t.y1;
    }
}

// ------------------------------------------------------------------------------------------------
// Stand-alone operator kernels for the drop-in Python API (network.py / render.py / camera.py functions called one
// at a time).  The fused pipeline does not use them: shade_inputs_kernel / ray_render_kernel compute the same
// quantities without the HBM round trips.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
view_dir_map_kernel(const float* __restrict__ proj_inv, const float* __restrict__ R_inv, float* __restrict__ out_world,
                    float* __restrict__ out_cam, long npix, int H, int W) {
    const long pix = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= npix) return;
    int n, row, col;
    pixel_coords(pix, H, W, n, row, col);
    float3 dc, vd;
    view_dir<NormExact>(proj_inv, R_inv, n, row, col, dc, vd);
    out_world[pix * 3 + 0] = vd.x; out_world[pix * 3 + 1] = vd.y; out_world[pix * 3 + 2] = vd.z;
    if (out_cam) { out_cam[pix * 3 + 0] = dc.x; out_cam[pix * 3 + 1] = dc.y; out_cam[pix * 3 + 2] = dc.z; }
}

// test_rnr.py:386-391 for one probe: the background the object stands in front of, [N,H,W,3] float32.  The directions are
// the bits view_dir_map_kernel writes (same view_dir<NormExact>), the mapping ocml's in the reference's operation order
__global__ void __launch_bounds__(256)
env_background_kernel(const float* __restrict__ proj_inv, const float* __restrict__ R_inv, const float* __restrict__ lp,
                      int lp_n, int lp_h, int lp_w, float* __restrict__ out, long npix, int H, int W) {
    const long pix = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= npix) return;
    int n, row, col;
    pixel_coords(pix, H, W, n, row, col);
    const float* lpn = lp + (lp_n == 1 ? 0 : (size_t)n * lp_h * lp_w * 3);
    float c0, c1, c2;
    background_colour<NormExact, TrigOcml, false>(proj_inv, R_inv, lpn, lp_h, lp_w, n, row, col, c0, c1, c2);
    out[pix * 3 + 0] = c0; out[pix * 3 + 1] = c1; out[pix * 3 + 2] = c2;
}

__global__ void __launch_bounds__(256)
tbn_map_kernel(const float* __restrict__ normal_map, const int32_t* __restrict__ face_index_map,
               const float* __restrict__ tangents, int num_faces, float* __restrict__ out, long npix) {
    const long pix = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= npix) return;
    const int fi = wrap_face_index(face_index_map[pix], num_faces);
    const float3 tg = f3(tangents[fi * 3 + 0], tangents[fi * 3 + 1], tangents[fi * 3 + 2]);
    float3 tt, bt, nm;
    tbn_frame<NormExact>(f3(normal_map[pix * 3 + 0], normal_map[pix * 3 + 1], normal_map[pix * 3 + 2]), tg, tt, bt, nm);
    float* o = out + pix * 9;      // [3,3] row-major, columns (T, B, N)  (render.py:164)
    o[0] = tt.x; o[1] = bt.x; o[2] = nm.x;
    o[3] = tt.y; o[4] = bt.y; o[5] = nm.y;
    o[6] = tt.z; o[7] = bt.z; o[8] = nm.z;
}

struct RaySamplerParams {
    const float* tbn; const float* view_tangent; const float* alpha;
    float* rays_dir; float* rays_uv; float* rays_dir_tangent;
    float piv[MAX_RAYS * 3];
    int n_rays, reflect;
    long npix;
};

__global__ void __launch_bounds__(256)
ray_sampler_kernel(const RaySamplerParams P) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.npix * P.n_rays) return;
    const long pix = i / P.n_rays;
    const int r = (int)(i % P.n_rays);
    const float* M = P.tbn + pix * 9;
    const float a = P.alpha[pix];
    const float3 pv = f3(P.piv[r * 3 + 0], P.piv[r * 3 + 1], P.piv[r * 3 + 2]);
    float3 lt;
    if (P.reflect) {
        lt = reflect_ray<NormExact>(pv, f3(P.view_tangent[pix * 3 + 0], P.view_tangent[pix * 3 + 1], P.view_tangent[pix * 3 + 2]), a);
    } else {
        lt = pv;
    }
    // the stored 3x3 is row-major with columns (T, B, N): row i of M . lt is the sum tbn_ray writes column-wise
    const float3 d = tbn_ray<NormExact>(f3(M[0], M[3], M[6]), f3(M[1], M[4], M[7]), f3(M[2], M[5], M[8]), lt);
    const int R = P.n_rays;
    P.rays_dir[(pix * 3 + 0) * R + r] = d.x;
    P.rays_dir[(pix * 3 + 1) * R + r] = d.y;
    P.rays_dir[(pix * 3 + 2) * R + r] = d.z;
    if (P.rays_dir_tangent) {
        P.rays_dir_tangent[(pix * 3 + 0) * R + r] = lt.x;
        P.rays_dir_tangent[(pix * 3 + 1) * R + r] = lt.y;
        P.rays_dir_tangent[(pix * 3 + 2) * R + r] = lt.z;
    }
    float u, v;
    ray_uv<TrigOcml>(d, a, u, v);
    P.rays_uv[(pix * 2 + 0) * R + r] = u;
    P.rays_uv[(pix * 2 + 1) * R + r] = v;
}

struct TexMapCommon {                         // what texture_mapper_kernel and its adjoint both take
    const float* uv_map; const float* sh;   // sh may be NULL
    int tex_size[MAX_LEVELS], num_levels, C, sh_start;
    long npix; int hw;
};
struct TexMapParams : TexMapCommon {
    const float* tex[MAX_LEVELS];
    float* out;                              // [N,C,H,W]
};

// val times the factor f_c of channel c at batch pixel pix: the SH basis value sh[pix, c - sh_start] on the nine SH channels,
// else 1 (network.py:87-91); sh may be NULL.  The forward scales its sum with it, the adjoint the upstream gradient
__device__ __forceinline__ float sh_scaled(const float* sh, int sh_start, long pix, int c, float val) {
    return (sh && c >= sh_start && c < sh_start + 9) ? val * sh[pix * 9 + (c - sh_start)] : val;
}

// any channel count (DNR uses C = 30): one lane per (channel, pixel), pixel fastest so the NCHW store coalesces
__global__ void __launch_bounds__(256)
texture_mapper_kernel(const TexMapParams P) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.npix * P.C) return;
    long n, p, pix; int c;
    element_coords(i, P.C, P.hw, n, c, p, pix);
    const float u = P.uv_map[pix * 2 + 0], v = P.uv_map[pix * 2 + 1];
    float acc = 0.f;
    for (int l = 0; l < P.num_levels; l++) {
        const int s = P.tex_size[l];
        const Taps t = level_taps(u, v, s);
        const float* tex = P.tex[l] + c;
        const float lv = t.blend(tex[t.texel<size_t>(0, s, P.C)], tex[t.texel<size_t>(1, s, P.C)], tex[t.texel<size_t>(2, s, P.C)],
                                 tex[t.texel<size_t>(3, s, P.C)]);
        acc = (l == 0) ? lv : acc + lv;
    }
    P.out[i] = sh_scaled(P.sh, P.sh_start, pix, c, acc);
}

// ------------------------------------------------------------------------------------------------
// Adjoint of texture_mapper_kernel in the textures (rnr_texture_mapper_backward).  The forward is linear in them:
//     out[n,c,p] = f_c(n,p) sum_levels sum_taps w T_l[y, x, c],    f_c = sh[n,p,c - sh_start] on the nine SH channels, else 1
// so with gf = g[n,c,p] * f_c(n,p) every tap adds gf * w (in that product order) to grad_T_l[y, x, c]; no texture value is read.
// Taps, weights, offsets and f_c are the forward's own (level_taps, texel_offset, sh_scaled): same clamped indices, so no address
// leaves a level whatever uv_map holds, and the same weight bits.  A contribution whose weight or whose gf is 0 is never added
// (texbwd_scatter_tap, texbwd_idle: out-of-range uv, background pixels under a masked loss, -0); the entry point clears every
// level first, so untouched texels hold exactly 0.  Lanes are (pixel, channel) with the channel fastest in both forms: one wave
// instruction adds to whole texel records (64 / C texels of 4 C contiguous bytes).  Texel offsets are 64-bit.
// ------------------------------------------------------------------------------------------------
struct TexMapBwdParams : TexMapCommon {
    const float* g;                          // grad_out [N,C,H,W]
    float* grad[MAX_LEVELS];                 // [S_l,S_l,C] each, cleared by the entry point
    int H, W;
};

// gf of channel c at pixel p of view n
__device__ __forceinline__ float texbwd_gf(const TexMapBwdParams& P, long n, long p, int c) {
    return sh_scaled(P.sh, P.sh_start, n * P.hw + p, c, P.g[(n * P.C + c) * P.hw + p]);
}
// a lane whose gf is 0 adds nothing, and a wave none of whose lanes has anything skips together
__device__ __forceinline__ bool texbwd_idle(float gf) { return __ballot(gf != 0.0f) == 0ull || gf == 0.0f; }
// tap j of t adds gf * w to its texel of channel plane level_c of a level of size s, unless its weight is 0
__device__ __forceinline__ void texbwd_scatter_tap(float* level_c, int s, int C, const Taps& t, int j, float gf) {
    if (t.w(j) != 0.0f) atomicAdd(level_c + t.texel<size_t>(j, s, C), gf * t.w(j));
}

constexpr int TB_PIX = 64;      // form A: pixels per workgroup
constexpr int TB_CH = 64;       //         channels per pass through the LDS tile

// Form A, any shape: 64 consecutive pixels per workgroup.  grad_out is NCHW, so a pass stages gf of 64 pixels x up to 64 channels
// through LDS (read along the pixels of a channel, row stride 65) and then walks the tile with the channel fastest; one global
// atomicAdd per tap and channel.
__global__ void __launch_bounds__(256)
texture_mapper_bwd_kernel(const TexMapBwdParams P) {
    __shared__ float gf_sm[TB_PIX * (TB_CH + 1)];
    __shared__ float uv_sm[TB_PIX * 2];
    const long pix0 = (long)blockIdx.x * TB_PIX;
    const int valid = (int)min((long)TB_PIX, P.npix - pix0);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if ((int)threadIdx.x < valid * 2) uv_sm[threadIdx.x] = P.uv_map[pix0 * 2 + threadIdx.x];
    const bool live = lane < valid;
    const long n = live ? (pix0 + lane) / P.hw : 0, p = live ? (pix0 + lane) % P.hw : 0;
    for (int c0 = 0; c0 < P.C; c0 += TB_CH) {
        const int cw = min(TB_CH, P.C - c0);
        __syncthreads();        // the previous pass has been read (first pass: uv_sm is written)
        for (int ch = wv; ch < cw; ch += 4) gf_sm[lane * (TB_CH + 1) + ch] = live ? texbwd_gf(P, n, p, c0 + ch) : 0.0f;
        __syncthreads();
        for (int i = threadIdx.x; i < valid * cw; i += 256) {
            const int px = i / cw, ch = i - px * cw;
            const float gf = gf_sm[px * (TB_CH + 1) + ch];
            if (texbwd_idle(gf)) continue;
            const float u = uv_sm[px * 2 + 0], v = uv_sm[px * 2 + 1];
            for (int l = 0; l < P.num_levels; l++) {
                const int s = P.tex_size[l];
                const Taps t = level_taps(u, v, s);
#pragma unroll
                for (int j = 0; j < 4; j++) texbwd_scatter_tap(P.grad[l] + c0 + ch, s, P.C, t, j, gf);
            }
        }
    }
}

constexpr int TT = 16;          // form B: the workgroup's image tile is TT x TT pixels, one thread per pixel
constexpr int TT_CH = 16;       //         channels per pass
constexpr int TT_BOX = 8192;    //         floats of the LDS accumulator (32 KB): 512 texels of 16 channels

// Form B, the tile form.  Per pass of up to 16 channels the workgroup stages gf of its 16 x 16 pixels; per level every thread
// writes its pixel's taps to LDS and the workgroup reduces the bounding box of the texels its live pixels touch (live: some gf
// != 0 and some weight != 0).  When box x channels fits TT_BOX floats the whole footprint is accumulated there with LDS float
// adds and each non-zero entry is flushed with ONE global atomicAdd; when it does not (a uv seam, a silhouette, random uv) a
// box of that capacity is laid around the texel of the tile's first live pixel and the taps outside it go straight to global
// atomics.  LDS: 17 KB gf + 8 KB taps + 32 KB box = 57 KB, two workgroups per CU.
__global__ void __launch_bounds__(256)
texture_mapper_bwd_tile_kernel(const TexMapBwdParams P, int tiles_x, int tiles_y) {
    __shared__ float gf_sm[TT * TT * (TT_CH + 1)];
    __shared__ int4 tap_xy[TT * TT];
    __shared__ float4 tap_w[TT * TT];
    __shared__ float box_sm[TT_BOX];
    __shared__ int red_sm[5];           // min x0, min y0, max x1, max y1 over the live pixels, and the first live thread
    const int t = threadIdx.x, lane = t & 63;
    const int tile = blockIdx.x % (tiles_x * tiles_y);
    const long n = blockIdx.x / (tiles_x * tiles_y);
    const int row = (tile / tiles_x) * TT + t / TT, col = (tile % tiles_x) * TT + t % TT;
    const bool inimg = row < P.H && col < P.W;
    const long p = inimg ? (long)row * P.W + col : 0;
    const float u = inimg ? P.uv_map[(n * P.hw + p) * 2 + 0] : 0.0f, v = inimg ? P.uv_map[(n * P.hw + p) * 2 + 1] : 0.0f;
    for (int c0 = 0; c0 < P.C; c0 += TT_CH) {
        const int cw = min(TT_CH, P.C - c0);
        const int cap = TT_BOX / cw;                    // texels the box can hold
        bool any = false;
        __syncthreads();        // the previous pass has been read
        for (int ch = 0; ch < cw; ch++) {
            const float gf = inimg ? texbwd_gf(P, n, p, c0 + ch) : 0.0f;
            gf_sm[t * (TT_CH + 1) + ch] = gf;
            any = any || gf != 0.0f;
        }
        if (!__syncthreads_or(any)) continue;           // nothing to add from this tile and these channels
        for (int l = 0; l < P.num_levels; l++) {
            const int s = P.tex_size[l];
            const Taps tp = level_taps(u, v, s);
            const bool live = any && (tp.w00 != 0.0f || tp.w10 != 0.0f || tp.w01 != 0.0f || tp.w11 != 0.0f);
            __syncthreads();    // the previous level's taps, box and bounds have been read
            if (t < 4) red_sm[t] = t < 2 ? 0x7fffffff : -1;
            if (t == 4) red_sm[4] = 0x7fffffff;
            tap_xy[t] = make_int4(tp.x0, tp.y0, tp.x1, tp.y1);
            tap_w[t] = make_float4(tp.w00, tp.w10, tp.w01, tp.w11);
            int mnx = live ? tp.x0 : 0x7fffffff, mny = live ? tp.y0 : 0x7fffffff, mxx = live ? tp.x1 : -1, mxy = live ? tp.y1 : -1;
            int first = live ? t : 0x7fffffff;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                mnx = min(mnx, __shfl_xor(mnx, d, 64)); mny = min(mny, __shfl_xor(mny, d, 64));
                mxx = max(mxx, __shfl_xor(mxx, d, 64)); mxy = max(mxy, __shfl_xor(mxy, d, 64));
                first = min(first, __shfl_xor(first, d, 64));
            }
            __syncthreads();    // red_sm is initialised
            if (lane == 0 && first != 0x7fffffff) {
                atomicMin(&red_sm[0], mnx); atomicMin(&red_sm[1], mny);
                atomicMax(&red_sm[2], mxx); atomicMax(&red_sm[3], mxy);
                atomicMin(&red_sm[4], first);
            }
            __syncthreads();
            const int anchor = red_sm[4];
            if (anchor == 0x7fffffff) continue;         // no live pixel on this level (every uv out of range)
            int bx0 = red_sm[0], by0 = red_sm[1];
            int bw = red_sm[2] - bx0 + 1, bh = red_sm[3] - by0 + 1;
            if (bw > cap / bh) {                        // does not fit: a box of the capacity around the anchor's texel
                const int ex = bx0 + bw, ey = by0 + bh; // one past the footprint
                int side = (int)sqrtf((float)cap);
                while (side * side > cap) side--;
                bw = min(bw, side);
                bh = min(bh, cap / bw);
                bw = min(ex - bx0, cap / bh);
                const int4 a = tap_xy[anchor];
                bx0 = min(max(a.x - bw / 2, bx0), ex - bw);
                by0 = min(max(a.y - bh / 2, by0), ey - bh);
            }
            const int nbox = bw * bh * cw;
            for (int i = t; i < nbox; i += 256) box_sm[i] = 0.0f;
            __syncthreads();
            float* gl = P.grad[l] + c0;
            for (int i = t; i < TT * TT * cw; i += 256) {       // cw rounds for every thread
                const int px = i / cw, ch = i - px * cw;
                const float gf = gf_sm[px * (TT_CH + 1) + ch];
                if (texbwd_idle(gf)) continue;
                const int4 xy = tap_xy[px];
                const float4 w = tap_w[px];
                const Taps tq = {xy.x, xy.y, xy.z, xy.w, w.x, w.y, w.z, w.w};
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int rx = tq.x(j) - bx0, ry = tq.y(j) - by0;
                    if (tq.w(j) != 0.0f && (unsigned)rx < (unsigned)bw && (unsigned)ry < (unsigned)bh)
                        atomicAdd(&box_sm[(ry * bw + rx) * cw + ch], gf * tq.w(j));
                    else
                        texbwd_scatter_tap(gl + ch, s, P.C, tq, j, gf);     // outside the box (or weight 0: nothing)
                }
            }
            __syncthreads();
            for (int i = t; i < nbox; i += 256) {
                const float val = box_sm[i];
                if (val == 0.0f) continue;
                const int q = i / cw, ch = i - q * cw;
                const int ry = q / bw, rx = q - ry * bw;
                atomicAdd(gl + texel_offset<size_t>(bx0 + rx, by0 + ry, s, P.C) + ch, val);
            }
        }
    }
}

// RayRenderer.forward with API-shaped inputs (network.py:481-527): one lane per (pixel, channel)
struct RayApiParams {
    const float* rays_uv;    // [N,H,W,2,R]
    const float* rays_lt;    // [N,R,C,H,W]
    const float* lp;         // [Nl,Hl,Wl,C], Nl = 1 or N
    const float* alb_spec;   // [N,C,H,W]
    const float* alb_diff;   // [N,C,H,W] or NULL
    int lp_n, lp_h, lp_w, C, R, n_diff, no_albedo, separate;
    float lp_scale;
    float* out; float* out_spec; float* out_diff; float* ltt_spec; float* ltt_diff; float* rays_color;  // last may be NULL
    long npix; int hw;
};

// The group rule of RayRenderer.forward (network.py:505-527), for the forward and its adjoint: the first R - n_diff rays are specular,
// the rest diffuse; without diffuse rays the diffuse outputs are constants (0, no gradient); the diffuse group is multiplied by its
// own albedo map only when asked and given one, else by the specular map
__device__ __forceinline__ int ray_n_spec(const RayApiParams& P) { return P.R - P.n_diff; }
__device__ __forceinline__ bool ray_has_diffuse(const RayApiParams& P) { return P.n_diff > 0; }
__device__ __forceinline__ bool ray_own_diffuse_albedo(const RayApiParams& P) { return P.separate && P.alb_diff; }
// s / ray count of each group: the means of the forward's sums, and of the adjoint's group gradients per ray
__device__ __forceinline__ void ray_group_means(const RayApiParams& P, float s_spec, float s_diff, float& m_spec, float& m_diff) {
    m_spec = s_spec / (float)ray_n_spec(P);
    m_diff = ray_has_diffuse(P) ? s_diff / (float)P.n_diff : 0.0f;
}
// the albedo each group is multiplied by at output element i (1 with no_albedo: the product is then exact)
__device__ __forceinline__ void ray_group_albedo(const RayApiParams& P, long i, float& as, float& ad) {
    as = P.no_albedo ? 1.0f : P.alb_spec[i];
    ad = P.no_albedo ? 1.0f : (ray_own_diffuse_albedo(P) ? P.alb_diff[i] : as);
}

// output element i = (n, c, pixel) from its sums over the specular and the diffuse rays: the group rule, then the five stores
__device__ __forceinline__ void finish_ray_api(const RayApiParams& P, long i, float s_spec, float s_diff) {
    float ls, ld, as, ad;
    ray_group_means(P, s_spec, s_diff, ls, ld);
    ray_group_albedo(P, i, as, ad);
    const float os = as * ls, od = ray_has_diffuse(P) ? ad * ld : 0.0f;
    P.out[i] = os + od;
    if (P.out_spec) P.out_spec[i] = os;
    if (P.out_diff) P.out_diff[i] = od;
    if (P.ltt_spec) P.ltt_spec[i] = ls;
    if (P.ltt_diff) P.ltt_diff[i] = ld;
}

__global__ void __launch_bounds__(256)
ray_renderer_api_kernel(const RayApiParams P) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;     // over N*C*hw
    if (i >= P.npix * P.C) return;
    long n, p, pix; int c;
    element_coords(i, P.C, P.hw, n, c, p, pix);
    const int n_spec = ray_n_spec(P);
    const float* lp = P.lp + (P.lp_n == 1 ? 0 : (size_t)n * P.lp_h * P.lp_w * P.C);
    float ss = 0.f, sd = 0.f;
    for (int r = 0; r < P.R; r++) {
        const float u = P.rays_uv[(pix * 2 + 0) * P.R + r], v = P.rays_uv[(pix * 2 + 1) * P.R + r];
        const Taps t = envmap_taps(u, v, P.lp_w, P.lp_h);
        const float col = probe_colour<size_t>(t, lp + c, P.lp_w, P.C, P.lp_scale);
        const size_t li = (((size_t)n * P.R + r) * P.C + c) * P.hw + p;
        if (P.rays_color) P.rays_color[li] = col;
        const float prod = P.rays_lt[li] * col;
        if (r < n_spec) ss += prod; else sd += prod;
    }
    finish_ray_api(P, i, ss, sd);
}

// ---- the tiled form of the operator and of its adjoint: one layout for both kernels and for launch_ray_api on the host ----
constexpr int RA_PIX = 64;      // pixels per workgroup: a wave holds the tile's 64 pixels on one ray quarter
constexpr int RA_QTR = 4;       // ray quarters: thread (pixel lane, quarter q) takes the rays q, q + RA_QTR, ... of its pixel
constexpr int RA_CH = 4;        // channel limit: thread (lane, c = its quarter) finishes channel c of its pixel
constexpr int RA_MAX_RAYS = 64; // ray limit: the uv tile stays at 33 KB
static_assert(RA_PIX == 64 && RA_CH <= RA_QTR, "a wave per ray quarter, a quarter per channel");

struct RayTile {
    int lane, qtr, urow;        // pixel lane, ray quarter, row stride of the uv tile (2 R + 1: conflict-free)
    bool live; long n, p;       // whether the lane holds a pixel of the batch; its view and its pixel of the view (0 where not)
    // workgroup prologue: the uv rows of the tile's pixels go to sm; ends with a barrier
    __device__ __forceinline__ RayTile(const RayApiParams& P, float* sm) {
        const long pix0 = (long)blockIdx.x * RA_PIX;
        const int R = P.R, valid = (int)min((long)RA_PIX, P.npix - pix0);
        lane = threadIdx.x & (RA_PIX - 1); qtr = threadIdx.x / RA_PIX; urow = 2 * R + 1;
        for (int i = threadIdx.x; i < valid * 2 * R; i += RA_PIX * RA_QTR) {
            const int px = i / (2 * R), k = i - px * 2 * R;
            sm[px * urow + k] = P.rays_uv[pix0 * 2 * R + i];
        }
        __syncthreads();
        live = lane < valid;
        n = live ? (pix0 + lane) / P.hw : 0; p = live ? (pix0 + lane) % P.hw : 0;
    }
    // uv of ray r of the lane's pixel; a lane without a pixel gets the background's -1, which has no tap
    __device__ __forceinline__ float2 uv(const float* sm, int R, int r) const {
        return live ? make_float2(sm[lane * urow + r], sm[lane * urow + R + r]) : make_float2(-1.0f, -1.0f);
    }
    // workgroup epilogue: the quarters' partial sums meet in sm, which the uv tile has left, as [quarter][spec | diff][channel][lane];
    // a thread (lane, c = qtr) that finishes a channel gets true and the sums of channel c over all rays of its pixel
    __device__ __forceinline__ int slot(int q, int group, int c) const { return ((q * 2 + group) * RA_CH + c) * RA_PIX + lane; }
    __device__ __forceinline__ bool sums(float* sm, int C, const float (&ss)[RA_CH], const float (&sd)[RA_CH], float& s_spec, float& s_diff) const {
        __syncthreads();
#pragma unroll
        for (int c = 0; c < RA_CH; c++) { sm[slot(qtr, 0, c)] = ss[c]; sm[slot(qtr, 1, c)] = sd[c]; }
        __syncthreads();
        if (!live || qtr >= C) return false;
        s_spec = 0.f; s_diff = 0.f;
#pragma unroll
        for (int q = 0; q < RA_QTR; q++) { s_spec += sm[slot(q, 0, qtr)]; s_diff += sm[slot(q, 1, qtr)]; }
        return true;
    }
};

// The same operator for <= RA_CH colour channels (the repo's probes have 3) in the RayTile layout: the taps of a (pixel, ray) are
// computed once for ALL channels, rays_lt / rays_color are touched along the pixels (128-byte rows per wave instruction), the uv rows
// come through LDS.  Sums over the rays are four interleaved partial sums instead of one chain: <= 1e-6 from the
// one-thread-per-(channel, pixel) form above (which reads uv with a stride of 2 R floats and recomputes the taps per channel).
__global__ void __launch_bounds__(RA_PIX * RA_QTR)
ray_renderer_api_tiled_kernel(const RayApiParams P) {
    extern __shared__ float ra_sm[];
    const int R = P.R, C = P.C, n_spec = ray_n_spec(P);
    const RayTile T(P, ra_sm);
    const float* lp = P.lp + (P.lp_n == 1 ? 0 : (size_t)T.n * P.lp_h * P.lp_w * C);
    float ss[RA_CH] = {0.f, 0.f, 0.f, 0.f}, sd[RA_CH] = {0.f, 0.f, 0.f, 0.f};
    if (T.live) {
        for (int r = T.qtr; r < R; r += RA_QTR) {
            const float2 uv = T.uv(ra_sm, R, r);
            const Taps t = envmap_taps(uv.x, uv.y, P.lp_w, P.lp_h);
#pragma unroll
            for (int c = 0; c < RA_CH; c++) {
                if (c >= C) break;
                const float col = probe_colour<size_t>(t, lp + c, P.lp_w, C, P.lp_scale);
                const size_t li = (((size_t)T.n * R + r) * C + c) * P.hw + T.p;
                if (P.rays_color) P.rays_color[li] = col;
                const float prod = P.rays_lt[li] * col;
                if (r < n_spec) ss[c] += prod; else sd[c] += prod;
            }
        }
    }
    float s_spec, s_diff;
    if (T.sums(ra_sm, C, ss, sd, s_spec, s_diff)) finish_ray_api(P, (T.n * C + T.qtr) * P.hw + T.p, s_spec, s_diff);
}

// ------------------------------------------------------------------------------------------------
// Adjoint of the two kernels above (rnr_ray_renderer_backward).  With ns = R - n_diff and a_s, a_d the albedo each group is
// multiplied by (1 with no_albedo), for output element (n, c, p):
//     G_os = g_out + g_out_specular        G_ls = g_ltt_specular + G_os a_s
//     G_od = g_out + g_out_diffuse         G_ld = g_ltt_diffuse  + G_od a_d
// per ray r:  G_p = G_ls / ns (specular) or G_ld / n_diff (diffuse);  grad_rays_lt[r] = G_p colour_r;
//     G_col = g_rays_color[r] + G_p rays_lt[r];  each of the four taps adds G_col w_tap lp_scale_factor to grad_lp at its texel;
// grad_albedo = G_o ltt of its group (both groups onto the specular albedo when the diffuse group uses it too).
// Taps, offsets, colour and the group rule are the forward's own (envmap_taps, tap_offsets, probe_colour, ray_group_*): same
// indices, same bits.  The scatter is made of global float atomics (one per tap and channel, merged across a wave in the tiled
// form); a contribution whose weight or G_col is 0 is never added, so untouched texels keep the 0 the entry point cleared them to.
// ------------------------------------------------------------------------------------------------
struct RayApiBwdParams {
    RayApiParams F;         // the forward's operands (its output pointers are unused)
    const float *g_out, *g_out_spec, *g_out_diff, *g_ltt_spec, *g_ltt_diff;     // [N,C,H,W], NULL = zero
    const float* g_rays_color;                                                  // [N,R,C,H,W], NULL = zero
    float* grad_rays_lt;    // [N,R,C,H,W] or NULL
    float *grad_alb_spec, *grad_alb_diff;   // [N,C,H,W] or NULL
    float* grad_lp;         // [Nl,Hl,Wl,C] or NULL, cleared by the entry point
};

__device__ __forceinline__ float grad_or_zero(const float* g, size_t i) { return g ? g[i] : 0.0f; }
// the upstream gradients of output element i = (n, c, pixel) folded onto its two outputs and, per ray, onto its group means
__device__ __forceinline__ void ray_api_heads(const RayApiBwdParams& P, long i, float& G_os, float& G_od, float& gp_spec, float& gp_diff) {
    const RayApiParams& F = P.F;
    const bool diff = ray_has_diffuse(F);
    const float go = grad_or_zero(P.g_out, i);
    G_os = go + grad_or_zero(P.g_out_spec, i);
    G_od = diff ? go + grad_or_zero(P.g_out_diff, i) : 0.0f;
    float as, ad;
    ray_group_albedo(F, i, as, ad);
    const float G_ls = grad_or_zero(P.g_ltt_spec, i) + G_os * as;
    const float G_ld = diff ? grad_or_zero(P.g_ltt_diff, i) + G_od * ad : 0.0f;
    ray_group_means(F, G_ls, G_ld, gp_spec, gp_diff);
}

// albedo gradients of output element i from the forward's sums over the specular and the diffuse rays
__device__ __forceinline__ void finish_ray_api_bwd(const RayApiBwdParams& P, long i, float G_os, float G_od, float s_spec, float s_diff) {
    const RayApiParams& F = P.F;
    float gs = 0.f, gd = 0.f, ls, ld;
    ray_group_means(F, s_spec, s_diff, ls, ld);
    if (!F.no_albedo) {
        gs = G_os * ls;
        if (ray_has_diffuse(F)) {
            const float t = G_od * ld;
            if (ray_own_diffuse_albedo(F)) gd = t; else gs = gs + t;
        }
    }
    if (P.grad_alb_spec) P.grad_alb_spec[i] = gs;
    if (P.grad_alb_diff) P.grad_alb_diff[i] = gd;
}

__device__ __forceinline__ void scatter_tap(float* texel, float G_col, float w, float lp_scale) {
    if (w != 0.0f && G_col != 0.0f) atomicAdd(texel, G_col * w * lp_scale);
}

// one lane per (pixel, channel), as ray_renderer_api_kernel
__global__ void __launch_bounds__(256)
ray_renderer_api_bwd_kernel(const RayApiBwdParams P) {
    const RayApiParams& F = P.F;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;     // over N*C*hw
    if (i >= F.npix * F.C) return;
    long n, p, pix; int c;
    element_coords(i, F.C, F.hw, n, c, p, pix);
    const int n_spec = ray_n_spec(F);
    const size_t lp_off = F.lp_n == 1 ? 0 : (size_t)n * F.lp_h * F.lp_w * F.C;
    const float* lp = F.lp + lp_off + c;
    float* glp = P.grad_lp ? P.grad_lp + lp_off + c : nullptr;
    float G_os, G_od, gp_spec, gp_diff;
    ray_api_heads(P, i, G_os, G_od, gp_spec, gp_diff);
    float ss = 0.f, sd = 0.f;
    for (int r = 0; r < F.R; r++) {
        const float u = F.rays_uv[(pix * 2 + 0) * F.R + r], v = F.rays_uv[(pix * 2 + 1) * F.R + r];
        const Taps t = envmap_taps(u, v, F.lp_w, F.lp_h);
        const float col = probe_colour<size_t>(t, lp, F.lp_w, F.C, F.lp_scale);
        const size_t li = (((size_t)n * F.R + r) * F.C + c) * F.hw + p;
        const float lt = F.rays_lt[li];
        const float gp = r < n_spec ? gp_spec : gp_diff;
        if (P.grad_rays_lt) P.grad_rays_lt[li] = gp * col;
        const float prod = lt * col;
        if (r < n_spec) ss += prod; else sd += prod;
        if (glp) {
            const float G_col = grad_or_zero(P.g_rays_color, li) + gp * lt;
#pragma unroll
            for (int j = 0; j < 4; j++) scatter_tap(glp + t.texel<size_t>(j, F.lp_w, F.C), G_col, t.w(j), F.lp_scale);
        }
    }
    if (P.grad_alb_spec || P.grad_alb_diff) finish_ray_api_bwd(P, i, G_os, G_od, ss, sd);
}

// The RayTile form.  A wave's 64 lanes are 64 consecutive pixels on ONE ray index, and on a probe of a few hundred columns neighbouring
// pixels mostly hit the same texels: before the atomic, adjacent lanes holding the same texel add their contributions with a segmented
// shuffle reduction over the run, and the run's first lane issues one add (3.8x faster than one add per lane, tap and channel at
// 16 x 512^2: DESIGN.md 3.4b; the plain form is kept as scripts/experiments/ray_backward_atomic_per_tap.diff).  32-bit probe offsets.
__global__ void __launch_bounds__(RA_PIX * RA_QTR)
ray_renderer_api_bwd_tiled_kernel(const RayApiBwdParams P) {
    extern __shared__ float rb_sm[];
    const RayApiParams& F = P.F;
    const int R = F.R, C = F.C, n_spec = ray_n_spec(F);
    const RayTile T(F, rb_sm);
    const unsigned lp_off = F.lp_n == 1 ? 0u : (unsigned)T.n * (unsigned)(F.lp_h * F.lp_w * C);    // < 2^31 floats (entry point)
    const float* lp = F.lp + lp_off;
    float gp_spec[RA_CH] = {0.f, 0.f, 0.f, 0.f}, gp_diff[RA_CH] = {0.f, 0.f, 0.f, 0.f};
    if (T.live) {
#pragma unroll
        for (int c = 0; c < RA_CH; c++) {
            if (c >= C) break;
            float G_os, G_od;
            ray_api_heads(P, (T.n * C + c) * F.hw + T.p, G_os, G_od, gp_spec[c], gp_diff[c]);
        }
    }
    float ss[RA_CH] = {0.f, 0.f, 0.f, 0.f}, sd[RA_CH] = {0.f, 0.f, 0.f, 0.f};
    for (int r = T.qtr; r < R; r += RA_QTR) {   // wave-uniform trip count: every lane reaches the shuffles
        const float2 uv = T.uv(rb_sm, R, r);
        const Taps t = envmap_taps(uv.x, uv.y, F.lp_w, F.lp_h);
        float G_col[RA_CH] = {0.f, 0.f, 0.f, 0.f};
        if (T.live) {
#pragma unroll
            for (int c = 0; c < RA_CH; c++) {
                if (c >= C) break;
                const float col = probe_colour<unsigned>(t, lp + c, F.lp_w, C, F.lp_scale);
                const size_t li = (((size_t)T.n * R + r) * C + c) * F.hw + T.p;
                const float lt = F.rays_lt[li];
                const float gp = r < n_spec ? gp_spec[c] : gp_diff[c];
                if (P.grad_rays_lt) P.grad_rays_lt[li] = gp * col;
                const float prod = lt * col;
                if (r < n_spec) ss[c] += prod; else sd[c] += prod;
                if (P.grad_lp) G_col[c] = grad_or_zero(P.g_rays_color, li) + gp * lt;
            }
        }
        if (!P.grad_lp) continue;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            // key: the texel's offset in grad_lp; -1 where there is nothing to add (such a lane is a run of its own)
            const int key = (T.live && t.w(j) != 0.0f) ? (int)(lp_off + t.texel<unsigned>(j, F.lp_w, C)) : -1;
            float val[RA_CH];
#pragma unroll
            for (int c = 0; c < RA_CH; c++) val[c] = (key >= 0 && c < C) ? G_col[c] * t.w(j) * F.lp_scale : 0.0f;
            const int prev = __shfl_up(key, 1, 64);
            const bool head = T.lane == 0 || prev != key || key < 0;
            const unsigned long long heads = __ballot(head);
            const unsigned long long above = T.lane == 63 ? 0ull : heads >> (T.lane + 1);
            const int end = above ? T.lane + __ffsll((long long)above) - 1 : 63;      // last lane of this lane's run
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
                for (int c = 0; c < RA_CH; c++) {
                    if (c >= C) break;
                    const float o = __shfl_down(val[c], d, 64);
                    if (T.lane + d <= end) val[c] += o;
                }
            }
            if (head && key >= 0) {
#pragma unroll
                for (int c = 0; c < RA_CH; c++) {
                    if (c >= C) break;
                    if (val[c] != 0.0f) atomicAdd(P.grad_lp + key + c, val[c]);
                }
            }
        }
    }
    if (!P.grad_alb_spec && !P.grad_alb_diff) return;
    float s_spec, s_diff;
    if (!T.sums(rb_sm, C, ss, sd, s_spec, s_diff)) return;
    const long i = (T.n * C + T.qtr) * F.hw + T.p;
    float G_os, G_od, gs, gd;
    ray_api_heads(P, i, G_os, G_od, gs, gd);
    finish_ray_api_bwd(P, i, G_os, G_od, s_spec, s_diff);
}

// ---- layout helpers --------------------------------------------------------------------------------
// one element per thread: the form for channel counts whose 64-pixel tile does not fit 64 KB of LDS (c_pad > 240)
__global__ void __launch_bounds__(256)
nchw_to_nhwc_wide_kernel(const float* __restrict__ in, float* __restrict__ out, int c, int hw, int c_pad, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;   // over n*hw*c_pad
    if (i >= total) return;
    const int ch = (int)(i % c_pad);
    const long np = i / c_pad;
    const long n = np / hw, p = np % hw;
    out[i] = ch < c ? in[(n * c + ch) * hw + p] : 0.0f;
}
__global__ void __launch_bounds__(256)
nhwc_to_nchw_wide_kernel(const float* __restrict__ in, float* __restrict__ out, const float* __restrict__ bias,
                         int apply_tanh, int c, int hw, int c_pad, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;   // over n*c*hw (output order)
    if (i >= total) return;
    const long p = i % hw;
    const long nc = i / hw;
    const int ch = (int)(nc % c);
    const long n = nc / c;
    float v = in[(n * hw + p) * c_pad + ch];
    if (bias) v += bias[ch];
    if (apply_tanh) v = tanhf(v);
    out[i] = v;
}

__global__ void __launch_bounds__(256)
nchw_to_nhwc_kernel(const float* __restrict__ in, float* __restrict__ out, int c, int hw, int c_pad, long total) {
    // r05: through an LDS tile of 64 pixels x c_pad channels — reads coalesced along the pixels of a channel (NCHW rows), writes
    // coalesced along the channels of a pixel (the one-element-per-thread form reads with a stride of hw floats: 0.143 ms for the
    // 108-channel network input at 512^2, the layout change in front of the drop-in RenderingNet)
    extern __shared__ float lt_tile[];          // [c_pad][65]
    const long pix0 = (long)blockIdx.x * 64;    // over n * hw (hw is a multiple of 64 or the tail is masked)
    const long npix = total / c_pad;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long pp = pix0 + lane;
    const long n = pp / hw, p = pp % hw;
    for (int ch = w; ch < c_pad; ch += 4)
        lt_tile[ch * 65 + lane] = (ch < c && pp < npix) ? in[(n * c + ch) * hw + p] : 0.0f;
    __syncthreads();
    const int per = 64 * c_pad;
    float* dst = out + pix0 * c_pad;
    for (int i = threadIdx.x; i < per; i += 256) {
        const int px = i / c_pad, ch = i - px * c_pad;
        if (pix0 + px < npix) dst[i] = lt_tile[ch * 65 + px];
    }
}

__global__ void __launch_bounds__(256)
nhwc_to_nchw_kernel(const float* __restrict__ in, float* __restrict__ out, const float* __restrict__ bias,
                    int apply_tanh, int c, int hw, int c_pad, long total) {
    // the reverse through the same tile: reads coalesced along the channels of a pixel, writes along the pixels of a channel
    extern __shared__ float lt_tile[];          // [c_pad][65]
    const long npix = total / c;                // total = n * c * hw
    const long pix0 = (long)blockIdx.x * 64;
    const int per = 64 * c_pad;
    const float* src = in + pix0 * c_pad;
    for (int i = threadIdx.x; i < per; i += 256) {
        const int px = i / c_pad, ch = i - px * c_pad;
        if (pix0 + px < npix) lt_tile[ch * 65 + px] = src[i];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long pp = pix0 + lane;
    if (pp >= npix) return;
    const long n = pp / hw, p = pp % hw;
    for (int ch = w; ch < c; ch += 4) {
        float v = lt_tile[ch * 65 + lane];
        if (bias) v += bias[ch];
        if (apply_tanh) v = tanhf(v);
        out[(n * c + ch) * hw + p] = v;
    }
}

}  // namespace rnr

using namespace rnr;

// ---- host helpers ----------------------------------------------------------------------------------
// workgroups of 256 threads for `total` one-thread items
static dim3 grid256(long total) { return dim3((unsigned)((total + 255) / 256)); }

// ray pivots arrive as [3][R] (the reference's layout); the kernels read [R][3]
static void transpose_pivots(float* dst, const float* src_host, int num_rays) {
    for (int r = 0; r < num_rays; r++)
        for (int k = 0; k < 3; k++) dst[r * 3 + k] = src_host[k * num_rays + r];
}

// texture-level table of a kernel parameter block (F = const float for the forward kernels, float for the gradient levels of
// rnr_texture_mapper_backward, which also takes a 1 x 1 level: min_size).  max_level_bytes > 0 bounds a level's size: the
// buffer-resource path of shade_inputs_kernel addresses texels with 32-bit offsets
template <class F>
static int fill_texture_levels(const char* fn, F** tex, int* tex_size, F* const* textures_host, const int* tex_sizes_host,
                               int num_levels, int tex_channels, size_t max_level_bytes, int min_size = 2) {
    for (int l = 0; l < num_levels; l++) {
        RNR_REQUIRE(textures_host[l] && tex_sizes_host[l] >= min_size, "%s: bad texture level %d", fn, l);
        RNR_REQUIRE(!max_level_bytes || (size_t)tex_sizes_host[l] * tex_sizes_host[l] * tex_channels * sizeof(float) < max_level_bytes,
                    "%s: texture level %d exceeds 2 GiB (32-bit texel offsets)", fn, l);
        tex[l] = textures_host[l];
        tex_size[l] = tex_sizes_host[l];
    }
    return 0;
}

// What rnr_ray_render and rnr_ray_weights check alike, and ni_need: the floats of a net_in row their kernels stage (ray
// directions, normal / view, the albedo channels, rounded up to whole float4s).  max_diff is each kernel's own limit.
static int ray_launch_checks(const char* fn, int num_spec, int num_diff, int max_diff, int lp_h, int lp_w, int albedo_diff_ch,
                             int albedo_spec_ch, int c_pad, int* ni_need) {
    RNR_REQUIRE(num_spec >= 1 && num_spec <= 16 && num_diff >= 0 && num_diff <= max_diff,
                "%s: at most 16 specular / %d diffuse rays (got %d, %d)", fn, max_diff, num_spec, num_diff);
    RNR_REQUIRE(lp_h >= 2 && lp_w >= 2, "%s: bad light-probe size", fn);
    const int alb_hi = (albedo_diff_ch > albedo_spec_ch ? albedo_diff_ch : albedo_spec_ch) + 3;
    *ni_need = (3 * (num_spec + num_diff) + 6 + alb_hi + 3) / 4 * 4;
    RNR_REQUIRE(*ni_need <= c_pad && c_pad % 4 == 0, "%s: channel stride must be a multiple of 4 and cover the albedo channels", fn);
    return 0;
}
// workgroups of the two ray kernels: 32 lanes per pixel group of RR_PIX pixels
static dim3 ray_grid(long npix) { return grid256((npix + RR_PIX - 1) / RR_PIX * 32); }

extern "C" int rnr_project_vertices(const float* vertices, const float* K, const float* R, const float* t,
                                    const float* dist_coeffs, const float* offset, const float* scale,
                                    float* out, int num_views, int num_vertices, float orig_size, float eps,
                                    void* stream) {
    RNR_REQUIRE(vertices && K && R && t && out, "rnr_project_vertices: null pointer argument");
    RNR_REQUIRE((offset == nullptr) == (scale == nullptr), "rnr_project_vertices: offset and scale go together");
    RNR_REQUIRE(num_views > 0 && num_vertices > 0, "rnr_project_vertices: bad sizes");
    RNR_REQUIRE(aligned_to(4, {vertices, K, R, t, dist_coeffs, offset, scale, out}),
                "rnr_project_vertices: vertices, K, R, t, dist_coeffs, offset, scale and out must be 4-byte aligned");
    const long total = (long)num_views * num_vertices;
    hipLaunchKernelGGL(project_vertices_kernel, grid256(total), dim3(256), 0,
                       as_stream(stream), vertices, K, R, t, dist_coeffs, offset, scale, out, num_views,
                       num_vertices, orig_size, eps);
    return check_launch("project_vertices_kernel");
}

extern "C" int rnr_face_tangents(const rnr_mesh* mesh, float* out, void* stream) {
    RNR_REQUIRE(mesh && out && mesh->v && mesh->vt && mesh->f_v_idx && mesh->f_vt_idx && mesh->num_faces > 0,
                "rnr_face_tangents: incomplete mesh");
    RNR_REQUIRE(aligned_to(4, {mesh->v, mesh->vt, mesh->vn, mesh->f_v_idx, mesh->f_vt_idx, mesh->f_vn_idx, out}),
                "rnr_face_tangents: the mesh arrays and out must be 4-byte aligned");
    hipLaunchKernelGGL(face_tangents_kernel, dim3((mesh->num_faces + 255) / 256), dim3(256), 0,
                       as_stream(stream), *mesh, out);
    return check_launch("face_tangents_kernel");
}

extern "C" int rnr_shade_inputs(const int32_t* face_index_map, const float* alpha, const float* uv_map,
                                const float* normal_map, const float* face_tangents, int num_faces,
                                const float* proj_inv, const float* R_inv, const float* const* textures_host,
                                const int* tex_sizes_host, int num_levels, int tex_channels, int sh_start_ch,
                                const rnr_rays* rays, float* net_in, int c_pad, float* rays_uv,
                                float* neural_img, float* sh_basis_map, int num_views, int height, int width,
                                void* stream) {
    RNR_REQUIRE(face_index_map && alpha && uv_map && normal_map && face_tangents && proj_inv && R_inv &&
                    textures_host && tex_sizes_host && rays && net_in,
                "rnr_shade_inputs: null pointer argument");
    RNR_REQUIRE(num_levels >= 1 && num_levels <= MAX_LEVELS, "rnr_shade_inputs: num_levels %d not in [1,%d]",
                num_levels, MAX_LEVELS);
    RNR_REQUIRE(tex_channels > 0 && tex_channels % 4 == 0, "rnr_shade_inputs: texture channels must be a multiple of 4");
    RNR_REQUIRE(rays->num_spec >= 0 && rays->num_spec <= MAX_RAYS && rays->num_diff >= 0 && rays->num_diff <= MAX_RAYS,
                "rnr_shade_inputs: at most %d rays per sampler", MAX_RAYS);
    const int c_in = 3 * (rays->num_spec + rays->num_diff) + 6 + tex_channels;
    RNR_REQUIRE(c_pad >= c_in && c_pad % 4 == 0, "rnr_shade_inputs: c_pad %d < %d or not a multiple of 4", c_pad, c_in);
    RNR_REQUIRE((3 * (rays->num_spec + rays->num_diff) + 6) % 4 == 0,
                "rnr_shade_inputs: 3*rays+6 must be a multiple of 4 (texture channels are written as float4)");
    RNR_REQUIRE(sh_start_ch < 0 || sh_start_ch + 9 <= tex_channels, "rnr_shade_inputs: sh_start_ch + 9 > channels");
    RNR_REQUIRE(num_views > 0 && height > 0 && width > 0 && num_faces > 0, "rnr_shade_inputs: bad sizes");
    RNR_REQUIRE(aligned_to(16, {net_in}), "rnr_shade_inputs: net_in must be 16-byte aligned");
    RNR_REQUIRE(aligned_to(4, {face_index_map, alpha, uv_map, normal_map, face_tangents, proj_inv, R_inv, rays_uv, neural_img, sh_basis_map}),
                "rnr_shade_inputs: face_index_map, alpha, uv_map, normal_map, face_tangents, proj_inv, R_inv, rays_uv, neural_img and "
                "sh_basis_map must be 4-byte aligned");
    for (int l = 0; l < num_levels; l++)
        RNR_REQUIRE(aligned_to(16, {textures_host[l]}), "rnr_shade_inputs: textures_host[%d] must be 16-byte aligned", l);
    ShadeParams P = {};
    P.face_index_map = face_index_map; P.alpha = alpha; P.uv_map = uv_map; P.normal_map = normal_map;
    P.tangents = face_tangents; P.num_faces = num_faces; P.proj_inv = proj_inv; P.R_inv = R_inv;
    if (int e = fill_texture_levels("rnr_shade_inputs", P.tex, P.tex_size, textures_host, tex_sizes_host, num_levels, tex_channels,
                                    (size_t)1 << 31))
        return e;
    P.num_levels = num_levels; P.C = tex_channels; P.sh_start = sh_start_ch;
    P.n_spec = rays->num_spec; P.n_diff = rays->num_diff;
    transpose_pivots(P.piv_spec, rays->pivots_spec_host, rays->num_spec);
    transpose_pivots(P.piv_diff, rays->pivots_diff_host, rays->num_diff);
    P.net_in = net_in; P.c_pad = c_pad; P.rays_uv = rays_uv; P.neural_img = neural_img; P.sh_basis_map = sh_basis_map;
    P.npix = (long)num_views * height * width; P.H = height; P.W = width;
    const size_t lds = (size_t)(SH_PIX * c_pad + SH_PIX * GEO) * sizeof(float);
    RNR_REQUIRE(lds <= 160 * 1024, "rnr_shade_inputs: c_pad too large for LDS");
    const unsigned blocks = (unsigned)((P.npix + SH_PIX - 1) / SH_PIX);
    hipLaunchKernelGGL(shade_inputs_kernel, dim3(blocks), dim3(SH_THREADS), lds, as_stream(stream), P);
    return check_launch("shade_inputs_kernel");
}

extern "C" int rnr_ray_render(const float* unet_raw, int c_out_pad, const float* bias, const float* net_in,
                              int c_pad, const float* alpha, const float* lp, int lp_h, int lp_w, int num_spec,
                              int num_diff, int albedo_diff_ch, int albedo_spec_ch, float* image, int num_views,
                              int height, int width, void* stream) {
    RNR_REQUIRE(unet_raw && bias && net_in && alpha && lp && image, "rnr_ray_render: null pointer argument");
    RNR_REQUIRE(num_views > 0 && height > 0 && width > 0, "rnr_ray_render: bad sizes");
    RNR_REQUIRE(aligned_to(16, {unet_raw, net_in}), "rnr_ray_render: unet_raw and net_in must be 16-byte aligned");
    RNR_REQUIRE(aligned_to(4, {bias, alpha, lp, image}), "rnr_ray_render: bias, alpha, lp and image must be 4-byte aligned");
    RayParams P;
    // 16 diffuse rays: one per lane of the second 16-lane segment
    if (int e = ray_launch_checks("rnr_ray_render", num_spec, num_diff, 16, lp_h, lp_w, albedo_diff_ch, albedo_spec_ch, c_pad, &P.ni_need))
        return e;
    RNR_REQUIRE(c_out_pad % 4 == 0, "rnr_ray_render: c_out_pad must be a multiple of 4");
    P.unet_raw = unet_raw; P.c_out_pad = c_out_pad; P.bias = bias; P.net_in = net_in; P.c_pad = c_pad;
    P.alpha = alpha; P.lp = lp; P.lp_h = lp_h; P.lp_w = lp_w; P.n_spec = num_spec; P.n_diff = num_diff;
    P.alb_diff_ch = albedo_diff_ch; P.alb_spec_ch = albedo_spec_ch; P.image = image;
    P.npix = (long)num_views * height * width; P.hw = height * width;
    const size_t lds = (size_t)RR_WG_PIX * (size_t)(c_out_pad + P.ni_need) * sizeof(float);
    RNR_REQUIRE(lds <= 64 * 1024, "rnr_ray_render: rows too wide for the LDS staging (%zu bytes)", lds);
    hipLaunchKernelGGL(ray_render_kernel, ray_grid(P.npix), dim3(256), lds, as_stream(stream), P);
    return check_launch("ray_render_kernel");
}

extern "C" int rnr_ray_weights(const float* net_in, int c_pad, const float* alpha, const float* lp, int lp_h, int lp_w,
                               int num_spec, int num_diff, int albedo_diff_ch, int albedo_spec_ch, float* ray_w, int c_w,
                               int num_views, int height, int width, void* stream) {
    RNR_REQUIRE(net_in && alpha && lp && ray_w, "rnr_ray_weights: null pointer argument");
    RNR_REQUIRE(num_views > 0 && height > 0 && width > 0, "rnr_ray_weights: bad sizes");
    RNR_REQUIRE(aligned_to(16, {net_in, ray_w}), "rnr_ray_weights: net_in and ray_w must be 16-byte aligned");
    RNR_REQUIRE(aligned_to(4, {alpha, lp}), "rnr_ray_weights: alpha and lp must be 4-byte aligned");
    RayWeightParams P;
    // 15 diffuse rays: lane 31 never holds a ray, it writes the padding columns
    if (int e = ray_launch_checks("rnr_ray_weights", num_spec, num_diff, 15, lp_h, lp_w, albedo_diff_ch, albedo_spec_ch, c_pad, &P.ni_need))
        return e;
    RNR_REQUIRE(c_w >= 3 * (num_spec + num_diff), "rnr_ray_weights: c_w %d < 3 * rays", c_w);
    P.net_in = net_in; P.c_pad = c_pad; P.alpha = alpha; P.lp = lp; P.lp_h = lp_h; P.lp_w = lp_w;
    P.n_spec = num_spec; P.n_diff = num_diff; P.alb_diff_ch = albedo_diff_ch; P.alb_spec_ch = albedo_spec_ch;
    P.ray_w = ray_w; P.c_w = c_w; P.npix = (long)num_views * height * width;
    RNR_REQUIRE(c_w % 4 == 0, "rnr_ray_weights: c_w must be a multiple of 4");
    const size_t lds = (size_t)RR_WG_PIX * (size_t)(P.ni_need + c_w) * sizeof(float);
    RNR_REQUIRE(lds <= 64 * 1024, "rnr_ray_weights: rows too wide for the LDS staging (%zu bytes)", lds);
    hipLaunchKernelGGL(ray_weights_kernel, ray_grid(P.npix), dim3(256), lds, as_stream(stream), P);
    return check_launch("ray_weights_kernel");
}

extern "C" int rnr_sh_basis(const float* dirs, float* out, int n, int lmax, void* stream) {
    RNR_REQUIRE(dirs && out && n > 0, "rnr_sh_basis: bad arguments");
    RNR_REQUIRE(lmax >= 0 && lmax <= SH_LMAX_MAX, "rnr_sh_basis: lmax %d not in [0,%d]", lmax, SH_LMAX_MAX);
    RNR_REQUIRE(aligned_to(4, {dirs, out}), "rnr_sh_basis: dirs and out must be 4-byte aligned");
    hipLaunchKernelGGL(sh_basis_kernel, dim3((n + 127) / 128), dim3(128), 0, as_stream(stream), dirs, out, n, lmax);
    return check_launch("sh_basis_kernel");
}

extern "C" int rnr_sh_reconstruct(const float* basis, const float* coeff, float* out, int num_samples,
                                  int num_basis, int num_channels, void* stream) {
    RNR_REQUIRE(basis && coeff && out && num_samples > 0 && num_basis > 0 && num_channels > 0,
                "rnr_sh_reconstruct: bad arguments");
    RNR_REQUIRE(aligned_to(4, {basis, coeff, out}), "rnr_sh_reconstruct: basis, coeff and out must be 4-byte aligned");
    const size_t lds = (size_t)(SHR_ROWS * num_basis + num_basis * num_channels) * sizeof(float);
    RNR_REQUIRE(lds <= 64 * 1024, "rnr_sh_reconstruct: num_basis * (64 + num_channels) floats must fit 64 KiB of LDS");
    hipLaunchKernelGGL(sh_reconstruct_kernel, dim3((unsigned)((num_samples + SHR_ROWS - 1) / SHR_ROWS)), dim3(256), lds,
                       as_stream(stream), basis, coeff, out, num_samples, num_basis, num_channels);
    return check_launch("sh_reconstruct_kernel");
}

extern "C" int rnr_frame_prepare(const rnr_mesh* mesh, const float* K, const float* pose, int num_views, int image_size,
                                 float eps, float* v_uvz, float* tangents, const float* lp_basis, const float* lp_coeff,
                                 float* light_probe, int lp_samples, int lp_num_basis, int lp_channels,
                                 void* gbuffer_workspace, void* stream) {
    RNR_REQUIRE(mesh && mesh->v && mesh->num_vertices > 0 && mesh->num_faces > 0, "rnr_frame_prepare: incomplete mesh");
    RNR_REQUIRE(num_views > 0 && image_size > 0, "rnr_frame_prepare: bad sizes");
    RNR_REQUIRE(!v_uvz || (K && pose), "rnr_frame_prepare: the projection needs K and pose");
    RNR_REQUIRE(!tangents || (mesh->vt && mesh->f_v_idx && mesh->f_vt_idx), "rnr_frame_prepare: tangents need vt and the index arrays");
    RNR_REQUIRE(!light_probe || (lp_basis && lp_coeff && lp_samples > 0 && lp_num_basis > 0 && lp_channels > 0),
                "rnr_frame_prepare: the light probe needs basis, coefficients and sizes");
    RNR_REQUIRE(aligned_to(16, {gbuffer_workspace}), "rnr_frame_prepare: gbuffer_workspace must be 16-byte aligned");
    RNR_REQUIRE(aligned_to(4, {mesh->v, mesh->vt, mesh->vn, mesh->f_v_idx, mesh->f_vt_idx, mesh->f_vn_idx, K, pose, v_uvz, tangents, lp_basis,
                               lp_coeff, light_probe}),
                "rnr_frame_prepare: the mesh arrays, K, pose, v_uvz, tangents, lp_basis, lp_coeff and light_probe must be 4-byte aligned");
    FramePrepParams P = {};
    P.mesh = *mesh; P.K = K; P.pose = pose; P.v_uvz = v_uvz; P.nviews = num_views; P.orig_size = (float)image_size; P.eps = eps;
    P.tangents = tangents;
    P.lp_basis = lp_basis; P.lp_coeff = lp_coeff; P.lp_out = light_probe; P.lp_ns = lp_samples; P.lp_nb = lp_num_basis;
    P.lp_nc = lp_channels;
    size_t lds = 0;
    long nb = 0;
    if (v_uvz) nb += ((long)num_views * mesh->num_vertices + 255) / 256;
    P.b_proj = (int)nb;
    if (tangents) nb += (mesh->num_faces + 255) / 256;
    P.b_tan = (int)nb;
    if (light_probe) {
        lds = (size_t)(SHR_ROWS * lp_num_basis + lp_num_basis * lp_channels) * sizeof(float);
        RNR_REQUIRE(lds <= 64 * 1024, "rnr_frame_prepare: num_basis * (64 + num_channels) floats must fit 64 KiB of LDS");
        nb += (lp_samples + SHR_ROWS - 1) / SHR_ROWS;
    }
    P.b_lp = (int)nb;
    if (gbuffer_workspace) {
        gbuffer_clear_regions(gbuffer_workspace, num_views, mesh->num_faces, image_size, &P.counters, &P.counter_vec, &P.keys,
                              &P.key_vec);
        nb += (P.counter_vec + P.key_vec + 255) / 256;
    }
    P.b_clear = (int)nb;
    RNR_REQUIRE(nb > 0 && nb < (1L << 31), "rnr_frame_prepare: nothing to do / grid too large");
    hipLaunchKernelGGL(frame_prepare_kernel, dim3((unsigned)nb), dim3(256), lds, as_stream(stream), P);
    return check_launch("frame_prepare_kernel");
}

extern "C" int rnr_sh_fit(const float* samples, const float* basis, float* out, int num_samples, int num_basis,
                          int num_channels, void* stream) {
    RNR_REQUIRE(samples && basis && out && num_samples > 0 && num_basis > 0 && num_channels > 0,
                "rnr_sh_fit: bad arguments");
    RNR_REQUIRE(aligned_to(4, {samples, basis, out}), "rnr_sh_fit: samples, basis and out must be 4-byte aligned");
    hipLaunchKernelGGL(sh_fit_kernel<true>, dim3(num_basis * num_channels), dim3(256), 0, as_stream(stream), samples,
                       basis, out, num_samples, num_basis, num_channels);
    return check_launch("sh_fit_kernel");
}

extern "C" int rnr_sh_reconstruct_backward(const float* basis, const float* grad_out, float* grad_coeff, int num_samples,
                                           int num_basis, int num_channels, void* stream) {
    RNR_REQUIRE(basis && grad_out && grad_coeff && num_samples > 0 && num_basis > 0 && num_channels > 0,
                "rnr_sh_reconstruct_backward: bad arguments");
    RNR_REQUIRE(aligned_to(4, {basis, grad_out, grad_coeff}),
                "rnr_sh_reconstruct_backward: basis, grad_out and grad_coeff must be 4-byte aligned");
    hipLaunchKernelGGL(sh_fit_kernel<false>, dim3(num_basis * num_channels), dim3(256), 0, as_stream(stream), grad_out,
                       basis, grad_coeff, num_samples, num_basis, num_channels);
    return check_launch("sh_fit_kernel");
}

extern "C" int rnr_interpolate_bilinear(const float* data, int h, int w, int c, const float* x, const float* y,
                                        float* out, int32_t* taps, int n, void* stream) {
    RNR_REQUIRE(data && x && y && out && h > 0 && w > 0 && c > 0 && n > 0, "rnr_interpolate_bilinear: bad arguments");
    RNR_REQUIRE(aligned_to(4, {data, x, y, out, taps}), "rnr_interpolate_bilinear: data, x, y, out and taps must be 4-byte aligned");
    const long total = (long)n * c;
    hipLaunchKernelGGL(interpolate_bilinear_kernel, grid256(total), dim3(256), 0,
                       as_stream(stream), data, h, w, c, x, y, out, taps, n);
    return check_launch("interpolate_bilinear_kernel");
}

// ------------------------------------------------------------------------------------------------
// Area-average image resize: what LightingLP.__init__ asks of cv2.resize(..., interpolation=cv2.INTER_AREA)
// (network.py:667) for the 1600 x 3200 light probes.  Restated from OpenCV's published algorithm (imgproc/resize.cpp):
//   * shrinking on both axes (scale = src/dst >= 1): separable box filter with fractional cell coverage
//     (computeResizeAreaTab): cell [d*scale, (d+1)*scale) of the source axis; a partially covered first pixel weighs
//     (ceil(f1) - f1), whole pixels 1, a partially covered last pixel min(f2 - floor(f2), 1), all divided by
//     cellWidth = min(scale, ssize - f1); partial coverage below 1e-3 is dropped.  Integer ratios reduce to the plain
//     box mean.
//   * otherwise (enlarging on an axis): OpenCV switches to its "area-mode" bilinear: s = floor(d*scale),
//     f = (d+1) - (s+1)/scale, f <= 0 ? 0 : f - floor(f); out = (1-f)*src[s] + f*src[min(s+1, ssize-1)].
// cv2 is absent from this image: parity with OpenCV is UNPINNED (the oracle pins the integer-ratio case against a
// numpy box mean).  One lane per (output pixel, channel); an init-time operator, not on the per-view path.
// The arithmetic itself is rnr_internal.h's resize_area_pixel (area_cell + the accumulation), shared with photo.hip.
__global__ void __launch_bounds__(256)
resize_area_kernel(const float* __restrict__ src, float* __restrict__ dst, int sh, int sw, int dh, int dw, int c) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)dh * dw * c) return;
    const int ch = (int)(i % c);
    const int dx = (int)((i / c) % dw), dy = (int)(i / ((long)c * dw));
    float acc[1];
    resize_area_pixel<1>(dy, dx, sh, sw, dh, dw, [&](int y, int x, int) { return src[((size_t)y * sw + x) * c + ch]; }, acc);
    dst[i] = acc[0];
}

extern "C" int rnr_resize_area(const float* src, float* dst, int src_h, int src_w, int dst_h, int dst_w, int channels,
                               void* stream) {
    RNR_REQUIRE(src && dst && src_h > 0 && src_w > 0 && dst_h > 0 && dst_w > 0 && channels > 0, "rnr_resize_area: bad arguments");
    RNR_REQUIRE(aligned_to(4, {src, dst}), "rnr_resize_area: src and dst must be 4-byte aligned");
    const long total = (long)dst_h * dst_w * channels;
    hipLaunchKernelGGL(resize_area_kernel, grid256(total), dim3(256), 0, as_stream(stream), src, dst,
                       src_h, src_w, dst_h, dst_w, channels);
    return check_launch("resize_area_kernel");
}

extern "C" int rnr_nchw_to_nhwc(const float* in, float* out, int n, int c, int h, int w, int c_pad, void* stream) {
    RNR_REQUIRE(in && out && n > 0 && c > 0 && c_pad >= c, "rnr_nchw_to_nhwc: bad arguments");
    RNR_REQUIRE(h > 0 && w > 0, "rnr_nchw_to_nhwc: bad sizes");
    RNR_REQUIRE(aligned_to(4, {in, out}), "rnr_nchw_to_nhwc: in and out must be 4-byte aligned");
    const long total = (long)n * h * w * c_pad;
    const long npix = (long)n * h * w;
    if (c_pad <= 240)       // 64-pixel x c_pad tile in LDS (<= 62.4 KB)
        hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3((unsigned)((npix + 63) / 64)), dim3(256), (size_t)c_pad * 65 * sizeof(float),
                           as_stream(stream), in, out, c, h * w, c_pad, total);
    else
        hipLaunchKernelGGL(nchw_to_nhwc_wide_kernel, grid256(total), dim3(256), 0, as_stream(stream),
                           in, out, c, h * w, c_pad, total);
    return check_launch("nchw_to_nhwc_kernel");
}

extern "C" int rnr_nhwc_to_nchw(const float* in, float* out, const float* bias, int apply_tanh, int n, int c,
                                int h, int w, int c_pad, void* stream) {
    RNR_REQUIRE(in && out && n > 0 && c > 0 && c_pad >= c, "rnr_nhwc_to_nchw: bad arguments");
    RNR_REQUIRE(h > 0 && w > 0, "rnr_nhwc_to_nchw: bad sizes");
    RNR_REQUIRE(aligned_to(4, {in, out, bias}), "rnr_nhwc_to_nchw: in, out and bias must be 4-byte aligned");
    const long total = (long)n * c * h * w;
    const long npix = (long)n * h * w;
    if (c_pad <= 240)
        hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3((unsigned)((npix + 63) / 64)), dim3(256), (size_t)c_pad * 65 * sizeof(float),
                           as_stream(stream), in, out, bias, apply_tanh, c, h * w, c_pad, total);
    else
        hipLaunchKernelGGL(nhwc_to_nchw_wide_kernel, grid256(total), dim3(256), 0, as_stream(stream),
                           in, out, bias, apply_tanh, c, h * w, c_pad, total);
    return check_launch("nhwc_to_nchw_kernel");
}

extern "C" int rnr_view_dir_map(const float* proj_inv, const float* R_inv, float* out_world, float* out_cam,
                                int num_views, int height, int width, void* stream) {
    RNR_REQUIRE(proj_inv && R_inv && out_world && num_views > 0 && height > 0 && width > 0, "rnr_view_dir_map: bad arguments");
    RNR_REQUIRE(aligned_to(4, {proj_inv, R_inv, out_world, out_cam}),
                "rnr_view_dir_map: proj_inv, R_inv, out_world and out_cam must be 4-byte aligned");
    const long npix = (long)num_views * height * width;
    hipLaunchKernelGGL(view_dir_map_kernel, grid256(npix), dim3(256), 0, as_stream(stream),
                       proj_inv, R_inv, out_world, out_cam, npix, height, width);
    return check_launch("view_dir_map_kernel");
}

// envmap_texels addresses the probe with 24-bit multiplies
static int probe_checks(const char* fn, int lp_h, int lp_w) {
    RNR_REQUIRE(lp_h >= 1 && lp_w >= 1, "%s: bad light-probe size %d x %d", fn, lp_h, lp_w);
    RNR_REQUIRE((long)lp_h * lp_w * 3 < (1L << 24), "%s: light probe %d x %d has 2^24 floats or more (24-bit texel offsets)", fn, lp_h, lp_w);
    return 0;
}

extern "C" int rnr_env_background(const float* proj_inv, const float* R_inv, const float* lp, int lp_n, int lp_h, int lp_w,
                                  float* out, int num_views, int height, int width, void* stream) {
    RNR_REQUIRE(proj_inv && R_inv && lp && out, "rnr_env_background: null pointer argument");
    RNR_REQUIRE(num_views > 0 && height > 0 && width > 0 && (long)height * width < (1L << 31), "rnr_env_background: bad sizes");
    if (int e = probe_checks("rnr_env_background", lp_h, lp_w)) return e;
    RNR_REQUIRE(lp_n == 1 || lp_n == num_views, "rnr_env_background: lp batch must be 1 or N");
    RNR_REQUIRE(aligned_to(4, {proj_inv, R_inv, lp, out}), "rnr_env_background: proj_inv, R_inv, lp and out must be 4-byte aligned");
    const long npix = (long)num_views * height * width;
    hipLaunchKernelGGL(env_background_kernel, grid256(npix), dim3(256), 0, as_stream(stream), proj_inv, R_inv, lp, lp_n, lp_h,
                       lp_w, out, npix, height, width);
    return check_launch("env_background_kernel");
}

extern "C" int rnr_present_u8(const float* image, const float* alpha, const float* proj_inv, const float* R_inv,
                              const float* lp, int lp_h, int lp_w, int mode, uint8_t* out, int num_views, int height, int width,
                              void* stream) {
    const int m = mode & ~RNR_PRESENT_RGB;
    RNR_REQUIRE(m == RNR_PRESENT_FRAME || m == RNR_PRESENT_COMPOSITE || m == RNR_PRESENT_BACKGROUND, "rnr_present_u8: unknown mode %d", mode);
    RNR_REQUIRE(out, "rnr_present_u8: null pointer argument (out)");
    RNR_REQUIRE(m == RNR_PRESENT_BACKGROUND || image, "rnr_present_u8: null pointer argument (image)");
    RNR_REQUIRE(m != RNR_PRESENT_COMPOSITE || alpha, "rnr_present_u8: null pointer argument (alpha)");
    RNR_REQUIRE(num_views > 0 && height > 0 && width > 0 && (long)height * width < (1L << 31), "rnr_present_u8: bad sizes");
    if (m != RNR_PRESENT_FRAME) {
        RNR_REQUIRE(proj_inv && R_inv && lp, "rnr_present_u8: null pointer argument (proj_inv, R_inv, lp)");
        if (int e = probe_checks("rnr_present_u8", lp_h, lp_w)) return e;
    }
    PresentParams P;
    P.image = image; P.alpha = alpha; P.proj_inv = proj_inv; P.R_inv = R_inv; P.lp = lp; P.lp_h = lp_h; P.lp_w = lp_w;
    P.mode = m; P.rgb = (mode & RNR_PRESENT_RGB) ? 1 : 0; P.out = out;
    P.npix = (long)num_views * height * width; P.H = height; P.W = width;
    // four pixels per thread: whole groups inside a view, dword stores, float4 loads of the planes the mode reads
    const bool vec = ((long)height * width) % 4 == 0 && (uintptr_t)out % 4 == 0 &&
                     (m == RNR_PRESENT_BACKGROUND || (uintptr_t)image % 16 == 0) &&
                     (m != RNR_PRESENT_COMPOSITE || (uintptr_t)alpha % 16 == 0);
    if (vec) hipLaunchKernelGGL(present_u8_kernel<4>, grid256(P.npix / 4), dim3(256), 0, as_stream(stream), P);
    else hipLaunchKernelGGL(present_u8_kernel<1>, grid256(P.npix), dim3(256), 0, as_stream(stream), P);
    return check_launch("present_u8_kernel");
}

extern "C" int rnr_tbn_map(const float* normal_map, const int32_t* face_index_map, const float* face_tangents,
                           int num_faces, float* out, int num_views, int height, int width, void* stream) {
    RNR_REQUIRE(normal_map && face_index_map && face_tangents && out && num_faces > 0, "rnr_tbn_map: bad arguments");
    RNR_REQUIRE(num_views > 0 && height > 0 && width > 0, "rnr_tbn_map: bad sizes");
    RNR_REQUIRE(aligned_to(4, {normal_map, face_index_map, face_tangents, out}),
                "rnr_tbn_map: normal_map, face_index_map, face_tangents and out must be 4-byte aligned");
    const long npix = (long)num_views * height * width;
    hipLaunchKernelGGL(tbn_map_kernel, grid256(npix), dim3(256), 0, as_stream(stream), normal_map,
                       face_index_map, face_tangents, num_faces, out, npix);
    return check_launch("tbn_map_kernel");
}

// out[p][i] = sum_j M[p][i][j] v[p][j] with M = tbn[p] (transposed = 0) or tbn[p]^T (transposed = 1): the per-pixel 3x3 products of
// test_rnr.py:314 (torch.matmul(TBN_map.reshape((-1, 3, 3)).transpose(-2, -1), view_dir_map.reshape((-1, 3, 1)))), which torch hands to
// rocBLAS as 262 144 batched 3 x 3 GEMMs (1.9 ms per 512^2 view; this launch: a few us).  One pixel per thread; the 36 + 12 bytes of
// a pixel are read with 4-byte loads that the L1 merges (consecutive threads, consecutive records).
__global__ void __launch_bounds__(256)
tbn_matvec_kernel(const float* __restrict__ tbn, const float* __restrict__ v, float* __restrict__ out, long npix, int transposed) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const float* m = tbn + p * 9;
    const float x = v[p * 3 + 0], y = v[p * 3 + 1], z = v[p * 3 + 2];
    float o[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float a = transposed ? m[i] : m[3 * i], b = transposed ? m[3 + i] : m[3 * i + 1], c = transposed ? m[6 + i] : m[3 * i + 2];
        o[i] = __builtin_fmaf(c, z, __builtin_fmaf(b, y, a * x));
    }
    out[p * 3 + 0] = o[0]; out[p * 3 + 1] = o[1]; out[p * 3 + 2] = o[2];
}

extern "C" int rnr_tbn_matvec(const float* tbn, const float* vec, float* out, long num_pixels, int transposed, void* stream) {
    RNR_REQUIRE(tbn && vec && out && num_pixels > 0, "rnr_tbn_matvec: bad arguments");
    RNR_REQUIRE(aligned_to(4, {tbn, vec, out}), "rnr_tbn_matvec: tbn, vec and out must be 4-byte aligned");
    hipLaunchKernelGGL(tbn_matvec_kernel, grid256(num_pixels), dim3(256), 0, as_stream(stream), tbn, vec, out,
                       num_pixels, transposed);
    return check_launch("tbn_matvec_kernel");
}

extern "C" int rnr_ray_sampler(int reflect, const float* pivots_host, int num_rays, const float* tbn,
                               const float* view_tangent, const float* alpha, float* rays_dir, float* rays_uv,
                               float* rays_dir_tangent, long num_pixels, void* stream) {
    RNR_REQUIRE(pivots_host && tbn && alpha && rays_dir && rays_uv, "rnr_ray_sampler: null pointer argument");
    RNR_REQUIRE(!reflect || view_tangent, "rnr_ray_sampler: reflect mode needs view_tangent");
    RNR_REQUIRE(num_rays >= 1 && num_rays <= MAX_RAYS, "rnr_ray_sampler: 1..%d rays", MAX_RAYS);
    RNR_REQUIRE(num_pixels > 0, "rnr_ray_sampler: bad sizes");
    RNR_REQUIRE(aligned_to(4, {tbn, view_tangent, alpha, rays_dir, rays_uv, rays_dir_tangent}),
                "rnr_ray_sampler: tbn, view_tangent, alpha, rays_dir, rays_uv and rays_dir_tangent must be 4-byte aligned");
    RaySamplerParams P;
    P.tbn = tbn; P.view_tangent = view_tangent; P.alpha = alpha; P.rays_dir = rays_dir; P.rays_uv = rays_uv;
    P.rays_dir_tangent = reflect ? rays_dir_tangent : nullptr;
    transpose_pivots(P.piv, pivots_host, num_rays);
    P.n_rays = num_rays; P.reflect = reflect; P.npix = num_pixels;
    const long total = num_pixels * num_rays;
    hipLaunchKernelGGL(ray_sampler_kernel, grid256(total), dim3(256), 0, as_stream(stream), P);
    return check_launch("ray_sampler_kernel");
}

// What rnr_texture_mapper and rnr_texture_mapper_backward check alike, and what their parameter blocks share (levels: the block's
// textures or gradient levels).  No size bound on a level: both address texels with 64-bit offsets
template <class F>
static int texture_mapper_operands(const char* fn, TexMapCommon& p, F** levels, const float* uv_map, const float* sh, const void* other, const char* other_name,
                                   F* const* levels_host, const int* sizes, int num_levels, int C, int sh_start, int min_size, int N, int H, int W) {
    RNR_REQUIRE(uv_map && other && levels_host && sizes, "%s: null pointer argument", fn);
    RNR_REQUIRE(num_levels >= 1 && num_levels <= MAX_LEVELS && C > 0 && N > 0 && H > 0 && W > 0, "%s: bad sizes", fn);
    RNR_REQUIRE(!sh || (sh_start >= 0 && sh_start + 9 <= C), "%s: sh_start_ch + 9 > channels", fn);
    RNR_REQUIRE(aligned_to(4, {uv_map, sh, other}), "%s: uv_map, sh_basis_map and %s must be 4-byte aligned", fn, other_name);
    if (int e = fill_texture_levels(fn, levels, p.tex_size, levels_host, sizes, num_levels, C, 0, min_size)) return e;
    for (int l = 0; l < num_levels; l++) RNR_REQUIRE(aligned_to(4, {levels_host[l]}), "%s: texture level %d must be 4-byte aligned", fn, l);
    p.uv_map = uv_map; p.sh = sh; p.num_levels = num_levels; p.C = C; p.sh_start = sh_start; p.npix = (long)N * H * W; p.hw = H * W;
    return 0;
}

extern "C" int rnr_texture_mapper(const float* uv_map, const float* sh_basis_map, const float* const* textures_host,
                                  const int* tex_sizes_host, int num_levels, int tex_channels, int sh_start_ch,
                                  float* out, int num_views, int height, int width, void* stream) {
    TexMapParams P = {};
    if (int e = texture_mapper_operands("rnr_texture_mapper", P, P.tex, uv_map, sh_basis_map, out, "out", textures_host, tex_sizes_host,
                                        num_levels, tex_channels, sh_start_ch, 2, num_views, height, width))
        return e;
    P.out = out;
    hipLaunchKernelGGL(texture_mapper_kernel, grid256(P.npix * tex_channels), dim3(256), 0, as_stream(stream), P);
    return check_launch("texture_mapper_kernel");
}

// RNR_TEXTURE_BWD_FORM=a / b forces a form (scripts/texture_backward_time.py times both in one process); read on every call
static int texture_bwd_forced_form() {
    const char* e = getenv("RNR_TEXTURE_BWD_FORM");
    return !e ? 0 : (e[0] == 'a' || e[0] == 'A') ? 1 : (e[0] == 'b' || e[0] == 'B') ? 2 : 0;
}

extern "C" int rnr_texture_mapper_backward(const float* uv_map, const float* sh_basis_map, const float* grad_out,
                                           float* const* grad_textures_host, const int* tex_sizes_host, int num_levels,
                                           int tex_channels, int sh_start_ch, int num_views, int height, int width,
                                           void* stream) {
    TexMapBwdParams P = {};
    // a 1 x 1 level is a texture like any other to the adjoint
    if (int e = texture_mapper_operands("rnr_texture_mapper_backward", P, P.grad, uv_map, sh_basis_map, grad_out, "grad_out", grad_textures_host,
                                        tex_sizes_host, num_levels, tex_channels, sh_start_ch, 1, num_views, height, width))
        return e;
    P.g = grad_out; P.H = height; P.W = width;
    for (int l = 0; l < num_levels; l++)
        RNR_HIP(hipMemsetAsync(P.grad[l], 0, (size_t)P.tex_size[l] * P.tex_size[l] * tex_channels * sizeof(float), as_stream(stream)));
    // the tile form (7.53 against 8.09 ms on the bench scene at 16 x 512^2 with every channel live, 2.30 against 3.36 ms with the
    // six albedo channels alone: DESIGN.md 3.4d) wherever an image holds a whole 16 x 16 tile; one lane per (pixel, channel)
    // for smaller images, whose tiles would be mostly empty
    const int tiles_x = (width + TT - 1) / TT, tiles_y = (height + TT - 1) / TT;
    const long tiles = (long)num_views * tiles_x * tiles_y;
    const int forced = texture_bwd_forced_form();
    const bool tile_form = forced ? forced == 2 : (height >= TT && width >= TT);
    RNR_REQUIRE(tiles < ((long)1 << 31) && (P.npix + TB_PIX - 1) / TB_PIX < ((long)1 << 31), "rnr_texture_mapper_backward: too many pixels");
    if (tile_form) {
        hipLaunchKernelGGL(texture_mapper_bwd_tile_kernel, dim3((unsigned)tiles), dim3(256), 0, as_stream(stream), P, tiles_x, tiles_y);
        return check_launch("texture_mapper_bwd_tile_kernel");
    }
    hipLaunchKernelGGL(texture_mapper_bwd_kernel, dim3((unsigned)((P.npix + TB_PIX - 1) / TB_PIX)), dim3(256), 0, as_stream(stream), P);
    return check_launch("texture_mapper_bwd_kernel");
}

// What rnr_ray_renderer and rnr_ray_renderer_backward check alike, and the forward's operands in the parameter block.  The probe
// batch stays below 2^31 floats: ray_renderer_api_bwd_tiled_kernel addresses it with 32-bit offsets
static int ray_renderer_operands(const char* fn, RayApiParams& F, const float* rays_uv, const float* rays_lt, const float* lp, int lp_n, int lp_h,
                                 int lp_w, const float* alb_spec, const float* alb_diff, int C, int R, int n_diff, int no_albedo, int separate,
                                 float lp_scale, int N, int H, int W) {
    RNR_REQUIRE(rays_uv && rays_lt && lp && alb_spec, "%s: null pointer argument", fn);
    RNR_REQUIRE(R > n_diff && n_diff >= 0, "%s: bad ray counts", fn);
    RNR_REQUIRE(lp_n == 1 || lp_n == N, "%s: lp batch must be 1 or N", fn);
    RNR_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && lp_h > 0 && lp_w > 0, "%s: bad sizes", fn);
    RNR_REQUIRE((size_t)lp_n * lp_h * lp_w * C < ((size_t)1 << 31), "%s: probe batch of 2^31 floats or more", fn);
    RNR_REQUIRE(aligned_to(4, {rays_uv, rays_lt, lp, alb_spec, alb_diff}),
                "%s: rays_uv, rays_lt, lp, albedo_specular and albedo_diffuse must be 4-byte aligned", fn);
    F.rays_uv = rays_uv; F.rays_lt = rays_lt; F.lp = lp; F.alb_spec = alb_spec; F.alb_diff = alb_diff; F.lp_n = lp_n; F.lp_h = lp_h; F.lp_w = lp_w;
    F.C = C; F.R = R; F.n_diff = n_diff; F.no_albedo = no_albedo; F.separate = separate; F.lp_scale = lp_scale;
    F.npix = (long)N * H * W; F.hw = H * W;
    return 0;
}
// The tiled kernel where the shape allows (r05: 0.48 -> ms per 512^2 view in the drop-in loop), else the one with a lane per (pixel,
// channel); the launch is reported under the name of the kernel that ran
template <class P>
static int launch_ray_api(void (*tiled)(P), const char* tiled_name, void (*plain)(P), const char* plain_name, const P& p,
                          const RayApiParams& F, void* stream) {
    if (F.C <= RA_CH && F.R <= RA_MAX_RAYS) {        // LDS: the uv tile, then in its place the partial sums (RayTile)
        const size_t lds = sizeof(float) * (size_t)std::max(RA_PIX * (2 * F.R + 1), RA_QTR * 2 * RA_CH * RA_PIX);
        hipLaunchKernelGGL(tiled, dim3((unsigned)((F.npix + RA_PIX - 1) / RA_PIX)), dim3(RA_PIX * RA_QTR), lds, as_stream(stream), p);
        return check_launch(tiled_name);
    }
    hipLaunchKernelGGL(plain, grid256(F.npix * F.C), dim3(256), 0, as_stream(stream), p);
    return check_launch(plain_name);
}

extern "C" int rnr_ray_renderer(const float* rays_uv, const float* rays_lt, const float* lp, int lp_n, int lp_h,
                                int lp_w, const float* albedo_specular, const float* albedo_diffuse, int channels,
                                int num_rays, int num_ray_diffuse, int no_albedo, int seperate_albedo,
                                float lp_scale_factor, float* out, float* out_specular, float* out_diffuse,
                                float* ltt_specular, float* ltt_diffuse, float* rays_color, int num_views, int height,
                                int width, void* stream) {
    RNR_REQUIRE(out, "rnr_ray_renderer: null pointer argument");
    RayApiParams P = {};
    if (int e = ray_renderer_operands("rnr_ray_renderer", P, rays_uv, rays_lt, lp, lp_n, lp_h, lp_w, albedo_specular, albedo_diffuse,
                                      channels, num_rays, num_ray_diffuse, no_albedo, seperate_albedo, lp_scale_factor, num_views,
                                      height, width))
        return e;
    RNR_REQUIRE(aligned_to(4, {out, out_specular, out_diffuse, ltt_specular, ltt_diffuse, rays_color}),
                "rnr_ray_renderer: out, out_specular, out_diffuse, ltt_specular, ltt_diffuse and rays_color must be 4-byte aligned");
    P.out = out; P.out_spec = out_specular; P.out_diff = out_diffuse; P.ltt_spec = ltt_specular; P.ltt_diff = ltt_diffuse; P.rays_color = rays_color;
    return launch_ray_api(ray_renderer_api_tiled_kernel, "ray_renderer_api_tiled_kernel", ray_renderer_api_kernel,
                          "ray_renderer_api_kernel", P, P, stream);
}

extern "C" int rnr_ray_renderer_backward(const float* rays_uv, const float* rays_lt, const float* lp, int lp_n, int lp_h,
                                         int lp_w, const float* albedo_specular, const float* albedo_diffuse, int channels,
                                         int num_rays, int num_ray_diffuse, int no_albedo, int seperate_albedo,
                                         float lp_scale_factor, const float* g_out, const float* g_out_specular,
                                         const float* g_out_diffuse, const float* g_ltt_specular,
                                         const float* g_ltt_diffuse, const float* g_rays_color, float* grad_rays_lt,
                                         float* grad_albedo_specular, float* grad_albedo_diffuse, float* grad_lp,
                                         int num_views, int height, int width, void* stream) {
    RayApiBwdParams P = {};
    if (int e = ray_renderer_operands("rnr_ray_renderer_backward", P.F, rays_uv, rays_lt, lp, lp_n, lp_h, lp_w, albedo_specular,
                                      albedo_diffuse, channels, num_rays, num_ray_diffuse, no_albedo, seperate_albedo, lp_scale_factor,
                                      num_views, height, width))
        return e;
    RNR_REQUIRE(!grad_albedo_diffuse || albedo_diffuse, "rnr_ray_renderer_backward: grad_albedo_diffuse without albedo_diffuse");
    RNR_REQUIRE(aligned_to(4, {g_out, g_out_specular, g_out_diffuse, g_ltt_specular, g_ltt_diffuse, g_rays_color, grad_rays_lt,
                               grad_albedo_specular, grad_albedo_diffuse, grad_lp}),
                "rnr_ray_renderer_backward: the upstream gradients, grad_rays_lt, grad_albedo_specular, grad_albedo_diffuse and grad_lp "
                "must be 4-byte aligned");
    if (grad_lp) RNR_HIP(hipMemsetAsync(grad_lp, 0, (size_t)lp_n * lp_h * lp_w * channels * sizeof(float), as_stream(stream)));
    if (!grad_rays_lt && !grad_albedo_specular && !grad_albedo_diffuse && !grad_lp) return 0;
    P.g_out = g_out; P.g_out_spec = g_out_specular; P.g_out_diff = g_out_diffuse; P.g_ltt_spec = g_ltt_specular; P.g_ltt_diff = g_ltt_diffuse;
    P.g_rays_color = g_rays_color; P.grad_rays_lt = grad_rays_lt; P.grad_alb_spec = grad_albedo_specular; P.grad_alb_diff = grad_albedo_diffuse;
    P.grad_lp = grad_lp;
    return launch_ray_api(ray_renderer_api_bwd_tiled_kernel, "ray_renderer_api_bwd_tiled_kernel", ray_renderer_api_bwd_kernel,
                          "ray_renderer_api_bwd_kernel", P, P.F, stream);
}

extern "C" int rnr_ray_transport(const float* unet_raw, int c_out_pad, const float* bias, const float* net_in, int c_pad,
                                 const float* alpha, int num_spec, int num_diff, int albedo_diff_ch, int albedo_spec_ch,
                                 float* rays_uv, float* rays_lt, float* albedo_specular, float* albedo_diffuse,
                                 int num_views, int height, int width, void* stream) {
    RNR_REQUIRE(unet_raw && bias && net_in && alpha && rays_uv && rays_lt && albedo_specular && albedo_diffuse,
                "rnr_ray_transport: null pointer argument");
    RNR_REQUIRE(num_views > 0 && height > 0 && width > 0, "rnr_ray_transport: bad sizes");
    RNR_REQUIRE(aligned_to(16, {unet_raw, net_in}), "rnr_ray_transport: unet_raw and net_in must be 16-byte aligned");
    RNR_REQUIRE(aligned_to(4, {bias, alpha, rays_uv, rays_lt, albedo_specular, albedo_diffuse}),
                "rnr_ray_transport: bias, alpha, rays_uv, rays_lt, albedo_specular and albedo_diffuse must be 4-byte aligned");
    RayTransportParams P;
    // the lane layout of rnr_ray_render: 16 + 16 rays; no probe is read (the size arguments only pass the shared checks)
    if (int e = ray_launch_checks("rnr_ray_transport", num_spec, num_diff, 16, 2, 2, albedo_diff_ch, albedo_spec_ch, c_pad, &P.ni_need))
        return e;
    RNR_REQUIRE(c_out_pad % 4 == 0 && c_out_pad >= 3 * (num_spec + num_diff), "rnr_ray_transport: c_out_pad must be a multiple of 4 covering the rays");
    P.unet_raw = unet_raw; P.c_out_pad = c_out_pad; P.bias = bias; P.net_in = net_in; P.c_pad = c_pad; P.alpha = alpha;
    P.n_spec = num_spec; P.n_diff = num_diff; P.alb_diff_ch = albedo_diff_ch; P.alb_spec_ch = albedo_spec_ch;
    P.rays_uv = rays_uv; P.rays_lt = rays_lt; P.alb_spec = albedo_specular; P.alb_diff = albedo_diffuse;
    P.npix = (long)num_views * height * width; P.hw = height * width;
    const int R = num_spec + num_diff;
    const size_t lds = sizeof(float) * ((size_t)RR_WG_PIX * (size_t)(c_out_pad + P.ni_need + 2 * R) + (size_t)3 * R * (RR_WG_PIX + 1));
    RNR_REQUIRE(lds <= 64 * 1024, "rnr_ray_transport: rows too wide for the LDS staging (%zu bytes)", lds);
    hipLaunchKernelGGL(ray_transport_kernel, ray_grid(P.npix), dim3(256), lds, as_stream(stream), P);
    return check_launch("ray_transport_kernel");
}
