/*
 * rnr_hip.h — C ABI of librnr_hip.so: the MI355X (gfx950) implementation of the deferred-render hot path
 * of LansburyCH/relightable-nr (rasterize -> neural-texture sample -> SH basis -> RenderingNet U-Net ->
 * ray render).  Plain pointers and sizes only; no torch / ATen types.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless its name ends in `_host`;
 *   - tensors are dense, row-major, float32 / int32, in the layouts written next to each argument;
 *   - the CALLER allocates every output (and pre-fills it where the reference does, see each function);
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream, which is what the
 *     reference's <<<blocks, threads>>> launches use, rasterize_cuda_kernel.cu:615,629,670);
 *   - return value: 0 = success; non-zero = error, message available from rnr_last_error().
 *     Unlike the reference (which only printf()s kernel-launch failures, rasterize_cuda_kernel.cu:623-625)
 *     every launch is checked with hipGetLastError() and reported;
 *   - the device entry points only enqueue kernels on `stream` (no allocation, no host synchronisation, no
 *     hipMemset / hipMemcpy), so a sequence of calls can be captured into a HIP graph and replayed; no kernel uses
 *     scratch memory.
 *
 * Each entry point cites the reference interface it replaces (paths relative to /root/reference).
 */
#ifndef RNR_HIP_H
#define RNR_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RNR_ABI_VERSION 1

int rnr_abi_version(void);
/* Thread-local, NUL-terminated description of the last failing call on this thread ("" if none). */
const char* rnr_last_error(void);

/* =====================================================================================================
 * 1. neural_renderer.cuda.rasterize — drop-in for the pybind module (rasterize_cuda.cpp:124-191)
 * ===================================================================================================== */

/* Bytes of scratch rnr_forward_face_index_map needs for (batch, num_faces, image_size). */
size_t rnr_raster_workspace_bytes(int batch_size, int num_faces, int image_size);

/*
 * forward_face_index_map (rasterize_cuda.cpp:66-98 -> rasterize_cuda_kernel.cu:24-169, launch 595-650).
 *   faces          [B, nf, 3, 3]  (x_ndc, y_ndc, z_cam) per vertex
 *   face_index_map [B, is, is]    int32, caller pre-fills -1      (rasterize.py:50)
 *   weight_map     [B, is, is, 3] caller pre-fills 0              (rasterize.py:51)
 *   depth_map      [B, is, is]    caller pre-fills `far`          (rasterize.py:52)
 *   face_inv_map   [B, is, is, 3, 3] written when return_depth != 0 (may be NULL otherwise)
 *   faces_inv      [B, nf, 3, 3]  caller pre-fills 0              (rasterize.py:163)
 *   workspace      rnr_raster_workspace_bytes(B, nf, is) bytes of device scratch
 * Rows are in the extension's native order (row 0 = bottom of the image); the vertical flip is done by the
 * Python layer (rasterize.py:307-321).  Only covered pixels are written.  Results are bit-identical to the
 * reference kernels evaluated in IEEE binary32 without FMA contraction.
 */
int rnr_forward_face_index_map(const float* faces, int32_t* face_index_map, float* weight_map,
                               float* depth_map, float* face_inv_map, float* faces_inv,
                               int batch_size, int num_faces, int image_size, float near_, float far_,
                               int return_rgb, int return_alpha, int return_depth,
                               void* workspace, void* stream);

/*
 * forward_texture_sampling (rasterize_cuda.cpp:100-122 -> rasterize_cuda_kernel.cu:171-242, launch 652-691).
 *   textures [B, nf, ts, ts, ts, 3]; rgb_map [B, is, is, 3]; sampling_index_map [B, is, is, 8] int32;
 *   sampling_weight_map [B, is, is, 8].  Only covered pixels are written.
 */
int rnr_forward_texture_sampling(const float* faces, const float* textures, const int32_t* face_index_map,
                                 const float* weight_map, const float* depth_map, float* rgb_map,
                                 int32_t* sampling_index_map, float* sampling_weight_map,
                                 int batch_size, int num_faces, int image_size, int texture_size, float eps,
                                 void* stream);

/*
 * backward_pixel_map (rasterize_cuda.cpp:124-147 -> rasterize_cuda_kernel.cu:244-498, launch 693-732): gradient of
 * the rgb / alpha maps with respect to the NDC x,y of the face vertices (the silhouette sweep of Kato et al.).
 *   faces [B,nf,3,3]; face_index_map [B,is,is]; rgb_map / grad_rgb_map [B,is,is,3] (read when return_rgb);
 *   alpha_map / grad_alpha_map [B,is,is] (read when return_alpha); grad_faces [B,nf,3,3] caller pre-fills 0
 *   (rasterize.py:112): rows of front-facing faces are OVERWRITTEN, rows of back faces are left untouched.
 * Maps are in the extension's native row order.  Each gradient entry is accumulated by one thread in the
 * reference's order, so the result is bit-identical to the reference kernel run without FMA contraction.
 * No-op when both flags are 0 (rasterize.py:203-204).
 */
int rnr_backward_pixel_map(const float* faces, const int32_t* face_index_map, const float* rgb_map,
                           const float* alpha_map, const float* grad_rgb_map, const float* grad_alpha_map,
                           float* grad_faces, int batch_size, int num_faces, int image_size, float eps,
                           int return_rgb, int return_alpha, void* stream);

/*
 * backward_textures (rasterize_cuda.cpp:149-165 -> rasterize_cuda_kernel.cu:500-535, launch 734-763):
 *   grad_textures [B,nf,ts,ts,ts,3] += sampling_weight * grad_rgb at the 8 texels recorded by
 *   rnr_forward_texture_sampling (caller pre-fills 0, rasterize.py:114).  Float atomics: summation order is
 *   unspecified, as in the reference.
 */
int rnr_backward_textures(const int32_t* face_index_map, const float* sampling_weight_map,
                          const int32_t* sampling_index_map, const float* grad_rgb_map, float* grad_textures,
                          int batch_size, int num_faces, int image_size, int texture_size, void* stream);

/*
 * backward_depth_map (rasterize_cuda.cpp:167-189 -> rasterize_cuda_kernel.cu:537-592, launch 765-800): ADDS the
 * gradient of the depth map to grad_faces [B,nf,3,3] (called after rnr_backward_pixel_map, rasterize.py:145-152).
 *   depth_map [B,is,is]; face_inv_map [B,is,is,3,3] and weight_map [B,is,is,3] as written by
 *   rnr_forward_face_index_map(return_depth = 1); grad_depth_map [B,is,is].  Float atomics (pre-reduced per wave).
 */
int rnr_backward_depth_map(const float* faces, const float* depth_map, const int32_t* face_index_map,
                           const float* face_inv_map, const float* weight_map, const float* grad_depth_map,
                           float* grad_faces, int batch_size, int num_faces, int image_size, void* stream);

/*
 * neural_renderer.cuda.load_textures.load_textures (load_textures_cuda.cpp:20-34 -> load_textures_cuda_kernel.cu:6-152):
 * bake a texture image into the per-face texture cubes of the faces flagged in is_update.
 *   image [ih, iw, 3]; faces [nf, 3, 2] uv per face corner, WRAPPED IN PLACE (REPEAT 0 / MIRRORED_REPEAT 1 /
 *   CLAMP_TO_EDGE 2; CLAMP_TO_BORDER 3 leaves them and writes zero cubes); textures [nf, ts, ts, ts, 3] in/out;
 *   is_update [nf] int32.  The reference re-wraps the coordinates from every texel thread (a race when a coordinate is
 *   an exact integer); here each coordinate is wrapped once.
 */
int rnr_load_textures(const float* image, float* faces, float* textures, const int32_t* is_update, int num_faces,
                      int texture_size, int image_height, int image_width, int texture_wrapping, int use_bilinear,
                      void* stream);

/*
 * neural_renderer.cuda.create_texture_image.create_texture_image (create_texture_image_cuda.cpp:17-29 ->
 * create_texture_image_cuda_kernel.cu:8-163): lay the face cubes out as tiles of a texture atlas.
 *   vertices_all [nf, 3, 2] tile triangles in pixels (save_obj.py:10-24); textures [nf, tsi, tsi, tsi, 3];
 *   image [image_height, image_width, 3], tile grid width = int(sqrt(nf - 1)) + 1, tile size = image_width / that.
 *   Tiles beyond the last face are left as the caller filled them (the reference reads out of bounds there).
 */
int rnr_create_texture_image(const float* vertices_all, const float* textures, float* image, int num_faces,
                             int texture_size_in, int image_height, int image_width, float eps, void* stream);

/* =====================================================================================================
 * 2. Fused hot path (one view batch = N camera poses of one mesh)
 * ===================================================================================================== */

/*
 * Alignment of the operands of the shading and G-buffer entry points (this section's rnr_project_vertices ... rnr_shade_inputs,
 * rnr_ray_weights, rnr_ray_render, the layout helpers, the spherical-harmonics and resampling operators, and all of section 3):
 * every pointer operand needs the width of the widest access its kernel makes through it.  Unless the entry point's own
 * "Alignment:" line says otherwise that is its element's 4 bytes (float, int32_t); the operands named there are read or written
 * in 16-byte pieces and need 16-byte alignment.  HOST tables (textures_host, tex_sizes_host, pivots, rnr_mesh, rnr_gbuffer, rnr_rays)
 * are plain C arrays / structs; the device pointers they hold follow the same rule.  Every entry point checks this, and that its
 * sizes are positive, before any launch: a pointer that misses its alignment or a size <= 0 returns an error
 * (rnr_last_error names the entry point and the operands), and nothing is written (tests/test_gpu_shade_guard.py,
 * tests/test_gpu_gbuffer_guard.py).
 */

/*
 * nr.projection (neural_renderer/projection.py:6-53) for a shared mesh.
 *   vertices [nv, 3] world; K [N,3,3]; R [N,3,3]; t [N,3]; dist_coeffs [N,5] or NULL (= zeros);
 *   offset/scale [N,2] or both NULL; out [N, nv, 3] = (u_ndc, v_ndc, z_cam).
 * Alignment: every operand its element's 4 bytes.
 */
int rnr_project_vertices(const float* vertices, const float* K, const float* R, const float* t,
                         const float* dist_coeffs, const float* offset, const float* scale,
                         float* out, int num_views, int num_vertices, float orig_size, float eps,
                         void* stream);

/* Mesh description shared by the G-buffer kernels (all device pointers, int32 indices 0-based as produced
 * by load_obj.py:176-178).  Alignment: every array its element's 4 bytes. */
typedef struct rnr_mesh {
    const float* v;          /* [nv, 3] world positions (global_RT applied, network.py:127) */
    const float* vt;         /* [nvt, 2] */
    const float* vn;         /* [nvn, 3] (global_RT applied + normalised, network.py:128) */
    const int32_t* f_v_idx;  /* [nf, 3] */
    const int32_t* f_vt_idx; /* [nf, 3] */
    const int32_t* f_vn_idx; /* [nf, 3] */
    int num_vertices, num_texcoords, num_normals, num_faces;
} rnr_mesh;

/* Outputs of network.Rasterizer.forward (network.py:156-216) that are per-pixel maps; any pointer may be
 * NULL to skip that map.  Rows are already flipped (row 0 = top), as rasterize_rgbad returns them.
 * Alignment: every map its element's 4 bytes. */
typedef struct rnr_gbuffer {
    int32_t* face_index_map; /* [N,S,S]   -1 = background */
    float* alpha;            /* [N,S,S]   {0,1} */
    float* depth;            /* [N,S,S]   far on background */
    float* weight_map;       /* [N,S,S,3] perspective-corrected w'_k = w_k * depth / z_k (network.py:176-180) */
    float* raw_weight_map;   /* [N,S,S,3] the kernel's clamped+renormalised barycentrics */
    float* uv_map;           /* [N,S,S,2] wrapped to [0,1) (network.py:187-190) */
    float* normal_map;       /* [N,S,S,3] */
    float* normal_map_cam;   /* [N,S,S,3] */
    float* position_map;     /* [N,S,S,3] */
    float* position_map_cam; /* [N,S,S,3] */
} rnr_gbuffer;

size_t rnr_gbuffer_workspace_bytes(int num_views, int num_faces, int image_size);

/*
 * projected vertices -> per-face setup -> tiled z-resolve -> attribute interpolation, i.e.
 * renderer.py:244-257 + rasterize.py:255-340 + network.py:156-214 in one pass (no texture kernel: the hot
 * path feeds it an all-zero texture and discards rgb, network.py:140-142,157).
 *   v_uvz [N, nv, 3] from rnr_project_vertices; pose [N,4,4] (for the *_cam maps; may be NULL if unused).
 *   workspace: rnr_gbuffer_workspace_bytes(num_views, mesh->num_faces, image_size) bytes; nothing beyond them is touched.
 * Alignment: workspace is cleared in 16-byte pieces and holds 16-byte face records and 64-bit depth keys, each region a multiple
 * of 256 bytes from its start: it needs 16-byte alignment; the mesh arrays, v_uvz, pose and the maps of `out` their element's
 * 4 bytes.  Refused before any launch: a misaligned operand, num_views or image_size <= 0.
 */
int rnr_rasterize_gbuffer(const rnr_mesh* mesh, const float* v_uvz, const float* pose, int num_views,
                          int image_size, float near_, float far_, const rnr_gbuffer* out,
                          void* workspace, void* stream);

/* rnr_rasterize_gbuffer for a workspace whose per-call regions rnr_frame_prepare has already cleared on the same stream
 * (same arguments, same results; one launch fewer). */
int rnr_rasterize_gbuffer_prepared(const rnr_mesh* mesh, const float* v_uvz, const float* pose, int num_views,
                                   int image_size, float near_, float far_, const rnr_gbuffer* out,
                                   void* workspace, void* stream);

/*
 * The per-call preliminaries of a frame batch in ONE launch (test_rnr.py:283-300 per view: R / t from the pose, nr.projection;
 * render.get_TBN_map's per-face tangents, render.py:135-150; LightingSH.reconstruct_lp, network.py:622-627), plus the clearing
 * of the rnr_rasterize_gbuffer workspace.  Every part is optional (NULL output = skipped) and bit-identical to its
 * stand-alone entry point (rnr_project_vertices with R = pose[:, :3, :3], t = pose[:, :3, 3], no distortion / offset / scale;
 * rnr_face_tangents; rnr_sh_reconstruct):
 *   K [N,3,3], pose [N,4,4] -> v_uvz [N, nv, 3];   tangents [nf, 3];
 *   lp_basis [lp_samples, lp_num_basis], lp_coeff [lp_num_basis, lp_channels] -> light_probe [lp_samples, lp_channels];
 *   gbuffer_workspace: an rnr_gbuffer_workspace_bytes(num_views, mesh->num_faces, image_size) buffer -> cleared for
 *   rnr_rasterize_gbuffer_prepared.
 * Alignment: gbuffer_workspace is cleared in 16-byte pieces and needs 16-byte alignment; every other operand its element's
 * 4 bytes.  The two cleared regions (bin counters to 0, depth keys to ~0) lie in the MIDDLE of the workspace's layout, each
 * followed by a region the rasterizer fills: the clear does not end at rnr_gbuffer_workspace_bytes, and an over-long clear
 * would damage no neighbour of the buffer — tests/test_gpu_gbuffer_guard.py reads the workspace back instead.
 */
int rnr_frame_prepare(const rnr_mesh* mesh, const float* K, const float* pose, int num_views, int image_size, float eps,
                      float* v_uvz, float* tangents, const float* lp_basis, const float* lp_coeff, float* light_probe,
                      int lp_samples, int lp_num_basis, int lp_channels, void* gbuffer_workspace, void* stream);

/* Per-face unit tangents of render.get_TBN_map (render.py:135-150); static per mesh.  out [nf,3].
 * Alignment: the mesh arrays and out their element's 4 bytes. */
int rnr_face_tangents(const rnr_mesh* mesh, float* out, void* stream);

/* Ray-sampler constants (network.RaySampler buffers `pivots_dir`, network.py:441-443), HOST pointers. */
typedef struct rnr_rays {
    const float* pivots_spec_host; /* [3, num_spec] */
    const float* pivots_diff_host; /* [3, num_diff] */
    int num_spec, num_diff;        /* <= 32 each */
} rnr_rays;

/*
 * G-buffer -> RenderingNet input, fusing render.get_TBN_map (render.py:152-166), camera.get_view_dir_map
 * (camera.py:5-32), the tangent-space view direction (test_rnr.py:314-315), the lmax=2 SH basis
 * (sph_harm.py:41-71), TextureMapper.forward (network.py:67-91 + misc.py:5-42), both RaySamplers
 * (network.py:445-472) and the channel assembly of test_rnr.py:349-356.
 *   textures[level] [S_l, S_l, C] (level sizes tex_sizes_host[level]); num_levels <= 8
 *   net_in  [N, H, W, Cpad] channel-last; channel order 3*(num_spec+num_diff) ray dirs (ray-major), normal (3),
 *           view_dir (3), neural texture (C); channels >= Cin are zero-filled
 *   rays_uv [N, H, W, 2, num_spec+num_diff] or NULL; neural_img [N, C, H, W] or NULL (API copies)
 *   sh_basis_map [N,H,W,9] or NULL (written when non-NULL)
 * Alignment: net_in is written, and every texture level read, in 16-byte pieces (four channels of a pixel / a texel): net_in and
 * each textures_host[level] need 16-byte alignment — what every view n > 0 of net_in has, c_pad being a multiple of 4, and every
 * texel, tex_channels being one; every other operand its element's 4 bytes.  Refused before any launch: a misaligned operand,
 * num_views, height, width or num_faces <= 0.
 */
int rnr_shade_inputs(const int32_t* face_index_map, const float* alpha, const float* uv_map,
                     const float* normal_map, const float* face_tangents, int num_faces,
                     const float* proj_inv, const float* R_inv,
                     const float* const* textures_host, const int* tex_sizes_host, int num_levels,
                     int tex_channels, int sh_start_ch, const rnr_rays* rays,
                     float* net_in, int c_pad, float* rays_uv, float* neural_img, float* sh_basis_map,
                     int num_views, int height, int width, void* stream);

/* ---- U-Net convolution stack (pytorch_prototyping.py:96-277, 370-536), channel-last activations ---- */

enum { RNR_ACT_NONE = 0, RNR_ACT_LRELU02 = 1, RNR_ACT_RELU = 2 };
enum { RNR_CONV3x3_REFLECT = 0, RNR_CONV4x4S2_REFLECT = 1, RNR_CONVT4x4S2 = 2 };

/* One input source of a convolution: a raw (pre-normalisation) channel-last tensor plus the per-view,
 * per-channel affine + activation the producer's BatchNorm/bias/activation implies:
 *     value(n,h,w,c) = act(scale[n,c] * raw[n,h,w,c] + shift[n,c]).
 * scale/shift NULL = identity.  Two sources = torch.cat([src0, src1], 1) (pytorch_prototyping.py:429).
 * Non-finite values PROPAGATE through every activation: act(v) is computed as max(v, slope * v) with slope 1 / 0.2 / 0, and a NaN
 * v makes both operands NaN — RNR_ACT_RELU does not turn a NaN into 0, in any kernel family (direct, Winograd, emulated), so a
 * non-finite raw value (or scale / shift) surfaces in out_raw where "Non-finite inputs" below says
 * (tests/test_gpu_conv_guard.py; UNetPlan's check_finite = 'first' relies on it).
 * Alignment of the convolution entry points' operands: the channel-strided tensors (data, scale, shift, out_raw, ray_w, stats,
 * the packed weight, workspace) are read and written in 16-byte pieces and need 16-byte alignment — what every view n > 0 or row
 * slice of a channel-last tensor has, its stride being a multiple of 16 channels (64 bytes); gamma, beta, bias, the unpacked
 * weight and image need their element's 4 bytes, tile_mask none; only `sync` asks for more (256, see rnr_conv2d_fused). */
typedef struct rnr_conv_src {
    const float* data;  /* [N, H, W, channels] */
    const float* scale; /* [N, channels] or NULL */
    const float* shift; /* [N, channels] or NULL */
    int channels;       /* multiple of 4 */
    int act;            /* RNR_ACT_* */
} rnr_conv_src;

/* Static description of one convolution of the U-Net.  Channel counts `*_pad` are the channel strides of the
 * channel-last tensors (multiples of 16; padding channels hold zeros / meet zero weights). */
typedef struct rnr_conv_desc {
    int kind;                 /* RNR_CONV3x3_REFLECT | RNR_CONV4x4S2_REFLECT | RNR_CONVT4x4S2 */
    int c_in0, c_in0_pad;     /* first source: live channels, channel stride */
    int c_in1, c_in1_pad;     /* second source of a skip concat (0, 0 if none) */
    int c_out, c_out_pad;     /* live output channels, channel stride of out_raw (multiple of 16) */
    int flags;                /* RNR_CONV_* bits, 0 by default */
} rnr_conv_desc;
/* `stats` already holds zeros when rnr_conv2d is called (rnr_bn_finalize_reset left them so): skip the memset. */
#define RNR_CONV_STATS_PREZEROED 1
/* fp32 emulation on the bf16 matrix cores: every operand is split exactly into three bf16 terms and the six leading
 * partial products are accumulated in fp32 by v_mfma_f32_32x32x16_bf16 (error of the order of fp32's own rounding,
 * 2.7x fewer MFMA cycles).  Must be set both when packing the weights and when convolving; layers it does not cover
 * (maps narrower than 16 pixels or of odd shape) run the fp32 MFMA kernels from the same buffer.  Range: finite operands below
 * 2^127 (the leading bf16 term of a larger value rounds to infinity).  The split is exact down to |x| = 2^-110; below, residual
 * terms under 2^-126 are bf16 subnormals, which gfx950 keeps (conversion and MFMA; a grid of 2^-133) rather than flushes: an
 * operand x then enters as x +- 2^-134 at the worst, |out - x w| <= 2^-126 |w| whatever a device does with them — precision
 * below 1e-38 (tests/test_gpu_conv_emu_terms.py, class R). */
#define RNR_CONV_F32_EMU_BF16X6 2
/* fp32 emulation on the fp16 matrix cores: every operand is split into TWO fp16 terms (22 significand bits, relative
 * representation error <= 2^-23) and the three leading partial products (hh, hl, lh) are accumulated in fp32 by
 * v_mfma_f32_32x32x16_f16: 5.3x fewer MFMA cycles than the exact-fp32 kernel, half of bf16x6.  Measured error against a
 * float64 convolution is below the exact-fp32 kernel's on every U-Net layer shape it covers (fewer accumulator roundings outweigh
 * the two missing significand bits; tests/test_gpu_unet.py).  Weights are pre-scaled per layer by a power of two at pack
 * time (2^k, k = min(12 - floor(log2 max |w|), 40), which brings max |w| into [2^12, 2^13), undone exactly in the epilogue; a
 * layer whose max |w| is below 2^-28 keeps fewer fp16 bits, and weights more than 2^-26 below the layer's largest keep fewer
 * bits as fp16 subnormals), so any finite weights are fine, up to FLT_MAX (k = -115); activations must satisfy
 * |act(scale * x + shift)| < 65504 — true for BatchNorm outputs and bounded network inputs; values below 2^-14 keep an
 * absolute precision of 2^-25 (fp16 subnormals are honoured by the MFMA).  Same packing / fallback rules as BF16X6;
 * the two flags are mutually exclusive. */
#define RNR_CONV_F32_EMU_F16X3 4
#define RNR_CONV_F32_EMU_ANY (RNR_CONV_F32_EMU_BF16X6 | RNR_CONV_F32_EMU_F16X3)
/* Half-precision operands on the fp16 matrix cores.  NOT an emulation of fp32: every activation act(scale * x + shift) and every
 * prescaled weight is rounded ONCE to fp16 (round-to-nearest-even, fp16 subnormals kept) and the products, each exact in fp32,
 * are accumulated in fp32 by v_mfma_f32_32x32x16_f16 — one MFMA where F16X3 issues three, 16 x fewer MFMA cycles than the
 * exact-fp32 kernel.  Relative error 2^-11 per operand, i.e. |out - conv(x, w)| <= ((1 + 2^-11)^2 - 1) sum |x w| plus the fp32
 * accumulation's rounding (tests/test_gpu_conv_f16.py, class D); a U-Net's tanh output keeps >= 50 dB PSNR against the fp32 one
 * (tests/test_gpu_unet_f16.py).  Weights take F16X3's per-layer power-of-two prescale — the same 2^k, k = min(12 - floor(log2
 * max |w|), 40), undone exactly in the epilogue — so any finite weights are fine, up to FLT_MAX; a layer whose max |w| is below
 * 2^-28, and weights more than 2^-26 below the layer's largest, are fp16 subnormals on the 2^-24 grid of the prescaled value and
 * keep fewer bits.  Range of the activations: magnitudes below 65520 round to a finite fp16 (at most 65504); anything larger
 * becomes infinite and surfaces in out_raw per "Non-finite inputs" of the direct kernels (the outputs whose window contains it);
 * values below 2^-14 lie on the 2^-24 grid (fp16 subnormals, honoured by conversion and MFMA), |x| <= 2^-25 enters as 0.  The
 * weight image is ONE fp16 plane behind the fp32 image (rnr_packed_weight_floats = f32 + 16 + ceil(f32 / 2)).  Same packing /
 * fallback rules as F16X3: set when packing AND convolving, tile and split-K plans are F16X3's on every shape, shapes the 16-bit
 * kernels do not cover run the fp32 MFMA kernels from the same buffer (exactly), rnr_conv_algorithm reports 0, refused wherever
 * the emulation flags are.  Mutually exclusive with both emulation flags and with RNR_CONV_WINOGRAD*; a flag of its own, outside
 * RNR_CONV_F32_EMU_ANY. */
#define RNR_CONV_F16 256
/* Winograd minimal filtering (Lavin & Gray 2016): F(2x2, 3x3) for the 3x3 convolutions — 16 multiplications per 2 x 2
 * output tile instead of 36 — and F(2x2, 2x2) for the two 4x4 stride-2 convolutions, which are sums of 2x2-tap correlations
 * (per input parity phase resp. per output parity class) — 9 instead of 16.  fp32 operands and fp32 accumulation on
 * v_mfma_f32_32x32x2_f32 like the direct kernels; the data transforms only add (F(2x2, 3x3) also halves weights), so the
 * result differs from the direct convolution by rounding of the order of a different summation order (scripts/wino_check.py,
 * tests/test_gpu_unet.py: max error against a float64 convolution <= 1.1e-5 of the output rms on every U-Net layer shape,
 * direct <= 8.6e-6).  Must be set both when packing the weights (the transformed image is stored behind the direct one) and
 * when convolving; calls it does not cover (maps that do not tile into 16 x 8 / 16 x 16 pixels, column counts that are not
 * multiples of 64 / 128, masked launches, too few tiles to fill the chip: rnr_conv_algorithm tells) run the direct kernels
 * from the same buffer.  Not combined with the emulation flags.  Non-finite inputs: the data transforms take differences of
 * neighbouring pixels, so an inf / NaN activation reaches every output of the 2 x 2 tiles whose patch contains it (a direct
 * convolution confines it to the outputs whose window contains it).  F(2x2, 3x3): tile (t, u) = outputs (2t .. 2t + 1,
 * 2u .. 2u + 1), patch = the reflection-padded input rows 2t - 1 .. 2t + 2, columns 2u - 1 .. 2u + 2.  F(2x2, 2x2)
 * (rnr_conv_algorithm 2) works per parity, 3 x 3 patches:
 *   stride 2: per input parity phase (py, px), tile (t, u) = outputs (2t .. 2t + 1, 2u .. 2u + 1), patch = the padded input
 *     pixels (2r - py, 2c - px), r = 2t .. 2t + 2, c = 2u .. 2u + 2 (reflected: -1 -> 1, H -> H - 2); an input pixel lies in
 *     exactly one phase and may reach the tiles whose patch of THAT phase contains it;
 *   transposed: per output parity class (py, px), tile (t, u) = the outputs (2y + py, 2x + px), y = 2t .. 2t + 1,
 *     x = 2u .. 2u + 1, patch = the input pixels (2t + py - 1 .. 2t + py + 1, 2u + px - 1 .. 2u + px + 1) inside the map; an
 *     input pixel may reach, in each of the four classes, the tiles whose patch in that class contains it.
 * In every case the outputs whose own window contains the pixel DO become non-finite; the rest of those tiles may. */
#define RNR_CONV_WINOGRAD 8
/* (with RNR_CONV_WINOGRAD) F(4x4, 3x3) for the 3x3 convolutions whose maps tile into 32 x 16 pixels, whose columns into 64s and
 * whose grid fills the chip: 36 multiplications per 4 x 4 outputs (2.25 per output; F(2x2, 3x3): 4, direct: 9) on the
 * interpolation points (0, +-3/4, +-3/2, inf).  A flag of its own because the larger transforms (coefficients up to 3.375) put the
 * rounding error at ~4.5 x the direct form's (rms; F(2x2, 3x3): 1.3 x) — scripts/experiments/winograd_accuracy_study.py,
 * tests/test_gpu_unet.py: <= 1e-4 of the output peak against a float64 convolution on every U-Net layer shape.  The Python host
 * layer (rnr_amd.unet.UNetPlan) sets it BY DEFAULT since r04 (conv_algo 'winograd4'); a C caller chooses per descriptor.
 * Non-finite inputs: an inf / NaN activation reaches every output of the 4 x 4 tiles whose 6 x 6 input patch contains it
 * (F(2x2, .): 2 x 2 tiles of a 4 x 4 patch; direct: the outputs whose window contains it).  The F(4x4, 3x3) weight image is stored behind the F(2x2, 3x3) one (both flags when packing AND
 * convolving); shapes it does not cover run F(2x2, 3x3) / direct from the same buffer.  rnr_conv_algorithm reports 4. */
#define RNR_CONV_WINOGRAD4 16
/* (with RNR_CONV_WINOGRAD) F(4x4, 2x2) for the transposed 4x4 stride-2 convolutions whose input maps tile into 32 x 16 pixels,
 * whose columns into 64s, whose input channels (both sources, padded) number at most 1024 and whose grid fills the chip: every
 * output parity class as 25 multiplications per 4 x 4 outputs (1.5625 per output; F(2x2, 2x2): 2.25, direct: 4) on the
 * interpolation points (0, +-3/4, 2, inf).  A flag of its own for the same reason as RNR_CONV_WINOGRAD4: the larger transforms round more
 * (a float32 study of the point set: rms error ~3.8 x the direct form's, F(2x2, 2x2) 2.3 x, scripts/experiments/winograd_accuracy_study.py);
 * the kernel measures 2.5 x the direct kernels' rms error and 2.5 x F(2x2, 2x2)'s on the U-Net's transposed layer shapes, at most 7.1e-6 of
 * the output peak against a float64 convolution (profiles/r07_winograd_f4x4_2x2_accuracy.txt; tests bound it at 1e-4).
 * Non-finite inputs: an inf / NaN activation reaches, in each parity class, every output of the 4 x 4 tiles whose 5 x 5 input
 * patch contains it.  The 25-plane weight image is stored behind the F(2x2, 2x2) one (both flags when packing AND convolving);
 * shapes it does not cover run F(2x2, 2x2) / direct from the same buffer.  rnr_conv_algorithm reports 2 for both forms (Winograd on
 * the 2x2-tap decomposition); rnr_conv_winograd_tile tells them apart (4 / 2). */
#define RNR_CONV_WINOGRAD42 32
/* (with RNR_CONV_WINOGRAD) F(4x4, 3x3) for the 3x3 OUT LAYER: 65 - 80 output channels in 80 padded columns, which
 * RNR_CONV_WINOGRAD4's 64-column tiles do not cover.  Taken when the map tiles into 16 x 16 pixels, the input channels (both
 * sources, padded) number at most 1024 and the grid gives every CU a workgroup (256 tiles; RNR_WINO80F4_MIN_WGS in the
 * environment); everything else runs the out layer's F(2x2, 3x3) kernel / the direct kernels from the same packed buffer (the
 * 36-plane image is stored behind the F(2x2, 3x3) one: both flags when packing AND convolving).  Same algorithm, interpolation
 * points and rounding behaviour as RNR_CONV_WINOGRAD4 (tests bound the error at 1e-4 of the output peak against a float64
 * convolution); a flag of its own because callers that pass RNR_CONV_WINOGRAD | RNR_CONV_WINOGRAD4 with 80 columns rely on the
 * 16 x 4 tiles of the F(2x2, 3x3) kernel.  Non-finite inputs: an inf / NaN activation reaches every output of the 4 x 4 tiles
 * whose 6 x 6 patch contains it.  rnr_conv_algorithm keeps reporting 3 (the out layer's Winograd kernels, both take a tile
 * mask); rnr_conv_winograd_tile tells them apart (4 / 2), and rnr_conv_tile_count / rnr_conv_active_tiles then describe
 * 16 x 16 pixel tiles. */
#define RNR_CONV_WINOGRAD4_OUT 64
/* (with RNR_CONV_WINOGRAD) F(4x4, 2x2) for the 4x4 stride-2 CONVOLUTIONS (RNR_CONV4x4S2_REFLECT; RNR_CONV_WINOGRAD42 is the
 * transposed ones' and is ignored by this kind): taken when the OUTPUT map tiles into 32 x 16 pixels, the columns into 64s, the
 * input channels (both sources, padded) number at most 1024, the 25-plane weight image stays below 2^31 bytes and the grid gives
 * every CU a workgroup (256 tiles; RNR_WINO42S_MIN_WGS in the environment).  The four input parity phases of a 4 x 4 output tile
 * cost 25 multiplications each where F(2x2, 2x2) takes 36; same interpolation points and rounding behaviour as
 * RNR_CONV_WINOGRAD42 (tests bound the error at 1e-4 of the output peak against a float64 convolution).  Everything else runs
 * F(2x2, 2x2) / the direct kernels from the same packed buffer (the 25-plane image, 6.25 x the direct one, is stored behind the
 * F(2x2, 2x2) image: both flags when packing AND convolving).  Non-finite inputs: an inf / NaN activation reaches every output
 * of the 4 x 4 tiles whose 5 x 5 patch of a phase image contains it.  rnr_conv_algorithm keeps reporting 2;
 * rnr_conv_winograd_tile tells the two forms apart (4 / 2). */
#define RNR_CONV_WINOGRAD42S 128

/* Floats in the packed weight of `d` ([taps][c_in0_pad + c_in1_pad][c_out_pad], x4 parity classes for convT). */
size_t rnr_packed_weight_floats(const rnr_conv_desc* d);
/* PyTorch layout -> packed.  Conv2d weight [c_out, c_in0 + c_in1, kh, kw] (pytorch_prototyping.py:116, 250-268);
 * ConvTranspose2d weight [c_in0 + c_in1, c_out, 4, 4] (pytorch_prototyping.py:154-159). */
int rnr_pack_conv_weight(const rnr_conv_desc* d, const float* weight, float* packed, void* stream);

/* Size limits of the forward convolutions (rnr_conv2d, rnr_conv2d_masked, rnr_conv2d_fused, rnr_conv2d_ray,
 * rnr_conv_active_tiles).  A call beyond one of them fails with "too large" and the limit BEFORE anything is launched; the
 * host queries below answer such sizes with their error value (rnr_conv_algorithm / rnr_conv_winograd_tile: -1;
 * rnr_conv_tile_count, rnr_conv_workspace_bytes, rnr_conv_sync_bytes: 0).  With OH x OW the output map:
 *   H * W < 2^31                          pixels of one view (the 32-bit pixel index)
 *   N * H * W < 2^31, N * OH * OW < 2^31  GEMM rows and output pixels of the call (int)
 *   workgroups of the launch < 2^31       (pixel tiles x column tiles x parity classes x K slices; binds only beyond 65536 columns)
 *   64 * OW * c_out_pad * 4 < 2^31        bytes of 64 output rows: the 32-bit store offsets behind a tile's first pixel
 *   N * c_out_pad < 2^24                  statistics entries (32-bit byte offsets into the eight statistics shards)
 *   rnr_packed_weight_floats(d) * 4 < 2^31  the packed weight (read with 32-bit byte offsets; rnr_pack_conv_weight refuses it too)
 * Buffers themselves may be of any size: views, output tiles and split-K slabs are addressed from 64-bit bases (tested with
 * input and output buffers beyond 4 GiB).  INSIDE one source view the halo and Winograd kernels use a 32-bit byte offset:
 * a source view of 2^31 bytes or more (H * W * c_in_pad * 4 of the larger source) runs the gather kernel (direct, algorithm
 * 0, no tile mask: rnr_conv_tile_count is 0) whatever Winograd flags the descriptor carries — exact fp32 — and, since that
 * kernel has no 16-bit form, a call with RNR_CONV_F32_EMU_* or RNR_CONV_F16 on such a view is refused ("no 16-bit-format kernel
 * for a source view of ... bytes").  A view of exactly 2^31 bytes (2048 x 2048 x 128) is already outside: the hardware would
 * lose its last dword. */

/* Which algorithm rnr_conv2d* runs for (desc, N, input H, input W): 0 = direct implicit GEMM, 1 = Winograd F(2x2, 3x3),
 * 3 = the same for the 80-column out layer (16 x 16 x 4 MFMA tiles; with RNR_CONV_WINOGRAD4_OUT it may run F(4x4, 3x3) under the
 * same code: rnr_conv_winograd_tile), 2 = Winograd F(2x2, 2x2) (16 multiplications per 2 x 2
 * outputs instead of 36, resp. 9 instead of 16; with RNR_CONV_WINOGRAD42 the transposed convolution may run F(4x4, 2x2) under the
 * same code: rnr_conv_winograd_tile), 4 = Winograd F(4x4, 3x3) (RNR_CONV_WINOGRAD4); -1 = bad arguments.
 * Non-zero only with RNR_CONV_WINOGRAD in desc->flags.
 * Masked launches (tile_mask != NULL) run 0 unless the plan is 3; rnr_conv2d_ray always runs 0. */
int rnr_conv_algorithm(const rnr_conv_desc* d, int num_views, int in_h, int in_w);
/* The output tile edge m of the Winograd algorithm F(m x m, r x r) that rnr_conv2d* runs for the same call: 0 = direct, 2 = F(2x2, 3x3)
 * / F(2x2, 2x2), 4 = F(4x4, 3x3) / F(4x4, 2x2); -1 = bad arguments.  Multiplications per output and tap set follow from it: (m + r - 1)^2
 * per m^2 outputs with r = 3 for the 3x3 convolution and r = 2 for the 2x2-tap correlations of the 4x4 stride-2 ones. */
int rnr_conv_winograd_tile(const rnr_conv_desc* d, int num_views, int in_h, int in_w);

/* Scratch bytes rnr_conv2d may need for (desc, N, input H, input W) (split-K partial slabs). */
size_t rnr_conv_workspace_bytes(const rnr_conv_desc* d, int num_views, int in_h, int in_w);

/*
 * out_raw[n,ho,wo,co] = sum_{taps,ci} value(src)[...] * weight  (no bias: it is folded into the consumer's
 * `shift`, or applied by rnr_ray_render / rnr_nhwc_to_nchw for the last layer).  When stats != NULL the call
 * also zeroes and then accumulates per-view, per-channel sum / sum-of-squares of out_raw into
 * stats [N, c_out_pad, 2] (float64), for the batch-statistics BatchNorm the reference runs at inference
 * (test_rnr.py:229-233).
 *   src0/src1: `channels` must equal c_in0_pad / c_in1_pad; src1 may be NULL when c_in1_pad == 0.
 *   out_raw [N, Ho, Wo, c_out_pad]  (Ho,Wo = H,W | H/2,W/2 | 2H,2W by kind)
 * Reproducibility: out_raw is bit-reproducible run to run (fixed summation order, also across split-K slabs); `stats` is
 * NOT — every workgroup adds its column sums with one float64 atomicAdd per channel, whose order varies, so the last
 * bits of the statistics (and of everything normalised with them) may differ between runs (tests compare at 1e-5).
 */
int rnr_conv2d(const rnr_conv_desc* d, const rnr_conv_src* src0, const rnr_conv_src* src1,
               const float* weight_packed, float* out_raw, double* stats, int num_views, int in_h, int in_w,
               void* workspace, size_t workspace_bytes, void* stream);

/*
 * Output-tile masking for a convolution whose output is consumed only where a mask is set — the out layer of
 * RenderingNet: the ray renderer zeroes every background pixel (rays_uv = -1 there, network.py:469-470, 497), so the
 * out-layer activations of all-background pixel tiles are never read.
 *   rnr_conv_tile_count   number of pixel tiles rnr_conv2d launches for (desc, N, H, W); 0 if that convolution cannot
 *                         be masked (only 3x3 convolutions on the LDS-halo plan without split-K can);
 *   rnr_conv_active_tiles tile_mask[t] = 1 iff any alpha [N,H,W] > 0 inside tile t;
 *   rnr_conv2d_masked     rnr_conv2d that leaves out_raw of tiles with tile_mask[t] == 0 untouched.  stats must be NULL
 *                         (batch statistics need every pixel).  tile_mask == NULL is rnr_conv2d.
 */
size_t rnr_conv_tile_count(const rnr_conv_desc* d, int num_views, int in_h, int in_w);
int rnr_conv_active_tiles(const rnr_conv_desc* d, const float* alpha, uint8_t* tile_mask, int num_views, int in_h,
                          int in_w, void* stream);
int rnr_conv2d_masked(const rnr_conv_desc* d, const rnr_conv_src* src0, const rnr_conv_src* src1,
                      const float* weight_packed, float* out_raw, double* stats, int num_views, int in_h, int in_w,
                      void* workspace, size_t workspace_bytes, const uint8_t* tile_mask, void* stream);

/*
 * The convolution of the product path (rnr_amd.unet.UNetPlan): rnr_conv2d_masked plus what the reference runs as separate
 * passes behind it — the train-mode BatchNorm2d that follows the convolution (pytorch_prototyping.py:117-120, 250-268,
 * 154-161; per-view batch statistics, test_rnr.py:229-233) — inside ONE launch:
 *   bn != NULL && bn->gamma != NULL: the workgroups add the per-view, per-channel sum / sum of squares of out_raw into
 *     statistics shards inside `sync`; the last workgroup of a view to arrive turns them into
 *       scale[n,c] = gamma[c] / sqrt(var_biased + eps),  shift[n,c] = beta[c] - mean * scale[n,c]   (rnr_bn_finalize)
 *     and leaves the shards at zero.  Channels >= c_out of scale / shift get 0.
 *   split-K (small maps): the slices write partial-output slabs into `workspace` that the reduce kernel adds in slice
 *     order; a BatchNorm finalise launch follows it.  Grids of one workgroup per CU or fewer also finalise in a launch of
 *     their own.
 * `sync` (rnr_conv_sync_bytes(d, max_views, in_h, in_w) bytes, 256-byte aligned): arrival counters and statistics.  The
 * caller zero-fills it ONCE; every call expects zeros and leaves zeros, also for a different num_views <= max_views.  One
 * buffer per convolution in flight (calls on the same stream may share one).  After a failed launch: zero it again.
 * Run-to-run reproducibility: the statistics are double-precision atomics whose order varies between runs.  What a workgroup
 * adds is a sum of six to twelve float32 lane sums (<= 28 significant bits), so the double additions are EXACT — hence
 * order-independent — as long as the non-zero partial sums of a channel and view span less than ~2^17 in magnitude (53 - 28 - log2(number
 * of workgroups) bits of headroom for 512 workgroups per view); that is the case for activations of any trained network and is why 16 000 frame groups have
 * come out bit-identical run after run (scripts/t_fused_stress.py), but it is a property of the data, not of the code: with a wider
 * spread scale / shift — and everything downstream — may differ in the last bits between runs, exactly like rnr_conv2d +
 * rnr_bn_finalize.
 */
/* ZERO-INITIALISE this struct (`rnr_conv_bn bn = {0};` / memset) before filling it: it has grown (running_mean, running_var,
 * momentum were added in r05) and carries no size field — a caller compiled against the five-field form that leaves the tail
 * uninitialised hands garbage running_* pointers to rnr_conv2d_fused, i.e. a wild device write when num_views == 1. */
typedef struct rnr_conv_bn {
    const float* gamma; /* [c_out] BatchNorm weight; NULL = no BatchNorm behind this convolution */
    const float* beta;  /* [c_out] */
    float* scale;       /* [N, c_out_pad] out */
    float* shift;       /* [N, c_out_pad] out */
    float eps;
    /* torch.nn.BatchNorm2d's train-mode side effect (pytorch_prototyping.py:109, test_rnr.py:229-233 keep the layers in train mode):
     * running = (1 - momentum) * running + momentum * (batch mean | unbiased batch variance), [c_out] float32, updated in place by
     * the launch that finalises the statistics.  Statistics are per VIEW in this entry point and torch pools the whole batch, so
     * the two agree for num_views == 1 only: non-NULL pointers with num_views > 1 are refused (use rnr_conv2d +
     * rnr_bn_finalize_batch there).  NULL = no update. */
    float* running_mean;
    float* running_var;
    float momentum;
} rnr_conv_bn;
size_t rnr_conv_sync_bytes(const rnr_conv_desc* d, int max_views, int in_h, int in_w);
int rnr_conv2d_fused(const rnr_conv_desc* d, const rnr_conv_src* src0, const rnr_conv_src* src1,
                     const float* weight_packed, float* out_raw, const rnr_conv_bn* bn, int num_views, int in_h, int in_w,
                     void* workspace, size_t workspace_bytes, void* sync, size_t sync_bytes, const uint8_t* tile_mask,
                     void* stream);

/*
 * The ray renderer folded into the out layer (opt-in: RNRPipeline(fuse_ray=True); network.py:253, 481-527, test_rnr.py:357-368).
 *   rnr_ray_weights  the half that does not depend on the U-Net: for pixel p, ray r, colour channel c
 *                        ray_w[p, 3 r + c] = albedo_group(r)[p, c] * env-map colour(direction of ray r)[c] / rays in the group
 *                    from the ray directions / albedo channels of net_in and the light probe (same arithmetic as
 *                    rnr_ray_render); background pixels (alpha = 0) and the padding columns >= 3 * rays get 0.
 *                    ray_w [N, H, W, c_w], c_w = the out layer's c_out_pad.
 *   rnr_conv2d_ray   the out-layer convolution whose epilogue produces the FRAME instead of its 78-channel output:
 *                        image[n, c, y, x] = sum_r (tanh(conv[n, y, x, 3 r + c] + bias[3 r + c]) + 1) * ray_w[n, y, x, 3 r + c]
 *                    straight from the MFMA accumulators (LDS transpose, 26 columns per sum): 12 bytes per pixel leave the
 *                    kernel instead of 320.  Only the exact-fp32 3x3 convolution on the 80-column plan (65 <= c_out <= 80,
 *                    c_out = 3 x rays, map width a multiple of 32, height of 8); anything else returns an error — run
 *                    rnr_conv2d_masked + rnr_ray_render there.  tile_mask as in rnr_conv2d_masked (skipped tiles get 0), laid
 *                    out for the DIRECT plan's 32 x 8-pixel tiles: RNR_CONV_WINOGRAD in d->flags is ignored by this entry
 *                    point, so build the mask with rnr_conv_active_tiles / rnr_conv_tile_count from the descriptor with
 *                    that flag cleared (with it set those describe the Winograd out layer's 16 x 4-pixel tiles).  A map whose
 *                    direct grid would split K (fewer than 257 tiles) runs unsplit here but takes no mask: rnr_conv_tile_count is 0.
 *                    bias [c_out_pad] — NOT [3 * rays] as for rnr_ray_render: the kernel loads the bias of all 80 columns of its
 *                    tile; entries >= c_out reach no output, whatever they hold.
 *                    ray_w [N, H, W, c_out_pad] as written by rnr_ray_weights; a pixel whose weights are all 0 gives exactly 0.
 * Differs from rnr_ray_render in summation order only (<= 1e-6 on frames in [0, 2]).
 * Alignment of rnr_ray_weights' operands: net_in is read and ray_w written in 16-byte pieces (whole rows of a workgroup's pixels,
 * c_pad and c_w being multiples of 4): both need 16-byte alignment; alpha and lp their element's 4 bytes.  Refused before any
 * launch: a misaligned operand, num_views, height or width <= 0, rows too wide for the 64 KiB LDS staging
 * (32 * (staged net_in floats + c_w) floats).
 */
int rnr_ray_weights(const float* net_in, int c_pad, const float* alpha, const float* lp, int lp_h, int lp_w, int num_spec,
                    int num_diff, int albedo_diff_ch, int albedo_spec_ch, float* ray_w, int c_w, int num_views, int height,
                    int width, void* stream);
int rnr_conv2d_ray(const rnr_conv_desc* d, const rnr_conv_src* src0, const rnr_conv_src* src1, const float* weight_packed,
                   const float* ray_w, const float* bias, float* image, int num_views, int in_h, int in_w,
                   const uint8_t* tile_mask, void* stream);

/* stats [N,c_pad,2] (sum, sumsq over `count` pixels) + gamma/beta [channels] -> scale/shift [N,c_pad]:
 * scale = gamma / sqrt(var_biased + eps), shift = beta - mean * scale  (BatchNorm2d in train mode: per-view
 * batch statistics, biased variance); channels >= `channels` get scale = shift = 0. */
int rnr_bn_finalize(const double* stats, const float* gamma, const float* beta, float* scale, float* shift,
                    int num_views, int channels, int c_pad, double count, float eps, void* stream);
/* rnr_bn_finalize that also resets stats to zero once consumed, so that the next rnr_conv2d into the same statistics
 * buffer can run with RNR_CONV_STATS_PREZEROED (no memset launch per layer). */
int rnr_bn_finalize_reset(double* stats, const float* gamma, const float* beta, float* scale, float* shift,
                    int num_views, int channels, int c_pad, double count, float eps, void* stream);

/* Whole-batch variant: torch's train-mode BatchNorm2d reduces over (N,H,W) of the call (the reference forces that mode
 * at inference, test_rnr.py:229-233; with its N = 1 per call the two coincide).  The per-view partial sums of
 * rnr_conv2d are added over the `num_views` views (count = num_views * count_per_view), the same scale/shift is
 * written to every view, and — when the pointers are non-NULL — running_mean / running_var [channels] are updated as
 * torch does: running = (1 - momentum) * running + momentum * {mean, UNBIASED variance}.  Resets stats to zero. */
int rnr_bn_finalize_batch(double* stats, const float* gamma, const float* beta, float* scale, float* shift,
                          float* running_mean, float* running_var, float momentum, int num_views, int channels,
                          int c_pad, double count_per_view, float eps, void* stream);

/* ---- U-Net backward (train_rnr.py:376 optimises RenderingNet's 22 convolutions and 17 BatchNorms): exact fp32 only ----
 *
 * Per layer, with y the raw convolution output, v = a[n,c] * y + b[n,c] (BatchNorm's scale / shift, or identity / bias) and
 * z = act(v) what the consumers read (rnr_conv_src), the backward runs
 *   rnr_conv_out_backward          g_z (the sum over the consumers of z) -> g_y, g_gamma / g_beta or g_bias
 *   rnr_conv2d_weight_backward     g_y, the layer's sources -> grad_weight
 *   per source s: rnr_conv2d(rnr_conv_backward_desc(d, s)) on g_y, then rnr_conv2d_input_backward_ring -> the gradient of s's z
 * No entry point of this section uses atomics: every output is bit-reproducible run to run (the data gradient inherits
 * rnr_conv2d's reproducibility, called with stats == NULL).  Emulation flags (RNR_CONV_F32_EMU_*) in a descriptor are refused.
 * Alignment: the channel-last tensors and per-view vectors rnr_conv_out_backward and rnr_conv2d_weight_backward take (y, scale,
 * shift, g_z0, g_z1, g_y; the sources' data / scale / shift) are read and written in 16-byte pieces and need 16-byte alignment,
 * like the forward's; `saved` needs its element's 8 bytes; gamma, g_gamma, g_beta, grad_weight, the unpacked weight, and every
 * operand of rnr_conv2d_input_backward_ring and rnr_unet_out_backward (moved one float at a time) their element's 4 bytes.  The
 * workspaces: as stated with each entry point.  No entry point reads or writes outside the extents stated here
 * (tests/test_gpu_unet_backward_guard.py).
 */

/* rnr_bn_finalize_reset (whole_batch == 0: one group per view, running_mean / running_var must be NULL) or rnr_bn_finalize_batch
 * (whole_batch != 0: one group for the call) that also writes what the backward needs:
 *   saved [groups, c_pad, 2] float64 = (mean, 1 / sqrt(var_biased + eps)) of every group; channels >= `channels` get (0, 0).
 * scale / shift, the running statistics and the reset of stats are those entry points', bit for bit. */
int rnr_bn_finalize_saved(double* stats, const float* gamma, const float* beta, float* scale, float* shift,
                          float* running_mean, float* running_var, float momentum, double* saved, int whole_batch,
                          int num_views, int channels, int c_pad, double count_per_view, float eps, void* stream);

/* BatchNorm modes of rnr_conv_out_backward: statistics per view (UNetPlan's 'batch'), over the whole call (torch's train mode,
 * 'batch_all'), or the running statistics (eval mode, 'running'). */
enum { RNR_BN_BWD_BATCH = 0, RNR_BN_BWD_BATCH_ALL = 1, RNR_BN_BWD_RUNNING = 2 };

/*
 * Activation + BatchNorm (or bias) backward of one layer, in two launches (reduce, apply).
 *   y [N,h,w,c_pad] raw convolution output; scale / shift [N,c_pad] the affine its consumers apply (NULL = 1 / 0); act RNR_ACT_*;
 *   g_z0 [N,h,w,c_pad] upstream gradient of z, g_z1 the second consumer's (NULL = none), added to it;
 *   gamma [channels] BatchNorm weight, NULL = no BatchNorm behind this convolution; mode RNR_BN_BWD_* (ignored without gamma);
 *   saved [groups,c_pad,2] float64 (mean, 1 / sqrt(var + eps)): as rnr_bn_finalize_saved wrote it (groups = N for
 *   RNR_BN_BWD_BATCH, 1 for RNR_BN_BWD_BATCH_ALL), or the running statistics in that form (1 group) for RNR_BN_BWD_RUNNING.
 * With g_v = (g_z0 + g_z1) * (v > 0 ? 1 : slope), slope 0.2 / 0 / 1 (torch's convention at v == 0), and per group of m pixels
 *   S1 = sum g_v,  S2 = sum g_v y,  D = r (S2 - mu S1)        (float64; (mu, r) from saved):
 *   train modes   g_beta = sum over groups S1, g_gamma = sum over groups D, g_y = gamma r (g_v - S1/m - (y - mu) r D/m), evaluated
 *                 in float64 per element and rounded once;
 *   running       g_beta = S1, g_gamma = D (one group: the call), g_y = scale * g_v;
 *   no BatchNorm  g_beta = S1 (the bias gradient), g_y = g_v; g_gamma is not written.
 * Outputs: g_y [N,h,w,c_pad], channels >= `channels` exactly 0; g_gamma, g_beta [channels] float32, OVERWRITTEN (either may be
 * NULL: not wanted).  The sums are float64 over per-workgroup partials in `workspace`, added in workgroup order.
 * workspace: rnr_conv_out_backward_workspace_bytes(N, h, w, c_pad) bytes, 8-byte aligned.  c_pad: a multiple of 16, <= 1024.
 */
size_t rnr_conv_out_backward_workspace_bytes(int num_views, int h, int w, int c_pad);
int rnr_conv_out_backward(const float* y, const float* scale, const float* shift, int act, const float* g_z0,
                          const float* g_z1, const float* gamma, const double* saved, int mode, float* g_y,
                          float* g_gamma, float* g_beta, int num_views, int h, int w, int channels, int c_pad,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ---- Dropout2d in train mode (network.py:236-247 builds the U-Net with use_dropout = True, train_rnr.py:398-405 trains with it on) ----
 *
 * Dropout2d multiplies a whole channel of one view by m[n,c] in {0, 1 / (1 - p)}.  LeakyReLU and ReLU are positively homogeneous
 * and m >= 0, so m act(a y + b) = act((m a) y + m b): a dropped layer hands its consumers (rnr_conv_src, the weight gradient,
 * the data gradient) the tables (m a, m b) instead of (a, b), and only rnr_conv_out_backward's arithmetic changes
 * (rnr_conv_out_backward_dropout).  Alignment: mult and the scale / shift tables are read and written in 16-byte pieces and need
 * 16-byte alignment; extents are the [num_views, c_pad] rows stated with each entry point, nothing outside them is touched.
 */
#define RNR_DROPOUT_MAX_LAYERS 32
typedef struct rnr_dropout_layer {
    float* mult;            /* [N, c_pad] device, written: the multipliers of this layer */
    int channels, c_pad;    /* live channels; c_pad a multiple of 16 */
    float p;                /* drop probability, 0 <= p <= 1 */
} rnr_dropout_layer;

/*
 * One launch draws the multipliers of every layer of a plan.  layers: HOST array of num_layers <= RNR_DROPOUT_MAX_LAYERS entries.
 * With C_total = sum of c_pad and cbase_l = sum of c_pad over the layers before l (array order; layers with p = 0 included),
 * element (n, l, c) has index i = n C_total + cbase_l + c (view-major: the masks of view n do not depend on num_views) and takes
 * word i & 3 of Philox4x32-10 on counter (lo32 b, hi32 b, 0, 0x524E5244), key (lo32 seed, hi32 seed), b = (uint64)offset + (i >> 2)
 * (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85; seed and offset are 64-bit patterns passed as
 * int64_t).  u = (word >> 8) 2^-24, keep = u >= p in float32, mult = keep ? 1.0f / (1.0f - p) : 0; p = 1 gives 0 everywhere
 * without a division, p = 0 exactly 1; channels >= `channels` get 0.  Rows >= num_views of mult are not written.
 * More than RNR_DROPOUT_MAX_LAYERS layers, a p outside [0, 1] or a c_pad that is not a multiple of 16 is an error before any launch.
 */
int rnr_dropout_draw(const rnr_dropout_layer* layers, int num_layers, int num_views, int64_t seed, int64_t offset, void* stream);

/* The consumers' tables of one dropped layer: scale_out = mult * scale, shift_out = mult * shift (scale NULL = 1, shift NULL = 0),
 * one float32 product each, all [N, c_pad]; scale_out == scale and shift_out == shift (in place) are allowed; rows >= num_views
 * are untouched.  c_pad: a multiple of 4. */
int rnr_dropout_affine(const float* scale, const float* shift, const float* mult, float* scale_out, float* shift_out,
                       int num_views, int c_pad, void* stream);

/*
 * rnr_conv_out_backward for a layer whose consumers read z = mult[n,c] act(a y + b): mult [N,c_pad] (NULL = none: then this IS
 * rnr_conv_out_backward, bit for bit).  scale / shift are the tables the consumers applied, (mult a, mult b); the sign of
 * v' = scale y + shift is taken from them — the function the forward evaluated — and
 *   g_v = mult[n,c] (g_z0 + g_z1) (v' > 0 ? 1 : slope),
 * the sum in float32 as in rnr_conv_out_backward; the factor mult (v' > 0 ? 1 : slope) is formed in float64 (exact) and applied
 * after the conversion to float64: no float32 rounding beyond the sum's.  (rnr_conv_out_backward rounds the slope product to
 * float32.  Here a view that drops a channel contributes zeros to a whole-batch group, S1 and D are left to the other views'
 * terms, and that rounding is no longer small against 16 roundings of the result's own terms; a table of ones is therefore not
 * bitwise mult = NULL.)  S1, S2, D, g_beta, g_gamma and the train-mode g_y are rnr_conv_out_backward's formulas on that
 * g_v; RNR_BN_BWD_RUNNING: g_y = gamma r g_v with r from `saved`, in float64, rounded once (scale holds mult and cannot be used);
 * no BatchNorm: g_y = (float)g_v.  No atomics, bit-reproducible.  Workspace and limits as rnr_conv_out_backward.
 */
int rnr_conv_out_backward_dropout(const float* y, const float* scale, const float* shift, const float* mult, int act,
                                  const float* g_z0, const float* g_z1, const float* gamma, const double* saved, int mode,
                                  float* g_y, float* g_gamma, float* g_beta, int num_views, int h, int w, int channels,
                                  int c_pad, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Weight gradient of rnr_conv2d for the three kinds and one or two sources:
 *   grad_weight[co, ci, tap] = sum over views and output pixels o of  g_y[n, o, co] * value(src)[n, pad(o, tap), ci]
 * with value() the consumer-side value of rnr_conv_src, recomputed from raw + scale / shift / act while staging, exactly as the
 * forward stages it.  (in_h, in_w), d, src0, src1 as given to rnr_conv2d; g_y [N,Ho,Wo,c_out_pad].
 * grad_weight is written in torch's layout — [c_out, c_in0 + c_in1, k, k], or [c_in0 + c_in1, c_out, 4, 4] for RNR_CONVT4x4S2
 * — live channels only, OVERWRITTEN.  An implicit GEMM on v_mfma_f32_32x32x2_f32 with M = output channels, N = input channels
 * of one tap and K = pixels; K is split over pixel ranges so that the grid fills the chip, every range writes a partial slab
 * into `workspace` and a second launch adds the slabs in range order: no float atomics, bit-reproducible.
 * A non-finite g_y or source value surfaces in exactly the (co, ci, tap) whose sum holds a term with it: for RNR_CONVT4x4S2 a tap
 * that falls outside the output map at some pixel has no term there, and the source value of that pixel does not enter it.
 * workspace: rnr_conv2d_weight_backward_workspace_bytes(d, N, in_h, in_w) bytes, 16-byte aligned.
 */
size_t rnr_conv2d_weight_backward_workspace_bytes(const rnr_conv_desc* d, int num_views, int in_h, int in_w);
int rnr_conv2d_weight_backward(const rnr_conv_desc* d, const rnr_conv_src* src0, const rnr_conv_src* src1,
                               const float* g_y, float* grad_weight, int num_views, int in_h, int in_w,
                               void* workspace, size_t workspace_bytes, void* stream);

/*
 * The data gradient of a convolution is one of the forward kernels run on g_y, except on a border ring:
 *   RNR_CONV3x3_REFLECT    rnr_conv2d of the same kind with W'[ci, co, ky, kx] = W[co, ci, 2 - ky, 2 - kx]; it reflects g_y where the
 *                          adjoint wants zero and lacks the fold of the padding: rows {0, 1, H-2, H-1} and columns {0, 1, W-2, W-1};
 *   RNR_CONV4x4S2_REFLECT  RNR_CONVT4x4S2 with the forward weight read as [in, out, 4, 4]; lacks the fold: rows {1, H-2}, columns
 *                          {1, W-2};
 *   RNR_CONVT4x4S2         RNR_CONV4x4S2_REFLECT with the forward weight read as [out, in, 4, 4]; reflects where zero is wanted:
 *                          rows {0, H-1}, columns {0, W-1}.
 * rnr_conv_backward_desc fills the descriptor of that convolution for source `source` (0 / 1) of forward descriptor d: one
 * source of c_out (c_out_pad) channels — g_y, no affine, RNR_ACT_NONE —, c_in_s (c_in_s_pad) output columns, and the forward's
 * algorithm choice: RNR_CONV_WINOGRAD if d has it, plus the F(4x4, .) flag of the gradient's own kind, under that flag's
 * column rule, if d has any of them.  Its weight (sliced on the input-channel axis for two sources) is packed with
 * rnr_pack_conv_weight like any other.
 * rnr_conv2d_input_backward_ring then OVERWRITES the ring pixels of grad_in [N,H,W,c_in_s_pad] (H, W = the forward's input map)
 * with the exact adjoint, the defining sum over the (output pixel, tap) pairs that read the pixel, as an fmaf chain over
 * (co, oy, ky, ox, kx) in that order; padding channels of those pixels get 0.  weight: the FORWARD weight in torch's layout,
 * all sources.  Correct for every size the forward accepts, including H = 2 and H = 3 where the fold rows coincide.
 */
int rnr_conv_backward_desc(const rnr_conv_desc* d, int source, rnr_conv_desc* out);
int rnr_conv2d_input_backward_ring(const rnr_conv_desc* d, int source, const float* g_y, const float* weight,
                                   float* grad_in, int num_views, int in_h, int in_w, void* stream);

/* Adjoint of rnr_nhwc_to_nchw: g_raw[n,h,w,c] = g_out[n,c,h,w] * (apply_tanh ? 1 - out[n,c,h,w]^2 : 1), out the forward's result;
 * g_raw [n,h,w,c_pad] with channels >= c exactly 0.  (The bias gradient is rnr_conv_out_backward's g_beta on g_raw.) */
int rnr_unet_out_backward(const float* g_out, const float* out, int apply_tanh, float* g_raw, int n, int c, int h,
                          int w, int c_pad, void* stream);

/* Layout helpers for the drop-in RenderingNet.forward (NCHW in / NCHW out).  Alignment: every operand its element's 4 bytes;
 * n, c, h, w <= 0 are refused before any launch. */
int rnr_nchw_to_nhwc(const float* in, float* out, int n, int c, int h, int w, int c_pad, void* stream);
/* out[n,c,h,w] = f(in[n,h,w,c] + bias[c]) with bias optional (NULL) and f = tanhf when apply_tanh != 0 */
int rnr_nhwc_to_nchw(const float* in, float* out, const float* bias, int apply_tanh,
                     int n, int c, int h, int w, int c_pad, void* stream);

/*
 * Last stage of a frame: out-layer bias + tanh (network.py:253), rays_lt = (y*0.5+0.5)*2
 * (test_rnr.py:357-359) and RayRenderer.forward (network.py:481-527) with seperate_albedo=True:
 * equirect uv of every ray from the ray directions stored in net_in, bilinear env-map taps
 * (network.py:497 + misc.py:5-42), light-transport weighted sums / num rays, times the albedos.
 *   unet_raw [N,H,W,c_out_pad] raw output of the out-layer conv (78 live channels, ray-major RGB)
 *   bias [3*(num_spec+num_diff)]; net_in as written by rnr_shade_inputs; alpha [N,H,W]
 *   lp [Hl, Wl, 3] environment map (LightingSH.reconstruct_lp, network.py:622-627)
 *   image [N,3,H,W]
 * Read: of unet_raw the first 3 * (num_spec + num_diff) columns, of net_in the ray directions (channels < 3 rays), normal / view
 * (the next 6) and the two albedo triples; whole rows are staged in 16-byte pieces, so the other columns and channels are loaded
 * but reach no output, whatever they hold.  On a background pixel (alpha == 0) the unet_raw row and the ray directions reach no
 * output either (the ray sums are set to 0 by select: rnr_conv2d_masked leaves skipped tiles unwritten), but the two albedo
 * triples are still multiplied with those zero sums, as RayRenderer.forward's albedo * ltt is (network.py:515-522): they must
 * be finite there, as rnr_shade_inputs writes them.  A workgroup of 32 pixels that are all background reads neither tensor.
 * Alignment: unet_raw and net_in are read in 16-byte pieces and need 16-byte alignment; bias, alpha, lp and image their
 * element's 4 bytes.  Refused before any launch: a misaligned operand, num_views, height or width <= 0.
 */
int rnr_ray_render(const float* unet_raw, int c_out_pad, const float* bias, const float* net_in, int c_pad,
                   const float* alpha, const float* lp, int lp_h, int lp_w, int num_spec, int num_diff,
                   int albedo_diff_ch, int albedo_spec_ch, float* image, int num_views, int height,
                   int width, void* stream);

/*
 * The frame as the reference script presents it (test_rnr.py:376-393): 8-bit, channel-last, optionally composited over the
 * light-probe background the object stands in front of (--save_img_bg), in ONE launch behind rnr_ray_render / rnr_conv2d_ray.
 *   image [N,3,H,W] (may be NULL for RNR_PRESENT_BACKGROUND); alpha [N,H,W], read by RNR_PRESENT_COMPOSITE only;
 *   proj_inv / R_inv [N,3,3] and lp [lp_h, lp_w, 3] (ONE probe, lp_h, lp_w >= 1, fewer than 2^24 floats): unused by
 *   RNR_PRESENT_FRAME (may be NULL / 0 there);
 *   out [N,H,W,3] uint8, row 0 = top as the frame already is; channel order B, G, R (what cv2.imwrite is given,
 *   test_rnr.py:377), or R, G, B with RNR_PRESENT_RGB or-ed into mode.
 *     RNR_PRESENT_FRAME       out = q(image)
 *     RNR_PRESENT_BACKGROUND  out = q(background)
 *     RNR_PRESENT_COMPOSITE   out = alpha > 0 ? q(image) : q(background)      (a NaN alpha shows the background)
 *   q(v) = saturate_u8(round_half_even(v * 255.0f)): one float32 product; NaN -> 0, +inf -> 255, -inf -> 0.  This is what
 *   cv::Mat::convertTo(CV_8U) does to the float array the script hands to imwrite; no test compares with cv2:
 *   parity with OpenCV is unpinned (as for rnr_resize_area).
 *   background = rnr_env_background's formula, computed only for the pixels that show it, with the fused path's arithmetic
 *   (v_rsq normalisation, polynomial atan2 / acos, FMA blend — as rnr_ray_render's env-map taps): within float rounding of
 *   rnr_env_background (tests/test_gpu_present.py derives the bound), same column on the seam z = +-0, same row at the poles.
 * out needs no alignment.  When H * W is a multiple of 4, out is 4-byte aligned and the planes the mode reads (image, alpha)
 * are 16-byte aligned, a thread handles four pixels (float4 loads, 12 bytes stored as three dwords); otherwise one pixel per
 * thread with byte stores.  The bytes are the same either way.  Errors (unknown mode, a NULL pointer the mode reads, lp_h or
 * lp_w < 1, sizes <= 0) are reported before any launch.
 */
enum { RNR_PRESENT_FRAME = 0, RNR_PRESENT_COMPOSITE = 1, RNR_PRESENT_BACKGROUND = 2 };
#define RNR_PRESENT_RGB 8            /* or-ed into mode: channel order R,G,B instead of cv2's B,G,R */
int rnr_present_u8(const float* image, const float* alpha, const float* proj_inv, const float* R_inv,
                   const float* lp, int lp_h, int lp_w, int mode, uint8_t* out,
                   int num_views, int height, int width, void* stream);

/*
 * The score of frames against photographs: the twelve per-view numbers of metric.compute_err_metrics (metric.py:19-84), for
 * N views in three launches (sums and box per band of rows; SSIM per tile of 32 x 32 windows; one finaliser per view).
 *   est, gt [N,3,H,W] (layout RNR_METRIC_PLANAR) or [N,H,W,3] (RNR_METRIC_CHANNELS_LAST); neither is written (the reference
 *   zeroes its arguments in place outside the mask);
 *   mask [N,H,W]: a pixel is valid where mask == 1 exactly (metric.py:29; 0.5 and NaN are not valid); NULL = every pixel valid;
 *   every value is x = float32(v * scale) (ONE float32 product, as the reference's callers do with `* 255.0`; scale = 1 for
 *   inputs already on the 0..255 scale) where the pixel is valid and 0 elsewhere — a select, so a NaN or an infinity outside
 *   the mask never enters the arithmetic — then widened to double: all moments and sums are float64, no atomics, and two
 *   calls on the same inputs give bit-identical outputs;
 *   out [N,12] float64 in the order of the enum below; box [N,5] int32 (xmin, xmax+1, ymin, ymax+1, count) of the mask, may
 *   be NULL; workspace: rnr_image_metrics_workspace_bytes(N, H, W) bytes, 8-byte aligned like out, every word that is read
 *   is written earlier in the same call.
 * With d = x_est - x_gt, S1 = sum |d|, S2 = sum d^2 over the three channels:
 *     mae = S1 / (3 H W)        mae_bb = S1 / (3 box area)        mae_valid = S1 / (3 count);     mse* likewise from S2;
 *     psnr* = 100 if mse* / 255^2 < 1e-10 else -10 log10(mse* / 255^2);
 *     ssim: per channel a separable 11-tap Gaussian (sigma 1.5, float64 weights exp(-k^2/4.5) / sum) as a VALID convolution of
 *       X, Y, X^2, Y^2, XY; C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2;
 *       map = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1) * (2 s12 + C2) / (s1^2 + s2^2 + C2); mean over the map and the channels.
 *       This is the definition pytorch_msssim.ssim(X, Y, data_range=255, size_average=False) documents; that library is not
 *       available here and no test compares with it: parity with pytorch_msssim is unpinned (as with OpenCV above);
 *     ssim_bb: the same on the crop to the box = the mean of the image's map over the windows that lie inside the box
 *       (top-left corner in [ymin, ymax+1-10) x [xmin, xmax+1-10));
 *     ssim_valid = ssim_bb: metric.py:79-82 copies ground truth over estimate pixels outside the mask, which both are 0 already.
 * Edge cases: an empty mask gives box = 0 0 0 0 0, NaN in the six _bb / _valid error outputs and the two box SSIMs, and the
 * whole-image outputs as usual (0, 0, 100, 1 for equal images); H < 11 or W < 11 gives ssim = NaN, a box side below 11
 * ssim_bb = ssim_valid = NaN; compute_ssim == 0 skips the SSIM launch and gives NaN in the three SSIM outputs; a NaN inside a
 * view's mask propagates to that view's outputs only.  Errors (NULL est, gt, out or workspace; sizes <= 0;
 * N * 3 * H * W >= 2^31; unknown layout; misaligned out or workspace) are reported before any launch.
 */
enum { RNR_METRIC_PLANAR = 0, RNR_METRIC_CHANNELS_LAST = 1 };
enum { RNR_METRIC_MAE = 0, RNR_METRIC_MAE_BB, RNR_METRIC_MAE_VALID, RNR_METRIC_MSE, RNR_METRIC_MSE_BB, RNR_METRIC_MSE_VALID,
       RNR_METRIC_PSNR, RNR_METRIC_PSNR_BB, RNR_METRIC_PSNR_VALID, RNR_METRIC_SSIM, RNR_METRIC_SSIM_BB, RNR_METRIC_SSIM_VALID };
size_t rnr_image_metrics_workspace_bytes(int num_views, int height, int width);
int rnr_image_metrics(const float* est, const float* gt, const float* mask, int layout, float scale,
                      int compute_ssim, double* out, int32_t* box, void* workspace,
                      int num_views, int height, int width, void* stream);

/*
 * The two per-pixel terms of train_rnr.py's objective (csrc/loss.hip), each a streaming pass plus a one-workgroup finalise
 * forward and one streaming pass backward.  Inputs and gradients are float32; the per-pixel arithmetic and every sum are
 * float64 and a gradient is rounded to float32 once (the reference's float32 `1 - c . mh` cancels to 1.7e-5 relative on
 * gradient elements where the chromaticities agree, which is where training converges to).  No atomics and fixed-order sums:
 * two calls on the same inputs give the same bits.  Every workspace word that is read is written earlier in the same call.
 * Nothing syncs with the host: the backward passes read g_loss (one float32) and the forward's loss_out from device memory.
 *
 * Ray chromaticity loss (network.RaysLTChromLoss, network.py:391-411):
 *   rays_lt [N,R,3,H,W], alpha [N,1,H,W], img [N,3,H,W] or NULL.  With x_r the 3-vector of ray r at a pixel and
 *   eps = 1e-12 (F.normalize's default):
 *     n_r = |x_r|;  c_r = x_r / max(n_r, eps);  S = sum_r c_r;  m = S / R;  M = |m|;  mh = m / max(M, eps)
 *     w = min(20 |img|, 1)  (1 when img is NULL; a NaN stays NaN);   d_r = (1 - c_r . mh) alpha w
 *     loss = sum d / sum alpha / R,   the per-pixel sum taken as sum_r d_r = alpha w (R - S . mh)
 *   loss_out [2] float64: loss, sum alpha.  The optional float32 maps (each written only when its pointer is not NULL; all
 *   NULL is the training call and never forms them): chrom [N,R,3,H,W] = c_r, chrom_mean [N,1,3,H,W] = mh,
 *   chrom_diff [N,R,H,W] = d_r.  workspace: rnr_rays_chrom_loss_workspace_bytes(N, R, H, W) bytes, 8-byte aligned like loss_out.
 *   Backward, with g = *g_loss, k = g alpha w / (sum alpha R):
 *     t    = (S - (S . mh) mh) / M / R   if M >= eps,    else S / eps / R
 *     gc   = -k (mh + t)                                  (the same for every ray of the pixel)
 *     gx_r = (gc - (gc . c_r) c_r) / n_r  if n_r >= eps,  else gc / eps
 *   grad_rays_lt [N,R,3,H,W] is overwritten; c, S and mh are recomputed from rays_lt (at R = 26 the pixel's 78 values stay in
 *   registers between the two sweeps, at other ray counts the second sweep reads them again).
 *   Edge cases: a pixel with alpha w == 0 contributes exactly 0, gets an exactly zero gradient and exactly zero chrom_diff, and
 *   its rays are not read by the training call — a select, so a NaN ray under alpha = 0 does not reach the loss (DEVIATION: the
 *   reference multiplies, so there such a NaN poisons the loss); sum alpha == 0 gives loss = NaN as in the reference, the
 *   gradient is then unspecified; a zero or sub-eps ray, and M < eps, follow the formulas above, which is what torch's
 *   normalize and its autograd give (the gradient at a zero ray is of order k / eps).  Errors (a NULL required pointer,
 *   N, H, W < 1, R < 1, N R 3 H W >= 2^31, misaligned loss_out or workspace) are reported before any launch.
 *
 * Cropped L1 (train_rnr.py:564-569, 581-585): est, gt [N,C,H,W], alpha [N,1,H,W], b = border >= 0:
 *     loss = mean over N C (H - 2b) (W - 2b) of |fl32(est alpha) - fl32(gt alpha)|     on the crop [b, H-b) x [b, W-b)
 *   (the two products rounded to float32 as the reference rounds them, then widened); loss_out [1] float64;
 *   workspace: rnr_masked_l1_loss_workspace_bytes(N, H, W) bytes, 8-byte aligned.
 *   Backward: grad_est [N,C,H,W] = g sign(fl32(est alpha) - fl32(gt alpha)) alpha / count inside the crop, sign(0) = 0, and
 *   exactly 0 in the border; gt and alpha get no gradient.
 *   Errors: as above, C < 1, N C H W >= 2^31, border < 0, and H <= 2b or W <= 2b (DEVIATION: the reference's mean over an
 *   empty crop is NaN).
 */
size_t rnr_rays_chrom_loss_workspace_bytes(int num_views, int num_rays, int height, int width);
int rnr_rays_chrom_loss(const float* rays_lt, const float* alpha, const float* img, double* loss_out, float* chrom,
                        float* chrom_mean, float* chrom_diff, void* workspace, int num_views, int num_rays, int height,
                        int width, void* stream);
int rnr_rays_chrom_loss_backward(const float* rays_lt, const float* alpha, const float* img, const double* loss_out,
                                 const float* g_loss, float* grad_rays_lt, int num_views, int num_rays, int height, int width,
                                 void* stream);
size_t rnr_masked_l1_loss_workspace_bytes(int num_views, int height, int width);
int rnr_masked_l1_loss(const float* est, const float* gt, const float* alpha, int border, double* loss_out, void* workspace,
                       int num_views, int channels, int height, int width, void* stream);
int rnr_masked_l1_loss_backward(const float* est, const float* gt, const float* alpha, int border, const float* g_loss,
                                float* grad_est, int num_views, int channels, int height, int width, void* stream);

/*
 * The stitched light probe (stitch_lp.py) and what train_rnr.py:288-295 does to it before use (csrc/stitch.hip): the scatter
 * direction of rnr_env_background's geometry.  Nothing syncs with the host, there are no float atomics, every sum has a fixed
 * order: two runs on the same inputs give the same bits.
 *
 * rnr_background_mask (in place of stitch_lp.py:135-140): alpha [N,H,W] float32, 0 <= radius <= 32 -> background [N,H,W] uint8,
 *   background = 1 iff no pixel with alpha > 0 lies within Chebyshev distance radius inside the image (a NaN alpha counts as
 *   not covered, as in rnr_present_u8): the complement of a (2 radius + 1)^2 dilation of the rasterizer's coverage.  One 32 x 32
 *   tile and its halo per workgroup in LDS, row maximum, then column maximum.  Floor: 5 N H W bytes (4 read, 1 written).
 *   UNPINNED against OpenCV: the reference fills the projected triangles with cv2.fillPoly on integer-truncated vertices,
 *   resizes to 512 x 512 bilinearly, dilates 17 x 17 and resizes back; cv2 is not available here.  The two masks differ in a thin
 *   band along the dilated silhouette.  radius = ceil(8 max(H, W) / 512) is that window at the image's own resolution.
 *
 * rnr_stitch_accumulate (stitch_lp.py:142-150): images [N,3,H,W] float32, or [N,H,W,3] with channels_last != 0;
 *   background [N,H,W] uint8 (non-zero = stitch this pixel); proj_inv, R_inv [N,3,3] FLOAT64 (K^-1 and R^-1 as the reference
 *   forms them); state sum [lp_h,lp_w,3] float64 and count [lp_h,lp_w] int32, zero before the first call;
 *   workspace: rnr_stitch_workspace_bytes(N, lp_h, lp_w) = 4 N lp_h lp_w bytes, 4-byte aligned, ALL ZERO before the first call;
 *   every call leaves it all zero again.  workspace_bytes is what the caller allocated: less than needed is an error.
 *   For every background pixel (x, y) of view n, in float64:
 *     d = normalize(R_inv[n] (proj_inv[n] (x + 0.5, y + 0.5, 1)))         = -view_dir of rnr_view_dir_map
 *     u = atan2(d.z, d.x) * 0.5 / pi + 0.5;   v = acos(d.y) / pi
 *     row = rint(min(v lp_h, lp_h - 1));   col = rint(min(u lp_w, lp_w - 1))          (half to even, as np.round)
 *   numpy's fancy-index `+=` does not accumulate over repeated indices, so per view a texel takes the value of the pixel with
 *   the HIGHEST row-major index that maps to it, sum[row, col] += (double)that pixel's three floats, count[row, col] += 1;
 *   views add up in view order, within a call and across successive calls, so any split of the views over calls gives the same
 *   bits.  Pass 1 (per pixel) finds the winners with an integer atomicMax of pixel index + 1 into workspace[n][texel]; pass 2
 *   (per texel) walks the call's views in order, adds, counts and clears the winners.  The products are not contracted to FMAs;
 *   a texel index agrees with the reference's wherever u lp_w and v lp_h are farther from a rounding tie than the float64
 *   error of atan2 / acos (~1e-16 lp_w).  A pixel whose direction is not finite (singular matrices) is skipped (the reference
 *   raises an index error there).  Limits: lp_h lp_w < 2^31 / 3, H W < 2^32 - 1.
 *
 * rnr_stitch_finalize (stitch_lp.py:152-153, 157): mask [lp_h,lp_w] uint8 = count > 0; lp [lp_h,lp_w,3] float32 =
 *   (float)(sum / count) where the mask is set and 0 elsewhere.  The state is not written: more views can follow.
 *
 * rnr_probe_prepare (train_rnr.py:288-295): lp [lp_h,lp_w,3] float32, mask [lp_h,lp_w] uint8 -> out [lp_h,lp_w,3] (may be lp):
 *     x = NaN -> 0;   x = (float)pow((double)x, gamma)  (one rounding; gamma == 1 leaves the bits alone);
 *     per channel, every texel with mask == 0 gets (float)(mean of x over the texels with mask != 0)
 *   The mean is a float64 sum in a fixed order (one partial record per workgroup, then one workgroup).  An empty mask gives NaN
 *   in every texel, as the reference's mean of nothing does; no error is raised (that would need a host sync).  A negative
 *   value under a fractional gamma is NaN as in numpy.  The reference swaps cv2's B,G,R to R,G,B first; here the channels keep
 *   the order of the images that were stitched.  workspace: rnr_probe_prepare_workspace_bytes(lp_h, lp_w) bytes, 8-byte
 *   aligned; every word that is read is written earlier in the same call.
 *
 * Errors (a NULL pointer, sizes <= 0, radius outside 0..32, a limit above, a workspace too small, misalignment) are reported
 * before any launch.
 */
#define RNR_BACKGROUND_MASK_MAX_RADIUS 32
int rnr_background_mask(const float* alpha, int radius, uint8_t* background, int num_views, int height, int width, void* stream);
size_t rnr_stitch_workspace_bytes(int num_views, int lp_h, int lp_w);
int rnr_stitch_accumulate(const float* images, int channels_last, const uint8_t* background, const double* proj_inv,
                          const double* R_inv, double* sum, int32_t* count, void* workspace, size_t workspace_bytes,
                          int num_views, int height, int width, int lp_h, int lp_w, void* stream);
int rnr_stitch_finalize(const double* sum, const int32_t* count, float* lp, uint8_t* mask, int lp_h, int lp_w, void* stream);
size_t rnr_probe_prepare_workspace_bytes(int lp_h, int lp_w);
int rnr_probe_prepare(const float* lp, const uint8_t* mask, double gamma, float* out, void* workspace, int lp_h, int lp_w,
                      void* stream);

/*
 * Adam step (csrc/optim.hip): torch.optim.Adam (train_rnr.py:376; no amsgrad, no maximize, L2 weight_decay in torch's default,
 * coupled form) for every tensor of a step in ONE launch, adam_multi_kernel, 256 threads per workgroup.  Workgroup b handles
 * chunk chunks[b]: elements [chunk * RNR_ADAM_CHUNK, min(n, (chunk + 1) * RNR_ADAM_CHUNK)) of tensors[chunks[b].tensor].  Per
 * element, in float32, every operation rounded once and none contracted, sqrt and / correctly rounded:
 *     g  = grad                      (+ wd * p            when wd != 0)
 *     m  = b1 * m + omb1 * g         (omb1 = float32(1 - b1), the subtraction made in double)
 *     v  = b2 * v + (omb2 * g) * g   (omb2 = float32(1 - b2))
 *     d  = sqrt(v) / bc2s + eps
 *     p  = p - step_size * (m / d)
 *   with step_size = float32(lr / (1 - b1^t)) and bc2s = float32(sqrt(1 - b2^t)) formed by the caller in double for the step
 *   count t the tensor has AFTER this step.  torch keeps t per parameter and lr, betas, eps, weight_decay per group, so b1 .. wd
 *   stand in the tensor's table entry, and (step_size, bc2s), which change every step, come from scalars[tensor.slot]: a HOST
 *   array of num_scalars <= RNR_ADAM_MAX_SLOTS entries that travels by value in the kernel arguments.  The call therefore
 *   neither synchronises nor copies on the stream; `tensors` and `chunks` are DEVICE arrays the caller builds once per
 *   parameter set and keeps alive until the launch has run.  Two calls on the same inputs give the same bits.
 *   p, g, m, v need 4-byte alignment only: a chunk whose four streams are 16-byte aligned moves float4s, any other chunk one
 *   element per thread (a parameter may be a view at an odd storage offset).  A tensor with n == 0 has no chunk; n < 2^31.
 * Mirrors: the new p is also stored through the tensor's num_mirrors <= 3 descriptors, each a strided scatter.  `shape` is the
 *   parameter as a 4-D array (leading dimensions 1); element (i0, i1, i2, i3) goes, when lo <= i_dim < hi, to
 *     dst[i0 stride[0] + i1 stride[1] + i2 stride[2] + i3 stride[3] + q repeat_stride]     for q = 0 .. repeat - 1
 *   Strides are in elements and may be negative; dst is the address index (0, 0, 0, 0) maps to, which lies outside the
 *   destination buffer when the range starts above 0 or a stride is negative.  These express what a U-Net training plan builds
 *   from its weights (rnr_conv_backward_desc): the identity copy of the forward staging, w[:, off:off+c].flip(2, 3).transpose(0, 1)
 *   of a 3x3 gradient convolution, the channel slices of the two 4x4 kinds, the padded BatchNorm / bias vectors and every row
 *   (repeat) of a consumer's shift.  A mirror with the parameter's own contiguous strides and its range on dimension 0 is stored
 *   as float4s where the chunk is.  The kernel cannot check a descriptor: the caller guarantees that every address it produces
 *   lies in a live buffer, and that no two descriptors of a launch write one address.
 * Errors (negative counts, num_scalars outside 1 .. RNR_ADAM_MAX_SLOTS, NULL tables with chunks to run) are reported before the
 * launch; num_chunks == 0 launches nothing.
 */
#define RNR_ADAM_CHUNK 4096
#define RNR_ADAM_MAX_SLOTS 64
#define RNR_ADAM_MAX_MIRRORS 3
typedef struct rnr_adam_mirror {
    float* dst;
    int64_t stride[4];
    int64_t repeat_stride;
    int dim, lo, hi, repeat;
} rnr_adam_mirror;
typedef struct rnr_adam_tensor {
    float* p;
    const float* g;
    float* m;
    float* v;
    int64_t n;
    float b1, omb1, b2, omb2, eps, wd;
    int slot, num_mirrors;
    int shape[4];
    int reserved[2];            /* 0 */
    rnr_adam_mirror mirror[RNR_ADAM_MAX_MIRRORS];
} rnr_adam_tensor;
typedef struct rnr_adam_chunk {
    int tensor, chunk;
} rnr_adam_chunk;
typedef struct rnr_adam_scalars {
    float step_size, bc2s;
} rnr_adam_scalars;
int rnr_adam_step(const rnr_adam_tensor* tensors, int num_tensors, const rnr_adam_chunk* chunks, int num_chunks,
                  const rnr_adam_scalars* scalars, int num_scalars, void* stream);

/* rnr_pack_conv_weight for descs[i], weights[i], packed[i], i = 0 .. count - 1, in that order on `stream`: the same kernels and
 * the same bytes, one call for a whole network (what follows rnr_adam_step in a training step).  Stops at the first error. */
int rnr_pack_conv_weights(const rnr_conv_desc* descs, const float* const* weights, float* const* packed, int count,
                          void* stream);

/* ---- spherical harmonics (sph_harm.py:41-102) ---- */

/* Alignment of the four SH operators' operands, rnr_interpolate_bilinear's and rnr_resize_area's: every operand its element's
 * 4 bytes. */
/* Real orthonormal SH without Condon-Shortley phase, columns (l, m=-l..l); dirs [n,3] (need not be unit),
 * out [n, (lmax+1)^2].  lmax <= 16. */
int rnr_sh_basis(const float* dirs, float* out, int n, int lmax, void* stream);
/* out[s, c] = sum_b basis[s,b] * coeff[b,c]  (sph_harm.reconstruct_sh, sph_harm.py:91-102) */
int rnr_sh_reconstruct(const float* basis, const float* coeff, float* out, int num_samples, int num_basis,
                       int num_channels, void* stream);
/* out[b, c] = 4pi/num_samples * sum_s samples[s,c] * basis[s,b]  (sph_harm.fit_sh_coeff, sph_harm.py:74-88) */
int rnr_sh_fit(const float* samples, const float* basis, float* out, int num_samples, int num_basis,
               int num_channels, void* stream);

/* Adjoint of rnr_sh_reconstruct in the coefficients: grad_coeff[b, c] = sum_s basis[s,b] * grad_out[s,c], grad_out [ns, nc]
 * the gradient of rnr_sh_reconstruct's out.  rnr_sh_fit's kernel without the 4pi/num_samples factor: one workgroup per
 * output and a fixed summation tree, so the result is deterministic.  grad_coeff [nb, nc] is overwritten. */
int rnr_sh_reconstruct_backward(const float* basis, const float* grad_out, float* grad_coeff, int num_samples,
                                int num_basis, int num_channels, void* stream);

/* misc.interpolate_bilinear (misc.py:5-42): data [H,W,C], x/y [n] -> out [n,C]; optional tap index output
 * taps [n,4] int32 = (x0,y0,x1,y1) fetch indices (bit-exact integer part of the sampler). */
int rnr_interpolate_bilinear(const float* data, int h, int w, int c, const float* x, const float* y,
                             float* out, int32_t* taps, int n, void* stream);

/* Area-average resize of a channel-last image src [src_h,src_w,C] -> dst [dst_h,dst_w,C]: the
 * cv2.resize(..., interpolation=cv2.INTER_AREA) call of LightingLP.__init__ (network.py:667) restated from OpenCV's
 * published algorithm (fractional-coverage box filter when shrinking on both axes, "area-mode" bilinear otherwise).
 * cv2 is not available in this image: parity with OpenCV is unpinned; the integer-ratio case is the plain box mean. */
int rnr_resize_area(const float* src, float* dst, int src_h, int src_w, int dst_h, int dst_w, int channels, void* stream);

/* A photograph for training: src [src_h,src_w,src_channels] interleaved 8-bit, src_channels 3 or 4 (the first three channels are
 * used in their order, a fourth is ignored) -> dst [3,dst_h,dst_w] planar float32, in one launch.  What
 * data_util.load_img(square_crop=True, downsampling_order=1) + [:, :, :3] + transpose(2,0,1) + ** img_gamma do on the host
 * (data_util.py:21-54, dataio.py:171-174):
 *   v   = (float)byte / 255.0f, correctly rounded (numpy's float32 quotient, bit for bit);
 *   r   = rnr_resize_area of v over the window rows [crop_y0, crop_y0 + crop_h), columns [crop_x0, crop_x0 + crop_w) to
 *         dst_h x dst_w: the same device function, so the bits are those of rnr_resize_area on the float window;
 *   out = gamma == 1 ? r : (float)pow((double)r, gamma): the float32 nearest to the float64 power (numpy's float32 ** lies up to
 *         10 ulp from it, so the reference's own bits are not reproducible).
 * Parity: as for rnr_resize_area, parity of the resize with OpenCV is unpinned (cv2 is not available in this image).  JPEG
 * decoders may differ by one level between two libjpeg builds; PNG and BMP decode exactly.
 * Alignment: src 1 byte (any address), dst its element's 4 bytes.
 * Refused before any launch: a NULL pointer, a size <= 0, src_channels other than 3 or 4, a window that is not inside the image,
 * a gamma that is not finite or not > 0, a misaligned dst. */
int rnr_photo_prepare(const uint8_t* src, int src_h, int src_w, int src_channels, int crop_y0, int crop_x0, int crop_h,
                      int crop_w, double gamma, float* dst, int dst_h, int dst_w, void* stream);

/* ---- OpenEXR photographs and probes (rnr_amd/exr.py reads and validates the file on the host) ---- */

/* Pixel types of an OpenEXR channel, with the file format's own codes. */
#define RNR_EXR_HALF 1
#define RNR_EXR_FLOAT 2
/* Bytes of a coded chunk that one pass of rnr_exr_unpack's workgroup covers: 256 lanes x 16 bytes of each half of the chunk.  A
 * longer chunk takes ceil(bytes / RNR_EXR_PASS_BYTES) passes of the same workgroup, the running sums carried in registers. */
#define RNR_EXR_PASS_BYTES 8192

/* The scanline chunks of an OpenEXR file -> its raw scanline buffer.  payload: the chunks' bytes one behind the other (a ZIP /
 * ZIPS chunk after inflate, any other as the file stores it); table [num_chunks, 4] int64 rows (src_offset into payload,
 * dst_offset into raw, bytes, coded); one workgroup per row:
 *   coded = 0   raw[dst_offset + i] = payload[src_offset + i], 0 <= i < bytes;
 *   coded = 1   with t = payload + src_offset and n = bytes, the format's two reconstruction steps:
 *                 predictor   t'[0] = t[0], t'[i] = (t'[i-1] + t[i] - 128) mod 256   (a prefix sum mod 256: any order, same bytes)
 *                 interleave  raw[dst_offset + 2k] = t'[k], raw[dst_offset + 2k + 1] = t'[(n + 1) / 2 + k].
 * CONTRACT: the table's CONTENTS are the host's responsibility.  The kernel trusts every row: [src_offset, src_offset + bytes)
 * must lie inside payload, [dst_offset, dst_offset + bytes) inside raw, the destination ranges must not overlap, bytes >= 0,
 * coded 0 or 1.  rnr_amd.exr checks all of this against the file before a byte is uploaded; a caller with a table of its own must
 * do the same.  payload is not modified; bytes of raw that no row covers are not written.
 * Alignment: payload and raw 1 byte (any address, and any offsets), table 8 bytes.
 * Refused before any launch: a NULL pointer, num_chunks <= 0, a misaligned table. */
int rnr_exr_unpack(const uint8_t* payload, const int64_t* table, int num_chunks, uint8_t* raw, void* stream);

/* The bound of rnr_amd.exr (MAX_RAW_BYTES) on the raw scanline buffer of one image, which rnr_exr_pack shares: 2^31 bytes. */
#define RNR_EXR_MAX_RAW_BYTES 2147483648
/* 16-bit units of a chunk (bytes of EACH half of the coded chunk) that one workgroup of rnr_exr_pack produces: 256 lanes x 16.
 * A longer chunk is ceil(bytes / 2 / RNR_EXR_PACK_SEGMENT) workgroups of one launch, never several passes of one. */
#define RNR_EXR_PACK_SEGMENT 4096

/* OpenEXR out: num_images float32 RGB images on the device -> the bytes the file format hands to deflate, in one
 * launch.  The inverse of rnr_exr_unpack for three channels of one type.
 * Source: value k in (r, g, b) of pixel (y, x) of image n is the float at
 *   src + n * image_stride + y * row_stride + x * x_stride + k_offset      (all in floats, all >= 0)
 * so [3,H,W], [H,W,3], [N,3,H,W], a crop of a larger image and channels 0..2 of an [H,W,4] buffer go in without a copy.
 * Destination: dst uint8 [num_images, height * row_bytes], row_bytes = 3 * width * size, size = 2 (RNR_EXR_HALF) or 4
 * (RNR_EXR_FLOAT).  With L = lines_per_chunk (1 for NONE / ZIPS, 16 for ZIP), chunk c of an image is the byte range
 * [c * L * row_bytes, min(height, (c + 1) * L) * row_bytes); its n bytes `raw` are, per scanline in increasing y, the run of B, then
 * of G, then of R values, little endian (the format's alphabetical channel order).
 *   coded = 0   dst holds raw: what a NONE file stores, and a ZIP / ZIPS file for a chunk that deflate does not shrink;
 *   coded = 1   per chunk, in integer arithmetic, the exact inverse of rnr_exr_unpack's two steps (n is even, row_bytes is):
 *                 split[k] = raw[2k], split[n / 2 + k] = raw[2k + 1];  coded[0] = split[0],
 *                 coded[i] = (split[i] - split[i-1] + 128) mod 256.
 * Float -> half (RNR_EXR_HALF) is done on the bit pattern, so the wave's denormal mode cannot change it: round to nearest, ties
 * to even; results below the half normal range are half subnormals (|x| <= 2^-25 gives +-0); magnitudes that round past 65504
 * (from 65520 on) give +-inf; +-0 and +-inf keep their sign; a NaN becomes sign | 0x7c00 | (mantissa >> 13), with the lowest bit
 * set when that field is 0 (OpenEXR's half(float) and numpy's software conversion: 0x7f800001 -> 0x7c01, 0xffc12000 -> 0xfe09).
 * RNR_EXR_FLOAT passes the 32 bits through untouched.
 * src is not modified; floats of src that no (n, y, x, k) addresses are not read; exactly num_images * height * row_bytes bytes
 * of dst are written.
 * Alignment: src its element's 4 bytes, dst 1 byte (any address: the kernel stores dwords where the address allows, single
 * bytes at the ragged ends).
 * Refused before any launch: a NULL pointer, a size <= 0, a negative stride or offset, a pixel_type other than the two above,
 * coded other than 0 / 1, lines_per_chunk <= 0, a misaligned src, height * row_bytes above RNR_EXR_MAX_RAW_BYTES, more than
 * 2^31 - 1 workgroups. */
int rnr_exr_pack(const float* src, int num_images, int height, int width, int64_t image_stride, int64_t row_stride,
                 int64_t x_stride, int64_t r_offset, int64_t g_offset, int64_t b_offset, int pixel_type, int lines_per_chunk,
                 int coded, uint8_t* dst, void* stream);

/* rnr_photo_prepare with a floating-point source and no / 255: src is a byte buffer of src_h rows of row_bytes bytes; the value
 * of channel k in (R, G, B) at (y, x) lives at src + y * row_bytes + k_offset + x * k_stride and has type k_type, RNR_EXR_HALF
 * (IEEE binary16, little endian) or RNR_EXR_FLOAT (binary32).  This covers OpenEXR's scanline-planar rows (offset: where the
 * channel's run starts in a scanline, stride: its element size) and interleaved float32 [H,W,C] (row_bytes 4 C W, offsets 0 / 4 /
 * 8, stride 4 C) alike.
 *   v   = the value as float32: binary16 -> binary32 is exact for all 65 536 patterns (subnormals, infinities; a NaN stays a NaN
 *         with its payload);
 *   r   = rnr_resize_area of v over the window, the same device function: the bits of rnr_resize_area on the float window;
 *   out = gamma == 1 ? r : (float)pow((double)r, gamma).
 * Negative and non-finite values pass through the arithmetic as IEEE has it (a negative r under gamma != 1 gives NaN).
 * Alignment: src 1 byte (with an odd width a HALF row starts at an odd multiple of 2 and a FLOAT run behind a HALF run at 2 mod 4;
 * the kernel loads 4, 2 or 1 bytes at a time as the address allows), dst its element's 4 bytes.
 * Refused before any launch: what rnr_photo_prepare refuses, row_bytes <= 0, a type other than the two above, a negative offset, a
 * stride below the type's size, and a channel row that does not fit: k_offset + (src_w - 1) * k_stride + size > row_bytes. */
int rnr_photo_prepare_hdr(const uint8_t* src, int src_h, int src_w, int64_t row_bytes, int64_t r_offset, int r_stride, int r_type,
                          int64_t g_offset, int g_stride, int g_type, int64_t b_offset, int b_stride, int b_type, int crop_y0,
                          int crop_x0, int crop_h, int crop_w, double gamma, float* dst, int dst_h, int dst_w, void* stream);

/* =====================================================================================================
 * 3. Stand-alone operators for the drop-in Python API (one reference function each).  The fused entry
 *    points above compute the same quantities without the intermediate HBM round trips.
 *    Alignment: every device operand of this section its element's 4 bytes (no kernel here moves more than one element at a
 *    time), the levels of textures_host / grad_textures_host included — except rnr_ray_transport's unet_raw and net_in (16, see
 *    there).  Sizes <= 0 and misaligned operands are refused before any launch.
 * ===================================================================================================== */

/* camera.get_view_dir_map (camera.py:5-32): out_world/out_cam [N,H,W,3] (out_cam may be NULL). */
int rnr_view_dir_map(const float* proj_inv, const float* R_inv, float* out_world, float* out_cam,
                     int num_views, int height, int width, void* stream);

/* test_rnr.py:386-391 for one probe: out[n,y,x,:] = bilinear(lp[lp_n == 1 ? 0 : n],
 *   min(u * lp_w, lp_w - 1), min(v * lp_h, lp_h - 1)),  (u, v) = spherical_mapping(-view_dir_world(n, y, x)).
 * proj_inv / R_inv [N,3,3]; lp [lp_n, lp_h, lp_w, 3], lp_n = 1 or N (lp_h, lp_w >= 1, a probe of fewer than 2^24 floats);
 * out [N,H,W,3] float32.  The directions are bit-identical to rnr_view_dir_map's out_world; the negation flips the sign bit
 * (-(+0) = -0 reaches atan2f, which decides the seam by it); atan2f / acosf in the reference's operation order
 * (render.py:96-102), taps and blend as rnr_interpolate_bilinear. */
int rnr_env_background(const float* proj_inv, const float* R_inv, const float* lp, int lp_n, int lp_h, int lp_w,
                       float* out, int num_views, int height, int width, void* stream);

/* render.get_TBN_map (render.py:152-166) given per-face unit tangents: out [N,H,W,3,3], columns (T,B,N). */
int rnr_tbn_map(const float* normal_map, const int32_t* face_index_map, const float* face_tangents,
                int num_faces, float* out, int num_views, int height, int width, void* stream);

/* The per-pixel 3x3 products of the reference's view loop, test_rnr.py:314:
 *   torch.matmul(TBN_map.reshape((-1, 3, 3)).transpose(-2, -1), view_dir_map.reshape((-1, 3, 1)))
 * tbn [P,3,3] (row-major records, as rnr_tbn_map writes them), vec [P,3], out [P,3];  out[p] = tbn[p]^T vec[p] when transposed != 0,
 * tbn[p] vec[p] otherwise.  ((c z + (b y + a x)) with fused multiply-adds: <= 1 ulp per term from the batched-GEMM result.)
 * The drop-in render.get_TBN_map returns a tensor that answers exactly this torch.matmul call with this entry point. */
int rnr_tbn_matvec(const float* tbn, const float* vec, float* out, long num_pixels, int transposed, void* stream);

/* network.RaySampler.forward (network.py:445-472).  reflect != 0: mode 'reflect' (needs view_tangent), else the
 * pivots themselves.  pivots_host [3,R] (HOST).  tbn [P,3,3], view_tangent [P,3], alpha [P];
 * rays_dir [P,3,R], rays_uv [P,2,R], rays_dir_tangent [P,3,R] (reflect mode only; may be NULL). */
int rnr_ray_sampler(int reflect, const float* pivots_host, int num_rays, const float* tbn,
                    const float* view_tangent, const float* alpha, float* rays_dir, float* rays_uv,
                    float* rays_dir_tangent, long num_pixels, void* stream);

/* network.TextureMapper.forward (network.py:67-91) for any channel count: uv_map [N,H,W,2],
 * sh_basis_map [N,H,W,9] or NULL, textures[level] [S_l,S_l,C] -> out [N,C,H,W].  Refuses what its adjoint refuses: sizes <= 0,
 * more than 8 levels, sh_start_ch + 9 > tex_channels with an SH map. */
int rnr_texture_mapper(const float* uv_map, const float* sh_basis_map, const float* const* textures_host,
                       const int* tex_sizes_host, int num_levels, int tex_channels, int sh_start_ch,
                       float* out, int num_views, int height, int width, void* stream);

/*
 * Adjoint of rnr_texture_mapper in the textures: the path from an image loss to the neural texture (TextureMapper.textures,
 * train_rnr.py:376).  The operator is linear in them, so no texture value is needed.  No gradient for uv_map or sh_basis_map: in
 * the reference they come from the data loader and carry none.
 *   forward operands   uv_map [N,H,W,2], sh_basis_map [N,H,W,9] or NULL, tex_sizes_host, num_levels, tex_channels, sh_start_ch
 *                      exactly as given to rnr_texture_mapper (a level may also be 1 x 1 here);
 *   upstream gradient  grad_out [N,C,H,W];
 *   outputs            grad_textures_host: HOST array of num_levels device pointers, level l [S_l,S_l,C].
 * With f_c(n,p) = sh_basis_map[n,p,c - sh_start_ch] on the nine SH channels (when the map is given) and 1 elsewhere, every
 * bilinear tap (y, x) of weight w of pixel (n,p) on level l adds
 *   (grad_out[n,c,p] * f_c(n,p)) * w      (in that product order)
 * to grad_textures[l][y, x, c].  Taps and weights are those of the forward (same code, same bits): the clamped indices, so no
 * address leaves a level whatever uv_map holds.  uv_map must be finite: as the forward yields NaN for a NaN uv (NaN weights on
 * texel (0, 0)), the adjoint adds NaN there.  A contribution whose weight or whose grad_out * f is 0 is never added:
 * out-of-range uv, background pixels under a masked loss, -0.
 * Every level is OVERWRITTEN: it is cleared on `stream` first and texels that nothing reaches end at exactly 0.  The sums are
 * made with float atomic adds (in LDS per workgroup, then global), whose order of arrival is not fixed: the gradients may
 * differ in the last bits from run to run.  For a texel and channel that receives n contributions the deviation from the
 * exact sum stays within (n + 6) 2^-24 times the sum of their magnitudes (tests/test_gpu_texture_backward.py).
 * Two kernel forms: images of 16 x 16 pixels or more -> a workgroup per 16 x 16-pixel tile that accumulates each level's
 * texel footprint in LDS and flushes it with one global add per entry; otherwise one lane per (pixel, channel) and one
 * global add per tap.  1 <= num_levels <= 8; sh_start_ch + 9 <= tex_channels when sh_basis_map is given.
 */
int rnr_texture_mapper_backward(const float* uv_map, const float* sh_basis_map, const float* grad_out,
                                float* const* grad_textures_host, const int* tex_sizes_host, int num_levels,
                                int tex_channels, int sh_start_ch, int num_views, int height, int width, void* stream);

/* network.RayRenderer.forward (network.py:481-527) on API-shaped tensors: rays_uv [N,H,W,2,R],
 * rays_lt [N,R,C,H,W], lp [lp_n,Hl,Wl,C] (lp_n = 1 or N), albedos [N,C,H,W] (albedo_diffuse may be NULL).
 * Outputs [N,C,H,W] (out required, others optional) and rays_color [N,R,C,H,W] (optional).  Refuses what its adjoint refuses:
 * sizes <= 0, num_rays <= num_ray_diffuse, a probe batch of 2^31 floats or more.
 * A NaN in rays_uv PROPAGATES, as through torch.clamp(max=) and the reference's blend: the tap coordinate min(u Wl, Wl - 1) is the
 * NaN-propagating minimum, the indices clamp to column / row 0 and the four weights are NaN, so that ray's colour and what sums
 * it are NaN (rnr_ray_render, rnr_ray_weights and rnr_env_background share the code; tests/test_gpu_shade_guard.py). */
int rnr_ray_renderer(const float* rays_uv, const float* rays_lt, const float* lp, int lp_n, int lp_h,
                     int lp_w, const float* albedo_specular, const float* albedo_diffuse, int channels,
                     int num_rays, int num_ray_diffuse, int no_albedo, int seperate_albedo,
                     float lp_scale_factor, float* out, float* out_specular, float* out_diffuse,
                     float* ltt_specular, float* ltt_diffuse, float* rays_color, int num_views, int height,
                     int width, void* stream);

/*
 * Adjoint of rnr_ray_renderer on the same API-shaped tensors: the path from the image loss to the light probe (and through
 * rnr_sh_reconstruct_backward to LightingSH.coeff, train_rnr.py:376), to rays_lt and to the albedos.  The operator is linear in
 * each of them.  No gradient for rays_uv: in the reference it comes from the rasterizer and carries none.
 *   forward operands   rays_uv, rays_lt, lp, the albedos, the flags and lp_scale_factor exactly as given to rnr_ray_renderer;
 *   upstream gradients g_out, g_out_specular, g_out_diffuse, g_ltt_specular, g_ltt_diffuse [N,C,H,W] and g_rays_color
 *                      [N,R,C,H,W]; each may be NULL, meaning zero;
 *   outputs            grad_rays_lt [N,R,C,H,W], grad_albedo_specular, grad_albedo_diffuse [N,C,H,W], grad_lp [lp_n,Hl,Wl,C];
 *                      each may be NULL: not wanted, its work is skipped (grad_albedo_diffuse needs albedo_diffuse).
 * With ns = R - num_ray_diffuse and a_s, a_d the albedo each group is multiplied by (1 with no_albedo):
 *   G_os = g_out + g_out_specular,  G_od = g_out + g_out_diffuse,  G_ls = g_ltt_specular + G_os a_s,  G_ld = g_ltt_diffuse + G_od a_d;
 *   per ray r: G_p = G_ls / ns (specular) or G_ld / num_ray_diffuse (diffuse);  grad_rays_lt[r] = G_p colour_r (the forward's
 *   rays_color, recomputed);  G_col = g_rays_color[r] + G_p rays_lt[r];  each of the ray's four env-map taps adds
 *   G_col * w_tap * lp_scale_factor to grad_lp at its texel;
 *   grad_albedo_* = G_o* ltt_* (0 with no_albedo), both groups summed onto the specular albedo when the diffuse group uses it
 *   (seperate_albedo == 0 or albedo_diffuse == NULL: grad_albedo_diffuse is then 0).  With num_ray_diffuse == 0 the diffuse
 *   outputs are constants: g_out_diffuse and g_ltt_diffuse are ignored.
 * Taps and weights are those of the forward (same code): the clamped indices, so no address leaves the probe whatever
 * rays_uv holds, NaN included.  A contribution whose tap weight is 0 is never added: every ray of a background pixel
 * (uv = -1) and every out-of-range coordinate.
 * grad_lp is OVERWRITTEN: it is cleared on `stream` first, texels that no valid tap touches end at exactly 0, and with
 * lp_n == 1 it is the sum over the views.  The sum is made with global float atomic adds, whose order of arrival is not
 * fixed: grad_lp may differ in the last bits from run to run (the other outputs are deterministic).  For a texel that
 * receives n contributions the deviation from the exact sum stays within about (n + 16) 2^-24 times the sum of their
 * magnitudes (tests/test_gpu_ray_backward.py).
 * Two kernel forms, chosen as in rnr_ray_renderer: channels <= 4 and num_rays <= 64 -> 64 pixels per workgroup with the uv
 * rows through LDS; otherwise one lane per (pixel, channel).  lp_n * Hl * Wl * C < 2^31.
 */
int rnr_ray_renderer_backward(const float* rays_uv, const float* rays_lt, const float* lp, int lp_n, int lp_h,
                              int lp_w, const float* albedo_specular, const float* albedo_diffuse, int channels,
                              int num_rays, int num_ray_diffuse, int no_albedo, int seperate_albedo,
                              float lp_scale_factor, const float* g_out, const float* g_out_specular,
                              const float* g_out_diffuse, const float* g_ltt_specular, const float* g_ltt_diffuse,
                              const float* g_rays_color, float* grad_rays_lt, float* grad_albedo_specular,
                              float* grad_albedo_diffuse, float* grad_lp, int num_views, int height, int width,
                              void* stream);

/*
 * The lighting-independent state of the fused ray stage (rnr_ray_render) unpacked into RayRenderer.forward's per-view tensors.
 * Inputs as rnr_ray_render takes them (no probe).  Outputs:
 *   rays_uv [N,H,W,2,R]   equirect uv of every ray, computed with rnr_ray_render's own arithmetic from the directions stored
 *                         in net_in: the env-map taps of these uv are the fused frame's taps;
 *   rays_lt [N,R,3,H,W]   tanh(raw + bias) + 1 with rnr_ray_render's tanh (absolute error ~1e-7);
 *   albedo_specular, albedo_diffuse [N,3,H,W]   copies of net_in's albedo channels.
 * Background pixels (alpha == 0) get uv = -1 and rays_lt = 0 by select, not multiply: unet_raw may hold non-finite values
 * there (rnr_conv2d_masked skips background tiles).  Then, for any probe lp,
 *   rnr_ray_renderer(rays_uv, rays_lt, lp, albedo_specular, albedo_diffuse, seperate_albedo = 1).out
 * is rnr_ray_render's frame up to the order of the sums over the rays, and rnr_ray_renderer_backward is its adjoint.
 * At most 16 specular and 16 diffuse rays; c_out_pad and c_pad multiples of 4.
 * Alignment: unet_raw and net_in are read in 16-byte pieces (whole rows, as by rnr_ray_render) and need 16-byte alignment; bias,
 * alpha and the four outputs their element's 4 bytes.
 */
int rnr_ray_transport(const float* unet_raw, int c_out_pad, const float* bias, const float* net_in, int c_pad,
                      const float* alpha, int num_spec, int num_diff, int albedo_diff_ch, int albedo_spec_ch,
                      float* rays_uv, float* rays_lt, float* albedo_specular, float* albedo_diffuse,
                      int num_views, int height, int width, void* stream);

/* =====================================================================================================
 * 4. Host-side data front-end: Wavefront OBJ reader behind nr.load_obj(normalization=False, load_texture=False)
 *    (neural_renderer/load_obj.py:108-209: four Python passes over the lines).  No GPU involved.
 *    Two calls: rnr_obj_scan counts the elements, the caller allocates, rnr_obj_parse fills:
 *    v [nv,3], vn [nvn,3], vt [nvt,2] float32 (correctly rounded double -> float32, like float() + astype(float32));
 *    f_v_idx / f_vt_idx / f_vn_idx [nf,3] int32, 0-based.  vt / vn index arrays are filled iff the file holds vt / vn
 *    lines (the reference's has_vt / has_vn, load_obj.py:133-176).  Triangles only; errors via rnr_last_error.
 * ===================================================================================================== */
typedef struct rnr_obj_counts {
    long num_vertices, num_normals, num_texcoords, num_faces;
} rnr_obj_counts;
int rnr_obj_scan(const char* text, size_t len, rnr_obj_counts* counts);
int rnr_obj_parse(const char* text, size_t len, const rnr_obj_counts* counts, float* v, float* vn, float* vt,
                  int32_t* f_v_idx, int32_t* f_vt_idx, int32_t* f_vn_idx);

/* =====================================================================================================
 * 5. Measurement aid (bench.py's `box_calibration`; no counterpart in the reference).
 *    rnr_calibrate_mfma_f32 runs `iters` x 32 register-resident v_mfma_f32_32x32x2_f32 per wave on every SIMD of the
 *    current device (`waves_per_simd` = 1 ... 8 waves per SIMD, full-mantissa operands, no memory traffic), times the launch with HIP events
 *    on `stream`, waits for it, and returns the rate in *tflops (and the duration in *seconds, if not NULL): what this
 *    device sustains NOW on the instruction the U-Net runs on (nominal 157.3 TFLOP/s).  scratch: >= 4 bytes of device
 *    memory (never written in practice).  Blocks the calling thread.
 * ===================================================================================================== */
int rnr_calibrate_mfma_f32(int iters, int waves_per_simd, float* scratch, double* tflops, double* seconds, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RNR_HIP_H */
