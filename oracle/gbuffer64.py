"""ORACLE (test infrastructure, not product): float64 evaluation of network.Rasterizer.forward's attribute interpolation
(network.py:176-214, as rnr_oracle.rasterizer_forward restates it), for tests that compare the fused G-buffer of
raster.hip (raster_tile_kernel<1>) with a high-precision reference at meshes, sizes and batches the fixtures do not cover.

In the same two parts the kernel has:
  * everything that is an integer or a raw rasterizer output comes from the float32 C oracle (oracle/raster.py), which the
    kernel matches bit for bit: face_index_map, alpha, depth, the raw barycentric weights, the vertical flip, and the
    projected vertex z the weights are divided by.  rasterize_rgbad supplies them exactly as rasterizer_forward uses them.
  * everything after that is float64: the perspective-corrected weights (1/z) * w * depth, the uv / normal / position
    interpolation, the uv wrap u - floor(u), F.normalize (x / max(|x|, 1e-12), with the clamp float32 rounds 1e-12 to, as
    torch applies it to the float32 maps), the camera-space maps R n and R p + t.
Background pixels (face index -1) take the last face, as torch indexing does in the reference (network.py:176-214); their
weights are 0 unless that face has a vertex at z = 0, where 1/z = inf and the reference's own weights are 0 * inf = NaN.

Inputs are torch CPU tensors: mesh dict v [nv,3], vt [nvt,2], vn [nvn,3], f_v_idx / f_vt_idx / f_vn_idx [nf,3]; v_uvz
[N,nv,3] float32 projected vertices (NDC x, y and camera z, as the kernel receives them); pose [N,4,4].
test_oracle_golden.py::test_gbuffer64_* pins this module against rnr_oracle (float32) and the reference-generated fixture.
"""
import numpy as np
import torch

from . import rnr_oracle as orc

D = torch.float64
NORMALIZE_EPS = float(np.float32(1e-12))     # F.normalize's eps as a float32 clamp_min applies it


def normalize(x, dim=-1):
    """F.normalize of a float32 map, in float64: x / max(||x||, fl32(1e-12))."""
    x = x.to(D)
    return x / x.norm(dim=dim, keepdim=True).clamp(min=NORMALIZE_EPS)


def rasterizer_forward(mesh, v_uvz, pose, img_size, near=0.0, far=1e5):
    """Returns a dict of the G-buffer maps by the names of ops.GBUFFER_MAPS (flipped rows, as the kernel writes them):
    face_index_map [N,S,S] int32, alpha, depth [N,S,S] and raw_weight_map [N,S,S,3] float32 (the C oracle's bits),
    weight_map32 [N,S,S,3] float32 (((1/z) * w) * depth as rasterizer_forward evaluates it), and float64 weight_map,
    uv_map [N,S,S,2], normal_map, normal_map_cam, position_map, position_map_cam [N,S,S,3].
    Also the per-pixel magnitudes the error bounds of a float32 evaluation scale with (float64):
      uv_abs [N,S,S,2] = sum_k |vt_k w_k|, normal_raw [N,S,S,3] = sum_k vn_k w_k (before normalisation),
      normal_abs [N,S,S,3] = sum_k |vn_k w_k|, position_abs [N,S,S,3] = sum_k |v_k w_k|."""
    S = int(img_size)
    v_uvz = v_uvz.to(torch.float32)
    N = v_uvz.shape[0]
    faces_v_uvz = orc.gather_faces(v_uvz, mesh['f_v_idx'][None])                 # [N,nf,3,3] float32
    ras = orc.rasterize_rgbad(faces_v_uvz, S, near, far)
    fim, depth, raw = ras['face_index_map'], ras['depth'], ras['weight_map']
    fl = fim.long()
    z = torch.stack([faces_v_uvz[i, fl[i]][..., 2] for i in range(N)])           # [N,S,S,3] float32
    w32 = ((1 / z) * raw) * depth[..., None]                                     # network.py:176-180, float32
    w = (1.0 / z.to(D)) * raw.to(D) * depth.to(D)[..., None]                     # [N,S,S,3] float64

    def interp(attr, idx):
        per_face = attr.to(D)[idx.long()]                                        # [nf,3,A]
        g = per_face[fl]                                                         # [N,S,S,3,A]; -1 wraps to the last face
        return (g * w[..., None]).sum(-2), (g.abs() * w.abs()[..., None]).sum(-2)

    uv, uv_abs = interp(mesh['vt'], mesh['f_vt_idx'])
    n, n_abs = interp(mesh['vn'], mesh['f_vn_idx'])
    p, p_abs = interp(mesh['v'], mesh['f_v_idx'])
    R = pose[:, :3, :3].to(D)
    t = pose[:, :3, 3].to(D)
    nu = normalize(n)
    return {
        'face_index_map': fim, 'alpha': ras['alpha'], 'depth': depth, 'raw_weight_map': raw, 'weight_map32': w32,
        'weight_map': w,
        'uv_map': uv - uv.floor(),
        'normal_map': nu,
        'normal_map_cam': normalize(torch.einsum('nij,nhwj->nhwi', R, nu)),
        'position_map': p,
        'position_map_cam': torch.einsum('nij,nhwj->nhwi', R, p) + t[:, None, None, :],
        'uv_abs': uv_abs, 'normal_raw': n, 'normal_abs': n_abs, 'position_abs': p_abs,
    }
